"""The claims of tests/match_cases.py, held against the oracle's streams on the CPU -- every case is in the catalogue for which
side of a rule's edge it is on, and this file is where that is checked -- and every case through the CPU model
(tests/model/zs_model.cpp: the kernels' own ZS_HD code) in the modes the device has for its level.  The device is not involved;
tests/test_gpu_match_cases.py asks it for these bytes."""
import collections
import os
import subprocess
import zlib

import pytest

import deflate_reader as dr
import match_cases as mc
from test_model import batch, model, run  # noqa: F401  (model: the fixture that builds build/zs_model)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_STREAMS = {}


def ref(oracle, name, level=None, strategy=None, hash_variant=0):
    """The oracle's stream of a case, by default at the case's own level and strategy, made once."""
    _, data, lvl, strat, writes, _ = mc.hash_variant_case(name) if hash_variant else mc.case(name)
    key = (name, lvl if level is None else level, strat if strategy is None else strategy, hash_variant)
    if key not in _STREAMS:
        _STREAMS[key] = oracle.compress(data, key[1], key[2], chunks=writes, hash_variant=hash_variant)
    return _STREAMS[key]


def test_names_counts_and_both_sides_of_every_edge():
    names = mc.case_names()
    assert len(set(names)) == len(names) == sum(mc.FAMILY_COUNTS.values()) == 444
    assert dict(collections.Counter(mc.META[n][0] for n in names)) == mc.FAMILY_COUNTS
    sides = collections.defaultdict(set)
    for n in names:
        family, edge, side = mc.META[n]
        sides[(family, edge)].add(side)
    # (a placement has no far side: it is the generic match moved over the device's grids)
    lost = sorted(k for k, v in sides.items() if v != {"in", "out"} and k[0] != "placement")
    assert not lost, lost
    assert {e for f, e in sides if f == "budget"} >= {"chain_L%d" % lv for lv in range(1, 10)} | {"quarter_L%d" % lv for lv in range(5, 10)}
    assert max(len(mc.case(n)[1]) for n in names) == 131072  # every stream under 140 KiB
    assert set(mc.NOT_UNDER_HASH_VARIANT_1) <= set(names) and len(mc.hash_variant_names()) == 19 + 43 - len(mc.NOT_UNDER_HASH_VARIANT_1)


@pytest.mark.parametrize("family", sorted(mc.FAMILY_COUNTS))
def test_claims_hold_on_the_oracles_streams(oracle, family):
    bad = []
    for name in mc.case_names(family):
        _, data, level, strategy, writes, claim = mc.case(name)
        assert writes is None or sum(writes) == len(data)
        z = ref(oracle, name)
        blocks = dr.read(z)
        assert zlib.decompress(z) == data and dr.replay(blocks) == data, name
        assert not any(b.kind == "stored" for b in blocks), name  # the tokens are visible
        if not claim(mc.tokens(blocks)):
            bad.append(name)
    assert not bad, bad


def test_claims_of_the_distance_and_budget_families_under_the_multiplicative_hash(oracle):
    bad = []
    for name in mc.hash_variant_names():
        _, data, level, strategy, writes, claim = mc.hash_variant_case(name)
        blocks = dr.read(ref(oracle, name, hash_variant=1))
        if dr.replay(blocks) != data or not claim(mc.tokens(blocks), 1):
            bad.append(name)
    assert not bad, bad


def test_triples_are_the_token_tools_view(oracle):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import deflate_tokens
    for name in ("quarter_L6_pend8_front31", "insert_L3_match6", "run_twice_p7_L6"):
        z = ref(oracle, name)
        assert mc.triples(dr.read(z)) == deflate_tokens.tokens(z)[0]


FAST_MODES = (("seq", {}), ("fvec", {}), ("fsweep", {}), ("fsweep", {"ZS_FS_W": "64", "ZS_FS_TILE": "256"}), ("frounds", {"ZS_FR_CHUNK": "1024"}),
              ("frounds", {"ZS_FR_CHUNK": "2048"}))


@pytest.mark.parametrize("family", sorted(mc.FAMILY_COUNTS))
def test_cases_through_the_cpu_model(model, tmp_path, family):
    """Levels 4-9 in the chunked form; levels 1-3 through the literal engine, the lanes of a wave, the sweeps (at the kernel's window
    and at a small one) and the rounds over chunks of 1024 and 2048 positions; a Write list as the model's wchunk.  The model
    compares symbols, blocks and bytes with the oracle itself."""
    with batch():
        for name in mc.case_names(family):
            _, data, level, strategy, writes, _ = mc.case(name)
            path = tmp_path / name
            path.write_bytes(data)
            wchunk = ",".join(map(str, writes)) if writes else None
            if level >= 4:
                run(str(path), level, strategy, "chunk", wchunk)
                continue
            for mode, env in FAST_MODES:
                if writes and mode == "fvec":
                    continue  # (the lanes of a wave take one Write)
                run(str(path), level, strategy, mode, wchunk, env=env or None)


ADLER_SEEDS = (1, 0, 0xFFF0FFF0, 65520 | 65520 << 16)
ADLER_LENGTHS = (0, 1, 255, 256, 257, 4095, 65535, 65536, 65537, 256 * 65536 + 1)


def test_adler_combine_against_zlib():
    """adler_combine (zs_core.h) is what seeds zs_adler32_device's result and what the trailer kernel folds a stream's 64 KiB
    pieces with: all-0xFF buffers (the largest sums), the seeds and lengths of the device test, the second part's Adler-32 from
    seed 1 as the kernels compute it."""
    exe = os.path.join(ROOT, "build", "test_adler_combine")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_adler_combine.cpp")], check=True)
    ff = b"\xff" * (ADLER_LENGTHS[-1] + 65537)
    rows, want = [], []
    for n in ADLER_LENGTHS:
        part = zlib.adler32(ff[:n])
        for seed in ADLER_SEEDS:
            rows.append("%d %d %d" % (seed, part, n))
            want.append(zlib.adler32(ff[:n], seed))
        for m in (1, 65536, 65537):  # two all-0xFF parts
            rows.append("%d %d %d" % (zlib.adler32(ff[:m]), part, n))
            want.append(zlib.adler32(ff[:m + n]))
    r = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, check=True)
    assert [int(x) for x in r.stdout.split()] == want
