"""The claims of tests/rle_cases.py, held against the oracle's streams on the CPU -- every case is in the catalogue for which side
of a rule's edge it is on, and this file is where that is checked --, the catalogue's reference parse against the oracle's tokens,
and every case through the CPU model in mode "rle" (tests/model/zs_model.cpp: the kernels' own ZS_HD code of zs_rle.h and the
literal engine behind the hand-over).  The `handover` and `block_cut` families run once more through the model built with the
address and undefined-behaviour sanitizers, a program of its own: that is what holds run_tail's room for the longest tail.  The
device is not involved; tests/test_gpu_rle_cases.py asks it for these bytes."""
import collections
import os
import subprocess
import zlib

import pytest

import deflate_reader as dr
import match_cases as mc
import rle_cases as rc
from test_model import batch, model, run  # noqa: F401  (model: the fixture that builds build/zs_model)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN_EXE = os.path.join(ROOT, "build", "zs_model_asan")
_STREAMS = {}
_VIEWS = {}


def ref(oracle, name, level=None):
    """The oracle's stream of a case as one Write, by default at the case's own level, made once."""
    _, data, lvl, _, _ = rc.case(name)
    key = (name, lvl if level is None else level)
    if key not in _STREAMS:
        _STREAMS[key] = oracle.compress(data, key[1], rc.RLE)
    return _STREAMS[key]


def view(oracle, name):
    """(tokens, blocks, slides) of the oracle's stream of a case, made once"""
    if name not in _VIEWS:
        _, data, level, _, _ = rc.case(name)
        z, _, slides = oracle.trace(data, level, rc.RLE, None)
        assert z == ref(oracle, name) and zlib.decompress(z) == data, name
        blocks = dr.read(z)
        _VIEWS[name] = (mc.tokens(blocks), blocks, slides)
    return _VIEWS[name]


def test_names_counts_and_both_sides_of_every_edge():
    names = rc.case_names()
    assert len(set(names)) == len(names) == sum(rc.FAMILY_COUNTS.values()) == 286
    assert dict(collections.Counter(rc.META[n][0] for n in names)) == rc.FAMILY_COUNTS
    sides = collections.defaultdict(set)
    for n in names:
        family, edge, side = rc.META[n]
        sides[(family, edge)].add(side)
    # (a placement has no far side: it is a slot shape moved over the device's grids)
    lost = sorted(k for k, v in sides.items() if v != {"in", "out"} and k[0] != "placement")
    assert not lost, lost
    assert {e for f, e in sides if f == "handover"} == {"shortest_body", "trigger_1", "trigger_2", "trigger_3", "tile_behind"}
    # every stream under 140 KiB but the two stored ones (300 000 bytes) and the pieces (4.2 to 9 MiB)
    sizes = {n: len(rc.case(n)[1]) for n in names}
    assert max(v for n, v in sizes.items() if rc.META[n][0] not in ("pieces", "stored")) == rc.trigger(3) + 258 + 786 < 140 << 10
    assert all((4 << 20) < sizes[n] < (9 << 20) for n in rc.case_names("pieces"))
    assert all(rc.case(n)[3] is None and rc.case(n)[2] == 6 for n in names)
    # the measure family: every length at all eight residues, the slot start's position of that residue
    at = collections.defaultdict(set)
    for n in rc.case_names("measure"):
        p, r = rc.slot_start(n)
        assert p % 8 == r and p < rc.body_end(sizes[n])
        at[rc.AT[n][0]].add(r)
    assert sorted(at) == list(rc.MEASURE_LEFT) and all(v == set(range(8)) for v in at.values())


def test_the_hand_over_position_is_zs_rle_hs():
    """rle_body_end itself (zs_rle.h, compiled for the host) and the catalogue's restatement of it, at the sizes the catalogue is
    built on: n - 786 = t - 1 and t + 258 are not moved, t and t + 257 move to t - 259 -- a trigger exactly 258 below H has fired
    at the loop-top before H at the latest -- and k_done counts the triggers at or below H."""
    exe = os.path.join(ROOT, "build", "test_rle_body_end")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_rle_body_end.cpp")], check=True)
    want = {4881: (-1, 0), 4882: (4096, 0), 8192 + 785: (8191, 0), 16383 + 786: (16383, 0), 2 * 16383 + 786: (32766, 0)}
    for k in (1, 2, 3):
        t = rc.trigger(k)
        for d, h, fired in ((-1, t - 1, k - 1), (0, t - 259, k - 1), (257, t - 259, k - 1), (258, t + 258, k)):
            want[t + d + 786] = (h, fired)
    sizes = sorted(set(want) | {len(rc.case(n)[1]) for n in rc.case_names()})
    r = subprocess.run([exe], input="".join("%d 1000\n" % n for n in sizes), capture_output=True, text=True, check=True)
    got = dict(zip(sizes, (tuple(map(int, line.split())) for line in r.stdout.splitlines())))
    assert len(got) == len(sizes) and {n: got[n] for n in want} == want
    assert all(got[n][0] == rc.body_end(n) for n in sizes)


@pytest.mark.parametrize("family", sorted(rc.FAMILY_COUNTS))
def test_claims_hold_on_the_oracles_streams(oracle, family):
    bad = []
    for name in rc.case_names(family):
        t, blocks, slides = view(oracle, name)
        assert dr.replay(blocks) == rc.case(name)[1], name
        if not rc.case(name)[4](t, blocks, slides):
            bad.append(name)
    assert not bad, bad


@pytest.mark.parametrize("family", sorted(rc.FAMILY_COUNTS))
def test_reference_parse_is_the_oracles(oracle, family):
    """parse() against the oracle's tokens, whole streams; a stream with a stored block shows no tokens there (the `stored`
    family and the block cuts in front of a stored block, and no other)"""
    bad = []
    for name in rc.case_names(family):
        t, blocks, _ = view(oracle, name)
        if any(b.kind == "stored" for b in blocks):
            assert family == "stored" or rc.META[name][1] == "cut_symbol_stored", name
        elif rc.parse(rc.case(name)[1]) != t:
            bad.append(name)
    assert not bad, bad


def test_the_stored_cases_begin_and_end_stored(oracle):
    """(where blocks are stored the parse is held through the model alone, test_cases_through_the_cpu_model)"""
    for name in rc.case_names("stored"):
        _, blocks, _ = view(oracle, name)
        assert blocks[0].kind == "stored" and blocks[-1].kind == "stored" and blocks[-1].final


@pytest.mark.parametrize("family", sorted(rc.FAMILY_COUNTS))
def test_cases_through_the_cpu_model(model, tmp_path, family):
    """Mode "rle" at levels 1, 6 and 9: the runs' closed form below the hand-over position, the literal engine behind it.  The
    model compares symbols, blocks, read events and bytes with the oracle itself."""
    with batch():
        for name in rc.case_names(family):
            path = tmp_path / name
            path.write_bytes(rc.case(name)[1])
            for level in (1, 6, 9):
                run(str(path), level, rc.RLE, "rle")


@pytest.fixture(scope="module")
def model_asan():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", ASAN_EXE,
                    os.path.join(ROOT, "tests/model/zs_model.cpp"), os.path.join(ROOT, "oracle/zs_oracle.c"), os.path.join(ROOT, "oracle/zs_inflate_oracle.c")],
                   check=True)
    return ASAN_EXE


@pytest.mark.parametrize("family", ["block_cut", "handover"])
def test_cases_through_the_model_under_the_sanitizers(model_asan, tmp_path, family):
    """The model as a stand-alone program built with -fsanitize=address,undefined -fno-sanitize-recover=all, level 6: a tail of up
    to 1302 symbols behind the hand-over (zs_rle.h kRleTailMax) has its room, and nothing else in the model or in the code it
    shares with the kernels reads or writes out of bounds on these inputs."""
    from concurrent.futures import ThreadPoolExecutor

    def one(name):
        path = tmp_path / name
        path.write_bytes(rc.case(name)[1])
        r = subprocess.run([model_asan, str(path), "6", str(rc.RLE), "rle", "0", "0"], capture_output=True, text=True)
        return None if r.returncode == 0 and "PASS" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr else \
            (name, r.returncode, r.stdout[-300:], r.stderr[-1500:])
    with ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0))))) as pool:
        bad = [b for b in pool.map(one, rc.case_names(family)) if b]
    assert not bad, bad[:3]
