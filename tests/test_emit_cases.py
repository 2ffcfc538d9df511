"""The claims of tests/emit_cases.py, held against the oracle's streams on the CPU: every case of the catalogue is in it for
what the reference's encoder does with it, and this file is where that is checked -- through tests/deflate_reader.py, which
tests/test_deflate_reader.py checks in turn.  The device is not involved; tests/test_gpu_emit_cases.py asks it for these bytes.
The figures asserted here are the ones in DESIGN.md section 4."""
import zlib

import pytest

import deflate_reader as dr
import emit_cases as ec

_STREAMS = {}


def ref(oracle, name, level=None, strategy=None):
    """The oracle's stream of a case, by default at the case's own level and strategy, made once."""
    _, data, lvl, strat, _ = ec.case(name)
    key = (name, lvl if level is None else level, strat if strategy is None else strategy)
    if key not in _STREAMS:
        _STREAMS[key] = oracle.compress(data, key[1], key[2])
    return _STREAMS[key]


def test_names():
    assert [c[0] for c in ec.catalogue()] == ec.case_names() and len(set(ec.case_names())) == len(ec.case_names())
    assert max(len(c[1]) for c in ec.catalogue()) == len(ec.case("dist_overflow")[1]) == 1079349  # the largest input: 1 MiB


@pytest.mark.parametrize("name", ec.case_names())
def test_claim_holds_on_the_oracles_stream(oracle, name):
    _, data, level, strategy, claim = ec.case(name)
    z = ref(oracle, name)
    assert zlib.decompress(z) == data
    blocks = dr.read(z)
    assert dr.replay(blocks) == data
    assert claim(blocks)


def test_dist_overflow_at_the_other_levels(oracle):
    _, data, _, _, claim = ec.case("dist_overflow")
    for level, strategy in ec.DIST_OVERFLOW_ALSO:
        assert claim(dr.read(ref(oracle, "dist_overflow", level, strategy))), (level, strategy)
    for level, strategy in ec.DIST_OVERFLOW_BYTES_ONLY:  # another parse, nothing to repair
        blocks = dr.read(ref(oracle, "dist_overflow", level, strategy))
        assert dr.replay(blocks) == data and not any(ec._dist_repair(b) for b in blocks if b.kind == "dynamic"), (level, strategy)


def test_repair_depths(oracle):
    """The shapes behind the three literal/length cases: 19, 17 and 16 symbols in use whose unconstrained Huffman depth is one
    less (a chain: each count exceeds the sum of all smaller ones by END_BLOCK's 1 at the most)."""
    for name, used, n15, extra in (("lit_overflow", 19, 6, 8), ("lit_overflow_by_one", 17, 4, 1), ("lit_natural_15", 16, 2, 0)):
        b = dr.read(ref(oracle, name))[0]
        lens = [l for l in b.lit_lengths if l]
        assert len(lens) == used and lens.count(15) == n15
        assert dr.code_cost(b.lit_hist, b.lit_lengths) - dr.optimal_cost(b.lit_hist) == extra
    assert dr.read(ref(oracle, "lit_overflow"))[0].lit_lengths[dr.END_BLOCK] == 15  # (last_eob_len of the flush accounting)
    b = dr.read(ref(oracle, "dist_overflow"))[0]
    assert (dr.code_cost(b.dist_hist, b.dist_lengths), dr.optimal_cost(b.dist_hist), len(b.symbols)) == (10926, 10925, 5102)
    assert ec._bl_repair(b)  # ... and its bit-length tree was repaired as well
    b = dr.read(ref(oracle, "bl_overflow"))[0]
    assert (dr.code_cost(dr.bl_hist(b), b.bl_lengths), dr.optimal_cost(dr.bl_hist(b))) == (634, 627)


def test_catalogue_as_a_whole(oracle):
    """HCLEN at its largest and at the smallest the catalogue reaches; the stored block of stored_phase at every bit phase; the
    repeat codes at both ends of their ranges; the longest symbol."""
    dyn = [(c[0], b) for c in ec.catalogue() for b in dr.read(ref(oracle, c[0])) if b.kind == "dynamic"]
    hclen = {b.hclen for _, b in dyn}
    assert (min(hclen), max(hclen)) == (15, 19), sorted(hclen)
    sent = {s for _, b in dyn for s in b.sent}
    assert sent >= {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)}
    assert {b.hlit for _, b in dyn} >= {257, 286} and {b.hdist for _, b in dyn} >= {2, 30}
    phases = sorted(dr.read(ref(oracle, "stored_phase_%02d" % v))[1].bit_pos % 8 for v in range(ec.STORED_PHASE_VARIANTS))
    assert sorted(set(phases)) == list(range(8)), phases
    long_block = dr.read(ref(oracle, "long_symbols"))[-1]
    assert max(long_block.sym_bits) == 44 and dr.k9_max_pending(long_block) == 58
    assert len({i % 8 for i, n in enumerate(long_block.sym_bits) if n >= 40}) >= 4
    # (48 bits is the format's longest symbol and 15 + 48 = 63 the most the accumulator can hold at a put, so `fl` never passes
    # 56: the cap is the put of 56 bits that leaves up to 7 behind)
    assert max(dr.k9_max_pending(b) for _, b in dyn) < 64


@pytest.mark.parametrize("level,strategy", ec.SWEEP_SETTINGS)
def test_block_type_sweep(oracle, level, strategy):
    kinds = {}
    for g, datas in ec.sweep_inputs().items():
        kinds[g] = []
        for d in datas:
            blocks = dr.read(oracle.compress(d, level, strategy))
            assert len(blocks) == 1 and dr.replay(blocks) == d
            kinds[g].append(blocks[0].kind)
    assert ec.sweep_claim(kinds, strategy), {g: [(n, k) for n, k in enumerate(ks) if n == 0 or k != ks[n - 1]] for g, ks in kinds.items()}


def test_flush_cases_end_in_the_block_kind_they_name(oracle):
    for name, data, level, strategy, kind in ec.flush_cases():
        blocks = dr.read(oracle.compress(data, level, strategy))
        assert [b.kind for b in blocks] == [kind], name
        for flush in (1, 2, 3):
            z = oracle.compress_writes(data + data, level, strategy, [len(data), len(data)], [flush, 0])
            blocks = dr.read(z)
            assert blocks[0].kind == kind and not blocks[0].final and dr.replay(blocks) == data + data
            assert any(b.kind != "stored" and b.symbols == [] or b.kind == "stored" and b.len == 0 for b in blocks[1:-1])  # the marker
