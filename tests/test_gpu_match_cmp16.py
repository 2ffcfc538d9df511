"""The match kernel's 16-byte first compare (zlibstream_amd/csrc/zs_kernels.hip, match_walk, ZS_CMP16) on the inputs of
tests/match_cmp16_cases.py, byte for byte against the oracle at levels 4, 6 and 9.  Why a case is here is its claim, which
tests/test_match_cmp16_cases.py holds against the oracle's stream on the CPU; here only bytes are compared."""
import zlib

import pytest

import match_cmp16_cases as cc

pytestmark = pytest.mark.gpu

NAMES = sorted(cc.CASES)


@pytest.mark.parametrize("level", cc.LEVELS)
def test_exact_lengths_in_one_batch(engine, oracle, level):
    """every case beside the others: deciding candidates of exactly 7 .. 258 bytes as the first of the chain, behind a shorter
    one and tying the best; nice_length reached at 16 and 17 bytes; zero runs that end with the input 9 .. 17 bytes behind a
    position; probes 3, 12 and 20 bytes in front of a tile boundary; the quarter-budget record frozen by an improvement in
    bytes 8 .. 15"""
    got = engine.deflate_batch([cc.CASES[n][0] for n in NAMES], level=level)
    assert [n for n, z in zip(NAMES, got) if z != cc.ref(oracle, n, level)] == []
    assert all(zlib.decompress(z) == cc.CASES[n][0] for n, z in zip(NAMES, got))


@pytest.mark.parametrize("level", cc.LEVELS)
def test_exact_lengths_alone(engine, oracle, level):
    """one stream per call, so that the tile holds nothing but the case: the candidate families, the tile crossings and the frozen
    records (the zero runs are in the batch above)"""
    names = [n for n in NAMES if not n.startswith("end_")]
    bad = [n for n in names if engine.deflate_batch([cc.CASES[n][0]], level=level)[0] != cc.ref(oracle, n, level)]
    assert bad == []


@pytest.mark.parametrize("level", cc.LEVELS)
def test_a_periodic_buffer_takes_the_runs_walk_as_before(engine, oracle, level):
    """80 000 bytes of period 7 and one text-like case behind them: the tiles of the run take the RUNS instance of the walk,
    whose 8-byte compare and hint are unchanged"""
    assert engine.deflate_batch([cc.PERIODIC], level=level)[0] == oracle.compress(cc.PERIODIC, level, 0)
