"""The claims of tests/match_cmp16_cases.py against the oracle's streams.  No GPU."""
import zlib

import pytest

import deflate_reader as dr
import match_cases as mc
import match_cmp16_cases as cc


def test_the_catalogue():
    assert len(cc.CASES) == 3 * len(cc.LENGTHS) + 5 + 9 * len(cc.LENGTHS) + 12 + 3
    assert all(len(d) <= 128 * 1024 for d, _ in cc.CASES.values()) and len(cc.PERIODIC) <= 128 * 1024


@pytest.mark.parametrize("level", cc.LEVELS)
def test_every_case_is_the_edge_it_claims_to_be(oracle, level):
    bad = []
    for name, (data, claim) in sorted(cc.CASES.items()):
        z = cc.ref(oracle, name, level)
        assert zlib.decompress(z) == data
        if not claim(mc.tokens(dr.read(z)), level):
            bad.append(name)
    assert bad == []
