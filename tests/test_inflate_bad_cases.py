"""The claims of tests/inflate_bad_cases.py, held against the oracle (code, message, length and bytes) and against zlib
(raises, or returns the plaintext) on the CPU.  The device is not involved; tests/test_gpu_inflate_bad_cases.py asks it for
the same answers."""
import zlib

import pytest

import deflate_builder as db
import inflate_bad_cases as bc

# every rule of the catalogue, and the messages its rejected side must produce between them
RULE_MESSAGES = {
    "CM": {"unknown compression method"},
    "CINFO": {"invalid window size"},
    "FCHECK": {"incorrect header check"},
    "FDICT": {"need dictionary"},
    "BTYPE": {"invalid block type"},
    "stored LEN/NLEN": {"invalid stored block lengths"},
    "HLIT / HDIST": {"too many length or distance symbols"},
    "bit-length code": {"oversubscribed dynamic bit lengths tree", "incomplete dynamic bit lengths tree"},
    "repeat": {"invalid bit length repeat"},
    "literal/length code": {"oversubscribed literal/length tree", "incomplete literal/length tree"},
    "distance code": {"oversubscribed distance tree", "incomplete distance tree", "empty distance tree with lengths"},
    "symbols": {"invalid literal/length code", "invalid distance code"},
    "distance reach": {"invalid distance code"},
    "trailer": {"incorrect data check"},
}


def test_rules_counts_and_both_sides_of_every_rule():
    assert len(set(bc.NAMES)) == len(bc.NAMES) == len(bc.CASES)
    assert set(bc.RULES) == set(RULE_MESSAGES)
    print("%d rules, %d cases (%d rejected, %d accepted)" % (len(bc.RULES), len(bc.CASES), sum(1 for c in bc.CASES if c[2] != bc.ZS_STREAM_END),
                                                         sum(1 for c in bc.CASES if c[2] == bc.ZS_STREAM_END)))
    for rule, sides in bc.RULES.items():
        print("  %-20s %2d rejected, %2d accepted" % (rule, len(sides["rejected"]), len(sides["accepted"])))
        assert sides["rejected"] and sides["accepted"], rule
        assert {bc.case(n)[3] for n in sides["rejected"]} == RULE_MESSAGES[rule], rule
        for n in sides["accepted"]:
            # legal, or -- the bit-length code's single 1-bit code, which no legal block can follow -- past this rule and refused by a later one
            if n in bc.PASSES_ONLY:
                assert bc.PASSES_ONLY[n] == rule and bc.case(n)[3] not in RULE_MESSAGES[rule], n
            else:
                assert bc.case(n)[2] == bc.ZS_STREAM_END and bc.case(n)[3] is None, n
    assert set(bc.PASSES_ONLY.values()) == {"bit-length code"}
    # every rejected kind that can be placed is there in the three placements
    placed = {}
    for n in bc.NAMES:
        for pl in bc.PLACEMENTS:
            if n.endswith("_" + pl) and bc.case(n)[2] != bc.ZS_STREAM_END:
                placed.setdefault(n[:-len(pl) - 1], set()).add(pl)
    whole = {k for k, v in placed.items() if v == set(bc.PLACEMENTS)}
    assert len(whole) >= 28, sorted(whole)
    header = {"CM", "CINFO", "FCHECK", "FDICT"}  # (a header cannot be placed)
    assert {bc.case(k + "_first")[3] for k in whole} == set().union(*(m for r, m in RULE_MESSAGES.items() if r not in header))
    for n in bc.NAMES:
        pl, z = bc.META[n][2], bc.case(n)[1]
        if pl in ("first", "short"):
            assert len(z) < db.PAR_MIN or n == "stored_len_65535", n
        if pl in ("behind_6k", "behind_100k", "long"):
            assert len(z) >= db.PAR_MIN, n
        if pl == "behind_100k":
            assert bc.case(n)[4] >= 100000, n
    assert max(len(c[1]) for c in bc.CASES) < 110000 and max(c[4] for c in bc.CASES) < 140000


def test_messages_are_the_oracles_whole_list():
    """Every message the oracle's inflate can give is claimed by a case (the sweeps claim "buffer error")."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "zs_inflate_oracle.c")).read()
    said = set(re.findall(r'(?:BAIL|fail)\([^"\n]*"([^"]+)"\)', src))
    assert len(said) == 19 and said == bc.messages()


@pytest.mark.parametrize("rule", sorted(RULE_MESSAGES))
def test_claims_hold_against_the_oracle_and_zlib(oracle, rule):
    bad = []
    for name in bc.NAMES:
        if bc.META[name][0] != rule:
            continue
        c = bc.case(name)
        _, z, rc, message, out_len, prefix = c
        assert out_len == len(prefix)
        got_rc, got, got_message = oracle.inflate(z, bc.capacity(c))
        if (got_rc, got_message, len(got)) != (rc, message, out_len) or got != prefix:
            bad.append((name, got_rc, got_message, len(got)))
        if rc == bc.ZS_STREAM_END:
            if zlib.decompress(z) != prefix:
                bad.append((name, "zlib differs"))
        else:
            try:
                zlib.decompress(z)
                bad.append((name, "zlib accepts"))
            except zlib.error:  # (its wording differs: only that it raises)
                pass
    assert not bad, bad


def test_every_cut_of_the_sweep_stream_is_a_buffer_error(oracle):
    z, plain, blocks, header_end = bc.sweep()
    assert zlib.decompress(z) == plain and oracle.inflate(z, len(plain)) == (1, plain, None)
    assert [k for k, _, _ in blocks] == ["dynamic"] * 3 + ["stored", "fixed", "dynamic"]
    bad = []
    for n in range(len(z)):
        rc, got, message = oracle.inflate(z[:n], len(plain))
        if (rc, message) != (bc.ZS_BUF_ERROR, "buffer error") or got != plain[:len(got)]:
            bad.append(n)
    assert not bad, bad
    cuts = bc.sweep_single_cuts()
    assert set(range(header_end + 1)) <= set(cuts) and max(cuts) == len(z) - 1 and len(cuts) < 110


def test_every_short_capacity_of_the_sweep_stream_is_a_buffer_error(oracle):
    z, plain, _, _ = bc.sweep()
    bad = []
    for cap in range(len(plain)):
        rc, got, message = oracle.inflate(z, cap)
        if (rc, message) != (bc.ZS_BUF_ERROR, "buffer error") or got != plain[:len(got)] or len(got) > cap:
            bad.append(cap)
    assert not bad, bad
