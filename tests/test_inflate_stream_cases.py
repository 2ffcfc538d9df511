"""The claims of tests/inflate_stream_cases.py, checked without the device: every stream is what zlib and the reader say it
is, delivered() is monotone, ends at the plaintext and is a prefix of what zlib's own streaming inflate hands out for the same
bytes, and the schedules run through the protocol's model to the end."""
import zlib

import pytest

import deflate_reader as dr
import inflate_stream_cases as sc

LEGAL = [n for n in sc.case_names() if not (n.startswith("too_far") and not n.endswith("_legal"))]
BAD = [n for n in sc.case_names() if n not in LEGAL]


def test_names_are_the_catalogue():
    assert [c.name for c in sc.catalogue()] == sc.case_names()


@pytest.mark.parametrize("name", LEGAL)
def test_stream_is_what_the_table_says(name):
    c = sc.case(name)
    assert zlib.decompress(c.z) == c.plain
    rd = dr.read(c.z)
    assert [(b.kind, b.bit_pos, b.bits) for b in rd] == [blk[:3] for blk in c.blocks]
    assert dr.replay(rd) == c.plain
    assert [blk[3] for blk in c.blocks] == sorted(blk[3] for blk in c.blocks) and c.blocks[-1][3] == len(c.plain)
    assert all(not b.final for b in rd[:-1]) and rd[-1].final


def _lengths(c):
    if len(c.z) <= 4096 and len(c.plain) <= 1 << 16:
        return range(len(c.z) + 1)
    near = {n + d for n in sc.block_ends(c) + [len(c.z) - 4] for d in range(-3, 4)}
    return sorted(n for n in near | set(range(0, len(c.z), 997)) | {len(c.z)} if 0 <= n <= len(c.z))


@pytest.mark.parametrize("name", LEGAL)
def test_delivered_is_monotone_and_a_prefix_of_zlibs(name):
    c = sc.case(name)
    last = 0
    for n in _lengths(c):
        d = sc.delivered(c, n)
        assert d >= last, n
        last = d
        got = zlib.decompressobj().decompress(c.z[:n])
        assert len(got) >= d and got == c.plain[:len(got)], n
    assert sc.delivered(c, len(c.z)) == len(c.plain)
    assert sc.delivered(c, len(c.z) - 1) == (c.blocks[-2][3] if len(c.blocks) > 1 else 0)  # the final block waits for its trailer


def test_mixed_small_phases_and_kinds():
    c = sc.case("mixed_small")
    assert len(c.z) < 1024
    assert {blk[1] & 7 for blk in c.blocks} == set(range(8))
    assert any(blk[0] == "stored" and blk[1] & 7 for blk in c.blocks)
    assert ("fixed", 10, 0) in {(blk[0], blk[2], blk[3] - (c.blocks[i - 1][3] if i else 0)) for i, blk in enumerate(c.blocks)}
    assert any(blk[0] == "stored" and blk[3] == c.blocks[i - 1][3] for i, blk in enumerate(c.blocks) if i)  # the flush marker
    assert {"dynamic", "fixed", "stored"} == {blk[0] for blk in c.blocks}
    # the fixed block's last match reaches the stream's first byte
    rd = dr.read(c.z)
    at = 0
    reaches = []
    for b in rd:
        for t in (b.symbols or []) if b.kind != "stored" else []:
            if isinstance(t, int):
                at += 1
            else:
                reaches.append((b.kind, t[1] == at))
                at += t[0]
        if b.kind == "stored":
            at += b.len
    assert ("fixed", True) in reaches


def test_mixed_probe_is_the_sweep():
    c = sc.case("mixed_probe")
    assert 2400 <= len(c.z) <= 3100 and {"dynamic", "fixed", "stored"} == {blk[0] for blk in c.blocks}


@pytest.mark.parametrize("name", [n for n in LEGAL if n.startswith("hist_edges")])
def test_hist_edges_first_token_reaches_the_oldest_byte(name):
    c = sc.case(name)
    h = c.info["h"]
    rd = dr.read(c.z)
    k = next(i for i, blk in enumerate(c.blocks) if blk[3] > h)
    assert c.blocks[k - 1][3] == h and sc.block_end_byte(c.blocks[k - 1]) == c.info["cut"]
    syms = rd[k].symbols
    assert syms[0] == (20, min(h, 32768)) and (258, 1) in syms and ((258, 32768) in syms) == (h >= 32767)
    if name.endswith("many") and h > 5120:
        sizes = [blk[3] - (c.blocks[i - 1][3] if i else 0) for i, blk in enumerate(c.blocks[:k])]
        assert all(3072 <= s <= 5120 for s in sizes[:-1]) and len(sizes) >= 7


@pytest.mark.parametrize("name", BAD)
def test_too_far_is_rejected_and_its_twin_accepted(name):
    c = sc.case(name)
    with pytest.raises(zlib.error, match="invalid distance too far back"):
        zlib.decompress(c.z)
    assert zlib.decompressobj().decompress(c.z[:c.info["cut"]]) == c.plain and len(c.plain) == c.info["h"]
    twin = sc.case(name.replace("_uncut", "") + "_legal")
    assert zlib.decompress(twin.z)[:len(c.plain)] == c.plain and twin.z[:c.info["cut"] - 1] == c.z[:c.info["cut"] - 1]


@pytest.mark.parametrize("name", ["ring_wrap", "ring_wrap_stored"])
def test_ring_wrap_places(name):
    c = sc.case(name)
    h = 32768
    rd = dr.read(c.z)
    at, found, stored = 0, [], []
    for b in rd:
        if b.kind == "stored":
            stored.append((at - h, at - h + b.len))
            at += b.len
            continue
        for t in b.symbols:
            if isinstance(t, int):
                at += 1
            else:
                found.append((at - h, t))
                at += t[0]
    assert [t for _, t in found] == [(258, 32768)] * len(c.info["matches"])
    for (p, _), edge in zip(found, c.info["matches"]):
        assert p <= edge - 1 and edge + 1 < p + 258  # bytes on both sides of the ring position
    (s0, s1), = [s for s in stored if s[1] - s[0] == 50000]
    assert any(s0 < e < s1 - 1 for e in range(32767, sc.RING_PIECE, 32768))
    assert c.blocks[-2][3] - h == sc.RING_PIECE


def test_full_output_shapes():
    c = sc.case("full_output")
    sizes = [blk[3] - (c.blocks[i - 1][3] if i else 0) for i, blk in enumerate(c.blocks)]
    assert len(sizes) == 7 and all(600000 <= s <= 640000 for s in sizes[:6]) and max(blk[2] for blk in c.blocks) < 8 * 1000
    assert max(8 * len(c.z), 1 << 20) < sizes[0] + sizes[1]  # the second block does not fit the first capacity
    t = sc.case("full_output_twin")
    assert t.blocks[0][3] == 3 << 20 and max(8 * len(t.z), 1 << 20) < 3 << 20


def test_tiny_phases_resumes():
    c = sc.case("tiny_phases")
    cuts = c.info["cuts"]
    assert len(cuts) == 300 and cuts == sorted(set(cuts))
    phases = [sc.resume_phase(c, n) for n in cuts]
    assert all(phases.count(p) >= 20 for p in range(8)), [phases.count(p) for p in range(8)]
    kinds = [blk[0] for blk in c.blocks if blk[2] != 10]
    assert kinds.count("fixed") >= 100 and kinds.count("dynamic") >= 100


@pytest.mark.parametrize("name", [n for n in sc.case_names() if not n.startswith("full_output")])
def test_schedule_runs_through_the_model(name):
    c = sc.case(name)
    steps, surplus = sc.expect(c, c.schedule)
    assert sum(t for _, t, _ in steps) == len(c.z) and surplus == b""
    got = b"".join(g for _, _, g in steps)
    if sc.is_bad(c):
        assert steps[-1][0] == sc.ZS_DATA_ERROR and got == (c.plain if not name.endswith("uncut") else b"")
    else:
        assert steps[-1][0] == sc.ZS_STREAM_END and got == c.plain
        assert [rc for rc, _, _ in steps].count(sc.ZS_STREAM_END) == 1
