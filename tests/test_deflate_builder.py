"""The hand-built deflate streams of tests/deflate_builder.py against two decoders that are not the device's: Python's zlib
and the oracle.  This is the ground tests/test_gpu_inflate_built.py stands on: every case of the catalogue is a conformant
stream with the plaintext the builder kept, whoever decodes it.  No case is left out."""
import zlib

import pytest

import deflate_builder as db


def test_catalogue_names_and_sizes():
    cat = db.catalogue()
    assert [c[0] for c in cat] == db.case_names()
    assert all(len(c[1]) <= db.MAX_STREAM for c in cat) and sum(len(c[1]) for c in cat) <= db.MAX_TOTAL
    want_fallback = {"empties_small", "tiny_blocks_dense", "tiny_blocks_sparse", "empty_fixed_run", "fixed_all_small", "long_block_over"}
    assert {c[0] for c in cat if c[3]} == want_fallback


@pytest.mark.parametrize("name", db.case_names())
def test_reference_decoders_accept_every_case(oracle, name):
    _, z, plain, _ = db.case(name)
    assert z[:2] == b"\x78\x9c"
    assert zlib.decompress(z) == plain
    assert oracle.inflate(z, len(plain)) == (1, plain, None)
    if name.startswith("threshold_"):
        assert len(z) == int(name.split("_")[1])
    else:
        assert len(z) >= db.PAR_MIN


def test_canonical_codes_of_a_known_length_list():
    # RFC 1951 3.2.2: lengths (3, 3, 3, 3, 3, 2, 4, 4) for A..H give 010 011 100 101 110 00 1110 1111
    assert db.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [(2, 3), (3, 3), (4, 3), (5, 3), (6, 3), (0, 2), (14, 4), (15, 4)]
    assert db.canonical_codes([0, 1, 0]) == [(0, 0), (0, 1), (0, 0)]  # one code of length 1: the format's one incomplete code
    assert db.canonical_codes([2, 0, 1, 2]) == [(2, 2), (0, 0), (0, 1), (3, 2)]


@pytest.mark.parametrize("lengths", [[2, 2, 2], [1, 1, 1], [2], [0, 0], [1, 16, 16], [3, 3, 3, 3, 3, 2, 4]])
def test_lengths_that_are_no_code_are_refused(lengths):
    with pytest.raises(ValueError):
        db.canonical_codes(lengths)


def test_bit_writer_fields_lsb_first_codes_msb_first():
    b = db.Builder()
    b.put(0b101, 3)        # a field: its low bit first
    b.code(0b110, 3)       # a Huffman code: its high bit first -> 1, 1, 0
    b.put(0x1FF, 9)
    b.align()
    assert bytes(b.buf[2:]) + b.acc.to_bytes(b.n // 8, "little") == bytes([0b11011101, 0b01111111])
    assert b.bit_pos == 32


def test_length_limits_and_header_forms():
    # a skewed code: plain Huffman lengths would pass 15 bits (literal / length) and 7 (the bit-length code)
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    assert max(db.huffman_lengths(fib, 64)) == 29
    for freqs, limit in ((fib, 15), (fib[:19], 7)):
        lens = db.huffman_lengths(freqs, limit)
        assert max(lens) <= limit and sum(1 << (limit - l) for l in lens) == 1 << limit  # within the limit, and complete
    b = db.Builder()
    toks = [s for s, f in enumerate(fib[:24]) for _ in range(f)]
    b.dynamic_block(toks, False)
    b.dynamic_block([], False)                      # end-of-block alone: one code of 1 bit, HLIT 257, HDIST 1 with a zero length
    b.dynamic_block([(258, 1)] * 3, False, alt258=True)
    b.stored_block(b"", False, pad_ones=True)
    b.fixed_block([1, (3, 1)], True)
    assert [k for k, _, _ in b.blocks] == ["dynamic", "dynamic", "dynamic", "stored", "fixed"]
    assert b.blocks[0][1] == 16 and all(b.blocks[i][1] + b.blocks[i][2] == b.blocks[i + 1][1] for i in range(4))
    z = b.finish(pad_ones=True)
    assert zlib.decompress(z) == bytes(b.plaintext) == bytes(toks) + bytes([toks[-1]]) * 774 + b"\x01" * 4


def test_the_same_seed_builds_the_same_stream():
    import random
    a = db.random_codes_stream(random.Random(9))
    assert a == db.random_codes_stream(random.Random(9)) and zlib.decompress(a[0]) == a[1] and len(a[0]) >= db.PAR_MIN
