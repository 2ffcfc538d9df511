"""tests/deflate_reader.py against tests/deflate_builder.py: what the reader finds in every stream of the builder's catalogue is
what the builder wrote -- block kinds and bit positions, the code lengths of every dynamic block, the plaintext.  The two share
the format's constant tables and nothing else.  tests/emit_cases.py states its claims through this reader."""
import pytest

import deflate_builder as db
import deflate_reader as dr


@pytest.mark.parametrize("name", db.case_names())
def test_reader_finds_what_the_builder_wrote(name):
    _, z, plain, _ = db.case(name)
    blocks, lengths = db.LAYOUT[z]
    got = dr.read(z)
    assert [(b.kind, b.bit_pos, b.bits) for b in got] == list(blocks)
    assert [b.final for b in got] == [False] * (len(got) - 1) + [True]
    dyn = [b for b in got if b.kind == "dynamic"]
    assert [(b.bit_pos, b.lit_lengths, b.dist_lengths, b.bl_lengths) for b in dyn] == [tuple(l) for l in lengths]
    for b in dyn:
        assert (b.hlit, b.hdist) == (len(b.lit_lengths), len(b.dist_lengths))
        assert sum(r for _, r in b.sent) == b.hlit + b.hdist
        assert b.hclen == max(4, max(i for i, s in enumerate(db.CL_ORDER) if b.bl_lengths[s]) + 1)
    for b in got:
        if b.kind == "stored":
            assert len(b.data) == b.len and b.bits == (-(b.bit_pos + 3) % 8) + 3 + 32 + 8 * b.len
        else:
            assert len(b.sym_bits) == len(b.symbols) + 1 and b.lit_hist[dr.END_BLOCK] == 1
            assert sum(b.lit_hist) == len(b.symbols) + 1 and sum(b.dist_hist) == sum(1 for t in b.symbols if not isinstance(t, int))
            header = b.bits - sum(b.sym_bits)
            assert header == 3 if b.kind == "fixed" else header >= 3 + 14 + 3 * b.hclen
    assert dr.replay(got) == plain


def test_damaged_streams_are_refused():
    _, z, _, _ = db.case("alt258")
    for bad in (z[:-1], z + b"\0", z[:-1] + bytes([z[-1] ^ 1]), b"\x78\x9d" + z[2:], z[:2] + bytes([z[2] | 6]) + z[3:]):
        with pytest.raises(ValueError):
            dr.read(bad)


def test_optimal_cost_is_the_huffman_cost_whatever_the_ties():
    assert dr.optimal_cost([]) == 0 and dr.optimal_cost([0, 7, 0]) == 7
    assert dr.optimal_cost([1, 1, 1, 1]) == 8 and dr.optimal_cost([1, 1, 2, 4]) == 2 + 4 + 8
    for limit, freqs in ((64, [1, 1, 2, 3, 5, 8, 13, 21, 34, 55]), (64, [5] * 19), (64, [3, 0, 9, 1, 1, 0, 40])):
        lens = db.huffman_lengths(freqs, limit)
        assert dr.code_cost(freqs, lens) == dr.optimal_cost(freqs) and not dr.repair_ran(freqs, lens, max(lens) + 1)
    fib = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55]
    assert dr.code_cost(fib, db.huffman_lengths(fib, 6)) > dr.optimal_cost(fib)   # a limit below the natural depth costs bits
    with pytest.raises(ValueError):
        dr.code_cost([1, 1], [1, 0])


def test_k9_max_pending_by_hand():
    class B:
        pass
    b = B()
    b.sym_bits = [15, 48]                 # nothing put at 15; 63 at the put, 56 leave
    assert dr.k9_max_pending(b) == 63
    b.sym_bits = [8] * 8 + [15, 42]       # a new group of 8 starts empty
    assert dr.k9_max_pending(b) == 57
    b.sym_bits = [8] * 7 + [15, 42]       # ... so 15 bits at a group's end do not meet the 42 behind them
    assert dr.k9_max_pending(b) == 42
    b.sym_bits = [9, 9, 9]                # 18 -> 2 stay; 11: no put
    assert dr.k9_max_pending(b) == 18
