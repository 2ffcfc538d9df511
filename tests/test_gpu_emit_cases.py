"""The encoder's back end on the device -- trees (K7, zs_trees_kernel: build_tree_wave and the sequential repair behind it), block
placement (K8, zs_offsets_kernel) and bit packing (K9, zs_emit_bits_kernel) -- on the inputs of tests/emit_cases.py, byte for
byte against the oracle.  Why a case is here is its claim, which tests/test_emit_cases.py holds against the oracle's stream on
the CPU; here only bytes are compared, and a claim is never evaluated on the device's stream."""
import io
import zlib

import pytest

import emit_cases as ec
from test_emit_cases import ref
from zlibstream_amd import CompressionLevel, CompressionStrategy, ZlibOptions, ZlibOutputStream, deflate_bound

pytestmark = pytest.mark.gpu

BATCH_SETTINGS = ((6, ec.DEFAULT), (1, ec.DEFAULT), (6, ec.HO), (1, ec.HO), (9, ec.HO), (6, ec.RLE), (6, ec.FIXED))


def _settings(name):
    _, _, level, strategy, _ = ec.case(name)
    out = [(level, strategy)]
    if strategy == ec.HO:
        out += [s for s in ((1, ec.HO), (9, ec.HO)) if s != (level, strategy)]
    if name == "dist_overflow":
        out += list(ec.DIST_OVERFLOW_ALSO + ec.DIST_OVERFLOW_BYTES_ONLY)
    return out


@pytest.mark.parametrize("name", ec.case_names())
def test_case_alone(engine, oracle, monkeypatch, name):
    data = ec.case(name)[1]
    for level, strategy in _settings(name):
        z = engine.deflate_batch([data], level=level, strategy=strategy)[0]
        assert z == ref(oracle, name, level, strategy), (name, level, strategy)
        assert zlib.decompress(z) == data
    if name == "dist_overflow":  # ... and with the symbols from the transfer maps instead of the speculative walk
        monkeypatch.setenv("ZS_NO_SPEC", "1")
        assert engine.deflate_batch([data], level=6)[0] == ref(oracle, name)


@pytest.mark.parametrize("order", ["catalogue", "reversed"])
@pytest.mark.parametrize("level,strategy", BATCH_SETTINGS)
def test_catalogue_in_one_batch(engine, oracle, level, strategy, order):
    """K7 and K9 run over flat lists of the batch's live blocks: every case beside every kind of neighbour."""
    names = ec.case_names()[::-1] if order == "reversed" else ec.case_names()
    got = engine.deflate_batch([ec.case(n)[1] for n in names], level=level, strategy=strategy)
    bad = [n for n, z in zip(names, got) if z != ref(oracle, n, level, strategy)]
    assert not bad, bad


@pytest.mark.parametrize("level,strategy", ec.SWEEP_SETTINGS)
def test_block_type_sweep_in_one_batch(engine, oracle, level, strategy):
    """n = 0..512 bytes of three generators: the sizes at which stored, static and dynamic blocks change over."""
    datas = [d for g in sorted(ec.sweep_inputs()) for d in ec.sweep_inputs()[g]]
    got = engine.deflate_batch(datas, level=level, strategy=strategy)
    bad = [len(d) for d, z in zip(datas, got) if z != oracle.compress(d, level, strategy)]
    assert not bad, bad[:20]


@pytest.mark.parametrize("name", ["lit_overflow", "stored_phase_00", "stored_phase_10", "tile_2048"])
def test_out_pointer_at_every_byte_offset_and_exact_capacity(engine, oracle, name):
    """deflate_batch_device with `out` 0, 1, 2 and 3 bytes into a buffer of 0xA5: K9 packs into the aligned words under the
    pointer, the block's first and last word by atomicOr.  With the bound as capacity and with the stream's exact length: the
    oracle's bytes, and not a byte changed in front of `out` or from `out + out_cap` on."""
    import torch
    _, data, level, strategy, _ = ec.case(name)
    want = ref(oracle, name)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    front, back = 64, 64
    for off in (0, 1, 2, 3):
        for cap in (deflate_bound(len(data)), len(want)):
            buf = torch.full((front + off + cap + back,), 0xA5, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 4 == 0
            torch.cuda.synchronize()
            n = engine.deflate_batch_device([d_in.data_ptr()], [len(data)], [buf.data_ptr() + front + off], [cap], level=level, strategy=strategy,
                                            stream=torch.cuda.current_stream().cuda_stream)[0]
            torch.cuda.synchronize()
            host = buf.cpu().numpy().tobytes()
            assert n == len(want) and host[front + off:front + off + n] == want, (off, cap)
            assert host[:front + off] == b"\xa5" * (front + off) and host[front + off + cap:] == b"\xa5" * back, (off, cap)


@pytest.mark.parametrize("flush", [1, 2, 3])
def test_flush_behind_a_block_of_each_kind(engine, oracle, flush):
    """A Write that ends in a dynamic block whose END_BLOCK code is 15 bits long (last_eob_len of K8's flush accounting), in a
    Fixed block and in a stored block; a Partial, Sync or Full flush; the same data once more."""
    for name, data, level, strategy, _ in ec.flush_cases():
        out = io.BytesIO()
        s = ZlibOutputStream(out, ZlibOptions(CompressionLevel=CompressionLevel(level), CompressionStrategy=CompressionStrategy(strategy),
                                              FlushMode=flush), engine=engine)
        s.write(data)
        s.Options.FlushMode = 0
        s.write(data)
        s.close()
        z = out.getvalue()
        assert z == oracle.compress_writes(data + data, level, strategy, [len(data), len(data)], [flush, 0]), (name, flush)
        assert zlib.decompress(z) == data + data
