"""Inflate's error classes on the device: every case of tests/inflate_bad_cases.py (tests/test_inflate_bad_cases.py holds the
claims against the oracle) through zs_inflate_batch_device -- code, message, length and bytes of each stream alone, in one
batch beside its legal twin, and through ZlibInputStream -- and one legal stream cut at every length and given every short
capacity.  Outputs lie between guard bytes: a failing stream writes nothing outside its capacity.

The C entry point is called through Engine._call_inflate, so that the return code, out_len[] and status[] come back and
nothing is raised."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

import inflate_bad_cases as bc
from zlibstream_amd import ZlibInputStream, ZlibStreamException

pytestmark = pytest.mark.gpu

MODES = {"default": None, "chain_walk": ("ZS_INF_CHAIN_WALK", "1"), "no_tokens": ("ZS_INF_MEASURE_DBG", "3")}
GUARD, FILL = 256, 0xEE
_ORACLE = {}


def ref(oracle, c):
    """The oracle's (code, bytes, message) of a case at the case's capacity, made once."""
    if c[0] not in _ORACLE:
        _ORACLE[c[0]] = oracle.inflate(c[1], bc.capacity(c))
    return _ORACLE[c[0]]


def run_device(engine, streams, caps, shared_input=False):
    """zs_inflate_batch_device on device buffers: every input at a multiple of 256, every output behind at least GUARD bytes
    of FILL and in front of at least GUARD more, which begin at out + cap.  Returns (code, out_len[], status[], what lies in
    out[i][:caps[i]], the streams with a byte changed outside every capacity)."""
    import torch
    n = len(streams)
    in_off, off = [], 0
    for k, z in enumerate(streams):
        in_off.append(0 if shared_input else off)
        if not shared_input or k == 0:
            off += (len(z) + 255) // 256 * 256 + 256
    host_in = np.zeros(off, dtype=np.uint8)
    for k, z in enumerate(streams):
        if not shared_input or k == 0:
            host_in[in_off[k]:in_off[k] + len(z)] = np.frombuffer(z, dtype=np.uint8)
    out_off, off = [], GUARD
    for cap in caps:
        out_off.append(off)
        off = (off + cap + 255) // 256 * 256 + GUARD
    d_in = torch.from_numpy(host_in).cuda()
    d_out = torch.full((off,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, lens, status = engine._call_inflate(engine._lib.zs_inflate_batch_device, [d_in.data_ptr() + o for o in in_off], [len(z) for z in streams],
                                            [d_out.data_ptr() + o for o in out_off], list(caps), (ctypes.c_void_p(0),))
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    outside = got != FILL
    for o, cap in zip(out_off, caps):
        outside[o:o + cap] = False
    dirty = sorted({int(np.searchsorted(out_off, i, side="right")) - 1 for i in np.flatnonzero(outside)})
    return rc, lens, status, [got[o:o + cap].tobytes() for o, cap in zip(out_off, caps)], dirty


def check_against_claims(cases, oracle, rc, lens, status, outs):
    """Element by element: the code; for an accepted stream the bytes; for a data error or a dictionary request the
    oracle's length and bytes."""
    bad = []
    for c, n, st, out in zip(cases, lens, status, outs):
        name, _, want_rc, _, want_len, prefix = c
        o_rc, o_out, _ = ref(oracle, c)
        assert (o_rc, o_out) == (want_rc, prefix), name  # (the claim is the oracle's: tests/test_inflate_bad_cases.py)
        if st != want_rc:
            bad.append((name, "status", st, want_rc))
        elif n != want_len or out[:n] != prefix:
            bad.append((name, "out_len" if n != want_len else "bytes", n, want_len))
    return bad


def test_the_devices_messages_are_the_catalogues():
    """Every message of kInfMessages but the empty one is claimed by a case (or, "buffer error", by the sweeps), so the tests
    below assert each of them on the device; and the catalogue claims none the device does not have."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "zlibstream_amd", "csrc", "zs_engine.hip")).read()
    body = re.search(r"kInfMessages\[kInfMsgCount\] = \{(.*?)\};", src, re.S).group(1)
    device = set(re.findall(r'"([^"]*)"', body)) - {""}
    assert len(device) == 19 and device == bc.messages()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", bc.NAMES)
def test_case_alone(engine, oracle, monkeypatch, name, mode):
    c = bc.case(name)
    _, z, want_rc, message, want_len, prefix = c
    if MODES[mode]:
        monkeypatch.setenv(*MODES[mode])  # (read per call)
    rc, lens, status, outs, dirty = run_device(engine, [z], [bc.capacity(c)])
    wave, said = engine.counter("inf_wave_streams"), engine.last_error()
    print("%s [%s]: %d bytes, rc %d, status %d, out_len %d, inf_wave_streams %d, %r" % (name, mode, len(z), rc, status[0], lens[0], wave, said))
    assert not dirty
    assert status[0] == want_rc
    assert not check_against_claims([c], oracle, rc, lens, status, outs)
    if want_rc == bc.ZS_STREAM_END:
        assert rc == 0 and outs[0] == prefix
        # who decoded it: what the host-pointer call of tests/test_gpu_inflate_built.py's test_built_stream_alone counts
        assert engine.inflate_batch([z], [len(prefix)]) == [prefix]
        assert engine.counter("inf_wave_streams") == wave
    else:
        assert rc == want_rc
        assert said == message == ref(oracle, c)[2]


@pytest.mark.parametrize("order", ["paired", "reversed"])
def test_everything_in_one_batch(engine, oracle, order):
    """Every rejected stream beside its legal twin and beside every other kind of failure: the codes element by element, the
    neighbours exact, and the call's code and message those of the batch's first failing stream."""
    cases = bc.paired()
    if order == "reversed":
        cases.reverse()
    rc, lens, status, outs, dirty = run_device(engine, [c[1] for c in cases], [bc.capacity(c) for c in cases])
    assert not dirty, [cases[i][0] for i in dirty]
    assert [c[0] for c, st in zip(cases, status) if st != c[2]] == []
    assert not check_against_claims(cases, oracle, rc, lens, status, outs)
    first = next(c for c in cases if c[2] != bc.ZS_STREAM_END)
    assert rc == first[2] != 0
    assert engine.last_error() == first[3]


def test_the_calls_message_is_the_first_failing_streams_on_either_path(engine):
    """The block-parallel pass and the one-wave decoder each report their own failures; the call's message goes by the
    caller's order, whichever of them had the first failing stream."""
    small, large = bc.case("btype_3_final_first"), bc.case("trailer_byte_3_behind_6k")  # one-wave decoder; block-parallel pass
    twin = bc.case("trailer_ok_behind_6k")
    for cases in ([small, large], [large, small], [twin, large, small], [twin, small, large]):
        rc, lens, status, outs, dirty = run_device(engine, [c[1] for c in cases], [bc.capacity(c) for c in cases])
        assert status == [c[2] for c in cases] and not dirty
        first = next(c for c in cases if c[2] != bc.ZS_STREAM_END)
        assert rc == first[2] and engine.last_error() == first[3], [c[0] for c in cases]


@pytest.mark.parametrize("mode", ["default", "no_tokens"])
def test_cuts_sweep_in_one_batch(engine, oracle, monkeypatch, mode):
    z, plain, _, _ = bc.sweep()
    if MODES[mode]:
        monkeypatch.setenv(*MODES[mode])
    cuts = [z[:n] for n in range(len(z))]
    rc, lens, status, outs, dirty = run_device(engine, cuts, [len(plain)] * len(cuts))
    assert not dirty, dirty
    assert rc == bc.ZS_BUF_ERROR and [n for n, st in enumerate(status) if st != bc.ZS_BUF_ERROR] == []
    assert [n for n in range(len(cuts)) if lens[n] > len(plain) or outs[n][:lens[n]] != plain[:lens[n]]] == []
    differ = [n for n in range(len(cuts)) if lens[n] != len(oracle.inflate(cuts[n], len(plain))[1])]
    print("cuts [%s]: %d of %d cuts give an out_len other than the oracle's" % (mode, len(differ), len(cuts)))
    assert differ == []  # out_len of a truncated stream: the bytes of the tokens that were complete, as the oracle counts them


def test_cuts_alone_say_buffer_error(engine, oracle):
    """The message, which a batch has only one of: every cut inside the first dynamic header, one inside each block, inside the
    stored block's LEN / NLEN and inside the trailer."""
    z, plain, _, _ = bc.sweep()
    bad = []
    for n in bc.sweep_single_cuts():
        rc, lens, status, outs, dirty = run_device(engine, [z[:n]], [len(plain)])
        want = oracle.inflate(z[:n], len(plain))
        assert (want[0], want[2]) == (bc.ZS_BUF_ERROR, "buffer error")
        if (rc, status[0], engine.last_error(), lens[0], outs[0][:lens[0]]) != (bc.ZS_BUF_ERROR, bc.ZS_BUF_ERROR, "buffer error", len(want[1]), want[1]) or dirty:
            bad.append((n, rc, status[0], engine.last_error(), lens[0], len(want[1]), dirty))
    assert not bad, bad


def test_cuts_of_the_short_rejected_streams(engine, oracle):
    """A malformed stream that is truncated as well: cut in front of the flaw it is a buffer error, behind it the flaw's own
    error, and a cut inside the bits that decide -- a repeat count half there, a code nobody has short of its 15th bit -- is
    still a buffer error.  Every cut of every rejected stream under 1 KiB in one batch, code and length against the
    oracle's; then, alone for the message, every cut at which both say buffer error where the whole stream is refused for
    its code-length sequence."""
    cases = [c for c in bc.CASES if c[2] != bc.ZS_STREAM_END and bc.META[c[0]][2] in ("first", "short", "first_token")]
    assert {bc.META[c[0]][0] for c in cases} == set(bc.RULES)  # (a short rejected stream of every rule)
    cuts = [(c, n) for c in cases for n in range(len(c[1]))]
    want = [oracle.inflate(c[1][:n], bc.capacity(c)) for c, n in cuts]
    rc, lens, status, outs, dirty = run_device(engine, [c[1][:n] for c, n in cuts], [bc.capacity(c) for c, _ in cuts])
    assert not dirty
    bad = [(c[0], n, st, w[0], k, len(w[1])) for (c, n), st, k, out, w in zip(cuts, status, lens, outs, want) if (st, k, out[:k]) != (w[0], len(w[1]), w[1])]
    print("%d cuts of %d short rejected streams: %d differ from the oracle" % (len(cuts), len(cases), len(bad)))
    assert not bad, bad[:20]
    bad = []
    for c in cases:
        if c[3] != "invalid bit length repeat":
            continue
        short = [n for (k, n), w in zip(cuts, want) if k is c and w[0] == bc.ZS_BUF_ERROR]
        assert short and short[-1] > 8  # (the last of them lie inside the code-length sequence)
        for n in short[-12:]:
            rc, lens, status, outs, dirty = run_device(engine, [c[1][:n]], [bc.capacity(c)])
            if (rc, status[0], engine.last_error()) != (bc.ZS_BUF_ERROR, bc.ZS_BUF_ERROR, "buffer error") or dirty:
                bad.append((c[0], n, rc, status[0], engine.last_error()))
    assert not bad, bad


def test_caps_sweep_in_one_batch(engine, oracle):
    """The whole stream into every capacity 0 .. plaintext - 1 (inside the 258-long match and the stored block among them):
    a buffer error, a prefix of the plaintext as long as the tokens that fit, and no byte at or beyond out + cap."""
    z, plain, _, _ = bc.sweep()
    caps = list(range(len(plain)))
    rc, lens, status, outs, dirty = run_device(engine, [z] * len(caps), caps, shared_input=True)
    assert not dirty, dirty
    assert rc == bc.ZS_BUF_ERROR and [cap for cap, st in zip(caps, status) if st != bc.ZS_BUF_ERROR] == []
    assert [cap for cap in caps if lens[cap] > cap or outs[cap][:lens[cap]] != plain[:lens[cap]]] == []
    differ = [cap for cap in caps if lens[cap] != len(oracle.inflate(z, cap)[1])]
    print("caps: %d of %d capacities give an out_len other than the oracle's" % (len(differ), len(caps)))
    assert differ == []
    # alone, for the message: no room at all, one byte, inside the first block's 258-long match, inside the stored block,
    # inside the fixed block's overlapping match, one byte short
    bad = []
    for cap in (0, 1, 600, 3 * 830 + 150, 3 * 830 + 300 + 100, len(plain) - 1):
        rc, lens, status, outs, dirty = run_device(engine, [z], [cap])
        want = oracle.inflate(z, cap)
        if (rc, status[0], engine.last_error(), lens[0], outs[0][:lens[0]]) != (bc.ZS_BUF_ERROR, bc.ZS_BUF_ERROR, "buffer error", len(want[1]), want[1]) or dirty:
            bad.append((cap, rc, status[0], engine.last_error(), lens[0], len(want[1]), dirty))
    assert not bad, bad


@pytest.mark.parametrize("name", [n for n in bc.NAMES if bc.META[n][2] == "behind_100k" and bc.case(n)[2] != bc.ZS_STREAM_END])
def test_rejected_behind_100k_through_zlib_input_stream(engine, name):
    """Read 70 000 bytes at a time.  With a BytesIO underneath the mirror feeds the whole stream before the first decode: the
    end of a malformed stream is not found, so the one call without input decodes it as a first piece that holds everything
    (no piece is resumed here; tests/test_gpu_inflate_stream.py does that).  The exception carries the message, and what
    read() returned before it is a prefix of the plaintext."""
    _, z, _, message, _, prefix = bc.case(name)
    s = ZlibInputStream(io.BytesIO(z), engine=engine)
    got = bytearray()
    with pytest.raises(ZlibStreamException) as ei:
        for _ in range(len(prefix) // 70000 + 3):
            part = s.read(70000)
            if not part:
                break
            got += part
    assert str(ei.value) == "inflating: " + message
    assert bytes(got) == prefix[:len(got)]
