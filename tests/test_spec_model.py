"""CPU model of the speculative chunk walk (tests/model/zs_spec_model.cpp) against the oracle's symbol, block and read trace:
every chunk of the speculative grid walked from a guessed entry, the guesses verified against the exits, the symbols emitted
from the verified entries -- with the same ZS_HD code the kernels compile.  A stream that does not verify (periodic data, an
equal-bucket read event) is the maps' and must say so; one that verifies must be the oracle's, symbol for symbol."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "zs_spec_model")
CORPUS = os.path.join(ROOT, "tests", "golden", "corpus")
LENS = "512,1024,2048"


def build_model():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", EXE, os.path.join(ROOT, "tests/model/zs_spec_model.cpp"),
                    os.path.join(ROOT, "oracle/zs_oracle.c"), os.path.join(ROOT, "oracle/zs_inflate_oracle.c")], check=True)
    return EXE


@pytest.fixture(scope="module")
def exe():
    return build_model()


def run_model(exe, path, level, strategy=0, lens=LENS, warm=128, corrupt=None):
    """{chunk length: {"path": "spec" | "maps", "wrong": wrong guesses, "bail": 0 | 1}} -- every line must be a PASS: what the
    model emits on the speculative path is the oracle's"""
    cmd = [exe, path, str(level), str(strategy), lens, str(warm)] + ([str(corrupt)] if corrupt is not None else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("PASS", "FAIL"))]
    assert r.returncode == 0 and lines and all(l.startswith("PASS") for l in lines), (cmd, r.stdout[-800:])
    out = {}
    for l in lines:
        f = dict(kv.split("=", 1) for kv in l.split() if "=" in kv)
        if "len" in f:
            out[int(f["len"])] = {"path": f["path"], "wrong": int(f.get("wrong", 0)), "bail": int(f.get("bail", 0))}
    return out


def _run(exe, path, level, strategy=0, lens=LENS, warm=128, corrupt=None):
    return {n: v["path"] for n, v in run_model(exe, path, level, strategy, lens, warm, corrupt).items()}


# ---- stream lengths on the structure of the speculative grid (single Write of n bytes, chunks of L) ----
# body_end = n - 262; chunk j >= 1 is [j L - 261, (j + 1) L - 261) cut at n - 261, so n = j L + 1 makes the last chunk one
# position long and n = j L removes it; window end k fires at 65536 + 32768 k - 261, the first position of a chunk.
GRID_D = (-262, -261, -260, -1, 0, 1, 260, 261, 262, 263)
GRID_B = {2048: (35, 51, 70), 1024: (71, 101, 141), 512: (143, 203, 287)}      # j L in 70-145 KB
GRID_B_BIG = {1024: (1024, 1025, 1027), 512: (2049, 2051)}                      # j L from 1 MiB on


def family_a(ks):
    """a window end one byte either side of the stream's end, of the body's end, of the last chunk's"""
    return sorted({65536 + 32768 * k + d for k in ks for d in GRID_D if 65536 + 32768 * k + d >= 65536})


def family_b(js):
    """the last chunk absent, one position long, two positions long"""
    return sorted({j * L + d for L, jl in js.items() for j in jl for d in (0, 1, 2)})


def grid_lengths(big=False):
    return sorted(set(family_a((31, 32, 33)) + family_b(GRID_B_BIG))) if big else sorted(set(family_a((0, 1, 2, 3)) + family_b(GRID_B)))


def alice_of(n):
    """alice29.txt as committed, repeated and cut to n bytes (the repeat distance is far beyond the window)"""
    d = open(os.path.join(CORPUS, "alice29.txt"), "rb").read()
    return (d * (n // len(d) + 1))[:n]


def _all(jobs, fn=None):
    with ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0))))) as pool:
        return [f.result() for f in [pool.submit(fn or _run, *j) for j in jobs]]


def test_corpus_at_every_chunk_length(exe):
    """The 11 corpus files at levels 4, 6, 9, chunks of 512 / 1024 / 2048: whatever path a stream takes, what the model
    emits on the speculative one is the oracle's.  Text takes it."""
    names = sorted(os.listdir(CORPUS))
    assert len(names) == 11
    # (all 33: ptt5 at level 9 -- chains of 4096 through runs of zeros -- is the model's slowest case, ~20 s of one core)
    jobs = [(exe, os.path.join(CORPUS, n), lvl) for n in names for lvl in (4, 6, 9)]
    res = dict(zip([(j[1], j[2]) for j in jobs], _all(jobs)))
    for n in ("alice29.txt", "asyoulik.txt", "plrabn12.txt"):
        assert res[(os.path.join(CORPUS, n), 6)][1024] == "spec", res[(os.path.join(CORPUS, n), 6)]
    for lvl in (4, 6, 9):
        assert set(res[(os.path.join(CORPUS, "ptt5"), lvl)].values()) == {"maps"}, res[(os.path.join(CORPUS, "ptt5"), lvl)]


def test_periodic_data_and_window_ends(exe, tmp_path):
    """Zeros, runs and image rows never verify (and their equal-bucket reads bail); sizes around the window ends -- 65 274 +- 2,
    multiples of 32 768 and 261 either side of them -- put a read event at every place of a chunk's head."""
    rng = np.random.default_rng(7)
    alice = open(os.path.join(CORPUS, "alice29.txt"), "rb").read() * 2
    files = {}

    def put(name, b):
        (tmp_path / name).write_bytes(b)
        files[name] = str(tmp_path / name)
    put("zeros", bytes(200000))
    put("runs", np.repeat(rng.integers(0, 4, 30000, dtype=np.uint8), rng.integers(1, 40, 30000))[:200000].tobytes())
    y, x = np.mgrid[0:512, 0:512]
    img = np.zeros((512, 512, 4), np.uint8)
    img[..., 0] = (4 * x + y) % 256
    img[..., 3] = 255
    put("sparse512", img.tobytes())
    sizes = [65274 + d for d in (-2, -1, 0, 1, 2)]
    for k in (2, 3, 5):
        sizes += [32768 * k + d for d in (-261, -1, 0, 1, 261)]
    for n in sizes:
        put("alice_%d" % n, alice[:n])
    jobs = [(exe, p, lvl) for p in files.values() for lvl in (4, 6, 9)]
    res = dict(zip([(j[1], j[2]) for j in jobs], _all(jobs)))
    for name in ("zeros", "runs", "sparse512"):
        assert all(v == "maps" for v in res[(files[name], 6)].values()), (name, res[(files[name], 6)])
    assert all(v == "spec" for v in res[(files["alice_%d" % (32768 * 5)], 6)].values())


def test_filtered_warmups_and_a_spoiled_guess(exe):
    """CompressionStrategy.Filtered, warm-ups of 64 and 256, and a guess spoiled on purpose: the verification sends the stream
    to the maps."""
    p = os.path.join(CORPUS, "lcet10.txt")
    assert set(_run(exe, p, 6, 1).values()) <= {"spec", "maps"}
    assert _run(exe, p, 6, 0, LENS, 256) == {512: "spec", 1024: "spec", 2048: "spec"}
    _run(exe, p, 6, 0, LENS, 64)
    assert _run(exe, p, 6, 0, LENS, 128, corrupt=7) == {512: "maps", 1024: "maps", 2048: "maps"}
    # (chunk 0's recorded entry is checked against the initial state: the walk that emits starts from the record)
    assert run_model(exe, p, 6, 0, LENS, 128, corrupt=0) == {n: {"path": "maps", "wrong": 1, "bail": 0} for n in (512, 1024, 2048)}


def test_lengths_on_the_speculative_grid(exe, tmp_path):
    """Window ends one byte from the stream's end and last chunks of zero, one and two positions (grid_lengths), levels 6 and 9,
    chunks of 512 / 1024 / 2048: every stream verifies and is the oracle's -- the expectation tests/test_gpu_spec.py holds the
    device to (there with ZS_SPEC_MIN=65536)."""
    jobs = []
    for n in grid_lengths():
        (tmp_path / ("alice_%d" % n)).write_bytes(alice_of(n))
        jobs += [(exe, str(tmp_path / ("alice_%d" % n)), lvl) for lvl in (6, 9)]
    assert len(jobs) == 2 * 63
    res = _all(jobs)
    notspec = [(os.path.basename(j[1]), j[2], r) for j, r in zip(jobs, res) if r != {512: "spec", 1024: "spec", 2048: "spec"}]
    assert not notspec, notspec
