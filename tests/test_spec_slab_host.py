"""The pure parts of the speculative walk's provisional symbols (zlibstream_amd/csrc/zs_core.h), run on the host by
tests/cpp/test_spec_slab.cpp.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slab_stride_cut_index_and_positions_on_the_host():
    """The slab stride against the most symbols a chunk of 512, 1024 and 2048 positions emits (reached by a chunk of
    literals); the cut index against a plain loop -- the cut at index 0, at the last index, none, base + count exactly on a
    multiple of kBlockSyms, and at random; a symbol's end and loop-top from the chunk's entry and the lengths in front of it,
    against what the shared chunk walk tells a sink, read events and the odd loop-top at the slide threshold included."""
    exe = os.path.join(ROOT, "build", "test_spec_slab")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_spec_slab.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), r.stdout[-2000:]
