"""The composing of an animated PNG's frames, the part that needs no GPU: the code the kernel compiles (zs_png.h
png_blend_over, png_compose_dispose, png_compose_group) run on the host against a restatement of the APNG specification's
rules (tests/cpp/test_png_compose.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blend_dispose_and_the_group_model_match_the_rules_restated():
    """OVER at RGBA8 on every (fa, ba) pair with six colour pairs, at RGBA16 on the edge values 0, 1, 257, 32767, 32768, 65534,
    65535 in every place and 400 000 random pixels; the dispose function on every (op, first frame or not) pair; random
    animations of 1, 2, 3 and 9 frames on canvases from 1x1 to 261x2, regions anywhere, touching the right and bottom edges
    or the whole canvas, all dispose-blend pairs, the output at every legal residue modulo 16, three PREVIOUS frames in a
    row and PREVIOUS on frame 0, against a frame-by-frame restatement on a full canvas; guard bytes around every output."""
    exe = os.path.join(ROOT, "build", "test_png_compose")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_png_compose.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), r.stdout[-2000:]
