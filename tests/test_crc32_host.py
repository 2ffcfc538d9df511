"""The CRC-32 code that the kernels and the host share (zlibstream_amd/csrc/zs_crc32.h), run on the host by
tests/cpp/test_crc32.cpp.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shared_crc32_code_on_the_host():
    """0xCBF43926 for "123456789"; the byte step, the table form and the slice tables against a bit-at-a-time loop on random
    buffers of every length 0..300; combine(crc(a), crc(b), |b|) == crc(a ++ b) for random splits, empty halves and |b| up to
    2^31; the tile algebra of the kernel in both forms with the kernel's tables, every head 0..15; the chunk walk's verdicts."""
    exe = os.path.join(ROOT, "build", "test_crc32")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_crc32.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), r.stdout[-2000:]
