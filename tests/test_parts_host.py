"""The rules that the container calls share (zlibstream_amd/csrc/zs_parts.h), run on the host by tests/cpp/test_parts.cpp under
AddressSanitizer and UBSan.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_shared_rules_of_the_container_calls():
    """The staging layout puts every item at a multiple of 256 behind the one before it, and an empty or over-limit item takes
    no room.  The 16-byte split gives back the position for every remainder and both header skips.  The zlib header check agrees
    with a restatement of its five branches on all 65 536 headers and on lengths 0 and 1.  The verdict on an inflated sub-stream
    agrees with the branches the ZIP, TIFF and OpenEXR calls had, for every status, message, length and trailer relation under
    each length rule.  The roll-up gives the earlier code's statuses, part codes and messages for both pairs of nouns.  The
    encode side marks what does not fit and leaves failed outputs alone."""
    exe = os.path.join(ROOT, "build", "test_parts")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_parts.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), r.stdout[-3000:] + r.stderr[-3000:]
