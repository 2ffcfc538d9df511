"""The shape key of a deflate call (zlibstream_amd/csrc/zs_plan_key.h), run on the host by tests/cpp/test_plan_key.cpp under
AddressSanitizer and UBSan.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_equal_arguments_equal_keys_and_every_field_counts():
    """Two keys built from the same arguments are equal; a change of any single field -- stream count, level, strategy, hash
    variant, any length or capacity, the presence of a Write list, a Write end, the number of Writes, a flush mode, chunk, raw,
    each environment switch -- makes them unequal; a key of a path that is never reused (a batch run again, an incremental
    run, the cut rounds' re-entry, forced literal streams, a call barred from the rounds) equals no key, itself included."""
    exe = os.path.join(ROOT, "build", "test_plan_key")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_plan_key.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), r.stdout[-2000:] + r.stderr[-2000:]
