"""The planner of a deflate call (zlibstream_amd/csrc/zs_plan.h), run on the host by tests/cpp/test_plan.cpp under
AddressSanitizer and UBSan.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_planner_reads_its_key_alone_and_lays_out_what_it_plans():
    """The planner compiles with getenv poisoned: every switch it has comes from the PlanEnv of the key.  On the edge shapes --
    lengths around 262 and 65 536, the walk's threshold, level 0 with and without flushing Writes, Rle with a Write end inside and
    outside the 262 bytes below a window end, level 1 with 81 920-byte and 5-byte Writes, the double plan and its striking, 64 and
    65 streams, a refused speculative grid, resumed runs -- equal arguments at other addresses give the same plan and layout;
    every stream's offsets are the sums of the earlier streams' counts; the work lists and tables have the layout's sizes; bound
    to plain memory and staged there, every descriptor's tables are its own stream's entries.  Every PlanEnv field the planner
    reads changes a named field of a named shape's plan."""
    exe = os.path.join(ROOT, "build", "test_plan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), r.stdout[-3000:] + r.stderr[-3000:]
