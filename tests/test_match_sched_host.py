"""The schedule of the match kernel's walk (zlibstream_amd/csrc/zs_kernels.hip, match_walk) as a 64-lane host model, run by
tests/cpp/test_match_sched.cpp under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess

from zlibstream_amd import datagen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_both_compare_widths_give_the_plain_walks_records_and_end():
    """With a first compare of 8 and of 16 bytes: every position's records for budgets K and K >> 2 equal walk_matches over
    links built as K1 defines them (multiplicative hash), at levels 4, 6 and 9, and the loop ends -- on word soup, on copies
    of exactly 3 .. 300 bytes, on periodic bytes, zeros, a run inside text, a four-letter alphabet, on 256 KiB of the
    benchmark's text and on tests/golden/corpus/alice29.txt.  For the text inputs the per-position counts of the kernel's blocks
    are printed; the 16-byte compare must never run more extension rounds, and must at least halve them on the benchmark's text.  (profiles/match_cmp16.md has the counts for
    2 MiB of the benchmark's text: the same program, built with -O2, on datagen.english(2 << 20).)"""
    exe = os.path.join(ROOT, "build", "test_match_sched")
    text = os.path.join(ROOT, "build", "match_sched_english.bin")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    with open(text, "wb") as f:
        f.write(datagen.english(256 * 1024, 17))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_match_sched.cpp")], check=True)
    r = subprocess.run([exe, text, os.path.join(ROOT, "tests", "golden", "corpus", "alice29.txt")], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), r.stdout[-2000:] + r.stderr[-2000:]
