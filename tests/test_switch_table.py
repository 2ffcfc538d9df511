"""DESIGN.md's switch table lists exactly the environment variables libzsgpu.so reads: every "ZS_..." literal handed to
getenv or ZS_ENV_FLAG under zlibstream_amd/csrc/ is in the table, and the table names nothing else.  Files only: no build,
no device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zlibstream_amd", "csrc")
TABLE_TITLE = "### Switches of the tests and the measurements"


def variables_read():
    found = set()
    for name in sorted(os.listdir(CSRC)):
        src = open(os.path.join(CSRC, name), encoding="utf-8").read()
        found.update(re.findall(r'\bgetenv\(\s*"(ZS_[A-Z0-9_]+)"', src))
        found.update(re.findall(r'\bZS_ENV_FLAG\(\s*\w+\s*,\s*"(ZS_[A-Z0-9_]+)"', src))
    return found


def variables_in_table():
    lines = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read().split("\n")
    at = next(i for i, l in enumerate(lines) if l.startswith(TABLE_TITLE))
    head = next(i for i in range(at, len(lines)) if lines[i].startswith("| variable |"))
    assert lines[head + 1].startswith("|---"), lines[head + 1]
    found, rows = set(), 0
    for l in lines[head + 2:]:
        if not l.startswith("|"):
            break
        rows += 1
        found.update(re.findall(r"\bZS_[A-Z0-9_]+", l))
    assert rows > 0
    return found


def test_the_switch_table_lists_what_the_library_reads():
    read, table = variables_read(), variables_in_table()
    assert len(read) > 40, sorted(read)  # (the scan found the sources)
    print("read by the library, not in the table:", sorted(read - table))
    print("in the table, not read by the library:", sorted(table - read))
    assert read == table
