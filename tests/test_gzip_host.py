"""The host side of the container calls, no GPU: the gzip header rules of zlibstream_amd/csrc/zs_gzip.h run by
tests/cpp/test_gzip_header.cpp, zs_wrap_bound for the three containers, and zs_gzip_file_info's walk."""
import gzip
import os
import random
import struct
import subprocess
import zlib

import pytest

import gzip_cases as gz
from zlibstream_amd import (WRAP_GZIP, WRAP_RAW, WRAP_ZLIB, ZlibStreamException, deflate_bound, gzip_file_info, wrap_bound)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shared_gzip_header_code_on_the_host():
    """Every FLG combination whole and cut at every byte, both sides of every error class, FEXTRA with and without the BGZF
    subfield, names of 0, 1 and 300 bytes and one with no terminator, the encoder's ten bytes (tests/cpp/test_gzip_header.cpp).
    The parser is given exactly the bytes it may read, in a buffer of their own."""
    exe = os.path.join(ROOT, "build", "test_gzip_header")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_gzip_header.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), (r.stdout[-2000:], r.stderr[-2000:])


def test_wrap_bound_for_the_three_containers():
    for n in (0, 1, 300, 65537, 1 << 20, (1 << 31) - 2048):
        assert wrap_bound(n, WRAP_ZLIB) == deflate_bound(n)
        assert wrap_bound(n, WRAP_RAW) == deflate_bound(n) - 6
        assert wrap_bound(n, WRAP_GZIP) == deflate_bound(n) + 12
    for bad in ((-1, WRAP_ZLIB), (10, -1), (10, 3)):
        with pytest.raises(ValueError):
            wrap_bound(*bad)


def test_file_info_of_a_plain_file_of_three_members():
    parts = [b"first member " * 40, b"", bytes(range(256)) * 9]
    f = (gz.member(parts[0], flg=gz.FNAME, name=b"one.txt", mtime=1234567, xfl=2, os_=3) + gz.member(parts[1]) +
         gz.member(parts[2], flg=gz.FNAME | gz.FHCRC, name=b"three"))
    assert gzip.decompress(f) == b"".join(parts)  # (the file is what gzip reads)
    assert gzip_file_info(f) == {"bgzf": 0, "xfl": 2, "os": 3, "mtime": 1234567, "n_members": -1, "name_off": 10, "name_len": 7, "isize_sum": -1}
    assert f[10:17] == b"one.txt"
    # the first header decides: every cut of it, and each of its error classes
    head = gz.header(gz.FNAME, name=b"one.txt")
    for cut in range(len(head)):
        with pytest.raises(ZlibStreamException, match=r"\(-5\)"):
            gzip_file_info(f[:cut])
    assert gzip_file_info(f[:len(head)])["name_len"] == 7
    for at, val in ((0, 0x1E), (1, 0x8A), (2, 9), (3, 0x28)):
        b = bytearray(f)
        b[at] = val
        with pytest.raises(ZlibStreamException, match=r"\(-3\)"):
            gzip_file_info(b)
    assert gzip_file_info(gz.member(b"x"))["name_off"] == 0


def test_file_info_of_a_bgzf_file():
    rnd = random.Random(5)
    blocks = [bytes(rnd.choice(b"ACGTN") for _ in range(n)) for n in (100, 7000, 60000, 1, 33333)]
    f = gz.bgzf_file(blocks)
    assert gzip.decompress(f) == b"".join(blocks)
    want = {"bgzf": 1, "xfl": 0, "os": 255, "mtime": 0, "n_members": 6, "name_off": 0, "name_len": 0, "isize_sum": sum(map(len, blocks))}
    assert gzip_file_info(f) == want
    assert gzip_file_info(f + b"\0" * 9) == want  # zero padding behind the end-of-file block
    # a BSIZE that points past the end: the third block's size one more than it is, then the file cut inside the last block
    sizes = [len(gz.bgzf_block(b)) for b in blocks]
    assert struct.unpack_from("<H", f, 16)[0] == sizes[0] - 1
    with pytest.raises(ZlibStreamException, match=r"\(-5\)"):
        gzip_file_info(f[:len(f) - 1])
    with pytest.raises(ZlibStreamException, match=r"\(-5\)"):
        gzip_file_info(f[:sum(sizes[:2]) + 30])
    last = sum(sizes)  # the end-of-file block: 28 bytes, alone at the end
    b = bytearray(f)
    struct.pack_into("<H", b, last + 16, 28)  # BSIZE 28: a block of 29 bytes
    with pytest.raises(ZlibStreamException, match=r"\(-5\)"):
        gzip_file_info(b)
    assert gzip_file_info(bytes(b) + b"\0")["n_members"] == 6  # (with the byte there the walk goes by the sizes and closes)
    # a member without the subfield in a BGZF file: the walk cannot go on
    with pytest.raises(ZlibStreamException, match=r"\(-3\)"):
        gzip_file_info(f + gz.member(b"plain"))
    # a first member that only looks like BGZF (SLEN 3) makes a plain file
    odd = gz.header(gz.FEXTRA, extra=struct.pack("<BBH", 66, 67, 3) + b"\1\2\3") + gz.raw_deflate(b"abc") + gz.trailer(b"abc")
    assert gzip_file_info(odd)["bgzf"] == 0 and gzip_file_info(odd)["n_members"] == -1
