"""gzip members and files built from zlib's raw deflate and struct, for tests/test_gzip_host.py and tests/test_gpu_wrap.py:
the container is written here byte by byte, so that what the library reads is not what another gzip writer chose to write."""
import struct
import zlib

FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return c.compress(data) + c.flush()


def header(flg=0, extra=b"", name=b"", comment=b"", mtime=0, xfl=0, os_=255):
    h = struct.pack("<BBBBIBB", 0x1F, 0x8B, 8, flg, mtime, xfl, os_)
    if flg & FEXTRA:
        h += struct.pack("<H", len(extra)) + extra
    if flg & FNAME:
        h += name + b"\0"
    if flg & FCOMMENT:
        h += comment + b"\0"
    if flg & FHCRC:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h


def trailer(data):
    return struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def member(data, body=None, **kw):
    """One member around `data`; body: its raw deflate stream, made at level 6 when not given."""
    return header(**kw) + (raw_deflate(data) if body is None else body) + trailer(data)


def bgzf_block(data, level=6, isize=None, bsize=None):
    """One BGZF block (SAM/BAM specification 4.1): FEXTRA with the subfield 'B' 'C', SLEN 2, BSIZE = the block's size - 1."""
    body = raw_deflate(data, level)
    total = 12 + 6 + len(body) + 8
    extra = struct.pack("<BBHH", 66, 67, 2, (total - 1) if bsize is None else bsize)
    return header(FEXTRA, extra=extra) + body + struct.pack("<II", zlib.crc32(data), len(data) if isize is None else isize)


def bgzf_file(blocks, level=6):
    """The blocks and the empty end-of-file block behind them."""
    return b"".join(bgzf_block(b, level) for b in blocks) + bgzf_block(b"")
