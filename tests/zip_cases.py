"""ZIP archives built from struct and zlib's raw deflate, for tests/test_zip_host.py and tests/test_gpu_zip.py: every record is
written here field by field, so that a bad case differs from a legal neighbour by the one field the test names, and what the
library reads is not only what zipfile chose to write.  legal() holds an archive against zipfile itself."""
import io
import struct
import zipfile
import zlib

STORED, DEFLATED = 0, 8
ENCRYPTED, DESCRIPTOR, UTF8 = 1, 8, 0x800


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def local(name, comp_len, size, crc, method=DEFLATED, flags=0, extra=b"", version=20, time=0, date=0x21, sig=b"PK\3\4", name_len=None,
          extra_len=None):
    return sig + struct.pack("<HHHHHIIIHH", version, flags, method, time, date, crc, comp_len, size, len(name) if name_len is None else name_len,
                             len(extra) if extra_len is None else extra_len) + name + extra


def central(name, comp_len, size, crc, local_off, method=DEFLATED, flags=0, extra=b"", comment=b"", version=20, made_by=20, time=0, date=0x21,
            disk=0, internal_attr=0, external_attr=0, sig=b"PK\1\2", name_len=None, extra_len=None, comment_len=None):
    return sig + struct.pack("<HHHHHHIIIHHHHHII", made_by, version, flags, method, time, date, crc, comp_len, size,
                             len(name) if name_len is None else name_len, len(extra) if extra_len is None else extra_len,
                             len(comment) if comment_len is None else comment_len, disk, internal_attr, external_attr, local_off) + name + extra + comment


def eocd(n, cd_len, cd_off, comment=b"", disk=0, cd_disk=0, n_here=None, comment_len=None, sig=b"PK\5\6"):
    return sig + struct.pack("<HHHHIIH", disk, cd_disk, n if n_here is None else n_here, n, cd_len, cd_off,
                             len(comment) if comment_len is None else comment_len) + comment


def eocd64(n, cd_len, cd_off, at, disk=0, cd_disk=0, n_here=None, n_disks=1, loc_disk=0, sig=b"PK\6\6", loc_sig=b"PK\6\7", size=44):
    """The ZIP64 end record and its locator; `at`: where the record lies in the archive (what the locator says)."""
    return (sig + struct.pack("<QHHIIQQQQ", size, 45, 45, disk, cd_disk, n if n_here is None else n_here, n, cd_len, cd_off) +
            loc_sig + struct.pack("<IQI", loc_disk, at, n_disks))


def zip64_extra(*values):
    return struct.pack("<HH", 1, 8 * len(values)) + b"".join(struct.pack("<Q", v) for v in values)


def entry(name, data, method=DEFLATED, body=None, level=6, flags=0, local_extra=b"", central_extra=b"", descriptor=False, lo=None, ce=None):
    """One entry of archive(): body is its bytes in the file (made from data by `method` when not given); lo / ce override
    fields of its local header / central record (keyword arguments of local() / central())."""
    if body is None:
        body = raw_deflate(data, level) if method == DEFLATED else data
    return dict(name=name, data=data, method=method, body=body, flags=flags | (DESCRIPTOR if descriptor else 0), local_extra=local_extra,
                central_extra=central_extra, descriptor=descriptor, lo=dict(lo or {}), ce=dict(ce or {}))


def archive(entries, prefix=b"", comment=b"", end64=False, end=None, end64_fields=None, places=None):
    """prefix | per entry [local header, name, extra, body, data descriptor] | central directory | [ZIP64 end record, locator]
    | end record, comment.  The offsets are the archive's own: bytes of `prefix` shift them, as those of a self-extractor do.
    end64: write the ZIP64 end record and saturate the end record's count, length and offset.  end / end64_fields override
    fields of eocd() / eocd64().  places (a dict, may be None) receives local_off, body_off (lists) and cd_off, cd_len, end_off,
    all counted in the returned bytes."""
    out, cd, local_off, body_off = b"", b"", [], []
    for e in entries:
        crc = zlib.crc32(e["data"])
        local_off.append(len(out))
        lo = dict(method=e["method"], flags=e["flags"], extra=e["local_extra"])
        lo.update(e["lo"])
        sizes = (0, 0, 0) if e["descriptor"] else (len(e["body"]), len(e["data"]), crc)
        h = local(e["name"], sizes[0], sizes[1], sizes[2], **lo)
        body_off.append(len(out) + len(h))
        out += h + e["body"]
        if e["descriptor"]:
            out += b"PK\7\x08" + struct.pack("<III", crc, len(e["body"]), len(e["data"]))
        ce = dict(method=e["method"], flags=e["flags"], extra=e["central_extra"])
        ce.update(e["ce"])
        args = dict(comp_len=len(e["body"]), size=len(e["data"]), crc=crc, local_off=local_off[-1])
        for k in list(args):
            if k in ce:
                args[k] = ce.pop(k)
        cd += central(e["name"], **args, **ce)
    cd_off, n = len(out), len(entries)
    out += cd
    if end64:
        out += eocd64(n, len(cd), cd_off, len(out), **(end64_fields or {}))
        tail = eocd(0xFFFF, 0xFFFFFFFF, 0xFFFFFFFF, comment, **(end or {}))
    else:
        tail = eocd(n, len(cd), cd_off, comment, **(end or {}))
    if places is not None:
        k = len(prefix)
        places.update(local_off=[o + k for o in local_off], body_off=[o + k for o in body_off], cd_off=cd_off + k, cd_len=len(cd), end_off=len(out) + k)
    return prefix + out + tail


def legal(arch, entries):
    """The archive is one to zipfile: it opens, every entry's CRC holds, names and contents are the entries'."""
    with zipfile.ZipFile(io.BytesIO(arch)) as z:
        assert z.testzip() is None
        assert [i.filename.encode("utf-8" if i.flag_bits & UTF8 else "cp437") for i in z.infolist()] == [e["name"] for e in entries]
        for i, e in zip(z.infolist(), entries):
            assert z.read(i) == e["data"]
    return arch


def three(middle=None):
    """Three small entries, deflated / stored / deflated: the legal neighbour of the bad cases, whose middle entry they replace."""
    return [entry(b"first.txt", b"the first entry " * 12), middle or entry(b"mid.bin", bytes(range(200)), method=STORED),
            entry(b"dir/last.txt", b"and the last one, " * 9)]
