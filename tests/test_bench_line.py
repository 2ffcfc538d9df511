"""bench.py's one stdout line must stay parsable by the driver: round 4's 21.7 KB line came back as `parsed: null`.
The line builder is run on canned numbers (round 4's full report, a leg added on top) -- no GPU, no engine call; one -m gpu
test runs a plain benchmark end to end."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("zs_bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _canned():
    return json.load(open(os.path.join(ROOT, "profiles", "r04_bench_final_build.json")))


def test_line_is_short_and_round_trips():
    m = _bench()
    full = _canned()
    assert len(json.dumps(full)) > 20000  # the report that broke the driver's parser
    # more legs than any run has: the line's size must not follow the report's
    for i in range(40):
        full["secondary"]["extra_leg_%d" % i] = dict(full["secondary"]["english64_L1"])
    text = m.compact_line(full)
    assert len(text) < 4096 and "\n" not in text
    line = json.loads(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["value"] == full["value"] and line["config"]["workload"].startswith("english64")
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in line["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in line["cpu_baseline"], k
    legs = line["secondary_summary"]["legs"]
    assert legs["english64_L1"] == [1375.01, 0.000262, 73.05]
    assert legs["inflate1g"][0] == full["secondary"]["inflate1g"]["value"]
    assert "secondary" not in line


def test_emit_report_prints_the_compact_line_last(tmp_path, capsys, monkeypatch):
    m = _bench()
    monkeypatch.setattr(m, "ROOT", str(tmp_path))
    m.emit_report(_canned())
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and len(out[0]) < 4096
    assert json.loads(out[0])["secondary_summary"]["full_report"] == "bench_secondary.json"
    full = json.load(open(tmp_path / "bench_secondary.json"))
    assert "corpus_L6" in full["secondary"] and "files" in full["secondary"]["corpus_L6"]


def test_traffic_names_its_source():
    m = _bench()
    b, src = m.pmc_traffic("zs_match_kernel", "traffic_english64_L6")
    assert b and src.startswith("profiles/") and src.endswith("pmc_traffic_english64_L6.json")
    r = m.roofline({"match": 2.7, "links": 0.3}, 94534690, b, None, src)
    assert r["traffic_source"] == src and r["scope"] == "kernel"
    r = m.roofline_with_pmc({"match": 2.7, "links": 0.3}, 94534690, "traffic_english64_L6")
    assert r["kernel"] == "zs_match_kernel" and r["traffic_source"] == src and r["traffic"] == b
    # the rounds of the chunk form are a stage of many launches, and say so
    b, src = m.pmc_traffic("zs_fast_sweep_kernel", "fast64_L1")
    r = m.roofline({"fast_sweep": 46.6, "links": 0.3}, 97620422, b, None, src)
    assert r["scope"] == "stage" and r["launches"] and r["traffic"] > 97620422 and r["traffic_source"] == src


def test_dump_outputs_writes_the_streams_as_floats(tmp_path):
    """--dump-outputs on a stand-in batch (zlib streams in host tensors, room behind each as the device buffers have): lengths,
    CRC-32s and, below DUMP_BYTES, every byte of the streams laid end to end; above it a seeded sample that is the same each time."""
    import zlib
    import numpy as np
    import torch
    m = _bench()
    datas = [bytes(range(256)) * 40, b"abc" * 50000, b""]
    zs = [zlib.compress(d, 6) for d in datas]

    class Batch:
        out_lens = [len(z) for z in zs]
        d_outs = [torch.frombuffer(bytearray(z + b"\xee" * 64), dtype=torch.uint8) for z in zs]

    m.dump_outputs(str(tmp_path / "a"), Batch)
    got = {f: np.load(tmp_path / "a" / (f + ".npy")) for f in ("stream_lengths", "stream_crc32", "stream_bytes", "stream_byte_positions")}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert got["stream_lengths"].tolist() == [len(z) for z in zs]
    assert got["stream_crc32"].tolist() == [zlib.crc32(z) for z in zs]
    flat = b"".join(zs)
    assert got["stream_bytes"].tolist() == list(flat) and got["stream_byte_positions"].tolist() == list(range(len(flat)))
    m.DUMP_BYTES = 100
    for d in ("b", "c"):
        m.dump_outputs(str(tmp_path / d), Batch)
    pos = np.load(tmp_path / "b" / "stream_byte_positions.npy")
    assert len(pos) == 100 and np.array_equal(pos, np.load(tmp_path / "c" / "stream_byte_positions.npy"))
    assert np.load(tmp_path / "b" / "stream_bytes.npy").tolist() == [flat[int(p)] for p in pos]


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_what_they_computed(tmp_path):
    """A plain `bench.py` run (no --full) in its own process: the line has the contract's keys and none of the --full legs, and the
    streams it dumps inflate to the seeded input it timed."""
    import subprocess
    import sys
    import zlib
    import numpy as np
    from zlibstream_amd import datagen
    size = 1 << 20
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--size", str(size), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in line, k
    assert not {"cpu_baseline", "bit_identical_to_cpu", "secondary_summary"} & set(line)
    lens = np.load(tmp_path / "stream_lengths.npy")
    z = np.load(tmp_path / "stream_bytes.npy").astype(np.uint8).tobytes()
    assert lens.tolist() == [len(z)] == [line["config"]["compressed_bytes"]]
    assert np.load(tmp_path / "stream_crc32.npy").tolist() == [zlib.crc32(z)]
    assert zlib.decompress(z) == datagen.english(size, datagen.GOLDEN & datagen.MASK)
