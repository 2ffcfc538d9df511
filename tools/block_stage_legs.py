"""The legs that the block back end (K7-K9) must not make slower, one process per call, one JSON line: sparse64 at levels 6 and
9, batch1024_L6, corpus_L6, fast512_L1 -- bench.py's own legs, through bench.py's own DeviceBatch -- a batch of 4096 x 32 KiB of
text at level 6 (a block list of 16 Ki entries, a quarter of them live), and one 64 KiB stream (tools/small_trace.py's floor).
ZS_DEV=1 ZS_LIB=<path> selects another build of the library, as for the other A/B tools.

    python tools/block_stage_legs.py [steps] [cache dir] [legs, comma-separated: all of them without]

The inputs take longer to make than to compress; with a cache directory the first process leaves them there for the next."""
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench
from zlibstream_amd import Engine, datagen

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
cache = (sys.argv[2] or None) if len(sys.argv) > 2 else None
only = set(sys.argv[3].split(",")) if len(sys.argv) > 3 else None


def want(name):
    return only is None or name in only


def cached(name, make):
    if cache is None:
        return make()
    path = os.path.join(cache, name + ".pickle")
    if os.path.exists(path):
        with open(path, "rb") as f:
            return pickle.load(f)
    data = make()
    os.makedirs(cache, exist_ok=True)
    with open(path + ".tmp", "wb") as f:
        pickle.dump(data, f, protocol=4)
    os.replace(path + ".tmp", path)
    return data


def leg(eng, dev, name, datas, level, n_steps, every=1):
    res, b = bench.secondary_deflate(eng, dev, name, datas, level, n_steps, check_every=every)
    del b
    torch.cuda.empty_cache()
    return {"ms_per_step": res["ms_per_step"], "MBps": res["value"], "stage_ms": {k: v for k, v in res["stage_ms"].items() if k in ("trees", "offsets", "emit_bits")}}


def main():
    dev = torch.device("cuda:0")
    eng = Engine(0)
    out = {"lib": os.environ.get("ZS_LIB") if os.environ.get("ZS_DEV") == "1" else "product", "steps": steps}
    if want("sparse64"):
        sp = datagen.sparse(4096, 4096)
        for lvl in (6, 9):
            out["sparse64_L%d" % lvl] = leg(eng, dev, "sparse64", [sp], lvl, steps)
        del sp
    if want("corpus"):
        res = bench.secondary_corpus(eng, dev, 6, steps, with_cpu=False)
        out["corpus_L6"] = {"ms_per_step": res["ms_per_step"], "MBps": res["value"], "stage_ms": {k: v for k, v in res["stage_ms"].items() if k in ("trees", "offsets", "emit_bits")}}
    if want("small"):
        out["text64KiB_L6"] = leg(eng, dev, "64 KiB", [datagen.english(65536, 9)], 6, 20)
    if not want("batches"):
        print(json.dumps(out), flush=True)
        return
    bufs = cached("batch1024", lambda: [datagen.batch_buffer(i, bench.BATCH_BYTES) for i in range(bench.BATCH_BUFFERS)])
    out["batch1024_L6"] = leg(eng, dev, "batch1024", bufs, 6, steps, every=256)
    del bufs
    texts = cached("fast512", lambda: [datagen.english(512 << 10, 1000 + i) for i in range(512)])
    out["fast512_L1"] = leg(eng, dev, "fast512", texts, 1, steps, every=128)
    small = [t[32768 * k:32768 * (k + 1)] for t in texts[:256] for k in range(16)]
    del texts
    out["batch4096x32KiB_L6"] = leg(eng, dev, "4096 x 32 KiB", small, 6, steps, every=1024)
    del small
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
