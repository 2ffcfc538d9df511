"""Random shapes, each called two to four times in a row on one context with other bytes every time: every output against the
oracle, and how many of the repeats took the kept plan (zs_ctx_counter "plan_reused").  tools/fuzz_batch.py never repeats a
shape in consecutive calls, so it never reuses a plan; this does nothing else.   python tools/fuzz_plan_reuse.py [seconds] [seed]"""
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import oracle_binding
from zlibstream_amd import Engine, datagen, deflate_bound

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = random.Random(seed)
O = oracle_binding.Oracle()
POOL = datagen.english(3 << 20, 4242 + seed)
ROWS = datagen.sparse(256, 2048)


def buffer(kind, n):
    if kind == "text":
        at = rng.randrange(0, len(POOL) - n)
        return POOL[at:at + n]
    if kind == "rows":
        at = rng.randrange(0, len(ROWS) - n)
        return ROWS[at:at + n]
    if kind == "random":
        return np.random.default_rng(rng.randrange(1 << 30)).integers(0, 256, n, dtype=np.uint8).tobytes()
    return bytes([rng.randrange(256)]) * n


def main():
    eng = Engine(0)
    t0 = time.time()
    cases = calls = repeats = reused = failures = 0
    while time.time() - t0 < budget:
        n = rng.choice([1, 1, 1, 2, 3, 5, 17, 70])
        level = rng.choice([1, 2, 3, 4, 5, 6, 6, 6, 7, 8, 9])
        strategy = rng.choice([0, 0, 0, 1, 2, 3])
        top = rng.choice([300, 5000, 70000, 70000, 300000, 1100000]) if n <= 5 else rng.choice([300, 5000, 40000])
        lens = [rng.randrange(max(1, top // 2), top + 1) for _ in range(n)]
        kinds = [rng.choice(["text", "text", "rows", "random", "byte"]) for _ in range(n)]
        ends = None
        if rng.random() < 0.25:
            ends = []
            for ln in lens:
                if rng.random() < 0.5 or ln < 8:
                    ends.append(None)
                    continue
                cuts = sorted(rng.sample(range(1, ln), min(ln - 1, rng.choice([1, 2, 5]))))
                ends.append(cuts + [ln])
        caps = [deflate_bound(ln) for ln in lens]
        for rep in range(rng.choice([2, 2, 3, 4])):
            datas = [buffer(k, ln) for k, ln in zip(kinds, lens)]
            off = rng.choice([0, 0, 1, 3])
            d_in = [torch.frombuffer(bytearray(off) + bytearray(d) + bytearray(64), dtype=torch.uint8).cuda() for d in datas]
            d_out = [torch.full((c + 64,), 0xEE, dtype=torch.uint8, device="cuda") for c in caps]
            torch.cuda.synchronize()
            got = eng.deflate_writes_batch_device([t.data_ptr() + off for t in d_in], lens, ends, [t.data_ptr() for t in d_out], caps, level=level,
                                                  strategy=strategy)
            calls += 1
            if rep:
                repeats += 1
                reused += eng.counter("plan_reused") == 1
            for i, d in enumerate(datas):
                sizes = None
                if ends and ends[i] and len(ends[i]) > 1:
                    sizes = [e - s for s, e in zip([0] + ends[i][:-1], ends[i])]
                if bytes(d_out[i][:got[i]].cpu().numpy()) != O.compress(d, level, strategy, chunks=sizes):
                    failures += 1
                    print("FAIL: seed %d case %d repeat %d stream %d: n %d level %d strategy %d lens %r kinds %r ends %r reused %d" %
                          (seed, cases, rep, i, n, level, strategy, lens, kinds, ends, eng.counter("plan_reused")), flush=True)
        cases += 1
        if cases % 50 == 0:
            print("... %d shapes, %d calls, %d failures, %.0f s" % (cases, calls, failures, time.time() - t0), flush=True)
    print("fuzz_plan_reuse: %d shapes from seed %d, %d calls, %d of %d repeats took the kept plan, %d failures, %.0f s" %
          (cases, seed, calls, reused, repeats, failures, time.time() - t0))
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
