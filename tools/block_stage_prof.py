"""K7's and K9's phases by their wall clocks: one level-6 call each on english64 and sparse64 with a library built with
-DZS_BS_PROF (zs_trees_kernel and zs_emit_bits_kernel then print the ticks of every 256th block, lane 0 of each wave that
counts).  The timers are compiled out of the product.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 -shared -fPIC -fvisibility=hidden -DZS_BS_PROF \
          -o build/variants/zs_bsprof.so zlibstream_amd/csrc/zs_engine.hip
    ZS_DEV=1 ZS_LIB=build/variants/zs_bsprof.so python tools/block_stage_prof.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from zlibstream_amd import Engine, datagen, deflate_bound

eng = Engine(0)
for name, data in (("english64", datagen.english(64 << 20)), ("sparse64", datagen.sparse(4096, 4096))):
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cap = deflate_bound(len(data))
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    print("BSPROF ---- %s, level 6" % name, flush=True)
    eng.deflate_batch_device([d_in.data_ptr()], [len(data)], [d_out.data_ptr()], [cap], level=6)
    torch.cuda.synchronize()
