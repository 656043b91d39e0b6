"""In-kernel phase stamps of the loss stage inside the C2 train step (a library built with -DSDUMC_LOSS_DBG=1 on loss.hip, loaded
through SDUMC_LIB): thread 0 of workgroup 0 of loss_stage1_kernel (rnc_row_body, slots 0-5) and of loss_stage2_kernel (rnc_dfeat_body,
slots 8-11) on the 100 MHz wall clock, averaged over the steps.  usage: SDUMC_LIB=<dbg build> python tools/loss_stamps.py [--bf16]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from sdumc_amd import engine, _lib

if not hasattr(_lib.lib, "sdumc_loss_stamps_"):
    sys.exit("this library was built without -DSDUMC_LOSS_DBG=1")
bf16 = "--bf16" in sys.argv
dev = torch.device("cuda:0")
flat, lay = bench.init_flat_params(engine, dev)
batches = [[t.to(dev) for t in bench.synthetic_shard(bench.B_PER_GPU, 0, k=k)] for k in range(bench.N_RESIDENT)]
step, run = bench.resident_step(engine, flat, batches, bf16=bf16)
for _ in range(12):
    run()
torch.cuda.synchronize()
N = 40
names = {1: "anchor row in LDS", 2: "distances", 3: "exp", 4: "row loss", 5: "G written", 9: "coef in LDS", 10: "column sums", 11: "df written"}
acc = {k: [] for k in names}
gap = []
for _ in range(N):
    run()
    torch.cuda.synchronize()
    t = (C.c_ulonglong * 16)()
    assert _lib.lib.sdumc_loss_stamps_(t) == 0
    for k in names:
        base = t[0] if k < 8 else t[8]
        acc[k].append((t[k] - base) * 0.01)
    gap.append((t[8] - t[5]) * 0.01)
for k, nm in names.items():
    v = sorted(acc[k])
    print(f"stage {1 if k < 8 else 2}  {0 if k < 8 else 8} -> {k:2d}  median {v[len(v) // 2]:6.2f} us  min {v[0]:6.2f}  max {v[-1]:6.2f}   {nm}")
v = sorted(gap)
print(f"stage 1 slot 5 -> stage 2 slot 8 (launch boundary, workgroup 0)  median {v[len(v) // 2]:6.2f} us")
