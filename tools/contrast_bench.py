#!/usr/bin/env python
"""ms/step of the fused step per contrastive criterion (rnc | supcon), driven as bench.py drives its headline:
one TrainStep over an arena of resident batches, `steps` launches timed from the host after `warmup`, the criteria
alternated `--rounds` times so that clock drift hits all of them alike.  One JSON line.

    python tools/contrast_bench.py [--steps 200] [--warmup 20] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import bench
from sdumc_amd import engine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    flat0, _ = bench.init_flat_params(engine, dev)
    batches = [[t.to(dev) for t in bench.synthetic_shard(bench.B_PER_GPU, 0, k=k)] for k in range(bench.N_RESIDENT)]
    K = len(batches)
    runs = {}
    for crit in ("rnc", "supcon"):
        flat = flat0.clone()
        arena = engine.StepArena(flat, bench.B_PER_GPU, bench.T_MOSEI, bench.DIMS, sets=K, planes=True)
        ts = engine.TrainStep(flat, bench.B_PER_GPU, bench.T_MOSEI, bench.DIMS, seed=2024, arena=arena, contrast=crit,
                              contrast_classes="round")
        for k in range(K):
            ts.use_set(k)
            ts.set_batch(*batches[k])
        runs[crit] = (ts, [0])
    out = {c: [] for c in runs}
    for _ in range(args.rounds):
        for crit, (ts, count) in runs.items():
            def run():
                ts.use_set(count[0] % K)
                count[0] += 1
                ts.launch()
            for _ in range(args.warmup):
                run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run()
            torch.cuda.synchronize()
            out[crit].append(round((time.perf_counter() - t0) / args.steps * 1e3, 4))
    final = {c: [round(float(v), 5) for v in runs[c][0].losses.cpu()[:7]] for c in runs}
    print(json.dumps({"ms_per_step": out, "steps": args.steps, "final_losses": final}), flush=True)


if __name__ == "__main__":
    main()
