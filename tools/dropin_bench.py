#!/usr/bin/env python
"""ms/step of the reference's LITERAL training loop (main_frame_val_text_missing.py:119-150) on the drop-in modules
(sdumc_amd.model.get_models + sdumc_amd.loss) at BASELINE configs[1] (B = 64), with the optimizer line (main :317) as
  (a) torch.optim.Adam(model.parameters(), ...)       (b) sdumc_amd.optim.Adam(model.parameters(), ...)
and, for scale, (c) the fused TrainStep on the same batches.  (a) and (b) run alternately in one process, `--rounds` windows
each, so that clock drift hits both alike; every window is `--steps` iterations after `--warmup`, timed with HIP events on the
stream (ms_per_step) and from the host (wall_ms_per_step); the host wall time of optimizer.step() alone -- the enqueue cost the
loop pays for the optimizer -- is measured inside the same windows.  One JSON line.

    python tools/dropin_bench.py [--steps 100] [--warmup 10] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import bench
from sdumc_amd import engine, optim
from sdumc_amd.loss import MSELoss, RMSELoss, RnCLoss
from sdumc_amd.model import get_models


class Loop:
    """One model + optimizer running the loop over the resident batches."""

    def __init__(self, flat0, lay, batches, make_optimizer, dev):
        self.model = get_models(types.SimpleNamespace(input_dims=bench.DIMS, model="wengnet_mosei_mult_views_text_missing"))
        net = self.model.model
        with torch.no_grad():
            for name, v in lay.views(flat0.cpu()).items():
                net._get(name).copy_(v)
        net.seed = 2024                      # the same dropout stream in every loop: the optimizers see the same gradients
        self.model = self.model.to(dev)
        self.model.train()
        self.losses = {'reg_loss': MSELoss().to(dev), 'rmse_loss': RMSELoss().to(dev), 'rnc_loss': RnCLoss().to(dev)}
        self.optimizer = make_optimizer(self.model.parameters())
        self.batches, self.count, self.opt_host_s = batches, 0, 0.0
        self.loss = None

    def step(self):
        model, losses, optimizer = self.model, self.losses, self.optimizer
        audio_feat, text_feat, visual_feat, feat4_feat, vals = self.batches[self.count % len(self.batches)]
        self.count += 1
        w = engine.DEFAULT_WEIGHTS
        optimizer.zero_grad()
        vals_out_0, embeddings_0 = model([audio_feat, text_feat, visual_feat, False])
        features_0, rnc_feat_0, text_feat_0, text_query_feat_0 = embeddings_0
        vals_out_1, embeddings_1 = model([audio_feat, feat4_feat, visual_feat, True])
        features_1, rnc_feat_1, text_feat_1, text_query_feat_1 = embeddings_1
        n_views_feature = torch.stack((rnc_feat_0, rnc_feat_1), dim=1)
        MSEloss_0 = losses['reg_loss'](vals_out_0, vals)
        MSEloss_1 = losses['reg_loss'](vals_out_1, vals)
        rnc_loss = losses['rnc_loss'](n_views_feature, vals.unsqueeze(1))
        loss = (w[0] * MSEloss_0 + w[1] * MSEloss_1 + w[2] * losses['rmse_loss'](text_feat_1, text_feat_0.detach())
                + w[3] * losses['rmse_loss'](text_query_feat_1, text_query_feat_0.detach())
                + w[4] * losses['rmse_loss'](features_1, features_0) + w[5] * rnc_loss)
        loss.backward()
        t0 = time.perf_counter()
        optimizer.step()
        self.opt_host_s += time.perf_counter() - t0
        self.loss = loss


def window(run, steps, warmup):
    """(HIP-event ms/step, host wall ms/step) of `steps` calls after `warmup`."""
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    flat0, lay = bench.init_flat_params(engine, dev)
    batches = [[t.to(dev) for t in bench.synthetic_shard(bench.B_PER_GPU, 0, k=k)] for k in range(bench.N_RESIDENT)]
    hp = dict(lr=1e-4, weight_decay=1e-5)
    loops = {"torch.optim.Adam": Loop(flat0, lay, batches, lambda p: torch.optim.Adam(p, **hp), dev),
             "sdumc_amd.optim.Adam": Loop(flat0, lay, batches, lambda p: optim.Adam(p, **hp), dev)}
    out = {k: {"ms_per_step": [], "wall_ms_per_step": [], "optimizer_step_host_ms": []} for k in loops}
    for _ in range(args.rounds):
        for name, loop in loops.items():
            def run():
                loop.step()
            for _ in range(args.warmup):
                run()
            loop.opt_host_s = 0.0
            ev, wall = window(run, args.steps, 0)
            out[name]["ms_per_step"].append(round(ev, 4))
            out[name]["wall_ms_per_step"].append(round(wall, 4))
            out[name]["optimizer_step_host_ms"].append(round(loop.opt_host_s / args.steps * 1e3, 4))
    for name, loop in loops.items():
        out[name]["final_loss"] = round(float(loop.loss.detach()), 6)
    # (c) the fused step on the same batches, as bench.py's headline runs it
    flat = flat0.clone()
    ts, run = bench.resident_step(engine, flat, batches)
    fused = {"ms_per_step": [], "wall_ms_per_step": []}
    for _ in range(args.rounds):
        ev, wall = window(run, args.steps, args.warmup)
        fused["ms_per_step"].append(round(ev, 4))
        fused["wall_ms_per_step"].append(round(wall, 4))
    out["fused TrainStep"] = fused
    print(json.dumps({"dropin_loop": out, "B": bench.B_PER_GPU, "steps": args.steps, "warmup": args.warmup,
                      "parameters_with_gradients": len(loops["sdumc_amd.optim.Adam"].optimizer._live)}), flush=True)


if __name__ == "__main__":
    main()
