#!/usr/bin/env python
"""Temporal pre-compression of a resident store (DeviceFeatureStore.resampled, sdumc_pool_frames), measured at the C2 shapes:
a synthetic store of `--n` utterances (default 2048) at T = (375, 32, 225, 32), widths (1024, 4096, 1024, 4096), fp32 with planes.

  kernel     per modality: sdumc_pool_frames alone for feat_scale = `--scale`, between two HIP events on the current stream
             (`--reps` launches after `--warmup`, median and best), and the GB/s of bytes read (every source frame once, the four
             tables) plus bytes written (the pooled rows and the zero row), beside the HBM ceiling (8.0 TB/s spec, 6.3 TB/s the
             best float4 copy measured on this chip).  `utt` rows: the same for feat_type='utt' (long pools, few rows written).
  resampled  store.resampled(feat_scale) INCLUDING its table uploads, allocations and make_planes(), host clock around a device
             synchronise (median of `--reps`), next to the host route on the same store, timed ONCE: download, resample_instances,
             DeviceFeatureStore(...), make_planes.  `--no-host` skips the host route.
  epoch      FusedTrainer.run_epoch ms/step over `--batches` ragged batches of 64 on the source store and on the compressed one
             (the same index vectors; warm-up by 10 batches and 0.3 s of wall clock as bench.py's epoch leg), alternated `--rounds`
             times.
One JSON line.

    python tools/resample_bench.py [--n 2048] [--scale 2] [--reps 20] [--warmup 3] [--batches 100] [--rounds 3] [--no-host]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bench
from sdumc_amd import _lib, engine
from sdumc_amd.data import DeviceFeatureStore, _target_lengths, resample_instances

HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.3


def kernel_leg(store, step, reps, warmup):
    """sdumc_pool_frames alone, one modality at a time, into a preallocated destination"""
    targets = _target_lengths([store._len_np[m] for m in store.MODS], step)
    out = {}
    for m, tgt in zip(store.MODS, targets):
        src, d = store.packed[m], store.dim[m]
        rows = int(tgt.sum())
        dst = torch.empty(rows + 1, d, dtype=src.dtype, device=src.device)
        start = torch.from_numpy(np.concatenate([[0], np.cumsum(tgt)[:-1]]).astype(np.int64)).to(src.device)
        length = torch.from_numpy(tgt.astype(np.int32)).to(src.device)
        p = _lib.PoolFrames()
        p.src, p.dst = src.data_ptr(), dst.data_ptr()
        p.src_start, p.src_len = store.start_d[m].data_ptr(), store.length_d[m].data_ptr()
        p.dst_start, p.dst_len = start.data_ptr(), length.data_ptr()
        p.src_rows, p.dst_rows, p.n_utts, p.cols, p.bf16 = src.shape[0] - 1, rows, len(store), d, int(src.dtype == torch.bfloat16)
        run = lambda: _lib.check(_lib.lib.sdumc_pool_frames(C.byref(p), 0, _lib.current_stream()), "sdumc_pool_frames")
        for _ in range(warmup):
            run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        # every source frame is read exactly once (whatever the pool), plus the four tables
        read = int(store._len_np[m].sum()) * d * src.element_size() + 24 * len(store)
        written = (rows + 1) * d * src.element_size()
        med = statistics.median(ms)
        out[m] = {"ms_median": round(med, 4), "ms_best": round(min(ms), 4), "src_rows": int(src.shape[0] - 1), "dst_rows": rows,
                  "width": d, "mb_read": round(read / 1e6, 1), "mb_written": round(written / 1e6, 1),
                  "gb_per_s_median": round((read + written) / med / 1e6, 1), "gb_per_s_best": round((read + written) / min(ms) / 1e6, 1)}
    return out


def host_route(store, scale):
    """download, resample_instances, rebuild the store, make_planes: what a user has to do without resampled()"""
    t0 = time.perf_counter()
    host = {m: store.packed[m].cpu().numpy() for m in store.MODS}
    vals = store.vals.cpu().numpy()
    inst = []
    for i, name in enumerate(store.names):
        one = {"name": name, "val": float(vals[i]), "emo": 0.0}
        for m in store.MODS:
            s, n = int(store.start[m][i]), int(store.length[m][i])
            one[m] = host[m][s:s + n]
        inst.append(one)
    t1 = time.perf_counter()
    inst = resample_instances(inst, feat_scale=scale)
    t2 = time.perf_counter()
    new = DeviceFeatureStore(inst, device=store.device, planes=True)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return new, {"download_s": round(t1 - t0, 3), "resample_instances_s": round(t2 - t1, 3), "rebuild_with_planes_s": round(t3 - t2, 3),
                 "total_s": round(t3 - t0, 3)}


def epoch_ms(tr, store, plan_w, plan_t, prewarm_s=0.3):
    t_w = time.perf_counter()
    tr.run_epoch(store, plan_w)
    torch.cuda.synchronize()
    while time.perf_counter() - t_w < prewarm_s:
        tr.run_epoch(store, plan_w)
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.run_epoch(store, plan_t)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / len(plan_t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--scale", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    T, dims, B = bench.T_MOSEI, bench.DIMS, bench.B_PER_GPU
    store = DeviceFeatureStore.synthetic(args.n, T, dims, seed=1234, device=dev, planes=True)
    out = {"store": {"utterances": len(store), "T": list(T), "dims": list(dims), "gb": round(store.nbytes / 1e9, 2)},
           "hbm_tb_per_s": {"spec": HBM_SPEC_TBS, "best_measured_copy": HBM_COPY_TBS},
           "kernel": {f"feat_scale={args.scale}": kernel_leg(store, args.scale, args.reps, args.warmup),
                      "feat_type=utt": kernel_leg(store, "utt", args.reps, args.warmup)}}
    # resampled(): everything a caller waits for, planes included
    for _ in range(args.warmup):
        store.resampled(feat_scale=args.scale)
    torch.cuda.synchronize()
    ts, ts_np = [], []
    for planes, acc in ((True, ts), (False, ts_np)):
        for _ in range(args.reps):
            t0 = time.perf_counter()
            small = store.resampled(feat_scale=args.scale, planes=planes)
            torch.cuda.synchronize()
            acc.append(1e3 * (time.perf_counter() - t0))
    small = store.resampled(feat_scale=args.scale)
    out["resampled"] = {"ms_median_with_planes": round(statistics.median(ts), 3), "ms_best_with_planes": round(min(ts), 3),
                        "ms_median_without_planes": round(statistics.median(ts_np), 3), "result_gb": round(small.nbytes / 1e9, 2)}
    if not args.no_host:
        host_store, out["host_route"] = host_route(store, args.scale)
        out["host_route"]["equal_to_resampled"] = all(torch.equal(small.packed[m], host_store.packed[m]) and
                                                      torch.equal(small.packed_p3[m], host_store.packed_p3[m]) for m in store.MODS)
        out["host_route"]["over_resampled"] = round(1e3 * out["host_route"]["total_s"] / statistics.median(ts), 1)
        del host_store
    # run_epoch on the source store and on the compressed one: the same index vectors, trainers of their own, alternated
    g = torch.Generator().manual_seed(7)
    batches = [torch.randperm(len(store), generator=g)[:B] for _ in range(args.batches + 10)]
    flat0, _ = bench.init_flat_params(engine, dev)
    legs = {}
    for name, st in (("source", store), ("compressed", small)):
        cap_T = tuple(int(st._len_np[m].max()) for m in st.MODS)
        legs[name] = (engine.FusedTrainer(flat0.clone(), dims, capacity=(B, cap_T), seed=2024), st, st.plan_epoch(batches[:10]),
                      st.plan_epoch(batches[10:]), [])
    for _ in range(args.rounds):
        for tr, st, pw, pt, acc in legs.values():
            acc.append(round(epoch_ms(tr, st, pw, pt), 4))
    for name, (tr, st, pw, pt, acc) in legs.items():
        if not torch.isfinite(tr.state.losses).all():
            raise SystemExit(f"non-finite loss on the {name} store")
    mean_T = {name: [round(float(np.mean([sh[1][i] for sh in legs[name][3].shapes])), 1) for i in range(4)] for name in legs}
    out["epoch"] = {"batch": B, "batches": args.batches, "ms_per_step": {k: v[4] for k, v in legs.items()}, "mean_padded_T": mean_T,
                    "compressed_over_source": round(statistics.median(legs["compressed"][4]) / statistics.median(legs["source"][4]), 4)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
