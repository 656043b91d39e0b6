"""The cost of keeping a training epoch's record (FusedTrainer.train_epoch: one sdumc_epoch_record call per step,
csrc/epoch_record.hip: one launch, two with grad_norm) over a synthetic C2-shaped resident store (bench.py: T_MOSEI, DIMS; tools/eval_epoch_bench.py's store, permutation
and batches -- a ragged epoch, every batch padded to its own frame maxima, the last one short when B does not divide n): ms per step of
  (b) run_epoch,
  (c) train_epoch()                      (predictions and the log row),
  (d) train_epoch(grad_norm=True)        (... and the L2 norm / non-finite count of the 15.4 MB gradient bucket),
  (d_emb) train_epoch(embeddings=True, grad_norm=True)   (all ten scatter segments),
  (f) train_epoch(grad_norm=True, by_tensor=True)        (... and sdumc_tensor_norms over the bucket: a norm and a count per tensor),
  (g) train_epoch(grad_norm=True, by_tensor='updates')   (... and a second call over the parameters against the record's snapshot),
  (e) run_epoch(on_step=clone)           (the workaround the record replaces: an allocation and a copy launch per step),
ALTERNATED: one warm-up epoch each, then `rounds` rounds of (b, c, d, d_emb, f, g, e), HIP events around every epoch, one synchronisation after
it -- best and all epochs of each, the extra microseconds per step over (b) (best over best, and the median of the per-round
differences), and the spread of the (b) epochs.  All legs continue ONE training run (the time of a step does not depend on the
parameters).  Every timed epoch is enqueued BEHIND an untimed run_epoch, with the first event between the two: the host's work in front
of an epoch's first launch (train_epoch checks the indices and refills the record; once per epoch, whatever its length) then overlaps
the device's previous epoch, as it does when epochs follow each other, and the events bracket the epoch's device time alone.  `cold`
drops that epoch: the device idles through the host's prologue and the window holds it (what a loop sees that synchronises after every
epoch, as one that reads rec.results() does); host_prologue_ms is that host work timed on its own.  Prints one JSON line.
(a), the parent commit's run_epoch: the same tool with `parent` and SDUMC_LIB=<the parent build's libsdumc_hip.so> times leg (b)
alone on that library (it has no sdumc_epoch_record); alternate the two processes.  A parent that has the record but not a newer leg
(f and g need sdumc_tensor_norms) is timed with SDUMC_LIB alone and only=b,c,d: the legs a library lacks are left out by name.
usage: python tools/epoch_record_bench.py [n=2048] [B=64] [bf16] [rounds=3] [parent] [cold] [only=c,d,...]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import bench
    from sdumc_amd import engine
    from sdumc_amd.data import DeviceFeatureStore
    args = sys.argv[1:]
    nums = [int(a) for a in args if a.isdigit()]
    n, B = nums[0] if nums else 2048, nums[1] if len(nums) > 1 else 64
    rounds = next((int(a.split("=")[1]) for a in args if a.startswith("rounds=")), 3)
    bf16, parent, cold = "bf16" in args, "parent" in args, "cold" in args
    only = next((a.split("=")[1].split(",") for a in args if a.startswith("only=")), None)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    DIMS, T = bench.DIMS, bench.T_MOSEI
    flat, _ = bench.init_flat_params(engine, dev)
    hf = engine.bf16_mode(bf16, DIMS) == 2
    store = DeviceFeatureStore.synthetic(n, T, DIMS, seed=1234, device=dev, bf16=hf, planes=not hf)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(7))
    batches = [perm[o:o + B] for o in range(0, n, B)]
    plan = store.plan_epoch(batches)
    nb = len(batches)
    tr = engine.FusedTrainer(flat, DIMS, lr=1e-5, seed=3, capacity=(B, T), **({"bf16": True} if bf16 else {}))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    hold, clones = {}, []

    def leg(name):
        if name == "b_run_epoch":
            tr.run_epoch(store, plan)
        elif name == "e_run_epoch_on_step_clone":
            clones.clear()
            tr.run_epoch(store, plan, on_step=lambda i, l: clones.append(l.clone()))
        else:
            kw = {"c_train_epoch": {}, "d_train_epoch_grad_norm": {"grad_norm": True},
                  "d_emb_train_epoch_embeddings_grad_norm": {"grad_norm": True, "embeddings": True},
                  "f_train_epoch_grad_norm_by_tensor": {"grad_norm": True, "by_tensor": True},
                  "g_train_epoch_grad_norm_by_tensor_updates": {"grad_norm": True, "by_tensor": "updates"}}[name]
            hold[name] = tr.train_epoch(store, plan, out=hold.get(name), **kw)

    def timed(name):
        if not cold:
            tr.run_epoch(store, plan)
        e0.record()
        leg(name)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    legs = ["b_run_epoch"] if parent else ["b_run_epoch", "c_train_epoch", "d_train_epoch_grad_norm",
                                           "d_emb_train_epoch_embeddings_grad_norm", "f_train_epoch_grad_norm_by_tensor",
                                           "g_train_epoch_grad_norm_by_tensor_updates", "e_run_epoch_on_step_clone"]
    if only is not None:
        legs = [name for name in legs if name.replace("_train_epoch", " ").replace("_run_epoch", " ").split()[0] in only]
    for name in legs:
        leg(name)
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(rounds):
        for name in legs:
            ms[name].append(timed(name))
    out = {"tool": "epoch_record_bench", "n": n, "B": B, "steps": nb, "bf16": bool(bf16), "rounds": rounds, "parent_library": parent,
           "library": os.environ.get("SDUMC_LIB", "tree"), "distinct_batch_shapes": len(set(plan.shapes)), "in_place": tr._in_place(store)}
    for name in legs:
        out[name] = {"ms_per_step": round(min(ms[name]) / nb, 5), "epoch_ms": [round(m, 3) for m in ms[name]]}
    base = ms.get("b_run_epoch")
    if base:
        out["b_spread"] = round(max(base) / min(base) - 1, 4)
    for name in legs[1:] if base else ():
        d = sorted(y - x for x, y in zip(base, ms[name]))
        out[name]["extra_us_per_step_best"] = round((min(ms[name]) - min(base)) / nb * 1e3, 2)
        out[name]["extra_us_per_step_median_of_rounds"] = round(d[len(d) // 2] / nb * 1e3, 2)
    for name, rec in hold.items():
        s = rec.summary()
        if rec.steps != nb or int((rec.seen != 0).sum()) != n or s["nonfinite_steps"]:
            raise SystemExit(f"{name}: the epoch did not fill its record")
        if ("grad_norm" in name) != bool(s["grad_norm_max"] == s["grad_norm_max"]):
            raise SystemExit(f"{name}: grad_norm column is not what the option asked for")
        bt = rec.by_tensor
        if ("by_tensor" in name) != (bt is not None) or ("updates" in name) != (bt is not None and bt.update_norm is not None):
            raise SystemExit(f"{name}: the record by tensor is not what the option asked for")
        if bt is not None:      # the tensors' norms add up to the bucket's, every row was filled
            import numpy as np
            tot = np.sqrt((bt.grad_norm[:nb].double().cpu().numpy() ** 2).sum(1))
            if bt.first_nonfinite() is not None or not np.allclose(tot, rec.log[:nb, 8].double().cpu().numpy(), rtol=1e-6, atol=0):
                raise SystemExit(f"{name}: the per-tensor gradient norms do not add up to the bucket's norm")
            if bt.update_norm is not None:
                r = bt.update_ratio()
                out["update_ratio_last_step"] = {"median": float(np.nanmedian(r[-1])), "max": float(np.nanmax(r[-1]))}
    if "d_train_epoch_grad_norm" in hold:
        s = hold["d_train_epoch_grad_norm"].summary()
        out["last_epoch"] = {k: round(s[k], 6) for k in ("total", "mse_full", "mse_missing", "grad_norm_max", "grad_norm_last")}
    out["cold"] = cold
    if hold:      # the host's work in front of a recorded epoch's first launch, on its own
        import time
        from sdumc_amd.evaluate import checked_plan
        rec, t = hold[next(iter(hold))], []
        for _ in range(5):
            t0 = time.perf_counter()
            checked_plan(plan, n)
            rec.fits(n, nb, dev, rec.embeddings is not None, rec.n_grads, rec.by_tensor.mode if rec.by_tensor is not None else False,
                     engine.ParamLayout.get(*DIMS[:3]))
            rec.reset()
            t.append(1e3 * (time.perf_counter() - t0))
            torch.cuda.synchronize()
        out["host_prologue_ms"] = round(min(t), 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
