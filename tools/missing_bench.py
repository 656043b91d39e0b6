"""What the random-missing protocol costs (DeviceFeatureStore.with_missing: the gather launch that writes a batch's row maps redirects the
absent frames to the store's zero row, csrc/elementwise.hip gather_batch_kernel) over a synthetic C2-shaped resident store (bench.py:
T_MOSEI, DIMS; tools/epoch_record_bench.py's store, permutation and batches -- a ragged epoch, every batch padded to its own frame
maxima):
  run_plain / run_plain2   FusedTrainer.run_epoch on the store, twice per round (the spread between two identical legs is the margin),
  run_view                 run_epoch on store.with_missing(frame={'audio': .2, 'video': .2}, seed=1234).redrawn(epoch), a new view per epoch,
  eval_plain / eval_plain2 / eval_view   FusedTrainer.eval_epoch likewise (samples/s),
  gather_plain / gather_view             the gather launch alone in its map-only form (one batch of B, `reps` launches between two events),
ALTERNATED in one process: one warm-up of each leg, then `rounds` rounds of all of them, HIP events around every epoch and one
synchronisation after it.  Every timed epoch is enqueued BEHIND an untimed one of the same kind, with the first event between the two,
so the events bracket the epoch's device time and the host's work in front of its first launch overlaps the previous epoch (as it does
when epochs follow each other).  All training legs continue ONE run (the time of a step does not depend on the parameters, nor on which
rows are zero).  Prints one JSON line: best and all epochs of each leg, the view's extra over the plain leg (best over best, and the
median of the per-round differences) and the spread of the plain legs.
The parent commit's legs: the same tool run from a checkout of the parent with `parent` (plain legs only: it has no with_missing);
alternate the two processes.
usage: python tools/missing_bench.py [n=2048] [B=64] [bf16] [rounds=6] [reps=200] [parent]"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import bench
    from sdumc_amd import engine, _lib
    from sdumc_amd.data import DeviceFeatureStore
    args = sys.argv[1:]
    nums = [int(a) for a in args if a.isdigit()]
    n, B = nums[0] if nums else 2048, nums[1] if len(nums) > 1 else 64
    rounds = next((int(a.split("=")[1]) for a in args if a.startswith("rounds=")), 6)
    reps = next((int(a.split("=")[1]) for a in args if a.startswith("reps=")), 200)
    bf16, parent = "bf16" in args, "parent" in args
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
    view = None if parent else store.with_missing(frame={"audio": .2, "video": .2}, seed=1234)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    epoch, hold = [0], {}

    # the gather launch alone, map-only: the first batch's descriptor on the plain store and on the view
    Bk, Tk = plan.shapes[0]
    maps = [torch.empty(Bk * t, dtype=torch.int32, device=dev) for t in Tk]
    labels = torch.empty(Bk, device=dev)

    def gather(s):
        g = s.gather_desc(plan.idx_ptr(0), Bk, Tk, None, labels, None, maps_out=maps)
        st = _lib.current_stream()
        for _ in range(reps):
            _lib.check(_lib.lib.sdumc_gather_batch(C.byref(g), 0, st), "sdumc_gather_batch")

    def leg(name):
        kind, who = name.split("_")
        s = store if who.startswith("plain") else view
        if kind == "run":
            epoch[0] += 1
            tr.run_epoch(s if s is store else view.redrawn(epoch[0]), plan)
        elif kind == "eval":
            hold[name] = tr.eval_epoch(s, plan, out=hold.get(name))
        else:
            gather(s)

    def timed(name):
        kind = name.split("_")[0]
        if kind != "gather":
            leg(kind + "_plain")      # (untimed: the device is busy while the host prepares the timed epoch)
        e0.record()
        leg(name)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    whos = ("plain", "plain2") if parent else ("plain", "view", "plain2")
    legs = [f"{k}_{w}" for k in ("run", "eval") for w in whos] + [f"gather_{w}" for w in whos if w != "plain2"]
    for name in legs:
        leg(name)
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(rounds):
        for name in legs:
            ms[name].append(timed(name))
    out = {"tool": "missing_bench", "n": n, "B": B, "steps": nb, "bf16": bool(bf16), "rounds": rounds, "parent": parent,
           "library": os.environ.get("SDUMC_LIB", "tree"), "distinct_batch_shapes": len(set(plan.shapes)), "in_place": tr._in_place(store)}
    for name in legs:
        kind = name.split("_")[0]
        best = min(ms[name])
        if kind == "run":
            out[name] = {"ms_per_step": round(best / nb, 5), "epoch_ms": [round(m, 3) for m in ms[name]]}
        elif kind == "eval":
            out[name] = {"samples_per_s": round(n / best * 1e3, 1), "epoch_ms": [round(m, 3) for m in ms[name]]}
        else:
            out[name] = {"us_per_launch": round(best / reps * 1e3, 3), "all_us": [round(m / reps * 1e3, 3) for m in ms[name]],
                         "rows": int(Bk * sum(Tk))}
    for kind in ("run", "eval"):
        a, b = ms[f"{kind}_plain"], ms[f"{kind}_plain2"]
        d = sorted(abs(y - x) / x for x, y in zip(a, b))
        out[f"{kind}_plain_spread"] = {"best_over_best": round(abs(min(b) / min(a) - 1), 5), "median_of_rounds": round(d[len(d) // 2], 5),
                                       "max_over_min_all": round(max(a + b) / min(a + b) - 1, 5)}
        if not parent:
            v = ms[f"{kind}_view"]
            d = sorted((y - x) / x for x, y in zip(a, v))
            out[f"{kind}_view_extra"] = {"best_over_best": round(min(v) / min(a) - 1, 5), "median_of_rounds": round(d[len(d) // 2], 5),
                                         "us_per_step_best": round((min(v) - min(a)) / nb * 1e3, 2)}
    import time      # the host's share: building one batch's descriptor (the loop does it once per step)
    out["host_desc_us"] = {}
    for who, s in (("plain", store),) + ((("view", view),) if not parent else ()):
        t0 = time.perf_counter()
        for _ in range(2000):
            s.gather_desc(plan.idx_ptr(0), Bk, Tk, None, labels, None, maps_out=maps)
        out["host_desc_us"][who] = round((time.perf_counter() - t0) / 2000 * 1e6, 2)
    if not parent:      # the view did drop frames: its predictions are not the plain store's
        p, v = hold["eval_plain"], hold["eval_view"]
        if int((v.seen != 0).sum()) != n or torch.equal(p.preds, v.preds) or not bool(torch.isfinite(v.preds).all()):
            raise SystemExit("eval_view: the view's epoch is not a full, finite epoch that differs from the plain store's")
        out["absent_share"] = {m: round(float(view.absent_rows(m).mean()), 4) for m in ("audio", "video")}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
