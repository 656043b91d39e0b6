"""The cost of keeping the attention maps in an evaluation epoch (evaluate.eval_epoch(..., attention=True): one
sdumc_net_export_attention launch per batch, csrc/attn_export.hip) over a synthetic C2-shaped resident store (bench.py: T_MOSEI, DIMS;
tools/eval_epoch_bench.py's store, permutation and batches): samples/s of the in-place epoch with the option off and on, ALTERNATED --
one warm-up epoch each, then `rounds` pairs (off, on), HIP events around every epoch, one synchronisation after it -- the best and all
epochs of both, the ratio on / off (best over best, and the median of the per-round ratios), the spread of the off epochs, and the
bytes the export writes per epoch.  Checks that preds and seen are bit-equal with and without the option.  Prints one JSON line.
usage: python tools/attn_export_bench.py [n=2048] [B=64] [bf16] [rounds=5]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import bench
    from sdumc_amd import engine, evaluate
    from sdumc_amd.data import DeviceFeatureStore
    args = sys.argv[1:]
    nums = [int(a) for a in args if a.isdigit()]
    n, B = nums[0] if nums else 2048, nums[1] if len(nums) > 1 else 64
    rounds = next((int(a.split("=")[1]) for a in args if a.startswith("rounds=")), 5)
    bf16 = "bf16" in args
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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    hold = {False: None, True: None}

    def epoch(attention):
        hold[attention] = evaluate.eval_epoch(flat, DIMS, store, plan, bf16=bf16, attention=attention, out=hold[attention])

    def timed(attention):
        e0.record()
        epoch(attention)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for a in (False, True):
        epoch(a)
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(rounds):
        for a in (False, True):
            ms[a].append(timed(a))
    off, on = hold[False], hold[True]
    if int((on.seen != 0).sum()) != n or not all(bool(torch.isfinite(t).all()) for d in on.attention.values() for t in d.values()):
        raise SystemExit("the epoch did not fill the attention maps")
    if not (torch.equal(off.preds, on.preds) and torch.equal(off.seen, on.seen)):
        raise SystemExit("the option changed the predictions")
    ratios = sorted(y / x for x, y in zip(ms[False], ms[True]))
    exported = sum(t.numel() * 4 for d in on.attention.values() for t in d.values())
    out = {"tool": "attn_export_bench", "n": n, "B": B, "batches": nb, "bf16": bool(bf16), "rounds": rounds,
           "store_gb": round(store.nbytes / 1e9, 2), "exported_bytes_per_epoch": exported,
           "exported_mb_per_batch": round(exported / nb / 1e6, 3)}
    for name, a in (("attention_off", False), ("attention_on", True)):
        out[name] = {"samples_per_s": round(n / min(ms[a]) * 1e3, 1), "ms_per_batch": round(min(ms[a]) / nb, 4),
                     "epoch_ms": [round(m, 2) for m in ms[a]]}
    out["off_spread"] = round(max(ms[False]) / min(ms[False]) - 1, 4)
    out["on_over_off_time_best"] = round(min(ms[True]) / min(ms[False]), 4)
    out["on_over_off_time_median_of_rounds"] = round(ratios[len(ratios) // 2], 4)
    out["extra_us_per_batch_best"] = round((min(ms[True]) - min(ms[False])) / nb * 1e3, 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
