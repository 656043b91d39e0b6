"""The cost of the selectable regression criterion (TrainStep / FusedTrainer(regress='mse' | 'l1' | 'huber' | 'ccc'); csrc/loss.hip: the
p == 3 workgroups of loss_stage2_kernel) over a synthetic C2-shaped resident store (bench.py: T_MOSEI, DIMS; tools/adamw_bench.py's
store, permutation and batches -- a ragged epoch of 32 steps at n = 2048, B = 64): ms per step of run_epoch on four trainers over the
same store,
  off    FusedTrainer()                   (the default: launch for launch the step without the option),
  l1     FusedTrainer(regress='l1'),
  huber  FusedTrainer(regress='huber', regress_delta=0.5),
  ccc    FusedTrainer(regress='ccc')      (two double-precision passes and the gradient pass in the workgroup that held an MSE term),
ALTERNATED: one warm-up epoch each, then `rounds` rounds of the four, HIP events around every epoch, one synchronisation after it; every
timed epoch is enqueued behind an untimed epoch of the same trainer, with the first event between the two, so the events bracket the
epoch's device time alone.  Best and all epochs of each leg, the extra microseconds per step over `off` (best over best, and the median
of the per-round differences; negative = faster) and the spread of the `off` epochs.
`parent` times `off` alone -- ONE trainer in the process; with SDUMC_LIB=<the parent build's libsdumc_hip.so> on that library.
ab=<that library>: the A/B itself -- `pairs` times a fresh process of `parent` on the parent's library and the same `parent` process
on this tree (like for like: one trainer, one leg; the two swap places from pair to pair), then this tree's four legs, one process at a
time (fresh child processes: the library is chosen when sdumc_amd is imported) -- and one JSON line with both sides' `off` epochs, the
run-to-run spread BETWEEN the parent's processes (best epoch of each: the yardstick for "off costs nothing"), tree over parent and the
tree's legs.
stage2 regress=<criterion>: `steps` plain TrainStep launches at B (n = 2B <= 256: the fused two-launch loss route) and nothing else,
for a kernel trace of loss_stage2_kernel under a profiler -- one criterion per process, e.g.
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/regress_bench.py stage2 regress=ccc
usage: python tools/regress_bench.py [n=2048] [B=64] [bf16] [rounds=5] [parent] [ab=<parent .so>] [pairs=3]
       python tools/regress_bench.py stage2 regress=<mse|l1|huber|ccc> [B=64] [bf16] [steps=50]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = {"off": {}, "l1": {"regress": "l1"}, "huber": {"regress": "huber", "regress_delta": 0.5}, "ccc": {"regress": "ccc"}}


def _opt(args, key, default):
    return next((a.split("=", 1)[1] for a in args if a.startswith(key + "=")), default)


def measure(args):
    import torch
    import bench
    from sdumc_amd import engine
    from sdumc_amd.data import DeviceFeatureStore
    nums = [int(a) for a in args if a.isdigit()]
    n, B = nums[0] if nums else 2048, nums[1] if len(nums) > 1 else 64
    rounds = int(_opt(args, "rounds", 5))
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
    legs = ["off"] if parent else list(LEGS)
    kw = {"bf16": True} if bf16 else {}
    tr = {name: engine.FusedTrainer(flat.clone(), DIMS, lr=1e-5, seed=3, capacity=(B, T), **LEGS[name], **kw) for name in legs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(name):
        tr[name].run_epoch(store, plan)
        e0.record()
        tr[name].run_epoch(store, plan)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for name in legs:
        tr[name].run_epoch(store, plan)
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(rounds):
        for name in legs:
            ms[name].append(timed(name))
    out = {"tool": "regress_bench", "n": n, "B": B, "steps": nb, "bf16": bool(bf16), "rounds": rounds, "parent_library": parent,
           "library": os.environ.get("SDUMC_LIB", "tree")}
    for name in legs:
        out[name] = {"ms_per_step": round(min(ms[name]) / nb, 5), "epoch_ms": [round(m, 3) for m in ms[name]]}
    base = ms["off"]
    out["off_spread"] = round(max(base) / min(base) - 1, 4)
    for name in legs[1:]:
        d = sorted(y - x for x, y in zip(base, ms[name]))
        out[name]["extra_us_per_step_best"] = round((min(ms[name]) - min(base)) / nb * 1e3, 2)
        out[name]["extra_us_per_step_median_of_rounds"] = round(d[len(d) // 2] / nb * 1e3, 2)
    for name in legs:
        if not bool(torch.isfinite(tr[name].params).all()):
            raise SystemExit(f"{name}: non-finite parameters")
        # what the legs claim to have done: another criterion trained other parameters than the default run
        if name != "off" and torch.equal(tr[name].params, tr["off"].params):
            raise SystemExit(f"{name}: the parameters of the default run")
    return out


def stage2(args):
    """plain fused steps of one criterion, for a profiler's kernel trace"""
    import torch
    import bench
    from sdumc_amd import engine
    crit = _opt(args, "regress", "mse")
    B, steps = int(_opt(args, "B", 64)), int(_opt(args, "steps", 50))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    flat, _ = bench.init_flat_params(engine, dev)
    kw = dict(LEGS["off" if crit == "mse" else crit])
    if "bf16" in args:
        kw["bf16"] = True
    ts = engine.TrainStep(flat, B, bench.T_MOSEI, bench.DIMS, seed=3, lr=1e-5, **kw)
    ts.set_batch(*[t.to(dev) for t in bench.synthetic_shard(B, 0, k=0)])
    for _ in range(steps):
        ts.launch()
    torch.cuda.synchronize()
    losses = ts.losses.cpu()
    if not bool(torch.isfinite(losses[:7]).all()):
        raise SystemExit(f"{crit}: non-finite losses")
    return {"tool": "regress_bench", "mode": "stage2", "regress": crit, "B": B, "steps": steps, "bf16": "bf16" in args,
            "losses": [round(float(v), 6) for v in losses[:7]]}


def ab(args, parent_lib):
    """fresh child processes, one at a time: the parent's library and this tree, alternated"""
    pairs = int(_opt(args, "pairs", 3))
    rest = [a for a in args if not a.startswith(("ab=", "pairs=")) and a != "parent"]
    runs = {"parent": [], "tree_off": [], "tree": []}
    for i in range(pairs):
        for side in (("parent", "tree_off") if i % 2 == 0 else ("tree_off", "parent")) + ("tree",):
            env = dict(os.environ)
            env.pop("SDUMC_LIB", None)
            if side == "parent":
                env["SDUMC_LIB"] = os.path.abspath(parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__)] + rest + (["parent"] if side != "tree" else [])
            text = subprocess.run(cmd, env=env, cwd=ROOT, check=True, stdout=subprocess.PIPE, timeout=600).stdout.decode()
            runs[side].append(json.loads(text.strip().splitlines()[-1]))
    out = {"tool": "regress_bench", "mode": "ab", "pairs": pairs, "parent_library": os.path.abspath(parent_lib)}
    for key in ("n", "B", "steps", "bf16", "rounds"):
        out[key] = runs["tree"][0][key]
    best = {side: [r["off"]["ms_per_step"] for r in rs] for side, rs in runs.items()}
    out["parent_off_ms_per_step"] = best["parent"]
    out["tree_off_ms_per_step"] = best["tree_off"]
    out["tree_off_in_the_four_leg_process_ms_per_step"] = best["tree"]
    out["epoch_spread_inside_a_process"] = {side: [r["off_spread"] for r in rs] for side, rs in runs.items()}
    out["parent_process_spread"] = round(max(best["parent"]) / min(best["parent"]) - 1, 4)
    out["tree_process_spread"] = round(max(best["tree_off"]) / min(best["tree_off"]) - 1, 4)
    out["tree_off_over_parent_best"] = round(min(best["tree_off"]) / min(best["parent"]) - 1, 4)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    out["tree_off_over_parent_median"] = round(med(best["tree_off"]) / med(best["parent"]) - 1, 4)
    for name in list(LEGS)[1:]:
        out[name] = {"ms_per_step": [r[name]["ms_per_step"] for r in runs["tree"]],
                     "extra_us_per_step_best": [r[name]["extra_us_per_step_best"] for r in runs["tree"]],
                     "extra_us_per_step_median_of_rounds": [r[name]["extra_us_per_step_median_of_rounds"] for r in runs["tree"]]}
    return out


def main():
    args = sys.argv[1:]
    parent_lib = _opt(args, "ab", None)
    if "stage2" in args:
        out = stage2(args)
    else:
        out = ab(args, parent_lib) if parent_lib else measure(args)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
