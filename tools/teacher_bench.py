"""The cost of distillation targets from a stored teacher (TrainStep / FusedTrainer(teacher=); csrc/loss.hip: the distillation
workgroups of loss_stage1_kernel / loss_stage2_kernel read their targets from store-ordered tables through the batch's index vector)
over a synthetic C2-shaped resident store (bench.py: T_MOSEI, DIMS; tools/regress_bench.py's store, permutation and batches -- a ragged
epoch of 32 steps at n = 2048, B = 64): ms per step of run_epoch on two trainers over the same store,
  off      FusedTrainer()                       (the default: launch for launch the step without the option),
  teacher  FusedTrainer(teacher=<three random store-ordered tables>),
ALTERNATED: one warm-up epoch each, then `rounds` rounds of the two, HIP events around every epoch, one synchronisation after it; every
timed epoch is enqueued behind an untimed epoch of the same trainer, with the first event between the two, so the events bracket the
epoch's device time alone.  Best and all epochs of each leg, the extra microseconds per step over `off` (best over best, and the median
of the per-round differences; negative = faster) and the spread of the `off` epochs.  Then, once per process, the price of a mean
teacher at epoch granularity: `refresh` = ms of trainer.refresh_teacher(store, plan, weights='ema') per epoch (best of `rounds`, wall
clock around a synchronised call) and per batch.
`parent` times `off` alone -- ONE trainer in the process; with SDUMC_LIB=<the parent build's libsdumc_hip.so> on that library.
ab=<that library>: the A/B itself -- `pairs` times a fresh process of `parent` on the parent's library and the same `parent` process
on this tree (like for like: one trainer, one leg; the two swap places from pair to pair), then this tree's legs, one process at a
time (fresh child processes: the library is chosen when sdumc_amd is imported) -- and one JSON line with both sides' `off` epochs, the
run-to-run spread BETWEEN the parent's processes (best epoch of each: the yardstick for "off costs nothing"), tree over parent and the
tree's legs.
stage teacher=<off|on>: `steps` plain TrainStep launches at B (n = 2B <= 256: the fused two-launch loss route) and nothing else, for a
kernel trace of loss_stage1_kernel / loss_stage2_kernel under a profiler -- one setting per process (off also on the parent's
library through SDUMC_LIB), e.g.
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/teacher_bench.py stage teacher=on
workaround: what the option replaces -- the module loop (get_models + the loss modules + autograd + the drop-in fused Adam over the
model's parameter tensors) with RMSELoss(x_1, table[idx]) for the three pairs: ms per step at B over `steps` steps of one resident batch.
usage: python tools/teacher_bench.py [n=2048] [B=64] [bf16] [rounds=5] [parent] [ab=<parent .so>] [pairs=3]
       python tools/teacher_bench.py stage teacher=<off|on> [B=64] [bf16] [steps=50]
       python tools/teacher_bench.py workaround [B=64] [steps=20]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTHS = {"text_hidden": (256,), "cross_text": (7, 128), "fused": (128,)}


def _opt(args, key, default):
    return next((a.split("=", 1)[1] for a in args if a.startswith(key + "=")), default)


def _tables(n, dev):
    import torch
    g = torch.Generator().manual_seed(11)
    return {k: (0.5 * torch.randn((n,) + w, generator=g)).to(dev) for k, w in WIDTHS.items()}


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
    kw = {"bf16": True} if bf16 else {}
    legs = {"off": {}}
    if not parent:
        from sdumc_amd.teacher import TeacherTargets
        legs["teacher"] = {"teacher": TeacherTargets(**_tables(n, dev))}
    tr = {name: engine.FusedTrainer(flat.clone(), DIMS, lr=1e-5, seed=3, capacity=(B, T), **opts, **kw) for name, opts in legs.items()}
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
    out = {"tool": "teacher_bench", "n": n, "B": B, "steps": nb, "bf16": bool(bf16), "rounds": rounds, "parent_library": parent,
           "library": os.path.basename(os.environ.get("SDUMC_LIB", "tree"))}
    for name in legs:
        out[name] = {"ms_per_step": round(min(ms[name]) / nb, 5), "epoch_ms": [round(m, 3) for m in ms[name]]}
    base = ms["off"]
    out["off_spread"] = round(max(base) / min(base) - 1, 4)
    for name in list(legs)[1:]:
        d = sorted(y - x for x, y in zip(base, ms[name]))
        out[name]["extra_us_per_step_best"] = round((min(ms[name]) - min(base)) / nb * 1e3, 2)
        out[name]["extra_us_per_step_median_of_rounds"] = round(d[len(d) // 2] / nb * 1e3, 2)
    for name in legs:
        if not bool(torch.isfinite(tr[name].params).all()):
            raise SystemExit(f"{name}: non-finite parameters")
        if name != "off" and torch.equal(tr[name].params, tr["off"].params):      # (what the leg claims to have done)
            raise SystemExit(f"{name}: the parameters of the default run")
    if not parent:
        # a mean teacher at epoch granularity: one evaluation pass over the averaged weights per epoch
        mt = engine.FusedTrainer(flat.clone(), DIMS, lr=1e-5, seed=3, capacity=(B, T), ema_decay=0.999, **kw)
        mt.run_epoch(store, plan)
        mt.refresh_teacher(store, plan, weights="ema")
        torch.cuda.synchronize()
        wall = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            mt.refresh_teacher(store, plan, weights="ema")
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        mt.run_epoch(store, plan)
        torch.cuda.synchronize()
        if not bool(torch.isfinite(mt.params).all()):
            raise SystemExit("mean teacher: non-finite parameters")
        out["refresh"] = {"ms_per_epoch": round(min(wall), 3), "ms_per_batch": round(min(wall) / nb, 4), "epochs_ms": [round(w, 3) for w in wall]}
    return out


def stage(args):
    """plain fused steps with or without a teacher, for a profiler's kernel trace"""
    import torch
    import bench
    from sdumc_amd import engine
    on = _opt(args, "teacher", "off") == "on"
    B, steps = int(_opt(args, "B", 64)), int(_opt(args, "steps", 50))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    flat, _ = bench.init_flat_params(engine, dev)
    kw = {"bf16": True} if "bf16" in args else {}
    rows = None
    if on:
        from sdumc_amd.teacher import TeacherTargets
        kw["teacher"] = TeacherTargets(**_tables(4 * B, dev))
        rows = torch.randperm(4 * B, generator=torch.Generator().manual_seed(5))[:B].to(dev)
    ts = engine.TrainStep(flat, B, bench.T_MOSEI, bench.DIMS, seed=3, lr=1e-5, **kw)
    ts.set_batch(*[t.to(dev) for t in bench.synthetic_shard(B, 0, k=0)])
    if on:
        ts.use_teacher_rows(rows)
    for _ in range(steps):
        ts.launch()
    torch.cuda.synchronize()
    losses = ts.losses.cpu()
    if not bool(torch.isfinite(losses[:7]).all()):
        raise SystemExit("non-finite losses")
    return {"tool": "teacher_bench", "mode": "stage", "teacher": on, "B": B, "steps": steps, "bf16": "bf16" in args,
            "library": os.path.basename(os.environ.get("SDUMC_LIB", "tree")), "losses": [round(float(v), 6) for v in losses[:7]]}


def workaround(args):
    """the module loop with table[idx] as the three targets: what a stored teacher cost before the option"""
    import types
    import torch
    import bench
    from sdumc_amd.loss import MSELoss, RMSELoss, RnCLoss
    from sdumc_amd.model import get_models
    from sdumc_amd.optim import Adam
    B, steps = int(_opt(args, "B", 64)), int(_opt(args, "steps", 20))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    model = get_models(types.SimpleNamespace(input_dims=bench.DIMS, model="wengnet_mosei_mult_views_text_missing")).to(dev)
    model.train()
    opt = Adam(model.parameters(), lr=1e-5, weight_decay=1e-5)
    reg, rmse, rnc = MSELoss().to(dev), RMSELoss().to(dev), RnCLoss().to(dev)
    audio, text, video, feat4, vals = [t.to(dev) for t in bench.synthetic_shard(B, 0, k=0)]
    tables = _tables(4 * B, dev)
    idx = torch.randperm(4 * B, generator=torch.Generator().manual_seed(5))[:B].to(dev)
    w = (0.5, 0.5, 0.1, 0.7, 0.1, 0.8)

    def step():
        opt.zero_grad()
        v0, (f0, r0, t0, q0) = model([audio, text, video, False])
        v1, (f1, r1, t1, q1) = model([audio, feat4, video, True])
        terms = [reg(v0, vals), reg(v1, vals), rmse(t1, tables["text_hidden"][idx]), rmse(q1, tables["cross_text"][idx]),
                 rmse(f1, tables["fused"][idx]), rnc(torch.stack((r0, r1), dim=1), vals.unsqueeze(1))]
        loss = sum(wi * t for wi, t in zip(w, terms))
        loss.backward()
        opt.step()
        return loss

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        loss = step()
    e1.record()
    torch.cuda.synchronize()
    if not bool(torch.isfinite(loss.detach()).all()):
        raise SystemExit("workaround: non-finite loss")
    return {"tool": "teacher_bench", "mode": "workaround", "B": B, "steps": steps, "tensors": len(list(model.parameters())),
            "ms_per_step": round(e0.elapsed_time(e1) / steps, 4)}


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
    out = {"tool": "teacher_bench", "mode": "ab", "pairs": pairs, "parent_library": os.path.basename(parent_lib)}      # (the name alone: results are kept beside the sources)
    for key in ("n", "B", "steps", "bf16", "rounds"):
        out[key] = runs["tree"][0][key]
    best = {side: [r["off"]["ms_per_step"] for r in rs] for side, rs in runs.items()}
    out["parent_off_ms_per_step"] = best["parent"]
    out["tree_off_ms_per_step"] = best["tree_off"]
    out["tree_off_in_the_two_leg_process_ms_per_step"] = best["tree"]
    out["epoch_spread_inside_a_process"] = {side: [r["off_spread"] for r in rs] for side, rs in runs.items()}
    out["parent_process_spread"] = round(max(best["parent"]) / min(best["parent"]) - 1, 4)
    out["tree_process_spread"] = round(max(best["tree_off"]) / min(best["tree_off"]) - 1, 4)
    out["tree_off_over_parent_best"] = round(min(best["tree_off"]) / min(best["parent"]) - 1, 4)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    out["tree_off_over_parent_median"] = round(med(best["tree_off"]) / med(best["parent"]) - 1, 4)
    out["teacher"] = {"ms_per_step": [r["teacher"]["ms_per_step"] for r in runs["tree"]],
                      "extra_us_per_step_best": [r["teacher"]["extra_us_per_step_best"] for r in runs["tree"]],
                      "extra_us_per_step_median_of_rounds": [r["teacher"]["extra_us_per_step_median_of_rounds"] for r in runs["tree"]]}
    out["refresh"] = {"ms_per_epoch": [r["refresh"]["ms_per_epoch"] for r in runs["tree"]],
                      "ms_per_batch": [r["refresh"]["ms_per_batch"] for r in runs["tree"]]}
    return out


def main():
    args = sys.argv[1:]
    parent_lib = _opt(args, "ab", None)
    if "stage" in args:
        out = stage(args)
    elif "workaround" in args:
        out = workaround(args)
    else:
        out = ab(args, parent_lib) if parent_lib else measure(args)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
