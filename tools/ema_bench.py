"""The cost of averaged weights in the fused step (TrainStep / FusedTrainer(ema_decay=): the EMA forms of adam_kernel and
adam_rates_kernel, csrc/adam.hip) over a synthetic C2-shaped resident store (bench.py: T_MOSEI, DIMS; tools/rates_bench.py's store,
permutation and batches -- a ragged epoch of 32 steps at n = 2048, B = 64): ms per step of run_epoch on four trainers over the same store,
  off        FusedTrainer()                                              (the default: launch for launch the step without the option),
  ema        FusedTrainer(ema_decay=0.999)                               (the EMA form of adam_kernel in Adam's place),
  ema+rates  FusedTrainer(ema_decay=0.999, lr_scale={'*': 1.0})          (the EMA form of adam_rates_kernel),
  callback   FusedTrainer() with on_step = torch._foreach_lerp_ over per-tensor views of a second flat tensor
                                                                         (the workaround the option replaces: a second pass over the bucket),
ALTERNATED: one warm-up epoch each, then `rounds` rounds of the four, HIP events around every epoch, one synchronisation after it; every
timed epoch is enqueued behind an untimed epoch of the same trainer, with the first event between the two, so the events bracket the
epoch's device time alone.  Best and all epochs of each leg, the extra microseconds per step over `off` (best over best, and the median
of the per-round differences; negative = faster) and the spread of the `off` epochs.
`kernels`: the launches alone over a bucket of the layout's live size, back to back on one stream between two events, microseconds per
call: sdumc_adam_step (hyper + adam_kernel), sdumc_adam_step_ema without and with a table of ones (hyper + the EMA form),
sdumc_adam_step_rates with that table, and sdumc_ema_multi alone over the layout's live tensors (what the drop-in loop runs behind its
step).  Prints one JSON line.
`parent` times `off` alone -- ONE trainer in the process, no `kernels`; with SDUMC_LIB=<the parent build's libsdumc_hip.so> on that
library (it has no sdumc_adam_step_ema).
ab=<that library>: the A/B itself -- `pairs` times a fresh process of `parent` on the parent's library and the same `parent` process
on this tree (like for like: one trainer, one leg; the two swap places from pair to pair), then this tree's four legs, one process at a
time (fresh child processes: the library is chosen when sdumc_amd is imported) -- and one JSON line with both sides' `off` epochs, the run-to-run spread BETWEEN the
parent's processes (best epoch of each: the yardstick for "off costs nothing"), tree over parent, and the tree's legs.
usage: python tools/ema_bench.py [n=2048] [B=64] [bf16] [rounds=5] [parent] [ab=<parent .so>] [pairs=3]"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DECAY = 0.999
# the weight the step applies: fp32(1 - fp32(decay)) -- sdumc_step_cfg.ema_decay is an fp32 field; the callback gets the same one
W = ctypes.c_float(1.0 - ctypes.c_float(DECAY).value).value
LEGS = {"off": {}, "ema": {"ema_decay": DECAY}, "ema+rates": {"ema_decay": DECAY, "lr_scale": {"*": 1.0}}, "callback": {}}


def _opt(args, key, default):
    return next((a.split("=", 1)[1] for a in args if a.startswith(key + "=")), default)


def _views(layout, flat):
    """the live tensors of a flat buffer, as the callback and sdumc_ema_multi see them"""
    v = layout.views(flat)
    return [v[name].reshape(-1) for name in layout.live_names()]


def kernels(engine, layout, dev, calls=200):
    """us per call of the launches alone"""
    import torch
    from sdumc_amd import _lib, ops
    n = layout.live
    p, g, m, v = (torch.randn(n, device=dev) * s for s in (0.02, 1e-4, 1e-4, 1e-4))
    v = v.abs()
    a = p.clone()
    hyper = torch.tensor([1e-5, 0.0, 0.0, 0.0], device=dev)
    lib, st = _lib.lib, _lib.current_stream()
    # the ctypes tables are built ONCE (building one per call would time the host, not the launch)
    ones = ops.rate_segments(engine.TensorRates(layout, lr_scale={"*": 1.0}).segments())
    ptrs = [t.data_ptr() for t in (p, g, m, v)]
    adam = (n, hyper.data_ptr(), 0.9, 0.999, 1e-8, 1e-5, 1.0)
    full = torch.zeros(layout.total, device=dev)
    avg = full.clone()
    emas, params = _views(layout, avg), _views(layout, full)
    segs = ops.ema_segments(emas, params)
    w = W
    runs = {"adam_step": lambda: ops.adam_step(p, g, m, v, hyper),
            "adam_step_ema": lambda: _lib.check(lib.sdumc_adam_step_ema(*ptrs, *adam, None, 0, a.data_ptr(), DECAY, 0, st), "sdumc_adam_step_ema"),
            "adam_step_rates_ones": lambda: _lib.check(lib.sdumc_adam_step_rates(*ptrs, *adam, ones, len(ones), st), "sdumc_adam_step_rates"),
            "adam_step_ema_rates_ones": lambda: _lib.check(lib.sdumc_adam_step_ema(*ptrs, *adam, ones, len(ones), a.data_ptr(), DECAY, 0, st),
                                                           "sdumc_adam_step_ema"),
            "ema_multi": lambda: _lib.check(lib.sdumc_ema_multi(segs, len(emas), w, st), "sdumc_ema_multi"),
            "foreach_lerp": lambda: torch._foreach_lerp_(emas, params, w)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = {}
    for _ in range(2):      # (the second pass is the one kept)
        for name, call in runs.items():
            call()
            e0.record()
            for _ in range(calls):
                call()
            e1.record()
            torch.cuda.synchronize()
            out[name] = round(e0.elapsed_time(e1) / calls * 1e3, 2)
    out["bucket_floats"] = n
    out["live_tensors"] = len(emas)
    return out


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
    lay = engine.ParamLayout.get(*DIMS[:3])
    on_step = {name: None for name in legs}
    if not parent:
        # the workaround: a second flat tensor, per-tensor views of both, one foreach call behind every step
        avg = tr["callback"].params.clone()
        emas, params = _views(lay, avg), _views(lay, tr["callback"].params)
        on_step["callback"] = lambda i, losses: torch._foreach_lerp_(emas, params, W)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(name):
        tr[name].run_epoch(store, plan, on_step=on_step[name])
        e0.record()
        tr[name].run_epoch(store, plan, on_step=on_step[name])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for name in legs:
        tr[name].run_epoch(store, plan, on_step=on_step[name])
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(rounds):
        for name in legs:
            ms[name].append(timed(name))
    out = {"tool": "ema_bench", "n": n, "B": B, "steps": nb, "bf16": bool(bf16), "rounds": rounds, "parent_library": parent,
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
    if not parent:
        # what the legs claim to have done: every leg trained the default run's parameters bit for bit, and the fused average is the
        # callback's to rounding (the two contract their products differently)
        for name in legs[1:]:
            if not torch.equal(tr[name].params, tr["off"].params):
                raise SystemExit(f"{name}: not the parameters of the default run")
        if not torch.equal(tr["ema"].ema_params, tr["ema+rates"].ema_params):
            raise SystemExit("ema+rates: not the average of the ema leg")
        a, b = tr["ema"].ema_params[:lay.live], avg[:lay.live]
        if not bool(((a - b).abs() <= 1e-5 * (a.abs() + b.abs()) + 1e-9).all()) or torch.equal(a, tr["ema"].params[:lay.live]):
            raise SystemExit("ema: the fused average is not the callback's")
        out["kernels_us_per_call"] = kernels(engine, lay, dev)
    return out


def ab(args, parent_lib):
    """fresh child processes, one at a time: the parent's library and this tree, alternated"""
    pairs = int(_opt(args, "pairs", 3))
    rest = [a for a in args if not a.startswith(("ab=", "pairs=")) and a != "parent"]
    runs = {"parent": [], "tree_off": [], "tree": []}
    for i in range(pairs):
        # the two `off` processes swap places from pair to pair: whichever runs first after the four-leg process does not always belong
        # to the same side
        for side in (("parent", "tree_off") if i % 2 == 0 else ("tree_off", "parent")) + ("tree",):
            env = dict(os.environ)
            env.pop("SDUMC_LIB", None)
            if side == "parent":
                env["SDUMC_LIB"] = os.path.abspath(parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__)] + rest + (["parent"] if side != "tree" else [])
            text = subprocess.run(cmd, env=env, cwd=ROOT, check=True, stdout=subprocess.PIPE, timeout=600).stdout.decode()
            runs[side].append(json.loads(text.strip().splitlines()[-1]))
    out = {"tool": "ema_bench", "mode": "ab", "pairs": pairs, "parent_library": os.path.abspath(parent_lib)}
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
    med = lambda v: sorted(v)[len(v) // 2]
    out["tree_off_over_parent_median"] = round(med(best["tree_off"]) / med(best["parent"]) - 1, 4)
    for name in list(LEGS)[1:]:
        out[name] = {"ms_per_step": [r[name]["ms_per_step"] for r in runs["tree"]],
                     "extra_us_per_step_best": [r[name]["extra_us_per_step_best"] for r in runs["tree"]],
                     "extra_us_per_step_median_of_rounds": [r[name]["extra_us_per_step_median_of_rounds"] for r in runs["tree"]]}
    out["kernels_us_per_call"] = [r["kernels_us_per_call"] for r in runs["tree"]]
    return out


def main():
    args = sys.argv[1:]
    parent_lib = _opt(args, "ab", None)
    print(json.dumps(ab(args, parent_lib) if parent_lib else measure(args)), flush=True)


if __name__ == "__main__":
    main()
