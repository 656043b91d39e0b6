"""The cost of decoupled weight decay (TrainStep / FusedTrainer(decoupled_decay=True), sdumc_adamw_step, sdumc_adamw_multi,
sdumc_amd.optim.AdamW; csrc/adam.hip) over a synthetic C2-shaped resident store (bench.py: T_MOSEI, DIMS; tools/ema_bench.py's store,
permutation and batches -- a ragged epoch of 32 steps at n = 2048, B = 64): ms per step of run_epoch on four trainers over the same store,
  off          FusedTrainer()                                                (the default: launch for launch the step without the option),
  adamw        FusedTrainer(decoupled_decay=True)                            (the decoupled form of adam_kernel in Adam's place),
  adamw+rates  FusedTrainer(decoupled_decay=True, lr_scale={'*': 1.0})       (the decoupled form of adam_rates_kernel),
  adamw+ema    FusedTrainer(decoupled_decay=True, ema_decay=0.999)           (the decoupled EMA form of adam_kernel),
ALTERNATED: one warm-up epoch each, then `rounds` rounds of the four, HIP events around every epoch, one synchronisation after it; every
timed epoch is enqueued behind an untimed epoch of the same trainer, with the first event between the two, so the events bracket the
epoch's device time alone.  Best and all epochs of each leg, the extra microseconds per step over `off` (best over best, and the median
of the per-round differences; negative = faster) and the spread of the `off` epochs.
`kernels`: the launches alone over a bucket of the layout's live size, back to back on one stream between two events, microseconds per
call (the one-thread hyper launch in front of each included, as the C entries make it): every coupled entry and its decoupled form --
sdumc_adam_step / _rates / _ema without and with a table of ones, sdumc_adam_multi over the layout's live tensors -- then the drop-in
loop's step() over those tensors with gradients: sdumc_amd.optim.Adam, sdumc_amd.optim.AdamW, torch.optim.AdamW(foreach=True) and
torch.optim.AdamW(foreach=False), microseconds per step() by the same events (the host's share included: that is what a loop pays).
`parent` times `off` and the kernels alone -- ONE trainer in the process, no drop-in loops; with SDUMC_LIB=<the parent build's
libsdumc_hip.so> on that library (the decoupled entries are timed on whichever library has them, sdumc_ema_multi beside them).
ab=<that library>: the A/B itself -- `pairs` times a fresh process of `parent` on the parent's library and the same `parent` process
on this tree (like for like: one trainer, one leg; the two swap places from pair to pair), then this tree's four legs, one process at a
time (fresh child processes: the library is chosen when sdumc_amd is imported) -- and one JSON line with both sides' `off` epochs, the
run-to-run spread BETWEEN the parent's processes (best epoch of each: the yardstick for "off costs nothing"), tree over parent, the
tree's legs, and every kernel form of the two like-for-like processes side by side with the spread between the parent's processes (a
decoupled form the parent's library lacks stands beside its coupled kernel of the same form).
usage: python tools/adamw_bench.py [n=2048] [B=64] [bf16] [rounds=5] [parent] [ab=<parent .so>] [pairs=3]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DECAY, WD = 0.999, 1e-2
LEGS = {"off": {}, "adamw": {"decoupled_decay": True}, "adamw+rates": {"decoupled_decay": True, "lr_scale": {"*": 1.0}},
        "adamw+ema": {"decoupled_decay": True, "ema_decay": DECAY}}
FORMS = ("adam_step", "adam_step_rates_ones", "adam_step_ema", "adam_step_ema_rates_ones", "adam_multi")


def _opt(args, key, default):
    return next((a.split("=", 1)[1] for a in args if a.startswith(key + "=")), default)


def _views(layout, flat):
    v = layout.views(flat)
    return [v[name].reshape(-1) for name in layout.live_names()]


def kernels(engine, layout, dev, parent, calls=200):
    """us per call of the launches alone, and of the drop-in loop's step()"""
    import torch
    from sdumc_amd import _lib, ops, optim
    n = layout.live
    p, g, m, v = (torch.randn(n, device=dev) * s for s in (0.02, 1e-4, 1e-4, 1e-4))
    v = v.abs()
    a = p.clone()
    hyper = torch.tensor([1e-5, 0.0, 0.0, 0.0], device=dev)
    lib, st = _lib.lib, _lib.current_stream()
    # the ctypes tables are built ONCE (building one per call would time the host, not the launch)
    ones = ops.rate_segments(engine.TensorRates(layout, lr_scale={"*": 1.0}).segments())
    ptrs = [t.data_ptr() for t in (p, g, m, v)]
    adam = (n, hyper.data_ptr(), 0.9, 0.999, 1e-8, WD, 1.0)
    full, gfull = torch.randn(layout.total, device=dev) * 0.02, torch.randn(layout.total, device=dev) * 1e-4
    params, grads = _views(layout, full), _views(layout, gfull)
    offs, o = [], 0
    for t in params:
        offs.append(o)
        o = (o + t.numel() + 3) & ~3
    mm, vv = torch.zeros(o, device=dev), torch.zeros(o, device=dev)
    msegs = ops.adam_segments(params, grads, offs)
    multi = (len(params), mm.data_ptr(), vv.data_ptr(), o, hyper.data_ptr(), 0.9, 0.999, 1e-8, WD, 1.0, st)
    chk = _lib.check
    runs = {"adam_step": lambda: chk(lib.sdumc_adam_step(*ptrs, *adam, st), "sdumc_adam_step"),
            "adam_step_rates_ones": lambda: chk(lib.sdumc_adam_step_rates(*ptrs, *adam, ones, len(ones), st), "sdumc_adam_step_rates"),
            "adam_step_ema": lambda: chk(lib.sdumc_adam_step_ema(*ptrs, *adam, None, 0, a.data_ptr(), DECAY, 0, st), "sdumc_adam_step_ema"),
            "adam_step_ema_rates_ones": lambda: chk(lib.sdumc_adam_step_ema(*ptrs, *adam, ones, len(ones), a.data_ptr(), DECAY, 0, st),
                                                    "sdumc_adam_step_ema"),
            "adam_multi": lambda: chk(lib.sdumc_adam_multi(msegs, *multi), "sdumc_adam_multi")}
    avg = full.clone()      # (kept: the table holds addresses)
    esegs = ops.ema_segments(_views(layout, avg), params)
    runs["ema_multi"] = lambda: chk(lib.sdumc_ema_multi(esegs, len(params), 1.0 - DECAY, st), "sdumc_ema_multi")
    if _lib.ADAMW_ABI:      # (whichever library has the decoupled entries: an A/B is then like for like on every form)
        w = lib.sdumc_adamw_step
        runs.update({"adamw_step": lambda: chk(w(*ptrs, *adam, None, 0, None, 0.0, 0, st), "sdumc_adamw_step"),
                     "adamw_step_rates_ones": lambda: chk(w(*ptrs, *adam, ones, len(ones), None, 0.0, 0, st), "sdumc_adamw_step"),
                     "adamw_step_ema": lambda: chk(w(*ptrs, *adam, None, 0, a.data_ptr(), DECAY, 0, st), "sdumc_adamw_step"),
                     "adamw_step_ema_rates_ones": lambda: chk(w(*ptrs, *adam, ones, len(ones), a.data_ptr(), DECAY, 0, st),
                                                              "sdumc_adamw_step"),
                     "adamw_multi": lambda: chk(lib.sdumc_adamw_multi(msegs, *multi), "sdumc_adamw_multi")})
    if not parent:
        def loop(cls, **kw):      # the drop-in loop's optimizer line over the live tensors, gradients in place
            ps = [torch.nn.Parameter(t.clone()) for t in params]
            for q, gr in zip(ps, grads):
                q.grad = gr.clone()
            return cls(ps, lr=1e-5, weight_decay=WD, **kw).step
        runs.update({"optim.Adam.step": loop(optim.Adam), "optim.AdamW.step": loop(optim.AdamW),
                     "torch.optim.AdamW(foreach=True).step": loop(torch.optim.AdamW, foreach=True),
                     "torch.optim.AdamW(foreach=False).step": loop(torch.optim.AdamW, foreach=False)})
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = {}
    for _ in range(2):      # (the second pass is the one kept)
        for name, call in runs.items():
            k = calls // 4 if "foreach=False" in name else calls
            call()
            e0.record()
            for _ in range(k):
                call()
            e1.record()
            torch.cuda.synchronize()
            out[name] = round(e0.elapsed_time(e1) / k * 1e3, 2)
    out["bucket_floats"] = n
    out["live_tensors"] = len(params)
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
    tr = {name: engine.FusedTrainer(flat.clone(), DIMS, lr=1e-5, seed=3, capacity=(B, T), weight_decay=WD, **LEGS[name], **kw)
          for name in legs}
    lay = engine.ParamLayout.get(*DIMS[:3])
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
    out = {"tool": "adamw_bench", "n": n, "B": B, "steps": nb, "bf16": bool(bf16), "rounds": rounds, "parent_library": parent,
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
        # what the legs claim to have done: the decoupled legs trained other parameters than the default run, the same ones with a
        # table of ones and with an average riding along
        if torch.equal(tr["adamw"].params, tr["off"].params):
            raise SystemExit("adamw: the parameters of the default run")
        for name in legs[2:]:
            if not torch.equal(tr[name].params, tr["adamw"].params):
                raise SystemExit(f"{name}: not the parameters of the adamw leg")
    out["kernels_us_per_call"] = kernels(engine, lay, dev, parent)
    return out


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
    out = {"tool": "adamw_bench", "mode": "ab", "pairs": pairs, "parent_library": os.path.abspath(parent_lib)}
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
    # every form both libraries have, like for like (the same one-trainer process on either side), with the spread between the parent's
    # processes; a decoupled form the parent lacks stands beside the parent's coupled kernel of the same form
    forms = {}
    for form in FORMS + tuple(f.replace("adam_", "adamw_", 1) for f in FORMS) + ("ema_multi",):
        tree = [r["kernels_us_per_call"][form] for r in runs["tree_off"]]
        beside = form if form in runs["parent"][0]["kernels_us_per_call"] else form.replace("adamw_", "adam_", 1)
        par = [r["kernels_us_per_call"][beside] for r in runs["parent"]]
        forms[form] = {"parent_form": beside, "parent_us": par, "tree_us": tree,
                       "parent_process_spread": round(max(par) / min(par) - 1, 4),
                       "tree_over_parent_best": round(min(tree) / min(par) - 1, 4),
                       "tree_over_parent_median": round(med(tree) / med(par) - 1, 4)}
    out["kernels"] = forms
    out["loop_step_us"] = {k: [r["kernels_us_per_call"][k] for r in runs["tree"]] for k in runs["tree"][0]["kernels_us_per_call"]
                           if k.endswith(".step")}
    return out


def main():
    args = sys.argv[1:]
    parent_lib = _opt(args, "ab", None)
    print(json.dumps(ab(args, parent_lib) if parent_lib else measure(args)), flush=True)


if __name__ == "__main__":
    main()
