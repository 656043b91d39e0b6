"""The cost, and the return, of per-tensor learning rates, decay and frozen tensors in the fused step (TrainStep / FusedTrainer(freeze=,
lr_scale=, decay_scale=): adam_rates_kernel in Adam's place, zero_segments_kernel in front of it, csrc/adam.hip; the skipped frame dW,
csrc/engine.hip) over a synthetic C2-shaped resident store (bench.py: T_MOSEI, DIMS; tools/grad_guard_bench.py's store, permutation
and batches -- a ragged epoch of 32 steps at n = 2048, B = 64): ms per step of run_epoch on four trainers over the same store,
  off     FusedTrainer()                                                    (the default: launch for launch the step without the options),
  ones    FusedTrainer(lr_scale={'*': 1.0})                                 (the same arithmetic through the rates kernel: its cost over adam_kernel),
  split   FusedTrainer(decay_scale={'*.bias': 0, '*.attention_context_vector': 0}, lr_scale={'frame_dim_reshape_*': 0.5})
                                                                            (the usual no-decay split and a smaller rate for the frame projections),
  freeze  FusedTrainer(freeze=('frame_dim_reshape_*',))                     (no frame dW, its segments zeroed, 1.57 M of 3.86 M elements not updated),
ALTERNATED: one warm-up epoch each, then `rounds` rounds of the four, HIP events around every epoch, one synchronisation after it; every
timed epoch is enqueued behind an untimed epoch of the same trainer, with the first event between the two, so the events bracket the
epoch's device time alone.  Best and all epochs of each leg, the extra microseconds per step over `off` (best over best, and the median
of the per-round differences; negative = faster) and the spread of the `off` epochs.
`kernels`: the launches alone over a bucket of the layout's live size, back to back on one stream between two events, microseconds per
call: sdumc_adam_step (hyper + adam_kernel), sdumc_adam_step_rates with the tables of `ones`, `split` and `freeze` (hyper +
adam_rates_kernel), sdumc_zero_segments with the table of `freeze`.  Prints one JSON line.
`parent` times `off` alone -- ONE trainer in the process, no `kernels`; with SDUMC_LIB=<the parent build's libsdumc_hip.so> on that
library (it has no sdumc_adam_step_rates).
ab=<that library>: the A/B itself -- `pairs` times a fresh process of `parent` on the parent's library, then the same `parent` process
on this tree (like for like: one trainer, one leg), then this tree's four legs, one process at a time (fresh child processes: the
library is chosen when sdumc_amd is imported) -- and one JSON line with both sides' `off` epochs, the run-to-run spread BETWEEN the
parent's processes (best epoch of each: the yardstick for "off costs nothing"), tree over parent, and the tree's legs.
usage: python tools/rates_bench.py [n=2048] [B=64] [bf16] [rounds=5] [parent] [ab=<parent .so>] [pairs=3]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = {"off": {}, "ones": {"lr_scale": {"*": 1.0}},
        "split": {"decay_scale": {"*.bias": 0.0, "*.attention_context_vector": 0.0}, "lr_scale": {"frame_dim_reshape_*": 0.5}},
        "freeze": {"freeze": ("frame_dim_reshape_*",)}}


def _opt(args, key, default):
    return next((a.split("=", 1)[1] for a in args if a.startswith(key + "=")), default)


def kernels(engine, layout, dev, calls=200):
    """us per call of the launches alone"""
    import torch
    from sdumc_amd import ops
    n = layout.live
    p, g, m, v = (torch.randn(n, device=dev) * s for s in (0.02, 1e-4, 1e-4, 1e-4))
    v = v.abs()
    hyper = torch.tensor([1e-5, 0.0, 0.0, 0.0], device=dev)
    from sdumc_amd import _lib
    lib, st = _lib.lib, _lib.current_stream()
    # the ctypes tables are built ONCE (83 entries each: building one per call would time the host, not the launch)
    tables = {name: engine.TensorRates(layout, **LEGS[name]).segments() for name in list(LEGS)[1:]}
    ctab = {name: ops.rate_segments(tb) for name, tb in tables.items()}
    ptrs = [t.data_ptr() for t in (p, g, m, v)]
    runs = {"adam_step": lambda: ops.adam_step(p, g, m, v, hyper)}
    for name, tb in ctab.items():
        runs["adam_step_rates_" + name] = lambda tb=tb: _lib.check(lib.sdumc_adam_step_rates(
            *ptrs, n, hyper.data_ptr(), 0.9, 0.999, 1e-8, 1e-5, 1.0, tb, len(tb), st), "sdumc_adam_step_rates")
    runs["zero_segments_freeze"] = lambda: _lib.check(lib.sdumc_zero_segments(ptrs[1], n, ctab["freeze"], len(ctab["freeze"]), st),
                                                      "sdumc_zero_segments")
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
    out["frozen_floats"] = sum(s[1] for s in tables["freeze"] if s[4])
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
    out = {"tool": "rates_bench", "n": n, "B": B, "steps": nb, "bf16": bool(bf16), "rounds": rounds, "parent_library": parent,
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
        # what the legs claim to have done: `ones` is the default run bit for bit, `freeze` left the frame projections alone
        if not torch.equal(tr["ones"].params, tr["off"].params):
            raise SystemExit("ones: not the parameters of the default run")
        lay = engine.ParamLayout.get(*DIMS[:3])
        for name, same in (("freeze", True), ("split", False), ("off", False)):
            w, w0 = lay.views(tr[name].params)["frame_dim_reshape_1.weight"], lay.views(flat)["frame_dim_reshape_1.weight"]
            if torch.equal(w, w0) != same:
                raise SystemExit(f"{name}: frame_dim_reshape_1.weight " + ("moved" if same else "did not move"))
        out["kernels_us_per_call"] = kernels(engine, lay, dev)
    return out


def ab(args, parent_lib):
    """fresh child processes, one at a time: the parent's library and this tree, alternated"""
    pairs = int(_opt(args, "pairs", 3))
    rest = [a for a in args if not a.startswith(("ab=", "pairs=")) and a != "parent"]
    runs = {"parent": [], "tree_off": [], "tree": []}
    for _ in range(pairs):
        for side in runs:
            env = dict(os.environ)
            env.pop("SDUMC_LIB", None)
            if side == "parent":
                env["SDUMC_LIB"] = os.path.abspath(parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__)] + rest + (["parent"] if side != "tree" else [])
            text = subprocess.run(cmd, env=env, cwd=ROOT, check=True, stdout=subprocess.PIPE, timeout=600).stdout.decode()
            runs[side].append(json.loads(text.strip().splitlines()[-1]))
    out = {"tool": "rates_bench", "mode": "ab", "pairs": pairs, "parent_library": os.path.abspath(parent_lib)}
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
