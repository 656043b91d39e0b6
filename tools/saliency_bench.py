"""Saliency epochs at C2 shapes (frame maxima 375 / 32 / 225 / 32, widths 1024 / 4096 / 1024 / 4096) on a synthetic resident store,
fp32 storage, read in place (run on the GPU box):
  1. sdumc_frame_saliency alone, per modality, on full C2 batches (B samples of ragged length, min_frac 0.25): every timed launch on
     the next of several independent operand sets (together > 256 MB: nothing stays in the Infinity Cache); bytes = what the kernel
     reads (both operands of every VALID frame, 4 bytes of row map per padded frame, the tables) and writes (8 bytes per valid frame);
  2. ms per batch of an epoch over N utterances in batches of B, the legs alternated, every leg ending in a synchronise:
       saliency_epoch, both streams  |  saliency_epoch, streams=('missing',)  |  the same epoch without the reduction launch (forward +
       the feature-gradient backwards alone)  |  eval_epoch.
Every shape is warmed by one epoch of every leg first.  Kernel times per launch inside the epoch come from a separate run under
rocprofv3 --kernel-trace --stats with `--profile` (one warm and one measured two-stream epoch, nothing else).
usage: python tools/saliency_bench.py [N, default 2048] [B, default 64] [--rounds R, default 3] [--profile]"""
import ctypes as C
import sys
import time

sys.path.insert(0, ".")
import torch
from sdumc_amd import _lib, engine, evaluate, saliency
from sdumc_amd.data import DeviceFeatureStore

lib = _lib.lib
args = [a for a in sys.argv[1:] if not a.startswith("--")]
N, B = (int(args[0]) if args else 2048), (int(args[1]) if len(args) > 1 else 64)
ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 3
TCAP, DIMS = (375, 32, 225, 32), (1024, 4096, 1024, 4096)
MODS = ("audio", "text", "video", "feat4")


def timeit(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us


def kernel_level(store):
    print(f"--- sdumc_frame_saliency alone, one modality per launch, B = {B}, in place through a row map; {ROUNDS} alternations ---")
    g = torch.Generator().manual_seed(2)
    legs, info, keep = {}, {}, []
    for k, m in enumerate(MODS):
        d = DIMS[k]
        rows = int(store.length[m].sum())
        dst = torch.empty(rows, 2, device="cuda")
        per_set = 4.0 * B * TCAP[k] * d * 2
        nsets = max(3, int(300e6 / per_set) + 1)
        fns, read, written = [], 0.0, 0.0
        for _ in range(nsets):
            ix = torch.randperm(N, generator=g)[:B]
            (Bk, T), idx = store.batch_shape(ix), ix.cuda()
            maps = [torch.zeros(Bk * t + 64, dtype=torch.int32, device="cuda") for t in T]
            labels = torch.empty(Bk, device="cuda")
            gd = store.gather_desc(idx.data_ptr(), Bk, T, None, labels, None, maps_out=maps)
            _lib.check(lib.sdumc_gather_batch(C.byref(gd), 0, _lib.current_stream()), "sdumc_gather_batch")
            grad = torch.randn(Bk * T[k] * d, device="cuda")
            p = (_lib.SaliencyDesc * 1)()
            p[0].grad, p[0].feat, p[0].row_map, p[0].store_rows = grad.data_ptr(), store.packed[m].data_ptr(), maps[k].data_ptr(), store.packed[m].shape[0]
            p[0].start, p[0].length, p[0].n_utt = store.start_d[m].data_ptr(), store.length_d[m].data_ptr(), N
            p[0].dst, p[0].dst_rows, p[0].B, p[0].T, p[0].d = dst.data_ptr(), rows, Bk, T[k], d
            valid = float(store.length[m][ix].sum())
            read += valid * d * 8 + 4.0 * Bk * T[k] + 20.0 * Bk
            written += valid * 8
            keep.append((idx, maps, grad, p))
            fns.append(lambda p=p, idx=idx: _lib.check(lib.sdumc_frame_saliency(p, 1, idx.data_ptr(), _lib.current_stream()), "sdumc_frame_saliency"))
        state = {"i": 0}

        def rot(fns=fns, state=state):
            fns[state["i"] % len(fns)]()
            state["i"] += 1
        legs[m], info[m] = rot, (read / nsets, written / nsets, nsets)
    for fn in legs.values():      # clocks up, code object loaded
        t0 = time.time()
        while time.time() - t0 < 0.3:
            fn()
        torch.cuda.synchronize()
    times = {m: [] for m in MODS}
    for _ in range(ROUNDS):
        for m, fn in legs.items():
            times[m].append(timeit(fn, 60))
    for m in MODS:
        rd, wr, nsets = info[m]
        best = min(times[m])
        print(f"    {m:6s} {min(times[m]):7.1f} .. {max(times[m]):7.1f} us   {rd / 1e6:6.1f} MB read, {wr / 1e3:6.1f} KB written per launch "
              f"({nsets} operand sets)   best: {(rd + wr) / best / 1e6:5.2f} TB/s")


class _NoReduce(saliency.Saliency):
    def _reduce(self, descs, idx_ptr, st):
        pass


def epoch_level(store, flat, profile):
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(N, generator=g)
    batches = [perm[o:o + B] for o in range(0, N, B)]
    plan = store.plan_epoch(batches)
    nb = len(batches)
    full, bare = saliency.Saliency(flat, DIMS), _NoReduce(flat, DIMS)
    ev = evaluate.Evaluator(flat, DIMS)
    out = {}
    legs = {"saliency_epoch, both streams": lambda: out.__setitem__("a", full.saliency_epoch(store, plan, out=out.get("a"))),
            "saliency_epoch, 'missing' alone": lambda: out.__setitem__("b", full.saliency_epoch(store, plan, streams=("missing",), out=out.get("b"))),
            "forward + 2 feature-grad backwards": lambda: out.__setitem__("c", bare.saliency_epoch(store, plan, out=out.get("c"))),
            "eval_epoch": lambda: out.__setitem__("d", ev.eval_epoch(store, plan, out=out.get("d")))}
    if profile:
        legs = dict(list(legs.items())[:1])
    for fn in legs.values():      # every shape of the epoch warmed: arenas grown, per-shape dims cached, code objects loaded
        fn()
    torch.cuda.synchronize()
    assert full._in_place(store)
    times = {k: [] for k in legs}
    for _ in range(1 if profile else ROUNDS):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / nb)
    print(f"--- epochs over N = {N} utterances in {nb} batches of {B}, in place; ms per batch, {ROUNDS} alternations ---")
    for k, v in times.items():
        print(f"    {k:36s} {min(v):7.3f} .. {max(v):7.3f} ms")
    if not profile:
        a, c, d = (min(times[k]) for k in ("saliency_epoch, both streams", "forward + 2 feature-grad backwards", "eval_epoch"))
        print(f"    the reduction launches cost {1e3 * (a - c):.1f} us per batch (2 launches); forward + backwards are {c / a * 100:.1f} % of the epoch, "
              f"the forward, gather and scatter alone (eval_epoch) {d / a * 100:.1f} %")
        assert bool(torch.isfinite(out["a"].maps["full"]["audio"]).all()) and int((out["a"].seen != 0).sum()) == N


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the GPU"
    from oracle import sdumc_oracle as O      # (seeded parameters only)
    profile = "--profile" in sys.argv
    P = O.init_params(DIMS, seed=0)
    lay = engine.ParamLayout.get(*DIMS[:3])
    flat = torch.zeros(lay.total)
    for k, v in lay.views(flat).items():
        v.copy_(P[k])
    store = DeviceFeatureStore.synthetic(N, TCAP, DIMS, seed=7, min_frac=0.25, planes=True)
    print(f"store: {N} utterances, {store.nbytes / 1e9:.2f} GB with planes")
    if not profile:
        kernel_level(store)
    epoch_level(store, flat.cuda(), profile)
