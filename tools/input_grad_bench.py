"""Input-feature gradients at C2 (B = 64, T = (375, 32, 225, 32), widths 1024 / 4096 / 1024), fp32 storage (run on the GPU box):
  1. the two-stream NetCall backward with and without feature_grads, the two legs alternated (device events around the backward);
  2. per modality, sdumc_frame_dx alone against its two existing alternatives on the same operands:
       (a) sdumc_p3_split(dz) + sdumc_gemm_p3_nt on the transposed-packed weight, (b) sdumc_gemm_f32 NN,
     every timed launch on the next of several independent operand sets (together > 256 MB: nothing stays in the Infinity Cache),
     the candidates alternated; TF = 2 M N 256 / time, GB/s = the fp32 output's bytes / time.
The whole request is 28.7 GFLOP and 224 MB of fp32 output (audio 12.6, text 4.3, video 7.5, feat4 4.3 GFLOP).
usage: python tools/input_grad_bench.py [rounds, default 3]"""
import ctypes as C
import sys
import time

sys.path.insert(0, ".")
import torch
from sdumc_amd import _lib, engine, ops

lib = _lib.lib
dev = "cuda"
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 3
B, T, DIMS = 64, (375, 32, 225, 32), (1024, 4096, 1024, 4096)


def warm(fn, seconds=0.4):
    t0 = time.time()
    while time.time() - t0 < seconds:      # clocks up, code objects loaded
        fn()
    torch.cuda.synchronize()


def timeit(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us


class Rot:
    def __init__(self, fns):
        self.fns, self.i = fns, 0

    def __call__(self):
        self.fns[self.i % len(self.fns)]()
        self.i += 1


def spread(v):
    return f"{min(v):7.1f} .. {max(v):7.1f} us"


def kernel_level():
    torch.manual_seed(0)
    print(f"--- sdumc_frame_dx against (a) p3_split + gemm_p3_nt and (b) gemm_f32 NN; {ROUNDS} alternations ---")
    for name, M, N in (("audio", B * T[0], DIMS[0]), ("text", B * T[1], DIMS[1]), ("video", B * T[2], DIMS[2]), ("feat4", B * T[3], DIMS[3])):
        flops, out_bytes = 2.0 * M * N * 256, 4.0 * M * N
        nsets = max(3, int(300e6 / (out_bytes + 1024 * M)) + 1)
        W = torch.randn(256, N, device=dev) / 16
        Wf = ops.p3_split_frag_t(W)
        t_pack = timeit(lambda: ops.p3_split_frag_t(W, out=Wf), 20)
        fx, fa, fb, keep = [], [], [], []
        for _ in range(nsets):
            dz = torch.randn(M, 256, device=dev)
            Cx = torch.empty(M, N, device=dev)
            q = _lib.FrameDx()
            q.M, q.N, q.A, q.W, q.W_frag, q.C, q.ldw, q.ldc = M, N, dz.data_ptr(), W.data_ptr(), Wf.data_ptr(), Cx.data_ptr(), N, N
            A3 = torch.empty(M, 6 * 256, dtype=torch.uint8, device=dev)
            launch_a, _ = ops.gemm_p3_nt_call(A3, Wf, M, N, 256, C_out=Cx)
            keep.append((dz, Cx, q, A3))
            fx.append(lambda q=q: _lib.check(lib.sdumc_frame_dx(C.byref(q), _lib.current_stream()), "sdumc_frame_dx"))
            fa.append(lambda dz=dz, A3=A3, la=launch_a: (ops.p3_split(dz, out=A3), la()))
            fb.append(lambda dz=dz, Cx=Cx: ops.gemm(ops.NN, dz, W, M, N, 256, C_out=Cx))
        # the three forms agree (same arithmetic family for (a); (b) is the fp32-MFMA form)
        fx[0]()
        got = keep[0][1].clone()
        fa[0]()
        same_a = float((keep[0][1] - got).abs().max())
        fb[0]()
        same_b = float((keep[0][1] - got).abs().max())
        legs = {"frame_dx": Rot(fx), "(a) split + p3_nt": Rot(fa), "(b) gemm_f32 NN": Rot(fb)}
        for fn in legs.values():
            warm(fn)
        times = {k: [] for k in legs}
        reps = max(10, min(1000, int(0.3e6 / max(20.0, flops / 150e6))))
        for _ in range(ROUNDS):
            for k, fn in legs.items():
                times[k].append(timeit(fn, reps))
        print(f"{name:6s} M = {M:6d} N = {N:5d}  {flops / 1e9:5.2f} GFLOP  {out_bytes / 1e6:6.1f} MB out  ({nsets} operand sets, {reps} launches per leg; "
              f"weight pack {t_pack:.1f} us; max |frame_dx - (a)| {same_a:.2e}, - (b)| {same_b:.2e})")
        for k, v in times.items():
            best = min(v)
            print(f"    {k:20s} {spread(v)}   best: {flops / best / 1e6:6.1f} TF  {out_bytes / best / 1e3:7.1f} GB/s")
        del keep, fx, fa, fb, legs
        torch.cuda.empty_cache()


def network_level():
    from oracle import sdumc_oracle as O      # (seeded parameters only)
    print(f"--- two-stream NetCall backward at C2, with and without feature_grads; {ROUNDS} alternations ---")
    P = O.init_params(DIMS, seed=0)
    lay = engine.ParamLayout.get(*DIMS[:3])
    flat = torch.zeros(lay.total)
    for k, v in lay.views(flat).items():
        v.copy_(P[k])
    flat = flat.cuda()
    g = torch.Generator(device=dev).manual_seed(1)
    audio, text, video, feat4 = [torch.randn(B, T[i], DIMS[i], device=dev, generator=g) for i in range(4)]
    call = engine.NetCall(flat, audio, [text, feat4], video, True, engine.RngState(3, dev))
    outs = call.forward()
    douts = [torch.randn(o.shape, device=dev, generator=g) for o in outs]
    grads = torch.zeros(lay.live, device=dev)

    def leg(feature_grads, reps=20):
        tot = 0.0
        for _ in range(reps):
            call.forward()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call.backward(*douts, grads=grads, feature_grads=feature_grads)
            e1.record()
            torch.cuda.synchronize()
            tot += e0.elapsed_time(e1)
        return tot / reps * 1e3
    for fg in (None, True):
        leg(fg, 10)
    res = {"without": [], "with": []}
    for _ in range(ROUNDS):
        res["without"].append(leg(None))
        res["with"].append(leg(True))
    for k, v in res.items():
        print(f"    backward {k:8s} feature_grads: {spread(v)}")
    extra = min(res["with"]) - min(res["without"])
    print(f"    feature gradients cost {extra:.1f} us of the backward (best against best): 28.7 GFLOP, 224 MB -> "
          f"{28.7e3 / max(extra, 1e-3):.1f} TF, {224e3 / max(extra, 1e-3):.1f} GB/s beside the rest of the backward")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the GPU"
    kernel_level()
    network_level()
