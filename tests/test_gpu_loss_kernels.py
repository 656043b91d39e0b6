"""GPU kernel-level tests of loss.hip: Rank-N-Contrast on each of its routes (the direct row kernel, the sorted kernel, the direct
body inside the fused two-launch losses), and the small MSE / SSD / RMSE kernels, through the C ABI against float64.

Conventions (those of tests/test_gpu_elementwise.py, whose `Out` and `within` are used here):
  * every output -- the RnC workspace included -- has a guard band behind it and is pre-filled with NaN, or with a known pattern
    where the contract is "accumulate"; the guard must come back untouched and "writes nothing" means the fill is still there;
  * Rank-N-Contrast is compared ELEMENT BY ELEMENT, intermediates first: dist, rowloss and G are read back from the workspace
    (layout dist | e | ldiff | invD | G | rowmax | rowloss) and held to the bars derived in tests/loss_bars.py from the loop
    lengths; no element is excluded; diagonals are exactly 0;
  * membership is fp32 torch's (oracle/rnc_reference.py); tests/test_oracle_vs_golden.py shows that ONE differing membership
    decision moves some element of rowloss or G by more than 4 bars in the threshold-straddling cases used here;
  * what the code promises as "the same bits" (scalar vs vector distance loop, _rep vs materialised labels, partial rows vs the full
    call, fused vs separate launches) is asserted with torch.equal.
Each test prints `LOSSERR <case> <quantity>=<worst error / bar> ...` before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle.rnc_reference import rnc_reference
from tests.loss_bars import U, rnc_case, rnc_df_ref_and_bar, rnc_loss_bar, rnc_row_bars
from tests.test_gpu_elementwise import EINVAL, GUARD, L, Out, dev, within  # noqa: F401  (L: the library fixture)

pytestmark = pytest.mark.gpu

D, H, NQ = 256, 128, 7
NAN = float("nan")


def untouched(out):
    """True when every element of an Out that was pre-filled with NaN is still NaN (and its guard band intact)."""
    return bool(torch.isnan(out.get()).all())


def ratio(got, ref, bar):
    """Worst |got - ref| / bar; an element with bar 0 must match exactly (ratio 0 or inf); a NaN in got gives inf."""
    err = (got.double() - ref.double().reshape(got.shape)).abs()
    bar = bar.double().reshape(got.shape) if isinstance(bar, torch.Tensor) else torch.full_like(err, float(bar))
    r = torch.where(err == 0, torch.zeros_like(err), err / bar)
    return float(r.nan_to_num(nan=float("inf")).max())


def report(case, **ratios):
    print("LOSSERR " + case + " " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))


class RncRun:
    """One call of sdumc_rnc_fwd_bwd / _rep into NaN-filled, guarded buffers; .dist .G .rowloss .loss .df on the host afterwards."""

    def __init__(self, L, f, y, t, weight=1.0, row0=0, rows_local=None, rep=False, offset=False, want_df=True, expect=0):
        n, dim = f.shape
        self.n, self.dim = n, dim
        rows_local = n if rows_local is None else rows_local
        if offset:                       # the same floats 4 bytes further on: no longer 16-byte aligned -> the scalar distance loop
            buf = torch.zeros(n * dim + 1, device="cuda")
            buf[1:] = f.reshape(-1).cuda()
            self.fd, fptr = buf, buf.data_ptr() + 4
            assert buf.data_ptr() % 16 == 0
        else:
            self.fd = dev(f)
            fptr = self.fd.data_ptr()
            assert fptr % 16 == 0
        self.fptr = fptr
        yd = dev(y[:n // 2] if rep else y)
        nbytes = L.lib.sdumc_rnc_workspace_bytes(n)
        assert nbytes == (5 * n * n + 2 * n) * 4
        self.ws, self.loss_out, self.df_out = Out(nbytes // 4), Out(1), Out(max(1, rows_local * dim))
        fn = L.lib.sdumc_rnc_fwd_bwd_rep if rep else L.lib.sdumc_rnc_fwd_bwd
        self.rc = fn(fptr, yd.data_ptr(), n, dim, t, weight, row0, rows_local, self.loss_out.ptr(),
                     self.df_out.ptr() if want_df else None, self.ws.ptr(), None)
        assert self.rc == expect, f"return code {self.rc}"
        if expect != 0:
            return
        w = self.ws.get()
        nn = n * n
        self.dist, self.G = w[:nn].reshape(n, n), w[4 * nn:5 * nn].reshape(n, n)
        self.rowloss = w[5 * nn + n:]
        self.loss = self.loss_out.get()
        self.df = self.df_out.get()[:rows_local * dim].reshape(rows_local, dim)

    def same_bits(self, other, what):
        for name in ("dist", "G", "rowloss", "loss", "df"):
            assert torch.equal(getattr(self, name), getattr(other, name)), f"{what}: {name} differs in its bits"


@functools.lru_cache(maxsize=None)
def case_and_reference(n, dim, kind, t, dup=False):
    """Inputs and the float64 reference with its bars, computed once per case and shared (never modified)."""
    f, y = rnc_case(n, dim, kind, t, dup=dup)
    ref = rnc_reference(f, y, t)
    return f, y, ref, rnc_row_bars(ref, dim, t)


def check_full(L, n, dim, kind, t, weight, dup=False, **run):
    """Run one full call and hold dist, rowloss, G, loss and df to their bars.  Returns (RncRun, {quantity: worst error / bar})."""
    f, y, ref, (b_dist, b_rl, b_G) = case_and_reference(n, dim, kind, t, dup)
    r = RncRun(L, f, y, t, weight=weight, **run)
    df_ref, b_df = rnc_df_ref_and_bar(ref.G, ref.dist, b_G, f.double(), list(range(n)), t, weight)
    out = {"dist": ratio(r.dist, ref.dist, b_dist), "rowloss": ratio(r.rowloss, ref.rowloss, b_rl), "G": ratio(r.G, ref.G, b_G),
           "loss": ratio(r.loss, ref.loss.reshape(1), rnc_loss_bar(ref, b_rl)), "df": ratio(r.df, df_ref, b_df)}
    case = f"n={n} dim={dim} labels={kind} t={t:g} w={weight:g}" + (" dup" if dup else "") + "".join(f" {k}" for k, v in run.items() if v)
    report(case, **out)
    assert torch.equal(r.dist.diagonal(), torch.zeros(n)), case + ": dist_ii is exactly 0"
    assert torch.equal(r.G.diagonal(), torch.zeros(n)), case + ": G_ii is exactly 0"
    if dup:
        assert float(r.dist[1, 2]) == 0.0 and float(r.dist[0, n // 2]) == 0.0 and float(r.dist[n // 2, 0]) == 0.0
    for k, v in out.items():
        assert v <= 1.0, f"{case}: {k} is {v:.3g} x its bar"
    return r, out


# every n, every dim, every kind of labels and every temperature of the list at least once on each path; weight != 1 throughout
DIRECT = [(2, 64, "cont", 2.0), (2, 1, "straddle", 7.0), (3, 1, "cont", 0.5), (3, 100, "straddle", 2.0), (5, 3, "ties", 7.0),
          (5, 36, "equal", 2.0), (96, 64, "straddle", 2.0), (96, 36, "cont", 0.5), (96, 100, "equal", 7.0), (96, 3, "ties", 2.0),
          (255, 100, "ties", 2.0), (255, 3, "straddle", 7.0), (255, 64, "cont", 0.5), (256, 64, "cont", 2.0),
          (256, 36, "straddle", 0.5), (256, 1, "ties", 7.0), (256, 100, "equal", 2.0)]
SORTED = [(257, 64, "straddle", 2.0), (257, 36, "cont", 0.5), (258, 64, "straddle", 2.0), (258, 3, "ties", 7.0),
          (258, 1, "cont", 2.0), (511, 64, "ties", 2.0), (511, 100, "equal", 0.5), (511, 36, "straddle", 7.0),
          (1024, 64, "straddle", 2.0)]


@pytest.mark.parametrize("n,dim,kind,t", DIRECT + SORTED)
def test_rnc_against_fp64(L, n, dim, kind, t):
    """dist, rowloss, G, loss and df element by element against float64 (bars: tests/loss_bars.py).  n <= 256 is the direct row
    kernel (n = 2, 3, 5: most threads idle; 255 | 256: the last sizes before the switch), n >= 257 the sorted one (257, 511: block_scan
    threads without an element; 258: the first even size; 1024: four elements per thread).  dim = 36 ends the 8-wide vector loop in its
    tail (9 groups), dim = 100 takes 25 groups, dim = 1 and 3 the scalar loop."""
    check_full(L, n, dim, kind, t, 0.8)


@pytest.mark.parametrize("n,kind", [(96, "straddle"), (258, "straddle"), (5, "cont"), (257, "ties")])
def test_rnc_scalar_loop_is_bit_equal_to_vector_loop(L, n, kind):
    """dim = 64 from a pointer 4 bytes off 16-byte alignment takes the scalar distance loop; loss.hip says it sums in the same order,
    so everything downstream has the same bits -- and the offset run meets the fp64 bars on its own."""
    aligned, _ = check_full(L, n, 64, kind, 2.0, 0.8)
    off, _ = check_full(L, n, 64, kind, 2.0, 0.8, offset=True)
    assert off.fptr % 16 == 4
    off.same_bits(aligned, f"n={n}: scalar (offset) vs vector (aligned) distance loop")


@pytest.mark.parametrize("n", [96, 258])
def test_rnc_duplicate_feature_rows(L, n):
    """Two pairs of identical rows (one of them a sample whose two views coincide): dist = 0 off the diagonal, whose df terms are
    dropped (coef = 0) instead of dividing by zero; e = 1 there, the largest term of every sum it is a member of."""
    r, _ = check_full(L, n, 64, "straddle", 2.0, 0.8, dup=True)
    assert bool(torch.isfinite(r.df).all())


@pytest.mark.parametrize("n,dim,kind", [(2, 64, "cont"), (96, 64, "straddle"), (256, 36, "straddle"), (258, 64, "straddle"),
                                        (1024, 64, "straddle")])
def test_rnc_rep_is_bit_equal_to_materialised_labels(L, n, dim, kind):
    """sdumc_rnc_fwd_bwd_rep reads labels[j % (n/2)]; the same labels written out twice give the same bits, on both paths."""
    t = 2.0 if dim == 64 else 0.5
    f, y = rnc_case(n, dim, kind, t)
    assert torch.equal(y[:n // 2], y[n // 2:])
    full = RncRun(L, f, y, t, weight=0.8)
    rep = RncRun(L, f, y, t, weight=0.8, rep=True)
    rep.same_bits(full, f"n={n}: _rep vs materialised labels")


@pytest.mark.parametrize("n", [96, 258])
def test_rnc_partial_rows(L, n):
    """A data-parallel rank asks for the df rows it owns: (row0, rows_local) = (0, n/2), (n/2, n/2), (n-1, 1), through
    sdumc_rnc_fwd_bwd and through sdumc_rnc_dfeat_rows on the full call's workspace.  Each is the matching slice of the full call bit
    for bit (and so meets the fp64 bars the full call is held to), nothing is written behind rows_local * dim, and the workspace and the
    loss do not depend on the rows asked for.  dfeats = NULL: G is not written, the loss is."""
    dim, t, w = 64, 2.0, 0.8
    f, y = rnc_case(n, dim, "straddle", t)
    full, _ = check_full(L, n, dim, "straddle", t, w)
    for row0, rows in ((0, n // 2), (n // 2, n // 2), (n - 1, 1)):
        what = f"n={n} rows [{row0}, {row0 + rows})"
        part = RncRun(L, f, y, t, weight=w, row0=row0, rows_local=rows)
        assert torch.equal(part.df, full.df[row0:row0 + rows]), what
        for name in ("dist", "G", "rowloss", "loss"):
            assert torch.equal(getattr(part, name), getattr(full, name)), f"{what}: {name}"
        out = Out(rows * dim)
        assert L.lib.sdumc_rnc_dfeat_rows(full.fd.data_ptr(), n, dim, t, w, row0, rows, out.ptr(), full.ws.ptr(), None) == 0
        assert torch.equal(out.get(rows, dim), full.df[row0:row0 + rows]), what + " (sdumc_rnc_dfeat_rows)"
    for kw in ({"want_df": False}, {"rows_local": 0}):
        nograd = RncRun(L, f, y, t, weight=w, **kw)
        assert bool(torch.isnan(nograd.G).all()), "no gradient asked for: G stays unwritten"
        assert untouched(nograd.df_out)
        assert torch.equal(nograd.loss, full.loss) and torch.equal(nograd.rowloss, full.rowloss) and torch.equal(nograd.dist, full.dist)
    out = Out(dim)
    for bad in ((n, 1), (-1, 1), (0, 0), (n - 1, 2)):
        assert L.lib.sdumc_rnc_dfeat_rows(full.fd.data_ptr(), n, dim, t, w, bad[0], bad[1], out.ptr(), full.ws.ptr(), None) == EINVAL
    assert untouched(out)


def test_rnc_direct_and_sorted_side_by_side(L):
    """The two formulations never see the same n (the switch is at 256 | 257 and the C ABI offers no way to force one), so they cannot be
    compared with each other directly: the SAME rows -- 258 of them for the sorted kernel, the first 256 of them for the direct one -- are
    each held to float64, and the two error-to-bar ratios are printed side by side."""
    dim, t, w = 64, 2.0, 0.8
    f, y = rnc_case(258, dim, "straddle", t)
    res = {}
    for name, rows in (("direct n=256", torch.arange(256)), ("sorted n=258", torch.arange(258))):
        fs, ys = f[rows].contiguous(), y[rows].contiguous()
        n = len(rows)
        ref = rnc_reference(fs, ys, t)
        b_dist, b_rl, b_G = rnc_row_bars(ref, dim, t)
        r = RncRun(L, fs, ys, t, weight=w)
        df_ref, b_df = rnc_df_ref_and_bar(ref.G, ref.dist, b_G, fs.double(), list(range(n)), t, w)
        res[name] = {"dist": ratio(r.dist, ref.dist, b_dist), "rowloss": ratio(r.rowloss, ref.rowloss, b_rl),
                     "G": ratio(r.G, ref.G, b_G), "loss": ratio(r.loss, ref.loss.reshape(1), rnc_loss_bar(ref, b_rl)),
                     "df": ratio(r.df, df_ref, b_df)}
        report("side-by-side " + name, **res[name])
    for name, out in res.items():
        for k, v in out.items():
            assert v <= 1.0, f"{name}: {k} is {v:.3g} x its bar"


@pytest.mark.parametrize("n", [2048, 2049])
def test_rnc_large_n_sampled_anchors(L, n):
    """n = 2048: the sorted kernel with (64 + 8 * 2048 + 8) * 4 = 65 824 B of dynamic LDS, more than 64 KB; n = 2049: back to the direct
    kernel (41 236 B).  Rows of dist, rowloss and G of 8 anchors -- the smallest and the largest label among them, whose windows end at
    an end of the sorted order -- against float64 with the usual bars; the loss against the float64 sum of the device's own rowloss (n u
    for the sum, 4u for the scale); the df rows of the same anchors against float64 of the device's own G and dist, which leaves only
    the df kernel's rounding."""
    dim, t, w = 64, 2.0, 0.8
    f, y = rnc_case(n, dim, "straddle", t)
    anchors = sorted({int(y.argmin()), int(y.argmax()), 0, n // 2 - 1, n // 2, n - 1, (5 * n) // 7, n // 3})
    assert len(anchors) == 8
    ref = rnc_reference(f, y, t, anchors=anchors)
    b_dist, b_rl, b_G = rnc_row_bars(ref, dim, t)
    r = RncRun(L, f, y, t, weight=w)
    at = torch.tensor(anchors)
    c = 1.0 / (n * (n - 1))
    rl64 = r.rowloss.double()
    loss64 = -rl64.sum() * c
    df_ref, b_df = rnc_df_ref_and_bar(r.G.double(), r.dist.double(), None, f.double(), anchors, t, w)
    out = {"dist": ratio(r.dist[at], ref.dist, b_dist), "rowloss": ratio(r.rowloss[at], ref.rowloss, b_rl),
           "G": ratio(r.G[at], ref.G, b_G),
           "loss": ratio(r.loss, loss64.reshape(1), float(c * n * U * rl64.abs().sum() + 4 * U * abs(loss64))),
           "df": ratio(r.df[at], df_ref, b_df)}
    report(f"n={n} dim={dim} labels=straddle t=2 w=0.8 (8 anchors)", **out)
    assert bool(torch.isfinite(r.rowloss).all()) and bool(torch.isfinite(r.df).all()) and bool(torch.isfinite(r.G).all())
    assert torch.equal(r.dist.diagonal(), torch.zeros(n)) and torch.equal(r.G.diagonal(), torch.zeros(n))
    for k, v in out.items():
        assert v <= 1.0, f"n={n}: {k} is {v:.3g} x its bar"


class RncRunRaw:
    """sdumc_rnc_fwd_bwd with n and dim that do not match the buffers (for rejections only; the buffers are those of a 6 x 4 case)."""

    def __init__(self, L, f, y, n, dim, t):
        self.fd, self.yd = dev(f), dev(y)
        self.ws, self.loss_out, self.df_out = Out(L.lib.sdumc_rnc_workspace_bytes(6) // 4), Out(1), Out(24)
        self.rc = L.lib.sdumc_rnc_fwd_bwd(self.fd.data_ptr(), self.yd.data_ptr(), n, dim, t, 1.0, 0, n, self.loss_out.ptr(), self.df_out.ptr(),
                                          self.ws.ptr(), None)


def test_rnc_rejects_bad_arguments(L):
    """n = 1, dim = 0, temperature = 0, row0 + rows_local > n, negative rows, and odd n for _rep: EINVAL before anything is launched --
    loss, df and the workspace keep their NaN fill."""
    f, y = rnc_case(6, 4, "cont", 2.0)
    for kw, shape in (({}, (1, 4)), ({}, (6, 0)), ({"t": 0.0}, (6, 4)), ({"t": -1.0}, (6, 4)), ({"row0": 4, "rows_local": 3}, (6, 4)),
                      ({"row0": -1, "rows_local": 2}, (6, 4)), ({"rows_local": -1}, (6, 4)), ({"rep": True}, (5, 4))):
        kw = dict(kw)
        t = kw.pop("t", 2.0)
        n, dim = shape
        if dim == 0:                     # a tensor without elements has no pointer worth passing: hand over the 6 x 4 buffers
            r = RncRunRaw(L, f, y, n, 0, t)
        else:
            r = RncRun(L, f[:n, :dim].contiguous(), y[:n].contiguous(), t, expect=EINVAL, **kw)
        assert r.rc == EINVAL, (kw, shape)
        assert untouched(r.ws) and untouched(r.loss_out) and untouched(r.df_out), (kw, shape)


# ---- the fused two-launch losses of the training step ------------------------------------------------------------------------------
def _bind_fused(L):
    fused = L.lib.sdumc_losses_fused_
    fused.restype = C.c_int
    fused.argtypes = ([C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_float, C.POINTER(C.c_float)] + [C.c_void_p] * 9 +
                      [C.c_double, C.c_double, C.c_int32, C.c_void_p])
    crit = L.lib.sdumc_distill_crit_
    crit.restype = C.c_int
    crit.argtypes = ([C.c_int32, C.c_float] + [C.c_void_p] * 5 + [C.POINTER(C.c_float)] + [C.c_void_p] * 7 + [C.c_int32, C.c_void_p])
    return fused, crit


class LossBuffers:
    def __init__(self, L, B, rd):
        n = 2 * B
        self.d_vals, self.d_th, self.d_ct, self.d_z, self.d_rnc = Out(n), Out(n * D), Out(n * NQ * H), Out(n * H), Out(n * rd)
        self.losses = Out(8)
        self.dws = Out(L.lib.sdumc_distill_workspace_bytes(B) // 4)
        self.rws = Out(L.lib.sdumc_rnc_workspace_bytes(n) // 4)

    def all(self):
        return {k: v for k, v in vars(self).items() if isinstance(v, Out)}


@pytest.mark.parametrize("distill", [0, 1, 2], ids=["rmse", "cosine", "kl"])
@pytest.mark.parametrize("B,rd", [(1, 64), (3, 36), (17, 3), (128, 64)])
def test_losses_fused_is_bit_equal_to_separate_launches(L, B, rd, distill):
    """sdumc_losses_fused_ (what a single-GPU training step runs) promises the bits of sdumc_distill_crit_ + sdumc_rnc_fwd_bwd_rep:
    losses[1..6], every gradient buffer and the RnC intermediates are compared with torch.equal; losses[0] and [7] are not its to
    write.  The Adam bias correction it folds in: hyper = {lr, t, lr / (1 - beta1^t), sqrt(1 - beta2^t)} advanced by one step, equal
    to the fp32 rounding of the double-precision formulas, over three consecutive calls.  B = 1 is n = 2; B = 128 is n = 256, the
    largest it takes."""
    fused, crit = _bind_fused(L)
    g = torch.Generator().manual_seed(100 * B + distill)
    n, t = 2 * B, 2.0
    vals, labels = torch.randn(n, generator=g), (torch.rand(B, generator=g) * 6 - 3).round(decimals=1)
    th, ct, z = torch.randn(n, D, generator=g), torch.randn(n, NQ, H, generator=g), torch.randn(n, H, generator=g)
    rf = 0.3 * torch.randn(n, rd, generator=g)
    vd, ld, thd, ctd, zd, rfd = (dev(x) for x in (vals, labels, th, ct, z, rf))
    w6 = (C.c_float * 6)(0.5, 0.5, 0.1, 0.7, 0.13, 0.8)
    lr, b1, b2 = 1e-4, 0.9, 0.999
    hyper = Out(4, fill=torch.tensor([lr, 0.0, NAN, NAN]))
    a = LossBuffers(L, B, rd)
    for step in (1, 2, 3):
        assert fused(B, vd.data_ptr(), ld.data_ptr(), thd.data_ptr(), ctd.data_ptr(), zd.data_ptr(), rfd.data_ptr(), rd, t, w6,
                     a.d_vals.ptr(), a.d_th.ptr(), a.d_ct.ptr(), a.d_z.ptr(), a.d_rnc.ptr(), a.losses.ptr(), a.dws.ptr(), a.rws.ptr(),
                     hyper.ptr(), b1, b2, distill, None) == 0
        want = [np.float32(lr), np.float32(step), np.float32(float(np.float32(lr)) / (1.0 - b1 ** step)), np.float32(np.sqrt(1.0 - b2 ** step))]
        assert hyper.get().tolist() == [float(x) for x in want], f"hyper after step {step}"
    b = LossBuffers(L, B, rd)
    assert crit(B, float(B), vd.data_ptr(), ld.data_ptr(), thd.data_ptr(), ctd.data_ptr(), zd.data_ptr(), w6, None, b.d_vals.ptr(),
                b.d_th.ptr(), b.d_ct.ptr(), b.d_z.ptr(), b.losses.ptr(), b.dws.ptr(), distill, None) == 0
    assert L.lib.sdumc_rnc_fwd_bwd_rep(rfd.data_ptr(), ld.data_ptr(), n, rd, t, float(w6[5]), 0, n, b.losses.ptr() + 6 * 4, b.d_rnc.ptr(),
                                       b.rws.ptr(), None) == 0
    la, lb = a.losses.get(), b.losses.get()
    assert bool(torch.isnan(la[0])) and bool(torch.isnan(la[7])), "losses[0] and losses[7] belong to the caller"
    assert bool(torch.isfinite(la[1:7]).all())
    assert torch.equal(la[1:7], lb[1:7]), f"losses: fused {la[1:7].tolist()} separate {lb[1:7].tolist()}"
    for name in ("d_vals", "d_th", "d_ct", "d_z", "d_rnc"):
        ga, gb = getattr(a, name).get(), getattr(b, name).get()
        assert bool(torch.isfinite(ga).all()), name
        assert torch.equal(ga, gb), f"{name}: {int((ga != gb).sum())} of {ga.numel()} elements differ"
    nn = n * n
    wa, wb = a.rws.get(), b.rws.get()
    for name, lo, hi in (("dist", 0, nn), ("G", 4 * nn, 5 * nn), ("rowloss", 5 * nn + n, 5 * nn + 2 * n)):
        assert torch.equal(wa[lo:hi], wb[lo:hi]), f"RnC workspace {name}"
    # ... and the separate RnC launches are the ones test_rnc_against_fp64 holds to float64: one fp64 check of the fused result too
    y2 = labels.repeat(2)
    ref = rnc_reference(rf, y2, t)
    b_dist, b_rl, b_G = rnc_row_bars(ref, rd, t)
    df_ref, b_df = rnc_df_ref_and_bar(ref.G, ref.dist, b_G, rf.double(), list(range(n)), t, float(w6[5]))
    out = {"rnc_loss": ratio(la[6:7], ref.loss.reshape(1), rnc_loss_bar(ref, b_rl)), "d_rnc": ratio(a.d_rnc.get(n, rd), df_ref, b_df)}
    report(f"fused B={B} rd={rd} distill={distill}", **out)
    assert max(out.values()) <= 1.0, out


def test_losses_fused_declines_what_it_does_not_take(L):
    """B = 129 (n = 258 belongs to the sorted kernel) returns 1 -- "not mine, run the separate launches" -- and writes nothing; an
    unknown criterion is EINVAL."""
    fused, _ = _bind_fused(L)
    B, rd = 129, 64
    n = 2 * B
    vd, ld, thd, ctd, zd, rfd = (torch.ones(k, device="cuda") for k in (n, B, n * D, n * NQ * H, n * H, n * rd))
    w6 = (C.c_float * 6)(0.5, 0.5, 0.1, 0.7, 0.13, 0.8)
    hyper = Out(4, fill=torch.tensor([1e-4, 5.0, 0.25, 0.5]))
    a = LossBuffers(L, B, rd)
    for distill, want in ((0, 1), (1, 1), (2, 1), (3, EINVAL), (-1, EINVAL)):
        assert fused(B, vd.data_ptr(), ld.data_ptr(), thd.data_ptr(), ctd.data_ptr(), zd.data_ptr(), rfd.data_ptr(), rd, 2.0, w6,
                     a.d_vals.ptr(), a.d_th.ptr(), a.d_ct.ptr(), a.d_z.ptr(), a.d_rnc.ptr(), a.losses.ptr(), a.dws.ptr(), a.rws.ptr(),
                     hyper.ptr(), 0.9, 0.999, distill, None) == want
    for name, out in a.all().items():
        assert untouched(out), name
    assert hyper.get().tolist() == [float(np.float32(1e-4)), 5.0, 0.25, 0.5]


# ---- MSE, SSD, RMSE ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1000])
def test_mse_fwd_bwd(L, rows):
    """loss = sum (p - t)^2 / denom, dpred = weight * 2 (p - t) / denom, denom != rows (the global batch under data parallelism), one
    workgroup of 256 threads striding over the rows.  Bars: each square carries 3u (difference, product), the sum is at most
    ceil(rows / 256) + 9 additions deep (thread loop, 6 shuffles, 3 for the four wave totals), 1 / denom and the final product 2u;
    dpred is five rounded operations."""
    g = torch.Generator().manual_seed(rows)
    p, t = torch.randn(rows, generator=g), torch.randn(rows, generator=g)
    denom, weight = float(2 * rows + 3), 0.7
    pd, td = dev(p), dev(t)
    sq = (p.double() - t.double()) ** 2
    depth = -(-rows // 256) + 9 + 3 + 2
    for with_grad in (True, False):
        loss, dp = Out(1), Out(rows)
        assert L.lib.sdumc_mse_fwd_bwd(pd.data_ptr(), td.data_ptr(), rows, denom, weight, loss.ptr(), dp.ptr() if with_grad else None, None) == 0
        within(loss.get(), (sq.sum() / denom).reshape(1), (sq.sum() / denom).reshape(1), depth, f"mse loss rows={rows}")
        if with_grad:
            ref = float(np.float32(weight)) * 2.0 * (p.double() - t.double()) / denom
            within(dp.get(), ref, ref.abs(), 5, f"mse dpred rows={rows}")
        else:
            assert untouched(dp)
    loss = Out(1)
    assert L.lib.sdumc_mse_fwd_bwd(pd.data_ptr(), td.data_ptr(), 0, denom, weight, loss.ptr(), None, None) == EINVAL
    assert L.lib.sdumc_mse_fwd_bwd(pd.data_ptr(), td.data_ptr(), rows, 0.0, weight, loss.ptr(), None, None) == EINVAL
    assert L.lib.sdumc_mse_fwd_bwd(pd.data_ptr(), None, rows, denom, weight, loss.ptr(), None, None) == EINVAL
    assert untouched(loss)


@pytest.mark.parametrize("n", [1, 255, 8191, 8192, 8193, 256 * 8192 + 1])
def test_ssd(L, n):
    """sum (a - b)^2 in chunks of 8192 (one workgroup each), then one workgroup over the chunk sums: one chunk, both sides of the chunk
    edge, and 257 chunks, where stage 2 strides a second time.  The workspace is exactly the stated size, guarded.  Bar: 3u per square +
    the depth of the two sums: 32 + 9 within a chunk (thread loop, 6 shuffles, 3 for the four wave totals), ceil(chunks / 256) + 9 over the chunks."""
    g = torch.Generator().manual_seed(n % 100003)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ad, bd = dev(a), dev(b)
    chunks = -(-n // 8192)
    nbytes = L.lib.sdumc_ssd_workspace_bytes(n)
    assert nbytes == chunks * 4
    ws, out = Out(chunks), Out(1)
    assert L.lib.sdumc_ssd(ad.data_ptr(), bd.data_ptr(), n, out.ptr(), ws.ptr(), None) == 0
    ref = ((a.double() - b.double()) ** 2).sum().reshape(1)
    within(out.get(), ref, ref, 3 + 41 + -(-chunks // 256) + 9, f"ssd n={n}")
    part = ws.get()
    sq = torch.nn.functional.pad((a.double() - b.double()) ** 2, (0, chunks * 8192 - n)).reshape(chunks, 8192).sum(1)
    within(part, sq, sq, 3 + 41, f"ssd n={n} chunk sums")
    out2 = Out(1)
    assert L.lib.sdumc_ssd(ad.data_ptr(), bd.data_ptr(), 0, out2.ptr(), ws.ptr(), None) == EINVAL
    assert L.lib.sdumc_ssd(ad.data_ptr(), bd.data_ptr(), n, out2.ptr(), None, None) == EINVAL
    assert untouched(out2)


@pytest.mark.parametrize("n_local", [1, 257, 1000])
def test_rmse_bwd(L, n_local):
    """loss = sqrt(ssd / numel), da = +-weight (a - b) / (numel * loss) from a GIVEN global sum of squares and a global element count
    larger than the local one (a data-parallel shard).  Every combination of the two accumulate flags onto a known pattern; da, db
    and loss_out NULL one at a time.  Bars: the loss is 1 / numel, a product and a square root (4u); a gradient is eight rounded
    operations on a single product (+ 1 for the accumulation, on |old| + |g|)."""
    g = torch.Generator().manual_seed(n_local)
    a, b = torch.randn(n_local, generator=g), torch.randn(n_local, generator=g)
    da0, db0 = 3 * torch.randn(n_local, generator=g), 3 * torch.randn(n_local, generator=g)
    numel, weight = 3.0 * n_local + 7, 0.7
    ssd = np.float32(float(((a.double() - b.double()) ** 2).sum()) * 2.9)       # "the other ranks" hold the rest
    ad, bd, sd = dev(a), dev(b), dev(torch.tensor([float(ssd)]))
    rmse = np.sqrt(float(ssd) / numel)
    gref = float(np.float32(weight)) * (a.double() - b.double()) / (numel * rmse)

    def run(da_acc, db_acc, no=None):
        loss, da, db = Out(1), Out(n_local, fill=da0 if da_acc else NAN), Out(n_local, fill=db0 if db_acc else NAN)
        assert L.lib.sdumc_rmse_bwd(ad.data_ptr(), bd.data_ptr(), n_local, sd.data_ptr(), numel, weight, None if no == "loss" else loss.ptr(),
                                    None if no == "da" else da.ptr(), da_acc, None if no == "db" else db.ptr(), db_acc, None) == 0
        what = f"rmse_bwd n_local={n_local} da_acc={da_acc} db_acc={db_acc} null={no}"
        if no == "loss":
            assert untouched(loss), what
        else:
            within(loss.get(), torch.tensor([rmse]), torch.tensor([rmse]), 4, what + " loss")
        for out, acc, old, sign, name in ((da, da_acc, da0, 1.0, "da"), (db, db_acc, db0, -1.0, "db")):
            if no == name:
                assert torch.equal(out.get(), old) if acc else untouched(out), what + f": {name} = NULL is not written"
            elif acc:
                within(out.get(), old.double() + sign * gref, old.double().abs() + gref.abs(), 9, what + " " + name)
            else:
                within(out.get(), sign * gref, gref.abs(), 8, what + " " + name)

    for da_acc in (0, 1):
        for db_acc in (0, 1):
            run(da_acc, db_acc)
    for no in ("da", "db", "loss"):
        run(1, 0, no)
        run(0, 1, no)
    loss = Out(1)
    assert L.lib.sdumc_rmse_bwd(ad.data_ptr(), bd.data_ptr(), 0, sd.data_ptr(), numel, weight, loss.ptr(), None, 0, None, 0, None) == EINVAL
    assert L.lib.sdumc_rmse_bwd(ad.data_ptr(), bd.data_ptr(), n_local, sd.data_ptr(), 0.0, weight, loss.ptr(), None, 0, None, 0, None) == EINVAL
    assert L.lib.sdumc_rmse_bwd(ad.data_ptr(), bd.data_ptr(), n_local, None, numel, weight, loss.ptr(), None, 0, None, 0, None) == EINVAL
    assert untouched(loss)


def test_rmse_bwd_of_equal_inputs_is_nan_like_torch(L):
    """a == b: ssd = 0, loss = 0 and every gradient is 0 / 0 = NaN.  loss.hip says that this is what torch's sqrt backward gives;
    torch is asked here, on the CPU."""
    n = 300
    a = torch.randn(n, generator=torch.Generator().manual_seed(9))
    ta, tb = a.clone().requires_grad_(), a.clone().requires_grad_()
    torch.sqrt(torch.nn.functional.mse_loss(ta, tb, reduction="mean")).backward()
    assert bool(torch.isnan(ta.grad).all()) and bool(torch.isnan(tb.grad).all()), "torch: NaN gradients for equal inputs"
    ad, bd = dev(a), dev(a.clone())
    ssd, ws = Out(1), Out(1)
    assert L.lib.sdumc_ssd(ad.data_ptr(), bd.data_ptr(), n, ssd.ptr(), ws.ptr(), None) == 0
    assert float(ssd.get()) == 0.0
    loss, da, db = Out(1, fill=5.0), Out(n, fill=5.0), Out(n, fill=5.0)
    assert L.lib.sdumc_rmse_bwd(ad.data_ptr(), bd.data_ptr(), n, ssd.ptr(), float(n), 1.0, loss.ptr(), da.ptr(), 0, db.ptr(), 0, None) == 0
    assert float(loss.get()) == 0.0
    assert bool(torch.isnan(da.get()).all()) and bool(torch.isnan(db.get()).all())
