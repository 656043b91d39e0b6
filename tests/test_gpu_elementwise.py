"""GPU kernel-level tests of elementwise.hip: every small kernel of the per-layer utterance path (and the batch-assembly / state
helpers beside them) through the C ABI against float64 torch of the same operation.

Conventions of this file:
  * every output buffer is allocated with a guard band behind it (`Out`), pre-filled with NaN where the contract is "overwrite" and
    with a known pattern where it is "accumulate" or "leaves the rest alone"; the guard must come back untouched;
  * the bar of a sum of n rounded fp32 operations is the standard n * 2^-24 * sum|terms| PER ELEMENT (`within`), with the sum of
    the absolute terms taken from the float64 reference: derived, not tuned.  Pure copies and selects are bit-exact."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                # unit roundoff of fp32
EINVAL = -1
GUARD = 64                    # elements behind every output
D, H, NQ = 256, 128, 7


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import _lib
    return _lib


def dev(t):
    return t.cuda().contiguous()


class Out:
    """n elements for a kernel to write, GUARD elements behind them that it must not."""

    def __init__(self, n, fill=float("nan"), dtype=torch.float32):
        self.n = n
        self.guard = -12345 if dtype in (torch.int32, torch.int16) else -777.25
        self.buf = torch.full((n + GUARD,), self.guard, dtype=dtype, device="cuda")
        if isinstance(fill, torch.Tensor):
            self.buf[:n] = fill.reshape(-1).to(dtype).cuda()
        else:
            self.buf[:n] = fill
        self.t = self.buf[:n]

    def ptr(self):
        return self.buf.data_ptr()

    def get(self, *shape):
        """The written part on the host; fails if the guard band was touched."""
        torch.cuda.synchronize()
        g = self.buf[self.n:].cpu()
        assert torch.equal(g, torch.full_like(g, self.guard)), "guard band behind the output was written"
        return self.t.cpu().reshape(*shape) if shape else self.t.cpu()


def within(got, ref, mag, nops, what, extra_rel=0.0):
    """|got - ref| <= nops * 2^-24 * mag (+ extra_rel * |ref|) element by element; a NaN in `got` fails."""
    got, ref, mag = got.double(), ref.double().reshape(got.shape), mag.double().reshape(got.shape)
    bar = nops * U * mag + extra_rel * ref.abs()
    bad = ~((got - ref).abs() <= bar)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bar; worst excess "
                                 f"{float(((got - ref).abs() - bar)[bad].nan_to_num(nan=float('inf')).max()):.3e}")


def randn(g, *shape):
    return torch.randn(*shape, generator=g)


# ---- modality fusion, second-level fusion, pooling (model :301-332, :346-358) ----------------------------------------------------
@pytest.mark.parametrize("V", [1, 5, 514])
def test_fusion_fwd_bwd(L, V):
    """qin [7][V,256] = (f, f_at, f_tv, f_av, u_a, u_t, u_v) with f = sum_m alpha_m u_m; backward: du overwritten, dalpha ACCUMULATED.
    V = 1, 5, 514 leave 3, 3 and 2 waves of the last workgroup without a sample."""
    g = torch.Generator().manual_seed(100 + V)
    u, alpha, dqin, dalpha0 = randn(g, V, 3, D), randn(g, V, 3), randn(g, 7, V, D), 3 * randn(g, V, 3)
    ud, ad, dqd = dev(u), dev(alpha), dev(dqin)
    qin = Out(7 * V * D)
    assert L.lib.sdumc_fusion_fwd(ud.data_ptr(), ad.data_ptr(), qin.ptr(), V, None) == 0
    got = qin.get(7, V, D)
    w = u.double() * alpha.double()[:, :, None]                       # [V,3,256]: alpha_m u_m
    a, t, v = w[:, 0], w[:, 1], w[:, 2]
    for i, (ref, mag, n) in enumerate([(a + t + v, a.abs() + t.abs() + v.abs(), 5), (a + t, a.abs() + t.abs(), 3),
                                       (t + v, t.abs() + v.abs(), 3), (a + v, a.abs() + v.abs(), 3)]):
        within(got[i], ref, mag, n, f"fusion_fwd qin[{i}]")
    for m in range(3):
        assert torch.equal(got[4 + m], u[:, m]), f"fusion_fwd qin[{4 + m}] is a copy of u_{m}"

    du, dalpha = Out(V * 3 * D), Out(V * 3, fill=dalpha0)
    assert L.lib.sdumc_fusion_bwd(ud.data_ptr(), ad.data_ptr(), dqd.data_ptr(), du.ptr(), dalpha.ptr(), V, None) == 0
    dq = dqin.double()
    gsum = torch.stack([dq[0] + dq[1] + dq[3], dq[0] + dq[1] + dq[2], dq[0] + dq[2] + dq[3]], 1)            # [V,3,256]
    gabs = torch.stack([dq[0].abs() + dq[1].abs() + dq[3].abs(), dq[0].abs() + dq[1].abs() + dq[2].abs(),
                        dq[0].abs() + dq[2].abs() + dq[3].abs()], 1)
    direct = dq[4:7].permute(1, 0, 2)                                                                          # [V,3,256]
    al = alpha.double()[:, :, None]
    within(du.get(V, 3, D), gsum * al + direct, gabs * al.abs() + direct.abs(), 4, "fusion_bwd du")
    within(dalpha.get(V, 3), dalpha0.double() + (gsum * u.double()).sum(2), dalpha0.abs().double() + (gabs * u.double().abs()).sum(2),
           D + 3, "fusion_bwd dalpha (added onto the second-level fusion's contribution)")


def _relu_like(g, *shape):
    """Post-ReLU/dropout-like values that ALSO hold exact zeros (+0 and -0) and negatives."""
    c = randn(g, *shape)
    sel = torch.rand(*shape, generator=g)
    c[sel < 0.2] = 0.0
    c[(sel >= 0.2) & (sel < 0.3)] = -0.0
    return c


@pytest.mark.parametrize("V", [1, 5, 514])
def test_hweight_fwd_bwd(L, V):
    """h = sum_m alpha_m c_m; backward dc_m = alpha_m dh (+ dct on m = 1) (* [c_m > 0] relu_scale), dalpha_m = <dh, c_m> OVERWRITTEN."""
    g = torch.Generator().manual_seed(200 + V)
    c, alpha, dh, dct = _relu_like(g, 3, V, NQ, H), randn(g, V, 3), randn(g, V, NQ, H), randn(g, V, NQ, H)
    assert (c == 0).any() and (c < 0).any()
    cd, ad, dhd, dctd = dev(c), dev(alpha), dev(dh), dev(dct)
    h = Out(V * NQ * H)
    assert L.lib.sdumc_hweight_fwd(cd.data_ptr(), ad.data_ptr(), h.ptr(), V, None) == 0
    w = c.double() * alpha.double().t()[:, :, None, None]             # [3,V,7,128]
    within(h.get(V, NQ, H), w.sum(0), w.abs().sum(0), 5, "hweight_fwd")
    for use_dct in (False, True):
        for relu_scale in (0.0, float(np.float32(1.0) / np.float32(0.7))):
            what = f"hweight_bwd dct={'given' if use_dct else 'NULL'} relu_scale={relu_scale:.4f}"
            dc, dalpha = Out(3 * V * NQ * H), Out(V * 3)
            assert L.lib.sdumc_hweight_bwd(cd.data_ptr(), ad.data_ptr(), dhd.data_ptr(), dctd.data_ptr() if use_dct else None,
                                           dc.ptr(), dalpha.ptr(), V, relu_scale, None) == 0, what
            ref = dh.double()[None] * alpha.double().t()[:, :, None, None]
            mag = ref.abs()
            if use_dct:
                ref[1] += dct.double()
                mag[1] += dct.double().abs()
            if relu_scale > 0:
                keep = (c > 0).double() * relu_scale
                ref, mag = ref * keep, mag * keep                     # mag = 0 where c <= 0: exactly zero there
            within(dc.get(3, V, NQ, H), ref, mag, 3, what + " dc")
            prod = dh.double()[None] * c.double()
            within(dalpha.get(V, 3), prod.sum((2, 3)).t(), prod.abs().sum((2, 3)).t(), NQ * H + 1, what + " dalpha")


@pytest.mark.parametrize("V", [1, 5, 514])
def test_zpool_fwd_bwd(L, V):
    """z = sum_i beta_i h_i; backward dh_i = beta_i dz, dbeta_i = <dz, h_i>, both OVERWRITTEN."""
    g = torch.Generator().manual_seed(300 + V)
    h, beta, dz = randn(g, V, NQ, H), randn(g, V, NQ), randn(g, V, H)
    hd, bd, dzd = dev(h), dev(beta), dev(dz)
    z = Out(V * H)
    assert L.lib.sdumc_zpool_fwd(hd.data_ptr(), bd.data_ptr(), z.ptr(), V, None) == 0
    w = h.double() * beta.double()[:, :, None]
    within(z.get(V, H), w.sum(1), w.abs().sum(1), 2 * NQ, "zpool_fwd")
    dh, dbeta = Out(V * NQ * H), Out(V * NQ)
    assert L.lib.sdumc_zpool_bwd(hd.data_ptr(), bd.data_ptr(), dzd.data_ptr(), dh.ptr(), dbeta.ptr(), V, None) == 0
    ref = dz.double()[:, None, :] * beta.double()[:, :, None]
    within(dh.get(V, NQ, H), ref, ref.abs(), 1, "zpool_bwd dh")
    prod = dz.double()[:, None, :] * h.double()
    within(dbeta.get(V, NQ), prod.sum(2), prod.abs().sum(2), H + 1, "zpool_bwd dbeta")


# ---- ReLU / dropout backward, sums ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 131587])
def test_relu_drop_bwd_in_place(L, n):
    """dz = dy * [y > 0] * scale with dz aliasing dy; +0, -0 and negative y all give exactly 0."""
    g = torch.Generator().manual_seed(n)
    y, dy = randn(g, n), randn(g, n)
    y[0::5] = 0.0
    y[1::5] = -0.0
    y[2::5] = -y[2::5].abs() - 1e-30
    scale = float(np.float32(1.0) / np.float32(0.7))
    buf = Out(n, fill=dy)
    yd = dev(y)
    assert L.lib.sdumc_relu_drop_bwd(buf.ptr(), yd.data_ptr(), scale, buf.ptr(), n, None) == 0
    got = buf.get()
    ref = torch.where(y > 0, dy.double() * scale, torch.zeros(n, dtype=torch.float64))
    within(got, ref, ref.abs(), 1, "relu_drop_bwd")
    assert (got[y <= 0] == 0).all()
    if n > 3:
        assert (got != 0).any()


def test_relu_drop_bwd_nothing_to_do(L):
    buf, y = Out(8, fill=2.5), dev(torch.ones(8))
    assert L.lib.sdumc_relu_drop_bwd(buf.ptr(), y.data_ptr(), 2.0, buf.ptr(), 0, None) == 0
    assert torch.equal(buf.get(), torch.full((8,), 2.5))
    assert L.lib.sdumc_relu_drop_bwd(buf.ptr(), y.data_ptr(), 2.0, buf.ptr(), -1, None) == EINVAL
    assert L.lib.sdumc_relu_drop_bwd(None, y.data_ptr(), 2.0, buf.ptr(), 8, None) == EINVAL


@pytest.mark.parametrize("k", [1, 3, 8])
def test_add_n(L, k):
    n = 1000
    g = torch.Generator().manual_seed(k)
    xs = [randn(g, n) for _ in range(k)]
    xd = [dev(x) for x in xs]
    arr = (C.c_void_p * k)(*[x.data_ptr() for x in xd])
    y = Out(n)
    assert L.lib.sdumc_add_n(arr, k, y.ptr(), n, None) == 0
    st = torch.stack(xs).double()
    if k == 1:
        assert torch.equal(y.get(), xs[0])
    else:
        within(y.get(), st.sum(0), st.abs().sum(0), k - 1, f"add_n k={k}")


def test_add_n_rejects_bad_arguments(L):
    n = 16
    xd = [dev(torch.ones(n)) for _ in range(9)]
    y = Out(n, fill=7.0)
    arr9 = (C.c_void_p * 9)(*[x.data_ptr() for x in xd])
    assert L.lib.sdumc_add_n(arr9, 0, y.ptr(), n, None) == EINVAL
    assert L.lib.sdumc_add_n(arr9, 9, y.ptr(), n, None) == EINVAL
    assert L.lib.sdumc_add_n(None, 3, y.ptr(), n, None) == EINVAL
    assert L.lib.sdumc_add_n(arr9, 3, None, n, None) == EINVAL
    hole = (C.c_void_p * 3)(xd[0].data_ptr(), None, xd[2].data_ptr())
    assert L.lib.sdumc_add_n(hole, 3, y.ptr(), n, None) == EINVAL
    assert torch.equal(y.get(), torch.full((n,), 7.0))


@pytest.mark.parametrize("rows", [1, 511, 512, 513, 1537])
def test_colsum(L, rows):
    """out[j] (+)= sum_r a[r, j] in 512-row chunks: one row, both sides of the chunk edge, three chunks and a ragged fourth; columns
    on both sides of the 64-wide stage-1 tile; lda > cols with NaN in the padding columns; a workspace of exactly the stated size."""
    g = torch.Generator().manual_seed(rows)
    for cols in (1, 3, 64, 65, 256):
        lda = cols + 3
        a = torch.full((rows, lda), float("nan"))
        a[:, :cols] = randn(g, rows, cols)
        ad = dev(a)
        out0 = 5 * randn(g, cols)
        nbytes = L.lib.sdumc_colsum_workspace_bytes(rows, cols)
        assert nbytes == ((rows + 511) // 512) * cols * 4
        for accumulate in (0, 1):
            ws = Out(nbytes // 4)
            out = Out(cols, fill=out0 if accumulate else float("nan"))
            assert L.lib.sdumc_colsum(ad.data_ptr(), rows, cols, lda, out.ptr(), accumulate, ws.ptr(), None) == 0
            x = a[:, :cols].double()
            ref, mag = x.sum(0), x.abs().sum(0)
            if accumulate:
                ref, mag = ref + out0.double(), mag + out0.double().abs()
            within(out.get(), ref, mag, rows + 1, f"colsum rows={rows} cols={cols} accumulate={accumulate}")
            ws.get()
    assert L.lib.sdumc_colsum(ad.data_ptr(), rows, 256, 255, out.ptr(), 0, ws.ptr(), None) == EINVAL


# ---- dropout-mask sum (backward of the dropout applications that read one projected feature tensor) -----------------------------
def _dropsum_case(L, terms, bf16, with_bits):
    from oracle import philox
    from sdumc_amd._lib import make_dropout
    samples, T, seed, call0, sample0 = 3, 5, (1 << 33) + 77, 6, 2
    g = torch.Generator().manual_seed(10 * terms + bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    p = L.DropSum()
    p.terms, p.samples, p.T, p.bf16 = terms, samples, T, int(bf16)
    keep, ref, mag = [], torch.zeros(samples, T, D, dtype=torch.float64), torch.zeros(samples, T, D, dtype=torch.float64)
    for k in range(terms):
        gk = randn(g, samples, T, D).to(dt)
        gd = dev(gk)
        keep.append(gd)
        p.g[k] = gd.data_ptr()
        stream, site, pk = (k * 3 + 1) % 2 if terms > 1 else 1, 4 + 3 * k, (0.5, 0.3)[k % 2]
        enabled = not (terms > 1 and k == terms // 2)                 # one disabled descriptor among the terms
        d = make_dropout(enabled, site, pk, T, D, samples, sample0=sample0, call0=call0, seed=seed)
        if with_bits and enabled:
            bits = torch.empty(2 * samples * T * (D // 4), dtype=torch.uint8, device="cuda")
            assert L.lib.sdumc_dropout_bits(C.byref(d), 2, bits.data_ptr(), None) == 0
            keep.append(bits)
            d.bits = bits.data_ptr()
        p.drop[k] = d
        p.stream_idx[k] = stream
        mask = philox.dropout_mask(samples, T, D, pk, seed, call0 + stream, site, sample0) if enabled else np.ones((samples, T, D), np.float32)
        term = gk.double() * torch.from_numpy(mask).double()
        ref += term
        mag += term.abs()
    if terms > 1:
        assert {p.stream_idx[k] for k in range(terms)} == {0, 1}
    dx = Out(samples * T * D, dtype=dt)
    p.dx = dx.ptr()
    assert L.lib.sdumc_dropsum_bwd(C.byref(p), None) == 0
    return dx.get(samples, T, D), ref, mag


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("terms", [1, 4, 8])
def test_dropsum_bwd(L, terms, bf16):
    """dx = sum_k g_k * mask_k with the masks of oracle/philox.py (the convention test_dropout_mask_bit_exact pins): streams 0 and 1
    mixed, a disabled (identity) term among them; the bf16 kernel rounds its fp32 sum once to bf16."""
    got, ref, mag = _dropsum_case(L, terms, bf16, False)
    within(got, ref, mag, terms, f"dropsum_bwd terms={terms} bf16={bf16}", extra_rel=2.0 ** -8 if bf16 else 0.0)
    if not bf16:          # keep-bits attached: the same masks from a table instead of Philox
        again, _, _ = _dropsum_case(L, terms, False, True)
        assert torch.equal(again, got), "dropsum_bwd with keep-bits differs from the Philox path"


def test_dropsum_bwd_rejects_bad_term_counts(L):
    x = dev(torch.ones(1, 1, D))
    p = L.DropSum()
    p.samples, p.T, p.dx = 1, 1, x.data_ptr()
    for k in range(8):
        p.g[k] = x.data_ptr()
    for terms in (0, 9):
        p.terms = terms
        assert L.lib.sdumc_dropsum_bwd(C.byref(p), None) == EINVAL
    p.terms, p.g[1] = 2, None
    assert L.lib.sdumc_dropsum_bwd(C.byref(p), None) == EINVAL


# ---- strided copies, fill ---------------------------------------------------------------------------------------------------------
def test_copy2d_axpy2d_strided(L):
    rows, cols, ld_src, ld_dst = 37, 19, 23, 29                      # 703 elements: three workgroups, the last one ragged
    g = torch.Generator().manual_seed(1)
    src, dst0 = randn(g, rows, ld_src), randn(g, rows, ld_dst)
    sd = dev(src)
    dst = Out(rows * ld_dst, fill=dst0)
    assert L.lib.sdumc_copy2d(sd.data_ptr(), ld_src, dst.ptr(), ld_dst, rows, cols, None) == 0
    got = dst.get(rows, ld_dst)
    assert torch.equal(got[:, :cols], src[:, :cols]) and torch.equal(got[:, cols:], dst0[:, cols:])
    dst = Out(rows * ld_dst, fill=dst0)
    assert L.lib.sdumc_axpy2d(sd.data_ptr(), ld_src, dst.ptr(), ld_dst, rows, cols, None) == 0
    got = dst.get(rows, ld_dst)
    ref = dst0[:, :cols].double() + src[:, :cols].double()
    within(got[:, :cols], ref, ref.abs(), 1, "axpy2d")
    assert not torch.equal(got[:, :cols], src[:, :cols]) and torch.equal(got[:, cols:], dst0[:, cols:])
    for fn in (L.lib.sdumc_copy2d, L.lib.sdumc_axpy2d):
        assert fn(sd.data_ptr(), cols - 1, dst.ptr(), ld_dst, rows, cols, None) == EINVAL
        assert fn(sd.data_ptr(), ld_src, dst.ptr(), cols - 1, rows, cols, None) == EINVAL
        assert fn(sd.data_ptr(), ld_src, dst.ptr(), ld_dst, 0, cols, None) == EINVAL


def test_copy2d_multi_unequal_segments(L):
    """Five strided copies in one launch whose grid is sized by the largest and capped at 256 workgroups: 514 x 896 elements is seven
    grid strides, the small segments leave most workgroups idle."""
    g = torch.Generator().manual_seed(2)
    shapes = [(514, 896, 900, 904), (1, 1, 1, 2), (37, 19, 23, 29), (256, 256, 256, 260), (3, 300, 301, 300)]   # rows, cols, ld_src, ld_dst
    segs = (L.CopySeg * 5)()
    srcs, dsts, keep = [], [], []
    for i, (rows, cols, ld_src, ld_dst) in enumerate(shapes):
        src, dst0 = randn(g, rows, ld_src), randn(g, rows, ld_dst)
        sd, dst = dev(src), Out(rows * ld_dst, fill=dst0)
        srcs.append(src)
        dsts.append((dst, dst0))
        keep.append(sd)
        segs[i].src, segs[i].dst = sd.data_ptr(), dst.ptr()
        segs[i].ld_src, segs[i].ld_dst, segs[i].rows, segs[i].cols = ld_src, ld_dst, rows, cols
    assert shapes[0][0] * shapes[0][1] > 65536
    assert L.lib.sdumc_copy2d_multi(segs, 5, None) == 0
    for (rows, cols, ld_src, ld_dst), src, (dst, dst0) in zip(shapes, srcs, dsts):
        got = dst.get(rows, ld_dst)
        assert torch.equal(got[:, :cols], src[:, :cols]), (rows, cols)
        assert torch.equal(got[:, cols:], dst0[:, cols:]), (rows, cols)
    segs9 = (L.CopySeg * 9)(*([segs[2]] * 9))
    assert L.lib.sdumc_copy2d_multi(segs9, 0, None) == EINVAL
    assert L.lib.sdumc_copy2d_multi(segs9, 9, None) == EINVAL
    assert L.lib.sdumc_copy2d_multi(None, 1, None) == EINVAL


def test_fill(L):
    n = 1000
    buf = Out(n)
    assert L.lib.sdumc_fill(buf.ptr(), 3.25, n, None) == 0
    assert torch.equal(buf.get(), torch.full((n,), 3.25))
    assert L.lib.sdumc_fill(buf.ptr(), -1.0, 0, None) == 0
    assert torch.equal(buf.get(), torch.full((n,), 3.25))
    assert L.lib.sdumc_fill(None, 1.0, n, None) == EINVAL


# ---- batch assembly from a packed store -----------------------------------------------------------------------------------------------
def _store(g, lens, d):
    start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return randn(g, int(sum(lens)) + 1, d), start          # (+ 1 row: a store is never empty)


@pytest.mark.parametrize("d", [4, 36])
def test_gather_pad_and_gather_pad_idx(L, d):
    """The collater's right-zero-padding against a Python loop: lengths 0, 1, Tmax and above Tmax (truncated)."""
    g = torch.Generator().manual_seed(d)
    Tmax = 6
    lens = [3, 0, 6, 9, 1]
    packed, start = _store(g, lens, d)
    pd = dev(packed)
    B = len(lens)
    sd, ld = torch.from_numpy(start).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    out = Out(B * Tmax * d)
    assert L.lib.sdumc_gather_pad(pd.data_ptr(), sd.data_ptr(), ld.data_ptr(), B, Tmax, d, out.ptr(), None) == 0
    want = torch.zeros(B, Tmax, d)
    for b in range(B):
        for t in range(min(lens[b], Tmax)):
            want[b, t] = packed[start[b] + t]
    assert torch.equal(out.get(B, Tmax, d), want)
    # store-wide tables + a device index vector, with a repeated and a skipped entry
    idx = [3, 1, 1, 4, 0, 2, 3]
    Bi = len(idx)
    out, len_out = Out(Bi * Tmax * d), Out(Bi, fill=-1, dtype=torch.int32)
    idd = torch.tensor(idx, dtype=torch.int64).cuda()
    assert L.lib.sdumc_gather_pad_idx(pd.data_ptr(), sd.data_ptr(), ld.data_ptr(), idd.data_ptr(), Bi, Tmax, d, out.ptr(), len_out.ptr(),
                                      None) == 0
    want = torch.zeros(Bi, Tmax, d)
    for b, e in enumerate(idx):
        for t in range(min(lens[e], Tmax)):
            want[b, t] = packed[start[e] + t]
    assert torch.equal(out.get(Bi, Tmax, d), want)
    assert len_out.get().tolist() == [min(lens[e], Tmax) for e in idx]
    out2 = Out(Bi * Tmax * d)                                     # len_out is optional
    assert L.lib.sdumc_gather_pad_idx(pd.data_ptr(), sd.data_ptr(), ld.data_ptr(), idd.data_ptr(), Bi, Tmax, d, out2.ptr(), None, None) == 0
    assert torch.equal(out2.get(Bi, Tmax, d), want)
    # 16-byte accesses: a misaligned tensor or a width that is no multiple of 4 is refused
    assert L.lib.sdumc_gather_pad(pd.data_ptr() + 4, sd.data_ptr(), ld.data_ptr(), B, Tmax, d, out.ptr(), None) == EINVAL
    assert L.lib.sdumc_gather_pad(pd.data_ptr(), sd.data_ptr(), ld.data_ptr(), B, Tmax, d, out.ptr() + 8, None) == EINVAL
    assert L.lib.sdumc_gather_pad(pd.data_ptr(), sd.data_ptr(), ld.data_ptr(), B, Tmax, d + 2, out.ptr(), None) == EINVAL
    assert L.lib.sdumc_gather_pad_idx(pd.data_ptr() + 4, sd.data_ptr(), ld.data_ptr(), idd.data_ptr(), Bi, Tmax, d, out.ptr(), None,
                                      None) == EINVAL
    assert L.lib.sdumc_gather_pad_idx(pd.data_ptr(), sd.data_ptr(), ld.data_ptr(), idd.data_ptr(), Bi, Tmax, d + 2, out.ptr(), None,
                                      None) == EINVAL
    assert torch.equal(out.get(Bi, Tmax, d), want)


# ---- device Philox state -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call0,inc", [(9, 5), (0xFFFFFFFE, 5), (7, 0), (3, 0xFFFFFFFF)])
def test_rng_advance(L, call0, inc):
    """state = {seed_lo, seed_hi, call0}: call0 += inc modulo 2^32, the seed words stay."""
    words = np.array([0x89ABCDEF, 0x01234567, call0], dtype=np.uint32)
    st = Out(3, fill=torch.from_numpy(words.view(np.int32).copy()), dtype=torch.int32)
    assert L.lib.sdumc_rng_advance(st.ptr(), inc, None) == 0
    got = st.get().numpy().view(np.uint32)
    assert got.tolist() == [0x89ABCDEF, 0x01234567, (call0 + inc) & 0xFFFFFFFF]
    assert L.lib.sdumc_rng_advance(None, 1, None) == EINVAL
