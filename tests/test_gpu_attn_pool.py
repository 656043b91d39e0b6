"""Every launch route of csrc/attn_pool.hip against the fp64 restatement of the operation, slice by slice: one parametrised test per
route, named after the kernel the launcher picks.  Cases, references, slicing and bars: tests/attn_pool_cases.py; what makes the bars
legitimate: tests/test_attn_pool_parity_cpu.py.  Every output tensor and workspace of a call starts NaN-filled (ops._out), so a slice
no kernel wrote fails; frames beyond a sample's length and the dz / dq of a sample with one valid frame are exact zeros on the device.
Each run prints one `attn pool route` line (worst output and gradient slice beside its e_ref): profiles/attn_pool_parity_by_route.txt."""
import os

import pytest
import torch

from tests import attn_pool_cases as AC

pytestmark = pytest.mark.gpu
D = AC.D


def _nan_out(*shape, **kw):
    t = torch.empty(*shape, **kw)
    return t.fill_(255) if t.dtype == torch.uint8 else t.fill_(float("nan"))        # (0xff bytes read as fp32 / bf16 are NaN too)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import ops as o
    saved, o._out = o._out, _nan_out
    yield o
    o._out = saved


def dev(t):
    return t.cuda().contiguous()


class Problem:
    """a case on the device.  mask: "philox" (recomputed in the kernels), "bits" (keep-bits attached), None; bf16: "pre" (masked frames
    per virtual sample, no x_drop) or "bits" (bf16 frames with keep-bits attached)"""

    def __init__(self, ops, name, nq, mask="bits", bf16=None, shared_q=False, dim=D, k3=False):
        from sdumc_amd._lib import make_dropout
        self.case, self.nq, self.bf16, self.shared_q, self.dim = AC.by_name(name), nq, bf16, shared_q, dim
        case = self.case
        B, S, V = AC.shape(case)
        T = case["T"]
        self.kw = dict(dim=dim, x_mask=mask is not None, bf16=bf16 is not None, shared_q=shared_q, k3=k3)
        I = self.I = AC.inputs(case, nq, **self.kw)
        self.L = I["lengths"]
        self.lengths = dev(torch.tensor(AC.case_lengths(T)[:V], dtype=torch.int32)) if case["lens"] else None      # (raw: 0 clamps to 1)
        self.odrop = make_dropout(True, AC.SITE_O, AC.P_DROP, nq, dim, B, call0=AC.CALL, seed=AC.SEED)
        self.xdrop = make_dropout(True, AC.SITE_X, AC.P_DROP, T, dim, B, call0=AC.CALL, seed=AC.SEED) if mask else None
        self.bits = ops.dropout_bits(self.xdrop, S) if mask == "bits" else None
        self.x_samples = B
        if bf16 == "pre":
            self.x = dev((I["x"][torch.arange(V) % B] * I["xmask"]).bfloat16())      # (mask 0 / 2: the product is a bf16 value)
            self.x_samples, self.xdrop = V, None
        else:
            self.x = dev(I["x"].bfloat16() if bf16 else I["x"])
        self.keys = dev(I["keys"].bfloat16() if bf16 else I["keys"])
        self.q, self.dout = dev(I["q"]), dev(I["dout"])
        self.hi, self.lo = AC.reference(case, nq, **self.kw), AC.reference(case, nq, torch.float32, **self.kw)

    def fwd_kw(self, **more):
        return dict(dict(x=self.x, keys=self.keys, q=self.q, nq=self.nq, x_samples=self.x_samples, q_shared=self.shared_q, x_drop=self.xdrop,
                         out_drop=self.odrop, lengths=self.lengths, bf16=self.bf16 is not None), **more)

    def fwd(self, ops, tickets=False, **more):
        more.setdefault("dim", 0 if self.dim == D else self.dim)
        return ops.attnpool_fwd(**self.fwd_kw(tickets=tickets, **more))

    def judge(self, route, outs, grads, shared_q=None):
        """outs / grads: name -> device tensor.  Judged against fp64, then the exact zeros."""
        torch.cuda.synchronize()
        outs, grads = {k: v.float().cpu() for k, v in outs.items()}, {k: v.float().cpu() for k, v in grads.items()}
        sq = self.shared_q if shared_q is None else shared_q
        what = "%s, %s nq %d" % (route, self.case["name"], self.nq)
        res = AC.judge(outs, grads, self.hi, self.lo, self.L, what, offset=self.case["offset"], shared_q=sq, bf16=self.bf16 is not None)
        for k, t in list(outs.items()) + list(grads.items()):
            if k in ("attn", "dz", "dxd"):
                assert AC.padded_frames_are_zero(t, self.L), "%s: %s is not exactly 0 beyond a sample's length" % (what, k)
        for v, n in enumerate(self.L):          # one valid frame: an exactly zero score gradient
            if n == 1:
                if "dz" in grads:
                    assert int(torch.count_nonzero(grads["dz"][v])) == 0, "%s: dz[v%d]" % (what, v)
                if "dq" in grads and grads["dq"].shape[0] == len(self.L):
                    assert int(torch.count_nonzero(grads["dq"][v])) == 0, "%s: dq[v%d]" % (what, v)
        if not self.case["offset"]:
            assert not any(r.between for r in res), what
        parts = []
        for r in res:
            if len(r):
                k = max(r, key=r.get)
                parts.append("%s %.3g (e_ref %.2g)" % (k, r[k], r.e_ref[k]))
        print("attn pool route %s | %s nq %d | worst %s" % (route, self.case["name"], self.nq, " | ".join(parts)))
        return res

    def both(self, ops, route, tickets=False, **more):
        """forward + backward through the single-site entry points, everything against fp64"""
        out, attn, pooled, desc = self.fwd(ops, tickets=tickets, **more)
        dz, dxd, dq = ops.attnpool_bwd(desc, self.dout, ())
        self.judge(route, dict(out=out, attn=attn, pooled=pooled), dict(dz=dz, dxd=dxd, dq=dq))
        if tickets:
            assert int(desc._keep_tickets.abs().sum()) == 0       # the counters re-armed themselves
        return (out, attn, pooled, desc), (dz, dxd, dq)


class v2_off:
    """the round-3 kernels for what the v2 kernels would take; restored on the way out"""

    def __enter__(self):
        from sdumc_amd import _lib
        _lib.lib.sdumc_attnpool_set_v2_(0)

    def __exit__(self, *exc):
        from sdumc_amd import _lib
        _lib.lib.sdumc_attnpool_set_v2_(1)


# ---- the engine's two routes, and v1 with recomputed masks: the whole T sweep and every V form ------------------------------------
@pytest.mark.parametrize("name", AC.SWEEP)
@pytest.mark.parametrize("nq", [7, 1])
def test_v2_fp32_keep_bits(ops, name, nq):
    """attn_fwd_partial_v2_kernel<false, nq> + combine, attnpool_bwd_v2_kernel<false, nq> + dq_reduce: what the engine launches"""
    Problem(ops, name, nq, mask="bits").both(ops, "v2 fp32 <false,%d> keep-bits" % nq)


@pytest.mark.parametrize("name", AC.SWEEP)
@pytest.mark.parametrize("nq", [7, 1])
@pytest.mark.parametrize("tickets", [False, True], ids=["two launches", "tickets"])
def test_v1_fp32_philox(ops, name, nq, tickets):
    """attn_fwd_partial_kernel<true, 1>, attnpool_bwd_kernel<1>: masks recomputed from Philox in the kernels"""
    Problem(ops, name, nq, mask="philox").both(ops, "v1 fp32 philox, %s" % ("tickets" if tickets else "two launches"), tickets=tickets)


# ---- every other route: T = 65, T = 130 with lengths, peaked, offset -----------------------------------------------------------------
@pytest.mark.parametrize("name", AC.BASIC)
@pytest.mark.parametrize("nq", [7, 1])
def test_v2_fp32_no_mask(ops, name, nq):
    Problem(ops, name, nq, mask=None).both(ops, "v2 fp32 <false,%d> no mask" % nq)


@pytest.mark.parametrize("name", AC.BASIC)
@pytest.mark.parametrize("nq", [7, 1])
def test_v1_fp32_keep_bits_tickets(ops, name, nq):
    """keep-bits attached and tickets: the v2 kernels refuse tickets, attn_fwd_partial_kernel<false, 1> combines in the last chunk"""
    Problem(ops, name, nq, mask="bits").both(ops, "v1 fp32 keep-bits, tickets", tickets=True)


@pytest.mark.parametrize("name", AC.BASIC)
@pytest.mark.parametrize("nq", [7, 1])
@pytest.mark.parametrize("mask", ["bits", None], ids=["keep-bits", "no mask"])
def test_v1_fp32_two_launches(ops, name, nq, mask):
    with v2_off():
        Problem(ops, name, nq, mask=mask).both(ops, "v1 fp32 %s, two launches" % (mask and "keep-bits" or "no mask"))


@pytest.mark.parametrize("name", AC.BASIC)
@pytest.mark.parametrize("nq", [8, 2])
def test_v1_fp32_nq_8_and_2(ops, name, nq):
    """nq = 8 = MAXQ: the edge of r16 < MAXQ and of the [MAXQ][LDQ] tiles; the v2 kernels take 1 and 7 only"""
    Problem(ops, name, nq, mask="bits").both(ops, "v1 fp32 nq %d keep-bits" % nq)


@pytest.mark.parametrize("name", AC.BASIC)
@pytest.mark.parametrize("dim,mask", [(512, "philox"), (1024, "philox"), (1024, None)], ids=["512 philox", "1024 philox", "1024 no mask"])
def test_v1_fp32_wide_rows(ops, name, dim, mask):
    """attn_fwd_partial_kernel<.., C>, attnpool_bwd_kernel<C> at C = 2 and 4: dim in the descriptor, workspaces by the _dim queries"""
    Problem(ops, name, 7, mask=mask, dim=dim).both(ops, "v1 fp32 dim %d %s" % (dim, mask or "no mask"))


@pytest.mark.parametrize("name", AC.BASIC)
@pytest.mark.parametrize("nq", [7, 1])
@pytest.mark.parametrize("mask", ["philox", None], ids=["pre-masked", "no mask"])
def test_v2_bf16_pre_masked(ops, name, nq, mask):
    """attn_fwd_partial_v2_kernel<true, nq>, attnpool_bwd_v2_kernel<true, nq>: bf16 frames and keys, bf16 dz / dxd stores"""
    Problem(ops, name, nq, mask=mask, bf16="pre").both(ops, "v2 bf16 <true,%d> %s" % (nq, "pre-masked" if mask else "no mask"))


@pytest.mark.parametrize("name", AC.BASIC)
@pytest.mark.parametrize("nq", [7, 1])
def test_v1_bf16_pre_masked(ops, name, nq):
    with v2_off():
        Problem(ops, name, nq, mask="philox", bf16="pre").both(ops, "v1 bf16 pre-masked")


@pytest.mark.parametrize("name", AC.BASIC)
@pytest.mark.parametrize("nq", [7, 1])
def test_v1_bf16_keep_bits_attached(ops, name, nq):
    """bf16 frames with the mask fused from keep-bits: the v2 kernels refuse it, attn_fwd_partial_kernel<false, 1, true> takes it"""
    Problem(ops, name, nq, mask="bits", bf16="bits").both(ops, "v1 bf16 keep-bits attached")


# ---- several sites in one launch pair ------------------------------------------------------------------------------------------------
MULTI = {"v2 multi, nq 7": ((7, 7, 7), False), "v2 multi, nq 1": ((1, 1, 1), False), "v1 multi, nq 7 / 1 / 7": ((7, 1, 7), False),
         "v1 multi, tickets": ((7, 7, 7), True)}


@pytest.mark.parametrize("route", list(MULTI))
def test_multi_sites(ops, route):
    """sdumc_attnpool_fwd_multi / _bwd_multi at T 130 (lengths) / 64 / 37 (lengths): every site against fp64, not only against single
    calls; equal nq takes the v2 multi kernels, mixed nq and tickets the round-3 ones"""
    nqs, tickets = MULTI[route]
    probs = [Problem(ops, name, nq, mask="bits") for name, nq in zip(("T130L", "T64", "T37L"), nqs)]
    fw = ops.attnpool_fwd_multi([p.fwd_kw(tickets=tickets) for p in probs])
    bw = ops.attnpool_bwd_multi([f[3] for f in fw], [p.dout for p in probs])
    for p, (out, attn, pooled, desc), (dz, dxd, dq) in zip(probs, fw, bw):
        p.judge(route, dict(out=out, attn=attn, pooled=pooled), dict(dz=dz, dxd=dxd, dq=dq))
        if tickets:
            assert int(desc._keep_tickets.abs().sum()) == 0


# ---- the shared query's gradient in one launch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AC.BASIC)
@pytest.mark.parametrize("nq", [1, 7])
def test_dq_sum(ops, name, nq):
    """dq_sum_kernel: a shared query (q_stride 0) at nq 1 and 7 -- the sum over the samples equals the fp64 gradient of the shared query"""
    p = Problem(ops, name, nq, mask="bits", shared_q=True)
    out, attn, pooled, desc = p.fwd(ops)
    dz, dxd, dq = ops.attnpool_bwd(desc, p.dout, (), shared_q_sum=True)
    assert tuple(dq.shape) == (1, nq, D)
    p.judge("dq_sum nq %d" % nq, dict(out=out, attn=attn, pooled=pooled), dict(dz=dz, dxd=dxd, dq=dq))
    again = ops.attnpool_bwd(desc, p.dout, (), shared_q_sum=True)[2]
    assert torch.equal(dq, again)


# ---- the hand-over to the rows GEMM ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AC.BASIC)
@pytest.mark.parametrize("nq", [7, 1])
def test_dout_masked_without_dxd(ops, name, nq):
    """dout_masked with dxd = NULL, what the step uses: dz / dq bit-identical to the call that writes dxd, dout_masked = dout * mask
    exactly, and the consumer (sdumc_rows_problem.pool_w / pool_g, zero A) reproduces dxd under the gradient bar"""
    p = Problem(ops, name, nq, mask="bits")
    (out, attn, pooled, desc), (dz, dxd, dq) = p.both(ops, "v2 fp32 <false,%d> keep-bits" % nq)
    V, T = desc.V, desc.T
    dm = ops._out(V, nq, D, device="cuda")
    dz2, none, dq2 = ops.attnpool_bwd(desc, p.dout, (), dout_masked=dm, want_dxd=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(dz2, dz) and torch.equal(dq2, dq)
    assert torch.equal(dm.cpu(), p.I["dout"] * p.I["omask"])        # (mask 0 or 2: exact in fp32)
    C = ops.gemm_rows256([{"A": torch.zeros(V * T, D, device="cuda"), "B": torch.zeros(D, D, device="cuda"),
                           "pool_w": attn.view(V * T, nq), "pool_g": dm, "pool_T": T, "C": ops._out(V * T, D, device="cuda")}])[0]
    p.judge("dout_masked, dxd = NULL -> rows GEMM nq %d" % nq, {}, dict(dxd=C.view(V, T, D)))


# ---- partial_only -----------------------------------------------------------------------------------------------------------------------
def _finish_softmax(ws, attn_un, V, T, nq, dim):
    """the header's layout: unnormalised pooled rows [V][nchunk][nq][dim], then {chunk max, chunk sum} [V][nchunk][2][8]; finished in fp64"""
    nch = (T + AC.CH - 1) // AC.CH
    ws = ws.double().cpu()
    part = ws[:V * nch * nq * dim].view(V, nch, nq, dim)
    stats = ws[V * nch * nq * dim:V * nch * nq * dim + V * nch * 16].view(V, nch, 2, 8)[..., :nq]
    m, l = stats[:, :, 0], stats[:, :, 1]                             # [V, nch, nq]
    fac = torch.exp(m - m.amax(1, keepdim=True))
    fac = fac / (fac * l).sum(1, keepdim=True)
    pooled = (part * fac[..., None]).sum(1)
    attn = attn_un.double().cpu() * fac.repeat_interleave(AC.CH, dim=1)[:, :T]
    return attn, pooled


@pytest.mark.parametrize("name", AC.BASIC)
@pytest.mark.parametrize("route,nq", [("v2", 7), ("v2", 1), ("v1", 7), ("v1", 8)])
def test_partial_only(ops, name, route, nq):
    """forward stops after the per-chunk pass: the workspace's partials, finished on the host in fp64, give the reference pooled and
    attn; the backward multi form leaves per-chunk dq slabs whose fp64 sum is dq"""
    from contextlib import nullcontext
    p = Problem(ops, name, nq, mask="bits")
    with (v2_off() if route == "v1" else nullcontext()):
        out, attn_un, pooled, desc = p.fwd(ops, partial_only=True)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(pooled).all())         # NOT written
        attn, pooled = _finish_softmax(desc._keep_ws, attn_un, desc.V, desc.T, nq, D)
        fw = ops.attnpool_fwd_multi([p.fwd_kw(tickets=False)])[0]                         # a complete forward for the backward's inputs
        fw[3].partial_only = 1
        dz, dxd, slabs = ops.attnpool_bwd_multi([fw[3]], [p.dout])[0]
        torch.cuda.synchronize()
    what = "partial_only %s nq %d" % (route, nq)
    p.judge(what, dict(attn=attn, pooled=pooled), dict(dz=dz, dxd=dxd, dq=slabs.double().sum(1)))


# ---- K3 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AC.BASIC)
@pytest.mark.parametrize("nq", [7, 1])
@pytest.mark.parametrize("form", ["split", "split off", "P3 planes", "no mask", "no keys"])
def test_k3_umca_fwd(ops, name, nq, form):
    """sdumc_umca_fwd: key projection + scores + softmax partials + pooling in one kernel -- the in-kernel split, the fp32 MFMAs, the
    operands split once per tensor; keep-bits or no mask; its keys against fp64 too, and driving the ordinary backward"""
    from sdumc_amd import _lib
    p = Problem(ops, name, nq, mask=None if form == "no mask" else "bits", k3=True)
    I = p.I
    try:
        if form == "split off":
            _lib.lib.sdumc_set_split_(0)
        out, attn, pooled, keys, desc = ops.umca_fwd(p.x, dev(I["W"]), dev(I["b"]), p.q, nq, x_samples=p.x_samples, x_drop=p.xdrop,
                                                     out_drop=p.odrop, lengths=p.lengths, want_keys=form != "no keys", V=len(p.L),
                                                     planes=form == "P3 planes")
    finally:
        _lib.lib.sdumc_set_split_(int(os.environ.get("SDUMC_SPLIT", "15")))
    outs, grads = dict(out=out, attn=attn, pooled=pooled), {}
    if form == "no keys":
        assert keys is None
    else:
        outs["keys"] = keys
        dz, dxd, dq = ops.attnpool_bwd(desc, p.dout, ())
        grads = dict(dz=dz, dxd=dxd, dq=dq)
    p.judge("K3 %s" % form, outs, grads)


# ---- what the launcher documents as refused: host checks, nothing is launched ---------------------------------------------------------
def test_refusals(ops):
    from sdumc_amd._lib import SdumcError
    p = Problem(ops, "T65", 7, mask="philox", bf16="bits")
    with pytest.raises(SdumcError):          # bf16 frames with recomputed Philox masks
        p.fwd(ops)
    p = Problem(ops, "T65", 8, mask="bits")
    desc = p.fwd(ops)[3]
    with pytest.raises(SdumcError):          # dxd = NULL on a round-3 route (nq 8)
        ops.attnpool_bwd(desc, p.dout, (), want_dxd=False)
    with pytest.raises(SdumcError):          # ... and dout_masked there
        ops.attnpool_bwd(desc, p.dout, (), dout_masked=torch.empty(len(p.L), 8, D, device="cuda"))
    p = Problem(ops, "T65", 7, mask="bits")
    desc = p.fwd(ops)[3]
    with pytest.raises(SdumcError):          # dq_sum with a per-sample query
        ops.attnpool_bwd(desc, p.dout, (), shared_q_sum=True)
    with pytest.raises(SdumcError):          # partial_only with tickets
        p.fwd(ops, tickets=True, partial_only=True)
    with pytest.raises(SdumcError):          # 300 channels
        p.fwd(ops, dim=300)
    x9 = Problem(ops, "T65", 8, mask=None)
    with pytest.raises(SdumcError):          # nq 9 > MAXQ
        ops.attnpool_fwd(x9.x, x9.keys, torch.zeros(6, 9, D, device="cuda"), 9, x_samples=x9.x_samples)
    torch.cuda.synchronize()
