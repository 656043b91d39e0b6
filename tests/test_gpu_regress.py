"""GPU: the selectable regression criterion of the fused step (sdumc_step_cfg.regress: MSE / L1 / Huber / CCC), its stand-alone
entry sdumc_reg_fwd_bwd and the three drop-in loss modules behind it (L1Loss, HuberLoss, CCCLoss).

Chain of evidence: tests/reg_ref.py (float64 closed forms) is held to torch's autograd and to tests/golden/reg_losses.npz by
tests/test_regress_cpu.py at a quarter of the bars used here; the modules and the kernel entry are held to the fixture and to
reg_ref; every step route reproduces the kernel entry bit for bit; the fused step equals the module route (get_models + these
modules + autograd)."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from tests.grad_parity import close_norm
from tests.reg_ref import reg_ref, reg_terms

pytestmark = pytest.mark.gpu

CRITERIA = ("l1", "huber", "ccc")
CODE = {"mse": 0, "l1": 1, "huber": 2, "ccc": 3}
TOY_DIMS, TOY_T = (64, 32, 48, 32), (21, 5, 13, 4)
D, H, NQ = 256, 128, 7
U = 2.0 ** -24
EINVAL = -1
SENTINEL = 7.0


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import engine
    return engine


@pytest.fixture(scope="module")
def L(E):
    from sdumc_amd import _lib
    return _lib


def close(got, want, tol=1e-4, msg=""):
    """the `close` rule of tests/test_gpu_distill.py"""
    got = got.detach().cpu().double().numpy()
    want = want.detach().cpu().double().numpy() if isinstance(want, torch.Tensor) else np.asarray(want, dtype=np.float64)
    scale = max(1.0, np.abs(want).max())
    print(f"{msg}: max |got - want| = {np.abs(got - want.reshape(got.shape)).max():.3e} (scale {scale:.3e}, tol {tol:g})")
    np.testing.assert_allclose(got, want.reshape(got.shape), rtol=tol, atol=tol * scale, err_msg=msg)


def flat_from(E, P, dims):
    lay = E.ParamLayout.get(*dims[:3])
    flat = torch.zeros(lay.total)
    for k, v in lay.views(flat).items():
        v.copy_(P[k])
    return flat.cuda(), lay


def _module(name, delta=1.0):
    from sdumc_amd import loss
    return {"mse": loss.MSELoss, "l1": loss.L1Loss, "ccc": loss.CCCLoss}[name]() if name != "huber" else loss.HuberLoss(delta=delta)


def buf(n):
    return torch.full((n,), SENTINEL, device="cuda")


def untouched(*ts):
    return all(bool((t == SENTINEL).all()) for t in ts)


def reg_call(L, p, t, rows, denom, w, code, delta, loss, dp):
    return L.lib.sdumc_reg_fwd_bwd(L.ptr(p), L.ptr(t), rows, denom, w, code, delta, L.ptr(loss), L.ptr(dp), None)


def host_sign(d):
    one = torch.ones_like(d)
    return torch.where(d > 0, one, torch.where(d < 0, -one, torch.where(d == d, torch.zeros_like(d), d)))


def host_dpred(name, p, t, denom, weight, delta):
    """the table's gradient as a fp32 torch expression on the host: (w * g_i) * inv, no addition anywhere"""
    d = p - t
    inv = torch.tensor(1.0) / torch.tensor(denom, dtype=torch.float32)
    w = torch.tensor(weight, dtype=torch.float32)
    if name == "l1":
        g = host_sign(d)
    else:
        dl = torch.tensor(delta, dtype=torch.float32)
        g = torch.where(d.abs() <= dl, d, dl * host_sign(d))
    return (w * g) * inv


# ---- 1. the modules against the fixture ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crit", CRITERIA)
def test_modules_against_the_fixture(E, golden, crit):
    """L1Loss / HuberLoss / CCCLoss on pred [16,1] / target [16], on the edge rows (d = 0, |d| = delta, one ulp either side, delta 0.25
    and 1.0), on all-equal predictions and on one row, against float64 torch: values 1e-6, gradients 1e-5 with the `close` rule --
    the bars MSE / RMSE and the row criteria are held to.  Edge rows element by element.  0-dim result with grad; nothing to the
    target."""
    g = golden("reg_losses")
    cases = [("", 1.0, crit), ("edge_d025_", 0.25, crit), ("edge_d100_", 1.0, crit), ("const_", 1.0, crit), ("one_", 1.0, crit)]
    if crit == "huber":
        cases.append(("", 0.25, "huber025"))
    for pre, delta, key in cases:
        p = torch.from_numpy(g[pre + "pred"]).cuda().requires_grad_()
        t = torch.from_numpy(g[pre + "target"]).cuda().requires_grad_()
        l = _module(crit, delta)(p, t)
        assert l.dim() == 0 and l.requires_grad
        l.backward()
        assert t.grad is None and p.grad.shape == p.shape
        close(l.reshape(1), g[pre + key].reshape(1), 1e-6, f"{pre}{key} value")
        want = g[f"{pre}{key}_dpred"]
        if pre.startswith("edge"):
            for r in range(p.shape[0]):
                close(p.grad[r], want[r], 1e-5, f"{pre}{key} dpred row {r}")
        else:
            close(p.grad, want, 1e-5, f"{pre}{key} dpred")
    # MSELoss's shape rules: [B, W] and [B, G, W] inputs are sums over every element / B
    a, b = torch.randn(6, 3, 5, device="cuda"), torch.randn(6, 3, 5, device="cuda")
    for shape in ((6, 15), (6, 3, 5)):
        x = a.reshape(shape).clone().requires_grad_()
        l = _module(crit, 0.5)(x, b.reshape(shape))
        l.backward()
        v, dp = reg_ref(crit, a.cpu(), b.cpu(), denom=6, delta=0.5)
        close(l.reshape(1), v.reshape(1), 1e-6, f"{crit} {shape} value")
        close(x.grad.reshape(-1), dp, 1e-5, f"{crit} {shape} dpred")


# ---- 2. the kernel entry at the shapes where it can go wrong ------------------------------------------------------------------------
ROWS = [1, 2, 63, 64, 65, 255, 256, 257, 513, 1024]      # idle threads, wave edges, the 256-stride loop entered once, twice, four times


def _case(rows):
    g = torch.Generator().manual_seed(1000 + rows)
    t = torch.rand(rows, generator=g) * 6 - 3
    p = t + torch.randn(rows, generator=g)
    return p, t


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("crit", ["l1", "huber"])
def test_entry_l1_huber(L, rows, crit):
    """dpred bit-equal to the fp32 host expression of the table.  Value against float64 within (ceil(rows / 256) + 13) * 2^-24 of the
    sum of the non-negative terms: the thread's loop is ceil(rows / 256) additions deep, six wave steps, three adds of the four wave
    sums, four rounded operations per term (the counting rule of tests/loss_bars.py; nothing here was tuned on the device).  A NaN
    label: NaN value, NaN at that element alone.  loss_out only works."""
    p, t = _case(rows)
    denom, weight, delta = float(2 * rows + 3), 0.7, 0.75
    pd, td = p.cuda(), t.cuda()
    loss, dp = buf(1), buf(rows)
    assert reg_call(L, pd, td, rows, denom, weight, CODE[crit], delta, loss, dp) == 0
    want = host_dpred(crit, p, t, denom, weight, delta)
    got = dp.cpu()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {rows} gradient elements differ from the host expression"
    if crit == "huber" and rows >= 63:
        inside = (p - t).abs() <= delta
        assert bool(inside.any()) and bool((~inside).any())      # both branches ran
    terms = reg_terms(crit, p, t, delta)
    ref = float(terms.sum()) / denom
    bar = (-(-rows // 256) + 13) * U * ref
    err = abs(float(loss.cpu().double()) - ref)
    print(f"{crit} rows={rows}: value {ref:.9g}, |error| {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    only = buf(1)
    assert reg_call(L, pd, td, rows, denom, weight, CODE[crit], delta, only, None) == 0
    assert torch.equal(only.cpu(), loss.cpu())
    k = rows // 2
    tn = t.clone()
    tn[k] = float("nan")
    loss2, dp2 = buf(1), buf(rows)
    assert reg_call(L, pd, tn.cuda(), rows, denom, weight, CODE[crit], delta, loss2, dp2) == 0
    g2 = dp2.cpu()
    assert math.isnan(float(loss2.cpu())) and math.isnan(float(g2[k]))
    keep = torch.ones(rows, dtype=torch.bool)
    keep[k] = False
    assert torch.equal(g2[keep], want[keep])


@pytest.mark.parametrize("rows", ROWS)
def test_entry_ccc(L, rows):
    """against reg_ref at the module bars; rows = 1: value == 1.0 and gradient +0.0; pred and target one shared constant: NaN value
    and gradient (0/0, no special case); a NaN label: NaN everywhere; loss_out only works."""
    p, t = _case(rows)
    pd, td = p.cuda(), t.cuda()
    loss, dp = buf(1), buf(rows)
    assert reg_call(L, pd, td, rows, float(rows), 0.7, CODE["ccc"], 1.0, loss, dp) == 0
    v, g = reg_ref("ccc", p, t, weight=float(np.float32(0.7)))
    close(loss, v.reshape(1), 1e-6, f"ccc rows={rows} value")
    close(dp, g, 1e-5, f"ccc rows={rows} dpred")
    if rows == 1:
        assert float(loss.cpu()) == 1.0 and bool((dp == 0).all()) and not bool(torch.signbit(dp).any())
    only = buf(1)
    assert reg_call(L, pd, td, rows, float(rows), 0.7, CODE["ccc"], 1.0, only, None) == 0
    assert torch.equal(only.cpu(), loss.cpu())
    c = torch.full((rows,), 0.25, device="cuda")
    loss, dp = buf(1), buf(rows)
    assert reg_call(L, c, c.clone(), rows, float(rows), 0.7, CODE["ccc"], 1.0, loss, dp) == 0
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(dp).all())
    tn = t.clone()
    tn[rows // 2] = float("nan")
    loss, dp = buf(1), buf(rows)
    assert reg_call(L, pd, tn.cuda(), rows, float(rows), 0.7, CODE["ccc"], 1.0, loss, dp) == 0
    assert bool(torch.isnan(loss).all()) and math.isnan(float(dp[rows // 2]))


def test_entry_refuses_bad_arguments_and_its_mse_case_is_the_mse_entry(L):
    rows = 65
    p, t = (x.cuda() for x in _case(rows))
    loss, dp = buf(1), buf(rows)
    nan, inf = float("nan"), float("inf")
    bad = [dict(p=None), dict(t=None), dict(loss=None), dict(rows=0), dict(rows=-1), dict(denom=0.0), dict(denom=-1.0),
           dict(code=4), dict(code=-1), dict(code=1 << 20)] + [dict(code=2, delta=d) for d in (0.0, -1.0, inf, nan)]
    for kw in bad:
        a = dict(p=p, t=t, rows=rows, denom=float(rows), code=1, delta=1.0, loss=loss)
        a.update(kw)
        rc = reg_call(L, a["p"], a["t"], a["rows"], a["denom"], 0.7, a["code"], a["delta"], a["loss"], dp)
        assert rc == EINVAL, kw
    torch.cuda.synchronize()
    assert untouched(loss, dp)
    # a delta no criterion but Huber reads is not looked at
    for code in (0, 1, 3):
        assert reg_call(L, p, t, rows, float(rows), 0.7, code, nan, loss, dp) == 0
    assert reg_call(L, p, t, rows, float(rows), 0.7, 0, 1.0, loss, dp) == 0
    l0, d0 = buf(1), buf(rows)
    assert L.lib.sdumc_mse_fwd_bwd(L.ptr(p), L.ptr(t), rows, float(rows), 0.7, L.ptr(l0), L.ptr(d0), None) == 0
    assert torch.equal(l0, loss) and torch.equal(d0, dp)


# ---- 3. every route gives the kernel entry's bits ------------------------------------------------------------------------------------
def _bind_routes(L):
    fused = L.lib.sdumc_losses_fused_reg_
    fused.restype = C.c_int
    fused.argtypes = ([C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_float, C.POINTER(C.c_float)] + [C.c_void_p] * 9 +
                      [C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_float, C.c_void_p])
    crit = L.lib.sdumc_distill_crit_reg_
    crit.restype = C.c_int
    crit.argtypes = ([C.c_int32, C.c_float] + [C.c_void_p] * 5 + [C.POINTER(C.c_float)] + [C.c_void_p] * 7 +
                     [C.c_int32, C.c_int32, C.c_float, C.c_void_p])
    return fused, crit


class _Outs:
    def __init__(self, L, B, rd):
        n = 2 * B
        self.d_vals, self.d_th, self.d_ct, self.d_z, self.d_rnc = buf(n), buf(n * D), buf(n * NQ * H), buf(n * H), buf(n * rd)
        self.losses = buf(8)
        self.dws = buf(L.lib.sdumc_distill_workspace_bytes(B) // 4)
        self.rws = buf(L.lib.sdumc_rnc_workspace_bytes(n) // 4)


@pytest.mark.parametrize("B", [1, 4, 128, 300])
def test_routes_agree_bit_for_bit(L, B):
    """sdumc_reg_fwd_bwd per stream, the two-launch distillation route and the fused two-launch route (n = 2B <= 256; beyond it
    declines with 1 and writes nothing): torch.equal losses[1:3] and d_vals.  Entries 3..6 and their gradients are torch.equal to the
    regress = MSE call on the same inputs."""
    fused, crit = _bind_routes(L)
    rd, temp = 64, 2.0
    n = 2 * B
    g = torch.Generator().manual_seed(77 + B)
    labels = torch.rand(B, generator=g) * 6 - 3
    vals = labels.repeat(2) + torch.randn(n, generator=g)
    th, ct, z = torch.randn(n, D, generator=g), torch.randn(n, NQ, H, generator=g), torch.randn(n, H, generator=g)
    rf = 0.3 * torch.randn(n, rd, generator=g)
    vd, ld, thd, ctd, zd, rfd = (x.cuda() for x in (vals, labels, th, ct, z, rf))
    w6 = (C.c_float * 6)(0.5, 0.45, 0.1, 0.7, 0.13, 0.8)

    def run_crit(code, delta):
        o = _Outs(L, B, rd)
        assert crit(B, float(B), vd.data_ptr(), ld.data_ptr(), thd.data_ptr(), ctd.data_ptr(), zd.data_ptr(), w6, None,
                    o.d_vals.data_ptr(), o.d_th.data_ptr(), o.d_ct.data_ptr(), o.d_z.data_ptr(), o.losses.data_ptr(),
                    o.dws.data_ptr(), 0, code, delta, None) == 0
        return o

    def run_fused(code, delta):
        o = _Outs(L, B, rd)
        rc = fused(B, vd.data_ptr(), ld.data_ptr(), thd.data_ptr(), ctd.data_ptr(), zd.data_ptr(), rfd.data_ptr(), rd, temp, w6,
                   o.d_vals.data_ptr(), o.d_th.data_ptr(), o.d_ct.data_ptr(), o.d_z.data_ptr(), o.d_rnc.data_ptr(),
                   o.losses.data_ptr(), o.dws.data_ptr(), o.rws.data_ptr(), None, 0.9, 0.999, 0, code, delta, None)
        return rc, o

    base_c = run_crit(0, 0.0)
    rc0, base_f = run_fused(0, 0.0)
    assert rc0 == (0 if n <= 256 else 1)
    for name in CRITERIA:
        code, delta = CODE[name], 0.75
        per = []
        for s in (0, 1):
            loss, dp = buf(1), buf(B)
            assert reg_call(L, vd[s * B:], ld, B, float(B), float(w6[s]), code, delta, loss, dp) == 0
            per.append((loss, dp))
        want_l = torch.cat([per[0][0], per[1][0]])
        want_d = torch.cat([per[0][1], per[1][1]])
        oc = run_crit(code, delta)
        assert torch.equal(oc.losses[1:3], want_l) and torch.equal(oc.d_vals, want_d), name
        assert not torch.equal(oc.losses[1:3], base_c.losses[1:3])
        assert torch.equal(oc.losses[3:6], base_c.losses[3:6])
        for k in ("d_th", "d_ct", "d_z"):
            assert torch.equal(getattr(oc, k), getattr(base_c, k)), (name, k)
        rc, of = run_fused(code, delta)
        if n > 256:
            assert rc == 1 and untouched(of.losses, of.d_vals, of.d_rnc)
            continue
        assert rc == 0
        assert torch.equal(of.losses[1:3], want_l) and torch.equal(of.d_vals, want_d), name
        assert torch.equal(of.losses[3:7], base_f.losses[3:7])
        for k in ("d_th", "d_ct", "d_z", "d_rnc"):
            assert torch.equal(getattr(of, k), getattr(base_f, k)), (name, k)
    # the forms with the old argument lists are the MSE case
    assert torch.equal(base_c.losses[1:6], base_f.losses[1:6]) if n <= 256 else True
    for bad_code, bad_delta in ((4, 1.0), (-1, 1.0), (2, 0.0), (2, float("nan"))):
        o = _Outs(L, B, rd)
        assert crit(B, float(B), vd.data_ptr(), ld.data_ptr(), thd.data_ptr(), ctd.data_ptr(), zd.data_ptr(), w6, None,
                    o.d_vals.data_ptr(), o.d_th.data_ptr(), o.d_ct.data_ptr(), o.d_z.data_ptr(), o.losses.data_ptr(),
                    o.dws.data_ptr(), 0, bad_code, bad_delta, None) == EINVAL
        assert run_fused(bad_code, bad_delta)[0] == EINVAL
        assert untouched(o.losses, o.d_vals, o.d_th)


# ---- 4. the fused step equals the module route ---------------------------------------------------------------------------------------
def _module_route(dims, P, batch, seed, crit, delta, weights):
    """main :119-150 with reg_loss swapped: module route + autograd (the _module_route of tests/test_gpu_distill.py)."""
    from sdumc_amd.loss import RMSELoss, RnCLoss
    from sdumc_amd.model import get_models
    model = get_models(types.SimpleNamespace(input_dims=dims, model="wengnet_mosei_mult_views_text_missing"))
    model.load_state_dict({"model." + k: v for k, v in P.items()})
    model = model.cuda()
    model.model.seed, model.model._calls = seed, 0
    model.train()
    audio_feat, text_feat, visual_feat, feat4_feat, vals = batch
    losses = {'reg_loss': _module(crit, delta).cuda(), 'rnc_loss': RnCLoss().cuda(), 'rmse_loss': RMSELoss().cuda()}
    vals_out_0, embeddings_0 = model([audio_feat, text_feat, visual_feat, False])
    features_0, rnc_feat_0, text_feat_0, text_query_feat_0 = embeddings_0
    vals_out_1, embeddings_1 = model([audio_feat, feat4_feat, visual_feat, True])
    features_1, rnc_feat_1, text_feat_1, text_query_feat_1 = embeddings_1
    n_views_feature = torch.stack((rnc_feat_0, rnc_feat_1), dim=1)
    terms = [losses['reg_loss'](vals_out_0, vals), losses['reg_loss'](vals_out_1, vals),
             losses['rmse_loss'](text_feat_1, text_feat_0.detach()),
             losses['rmse_loss'](text_query_feat_1, text_query_feat_0.detach()),
             losses['rmse_loss'](features_1, features_0), losses['rnc_loss'](n_views_feature, vals.unsqueeze(1))]
    loss = sum(wi * t for wi, t in zip(weights, terms))
    loss.backward()
    return loss, terms, model.model


@pytest.mark.parametrize("crit,shape", [("l1", "toy"), ("huber", "toy"), ("ccc", "toy"), ("l1", "c1")])
def test_fused_step_equals_module_route(E, crit, shape):
    """One TrainStep(regress=crit) against the reference loop on get_models + the loss modules + autograd, identical parameters,
    Philox seed and call index: the six losses and the total to 2e-5, every gradient tensor to 2e-4 of its own norm (the project's
    parity bars).  losses[3:7] are bit-equal to the default step's, losses[1:3] are not."""
    from oracle import sdumc_oracle as O
    if shape == "c1":
        dims, B, Tn = (1024, 4096, 1024, 4096), 16, (200, 16, 120, 16)
    else:
        dims, B, Tn = TOY_DIMS, 4, TOY_T
    seed, delta = 31, 0.5
    kw = {"regress_delta": delta} if crit == "huber" else {}
    P = O.init_params(dims, seed=0)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=1234)]
    flat, lay = flat_from(E, P, dims)
    ts = E.TrainStep(flat, B, Tn, dims, seed=seed, regress=crit, **kw)
    ts.set_batch(*batch)
    got = ts.run().cpu().numpy()
    loss, terms, mod = _module_route(dims, P, batch, seed, crit, delta, E.DEFAULT_WEIGHTS)
    print(crit, shape, "fused", got[:7], "module", float(loss), [float(t) for t in terms])
    np.testing.assert_allclose(got[0], float(loss), rtol=2e-5)
    np.testing.assert_allclose(got[1:7], [float(t) for t in terms], rtol=2e-5, atol=1e-6)
    gv = lay.views(torch.cat([ts.grads.cpu(), torch.zeros(lay.total - lay.live)]))
    worst = 0.0
    for k in lay.live_names():
        p = mod._get(k)
        assert p.grad is not None, k
        worst = max(worst, close_norm(gv[k], p.grad, 2e-4, k))
    print(crit, shape, "worst relative gradient error", worst)
    ts0 = E.TrainStep(flat_from(E, P, dims)[0], B, Tn, dims, seed=seed)
    ts0.set_batch(*batch)
    base = ts0.run().cpu().numpy()
    assert np.array_equal(base[3:7], got[3:7]) and not np.allclose(base[1:3], got[1:3], rtol=1e-2)


# ---- 5. the default is the default ---------------------------------------------------------------------------------------------------
def test_default_criterion_is_bit_identical(E, L):
    """the option left out, regress='mse' and a raw struct whose two fields were never written: losses, bucket and parameters bit
    for bit."""
    from oracle import sdumc_oracle as O
    dims, B, Tn, seed = TOY_DIMS, 4, TOY_T, 31
    P = O.init_params(dims, seed=0)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=1234)]
    outs = []
    for kw in ({}, {"regress": "mse"}, {"regress": "mse", "regress_delta": 1.0}):
        flat, _ = flat_from(E, P, dims)
        ts = E.TrainStep(flat, B, Tn, dims, seed=seed, **kw)
        assert ts.cfg.regress == L.REGRESS["mse"] == 0 and ts.cfg.regress_delta == 0.0 and L.StepCfg().regress == 0
        ts.set_batch(*batch)
        losses = ts.run().clone()
        torch.cuda.synchronize()
        outs.append((losses, ts.grads.clone(), flat.clone()))
    assert torch.isfinite(outs[0][0]).all()
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])) and all(torch.equal(a, b) for a, b in zip(outs[0], outs[2]))


# ---- 6. reproducible -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crit", CRITERIA)
def test_step_is_bit_reproducible_over_20_runs(E, crit):
    """Twenty train steps at the toy dims and B = 300 per criterion from identical state: losses, the flat gradient bucket and the
    updated parameters are bit-identical.  This guards the summation order (the 256-stride loop entered twice), CCC's double reduce
    included."""
    from oracle import sdumc_oracle as O
    B, dims, Tn = 300, TOY_DIMS, TOY_T
    P = O.init_params(dims, seed=0)
    flat0, lay = flat_from(E, P, dims)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=41)]
    flat = flat0.clone()
    ts = E.TrainStep(flat, B, Tn, dims, seed=5, regress=crit)
    ts.set_batch(*batch)
    ref, bad = None, []
    for rep in range(20):
        flat.copy_(flat0)
        ts.adam_m.zero_()
        ts.adam_v.zero_()
        ts.hyper[1] = 0.0
        ts.rng.set_call(0)
        torch.cuda.synchronize()
        losses = ts.run().clone()
        out = (losses, ts.grads.clone(), flat.clone())
        torch.cuda.synchronize()
        if ref is None:
            ref = out
            assert torch.isfinite(losses).all() and float(out[1].abs().max()) > 0 and float(losses[1:3].min()) > 0
        elif not all(torch.equal(a, b) for a, b in zip(ref, out)):
            bad.append(rep)
    assert not bad, f"{len(bad)} of 19 {crit} train steps differed from the first: runs {bad[:10]}"


# ---- 7. the trainer ------------------------------------------------------------------------------------------------------------------
def test_fused_trainer_takes_the_criterion_and_keys_its_cache_on_it(E):
    from oracle import sdumc_oracle as O
    dims, B, Tn = TOY_DIMS, 4, TOY_T
    P = O.init_params(dims, seed=1)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=2)]
    res = {}
    for crit, kw in (("mse", {}), ("l1", {}), ("huber", {"regress_delta": 0.5}), ("ccc", {})):
        flat, _ = flat_from(E, P, dims)
        ft = E.FusedTrainer(flat, dims, seed=3, regress=crit, **kw)
        res[crit] = ft.step(*batch).cpu().clone()
        (key,) = ft._steps
        assert crit in key and kw.get("regress_delta", 1.0) in key and ft._steps[key].cfg.regress == CODE[crit]
        flat1, _ = flat_from(E, P, dims)
        ts = E.TrainStep(flat1, B, Tn, dims, seed=3, regress=crit, **kw)
        ts.set_batch(*batch)
        assert torch.equal(ts.run().cpu(), res[crit])
        torch.cuda.synchronize()
        assert torch.equal(flat, flat1)
    assert len({tuple(v[1:3].tolist()) for v in res.values()}) == 4
    assert all(torch.equal(v[3:7], res["mse"][3:7]) for v in res.values())


def test_huber_with_guard_ema_and_decoupled_decay_runs(E):
    """regress='huber' beside clip_norm, skip_nonfinite, ema_decay and decoupled_decay: two steps, finite and changed (the composition
    of the four behind the loss stage is held to hand-computed inputs by the tests of each; the criterion only changes the
    gradients they see)."""
    from oracle import sdumc_oracle as O
    dims, B, Tn = TOY_DIMS, 4, TOY_T
    P = O.init_params(dims, seed=1)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=2)]
    flat, lay = flat_from(E, P, dims)
    start = flat.clone()
    ft = E.FusedTrainer(flat, dims, seed=3, regress="huber", regress_delta=0.5, clip_norm=1.0, skip_nonfinite=True, ema_decay=0.99,
                        decoupled_decay=True)
    l1 = ft.step(*batch).cpu().clone()
    mid = flat.clone()
    l2 = ft.step(*batch).cpu().clone()
    torch.cuda.synchronize()
    guard = ft.guard.cpu()
    assert torch.isfinite(l1).all() and torch.isfinite(l2).all() and torch.isfinite(flat).all()
    assert not torch.equal(start, mid) and not torch.equal(mid, flat) and not torch.equal(l1, l2)
    assert guard[3] == 0 and guard[2] == 0 and guard[0] > 0 and 0 < guard[1] <= 1
    assert torch.isfinite(ft.ema_params).all() and not torch.equal(ft.ema_params[:lay.live], start[:lay.live])


@pytest.mark.parametrize("crit", CRITERIA)
def test_nan_label_skips_the_step(E, crit):
    from oracle import sdumc_oracle as O
    dims, B, Tn = TOY_DIMS, 4, TOY_T
    P = O.init_params(dims, seed=1)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=2)]
    batch[4][1] = float("nan")
    flat, _ = flat_from(E, P, dims)
    ts = E.TrainStep(flat, B, Tn, dims, seed=3, regress=crit, skip_nonfinite=True)
    ts.set_batch(*batch)
    before = (flat.clone(), ts.adam_m.clone(), ts.adam_v.clone())
    losses = ts.run().cpu()
    torch.cuda.synchronize()
    assert math.isnan(float(losses[1])) and math.isnan(float(losses[2]))
    assert float(ts.guard[3]) == 1.0 and float(ts.guard[2]) > 0
    assert all(torch.equal(a, b) for a, b in zip(before, (flat, ts.adam_m, ts.adam_v)))


# ---- 8. data parallel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crit", ["l1", "huber"])
def test_two_simulated_ranks_equal_full_batch(E, crit):
    """The harness of tests/test_gpu_distill.py::test_two_simulated_ranks_equal_full_batch at regress = l1 / huber, same bars: the
    entries 1..2 are local sums / B_global and add over ranks exactly like the MSE entries."""
    from oracle import sdumc_oracle as O
    from sdumc_amd import engine
    from sdumc_amd.trainer import HipBackend
    dims, Tn, B, W, seed = TOY_DIMS, (70, 6, 30, 5), 4, 2, 99
    weights = engine.DEFAULT_WEIGHTS
    kw = {"regress_delta": 0.5} if crit == "huber" else {}
    P = O.init_params(dims, seed=3)
    lay = engine.ParamLayout.get(*dims[:3])

    def flat():
        f = torch.zeros(lay.total)
        for k, v in lay.views(f).items():
            v.copy_(P[k])
        return f.cuda()

    gb = [t.cuda() for t in O.synthetic_batch(B * W, Tn, dims, seed=8)]
    full_p = flat()
    ts = engine.TrainStep(full_p, B * W, Tn, dims, weights=weights, seed=seed, regress=crit, **kw)
    ts.set_batch(*gb)
    ref_losses = ts.run().cpu().clone()
    ref_grads = ts.grads.clone()
    bes = []
    for r in range(W):
        be = HipBackend(flat(), B, Tn, dims, weights, 1e-4, (0.9, 0.999), 1e-8, 1e-5, seed, r * B, B * W, regress=crit, **kw)
        be.set_batch(*[t[r * B:(r + 1) * B].contiguous() for t in gb])
        bes.append(be)
    rncs = [be.forward().clone() for be in bes]
    ssd = sum(be.local_ssd().clone() for be in bes)                                   # all-reduce
    feats = torch.cat([p[:B] for p in rncs] + [p[B:] for p in rncs]).contiguous()     # all-gather + reorder
    lab = torch.cat([be.labels for be in bes])
    labels2 = torch.cat([lab, lab]).contiguous()
    ls = [be.loss_backward(ssd, feats, labels2, (r * B, W * B + r * B)).cpu().clone() for r, be in enumerate(bes)]
    gsum = sum(be.backward().clone() for be in bes)                                   # gradient all-reduce
    np.testing.assert_allclose(gsum.cpu().numpy(), ref_grads.cpu().numpy(), rtol=2e-3, atol=2e-6)
    print(crit, "ranks", ls[0][1:7].numpy(), ls[1][1:7].numpy(), "full", ref_losses[1:7].numpy())
    np.testing.assert_allclose((ls[0][1:3] + ls[1][1:3]).numpy(), ref_losses[1:3].numpy(), rtol=1e-5)
    for r in range(W):      # RMSE (from the exchanged sums) and RnC are global already
        np.testing.assert_allclose(ls[r][3:7].numpy(), ref_losses[3:7].numpy(), rtol=1e-5)


def test_ccc_is_refused_under_data_parallelism(E, L):
    """'ccc' raises from DataParallelStep and from HipBackend; regress = 3 written into the raw struct of a rank with B_global = 2B
    is EINVAL from sdumc_loss_backward with nothing touched."""
    from oracle import sdumc_oracle as O
    from sdumc_amd.trainer import DataParallelStep, HipBackend
    dims, B, Tn = TOY_DIMS, 4, TOY_T
    P = O.init_params(dims, seed=1)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=2)]
    flat, _ = flat_from(E, P, dims)
    args = (flat, B, Tn, dims, E.DEFAULT_WEIGHTS, 1e-4, (0.9, 0.999), 1e-8, 1e-5, 3, 0, 2 * B)
    with pytest.raises(L.SdumcError, match="not built under data parallelism"):
        DataParallelStep(flat, B, Tn, dims, regress="ccc")
    with pytest.raises(L.SdumcError, match="not built under data parallelism"):
        HipBackend(*args, regress="ccc")
    be = HipBackend(*args, regress="l1")
    be.set_batch(*batch)
    rnc = be.forward().clone()
    outs = (be.d_vals, be.d_fused, be.d_rnc, be.d_text_hidden, be.d_cross_text, be.losses)
    for o in outs:
        o.fill_(SENTINEL)
    ssd = be.local_ssd().clone()
    feats = torch.cat([rnc[:B], rnc[:B], rnc[B:], rnc[B:]]).contiguous()
    labels2 = be.labels.repeat(4).contiguous()
    be.cfg.regress = 3
    with pytest.raises(L.SdumcError, match="EINVAL"):
        be.loss_backward(ssd, feats, labels2, (0, 2 * B))
    torch.cuda.synchronize()
    assert untouched(*outs)
    be.cfg.regress = 1
    assert torch.isfinite(be.loss_backward(ssd, feats, labels2, (0, 2 * B))[1:7]).all()
    # ... while a rank that IS the whole batch (B_global == B) takes it
    be1 = HipBackend(*args[:-1], B)
    be1.set_batch(*batch)
    be1.forward()
    be1.cfg.regress = 3
    assert torch.isfinite(be1.loss_backward()[1:7]).all()
    torch.cuda.synchronize()


# ---- 9. the raw struct ---------------------------------------------------------------------------------------------------------------
def test_invalid_fields_in_the_raw_struct_are_einval_and_touch_nothing(E, L):
    """regress in (4, -1, 1 << 20), and delta in (0, -1, inf, NaN) under Huber, written behind the Python checks: SDUMC_EINVAL from
    sdumc_train_step before anything is launched -- parameters, moments, hyper, the call counter and losses untouched.  Then the step
    runs with the field repaired."""
    from oracle import sdumc_oracle as O
    dims, B, Tn = TOY_DIMS, 4, TOY_T
    P = O.init_params(dims, seed=1)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=2)]
    flat, _ = flat_from(E, P, dims)
    ts = E.TrainStep(flat, B, Tn, dims, seed=3, regress="huber", regress_delta=0.5)
    ts.set_batch(*batch)
    ts.adam_m.fill_(0.25)
    ts.adam_v.fill_(0.5)
    before = (flat.clone(), ts.adam_m.clone(), ts.adam_v.clone(), ts.hyper.clone(), ts.rng.t.clone(), ts.losses.clone())
    cases = [(bad, 0.5) for bad in (4, -1, 1 << 20)] + [(2, d) for d in (0.0, -1.0, float("inf"), float("nan"))]
    for code, delta in cases:
        ts.cfg.regress, ts.cfg.regress_delta = code, delta
        rc = L.lib.sdumc_train_step(C.byref(ts.dims), C.byref(ts.io), C.byref(ts.cfg), L.current_stream())
        assert rc == EINVAL, (code, delta, rc)
        with pytest.raises(L.SdumcError, match="EINVAL"):
            ts.launch()
    torch.cuda.synchronize()
    after = (flat, ts.adam_m, ts.adam_v, ts.hyper, ts.rng.t, ts.losses)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    ts.cfg.regress, ts.cfg.regress_delta = 2, 0.5
    assert torch.isfinite(ts.run()).all() and not torch.equal(flat, before[0])      # the step itself was fine
    # CCC over a share of a larger batch: refused by the fused step too
    ts.cfg.regress, ts.cfg.B_global = 3, 2 * B
    assert L.lib.sdumc_train_step(C.byref(ts.dims), C.byref(ts.io), C.byref(ts.cfg), L.current_stream()) == EINVAL
    ts.cfg.B_global = B
    assert torch.isfinite(ts.run()).all()
    torch.cuda.synchronize()
