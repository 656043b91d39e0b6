"""GPU: the selectable distillation criterion of the fused step (sdumc_step_cfg.distill: RMSE / cosine / KL) and the three
drop-in loss modules behind it (CosineSimilarityLoss4Seq, KLLoss, CELoss).

Chain of evidence: the modules reproduce tests/golden/distill_losses.npz, recorded from the reference's own classes
(make_distill_goldens.py); the fused step equals the module route (get_models + these modules + autograd, the loop of
main :119-150 with the commented-out tail of :148 switched in), which test_dropin_module.py pins to the reference."""
import types

import numpy as np
import pytest
import torch

# the absolute bar below a reference norm of 1e-7 holds for the contrast head's biases alone, by name (analytically zero up to rounding);
# every other tensor is held to its own norm however small it is
from tests.grad_parity import close_norm

pytestmark = pytest.mark.gpu

DIMS, T_C2 = (1024, 4096, 1024, 4096), (375, 32, 225, 32)
CRITERIA = ("cosine", "kl")


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import engine
    return engine


def close(got, want, tol=1e-4, msg=""):
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


def _module(name):
    from sdumc_amd import loss
    return {"cosine": loss.CosineSimilarityLoss4Seq, "kl": loss.KLLoss, "cos": loss.CosineSimilarityLoss4Seq}[name]()


@pytest.mark.parametrize("crit", ["cos", "kl"])
def test_modules_against_reference_goldens(E, golden, crit):
    """CosineSimilarityLoss4Seq / KLLoss on the three pair shapes ([16,256], [16,7,128], [16,128]) and on the edge rows
    (an all-zero row on either side, identical rows, logits spread over +-30) against the reference's own classes: values 1e-6,
    gradients 1e-5 with the `close` helper of test_gpu_ops.py -- the bars test_losses_against_reference_goldens holds MSE / RMSE
    to.  The spread-logit case needs no wider bar: the reference's own fp32-vs-fp64 gap on kl_edge is 2.6e-7 on the value (11.03)
    and 1.8e-7 on the gradients (largest 0.76), recorded in the fixture as kl_edge_gap.
    Edge rows are compared row by row: the gradient of a zero row is ~1e6 (other / (eps * norm)), and one scale for the whole
    tensor would let it hide the ordinary rows."""
    g = golden("distill_losses")
    m = _module(crit)
    for tag in ("th", "ct", "z", "edge"):
        pre = f"{crit}_edge" if tag == "edge" else tag
        a = torch.from_numpy(g[f"{pre}_a"]).cuda().requires_grad_()
        b = torch.from_numpy(g[f"{pre}_b"]).cuda().requires_grad_()
        l = m(a, b)
        assert l.dim() == 0 and l.requires_grad
        l.backward()
        close(l.reshape(1), g[f"{crit}_{tag}"].reshape(1), 1e-6, f"{crit}_{tag} value")
        want_a, want_b = g[f"{crit}_{tag}_da"], g[f"{crit}_{tag}_db"]
        if tag == "edge":
            for r in range(a.shape[0]):
                close(a.grad[r], want_a[r], 1e-5, f"{crit}_edge da row {r}")
                close(b.grad[r], want_b[r], 1e-5, f"{crit}_edge db row {r}")
        else:
            close(a.grad, want_a, 1e-5, f"{crit}_{tag} da")
            close(b.grad, want_b, 1e-5, f"{crit}_{tag} db")
        # one detached side (main :148: loss(x_1, x_0.detach())): the other side's gradient is unchanged
        a2 = a.detach().clone().requires_grad_()
        m(a2, b.detach()).backward()
        assert torch.equal(a2.grad, a.grad)
        b2 = b.detach().clone().requires_grad_()
        m(a.detach(), b2).backward()
        assert torch.equal(b2.grad, b.grad)
    # identical inputs: value 0 and gradient 0 to rounding, never RMSE's 0/0
    x = torch.from_numpy(g["ct_a"]).cuda()
    a, b = x.clone().requires_grad_(), x.clone().requires_grad_()
    l = m(a, b)
    l.backward()
    assert abs(float(l.detach())) < 1e-5 and float(a.grad.abs().max()) < 1e-6 and float(b.grad.abs().max()) < 1e-6
    if crit == "kl":
        assert float(l.detach()) == 0.0 and not a.grad.any() and not b.grad.any()


def test_ce_module_against_reference_golden(E, golden):
    from sdumc_amd.loss import CELoss
    g = golden("distill_losses")
    x = torch.from_numpy(g["ce_logits"]).cuda().requires_grad_()
    for target in (torch.from_numpy(g["ce_target"]).cuda(), torch.from_numpy(g["ce_target"]).float().cuda()):
        x.grad = None
        l = CELoss()(x, target)
        assert l.dim() == 0
        l.backward()
        close(l.reshape(1), g["ce"].reshape(1), 1e-6, "ce value")
        close(x.grad, g["ce_dlogits"], 1e-5, "ce dlogits")


def test_row_criteria_abi_rejects_bad_arguments(E):
    from sdumc_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    a, b, out = torch.randn(4, 8, device="cuda"), torch.randn(4, 8, device="cuda"), torch.zeros(1, device="cuda")
    st = _lib.current_stream()
    for fn in (lib.sdumc_cosine_fwd_bwd, lib.sdumc_kl_fwd_bwd, lib.sdumc_ce_fwd_bwd):
        assert fn(None, ptr(b), 4, 1, 8, 4.0, 1.0, ptr(out), None, None, st) == -1
        assert fn(ptr(a), ptr(b), 4, 1, 8, 4.0, 1.0, None, None, None, st) == -1
        assert fn(ptr(a), ptr(b), 0, 1, 8, 4.0, 1.0, ptr(out), None, None, st) == -1
        assert fn(ptr(a), ptr(b), 4, 1, 1025, 4.0, 1.0, ptr(out), None, None, st) == -1
        assert fn(ptr(a), ptr(b), 4, 1, 8, 0.0, 1.0, ptr(out), None, None, st) == -1
    assert lib.sdumc_ce_fwd_bwd(ptr(a), ptr(b), 2, 2, 8, 4.0, 1.0, ptr(out), None, None, st) == -1      # groups
    assert lib.sdumc_ce_fwd_bwd(ptr(a), ptr(b), 4, 1, 8, 4.0, 1.0, ptr(out), None, ptr(b), st) == -1    # no gradient to targets
    assert lib.sdumc_kl_fwd_bwd(ptr(a), ptr(b), 4, 1, 8, 4.0, 1.0, ptr(out), None, None, st) == 0       # value only is fine
    torch.cuda.synchronize()


def _module_route(dims, P, batch, seed, crit, weights):
    """main :119-150 with the distillation criterion swapped (the commented-out tail of :148): module route + autograd."""
    from sdumc_amd.loss import MSELoss, RnCLoss
    from sdumc_amd.model import get_models
    model = get_models(types.SimpleNamespace(input_dims=dims, model="wengnet_mosei_mult_views_text_missing"))
    model.load_state_dict({"model." + k: v for k, v in P.items()})
    model = model.cuda()
    model.model.seed, model.model._calls = seed, 0
    model.train()
    audio_feat, text_feat, visual_feat, feat4_feat, vals = batch
    losses = {'reg_loss': MSELoss().cuda(), 'rnc_loss': RnCLoss().cuda(), 'distill': _module(crit).cuda()}
    vals_out_0, embeddings_0 = model([audio_feat, text_feat, visual_feat, False])
    features_0, rnc_feat_0, text_feat_0, text_query_feat_0 = embeddings_0
    vals_out_1, embeddings_1 = model([audio_feat, feat4_feat, visual_feat, True])
    features_1, rnc_feat_1, text_feat_1, text_query_feat_1 = embeddings_1
    n_views_feature = torch.stack((rnc_feat_0, rnc_feat_1), dim=1)
    terms = [losses['reg_loss'](vals_out_0, vals), losses['reg_loss'](vals_out_1, vals),
             losses['distill'](text_feat_1, text_feat_0.detach()),
             losses['distill'](text_query_feat_1, text_query_feat_0.detach()),
             losses['distill'](features_1, features_0), losses['rnc_loss'](n_views_feature, vals.unsqueeze(1))]
    loss = sum(wi * t for wi, t in zip(weights, terms))
    loss.backward()
    return loss, terms, model.model


@pytest.mark.parametrize("crit", CRITERIA)
@pytest.mark.parametrize("shape", ["c1", "toy"])
def test_fused_step_equals_module_route(E, crit, shape):
    """One TrainStep(distill=crit) against the reference loop written on get_models + the loss modules + autograd, identical
    parameters, Philox seed and call index: the six loss values and the total to 2e-5, every gradient tensor to 2e-4 of its own
    norm (README "Parity": outputs 2e-5, gradients 2e-4 relative).  C1 = B 16, T (200, 16, 120, 16), full widths; toy = the
    dims of the drop-in module tests."""
    from oracle import sdumc_oracle as O
    if shape == "c1":
        dims, B, Tn = DIMS, 16, (200, 16, 120, 16)
    else:
        dims, B, Tn = (64, 32, 48, 32), 4, (21, 5, 13, 4)
    seed = 31
    P = O.init_params(dims, seed=0)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=1234)]
    flat, lay = flat_from(E, P, dims)
    ts = E.TrainStep(flat, B, Tn, dims, seed=seed, distill=crit)
    ts.set_batch(*batch)
    got = ts.run().cpu().numpy()
    loss, terms, mod = _module_route(dims, P, batch, seed, crit, E.DEFAULT_WEIGHTS)
    print(crit, shape, "fused", got[:7], "module", float(loss), [float(t) for t in terms])
    np.testing.assert_allclose(got[0], float(loss), rtol=2e-5)
    np.testing.assert_allclose(got[1:7], [float(t) for t in terms], rtol=2e-5, atol=1e-6)
    assert got[3] > 0 and got[4] > 0 and got[5] > 0
    gv = lay.views(torch.cat([ts.grads.cpu(), torch.zeros(lay.total - lay.live)]))
    worst = 0.0
    for k in lay.live_names():
        p = mod._get(k)
        assert p.grad is not None, k
        worst = max(worst, close_norm(gv[k], p.grad, 2e-4, k))
    print(crit, shape, "worst relative gradient error", worst)
    # and it is not the RMSE step under another name
    ts0 = E.TrainStep(flat_from(E, P, dims)[0], B, Tn, dims, seed=seed)
    ts0.set_batch(*batch)
    base = ts0.run().cpu().numpy()
    assert np.array_equal(base[1:3], got[1:3]) and not np.allclose(base[3:6], got[3:6], rtol=1e-2)


def test_default_criterion_is_bit_identical(E):
    """distill='rmse', the argument left out, and a raw sdumc_step_cfg whose field was never written (a zeroed struct) are one
    and the same step: losses, gradients and updated parameters bit for bit."""
    from oracle import sdumc_oracle as O
    from sdumc_amd import _lib
    dims, B, Tn, seed = DIMS, 16, (200, 16, 120, 16), 31
    P = O.init_params(dims, seed=0)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=1234)]
    outs = []
    for kw in ({}, {"distill": "rmse"}):
        flat, _ = flat_from(E, P, dims)
        ts = E.TrainStep(flat, B, Tn, dims, seed=seed, **kw)
        assert ts.cfg.distill == _lib.DISTILL["rmse"] == 0 and _lib.StepCfg().distill == 0
        ts.set_batch(*batch)
        losses = ts.run().clone()
        torch.cuda.synchronize()
        outs.append((losses, ts.grads.clone(), flat.clone()))
    assert torch.isfinite(outs[0][0]).all()
    assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("crit", CRITERIA)
def test_two_simulated_ranks_equal_full_batch(E, crit):
    """The harness of test_gpu_dp.py::test_two_simulated_ranks_equal_full_batch at distill = cosine / kl, same bars.  The
    criterion's entries 3..5 are sums over local rows / B_global, so they add over ranks like the MSE entries; the exchanged sums
    of squares are handed in as before and not read."""
    from oracle import sdumc_oracle as O
    from sdumc_amd import engine
    from sdumc_amd.trainer import HipBackend
    dims, Tn, B, W, seed = (64, 32, 48, 32), (70, 6, 30, 5), 4, 2, 99
    weights = engine.DEFAULT_WEIGHTS
    P = O.init_params(dims, seed=3)
    lay = engine.ParamLayout.get(*dims[:3])

    def flat():
        f = torch.zeros(lay.total)
        for k, v in lay.views(f).items():
            v.copy_(P[k])
        return f.cuda()

    gb = [t.cuda() for t in O.synthetic_batch(B * W, Tn, dims, seed=8)]
    full_p = flat()
    ts = engine.TrainStep(full_p, B * W, Tn, dims, weights=weights, seed=seed, distill=crit)
    ts.set_batch(*gb)
    ref_losses = ts.run().cpu().clone()
    ref_grads = ts.grads.clone()

    bes = []
    for r in range(W):
        be = HipBackend(flat(), B, Tn, dims, weights, 1e-4, (0.9, 0.999), 1e-8, 1e-5, seed, r * B, B * W, distill=crit)
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
    # global loss terms: MSE and cosine / KL entries are local sums / B_global; RnC is global already
    print(crit, "ranks", ls[0][1:7].numpy(), ls[1][1:7].numpy(), "full", ref_losses[1:7].numpy())
    np.testing.assert_allclose((ls[0][1:6] + ls[1][1:6]).numpy(), ref_losses[1:6].numpy(), rtol=1e-5)
    np.testing.assert_allclose(ls[0][6:7].numpy(), ref_losses[6:7].numpy(), rtol=1e-5)
    np.testing.assert_allclose(ls[1][6:7].numpy(), ref_losses[6:7].numpy(), rtol=1e-5)
    for be in bes:
        be.grads.copy_(gsum)
        be.adam(1.0)
    torch.cuda.synchronize()
    assert torch.equal(bes[0].params, bes[1].params)
    np.testing.assert_allclose(((bes[0].params - flat()) * 1e4).cpu().numpy(), ((full_p - flat()) * 1e4).cpu().numpy(),
                               rtol=2e-2, atol=2e-2)
    assert bes[0].rng.call == 2


@pytest.mark.parametrize("crit", CRITERIA)
def test_c2_step_is_bit_reproducible_over_20_runs(E, crit):
    """Twenty C2 train steps (B = 64) per criterion from identical state: losses, the flat gradient bucket and the updated
    parameters are bit-identical.  The form of test_gpu_guard.py with fewer runs: this guards the summation order of the row
    criteria (per-wavefront row order, block partials in index order), not the packed-fp32 hazard."""
    from oracle import sdumc_oracle as O
    B = 64
    P = O.init_params(DIMS, seed=0)
    flat0, lay = flat_from(E, P, DIMS)
    g = torch.Generator(device="cuda").manual_seed(41)
    feats = [torch.randn(B, T_C2[i], DIMS[i], device="cuda", generator=g) for i in range(4)]
    vals = torch.rand(B, device="cuda", generator=g) * 6 - 3
    flat = flat0.clone()
    ts = E.TrainStep(flat, B, T_C2, DIMS, seed=5, planes=True, distill=crit)
    ts.set_batch(*feats, vals)
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
            assert torch.isfinite(losses).all() and float(out[1].abs().max()) > 0 and float(losses[3:6].min()) > 0
        elif not all(torch.equal(a, b) for a, b in zip(ref, out)):
            bad.append(rep)
    assert not bad, f"{len(bad)} of 19 {crit} train steps differed from the first: runs {bad[:10]}"


def test_fused_trainer_takes_the_criterion_and_keys_its_cache_on_it(E):
    from oracle import sdumc_oracle as O
    dims, B, Tn = (64, 32, 48, 32), 4, (21, 5, 13, 4)
    P = O.init_params(dims, seed=1)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=2)]
    res = {}
    for crit in ("rmse", "kl"):
        flat, _ = flat_from(E, P, dims)
        ft = E.FusedTrainer(flat, dims, seed=3, distill=crit)
        res[crit] = ft.step(*batch).cpu().clone()
        (key,) = ft._steps
        assert key[-1] == crit and ft._steps[key].cfg.distill == {"rmse": 0, "kl": 2}[crit]
        flat1, _ = flat_from(E, P, dims)
        ts = E.TrainStep(flat1, B, Tn, dims, seed=3, distill=crit)
        ts.set_batch(*batch)
        assert torch.equal(ts.run().cpu(), res[crit])
    assert not torch.equal(res["rmse"][3:6], res["kl"][3:6])


def test_invalid_criterion_in_the_raw_struct_is_einval_and_touches_nothing(E):
    """distill = 3 written into sdumc_step_cfg behind the Python checks: SDUMC_EINVAL from sdumc_train_step and from
    sdumc_loss_backward, before anything is launched -- parameters, Adam moments, step count and call counter untouched."""
    import ctypes as C
    from oracle import sdumc_oracle as O
    from sdumc_amd import _lib
    from sdumc_amd.trainer import HipBackend
    dims, B, Tn = (64, 32, 48, 32), 4, (21, 5, 13, 4)
    P = O.init_params(dims, seed=1)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=2)]
    flat, _ = flat_from(E, P, dims)
    ts = E.TrainStep(flat, B, Tn, dims, seed=3)
    ts.set_batch(*batch)
    ts.adam_m.fill_(0.25)
    ts.adam_v.fill_(0.5)
    before = (flat.clone(), ts.adam_m.clone(), ts.adam_v.clone(), ts.hyper.clone(), ts.rng.t.clone(), ts.losses.clone())
    for bad in (3, -1, 1 << 20):
        ts.cfg.distill = bad
        rc = _lib.lib.sdumc_train_step(C.byref(ts.dims), C.byref(ts.io), C.byref(ts.cfg), _lib.current_stream())
        assert rc == -1, (bad, rc)      # SDUMC_EINVAL
        with pytest.raises(_lib.SdumcError, match="EINVAL"):
            ts.launch()
    torch.cuda.synchronize()
    after = (flat, ts.adam_m, ts.adam_v, ts.hyper, ts.rng.t, ts.losses)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    ts.cfg.distill = 0
    assert torch.isfinite(ts.run()).all() and not torch.equal(flat, before[0])      # the step itself was fine
    be = HipBackend(flat, B, Tn, dims, E.DEFAULT_WEIGHTS, 1e-4, (0.9, 0.999), 1e-8, 1e-5, 3, 0, B)
    be.set_batch(*batch)
    be.forward()
    be.cfg.distill = 3
    with pytest.raises(_lib.SdumcError, match="EINVAL"):
        be.loss_backward()
    torch.cuda.synchronize()
