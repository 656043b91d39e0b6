"""GPU: SupConLoss (the reference's toolkit/utils/loss.py:143-240) as a HIP kernel -- the C entry, the drop-in class, and the
fused step's selectable contrastive criterion (sdumc_step_cfg.contrast: Rank-N-Contrast / SupCon).

Chain of evidence: the kernel reproduces tests/golden/supcon.npz, recorded in float64 from the reference's own class
(make_supcon_goldens.py); for shapes without a fixture it is compared with tests/supcon_ref.py, which test_supcon_cpu.py pins
to that fixture at 1e-12; the fused step equals the literal loop (get_models twice + the drop-in losses + SupConLoss(normalize=
True) + autograd), which test_dropin_module.py pins to the reference.

Bars of the kernel = the reference's own fp32 rounding, recorded per case in the fixture (<name>_gap), times 4 (torch's CPU sums
are pairwise, a wave-order sum of up to N terms is not), floored at one fp32 ulp of the quantity (some recorded gaps are
accidentally tiny):  value 4 * max(gap_value, 2^-23 |v|);  gradient, relative norm 4 * max(gap_relnorm, 2^-23);  gradient, largest
error 4 * max(gap_maxabs, 2^-23 max|g|).  Shapes without a fixture take the gaps recorded at N = 1024 (n1024_gap), each as a
fraction of the scale recorded beside it (|value|, max|g|) applied to the shape's own scale, with the same floors."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import supcon_ref  # noqa: E402

# the absolute bar below a reference norm of 1e-7 holds for the contrast head's biases alone, by name (analytically zero up to rounding);
# every other tensor is held to its own norm however small it is
from tests.grad_parity import close_norm

pytestmark = pytest.mark.gpu

DIMS = (1024, 4096, 1024, 4096)
CASES = ("cls7", "simclr", "one", "mask", "v1", "odd", "t05", "prenorm", "zero", "round")
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import engine
    return engine


def flat_from(E, P, dims):
    lay = E.ParamLayout.get(*dims[:3])
    flat = torch.zeros(lay.total)
    for k, v in lay.views(flat).items():
        v.copy_(P[k])
    return flat.cuda(), lay


def spread_params(P, gain=2.25):
    """The step tests' parameters: the oracle's init with every weight matrix scaled by `gain`.  At the plain init the network is
    bias-dominated and every sample's contrast row is the same to seven digits (oracle forward, eval mode: smallest cosine between
    two rows 0.9999996 at toy dims, 0.99999997 at C1).  SupCon's value is then log(N - 1) whatever the labels say, so the step test
    could not tell one class reading from another, and the contrast head's last bias receives a sum over rows that cancels to
    1e-4 .. 3e-6 of its terms -- below what fp32 rows resolve, on either side of the comparison.  With gain 2.25 (just under the gain at
    which the activations start to grow from layer to layer) the rows spread (smallest cosine 0.01 / 0.56), the value depends on
    the labels, that sum cancels to no less than 1/7 of its terms, and the activations stay O(1)."""
    return {k: (v * gain if k.endswith(".weight") and v.dim() == 2 and v.shape[0] > 1 and "layer_normali" not in k else v.clone())
            for k, v in P.items()}


def ratios(tag, v, g, want_v, want_g, gap_v, gap_max, gap_rel):
    """error / bar of the value, of the gradient by relative norm and of its largest error; printed, then returned."""
    v, g = float(v), g.detach().cpu().double().reshape(want_g.shape)
    r = (abs(v - want_v) / (4 * max(gap_v, ULP * abs(want_v))),
         float((g - want_g).norm() / want_g.norm()) / (4 * max(gap_rel, ULP)),
         float((g - want_g).abs().max()) / (4 * max(gap_max, ULP * float(want_g.abs().max()))))
    print(f"supcon {tag:24s} error / bar: value {r[0]:.3f}  grad rel-norm {r[1]:.3f}  grad max-abs {r[2]:.3f}")
    return r


def golden_case(g, name):
    o = g[f"{name}_opts"]
    opts = dict(temperature=float(o[0]), base_temperature=float(o[1]), contrast_mode="all" if o[2] else "one", normalize=bool(o[3]))
    extra = {k: torch.from_numpy(g[f"{name}_{k}"]).cuda() for k in ("labels", "mask") if f"{name}_{k}" in g.files}
    return opts, int(o[4]), extra


@pytest.mark.parametrize("name", CASES)
def test_class_and_entry_against_reference_goldens(E, golden, name):
    """Every recorded case through the drop-in class (autograd) and through ops.supcon_fwd_bwd (weight 0.5: the gradient is scaled,
    the value is not), against the reference's float64 value and gradient at the bars of the module docstring.  The class has no
    label mode: for `round` it is given rint(labels), the entry gets the recorded labels and label_mode 1."""
    from sdumc_amd import ops
    from sdumc_amd.loss import SupConLoss
    g = golden("supcon")
    opts, mode, extra = golden_case(g, name)
    want_v, want_g, gap = float(g[f"{name}_value"]), torch.from_numpy(g[f"{name}_grad"]), g[f"{name}_gap"]
    feat = torch.from_numpy(g[f"{name}_feat"]).cuda().requires_grad_()
    crit = SupConLoss(opts["temperature"], opts["contrast_mode"], opts["base_temperature"], normalize=opts["normalize"])
    cls_extra = {k: (torch.round(v) if mode == 1 else v) for k, v in extra.items()}
    l = crit(feat, **cls_extra)
    assert l.dim() == 0 and l.requires_grad and l.dtype == torch.float32
    l.backward()
    r_cls = ratios(name + " class", l.detach(), feat.grad, want_v, want_g, gap[0], gap[1], gap[2])
    bsz, views, D = feat.shape
    rows = feat.detach().transpose(0, 1).contiguous().view(bsz * views, D)
    lo, df = ops.supcon_fwd_bwd(rows, bsz, views, labels=extra.get("labels"), mask=extra.get("mask"),
                                temperature=opts["temperature"], base_temperature=opts["base_temperature"],
                                contrast_all=opts["contrast_mode"] == "all", label_mode=mode, normalize=opts["normalize"], weight=0.5)
    r_ops = ratios(name + " entry", lo, 2.0 * df.view(views, bsz, D).transpose(0, 1), want_v, want_g, gap[0], gap[1], gap[2])
    assert torch.equal(lo.reshape(()), l.detach())
    assert max(r_cls) <= 1.0 and max(r_ops) <= 1.0, (r_cls, r_ops)
    # a scaled upstream gradient scales the result; a value-only call returns the same value
    feat2 = feat.detach().clone().requires_grad_()
    (3.0 * crit(feat2, **cls_extra)).backward()
    assert torch.allclose(feat2.grad, 3.0 * feat.grad, rtol=1e-6, atol=0)
    with torch.no_grad():
        assert torch.equal(crit(feat.detach(), **cls_extra), l.detach())


def test_entry_is_bit_identical_over_20_calls(E, golden):
    from sdumc_amd.loss import SupConLoss
    g = golden("supcon")
    for name in ("cls7", "mask", "odd"):
        opts, _, extra = golden_case(g, name)
        crit = SupConLoss(opts["temperature"], opts["contrast_mode"], opts["base_temperature"], normalize=opts["normalize"])
        ref = None
        for _ in range(20):
            feat = torch.from_numpy(g[f"{name}_feat"]).cuda().requires_grad_()
            l = crit(feat, **extra)
            l.backward()
            out = (l.detach().clone(), feat.grad.clone())
            ref = ref or out
            assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1]), name


# bsz, n_views, D, normalised in the kernel
LARGER = [(65, 1, 64, True), (257, 1, 64, True), (512, 2, 64, True), (1024, 2, 64, True),
          (16, 2, 1, True), (16, 2, 1, False), (16, 2, 3, True), (16, 2, 256, True), (16, 2, 1024, True)]


@pytest.fixture(scope="module")
def larger_refs():
    """The float64 restatement of every larger shape, computed once on the CPU: {shape: (feat, labels, value, grad, zero_scale)}.
    zero_scale (D = 1 normalised only): a normalised 1-wide row is +-1 whatever its length, so the gradient is analytically ZERO and
    what either side returns is the rounding of (g - xhat (xhat . g)) / |x|, a cancelling difference of terms of size
    |dLoss/dxhat| / |x|: zero_scale is the largest of those, from the restatement on the pre-normalised rows."""
    out = {}
    for bsz, views, D, norm in LARGER:
        gen = torch.Generator().manual_seed(1000 * bsz + 10 * D + views)
        feat = torch.randn(bsz, views, D, generator=gen)
        labels = torch.randint(0, 7, (bsz,), generator=gen).float()
        v, gr = supcon_ref.value_and_grad(feat, labels=labels, normalize=norm)
        assert torch.isfinite(v) and torch.isfinite(gr).all()
        zero_scale = None
        if D == 1 and norm:
            _, gh = supcon_ref.value_and_grad(torch.nn.functional.normalize(feat, dim=-1), labels=labels, normalize=False)
            zero_scale = float((gh / feat.abs().double()).abs().max())
            assert float(gr.abs().max()) < 1e-12 * zero_scale
        out[(bsz, views, D, norm)] = (feat, labels, float(v), gr, zero_scale)
    return out


@pytest.mark.parametrize("shape", LARGER, ids=lambda s: f"N{s[0] * s[1]}_D{s[2]}" + ("" if s[3] else "_raw"))
def test_larger_shapes_against_the_restatement(E, golden, larger_refs, shape):
    """N = 65, 257, 1024, 2048 at D = 64 (N off the wavefront and workgroup sizes, more than one stride of every loop, the built
    maximum) and D = 1, 3, 256, 1024 at N = 32 (off the vector width, one lane, the built maximum), seven classes, normalised in
    the kernel, against tests/supcon_ref.py in float64.  Bars: the N = 1024 gaps of the fixture (module docstring).
    D = 1 normalised has an analytically zero gradient (larger_refs): its value is held to the bar, its gradient to
    4 * 2^-23 * zero_scale in absolute terms, and D = 1 is run once more on the raw rows (normalize=False: finite in float64
    at this width), where the gradient is an ordinary one and takes the ordinary bars."""
    from sdumc_amd.loss import SupConLoss
    n1024 = golden("supcon")["n1024_gap"]      # value gap, grad max-abs gap, grad rel-norm gap, |value|, max|g|
    feat, labels, want_v, want_g, zero_scale = larger_refs[shape]
    x = feat.cuda().requires_grad_()
    l = SupConLoss(normalize=shape[3])(x, labels.cuda())
    l.backward()
    assert torch.isfinite(l) and torch.isfinite(x.grad).all()
    tag = "N%d D%d%s" % (shape[0] * shape[1], shape[2], "" if shape[3] else " raw")
    if zero_scale is not None:
        rv = abs(float(l.detach()) - want_v) / (4 * max(n1024[0] / n1024[3] * abs(want_v), ULP * abs(want_v)))
        rg = float((x.grad.cpu().double() - want_g).abs().max()) / (4 * ULP * zero_scale)
        print(f"supcon {tag:24s} error / bar: value {rv:.3f}  zero gradient, max-abs {rg:.3g}")
        assert rv <= 1.0 and rg <= 1.0, (rv, rg)
        return
    r = ratios(tag, l.detach(), x.grad, want_v, want_g,
               n1024[0] / n1024[3] * abs(want_v), n1024[1] / n1024[4] * float(want_g.abs().max()), n1024[2])
    assert max(r) <= 1.0, r


def test_entry_rejects_bad_arguments_before_a_launch(E):
    from sdumc_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    f = torch.randn(8, 16, device="cuda")
    y, m = torch.zeros(4, device="cuda"), torch.eye(4, device="cuda")
    out, df = torch.full((1,), 7.0, device="cuda"), torch.full((8, 16), 7.0, device="cuda")
    ws = torch.zeros(lib.sdumc_supcon_workspace_bytes(4, 2, 1) + 8, dtype=torch.uint8, device="cuda")
    st = _lib.current_stream()

    def call(feats=ptr(f), labels=ptr(y), mask=None, bsz=4, views=2, dim=16, allv=1, mode=0, norm=1, t=0.07, bt=0.07, loss=ptr(out),
             w=ptr(ws)):
        return lib.sdumc_supcon_fwd_bwd(feats, labels, mask, bsz, views, dim, allv, mode, norm, t, bt, 1.0, loss, ptr(df), w, st)
    assert call(feats=None) == -1 and call(loss=None) == -1 and call(w=None) == -1
    assert call(mask=ptr(m)) == -1                                   # labels and mask both given
    assert call(views=0) == -1 and call(bsz=0) == -1 and call(dim=0) == -1
    assert call(t=0.0) == -1 and call(t=-1.0) == -1 and call(bt=0.0) == -1
    assert call(bsz=1, views=1) == -1                                # N = 1: no contrast row at all
    assert call(bsz=1025, views=2) == -1 and call(dim=1025) == -1    # beyond the built limits
    assert call(mode=2) == -1 and call(allv=2) == -1 and call(norm=-1) == -1
    assert call(w=ptr(ws) + 4) == -1                                 # the workspace holds doubles
    torch.cuda.synchronize()
    assert float(out) == 7.0 and bool((df == 7.0).all())              # nothing ran
    assert call() == 0 and call(labels=None) == 0 and call(labels=None, mask=ptr(m)) == 0
    torch.cuda.synchronize()
    assert float(out) != 7.0 and not bool((df == 7.0).any())


def _literal_loop(dims, P, batch, seed, classes, weights):
    """main :119-150 with SupConLoss over the stacked contrast features in RnC's place: get_models twice, the drop-in losses,
    autograd.  The rows are L2-normalised by the criterion itself (normalize=True: the driver's Proj, main :61-69)."""
    from sdumc_amd.loss import MSELoss, RMSELoss, SupConLoss
    from sdumc_amd.model import get_models
    model = get_models(types.SimpleNamespace(input_dims=dims, model="wengnet_mosei_mult_views_text_missing"))
    model.load_state_dict({"model." + k: v for k, v in P.items()})
    model = model.cuda()
    model.model.seed, model.model._calls = seed, 0
    model.train()
    audio_feat, text_feat, visual_feat, feat4_feat, vals = batch
    reg, rmse, con = MSELoss().cuda(), RMSELoss().cuda(), SupConLoss(normalize=True).cuda()
    vals_out_0, (features_0, rnc_feat_0, text_feat_0, text_query_feat_0) = model([audio_feat, text_feat, visual_feat, False])
    vals_out_1, (features_1, rnc_feat_1, text_feat_1, text_query_feat_1) = model([audio_feat, feat4_feat, visual_feat, True])
    n_views_feature = torch.stack((rnc_feat_0, rnc_feat_1), dim=1)
    cls = torch.round(vals) if classes == "round" else vals
    terms = [reg(vals_out_0, vals), reg(vals_out_1, vals), rmse(text_feat_1, text_feat_0.detach()),
             rmse(text_query_feat_1, text_query_feat_0.detach()), rmse(features_1, features_0), con(n_views_feature, cls)]
    loss = sum(wi * t for wi, t in zip(weights, terms))
    loss.backward()
    return loss, terms, model.model


@pytest.mark.parametrize("classes", ["eq", "round"])
@pytest.mark.parametrize("shape", ["c1", "toy"])
def test_fused_step_equals_the_literal_loop(E, shape, classes):
    """One TrainStep(contrast='supcon') against the literal loop, identical parameters, Philox seed and call index: the six loss
    values and the total to 2e-5, every gradient tensor to 2e-4 of its own norm (the bars of test_gpu_distill.py).  The step's
    Adam update is the one its own gradient bucket implies.  C1 = B 16, T (200, 16, 120, 16), full widths; toy = the dims of
    test_dropin_module.py.  Parameters: spread_params (the plain init gives SupCon nothing to tell apart).  Labels: sentiment
    scores with repeats, so that 'eq' has positives beyond the sample's other view."""
    from oracle import sdumc_oracle as O
    if shape == "c1":
        dims, B, Tn = DIMS, 16, (200, 16, 120, 16)
    else:
        dims, B, Tn = (64, 32, 48, 32), 4, (21, 5, 13, 4)
    seed, lr, wd, eps = 31, 1e-4, 1e-5, 1e-8
    P = spread_params(O.init_params(dims, seed=0))
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=1234)]
    gen = torch.Generator().manual_seed(5)
    vals = (torch.randint(-6, 7, (B,), generator=gen).float() * 0.4)      # multiples of 0.4 in [-2.4, 2.4]: repeats, and not integers
    vals[1] = vals[0]
    batch[4] = vals.cuda()
    flat, lay = flat_from(E, P, dims)
    before = flat.clone()
    ts = E.TrainStep(flat, B, Tn, dims, seed=seed, contrast="supcon", contrast_classes=classes)
    assert (ts.cfg.contrast, ts.cfg.supcon_label_mode) == (1, int(classes == "round"))
    ts.set_batch(*batch)
    got = ts.run().cpu().numpy()
    loss, terms, mod = _literal_loop(dims, P, batch, seed, classes, E.DEFAULT_WEIGHTS)
    print(shape, classes, "fused", got[:7], "loop", float(loss), [float(t) for t in terms])
    np.testing.assert_allclose(got[0], float(loss), rtol=2e-5)
    np.testing.assert_allclose(got[1:7], [float(t) for t in terms], rtol=2e-5, atol=1e-6)
    assert got[6] > 0 and got[7] == 0
    gv = lay.views(torch.cat([ts.grads.cpu(), torch.zeros(lay.total - lay.live)]))
    worst = 0.0
    for k in lay.live_names():
        p = mod._get(k)
        assert p.grad is not None, k
        worst = max(worst, close_norm(gv[k], p.grad, 2e-4, k))
    print(shape, classes, "worst relative gradient error", worst)
    # the Adam step that was applied: first step, so m / (1 - b1) = g and v / (1 - b2) = g^2 with g = grad + wd * p
    gg = ts.grads.double() + wd * before[:lay.live].double()
    want = before[:lay.live].double() - lr * gg / (gg.abs() + eps)
    assert float((flat[:lay.live].double() - want).abs().max()) < 2e-7 and not torch.equal(flat, before)
    # and it is not the RnC step under another name: the other five entries are the default step's, bit for bit
    ts0 = E.TrainStep(flat_from(E, P, dims)[0], B, Tn, dims, seed=seed)
    ts0.set_batch(*batch)
    base = ts0.run().cpu().numpy()
    assert np.array_equal(base[1:6], got[1:6]) and not np.allclose(base[6], got[6], rtol=1e-2)


def test_the_two_class_readings_differ_and_the_temperature_arrives(E):
    from oracle import sdumc_oracle as O
    dims, B, Tn = (64, 32, 48, 32), 4, (21, 5, 13, 4)
    P = spread_params(O.init_params(dims, seed=0))
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=1234)]
    batch[4] = torch.tensor([0.2, -0.3, 1.6, 2.4]).cuda()      # rint: 0, -0, 2, 2 -> two classes; all four labels differ
    res = {}
    for key, kw in {"eq": {}, "round": {"contrast_classes": "round"}, "t05": {"contrast_temperature": 0.5}}.items():
        ts = E.TrainStep(flat_from(E, P, dims)[0], B, Tn, dims, seed=3, contrast="supcon", **kw)
        ts.set_batch(*batch)
        res[key] = ts.run().cpu().clone()
        # the step's entry 6 is the class on the step's own contrast rows
        from sdumc_amd.loss import SupConLoss
        cls = torch.round(batch[4]) if key == "round" else batch[4]
        want = SupConLoss(temperature=0.5 if key == "t05" else 0.07, normalize=True)(torch.stack((ts.rnc[:B], ts.rnc[B:]), dim=1), cls)
        np.testing.assert_allclose(float(res[key][6]), float(want), rtol=1e-6)
    assert torch.isfinite(torch.stack(list(res.values()))).all()
    assert not torch.allclose(res["eq"][6], res["round"][6], rtol=1e-3) and not torch.allclose(res["eq"][6], res["t05"][6], rtol=1e-3)


def test_default_criterion_is_bit_identical(E):
    """contrast='rnc', the argument left out and contrast_temperature=2.0 spelt out are one and the same step: losses, gradients and
    parameters bit for bit after 3 steps."""
    from oracle import sdumc_oracle as O
    from sdumc_amd import _lib
    dims, B, Tn, seed = DIMS, 16, (200, 16, 120, 16), 31
    P = O.init_params(dims, seed=0)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=1234)]
    outs = []
    for kw in ({}, {"contrast": "rnc"}, {"contrast": "rnc", "contrast_temperature": 2.0, "contrast_classes": "round"}):
        flat, _ = flat_from(E, P, dims)
        ts = E.TrainStep(flat, B, Tn, dims, seed=seed, **kw)
        assert ts.cfg.contrast == _lib.CONTRAST["rnc"] == 0 and ts.cfg.temperature == 2.0 and ts.cfg.supcon_temperature == 0.0
        ts.set_batch(*batch)
        ls = [ts.run().clone() for _ in range(3)]
        torch.cuda.synchronize()
        outs.append(ls + [ts.grads.clone(), flat.clone()])
    assert torch.isfinite(torch.stack(outs[0][:3])).all() and not torch.equal(outs[0][0], outs[0][1])
    for other in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], other))


def test_invalid_contrast_in_the_raw_struct_is_einval_and_touches_nothing(E):
    """contrast = 2 (and a SupCon temperature of 0, a label mode of 2) written into sdumc_step_cfg behind the Python checks:
    SDUMC_EINVAL from sdumc_train_step and from sdumc_loss_backward before anything is launched -- parameters, Adam moments, step
    count, call counter and losses untouched.  SupCon with gathered rnc features (the data-parallel call) is refused the same way,
    and DataParallelStep refuses the criterion at construction."""
    import ctypes as C
    from oracle import sdumc_oracle as O
    from sdumc_amd import _lib
    from sdumc_amd.trainer import DataParallelStep, HipBackend
    dims, B, Tn = (64, 32, 48, 32), 4, (21, 5, 13, 4)
    P = O.init_params(dims, seed=1)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=2)]
    flat, _ = flat_from(E, P, dims)
    ts = E.TrainStep(flat, B, Tn, dims, seed=3, contrast="supcon")
    ts.set_batch(*batch)
    ts.adam_m.fill_(0.25)
    ts.adam_v.fill_(0.5)
    before = (flat.clone(), ts.adam_m.clone(), ts.adam_v.clone(), ts.hyper.clone(), ts.rng.t.clone(), ts.losses.clone())
    good = (ts.cfg.contrast, ts.cfg.supcon_temperature, ts.cfg.supcon_label_mode)
    for bad in ((2, good[1], 0), (-1, good[1], 0), (1 << 20, good[1], 0), (1, 0.0, 0), (1, -0.07, 0), (1, good[1], 2)):
        ts.cfg.contrast, ts.cfg.supcon_temperature, ts.cfg.supcon_label_mode = bad
        rc = _lib.lib.sdumc_train_step(C.byref(ts.dims), C.byref(ts.io), C.byref(ts.cfg), _lib.current_stream())
        assert rc == -1, (bad, rc)      # SDUMC_EINVAL
        with pytest.raises(_lib.SdumcError, match="EINVAL"):
            ts.launch()
    torch.cuda.synchronize()
    after = (flat, ts.adam_m, ts.adam_v, ts.hyper, ts.rng.t, ts.losses)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    ts.cfg.contrast, ts.cfg.supcon_temperature, ts.cfg.supcon_label_mode = good
    assert torch.isfinite(ts.run()).all() and not torch.equal(flat, before[0])      # the step itself was fine
    be = HipBackend(flat, B, Tn, dims, E.DEFAULT_WEIGHTS, 1e-4, (0.9, 0.999), 1e-8, 1e-5, 3, 0, B)
    be.set_batch(*batch)
    rnc = be.forward().clone()
    be.losses.fill_(-5.0)
    be.cfg.contrast = 2
    with pytest.raises(_lib.SdumcError, match="EINVAL"):
        be.loss_backward()
    be.cfg.contrast, be.cfg.supcon_temperature = 1, 0.07
    labels2 = torch.cat([be.labels, be.labels]).contiguous()
    with pytest.raises(_lib.SdumcError, match="EINVAL"):      # gathered features: the exchange carries RnC records only
        be.loss_backward(be.local_ssd().clone(), rnc, labels2, (0, B))
    torch.cuda.synchronize()
    assert bool((be.losses == -5.0).all())
    assert torch.isfinite(be.loss_backward()[:7]).all()       # the single-GPU call with SupCon is served
    with pytest.raises(_lib.SdumcError, match="data parallelism"):
        DataParallelStep(flat, B, Tn, dims, contrast="supcon")


def test_graph_replay_of_a_supcon_step_equals_eager(E):
    """The form of test_gpu_net.py::test_graph_replay_equals_eager_and_advances_state with contrast='supcon': three replays of the
    captured step equal three eager launches bit for bit (losses and parameters), state advancing alike."""
    from oracle import sdumc_oracle as O
    from sdumc_amd import _lib
    dims, B, Tn = (64, 32, 64, 32), 8, (40, 6, 20, 6)
    P = O.init_params(dims, seed=2)
    batch = O.synthetic_batch(B, Tn, dims, seed=3)
    res = []
    try:
        _lib.lib.sdumc_set_chain_cluster(0)      # a capture takes chain.hip's kernels: compare like with like
        _lib.lib.sdumc_set_background_lane(0)
        for use_graph in (False, True):
            flat, lay = flat_from(E, P, dims)
            ts = E.TrainStep(flat, B, Tn, dims, seed=5, contrast="supcon", contrast_classes="round")
            ts.set_batch(*[t.cuda() for t in batch])
            if use_graph:
                ts.capture()
            ls = [ts.run().cpu().clone() for _ in range(3)]
            torch.cuda.synchronize()
            res.append((flat.cpu().clone(), ls, ts.rng.call, float(ts.hyper[1])))
    finally:                                     # process-wide switches (tests/conftest.py restores them too)
        _lib.lib.sdumc_set_chain_cluster(1)
        _lib.lib.sdumc_set_background_lane(3)
    assert torch.equal(res[0][0], res[1][0]), "graph replay must equal eager launches bit for bit"
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a, b) and torch.isfinite(a).all() and float(a[6]) > 0
    assert res[0][2] == res[1][2] == 6 and res[0][3] == res[1][3] == 3.0
    assert not torch.equal(res[0][1][0], res[0][1][1])


def test_fused_trainer_keeps_one_criterion_per_cache_key(E):
    """Two batch shapes through one FusedTrainer(contrast='supcon'): two cached steps, both SupCon, each equal to a TrainStep of
    its shape continuing the same run; an RnC trainer's keys differ from the SupCon trainer's."""
    from oracle import sdumc_oracle as O
    dims = (64, 32, 48, 32)
    shapes = [(4, (21, 5, 13, 4)), (3, (17, 4, 9, 3))]
    P = O.init_params(dims, seed=1)
    batches = [[t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=2 + i)] for i, (B, Tn) in enumerate(shapes)]
    keys, res = {}, {}
    for crit in ("rnc", "supcon"):
        flat, _ = flat_from(E, P, dims)
        ft = E.FusedTrainer(flat, dims, seed=3, contrast=crit, contrast_classes="round")
        res[crit] = [ft.step(*b).cpu().clone() for b in batches]
        assert len(ft._steps) == 2
        for key, ts in ft._steps.items():
            assert key[-4:] == (crit, None, "round", "rmse") and ts.cfg.contrast == {"rnc": 0, "supcon": 1}[crit]
            assert ts.cfg.supcon_label_mode == (1 if crit == "supcon" else 0)
        keys[crit] = set(ft._steps)
    assert not keys["rnc"] & keys["supcon"]
    assert all(torch.isfinite(l).all() for l in res["supcon"])
    assert np.array_equal(res["rnc"][0][1:6].numpy(), res["supcon"][0][1:6].numpy()) and not torch.equal(res["rnc"][0][6], res["supcon"][0][6])
    # the first step of the SupCon trainer is the TrainStep of that shape
    flat1, _ = flat_from(E, P, dims)
    ts = E.TrainStep(flat1, shapes[0][0], shapes[0][1], dims, seed=3, contrast="supcon", contrast_classes="round")
    ts.set_batch(*batches[0])
    assert torch.equal(ts.run().cpu(), res["supcon"][0])
