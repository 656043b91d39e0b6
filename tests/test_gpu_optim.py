"""GPU: sdumc_amd.optim.Adam / sdumc_adam_multi -- bit-identity with the flat-bucket kernel (ops.adam_step), semantics
against torch.optim.Adam in float64, the reference's literal loop, checkpoint interchange with the fused step, moving
pointers, grad-set changes and determinism.

The semantic test bounds the deviation from float64 by twice the flat kernel's own deviation from the same float64 run on the
same inputs (`traj` below: 5 steps, 11 tensors / 19 312 elements, lr 1e-3 then 5e-4, weight_decay 1e-5), measured in the test
itself and printed per step (run with -s)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(256, 48), (1,), (3,), (4,), (5,), (255,), (256,), (257,), (1023,), (1025,), (4099,)]
STEPS, WD, LR0 = 5, 1e-5, 1e-3
OFFSET_GRAD, TRANSPOSED_GRAD = 6, 0       # SHAPES[6]: gradient = a view from element 1 of a larger tensor; SHAPES[0]: a transposed view


def _lr_lambda(e):
    return 1.0 if e < 2 else 0.5           # lr changes before step 3


def _numel(shape):
    return int(np.prod(shape))


def _offsets():
    offs, o = [], 0
    for s in SHAPES:
        offs.append(o)
        o += _numel(s)                      # back to back: most bases are only 4-byte aligned
    return offs, o


def _inputs():
    gen = torch.Generator().manual_seed(1234)
    offs, total = _offsets()
    p0 = torch.randn(total, generator=gen) * 0.1
    grads = [[torch.randn(s, generator=gen) * (10.0 ** ((i % 5) - 3)) for i, s in enumerate(SHAPES)] for _ in range(STEPS)]
    return p0, grads


def _place_grad(i, g, dev):
    """The gradient tensor as autograd might leave it: its own tensor, a view at an odd element offset, or non-contiguous."""
    g = g.to(dev)
    if i == OFFSET_GRAD:
        big = torch.zeros(g.numel() + 5, device=dev)
        big[1:1 + g.numel()] = g.reshape(-1)
        return big[1:1 + g.numel()].view(g.shape)
    if i == TRANSPOSED_GRAD:
        t = g.t().contiguous().t()
        assert not t.is_contiguous() and torch.equal(t, g)
        return t
    return g


def _run_ours(p0, grads, dev):
    from sdumc_amd.optim import Adam
    offs, total = _offsets()
    flat = p0.to(dev).clone()
    params = [torch.nn.Parameter(flat[o:o + _numel(s)].view(s)) for o, s in zip(offs, SHAPES)]
    assert sum(p.data_ptr() % 16 != 0 for p in params) >= 4
    opt = Adam(params, lr=LR0, weight_decay=WD)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=_lr_lambda)
    rec = []
    for k in range(STEPS):
        for i, p in enumerate(params):
            p.grad = _place_grad(i, grads[k][i], dev)
        opt.step()
        sched.step()
        rec.append({"p": flat.clone(),
                    "m": torch.cat([opt.state[p]["exp_avg"].reshape(-1) for p in params]),
                    "v": torch.cat([opt.state[p]["exp_avg_sq"].reshape(-1) for p in params]),
                    "hyper": opt._hyper.clone(), "step": [float(opt.state_dict()["state"][i]["step"]) for i in range(len(params))]})
    return rec


def _run_flat(p0, grads, dev):
    """The oracle: the flat-bucket kernel on an aligned bucket holding the same tensors concatenated."""
    from sdumc_amd import ops
    P = p0.to(dev).clone()
    m, v = torch.zeros_like(P), torch.zeros_like(P)
    hyper = torch.tensor([LR0, 0.0, 0.0, 0.0], device=dev)
    assert P.data_ptr() % 16 == 0
    rec = []
    for k in range(STEPS):
        hyper[0] = LR0 * _lr_lambda(k)
        G = torch.cat([g.reshape(-1) for g in grads[k]]).to(dev)
        ops.adam_step(P, G, m, v, hyper, weight_decay=WD)
        rec.append({"p": P.clone(), "m": m.clone(), "v": v.clone(), "hyper": hyper.clone()})
    return rec


def _run_torch64(p0, grads):
    offs, _ = _offsets()
    params = [torch.nn.Parameter(p0[o:o + _numel(s)].view(s).double().clone()) for o, s in zip(offs, SHAPES)]
    opt = torch.optim.Adam(params, lr=LR0, weight_decay=WD, foreach=False)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=_lr_lambda)
    rec = []
    for k in range(STEPS):
        for i, p in enumerate(params):
            p.grad = grads[k][i].double()
        opt.step()
        sched.step()
        rec.append({"p": torch.cat([p.detach().reshape(-1) for p in params]),
                    "m": torch.cat([opt.state[p]["exp_avg"].reshape(-1) for p in params]),
                    "v": torch.cat([opt.state[p]["exp_avg_sq"].reshape(-1) for p in params]),
                    "step": [float(opt.state_dict()["state"][i]["step"]) for i in range(len(params))]})
    return rec


@pytest.fixture(scope="module")
def traj():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    dev = torch.device("cuda", 0)
    p0, grads = _inputs()
    return {"inputs": (p0, grads), "ours": _run_ours(p0, grads, dev), "flat": _run_flat(p0, grads, dev),
            "f64": _run_torch64(p0, grads), "dev": dev}


def test_bit_identical_to_the_flat_kernel_after_every_step(traj):
    for k, (a, b) in enumerate(zip(traj["ours"], traj["flat"])):
        for key in ("p", "m", "v", "hyper"):
            assert torch.equal(a[key], b[key]), (k, key, float((a[key] - b[key]).abs().max()))
    assert float(traj["ours"][-1]["hyper"][1]) == STEPS
    assert not torch.equal(traj["ours"][-1]["p"], traj["inputs"][0].to(traj["dev"]))


@pytest.mark.parametrize("lead", [0, 1, 3])
def test_table_longer_than_one_launch(lead):
    """2 * capacity + 3 tensors of 8 elements: three launches behind ONE hyper update; lead = elements in front of the first
    parameter (0: every address 16-byte aligned, else none)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import _lib, ops
    dev = torch.device("cuda", 0)
    n = 2 * _lib.ADAM_MAX_SEGS + 3
    gen = torch.Generator().manual_seed(7 + lead)
    P0 = torch.randn(8 * n, generator=gen).to(dev)
    buf = torch.zeros(8 * n + 8, device=dev)
    buf[lead:lead + 8 * n] = P0
    mbuf, vbuf = torch.zeros_like(buf), torch.zeros_like(buf)
    params = [buf[lead + 8 * i:lead + 8 * i + 8] for i in range(n)]
    offs = [lead + 8 * i for i in range(n)]
    hyper = torch.tensor([1e-3, 0.0, 0.0, 0.0], device=dev)
    P, m, v = P0.clone(), torch.zeros_like(P0), torch.zeros_like(P0)
    hyper_ref = hyper.clone()
    for k in range(3):
        G = torch.randn(8 * n, generator=gen).to(dev)
        grads = [G[8 * i:8 * i + 8].clone() for i in range(n)]
        ops.adam_multi(params, grads, mbuf, vbuf, offs, hyper, weight_decay=WD)
        ops.adam_step(P, G, m, v, hyper_ref, weight_decay=WD)
        assert torch.equal(buf[lead:lead + 8 * n], P) and torch.equal(mbuf[lead:lead + 8 * n], m)
        assert torch.equal(vbuf[lead:lead + 8 * n], v) and torch.equal(hyper, hyper_ref)
    assert float(hyper[1]) == 3.0
    # nothing outside the segments is touched
    assert not buf[:lead].any() and not buf[lead + 8 * n:].any() and not mbuf[lead + 8 * n:].any() and not vbuf[:lead].any()


def test_semantics_against_torch_adam_in_float64(traj):
    ours, flat, f64 = traj["ours"], traj["flat"], traj["f64"]
    for k in range(STEPS):
        assert ours[k]["step"] == f64[k]["step"] == [float(k + 1)] * len(SHAPES)
        for key in ("p", "m", "v"):
            ref = f64[k][key]
            d_ours = float((ours[k][key].double().cpu() - ref).abs().max())
            d_flat = float((flat[k][key].double().cpu() - ref).abs().max())
            print(f"step {k + 1} {key}: |ours - f64| = {d_ours:.3e}  |flat kernel - f64| = {d_flat:.3e}")
            assert d_ours <= 2.0 * d_flat, (k, key, d_ours, d_flat)
    # the bound is not vacuous: fp32 results do differ from float64, by rounding only
    assert 0.0 < float((flat[-1]["p"].double().cpu() - f64[-1]["p"]).abs().max()) < 1e-5


def test_two_runs_are_bit_identical(traj):
    p0, grads = traj["inputs"]
    again = _run_ours(p0, grads, traj["dev"])
    for a, b in zip(traj["ours"], again):
        for key in ("p", "m", "v", "hyper"):
            assert torch.equal(a[key], b[key]), key


def _args(dims, model="wengnet_mosei_mult_views_text_missing"):
    return types.SimpleNamespace(input_dims=dims, model=model)


def test_reference_training_loop_with_the_dropin_optimizer(golden):
    """main :119-150 verbatim with our model / losses / sdumc_amd.optim.Adam against the golden step recorded from the real
    reference: tests/test_dropin_module.py::test_reference_training_loop_with_dropin_modules with the optimizer line swapped."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle import sdumc_oracle as O
    from sdumc_amd import optim
    from sdumc_amd.model import get_models
    from sdumc_amd.loss import MSELoss, RMSELoss, RnCLoss
    from tests.golden.make_goldens import digest
    g = golden("step")
    dims = tuple(int(v) for v in g["dims"])
    model = get_models(_args(dims))
    model.load_state_dict({"model." + k: v for k, v in O.init_params(dims, seed=int(g["pseed"])).items()})
    model = model.cuda()
    model.model.seed = int(g["seed"])
    model.model._calls = 2 * int(g["step"])
    losses = {'reg_loss': MSELoss().cuda(), 'rmse_loss': RMSELoss().cuda(), 'rnc_loss': RnCLoss().cuda()}
    optimizer = optim.Adam(model.parameters(), lr=1e-4, weight_decay=1e-5)
    w = [float(v) for v in g["weights"]]
    T = lambda k: torch.from_numpy(g[k]).cuda()
    audio_feat, text_feat, visual_feat, feat4_feat, vals = T("audio"), T("text"), T("video"), T("feat4"), T("vals")
    before = {k: v.detach().clone() for k, v in model.model.named_parameters()}
    model.train()
    optimizer.zero_grad()
    vals_out_0, embeddings_0 = model([audio_feat, text_feat, visual_feat, False])
    features_0, rnc_feat_0, text_feat_0, text_query_feat_0 = embeddings_0
    vals_out_1, embeddings_1 = model([audio_feat, feat4_feat, visual_feat, True])
    features_1, rnc_feat_1, text_feat_1, text_query_feat_1 = embeddings_1
    n_views_feature = torch.stack((rnc_feat_0, rnc_feat_1), dim=1)
    MSEloss_0 = losses['reg_loss'](vals_out_0, vals)
    MSEloss_1 = losses['reg_loss'](vals_out_1, vals)
    rnc_loss = losses['rnc_loss'](n_views_feature, vals.unsqueeze(1))
    terms = [MSEloss_0, MSEloss_1, losses['rmse_loss'](text_feat_1, text_feat_0.detach()),
             losses['rmse_loss'](text_query_feat_1, text_query_feat_0.detach()),
             losses['rmse_loss'](features_1, features_0), rnc_loss]
    loss = sum(wi * t for wi, t in zip(w, terms))
    loss.backward()
    optimizer.step()
    np.testing.assert_allclose(float(loss), float(g["loss"]), rtol=2e-5)
    dead = {str(n) for n in g["dead"]}
    names = [str(n) for n in g["names"]]
    checked = 0
    for i, k in enumerate(names):
        p = model.model._get(k)
        if k in dead:
            assert p.grad is None and torch.equal(p.detach(), before[k]) and p not in optimizer.state, k
            continue
        assert set(optimizer.state[p]) == {"step", "exp_avg", "exp_avg_sq"} and float(optimizer.state[p]["step"]) == 1.0, k
        scale = max(1e-6, abs(g["grad_digest"][i][1]))
        np.testing.assert_allclose(digest(p.grad.cpu(), k), g["grad_digest"][i], rtol=5e-4, atol=5e-5 * scale + 1e-6, err_msg=k)
        if "delta__" + k in g.files:
            ok = np.abs(g["grad__" + k].reshape(p.shape)) > 1e-5
            np.testing.assert_allclose(((p.detach() - before[k]) * 1e4).cpu().numpy()[ok], g["delta__" + k].reshape(p.shape)[ok],
                                       rtol=5e-3, atol=5e-3, err_msg=k)
            checked += 1
    assert checked and dead
    sd = optimizer.state_dict()
    assert sorted(sd["state"]) == [i for i, k in enumerate(names) if k not in dead]


DIMS, B, T = (64, 32, 48, 32), 4, (21, 5, 13, 4)


def _model(seed=5):
    from sdumc_amd.model import get_models
    torch.manual_seed(seed)
    return get_models(_args(DIMS)).cuda()


def _model_grads(net, steps, seed=11):
    """Synthetic gradients for the live parameters (the dead ones keep grad None), on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    return [{n: torch.randn(net._get(n).shape, generator=gen) * 1e-2 for n in net._live_names} for _ in range(steps)]


def _set_grads(net, gs, in_place=False):
    for n, g in gs.items():
        p = net._get(n)
        if in_place and p.grad is not None:
            p.grad.copy_(g)
        else:
            p.grad = g.to(p.device)


def test_state_interchange_with_the_fused_step_and_torch():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import checkpoint as ck, engine, ops
    from sdumc_amd.optim import Adam
    model = _model()
    net = model.model
    lay = net._layout
    gs = _model_grads(net, 4)
    opt = Adam(model.parameters(), lr=1e-4, weight_decay=WD)
    for k in range(3):
        _set_grads(net, gs[k])
        opt.step()
    sd = opt.state_dict()
    # ours -> flat moments -> the fused step's state and back
    m, v, step = ck.flat_from_adam_state(net, sd, net._flat.device)
    ts = engine.TrainStep(net._flat.clone(), B, T, DIMS, seed=3)
    ts.load_optimizer_state(m, v, step)
    m2, v2, step2 = ts.optimizer_state()
    assert step == 3 and step2 == 3
    for name in net._live_names:
        off, shape, _ = lay.entries[name]
        st = opt.state[net._get(name)]
        n = _numel(shape)
        assert torch.equal(m2[off:off + n], st["exp_avg"].reshape(-1)) and torch.equal(v2[off:off + n], st["exp_avg_sq"].reshape(-1)), name
    # torch accepts our state_dict (and counts per parameter: no `step` tensor is shared)
    ref = torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=WD)
    ref.load_state_dict(sd)
    assert len({ref.state[p]["step"].data_ptr() for p in ref.state}) == len(ref.state)
    # reverse: the fused step's state -> load_state_dict on a fresh optimizer -> one more step == the flat kernel, bit for bit
    P = net._flat[:lay.live].clone()
    G = torch.zeros(lay.live, device=P.device)
    for name, g in gs[3].items():
        off, shape, _ = lay.entries[name]
        G[off:off + _numel(shape)] = g.reshape(-1).to(P.device)
    mo, vo = m2.clone(), v2.clone()
    hyper = torch.tensor([1e-4, float(step2), 0.0, 0.0], device=P.device)
    ops.adam_step(P, G, mo, vo, hyper, weight_decay=WD)
    opt2 = Adam(model.parameters(), lr=1e-3, weight_decay=0.0)
    opt2.load_state_dict(ck.adam_state_from_flat(net, m2, v2, step2, lr=1e-4, weight_decay=WD))
    _set_grads(net, gs[3])
    opt2.step()
    for name in net._live_names:
        off, shape, _ = lay.entries[name]
        n = _numel(shape)
        p = net._get(name)
        assert torch.equal(p.detach().reshape(-1), P[off:off + n]), name
        assert torch.equal(opt2.state[p]["exp_avg"].reshape(-1), mo[off:off + n]), name
        assert torch.equal(opt2.state[p]["exp_avg_sq"].reshape(-1), vo[off:off + n]), name
    assert float(opt2.state_dict()["state"][0]["step"]) == 4.0
    # ... and a load_state_dict AFTER steps installs the state in place
    opt2.load_state_dict(sd)
    name = net._live_names[0]
    assert torch.equal(opt2.state[net._get(name)]["exp_avg"], opt.state[net._get(name)]["exp_avg"])
    assert float(opt2.state[net._get(name)]["step"]) == 3.0 and float(opt2._hyper[1]) == 3.0


def test_moving_pointers_and_grad_set_changes():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd.optim import Adam
    from sdumc_amd._lib import SdumcError
    a, b = _model(), _model()
    b.load_state_dict(a.state_dict())
    gs = _model_grads(a.model, 4)
    oa = Adam(a.parameters(), lr=1e-3, weight_decay=WD)
    ob = Adam(b.parameters(), lr=1e-3, weight_decay=WD)
    for k in range(4):
        _set_grads(a.model, gs[k], in_place=True)            # the same gradient tensors every step: the cached table
        oa.step()
        if k == 0:
            key = oa._key
        ob.zero_grad(set_to_none=True)                        # gradient pointers move
        if k == 2:
            old = b.model._flat.data_ptr()
            b = b.cuda()                                      # _apply -> _reflatten: parameter pointers move
            assert b.model._flat.data_ptr() != old
        _set_grads(b.model, gs[k])
        ob.step()
    assert oa._key == key
    for name in a.model._pnames:
        pa, pb = a.model._get(name), b.model._get(name)
        assert torch.equal(pa.detach(), pb.detach()), name
        if name in a.model._live_names:
            for s in ("exp_avg", "exp_avg_sq", "step"):
                assert torch.equal(oa.state[pa][s], ob.state[pb][s]), (name, s)
        else:
            assert pa not in oa.state
    # a grad-set change after the first step: refused, nothing applied
    net = a.model
    flat0, m0, v0, h0 = net._flat.clone(), oa._m.clone(), oa._v.clone(), oa._hyper.clone()
    victim = net._get(net._live_names[3])
    saved = victim.grad
    victim.grad = None
    with pytest.raises(SdumcError, match="parameter"):
        oa.step()
    victim.grad = saved
    dead = next(n for n in net._pnames if n not in net._live_names)
    net._get(dead).grad = torch.ones_like(net._get(dead))
    with pytest.raises(SdumcError, match="parameter"):
        oa.step()
    net._get(dead).grad = None
    assert torch.equal(net._flat, flat0) and torch.equal(oa._m, m0) and torch.equal(oa._v, v0) and torch.equal(oa._hyper, h0)
    assert float(oa.state[victim]["step"]) == 4.0
    oa.step()                                                 # the original set again: accepted
    assert float(oa.state[victim]["step"]) == 5.0 and float(oa._hyper[1]) == 5.0
