"""Decoupled weight decay at the kernel level: sdumc_adamw_step (the decoupled forms of adam_kernel and adam_rates_kernel, with and
without the averaged weights), sdumc_adamw_multi (adam_multi_kernel<true>) and sdumc_amd.optim.AdamW, against the kernels that were there
before -- bit for bit -- and against torch.optim.AdamW in float64.

The buffer is the one of tests/test_gpu_adam_rates.py, restated: ONE flat buffer of N (about 40 k) floats, segments of 1, 3, 7, 64, 255,
256, 1024, 4097 and 8197 elements with gaps of 0-3 floats between them so that starts and ends hit every residue mod 4, several segments
longer than a workgroup's 1024 elements, N % 4 == 3 with the last segment reaching into the scalar tail; magnitudes 2^-12 .. 2^12, the
second moment non-negative; three steps with a fresh gradient and a DIFFERENT hyper[0] each (the decay factor follows the learning rate
the launch reads).

The rule, as two operations of the code that was there before: p.mul_(dk) by torch with dk = fp32(1 - fp32(lr) * fp32(wd)) computed by
the test in double, then ops.adam_step(..., weight_decay=0).  Everything up to the torch comparison is bit equality."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import adamw_ref  # noqa: E402
import ema_ref  # noqa: E402

pytestmark = pytest.mark.gpu

LRS, WD, STEPS = (1e-3, 3.7e-4, 2.5e-3), 1e-2, 3
SIZES = (1, 3, 7, 64, 255, 256, 1024, 4097, 8197, 7, 1, 8197, 3, 1024, 255, 4097, 64, 256, 8197, 4097)
GAPS = (1, 0, 2, 3, 0, 1, 1, 2, 3, 0, 0, 3, 2, 1, 0, 2, 1, 3, 0, 2)


def _layout():
    segs, cur = [], 0
    for n, gap in zip(SIZES, GAPS):
        cur += gap
        segs.append((cur, n))
        cur += n
    while cur % 4 != 2:      # the last segment ends two floats into the scalar tail; one more float of padding behind it
        segs[-1] = (segs[-1][0], segs[-1][1] + 1)
        cur += 1
    return segs, cur + 1


SEGS, N = _layout()
assert 39000 < N < 42000 and N % 4 == 3
assert {off % 4 for off, _ in SEGS} == {0, 1, 2, 3} and {(off + n) % 4 for off, n in SEGS} == {0, 1, 2, 3}
assert all(a + n <= b for (a, n), (b, _) in zip(SEGS, SEGS[1:])) and SEGS[0][0] > 0 and SEGS[-1][0] + SEGS[-1][1] == N - 1
assert sum(1 for off, n in SEGS if off // 1024 != (off + n - 1) // 1024 and n > 1024) >= 2      # beyond one workgroup's span
assert (N // 4) * 4 < SEGS[-1][0] + SEGS[-1][1] < N                                            # into the scalar tail
assert len({float(np.float32(lr)) for lr in LRS}) == STEPS


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same(a, b, what):
    """bit equality; a failure names how many elements differ and the first of them"""
    bad = torch.nonzero(_bits(a) != _bits(b)).flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} of {a.numel()} elements differ, the first at {bad[:8].tolist()}"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import ops
    return ops


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(78)

    def values(sign=True):
        v = torch.exp2(torch.rand(N, generator=g) * 24 - 12)
        return (v * (torch.randint(0, 2, (N,), generator=g) * 2 - 1) if sign else v).cuda()
    return {"p": values(), "m": values(), "v": values(False), "g": [values() for _ in range(STEPS)], "a": values()}


def _hyper(lr, t=0.0):
    return torch.tensor([lr, t, 0.0, 0.0], device="cuda")


def _rule(ops, p, g, m, v, hyper, lr, wd):
    """ONE step of the rule by the code that was there before, in place: hyper[0] <- lr, p.mul_(dk), adam_step without L2"""
    hyper[0] = lr
    dk = np.float32(1 - float(np.float32(lr)) * float(np.float32(wd)))
    assert dk == adamw_ref.decay_factor(lr, wd)
    p.mul_(torch.tensor(dk, dtype=torch.float32, device=p.device))
    ops.adam_step(p, g, m, v, hyper, weight_decay=0.0)


def _steps(data, step, wd=WD, lrs=LRS):
    """STEPS steps from the data's start state: step(p, g, m, v, hyper) after hyper[0] <- that step's lr -> (p, m, v, hyper)"""
    p, m, v, hyper = data["p"].clone(), data["m"].clone(), data["v"].clone(), _hyper(lrs[0])
    for lr, g in zip(lrs, data["g"]):
        hyper[0] = lr
        step(p, g, m, v, hyper)
    return p, m, v, hyper


@pytest.fixture(scope="module")
def whole(ops, data):
    """the rule over the whole buffer: what case 1 is held to, and elements of no segment everywhere"""
    p, m, v, hyper = data["p"].clone(), data["m"].clone(), data["v"].clone(), _hyper(LRS[0])
    for lr, g in zip(LRS, data["g"]):
        _rule(ops, p, g, m, v, hyper, lr, WD)
    return p, m, v, hyper


@pytest.fixture(scope="module")
def plain(ops, data):
    return _steps(data, lambda p, g, m, v, h: ops.adamw_step(p, g, m, v, h, weight_decay=WD))


def test_no_table_is_the_decay_multiply_then_the_step_without_l2(ops, data, whole, plain):
    """1. p, m, v, hyper equal p.mul_(dk) followed by ops.adam_step(weight_decay=0), gaps and scalar tail included"""
    for name, a, b in zip(("p", "m", "v", "hyper"), plain, whole):
        _assert_same(a, b, name)
    assert float(plain[3][1]) == STEPS and float(plain[3][0]) == float(np.float32(LRS[-1]))
    # ... and the decay is no part of that step: the coupled kernel with the same weight_decay gives other parameters
    coupled = _steps(data, lambda p, g, m, v, h: ops.adam_step(p, g, m, v, h, weight_decay=WD))
    assert not torch.equal(coupled[0], plain[0])
    # grad_scale multiplies the gradient only: 0.5 is exact, so the step equals the one on halved gradients
    half = dict(data, g=[g * 0.5 for g in data["g"]])
    a = _steps(data, lambda p, g, m, v, h: ops.adamw_step(p, g, m, v, h, weight_decay=WD, grad_scale=0.5))
    b = _steps(half, lambda p, g, m, v, h: ops.adamw_step(p, g, m, v, h, weight_decay=WD))
    for name, x, y in zip("pmv", a, b):
        _assert_same(x, y, name + " with grad_scale 0.5")


def test_no_decay_is_the_step_that_was_there(ops, data):
    """2. weight_decay=0: equal to ops.adam_step(weight_decay=0), with and without a table of ones"""
    want = _steps(data, lambda p, g, m, v, h: ops.adam_step(p, g, m, v, h, weight_decay=0.0))
    ones = [(off, n, 1.0, 1.0, False) for off, n in SEGS]
    for segments in (None, ones):
        got = _steps(data, lambda p, g, m, v, h: ops.adamw_step(p, g, m, v, h, weight_decay=0.0, segments=segments))
        for name, a, b in zip(("p", "m", "v", "hyper"), got, want):
            _assert_same(a, b, f"{name} (table: {segments is not None})")


def test_a_table_of_ones_is_no_table(ops, data, plain):
    """3. all scales 1, nothing frozen; and a table that names one element in the middle"""
    for table in ([(off, n, 1.0, 1.0, False) for off, n in SEGS], [(SEGS[7][0] + 5, 1, 1.0, 1.0, False)]):
        got = _steps(data, lambda p, g, m, v, h: ops.adamw_step(p, g, m, v, h, weight_decay=WD, segments=table))
        for name, a, b in zip(("p", "m", "v", "hyper"), got, plain):
            _assert_same(a, b, f"{name} ({len(table)} segments)")


FROZEN = {1, 2, 5, 7, 8, 11, 19}      # 3, 7, 256, 4097, 8197, 8197 (unaligned ends) and the last one (into the scalar tail)
ZERO_LR = {0, 4, 9, 15}


def _scales(shift=0):
    lrs, wds = (0.25, 0.5, 2.0), (0.0, 0.5, 1.0, 2.0)
    return [(0.0 if i in ZERO_LR else lrs[(i + shift) % 3], wds[(i + 2 * shift) % 4], i in FROZEN) for i in range(len(SEGS))]


def _alone(ops, data, off, n, ls, ws):
    """the segment copied to aligned tensors of its own and stepped through the no-table decoupled call with lr ls and wd ws"""
    p, m, v = (data[k][off:off + n].clone() for k in "pmv")
    wd = float(np.float32(WD) * np.float32(ws))
    assert wd == float(np.float32(WD)) * ws                      # (a power of two, or zero: the product is exact)
    hyper = _hyper(0.0)
    for lr, g in zip(LRS, data["g"]):
        lr_s = float(np.float32(lr) * np.float32(ls))
        assert lr_s == float(np.float32(lr)) * ls
        hyper[0] = lr_s
        ops.adamw_step(p, g[off:off + n].clone(), m, v, hyper, weight_decay=wd)
    assert all(x.data_ptr() % 16 == 0 for x in (p, m, v))
    return p, m, v


def _gap_mask():
    mask = torch.ones(N, dtype=torch.bool)
    for off, n in SEGS:
        mask[off:off + n] = False
    return mask.cuda()


@pytest.mark.parametrize("shift", [0, 1])
def test_a_table_is_every_segment_stepped_alone(ops, data, whole, shift):
    """4. power-of-two lr_scale / wd_scale, a zero lr_scale, a zero wd_scale, frozen segments -- a NaN planted in a frozen segment's
    gradient is never read: each segment equals that segment stepped alone, frozen ones keep their bits, elements of no segment equal
    case 1"""
    scales = _scales(shift)
    assert any(ws == 0.0 and not fr for _, ws, fr in scales) and any(ls == 0.0 and not fr for ls, _, fr in scales)
    table = [(off, n, ls, ws, fr) for (off, n), (ls, ws, fr) in zip(SEGS, scales)]
    planted = dict(data, g=[g.clone() for g in data["g"]])
    for i in (2, 8):
        off, n = SEGS[i]
        planted["g"][1][off + n // 2] = float("nan")
        planted["g"][0][off] = float("inf")
    got = _steps(planted, lambda p, g, m, v, h: ops.adamw_step(p, g, m, v, h, weight_decay=WD, segments=table))
    for i, (off, n, ls, ws, fr) in enumerate(table):
        want = tuple(data[k][off:off + n] for k in "pmv") if fr else _alone(ops, data, off, n, ls, ws)
        for name, a, b in zip("pmv", got, want):
            _assert_same(a[off:off + n], b, f"{name} of segment ({off}, {n}) lr_scale {ls} wd_scale {ws} frozen {fr}")
        if i in ZERO_LR and not fr:      # torch's lr = 0 group: the parameter stays, the moments advance
            assert torch.equal(_bits(got[0][off:off + n]), _bits(data["p"][off:off + n]))
            assert not torch.equal(got[1][off:off + n], data["m"][off:off + n])
    gaps = _gap_mask()
    for name, a, b in zip("pmv", got, whole):
        _assert_same(a[gaps], b[gaps], f"{name}: elements of no segment")
    assert torch.equal(got[3], whole[3])
    assert all(bool(torch.isfinite(x).all()) for x in got[:3])


@pytest.mark.parametrize("table", [False, True], ids=["no table", "table"])
@pytest.mark.parametrize("decay,warmup", [(0.75, False), (0.999, False), (0.75, True)])
def test_the_average_rides_along(ops, data, plain, table, decay, warmup):
    """5. the EMA forms: parameters, moments and hyper are those without the average; the average is the rule of tests/ema_ref.py
    applied to the post-step parameters (bits where the weight is 0.25, its bound elsewhere); a frozen segment's average stays"""
    segments = [(off, n, ls, ws, fr) for (off, n), (ls, ws, fr) in zip(SEGS, _scales())] if table else None
    without = _steps(data, lambda p, g, m, v, h: ops.adamw_step(p, g, m, v, h, weight_decay=WD, segments=segments)) if table else plain
    live = torch.ones(N, dtype=torch.bool, device="cuda")
    if table:
        for (off, n), (_, _, fr) in zip(SEGS, _scales()):
            live[off:off + n] = not fr
    a = data["a"].clone()
    assert a.data_ptr() % 16 == 0
    p, m, v, hyper = data["p"].clone(), data["m"].clone(), data["v"].clone(), _hyper(LRS[0])
    worst = 0.0
    for t, (lr, g) in enumerate(zip(LRS, data["g"])):
        hyper[0] = lr
        before = a.clone()
        ops.adamw_step(p, g, m, v, hyper, weight_decay=WD, segments=segments, ema=a, ema_decay=decay, ema_warmup=warmup)
        w = ema_ref.weight(decay, t + 1, warmup)
        worst = max(worst, ema_ref.check(a[live], before[live], p[live], w, f"step {t + 1}"))
        _assert_same(a[~live], before[~live], "the average of frozen segments")
    print(f"decay {decay} warmup {warmup} table {table}: worst |ema - rule| / bound = {worst:.4f}")
    for name, x, y in zip(("p", "m", "v", "hyper"), (p, m, v, hyper), without):
        _assert_same(x, y, name)


@pytest.mark.parametrize("lead", [0, 1, 3])
def test_multi_over_views_is_the_flat_call_on_the_concatenation(ops, lead):
    """6. 2 * capacity + 3 tensors of 8 elements: three launches behind ONE hyper update; lead = elements in front of the first
    parameter (0: every address 16-byte aligned, else none).  Nothing outside the segments is written."""
    from sdumc_amd import _lib
    n = 2 * _lib.ADAM_MAX_SEGS + 3
    gen = torch.Generator().manual_seed(17 + lead)
    P0 = torch.randn(8 * n, generator=gen).cuda()
    buf = torch.zeros(8 * n + 8, device="cuda")
    buf[lead:lead + 8 * n] = P0
    mbuf, vbuf = torch.zeros_like(buf), torch.zeros_like(buf)
    params = [buf[lead + 8 * i:lead + 8 * i + 8] for i in range(n)]
    offs = [lead + 8 * i for i in range(n)]
    hyper = _hyper(LRS[0])
    P, m, v = P0.clone(), torch.zeros_like(P0), torch.zeros_like(P0)
    hyper_ref = hyper.clone()
    for lr in LRS:
        G = torch.randn(8 * n, generator=gen).cuda()
        grads = [G[8 * i:8 * i + 8].clone() for i in range(n)]
        hyper[0] = lr
        hyper_ref[0] = lr
        ops.adamw_multi(params, grads, mbuf, vbuf, offs, hyper, weight_decay=0.1)
        ops.adamw_step(P, G, m, v, hyper_ref, weight_decay=0.1)
        _assert_same(buf[lead:lead + 8 * n], P, "p")
        _assert_same(mbuf[lead:lead + 8 * n], m, "m")
        _assert_same(vbuf[lead:lead + 8 * n], v, "v")
        assert torch.equal(hyper, hyper_ref)
    assert float(hyper[1]) == 3.0
    assert not buf[:lead].any() and not buf[lead + 8 * n:].any() and not mbuf[:lead].any() and not mbuf[lead + 8 * n:].any()
    assert not vbuf[:lead].any() and not vbuf[lead + 8 * n:].any()
    # ... and it is the rule, not the coupled step: the flat call on the concatenation is case 1's
    Q, qm, qv, qh = P0.clone(), torch.zeros_like(P0), torch.zeros_like(P0), _hyper(LRS[0])
    gen = torch.Generator().manual_seed(17 + lead)
    torch.randn(8 * n, generator=gen)
    for lr in LRS:
        _rule(ops, Q, torch.randn(8 * n, generator=gen).cuda(), qm, qv, qh, lr, 0.1)
    _assert_same(P, Q, "the flat call against the rule")


# ------------------------------------------------------------------------------------------------------------------ against torch
VIEWS = (1, 3, 1025, 4098, 255, 8197)      # the leading tensors of the drop-in's parameter set; one more takes the rest of the N


def _view_bounds():
    cuts, o = [], 0
    for n in VIEWS:
        cuts.append((o, n))
        o += n
    cuts.append((o, adamw_ref.N - o))
    return cuts


def _dropin(cls, p0, grads, lr, wd, state=None, e0=0, **kw):
    """sdumc_amd.optim `cls` over views of one flat device buffer, a step per gradient under LambdaLR -> (flat parameters, optimizer)"""
    flat = p0.cuda().clone()
    params = [torch.nn.Parameter(flat[o:o + n]) for o, n in _view_bounds()]
    assert sum(p.data_ptr() % 16 != 0 for p in params) >= 4
    opt = cls(params, lr=lr, weight_decay=wd, **kw)
    if state is not None:
        opt.load_state_dict(state)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: adamw_ref.lr_lambda(e0 + e))
    for g in grads:
        gd = g.cuda()
        for p, (o, n) in zip(params, _view_bounds()):
            p.grad = gd[o:o + n].clone()
        opt.step()
        sched.step()
    return flat, opt


def _flat_run(ops, p0, grads, lr, wd):
    p = p0.cuda().clone()
    m, v, hyper = torch.zeros_like(p), torch.zeros_like(p), _hyper(lr)
    for e, g in enumerate(grads):
        hyper[0] = lr * adamw_ref.lr_lambda(e)
        ops.adamw_step(p, g.cuda(), m, v, hyper, weight_decay=wd)
    return p, m, v, hyper


@pytest.fixture(scope="module")
def torch_inputs():
    return adamw_ref.inputs()


@pytest.mark.parametrize("lr,wd", adamw_ref.CASES)
def test_against_torch_adamw_in_float64(ops, torch_inputs, lr, wd):
    """7. max |ours - torch AdamW fp64| <= 2 e32, e32 = max |torch AdamW fp32 - torch AdamW fp64| computed here from torch alone
    (tests/adamw_ref.py has the inputs and the reasoning), through the flat call and through optim.AdamW under LambdaLR -- which is bit
    for bit the flat call.  Measured on an MI355X: see the ratios this prints; profiles/README.md records them."""
    from sdumc_amd.optim import Adam, AdamW
    p0, grads = torch_inputs
    p64, e32, coupled = adamw_ref.references(p0, grads, lr, wd)
    flat, m, v, hyper = _flat_run(ops, p0, grads, lr, wd)
    d_flat = float((flat.double().cpu() - p64).abs().max())
    got, opt = _dropin(AdamW, p0, grads, lr, wd)
    d_opt = float((got.double().cpu() - p64).abs().max())
    print(f"lr {lr:g} wd {wd:g}: e32 {e32:.3e}  |flat - f64| {d_flat:.3e} ({d_flat / e32:.3f} e32)  |optim.AdamW - f64| {d_opt:.3e} "
          f"({d_opt / e32:.3f} e32)  coupled Adam fp32 {coupled:.3e} ({coupled / e32:.0f} e32)")
    assert e32 > 0.0
    assert d_flat <= 2.0 * e32, (lr, wd, d_flat, e32)
    assert d_opt <= 2.0 * e32, (lr, wd, d_opt, e32)
    _assert_same(got, flat, "optim.AdamW against the flat call: p")
    _assert_same(torch.cat([opt.state[p]["exp_avg"].reshape(-1) for p in opt._live]), m, "m")
    _assert_same(torch.cat([opt.state[p]["exp_avg_sq"].reshape(-1) for p in opt._live]), v, "v")
    assert torch.equal(opt._hyper, hyper) and float(opt._step_t) == adamw_ref.STEPS
    # Adam(decoupled_weight_decay=True) is the same thing
    same, _ = _dropin(Adam, p0, grads, lr, wd, decoupled_weight_decay=True)
    _assert_same(same, flat, "optim.Adam(decoupled_weight_decay=True)")


def test_state_interchange_with_torch(ops, torch_inputs):
    """8. three steps of ours -> torch.optim.AdamW takes the state and the parameters for the fourth; three steps of torch's -> ours
    takes them for the fourth; the drop-in's own save / load in between: each within 2 e32 of four steps of torch AdamW fp64, e32 from
    four steps of torch AdamW fp32.  Two runs of ours are bit-identical."""
    from sdumc_amd.optim import Adam, AdamW
    lr, wd = adamw_ref.CASES[0]
    p0, grads = torch_inputs
    head, tail = grads[:3], grads[3:4]
    p64, e32, _ = adamw_ref.references(p0, grads[:4], lr, wd)
    bounds = _view_bounds()

    def split(state):      # a one-parameter torch state <-> the drop-in's views
        st = state["state"][0]
        return {"state": {i: {"step": st["step"].clone(), "exp_avg": st["exp_avg"][o:o + n].clone(),
                              "exp_avg_sq": st["exp_avg_sq"][o:o + n].clone()} for i, (o, n) in enumerate(bounds)},
                "param_groups": [dict(state["param_groups"][0], params=list(range(len(bounds))))]}

    def join(state):
        sts = [state["state"][i] for i in range(len(bounds))]
        return {"state": {0: {"step": sts[0]["step"].clone().cpu(), "exp_avg": torch.cat([s["exp_avg"].reshape(-1) for s in sts]).cpu(),
                              "exp_avg_sq": torch.cat([s["exp_avg_sq"].reshape(-1) for s in sts]).cpu()}},
                "param_groups": [dict(state["param_groups"][0], params=[0])]}

    ours3, opt3 = _dropin(AdamW, p0, head, lr, wd)
    again3, _ = _dropin(AdamW, p0, head, lr, wd)
    _assert_same(ours3, again3, "two runs of ours")
    sd = opt3.state_dict()
    assert sd["param_groups"][0]["decoupled_weight_decay"] is True
    # ours -> torch
    t4, topt = adamw_ref.torch_run(torch.optim.AdamW, torch.float32, ours3.cpu(), tail, lr, wd, state=join(sd))
    assert topt.param_groups[0]["decoupled_weight_decay"] is True
    # ours -> ours (AdamW, and the Adam class, which takes the loaded group's flag), bit for bit an uninterrupted run
    straight, _ = _dropin(AdamW, p0, grads[:4], lr, wd)
    for cls in (AdamW, Adam):
        o4, oopt = _dropin(cls, ours3.cpu(), tail, lr, 0.0 if cls is Adam else wd, state=sd, e0=3)
        assert oopt.param_groups[0]["decoupled_weight_decay"] is True and oopt.param_groups[0]["weight_decay"] == wd
        _assert_same(o4, straight, f"resumed under sdumc_amd.optim.{cls.__name__}")
    # torch -> ours
    t3, topt3 = adamw_ref.torch_run(torch.optim.AdamW, torch.float32, p0, head, lr, wd)
    b4, _ = _dropin(AdamW, t3, tail, lr, wd, state=split(topt3.state_dict()), e0=3)
    for what, got in (("ours -> torch", t4), ("ours -> ours", straight), ("torch -> ours", b4)):
        d = float((got.double().cpu() - p64).abs().max())
        print(f"{what}: |p - f64| {d:.3e} ({d / e32:.3f} e32)")
        assert d <= 2.0 * e32, (what, d, e32)


def test_refusals_write_nothing(ops):
    """9. every refusal, with live allocations: SDUMC_EINVAL, and parameters, gradients, moments, average and hyper keep their
    sentinels"""
    from sdumc_amd import _lib
    lib, n = _lib.lib, 4096
    sent = (-11.0, -22.0, -33.0, -44.0, -55.0)
    bufs = [torch.full((n,), s, device="cuda") for s in sent]
    P, G, M, V, A = (b.data_ptr() for b in bufs)
    hyper = torch.tensor([1e-3, 5.0, 0.25, 0.5], device="cuda")
    good = [(0, 7, 1.0, 1.0, False), (8, 100, 0.5, 0.0, True), (108, 3988, 2.0, 1.0, False)]
    st = _lib.current_stream()

    def step(p=P, g=G, m=M, v=V, cnt=n, hy=hyper.data_ptr(), segs=None, nseg=None, a=None, decay=0.0, warm=0):
        tb = ops.rate_segments(segs) if segs is not None else None
        return lib.sdumc_adamw_step(p, g, m, v, cnt, hy, 0.9, 0.999, 1e-8, 1e-2, 1.0, tb, (len(segs) if segs is not None else 0)
                                    if nseg is None else nseg, a, decay, warm, st)

    cases = {"param": {"p": None}, "grad": {"g": None}, "exp_avg": {"m": None}, "exp_avg_sq": {"v": None}, "hyper": {"hy": None},
             "n": {"cnt": 0}, "n < 0": {"cnt": -4}, "param alignment": {"p": P + 4}, "grad alignment": {"g": G + 8},
             "moment alignment": {"m": M + 4}, "second moment alignment": {"v": V + 12},
             "a table without a count": {"segs": good, "nseg": 0}, "a count without a table": {"nseg": 3},
             "nseg 97": {"segs": [(4 * i, 3, 1.0, 1.0, True) for i in range(97)]},
             "overlapping": {"segs": [(0, 8, 1.0, 1.0, True), (7, 8, 1.0, 1.0, True)]},
             "descending": {"segs": [(64, 8, 1.0, 1.0, True), (0, 8, 1.0, 1.0, True)]},
             "behind the end": {"segs": [(4090, 7, 1.0, 1.0, True)]}, "in front of the start": {"segs": [(-2, 7, 1.0, 1.0, True)]},
             "empty": {"segs": [(16, 0, 1.0, 1.0, True)]}, "negative lr_scale": {"segs": [(0, 8, -0.5, 1.0, True)]},
             "NaN lr_scale": {"segs": [(0, 8, float("nan"), 1.0, True)]}, "negative wd_scale": {"segs": [(0, 8, 1.0, -2.0, True)]},
             "Inf wd_scale": {"segs": [(0, 8, 1.0, float("inf"), True)]},
             "a decay without an average": {"decay": 0.5}, "a warm-up without an average": {"warm": 1},
             "ema alignment": {"a": A + 4, "decay": 0.9}, "ema is param": {"a": P, "decay": 0.9},
             "ema overlaps param": {"a": P + 16, "decay": 0.9}, "decay < 0": {"a": A, "decay": -0.5},
             "decay > 1": {"a": A, "decay": 1.5}, "decay NaN": {"a": A, "decay": float("nan")}}
    for what, kw in cases.items():
        assert step(**kw) == -1, what
        if "segs" not in kw and "nseg" not in kw:
            assert step(segs=good, **kw) == -1, what + " (with a table)"
    seg = ops.adam_segments([bufs[0][:8]], [bufs[1][:8]], [0])
    multi = lib.sdumc_adamw_multi
    hy = hyper.data_ptr()
    assert multi(None, 1, M, V, n, hy, 0.9, 0.999, 1e-8, 1e-2, 1.0, st) == -1
    assert multi(seg, 0, M, V, n, hy, 0.9, 0.999, 1e-8, 1e-2, 1.0, st) == -1
    assert multi(seg, 1, None, V, n, hy, 0.9, 0.999, 1e-8, 1e-2, 1.0, st) == -1
    assert multi(seg, 1, M, None, n, hy, 0.9, 0.999, 1e-8, 1e-2, 1.0, st) == -1
    assert multi(seg, 1, M, V, n, None, 0.9, 0.999, 1e-8, 1e-2, 1.0, st) == -1
    assert multi(seg, 1, M, V, 0, hy, 0.9, 0.999, 1e-8, 1e-2, 1.0, st) == -1
    assert multi(seg, 1, M, V, 7, hy, 0.9, 0.999, 1e-8, 1e-2, 1.0, st) == -1          # state_offset + n > state_len
    for field, value in (("param", None), ("grad", None), ("n", 0), ("state_offset", -4), ("state_offset", n - 4)):
        seg = ops.adam_segments([bufs[0][:8]], [bufs[1][:8]], [0])
        setattr(seg[0], field, value)
        assert multi(seg, 1, M, V, n, hy, 0.9, 0.999, 1e-8, 1e-2, 1.0, st) == -1, (field, value)
    torch.cuda.synchronize()
    for b, s in zip(bufs, sent):
        assert bool((b == s).all()), s
    assert hyper.tolist() == [np.float32(1e-3), 5.0, 0.25, 0.5]
    with pytest.raises(_lib.SdumcError):      # the wrappers raise
        ops.adamw_step(*bufs[:4], hyper, segments=[(0, 8, -1.0, 1.0, False)])
    with pytest.raises(_lib.SdumcError):
        ops.adamw_step(*bufs[:4], hyper, ema_decay=0.5)
    with pytest.raises(_lib.SdumcError):
        ops.adamw_multi([bufs[0][:8]], [bufs[1][:8]], bufs[2], bufs[3][:100], [0], hyper)
