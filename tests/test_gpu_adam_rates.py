"""Per-tensor learning rates, decay and frozen tensors at the kernel level: sdumc_adam_step_rates (adam_rates_kernel) and
sdumc_zero_segments (zero_segments_kernel) of csrc/adam.hip against sdumc_adam_step, the parent's own launch.

ONE flat buffer of N (about 40 k) floats: segments of 1, 3, 7, 64, 255, 256, 1024, 4097 and 8197 elements (each twice or more), gaps of 0-3
floats between them so that segment starts hit every residue mod 4, several segments longer than a workgroup's span of 1024 elements, a
bucket length that is no multiple of 4 with the last segment reaching into the scalar tail.  Parameters, gradients and moments have
magnitudes 2^-12 .. 2^12, the second moment non-negative; three consecutive steps with a fresh gradient each.

References, all the parent's kernels: the WHOLE buffer through sdumc_adam_step (what elements of no segment get, and what a table of
ones gives everywhere), and every segment ALONE, copied to an aligned tensor of its own with its own hyper at the same step count,
through sdumc_adam_step with that segment's learning rate and decay.  Bit equality (torch.equal) wherever the arithmetic is the same
by construction; the one derived bar is stated where it is used."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, WD, STEPS = 1e-3, 1e-2, 3
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


# the layout is what the docstring says
assert 39000 < N < 42000 and N % 4 == 3
assert {off % 4 for off, _ in SEGS} == {0, 1, 2, 3} and {(off + n) % 4 for off, n in SEGS} == {0, 1, 2, 3}
assert all(a + n <= b for (a, n), (b, _) in zip(SEGS, SEGS[1:])) and SEGS[0][0] > 0 and SEGS[-1][0] + SEGS[-1][1] == N - 1
assert sum(1 for off, n in SEGS if off // 1024 != (off + n - 1) // 1024 and n > 1024) >= 2      # beyond one workgroup's span
assert (N // 4) * 4 < SEGS[-1][0] + SEGS[-1][1] < N                                            # into the scalar tail


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
    g = torch.Generator().manual_seed(77)

    def values(sign=True):
        v = torch.exp2(torch.rand(N, generator=g) * 24 - 12)
        return (v * (torch.randint(0, 2, (N,), generator=g) * 2 - 1) if sign else v).cuda()
    return {"p": values(), "m": values(), "v": values(False), "g": [values() for _ in range(STEPS)]}


def _hyper(lr, t=0.0):
    return torch.tensor([lr, t, 0.0, 0.0], device="cuda")


@pytest.fixture(scope="module")
def whole(ops, data):
    """STEPS steps of sdumc_adam_step over the whole buffer: (p, m, v, hyper)"""
    p, m, v, hyper = data["p"].clone(), data["m"].clone(), data["v"].clone(), _hyper(LR)
    for g in data["g"]:
        ops.adam_step(p, g, m, v, hyper, weight_decay=WD)
    return p, m, v, hyper


def _alone(ops, state, grads, off, n, lr, wd, t0=0.0):
    """the segment copied out of `state` = (p, m, v) and stepped alone by sdumc_adam_step, once per gradient: -> (p, m, v)"""
    p, m, v = (x[off:off + n].clone() for x in state)
    hyper = _hyper(lr, t0)
    for g in grads:
        ops.adam_step(p, g[off:off + n].clone(), m, v, hyper, weight_decay=wd)
    assert all(x.data_ptr() % 16 == 0 for x in (p, m, v))
    return p, m, v


def _run(ops, data, table):
    p, m, v, hyper = data["p"].clone(), data["m"].clone(), data["v"].clone(), _hyper(LR)
    for g in data["g"]:
        ops.adam_step_rates(p, g, m, v, hyper, table, weight_decay=WD)
    return p, m, v, hyper


def _gap_mask():
    mask = torch.ones(N, dtype=torch.bool)
    for off, n in SEGS:
        mask[off:off + n] = False
    return mask.cuda()


def _check_exact(ops, data, whole, scales):
    """scales: (lr_scale, wd_scale, frozen) per segment.  Every segment equal to its own run alone (frozen: to its initial bits),
    every element of no segment equal to the whole-buffer run, hyper equal."""
    table = [(off, n, ls, ws, fr) for (off, n), (ls, ws, fr) in zip(SEGS, scales)]
    got = _run(ops, data, table)
    start = (data["p"], data["m"], data["v"])
    for (off, n, ls, ws, fr) in table:
        if fr:
            want = tuple(x[off:off + n] for x in start)
        else:
            lr = float(np.float32(LR) * np.float32(ls))
            assert lr == float(np.float32(LR)) * ls      # (a power of two, or zero: the product is exact)
            want = _alone(ops, start, data["g"], off, n, lr, float(np.float32(WD) * np.float32(ws)))
        for name, a, b in zip("pmv", got, want):
            _assert_same(a[off:off + n], b, f"{name} of segment ({off}, {n}) lr_scale {ls} wd_scale {ws} frozen {fr}")
    gaps = _gap_mask()
    for name, a, b in zip("pmv", got, whole):
        _assert_same(a[gaps], b[gaps], f"{name}: elements of no segment")
    assert torch.equal(got[3], whole[3])
    return got


def test_a_table_of_ones_is_the_plain_step(ops, data, whole):
    """1. all scales 1, nothing frozen: p, m, v and hyper equal sdumc_adam_step's on a copy, gaps and scalar tail included"""
    got = _run(ops, data, [(off, n, 1.0, 1.0, False) for off, n in SEGS])
    for name, a, b in zip(("p", "m", "v", "hyper"), got, whole):
        _assert_same(a, b, name)
    assert float(got[3][1]) == STEPS
    # ... and so does a table that names only a part of the bucket (one segment in the middle, one element long)
    got = _run(ops, data, [(SEGS[7][0] + 5, 1, 1.0, 1.0, False)])
    for name, a, b in zip(("p", "m", "v", "hyper"), got, whole):
        _assert_same(a, b, name)


def test_power_of_two_rates_and_any_decay_are_the_segment_stepped_alone(ops, data, whole):
    """2. lr_scale in {0.25, 0.5, 2}, wd_scale in {0, 0.5, 1, 0.3}: every segment's p, m, v equal sdumc_adam_step on an aligned copy of
    that segment alone with lr fp32(lr 2^k) and weight decay fp32(wd) * fp32(s).  Exact by construction: a power of two commutes with
    every rounding involved, and the decay product is the same fp32 multiply on both sides."""
    lrs, wds = (0.25, 0.5, 2.0), (0.0, 0.5, 1.0, 0.3)
    _check_exact(ops, data, whole, [(lrs[i % 3], wds[i % 4], False) for i in range(len(SEGS))])
    _check_exact(ops, data, whole, [(lrs[(i + 1) % 3], wds[(i + 2) % 4], False) for i in range(len(SEGS))])


def test_arbitrary_rates_stay_within_the_derived_bar(ops, data):
    """3. lr_scale 0.3 and 1.7, step by step: the reference is the segment stepped alone FROM THE STATE THE RATES RUN HAD before that
    step (p feeds the next step's moments through the L2 term, so states are compared one step at a time), with lr fp32(fp32(lr) * fp32(s)).
    m and v do not see the learning rate: torch.equal.  p: |p - p_ref| <= ulp(p_ref) + 2^-21 |dp_ref|, dp_ref = p_ref - p_before.
    Derivation: our step size is fl(fl(lr / bc1) * s), the reference's fl(fl(lr * s) / bc1) (the quotient is evaluated in double and
    rounded once): four fp32 roundings apart, relative 4 * 2^-24 = 2^-22.  p = fl(p - step_size * q) is one fused multiply-add on either
    side, so the two differ by that relative part of the exact update plus at most one rounding of the result each: half an ulp
    each, one ulp(p_ref) together (two where a binade boundary lies between them -- the factor two on the first term, which also
    covers |dp_ref| being the ROUNDED update, pays for it wherever the update exceeds an ulp; where it does not, both sides round the
    same sub-ulp change and differ by at most one ulp).  The worst ratio is printed; on these inputs it is 0.9998: the bar has no slack
    to spare, as a derived bar should."""
    scales = [0.3 if i % 2 else 1.7 for i in range(len(SEGS))]
    table = [(off, n, s, 1.0, False) for (off, n), s in zip(SEGS, scales)]
    p, m, v, hyper = data["p"].clone(), data["m"].clone(), data["v"].clone(), _hyper(LR)
    worst = 0.0
    for t, g in enumerate(data["g"]):
        before = (p.clone(), m.clone(), v.clone())
        ops.adam_step_rates(p, g, m, v, hyper, table, weight_decay=WD)
        for (off, n), s in zip(SEGS, scales):
            lr = float(np.float32(LR) * np.float32(s))
            rp, rm, rv = _alone(ops, before, [g], off, n, lr, float(np.float32(WD)), t0=float(t))
            assert torch.equal(_bits(m[off:off + n]), _bits(rm)) and torch.equal(_bits(v[off:off + n]), _bits(rv)), (t, off, n)
            ulp = (torch.nextafter(rp.abs(), torch.full_like(rp, float("inf"))) - rp.abs()).double()
            bar = ulp + 2.0 ** -21 * (rp.double() - before[0][off:off + n].double()).abs()
            ratio = float(((p[off:off + n].double() - rp.double()).abs() / bar).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (t, off, n, s, ratio)
    print(f"arbitrary lr_scale: worst |p - p_ref| / (ulp(p_ref) + 2^-21 |dp_ref|) = {worst:.4f}")
    assert worst > 0.0      # (0.3 and 1.7 are no powers of two: somewhere the two step sizes do differ)


def test_frozen_segments_and_a_zero_rate(ops, data, whole):
    """4. frozen segments keep p, m, v bit for bit through three steps -- a NaN planted in a frozen segment's gradient is never read --
    while their neighbours are the segment stepped alone; lr_scale 0 keeps p and advances m and v like the reference's lr = 0"""
    frozen = {1, 2, 5, 7, 8, 11, 19}      # 3, 7, 256, 4097, 8197, 8197 (unaligned ends) and the last one (into the scalar tail)
    zero_lr = {0, 4, 9, 15}
    planted = dict(data, g=[g.clone() for g in data["g"]])
    for i in (2, 8):
        off, n = SEGS[i]
        planted["g"][1][off + n // 2] = float("nan")
        planted["g"][0][off] = float("inf")
    scales = [(0.0 if i in zero_lr else 0.5, 1.0 if i % 2 else 0.0, i in frozen) for i in range(len(SEGS))]
    got = _check_exact(ops, planted, whole, scales)
    for i in zero_lr:
        off, n = SEGS[i]
        assert torch.equal(_bits(got[0][off:off + n]), _bits(data["p"][off:off + n]))
        assert not torch.equal(got[1][off:off + n], data["m"][off:off + n])      # the moments did advance
    assert bool(torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all())


def test_zero_segments_writes_the_frozen_segments_and_nothing_else(ops):
    """sdumc_zero_segments: +0.0 over exactly the frozen segments; unfrozen neighbours and the gaps keep a sentinel"""
    for frozen in ({1, 2, 5, 7, 8, 11, 19}, set(range(len(SEGS))), {0}, {8, 9, 10}):
        buf = torch.full((N,), -77.0, device="cuda")
        ops.zero_segments(buf, [(off, n, 1.0, 1.0, i in frozen) for i, (off, n) in enumerate(SEGS)])
        want = torch.full((N,), -77.0)
        for i in frozen:
            want[SEGS[i][0]:SEGS[i][0] + SEGS[i][1]] = 0.0
        assert torch.equal(_bits(buf), _bits(want.cuda())), sorted(frozen)      # (bits: +0.0, not -0.0)
    buf = torch.full((N,), -77.0, device="cuda")
    ops.zero_segments(buf, [(off, n, 1.0, 1.0, False) for off, n in SEGS])      # nothing frozen: nothing to do
    assert bool((buf == -77.0).all())


def test_refusals_write_nothing(ops):
    """5. a refused table comes back as SDUMC_EINVAL and neither entry writes anything: parameters, gradients, moments and hyper keep
    their sentinels"""
    from sdumc_amd import _lib
    lib, n = _lib.lib, 4096
    many = [(4 * i, 3, 1.0, 1.0, True) for i in range(97)]
    tables = {"nseg 0": ([(0, 8, 1.0, 1.0, True)], 0), "nseg 97": (many, 97),
              "overlapping": ([(0, 8, 1.0, 1.0, True), (7, 8, 1.0, 1.0, True)], 2),
              "descending": ([(64, 8, 1.0, 1.0, True), (0, 8, 1.0, 1.0, True)], 2),
              "behind the end": ([(4090, 7, 1.0, 1.0, True)], 1), "in front of the start": ([(-2, 7, 1.0, 1.0, True)], 1),
              "empty": ([(16, 0, 1.0, 1.0, True)], 1),
              "negative lr_scale": ([(0, 8, -0.5, 1.0, True)], 1), "NaN lr_scale": ([(0, 8, float("nan"), 1.0, True)], 1),
              "negative wd_scale": ([(0, 8, 1.0, -2.0, True)], 1), "NaN wd_scale": ([(0, 8, 1.0, float("nan"), True)], 1),
              "Inf wd_scale": ([(0, 8, 1.0, float("inf"), True)], 1)}
    bufs = [torch.full((n,), s, device="cuda") for s in (-11.0, -22.0, -33.0, -44.0)]
    hyper = torch.tensor([1e-3, 5.0, 0.25, 0.5], device="cuda")
    for what, (segs, nseg) in tables.items():
        tb = ops.rate_segments(segs)
        rc = lib.sdumc_adam_step_rates(*[b.data_ptr() for b in bufs], n, hyper.data_ptr(), 0.9, 0.999, 1e-8, 1e-5, 1.0, tb, nseg,
                                       _lib.current_stream())
        assert rc == -1, what
        assert lib.sdumc_zero_segments(bufs[1].data_ptr(), n, tb, nseg, _lib.current_stream()) == -1, what
        torch.cuda.synchronize()
        for b, s in zip(bufs, (-11.0, -22.0, -33.0, -44.0)):
            assert bool((b == s).all()), what
        assert hyper.tolist() == [np.float32(1e-3), 5.0, 0.25, 0.5], what
    with pytest.raises(_lib.SdumcError):      # the wrappers raise
        ops.adam_step_rates(*bufs, hyper, [(0, 8, -1.0, 1.0, False)])
    with pytest.raises(_lib.SdumcError):
        ops.zero_segments(bufs[0], [(8, 8, 1.0, 1.0, True), (0, 8, 1.0, 1.0, True)])
    # a misaligned bucket is refused as sdumc_adam_step refuses it
    odd = torch.full((n + 4,), -55.0, device="cuda")[1:n + 1]
    tb = ops.rate_segments([(0, 8, 1.0, 1.0, True)])
    assert lib.sdumc_adam_step_rates(odd.data_ptr(), *[b.data_ptr() for b in bufs[1:]], n, hyper.data_ptr(), 0.9, 0.999, 1e-8, 1e-5, 1.0,
                                     tb, 1, _lib.current_stream()) == -1
    assert lib.sdumc_zero_segments(odd.data_ptr(), n, tb, 1, _lib.current_stream()) == -1
    # ... and sdumc_adam_step itself refuses it before the step count advances (hyper is compared below)
    assert lib.sdumc_adam_step(odd.data_ptr(), *[b.data_ptr() for b in bufs[1:]], n, hyper.data_ptr(), 0.9, 0.999, 1e-8, 1e-5, 1.0,
                               _lib.current_stream()) == -1
    torch.cuda.synchronize()
    assert bool((odd == -55.0).all()) and hyper.tolist() == [np.float32(1e-3), 5.0, 0.25, 0.5]
