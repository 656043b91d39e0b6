"""Averaged weights at the kernel level: sdumc_adam_step_ema (the EMA forms of adam_kernel and adam_rates_kernel, csrc/adam.hip) against
sdumc_adam_step / sdumc_adam_step_rates, the launches it is a form of, and against the rule of tests/ema_ref.py.

Buckets of n = 1, 3, 4, 5, 1023, 1024, 1025 and 4099 elements: below one 16-byte group, one group and a tail, the last whole workgroup,
more than one workgroup, a scalar tail (n % 4) of every length.  Random p, g, m, v >= 0 and a with magnitudes 2^-12 .. 2^12.  Every
buffer is a view 64 floats into a larger allocation filled with a sentinel: the bytes in front of and behind it must not change.
Without a table, and with tables whose segments start and end at odd offsets: a one-element segment, frozen segments, an
lr_scale = 0 segment, alignment gaps that belong to no segment, a last segment that reaches into the scalar tail (A) or stops short of
it (B).

For each: p, m, v and hyper are bit-equal to the plain call on copies; the EMA is torch.lerp's bit for bit for w in {0.25, 0.5, 1}
and within 2 * 2^-23 * max(|a|, |p|) of the fp64 rule for decay 0.999 and 0.9 (ema_ref has the derivation), from the EMA before
and the parameters AFTER the update; frozen elements keep all four buffers' bits."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ema_ref  # noqa: E402

pytestmark = pytest.mark.gpu

LR, WD = 1e-3, 1e-2
NS = (1, 3, 4, 5, 1023, 1024, 1025, 4099)
DECAYS = (0.75, 0.5, 0.0, 0.999, 0.9)      # w = 0.25, 0.5, 1 (bit equality) and two that are no powers of two (the bound)
MARGIN, SENTINEL = 64, -77.25
#          gap len  lr_scale wd_scale frozen
PATTERN_A = ((1, 1, 2.0, 1.0, False), (0, 3, 1.0, 1.0, True), (2, 7, 0.0, 1.0, False), (1, 250, 0.5, 0.0, False),
             (3, 513, 1.0, 1.0, True), (0, 300, 0.25, 0.5, False), (2, 1029, 1.0, 0.3, False), (1, 1, 1.0, 1.0, True),
             (3, 2000, 2.0, 1.0, False))
PATTERN_B = ((3, 2, 1.0, 1.0, True), (1, 1, 0.5, 1.0, False), (0, 5, 1.0, 0.0, False), (2, 258, 1.0, 1.0, True),
             (1, 255, 0.0, 0.0, False), (0, 1, 1.0, 1.0, False), (3, 1500, 1.0, 1.0, False), (2, 900, 0.5, 1.0, True),
             (0, 1200, 1.0, 1.0, False))


def _table(pattern, n, to_the_end):
    """segments of `pattern` laid into [0, n) until it is full; the last one is cut to end at n (into the scalar tail) or at n - 2"""
    end = n if to_the_end else n - 2
    segs, cur = [], 0
    for gap, length, ls, ws, fr in pattern:
        off = cur + gap
        if off >= end:
            break
        length = min(length, end - off)
        segs.append((off, length, ls, ws, fr))
        cur = off + length
    if segs and cur < end:      # (the pattern ran out first: the last segment takes the rest)
        off, length, ls, ws, fr = segs[-1]
        segs[-1] = (off, end - off, ls, ws, fr)
    return segs


def _tables(n):
    out = {"none": None}
    a, b = _table(PATTERN_A, n, True), _table(PATTERN_B, n, False)
    if a:
        out["A"] = a
    if b:
        out["B"] = b
    if n <= 5:      # (the patterns barely fit: the whole bucket as one segment, scaled and frozen)
        out["whole"], out["frozen"] = [(0, n, 0.5, 0.5, False)], [(0, n, 1.0, 1.0, True)]
    return out


# the tables are what the docstring says
_big = _tables(4099)
assert _big["A"][-1][0] + _big["A"][-1][1] == 4099 and _big["B"][-1][0] + _big["B"][-1][1] == 4097
for _tb in (_big["A"], _big["B"]):
    assert any(s[1] == 1 for s in _tb) and any(s[4] for s in _tb) and any(s[2] == 0.0 and not s[4] for s in _tb)
    assert {s[0] % 4 for s in _tb} == {0, 1, 2, 3} and any(a[0] + a[1] < b[0] for a, b in zip(_tb, _tb[1:]))
    assert all(a[0] + a[1] <= b[0] for a, b in zip(_tb, _tb[1:]))
assert all(len(_tables(n)) >= 3 for n in NS)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, what):
    bad = torch.nonzero(_bits(a) != _bits(b)).flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} of {a.numel()} elements differ, the first at {bad[:8].tolist()}"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import ops
    return ops


def _values(n, g, sign=True):
    v = torch.exp2(torch.rand(n, generator=g) * 24 - 12)
    return v * (torch.randint(0, 2, (n,), generator=g) * 2 - 1) if sign else v


class _Guarded:
    """a 16-byte aligned view of n floats with MARGIN sentinel floats in front of and behind it"""

    def __init__(self, values):
        n = values.numel()
        self.whole = torch.full((n + 2 * MARGIN,), SENTINEL, device="cuda")
        self.t = self.whole[MARGIN:MARGIN + n]
        self.t.copy_(values)
        assert self.t.data_ptr() % 16 == 0

    def margins_intact(self):
        return bool((self.whole[:MARGIN] == SENTINEL).all()) and bool((self.whole[MARGIN + self.t.numel():] == SENTINEL).all())


def _data(n):
    g = torch.Generator().manual_seed(1000 + n)
    return {"p": _values(n, g), "g": _values(n, g), "m": _values(n, g), "v": _values(n, g, False), "a": _values(n, g)}


def _hyper(t=0.0):
    return torch.tensor([LR, float(t), 0.0, 0.0], device="cuda")


def _plain(ops, d, table, t0):
    """the launch the EMA form is a form of, on copies -> (p, m, v, hyper)"""
    p, m, v, hyper = d["p"].cuda(), d["m"].cuda(), d["v"].cuda(), _hyper(t0)
    if table is None:
        ops.adam_step(p, d["g"].cuda(), m, v, hyper, weight_decay=WD)
    else:
        ops.adam_step_rates(p, d["g"].cuda(), m, v, hyper, table, weight_decay=WD)
    return p, m, v, hyper


def _ema_run(ops, d, table, t0, decay, warmup=False):
    bufs = {k: _Guarded(d[k]) for k in ("p", "g", "m", "v", "a")}
    hyper = _hyper(t0)
    ops.adam_step_ema(bufs["p"].t, bufs["g"].t, bufs["m"].t, bufs["v"].t, hyper, bufs["a"].t, decay, warmup, segments=table,
                      weight_decay=WD)
    torch.cuda.synchronize()
    return bufs, hyper


def _frozen_mask(n, table):
    mask = torch.zeros(n, dtype=torch.bool)
    for off, length, _, _, fr in table or ():
        if fr:
            mask[off:off + length] = True
    return mask.cuda()


def _check(ops, n, name, table, decay, t0=0.0, warmup=False, w=None):
    d = _data(n)
    want = _plain(ops, d, table, t0)
    bufs, hyper = _ema_run(ops, d, table, t0, decay, warmup)
    what = f"n {n}, table {name}, decay {decay}, warm-up {warmup}, step count {t0}"
    for key, ref in zip("pmv", want):
        _same(bufs[key].t, ref, f"{what}: {key}")
    _same(hyper, want[3], f"{what}: hyper")
    _same(bufs["g"].t, d["g"].cuda(), f"{what}: the gradient (read only)")
    for key, b in bufs.items():
        assert b.margins_intact(), f"{what}: bytes around {key} changed"
    if w is None:
        w = ema_ref.weight(decay)
    a0, fm = d["a"].cuda(), _frozen_mask(n, table)
    # the rule from the EMA before and the parameters AFTER the update, where the parameter is not frozen ...
    ratio = ema_ref.check(bufs["a"].t[~fm], a0[~fm], want[0][~fm], w, what)
    # ... and a frozen element keeps all four buffers' bits
    for key in "pmva":
        _same(bufs[key].t[fm], d[key].cuda()[fm], f"{what}: frozen {key}")
    return ratio


@pytest.mark.parametrize("n", NS)
def test_every_size_table_and_decay(ops, n):
    worst = 0.0
    for name, table in _tables(n).items():
        for decay in DECAYS:
            worst = max(worst, _check(ops, n, name, table, decay))
    print(f"n = {n}: worst |ema - rule| / (2 * 2^-23 * max(|a|, |p|)) over the tables, decay 0.999 and 0.9: {worst:.4f}")


def test_decay_zero_holds_the_parameters_bits_and_a_still_parameter_keeps_its_average(ops):
    d = _data(4099)
    for name, table in _tables(4099).items():
        bufs, _ = _ema_run(ops, d, table, 0.0, 0.0)
        fm = _frozen_mask(4099, table)
        _same(bufs["a"].t[~fm], bufs["p"].t[~fm], f"decay 0, table {name}")
    # the average starts as a copy of the parameters: where the parameter stays (lr_scale = 0) the average stays, by arithmetic
    d = dict(d, a=d["p"].clone())
    table = _tables(4099)["A"]
    bufs, _ = _ema_run(ops, d, table, 0.0, 0.999)
    for off, length, ls, _, fr in table:
        if ls == 0.0 and not fr:
            _same(bufs["p"].t[off:off + length], d["p"].cuda()[off:off + length], "lr_scale 0: the parameter")
            _same(bufs["a"].t[off:off + length], d["a"].cuda()[off:off + length], "lr_scale 0: the average")
            assert not torch.equal(bufs["m"].t[off:off + length], d["m"].cuda()[off:off + length])


def test_the_same_bits_on_every_run(ops):
    d = _data(4099)
    for table in _tables(4099).values():
        first, _ = _ema_run(ops, d, table, 3.0, 0.999)
        again, _ = _ema_run(ops, d, table, 3.0, 0.999)
        for key in "pmva":
            _same(first[key].t, again[key].t, key)


@pytest.mark.parametrize("t0", [0, 1, 7, 8, 1000])
def test_warmup_applies_the_closed_form(ops, t0):
    """The step count after the increment is t = t0 + 1; w = fp32(1 - min(decay, (1 + t) / (10 + t))).  t = 8 (from 7) gives w = 0.5:
    bit equality.  decay 0.9 is reached at t = 80: from 1000 the weight is the decay's own."""
    t = t0 + 1
    for decay in (0.999, 0.9):
        w = float(np.float32(1.0 - min(float(np.float32(decay)), (1.0 + t) / (10.0 + t))))
        assert w == ema_ref.weight(decay, t, warmup=True)
        if t == 8:
            assert w == 0.5
        if t0 == 1000 and decay == 0.9:
            assert w == ema_ref.weight(0.9)
        else:
            assert w > ema_ref.weight(decay)      # (the schedule is still in force: a wrong w would miss the checks below)
        for n in (5, 1025):
            for name, table in _tables(n).items():
                _check(ops, n, name, table, decay, t0=float(t0), warmup=True, w=w)
    # the flag off: the decay's own weight whatever the step count
    _check(ops, 1025, "A", _tables(1025)["A"], 0.999, t0=float(t0))


def test_a_wrong_reading_misses_the_bound(ops):
    """the check can tell: the rule fed the parameters BEFORE the update, or another step's warm-up weight, fails it"""
    n, decay = 4099, 0.9
    d = _data(n)
    bufs, _ = _ema_run(ops, d, None, 0.0, decay)
    a0, w = d["a"].cuda(), ema_ref.weight(decay)
    assert ema_ref.worst(bufs["a"].t, a0, bufs["p"].t, w) <= 1.0
    assert ema_ref.worst(bufs["a"].t, a0, d["p"].cuda(), w) > 1.0
    bufs, _ = _ema_run(ops, d, None, 3.0, 0.999, warmup=True)
    assert ema_ref.worst(bufs["a"].t, a0, bufs["p"].t, ema_ref.weight(0.999, 4, warmup=True)) <= 1.0
    assert ema_ref.worst(bufs["a"].t, a0, bufs["p"].t, ema_ref.weight(0.999, 3, warmup=True)) > 1.0


def test_refusals_write_nothing_and_leave_the_step_count(ops):
    from sdumc_amd import _lib
    lib, n = _lib.lib, 4096
    sent = (-11.0, -22.0, -33.0, -44.0, -55.0)
    bufs = [torch.full((n + 8,), s, device="cuda") for s in sent]
    p, g, m, v, a = (b[:n] for b in bufs)
    hyper = torch.tensor([1e-3, 5.0, 0.25, 0.5], device="cuda")
    good = ops.rate_segments([(0, 8, 1.0, 1.0, False)])

    def call(p=p, g=g, m=m, v=v, n=n, hy=hyper, segs=None, nseg=0, a=a, decay=0.9):
        return lib.sdumc_adam_step_ema(_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), n, _lib.ptr(hy), 0.9, 0.999, 1e-8, 1e-5, 1.0,
                                       segs, nseg, _lib.ptr(a), decay, 0, _lib.current_stream())

    odd = bufs[4][1:n + 1]
    cases = {"ema NULL": {"a": None}, "ema misaligned": {"a": odd}, "ema is param": {"a": p}, "ema overlaps param": {"a": bufs[0][4:n + 4]},
             "decay < 0": {"decay": -0.1}, "decay > 1": {"decay": 1.001}, "decay NaN": {"decay": float("nan")},
             "param NULL": {"p": None}, "grad NULL": {"g": None}, "exp_avg NULL": {"m": None}, "exp_avg_sq NULL": {"v": None},
             "hyper NULL": {"hy": None}, "n 0": {"n": 0}, "param misaligned": {"p": bufs[0][1:n + 1]},
             "grad misaligned": {"g": bufs[1][2:n + 2]}, "a table without a count": {"segs": good, "nseg": 0},
             "a count without a table": {"nseg": 1}, "nseg 97": {"segs": ops.rate_segments([(4 * i, 3, 1.0, 1.0, True) for i in range(97)]),
                                                                "nseg": 97},
             "overlapping": {"segs": ops.rate_segments([(0, 8, 1.0, 1.0, True), (7, 8, 1.0, 1.0, True)]), "nseg": 2},
             "behind the end": {"segs": ops.rate_segments([(4090, 7, 1.0, 1.0, True)]), "nseg": 1},
             "negative lr_scale": {"segs": ops.rate_segments([(0, 8, -0.5, 1.0, True)]), "nseg": 1}}
    for what, kw in cases.items():
        assert call(**kw) == -1, what
        torch.cuda.synchronize()
        for b, s in zip(bufs, sent):
            assert bool((b == s).all()), what
        assert hyper.tolist() == [np.float32(1e-3), 5.0, 0.25, 0.5], what
    with pytest.raises(_lib.SdumcError):      # the wrapper raises
        ops.adam_step_ema(p, g, m, v, hyper, a, 1.5)
    # ... and the accepted call goes through: the count advances once
    assert call(segs=good, nseg=1) == 0 and call() == 0
    torch.cuda.synchronize()
    assert float(hyper[1]) == 7.0 and bool((bufs[4][n:] == -55.0).all()) and bool((bufs[0][n:] == -11.0).all())
