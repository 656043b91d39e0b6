"""Averaged weights for the loop that keeps its module: sdumc_ema_multi (ema_multi_kernel, csrc/adam.hip) and
sdumc_amd.optim.ema_update_ / get_ema_multi_avg_fn against the rule of tests/ema_ref.py and torch's own EMA function.

Lists of 1, 3, 96, 97 and 200 tensors (96 = one launch's table, 97 = a second launch with one tensor) with sizes from 1 to 5000
mixed: below a 16-byte group, a group and a remainder, one chunk of 1024 exactly, one more, several chunks.  All tensors of a list
are views into ONE buffer per side, separated by 1 to 4 sentinel floats, so that they start at every residue mod 4 -- both addresses
16-byte aligned (the 16-byte path), one of them, neither (one float per lane) -- and a write outside a tensor shows in a sentinel.
Bit equality with torch.lerp for w in {0.25, 0.5, 1}, the bound 2 * 2^-23 * max(|a|, |p|) against the fp64 rule for 1 - 0.999
and 1 - 0.9."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ema_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 5000, 3, 1024, 4, 1025, 5, 255, 2048, 7, 4099, 64, 1023, 2, 3000, 256, 1, 513)
COUNTS = (1, 3, 96, 97, 200)
WEIGHTS = (0.25, 0.5, 1.0, float(np.float32(1.0 - 0.999)), float(np.float32(1.0 - 0.9)))
SENTINEL = -77.25


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import ops
    return ops


def _offsets(k, gaps):
    sizes = [SIZES[i % len(SIZES)] for i in range(k)]
    offsets, cur = [], 0
    for i, n in enumerate(sizes):
        cur += gaps[i % len(gaps)]
        offsets.append(cur)
        cur += n
    return sizes, offsets, cur + 4


class _Packed:
    """k tensors as views into one buffer; tensor i starts gaps[i % len(gaps)] sentinel floats behind the end of tensor i - 1"""

    def __init__(self, k, gaps, seed):
        g = torch.Generator().manual_seed(seed)
        self.sizes, self.offsets, total = _offsets(k, gaps)
        values = torch.exp2(torch.rand(total, generator=g) * 24 - 12) * (torch.randint(0, 2, (total,), generator=g) * 2 - 1)
        self.mask = torch.zeros(total, dtype=torch.bool)
        for off, n in zip(self.offsets, self.sizes):
            self.mask[off:off + n] = True
        values[~self.mask] = SENTINEL
        self.buf = values.cuda()
        self.mask = self.mask.cuda()
        assert self.buf.data_ptr() % 16 == 0

    def views(self, buf=None):
        buf = self.buf if buf is None else buf
        return [buf[off:off + n] for off, n in zip(self.offsets, self.sizes)]


GAPS_A, GAPS_P = (1, 2, 4, 3, 1, 1, 3), (4, 1, 2, 3, 3)


def _residues(k):
    return {(x % 4 == 0, y % 4 == 0) for x, y in zip(_offsets(k, GAPS_A)[1], _offsets(k, GAPS_P)[1])}


assert _residues(200) == {(True, True), (True, False), (False, True), (False, False)}      # every alignment pairing occurs


@pytest.mark.parametrize("k", COUNTS)
def test_lists_of_tensors_at_odd_offsets(ops, k):
    worst = 0.0
    for w in WEIGHTS:
        a, p = _Packed(k, GAPS_A, 10 + k), _Packed(k, GAPS_P, 20 + k)
        a0, p0 = a.buf.clone(), p.buf.clone()
        ops.ema_multi(a.views(), p.views(), w)
        torch.cuda.synchronize()
        assert torch.equal(_bits(p.buf), _bits(p0)), "the parameters are read only"
        assert bool((a.buf[~a.mask] == SENTINEL).all()), f"k {k}, w {w}: a write outside the tensors"
        for i, (got, before, param) in enumerate(zip(a.views(), a.views(a0), p.views())):
            worst = max(worst, ema_ref.check(got, before, param, w, f"k {k}, tensor {i} of {got.numel()} elements"))
    print(f"{k} tensors: worst |ema - rule| / (2 * 2^-23 * max(|a|, |p|)) for w = 1 - 0.999 and 1 - 0.9: {worst:.4f}")


def test_the_same_bits_whatever_the_alignment(ops):
    """the 16-byte path and the float-per-lane path: the same data at aligned and at odd addresses, every weight"""
    k = 40
    for w in WEIGHTS:
        a, p = _Packed(k, GAPS_A, 5), _Packed(k, GAPS_P, 6)
        al_a = [v.clone() for v in a.views()]      # (fresh allocations: 16-byte aligned)
        al_p = [v.clone() for v in p.views()]
        assert all(t.data_ptr() % 16 == 0 for t in al_a + al_p)
        ops.ema_multi(a.views(), p.views(), w)
        ops.ema_multi(al_a, al_p, w)
        again = [v.clone() for v in a.views(_Packed(k, GAPS_A, 5).buf)]
        ops.ema_multi(again, al_p, w)              # ... and once more: the same bits on every run
        torch.cuda.synchronize()
        for x, y, z in zip(a.views(), al_a, again):
            assert torch.equal(_bits(x), _bits(y)) and torch.equal(_bits(y), _bits(z))


def test_ema_update_takes_views_and_rounds_the_weight_once(ops):
    from sdumc_amd import optim
    from sdumc_amd._lib import SdumcError
    k = 97
    for decay in (0.999, 0.9, 0.75, 0.0):
        a, p = _Packed(k, GAPS_A, 31), _Packed(k, GAPS_P, 32)
        w = ema_ref.weight(decay, fp32_decay=False)
        assert w == float(np.float32(1.0 - decay))
        # once through ema_update_, once more through the closure with torch's multi_avg_fn signature, each from a snapshot
        for update in (lambda: optim.ema_update_(a.views(), p.views(), decay),
                       lambda: optim.get_ema_multi_avg_fn(decay)(a.views(), p.views(), torch.tensor(5))):
            a0 = a.buf.clone()
            update()
            torch.cuda.synchronize()
            for i, (got, before, param) in enumerate(zip(a.views(), a.views(a0), p.views())):
                ema_ref.check(got, before, param, w, f"decay {decay}, tensor {i}")
            assert bool((a.buf[~a.mask] == SENTINEL).all())
    x, y = torch.zeros(8, device="cuda"), torch.ones(8, device="cuda")
    for bad in (True, "0.9", torch.tensor(0.9), float("nan"), -0.1, 1.1, None):
        with pytest.raises(SdumcError, match="decay"):
            optim.ema_update_([x], [y], bad)
        with pytest.raises(SdumcError, match="decay"):
            optim.get_ema_multi_avg_fn(bad)
    for bad_a, bad_p in (([x], [y, y]), ([x.cpu()], [y]), ([x], [y.double()]), ([x], [y[:7]]), ([torch.zeros(4, 4, device="cuda").t()], [y[:16]])):
        with pytest.raises(SdumcError):
            optim.ema_update_(bad_a, bad_p, 0.9)
    assert bool((x == 0).all())
    optim.ema_update_([], [], 0.9)      # nothing to do


def test_averaged_model_over_the_dropin_module():
    """AveragedModel(model, multi_avg_fn=sdumc_amd.optim.get_ema_multi_avg_fn(d)) for three updates against torch's own
    get_ema_multi_avg_fn(d) on a copy of the average as it was before each update (nothing accumulates): within the bound of the
    fp64 rule, and within the bound of torch's result"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    from sdumc_amd import optim
    from sdumc_amd.model import get_models
    torch.manual_seed(5)
    model = get_models(types.SimpleNamespace(input_dims=(64, 32, 48, 32), model="wengnet_mosei_mult_views_text_missing")).cuda()
    for decay in (0.999, 0.9):
        w = ema_ref.weight(decay, fp32_decay=False)
        avg = AveragedModel(model, multi_avg_fn=optim.get_ema_multi_avg_fn(decay))
        avg.update_parameters(model)      # (the first call copies)
        for got, p in zip(avg.parameters(), model.parameters()):
            assert torch.equal(_bits(got.detach()), _bits(p.detach()))
        g = torch.Generator().manual_seed(3)
        worst = 0.0
        for k in range(3):
            with torch.no_grad():
                for p in model.parameters():
                    p.add_((torch.randn(p.shape, generator=g) * 1e-2).cuda())
            before = [a.detach().clone() for a in avg.parameters()]
            ref = [b.clone() for b in before]
            get_ema_multi_avg_fn(decay)(ref, [p.detach() for p in model.parameters()], k + 1)
            avg.update_parameters(model)
            torch.cuda.synchronize()
            n = 0
            for got, a, p, r in zip(avg.parameters(), before, model.parameters(), ref):
                got, p = got.detach().reshape(-1), p.detach().reshape(-1)
                worst = max(worst, ema_ref.check(got, a.reshape(-1), p, w, f"decay {decay}, update {k}"))
                assert bool(((got.double() - r.reshape(-1).double()).abs() <= ema_ref.bound(a.reshape(-1), p)).all()), (decay, k)
                assert not torch.equal(got, a.reshape(-1))
                n += 1
            assert n == len(before) > 80 and int(avg.n_averaged) == k + 2
        print(f"AveragedModel, decay {decay}: worst ratio to the bound over three updates {worst:.4f}")


def test_refusals_write_nothing(ops):
    from sdumc_amd import _lib
    lib = _lib.lib
    a, p = torch.full((64,), -11.0, device="cuda"), torch.full((64,), -22.0, device="cuda")

    def call(segs, nseg=None, w=0.25):
        tb = (_lib.EmaSeg * max(1, len(segs)))()
        for s, (x, y, n) in zip(tb, segs):
            s.ema, s.param, s.n = x, y, n
        return lib.sdumc_ema_multi(tb if segs else None, len(segs) if nseg is None else nseg, w, _lib.current_stream())

    A, P = a.data_ptr(), p.data_ptr()
    ok = [(A, P, 16), (A + 68, P + 132, 7)]
    for what, (segs, kw) in {"no table": ([], {}), "nseg 0": (ok, {"nseg": 0}), "nseg < 0": (ok, {"nseg": -1}),
                             "ema NULL": (ok + [(None, P, 8)], {}), "param NULL": (ok + [(A, None, 8)], {}), "n 0": (ok + [(A, P, 0)], {}),
                             "n < 0": (ok + [(A, P, -5)], {}), "w < 0": (ok, {"w": -0.5}), "w > 1": (ok, {"w": 1.5}),
                             "w NaN": (ok, {"w": float("nan")}), "not a float address": ([(A + 2, P, 4)], {})}.items():
        assert call(segs, **kw) == -1, what
        torch.cuda.synchronize()
        assert bool((a == -11.0).all()) and bool((p == -22.0).all()), what
    with pytest.raises(_lib.SdumcError):
        ops.ema_multi([a], [p], 2.0)
    assert call(ok, w=1.0) == 0
    torch.cuda.synchronize()
    want = torch.full((64,), -11.0)
    want[:16], want[17:24] = -22.0, -22.0
    assert torch.equal(a.cpu(), want)
