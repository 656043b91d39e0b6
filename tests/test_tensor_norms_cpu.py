"""CPU-only: the host side of the record by tensor (sdumc_tensor_norms, record.TensorNorms, train_epoch(by_tensor=...)): the ctypes
segment against the C compiler's view of include/sdumc_hip.h, the refusals the entry makes before any launch (they need no device),
the scratch query's dependence on the counts alone, TrainRecord.empty / fits / reset with the option, first_nonfinite() and
update_ratio() on a hand-made record, and the option's values checked on the host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segment_struct_matches_the_header(tmp_path):
    from sdumc_amd import _lib
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "sdumc_hip.h"
int main(){printf("%zu %zu %zu %zu %d\n", sizeof(sdumc_norm_seg), offsetof(sdumc_norm_seg, x), offsetof(sdumc_norm_seg, y),
 offsetof(sdumc_norm_seg, count), SDUMC_TENSOR_NORMS_MAX_SEGS); return 0;}
'''
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "t")]).split()]
    S = _lib.NormSeg
    assert got == [C.sizeof(S), S.x.offset, S.y.offset, S.count.offset, _lib.TENSOR_NORMS_MAX_SEGS]
    assert {"sdumc_tensor_norms", "sdumc_tensor_norms_scratch_bytes"} <= set(_lib.EXPORTS)


def _segs(counts, x=0x1000, y=0):
    from sdumc_amd import _lib
    segs = (_lib.NormSeg * len(counts))()
    for s, c in zip(segs, counts):
        s.x, s.y, s.count = x or None, y or None, c
    return segs


def test_refusals_without_a_device():
    """every refusal comes back as SDUMC_EINVAL before a launch: fake (never dereferenced) device addresses are enough"""
    from sdumc_amd import _lib
    lib, cap = _lib.lib, _lib.TENSOR_NORMS_MAX_SEGS
    ok = _segs([5, 4097])
    need = lib.sdumc_tensor_norms_scratch_bytes(ok, 2)
    assert need > 0 and need % 16 == 0
    out, cnt, dif, scr = 0x2000, 0x3000, 0x4000, 0x8000

    def call(segs, n, norm=out, bad=cnt, diff=None, scratch=scr, nbytes=need):
        return lib.sdumc_tensor_norms(segs, n, norm, bad, diff, scratch, nbytes, None)

    assert call(None, 2) == -1                                        # NULL table
    assert call(ok, 0) == -1 and call(ok, -1) == -1                   # n < 1
    assert call(_segs([1] * (cap + 1)), cap + 1, nbytes=1 << 20) == -1      # n above the cap
    assert call(_segs([5, -1]), 2) == -1                              # a negative count
    assert call(_segs([5, 4], x=0), 2) == -1                          # x NULL with elements to read
    assert call(_segs([5, 4], x=0x1002), 2) == -1                     # x not 4-byte aligned
    assert call(_segs([5, 4], y=0x5001), 2, diff=dif) == -1           # y not 4-byte aligned
    assert call(ok, 2, norm=None) == -1 and call(ok, 2, bad=None) == -1
    assert call(ok, 2, norm=out + 2) == -1 and call(ok, 2, bad=cnt + 1) == -1
    assert call(_segs([5, 4], y=0x5000), 2) == -1                     # a snapshot, and nowhere to write diff_norm
    assert call(_segs([5, 4], y=0x5000), 2, diff=dif + 2) == -1
    assert call(ok, 2, scratch=None) == -1 and call(ok, 2, scratch=scr + 8) == -1
    assert call(ok, 2, nbytes=need - 1) == -1 and call(ok, 2, nbytes=0) == -1      # a short scratch
    # a misaligned table: the same bytes, 4 past an 8-byte boundary
    raw = C.create_string_buffer(C.sizeof(ok) + 16)
    base = C.addressof(raw)
    base += (-base) % 8 + 4
    C.memmove(base, ok, C.sizeof(ok))
    assert call(C.cast(base, C.POINTER(_lib.NormSeg)), 2) == -1
    # the query refuses what the entry refuses
    assert lib.sdumc_tensor_norms_scratch_bytes(None, 2) == 0 and lib.sdumc_tensor_norms_scratch_bytes(ok, 0) == 0
    assert lib.sdumc_tensor_norms_scratch_bytes(_segs([5, -1]), 2) == 0
    assert lib.sdumc_tensor_norms_scratch_bytes(_segs([1] * (cap + 1)), cap + 1) == 0


def test_scratch_depends_on_the_counts_alone():
    """the chunk table is cut by count, never by address: 20 bytes per chunk of 8192 floats (at most 1024 per segment), rounded to 16"""
    from sdumc_amd import _lib
    q = _lib.lib.sdumc_tensor_norms_scratch_bytes
    counts = [0, 1, 8192, 8193, 1 << 20, (1 << 23) + 1, 1 << 30]
    chunks = [1, 1, 1, 2, 128, 1024, 1024]
    for c, k in zip(counts, chunks):
        assert q(_segs([c]), 1) == (20 * k + 15) // 16 * 16, c
    want = (20 * sum(chunks) + 15) // 16 * 16
    assert q(_segs(counts), len(counts)) == want
    assert q(_segs(counts, x=0x1004, y=0x700c), len(counts)) == want


def _layout():
    from sdumc_amd.engine import ParamLayout
    return ParamLayout.get(48, 32, 40)


def test_train_record_empty_fits_reset_with_the_option():
    from sdumc_amd import _lib
    from sdumc_amd.engine import ParamLayout
    from sdumc_amd.record import TrainRecord, layout_segments
    lay = _layout()
    names, offs, counts = layout_segments(lay)
    assert list(names) == lay.live_names() and len(names) == 83 and {1, 3, 7} <= set(counts)
    assert all(o == lay.entries[k][0] for o, k in zip(offs, names)) and max(o + c for o, c in zip(offs, counts)) <= lay.live
    plain = TrainRecord.empty(9, 4, "cpu").reset()
    assert plain.by_tensor is None and plain.fits(9, 4, "cpu", False) and not plain.fits(9, 4, "cpu", False, 0, True, lay)
    g = TrainRecord.empty(9, 4, "cpu", by_tensor=True, layout=lay).reset()
    bt = g.by_tensor
    assert bt.names == names and bt.grad_norm.shape == (4, 83) and bt.grad_norm.dtype == torch.float32
    assert bt.grad_nonfinite.shape == (4, 83) and bt.grad_nonfinite.dtype == torch.int32
    assert bt.param_norm is None and bt.update_norm is None and bt.snapshot is None and bt.scratch.numel() > 0 and bt.mode is True
    assert bool(torch.isnan(bt.grad_norm).all()) and not bool(bt.grad_nonfinite.any()) and bt.steps == 0
    assert g.fits(9, 4, "cpu", False, 0, True, lay) and g.fits(9, 3, "cpu", False, 0, True, lay)
    assert not g.fits(9, 5, "cpu", False, 0, True, lay)                       # more steps than rows
    assert not g.fits(9, 4, "cpu", False) and not g.fits(9, 4, "cpu", False, 0, "updates", lay)
    assert not g.fits(9, 4, "cpu", False, 0, True, ParamLayout.get(64, 32, 40))      # another run's tensors
    assert not g.fits(9, 4, "cpu", False, lay.live, True, lay)                # (the options are independent: no grad_norm scratch here)
    u = TrainRecord.empty(9, 4, "cpu", n_grads=lay.live, by_tensor="updates", layout=lay).reset()
    bu = u.by_tensor
    assert bu.mode == "updates" and bu.param_norm.shape == bu.update_norm.shape == (4, 83) and bu.snapshot.numel() == lay.live + 4
    assert u.fits(9, 4, "cpu", False, lay.live, "updates", lay) and not u.fits(9, 4, "cpu", False, lay.live, True, lay)
    # reset: NaN / 0 everywhere, no step filled -- and `steps` of the record is `steps` of its by_tensor part
    bu.grad_norm.fill_(1.0), bu.update_norm.fill_(2.0), bu.param_norm.fill_(3.0), bu.grad_nonfinite.fill_(4), bu.param_nonfinite.fill_(5)
    u.steps = 3
    assert bu.steps == 3
    u.reset()
    assert u.steps == bu.steps == 0 and not bool(bu.grad_nonfinite.any()) and not bool(bu.param_nonfinite.any())
    assert all(bool(torch.isnan(t).all()) for t in (bu.grad_norm, bu.update_norm, bu.param_norm))
    with pytest.raises(_lib.SdumcError):
        TrainRecord.empty(9, 4, "cpu", by_tensor="nonsense", layout=lay)
    with pytest.raises(_lib.SdumcError):
        TrainRecord.empty(9, 4, "cpu", by_tensor=True)                         # no layout
    with pytest.raises(_lib.SdumcError):
        g.fits(9, 4, "cpu", False, 0, "nonsense", lay)


def test_first_nonfinite_and_update_ratio_by_hand():
    from sdumc_amd import _lib
    from sdumc_amd.record import COL_B, TrainRecord
    lay = _layout()
    rec = TrainRecord.empty(9, 4, "cpu", by_tensor="updates", layout=lay).reset()
    bt = rec.by_tensor
    n = len(bt.names)
    bt.grad_norm[:3] = 1.0
    bt.param_norm[:3] = torch.arange(1, 3 * n + 1, dtype=torch.float32).reshape(3, n)
    bt.update_norm[:3] = 0.5
    rec.log[:3] = 0.0
    rec.log[:3, COL_B] = 3.0
    rec.steps = 3
    assert bt.first_nonfinite() is None and rec.summary()["first_nonfinite"] is None
    r = bt.update_ratio()
    assert r.dtype == np.float64 and r.shape == (3, n)
    assert np.array_equal(r, 0.5 / np.arange(1, 3 * n + 1, dtype=np.float64).reshape(3, n))
    # the first hit in step order, then in table order; a row beyond `steps` does not count
    bt.grad_nonfinite[3, 0] = 7
    assert bt.first_nonfinite() is None
    bt.grad_nonfinite[2, 5] = 1
    bt.grad_norm[2, 5] = float("nan")
    assert bt.first_nonfinite() == (2, bt.names[5])
    bt.grad_norm[1, 40] = float("inf")                       # an overflow of the one rounding to fp32: count 0, norm +Inf
    bt.grad_nonfinite[1, 60] = 2
    assert bt.first_nonfinite() == (1, bt.names[40]) and rec.summary()["first_nonfinite"] == (1, bt.names[40])
    # zero weights: inf, and NaN where the update is zero too -- no exception
    bt.param_norm[0, 0] = 0.0
    bt.param_norm[0, 1] = 0.0
    bt.update_norm[0, 1] = 0.0
    r = bt.update_ratio()
    assert np.isinf(r[0, 0]) and np.isnan(r[0, 1])
    plain = TrainRecord.empty(9, 4, "cpu", by_tensor=True, layout=lay).reset()
    with pytest.raises(_lib.SdumcError):
        plain.by_tensor.update_ratio()
    no = TrainRecord.empty(9, 4, "cpu").reset()
    no.log[:1] = 0.0
    no.log[:1, COL_B] = 3.0
    no.steps = 1
    assert "first_nonfinite" not in no.summary()


def test_train_epoch_refuses_an_unknown_option_on_the_host():
    """by_tensor='nonsense' is refused before the trainer's arena is asked for anything -- no device call is made"""
    from sdumc_amd import _lib, engine, record
    tr = object.__new__(engine.FusedTrainer)      # (no constructor: it would need a CUDA parameter buffer)
    tr.arena = type("A", (), {"sets": [0, 1]})()
    for bad in ("nonsense", "update", 2, "True"):
        with pytest.raises(_lib.SdumcError, match="by_tensor"):
            tr.train_epoch(None, None, by_tensor=bad)
        with pytest.raises(_lib.SdumcError, match="by_tensor"):
            record.by_tensor_mode(bad)
    assert record.by_tensor_mode(None) is False and record.by_tensor_mode(True) is True and record.by_tensor_mode("updates") == "updates"


def test_tensor_norms_helper_refuses_cpu_and_other_dtypes():
    from sdumc_amd import _lib, record
    with pytest.raises(_lib.SdumcError):
        record.tensor_norms([torch.zeros(4)])
    with pytest.raises(_lib.SdumcError):
        record.tensor_norms([])
    with pytest.raises(_lib.SdumcError):
        record.tensor_norms([torch.zeros(4, dtype=torch.float64)])
    with pytest.raises(_lib.SdumcError):
        record.tensor_norms([None])
