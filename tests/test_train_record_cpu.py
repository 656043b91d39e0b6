"""Host side of the training epoch's record (sdumc_amd/record.py), no GPU: TrainRecord built from CPU tensors -- results() is the
dictionary the reference's training pass returns (main_frame_val_text_missing.py:168-175) over the visited rows in store order,
summary() the epoch's B-weighted loss means, gradient-norm figures and non-finite steps from the [steps, 12] log -- and the argument
checks of sdumc_epoch_record, which come back before any HIP call."""
import types

import numpy as np
import pytest
import torch

N = 9
EMB_KEYS = {"fused": ("full_rep", "missing_rep", (128,)), "rnc": ("full_rnc", "missing_rnc", (64,)),
            "text_hidden": ("text_rep_query_full", "text_rep_query_missing", (256,)),
            "cross_text": ("text_rep_full", "text_rep_missing", (7, 128))}
BASE = {"val_mse_full", "val_mse_missing", "val_preds_full", "val_preds_missing", "val_labels", "names"}


def _store():
    g = torch.Generator().manual_seed(0)
    vals = torch.round((torch.rand(N, generator=g) * 6 - 3) * 10) / 10
    return types.SimpleNamespace(names=[f"utt{i:03d}" for i in range(N)], vals=vals)


def _record(embeddings, steps=4):
    from sdumc_amd import TrainRecord
    g = torch.Generator().manual_seed(1)
    visited = [7, 1, 4, 2, 8]      # a partial epoch, in sampler order
    rec = TrainRecord.empty(N, steps, "cpu", embeddings=embeddings).reset()
    rec.seen[visited] = 1
    rec.preds[:, visited] = torch.randn(2, len(visited), generator=g)
    for t in (rec.embeddings or {}).values():
        t[:, visited] = torch.randn((2, len(visited)) + tuple(t.shape[2:]), generator=g)
    return rec, sorted(visited)


def _log(rec, rows):
    """fill log[:len(rows)] from (losses[8], grad_norm, nonfinite, B, lr) tuples"""
    for i, (losses, gn, bad, b, lr) in enumerate(rows):
        rec.log[i] = torch.tensor(list(losses) + [gn, bad, b, lr], dtype=torch.float32)
    rec.steps = len(rows)
    return rec


def test_package_exports_the_record():
    import sdumc_amd
    from sdumc_amd import record
    assert sdumc_amd.TrainRecord is record.TrainRecord and record.LOG_COLS == 12 and len(record.LOSS_NAMES) == 8


@pytest.mark.parametrize("embeddings", [False, True])
def test_results_keeps_the_visited_rows_in_store_order(embeddings):
    rec, rows = _record(embeddings)
    store = _store()
    assert bool(torch.isnan(rec.preds[:, [0, 3, 5, 6]]).all())      # rows not visited hold NaN
    out = rec.results(store)
    assert out["names"] == [store.names[i] for i in rows]
    lab = store.vals.numpy()[rows]
    assert np.array_equal(out["val_labels"], lab) and out["val_labels"].shape == (5,)
    for s, k in enumerate(("val_preds_full", "val_preds_missing")):
        assert out[k].shape == (5, 1) and out[k].dtype == np.float32
        assert np.array_equal(out[k].reshape(-1), rec.preds[s].numpy()[rows])
    assert out["val_mse_full"] == float(np.mean((lab - rec.preds[0].numpy()[rows]) ** 2))
    assert out["val_mse_missing"] == float(np.mean((lab - rec.preds[1].numpy()[rows]) ** 2))
    if not embeddings:
        assert set(out) == BASE
        return
    assert set(out) == BASE | {k for v in EMB_KEYS.values() for k in v[:2]}
    for name, (kf, km, shape) in EMB_KEYS.items():
        for s, k in enumerate((kf, km)):
            assert out[k].shape == (5,) + shape
            assert np.array_equal(out[k], rec.embeddings[name][s].numpy()[rows])


def test_summary_weights_every_step_by_its_batch_size():
    """three steps of 8, 8 and 5 samples (a short last batch): every loss entry's mean is sum(B_i l_i) / sum(B_i) in float64 -- for the
    MSE entries the epoch's mean over its 21 utterances, not the mean of the three batch means"""
    from sdumc_amd.record import LOSS_NAMES
    rs = np.random.RandomState(3)
    losses = rs.uniform(0.1, 2.0, (3, 8)).astype(np.float32)
    losses[:, 7] = 0.0
    rec, _ = _record(False, steps=5)
    _log(rec, [(losses[0], 1.5, 0.0, 8, 1e-3), (losses[1], 4.25, 0.0, 8, 1e-3), (losses[2], 0.75, 0.0, 5, 5e-4)])
    s = rec.summary()
    w = np.array([8.0, 8.0, 5.0])
    for k, name in enumerate(LOSS_NAMES):
        assert s[name] == pytest.approx(float((losses[:, k].astype(np.float64) * w).sum() / 21.0), rel=1e-15), name
    assert LOSS_NAMES[:3] == ("total", "mse_full", "mse_missing") and LOSS_NAMES[6] == "contrast"
    assert abs(s["mse_full"] - float(losses[:, 1].mean())) > 1e-4      # (the unweighted mean is another number)
    assert s["grad_norm_max"] == 4.25 and s["grad_norm_last"] == 0.75 and s["nonfinite_steps"] == []
    assert s["steps"] == 3 and s["samples"] == 21
    assert bool(torch.isnan(rec.log[3:]).all())      # the rows beyond `steps` are not read and still NaN


def test_nonfinite_steps_name_bad_gradients_and_bad_losses():
    ok = [1.0, 0.5, 0.5, 0.1, 0.1, 0.1, 0.2, 0.0]
    nan_loss = list(ok)
    nan_loss[0] = float("nan")
    inf_term = list(ok)
    inf_term[6] = float("inf")
    rec, _ = _record(False, steps=6)
    _log(rec, [(ok, 1.0, 0.0, 8, 1e-3), (ok, float("inf"), 2.0, 8, 1e-3), (nan_loss, 1.0, 0.0, 8, 1e-3), (ok, 2.0, 0.0, 8, 1e-3),
               (inf_term, 1.0, 0.0, 8, 1e-3), (ok, float("nan"), 1.0, 4, 1e-3)])
    s = rec.summary()
    assert s["nonfinite_steps"] == [1, 2, 4, 5]
    assert np.isnan(s["grad_norm_max"]) and np.isnan(s["grad_norm_last"])      # a NaN norm is not hidden by the maximum
    assert np.isnan(s["total"]) and s["mse_full"] == pytest.approx(0.5)
    # an epoch without grad_norm: column 8 NaN, column 9 zero -- no step is flagged for that
    rec2, _ = _record(False, steps=2)
    _log(rec2, [(ok, float("nan"), 0.0, 8, 1e-3), (ok, float("nan"), 0.0, 8, 1e-3)])
    s2 = rec2.summary()
    assert s2["nonfinite_steps"] == [] and np.isnan(s2["grad_norm_max"]) and s2["total"] == pytest.approx(1.0)


def test_fits_and_reset():
    rec, _ = _record(True, steps=5)
    _log(rec, [([1.0] * 8, 1.0, 0.0, 8, 1e-3)])
    assert rec.fits(N, 5, "cpu", True) and rec.fits(N, 3, "cpu", True)      # a shorter epoch fits a longer log
    assert not rec.fits(N, 6, "cpu", True) and not rec.fits(N, 5, "cpu", False) and not rec.fits(N + 1, 5, "cpu", True)
    assert not rec.fits(N, 5, "cpu", True, n_grads=100)                     # no scratch for a gradient reduce
    assert rec.scratch is None and rec.log.shape == (5, 12)
    assert rec.reset() is rec
    assert rec.steps == 0 and int(rec.seen.sum()) == 0 and bool(torch.isnan(rec.preds).all()) and bool(torch.isnan(rec.log).all())
    assert all(bool(torch.isnan(t).all()) for t in rec.embeddings.values())


def test_nothing_visited_and_nothing_recorded_are_errors_not_nans():
    from sdumc_amd import TrainRecord
    from sdumc_amd._lib import SdumcError
    rec = TrainRecord.empty(N, 3, "cpu").reset()
    with pytest.raises(SdumcError):
        rec.results(_store())
    with pytest.raises(SdumcError):
        rec.summary()


def test_a_wrong_out_is_refused_before_the_trainer_touches_anything():
    """FusedTrainer.train_epoch's host-side refusals, reached without a device: a repeated index, then an out= that is no record of
    this store -- both before the plan is uploaded (the stand-in store has no plan_epoch to call) and with `out` as it was"""
    from sdumc_amd import engine
    from sdumc_amd._lib import SdumcError
    tr = object.__new__(engine.FusedTrainer)
    tr.arena = types.SimpleNamespace(sets=[None, None])
    tr.params, tr.dims = torch.zeros(4), (64, 128, 64, 128)
    store = list(range(N))      # (len() is all the checks ask of the store)
    rec, _ = _record(False, steps=2)
    before = (rec.log.clone(), rec.preds.clone(), rec.seen.clone())
    for batches, out in (([[0, 1, 2], [3, 1]], rec),                      # index 1 twice
                         ([[0, 1, 2], [3, 4], [5]], rec),                  # three steps, a log of two rows
                         ([[0, 1, 2], [3, 4]], _record(True, 2)[0]),      # a record with embeddings for an epoch without
                         ([[0, 1, 2], [3, 4]], "not a record")):
        with pytest.raises(SdumcError):
            tr.train_epoch(store, batches, out=out)
    for t, b in zip((rec.log, rec.preds, rec.seen), before):
        assert torch.equal(torch.nan_to_num(t.float(), nan=-7.0), torch.nan_to_num(b.float(), nan=-7.0))


def test_record_entry_refuses_bad_arguments_without_a_device():
    """sdumc_epoch_record's SDUMC_EINVAL cases come back before any HIP call (the pointers here are never dereferenced)"""
    import ctypes as C
    from sdumc_amd import _lib

    def call(nseg=0, seg=(0x1000, 0x2000, 5, 64, 11), **kw):
        r = _lib.EpochRec()
        r.nseg, r.B, r.idx, r.losses, r.hyper, r.log_row = nseg, 5, 0x3000, 0x4000, 0x5000, 0x6000
        for k in range(max(0, min(nseg, _lib.SCATTER_MAX_SEGS))):
            r.seg[k].src, r.seg[k].dst, r.seg[k].rows, r.seg[k].cols, r.seg[k].dst_rows = seg
        for k, v in kw.items():
            setattr(r, k, v)
        return _lib.lib.sdumc_epoch_record(C.byref(r), None)

    bad = [_lib.lib.sdumc_epoch_record(None, None), call(log_row=None), call(losses=None), call(hyper=None), call(log_row=0x6002),
           call(nseg=-1), call(nseg=_lib.SCATTER_MAX_SEGS + 1), call(nseg=1, idx=None), call(nseg=1, B=0),
           call(grads=0x7000, n_grads=0, scratch=0x8000), call(grads=0x7000, n_grads=16, scratch=None),
           call(grads=0x7002, n_grads=16, scratch=0x8000), call(grads=0x7000, n_grads=16, scratch=0x8008)]
    for seg in ((None, 0x2000, 5, 64, 11), (0x1000, None, 5, 64, 11), (0x1000, 0x2000, 0, 64, 11), (0x1000, 0x2000, 5, 0, 11),
                (0x1000, 0x2000, 6, 64, 11), (0x1000, 0x2000, 5, 64, 0), (0x1002, 0x2000, 5, 64, 11)):
        bad.append(call(nseg=2, seg=seg))
    assert bad == [-1] * len(bad)
    sb = _lib.lib.sdumc_epoch_record_scratch_bytes
    assert sb(0) == 0 and sb(-5) == 0 and sb(1) >= 16 and sb(1) % 16 == 0 and sb(1) <= sb(4099) <= sb(1 << 22) == sb(1 << 23)
