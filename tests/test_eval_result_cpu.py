"""Host side of the evaluation epoch (sdumc_amd/evaluate.py), no GPU: EvalResult built from CPU tensors -- results() is the dictionary
of checkpoint.run_inference (main_frame_val_text_missing_inference.py:166-215) over the visited rows in store order, metrics() is
metric.eval_mosei_metric of the same vectors (main :366-367) -- and the epoch's index check."""
import types

import numpy as np
import pytest
import torch

N = 9
EMB_KEYS = {"fused": ("full_rep", "missing_rep", (128,)), "rnc": ("full_rnc", "missing_rnc", (64,)),
            "text_hidden": ("text_rep_query_full", "text_rep_query_missing", (256,)),
            "cross_text": ("text_rep_full", "text_rep_missing", (7, 128))}


def _store():
    g = torch.Generator().manual_seed(0)
    vals = torch.round((torch.rand(N, generator=g) * 6 - 3) * 10) / 10
    vals[4] = 0.0      # (a zero label: left out of acc2 / f1)
    return types.SimpleNamespace(names=[f"utt{i:03d}" for i in range(N)], vals=vals)


def _result(embeddings):
    from sdumc_amd import EvalResult
    g = torch.Generator().manual_seed(1)
    visited = [7, 1, 4, 2, 8]      # a partial epoch, in sampler order
    res = EvalResult.empty(N, "cpu", embeddings=embeddings).reset()
    res.seen[visited] = 1
    res.preds[:, visited] = torch.randn(2, len(visited), generator=g)
    for t in (res.embeddings or {}).values():
        t[:, visited] = torch.randn((2, len(visited)) + tuple(t.shape[2:]), generator=g)
    return res, sorted(visited)


def test_package_exports():
    import sdumc_amd
    from sdumc_amd import evaluate
    assert sdumc_amd.eval_epoch is evaluate.eval_epoch and sdumc_amd.EvalResult is evaluate.EvalResult
    with pytest.raises(AttributeError):
        sdumc_amd.no_such_name


@pytest.mark.parametrize("embeddings", [False, True])
def test_results_keeps_the_visited_rows_in_store_order(embeddings):
    res, rows = _result(embeddings)
    store = _store()
    assert bool(torch.isnan(res.preds[:, [0, 3, 5, 6]]).all())      # rows not visited hold NaN
    out = res.results(store)
    assert out["names"] == [store.names[i] for i in rows]
    lab = store.vals.numpy()[rows]
    assert np.array_equal(out["val_labels"], lab) and out["val_labels"].shape == (5,)
    for s, k in enumerate(("val_preds_full", "val_preds_missing")):
        assert out[k].shape == (5, 1) and out[k].dtype == np.float32
        assert np.array_equal(out[k].reshape(-1), res.preds[s].numpy()[rows])
    assert out["val_mse"] == out["val_mse_full"] == float(np.mean((lab - res.preds[0].numpy()[rows]) ** 2))
    assert out["val_mse_missing"] == float(np.mean((lab - res.preds[1].numpy()[rows]) ** 2))
    base = {"val_preds_full", "val_preds_missing", "val_labels", "names", "val_mse", "val_mse_full", "val_mse_missing"}
    if not embeddings:
        assert set(out) == base
        return
    assert set(out) == base | {k for v in EMB_KEYS.values() for k in v[:2]}
    for name, (kf, km, shape) in EMB_KEYS.items():
        for s, k in enumerate((kf, km)):
            assert out[k].shape == (5,) + shape
            assert np.array_equal(out[k], res.embeddings[name][s].numpy()[rows])


def test_metrics_equal_eval_mosei_metric_on_the_same_vectors():
    from sdumc_amd.metric import eval_mosei_metric
    res, rows = _result(False)
    store = _store()
    m = res.metrics(store)
    lab = store.vals.numpy()[rows]
    assert m == {"full": eval_mosei_metric(res.preds[0].numpy()[rows], lab), "missing": eval_mosei_metric(res.preds[1].numpy()[rows], lab)}
    assert m["full"]["n"] == 5 and np.isfinite(list(m["full"].values())).all()


def test_nothing_visited_is_an_error_not_a_nan():
    from sdumc_amd import EvalResult
    from sdumc_amd._lib import SdumcError
    res = EvalResult.empty(N, "cpu").reset()
    with pytest.raises(SdumcError):
        res.results(_store())
    with pytest.raises(SdumcError):
        res.metrics(_store())


def test_reset_clears_a_reused_result():
    res, _ = _result(True)
    assert res.fits(N, "cpu", True) and not res.fits(N, "cpu", False) and not res.fits(N + 1, "cpu", True)
    res.reset()
    assert int(res.seen.sum()) == 0 and bool(torch.isnan(res.preds).all())
    assert all(bool(torch.isnan(t).all()) for t in res.embeddings.values())


def test_epoch_index_check_runs_on_the_host():
    from sdumc_amd.evaluate import check_epoch_indices
    from sdumc_amd._lib import SdumcError
    ok = check_epoch_indices([[3, 1, 2], torch.tensor([0, 8]), np.array([5])], N)
    assert ok.tolist() == [3, 1, 2, 0, 8, 5] and ok.dtype == torch.int64
    for bad in ([[3, 1], [2, 3]],            # twice, across batches
                [[4, 4]],                    # twice, within one batch
                [[0, N]], [[-1, 2]],         # out of range
                [], [[1], []]):              # no batches, an empty batch
        with pytest.raises(SdumcError):
            check_epoch_indices(bad, N)


def test_scatter_entry_refuses_bad_arguments_without_a_device():
    """sdumc_scatter_rows_multi's SDUMC_EINVAL cases come back before any HIP call (the pointers here are never dereferenced)"""
    from sdumc_amd import _lib

    def call(segs, n=None, idx=0x1000, b=5):
        arr = (_lib.ScatterSeg * max(1, len(segs)))()
        for a, s in zip(arr, segs):
            a.src, a.dst, a.rows, a.cols, a.dst_rows = s
        return _lib.lib.sdumc_scatter_rows_multi(arr, len(segs) if n is None else n, idx, b, None, None)

    good = (0x1000, 0x2000, 5, 64, 11)
    assert _lib.SCATTER_MAX_SEGS >= 10
    bad = [call([good], n=0), call([good] * (_lib.SCATTER_MAX_SEGS + 1)), call([good], idx=None), call([good], b=0),
           _lib.lib.sdumc_scatter_rows_multi(None, 1, 0x1000, 5, None, None)]
    for seg in ((None, 0x2000, 5, 64, 11), (0x1000, None, 5, 64, 11), (0x1000, 0x2000, 0, 64, 11), (0x1000, 0x2000, 5, 0, 11),
                (0x1000, 0x2000, 6, 64, 11), (0x1000, 0x2000, 5, 64, 0), (0x1002, 0x2000, 5, 64, 11)):
        bad.append(call([good, seg]))
    assert bad == [-1] * len(bad)
