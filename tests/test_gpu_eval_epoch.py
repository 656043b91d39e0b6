"""Evaluation epochs over a resident feature store (sdumc_amd/evaluate.py: eval_epoch, EvalResult; FusedTrainer.eval_epoch): the
validation / test passes of main_frame_val_text_missing.py:333-353 (:151-166 both streams in eval mode) as one enqueue-only loop --
sdumc_net_forward(train = 0) reading the store in place through row maps (or gathered copies), the next batch's assembly prefetched by
the forward, one sdumc_scatter_rows_multi launch per batch into store-ordered results.

The fixture: 37 synthetic utterances, frame maxima (40, 6, 24, 5), min_frac 0.25, batches of 8, 8, 8, 8, 5 in a shuffled order (every
batch padded to its own T, the last one short); widths (64, 128, 64, 128) in fp32 storage, (128, 128, 128, 128) in bf16 storage.
The per-batch references (engine.NetCall on store.batch's padded copies) are computed once per mode and shared."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_UTT, TCAP = 37, (40, 6, 24, 5)
DIMS = {"fp32": (64, 128, 64, 128), "bf16": (128, 128, 128, 128)}
NAMES = ("vals", "fused", "rnc", "text_hidden", "cross_text")
KEYS = ("audios", "texts", "videos", "feat4s")


def _batches(seed, sizes=(8, 8, 8, 8, 5), n=N_UTT):
    p = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    out, o = [], 0
    for b in sizes:
        out.append(p[o:o + b].clone())
        o += b
    return out


def _close(got, want, tol, msg=""):
    """the bar of tests/test_gpu_net.py's forward parity tests (its `close`)"""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    want = want.detach().cpu().double().numpy() if isinstance(want, torch.Tensor) else np.asarray(want, dtype=np.float64)
    scale = max(1.0, np.abs(want).max())
    np.testing.assert_allclose(got, want.reshape(got.shape), rtol=tol, atol=tol * scale, err_msg=msg)


class _Env:
    def __init__(self):
        from oracle import sdumc_oracle as O
        from sdumc_amd import engine, evaluate, _lib
        from sdumc_amd.data import DeviceFeatureStore
        self.O, self.engine, self.evaluate, self._lib = O, engine, evaluate, _lib
        self.P, self.flat, self.store = {}, {}, {}
        for mode, dims in DIMS.items():
            self.P[mode] = O.init_params(dims, seed=8)
            lay = engine.ParamLayout.get(*dims[:3])
            flat = torch.zeros(lay.total)
            for k, v in lay.views(flat).items():
                v.copy_(self.P[mode][k])
            self.flat[mode] = flat.cuda()
            self.store[mode] = DeviceFeatureStore.synthetic(N_UTT, TCAP, dims, seed=5, min_frac=0.25, bf16=mode == "bf16",
                                                            planes=mode == "fp32")
        self.batches = _batches(1)
        assert len({self.store["fp32"].batch_shape(ix) for ix in self.batches}) == len(self.batches)      # every batch its own padded T
        self._refs = {}

    def reference(self, mode, key_padding=False):
        """per batch: the five outputs of NetCall(train=False, planes=True) on the padded copies store.batch() makes (computed once)"""
        key = (mode, key_padding)
        if key not in self._refs:
            store, outs = self.store[mode], []
            for ix in self.batches:
                b = store.batch(ix)[0]
                lengths = [store.length[m][ix] for m in store.MODS] if key_padding else None
                call = self.engine.NetCall(self.flat[mode], b["audios"], [b["texts"], b["feat4s"]], b["videos"], False, None,
                                           planes=True, bf16=mode == "bf16", lengths=lengths)
                outs.append([t.clone() for t in call.forward()])
            torch.cuda.synchronize()
            self._refs[key] = outs
        return self._refs[key]

    def run(self, mode, batches=None, **kw):
        return self.evaluate.eval_epoch(self.flat[mode], DIMS[mode], self.store[mode], self.batches if batches is None else batches,
                                        bf16=mode == "bf16", **kw)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return _Env()


def _tensors(res):
    return [res.preds.unsqueeze(-1)] + [res.embeddings[n] for n in NAMES[1:]]


def _assert_equals_reference(res, refs, batches, what):
    visited = torch.cat(batches)
    for ix, ref in zip(batches, refs):
        B = ix.numel()
        for name, got, want in zip(NAMES, _tensors(res), ref):
            for s in range(2):
                assert torch.equal(got[s][ix.cuda()].reshape(B, -1), want[s * B:(s + 1) * B].reshape(B, -1)), (what, name, s)
    seen = torch.zeros(res.seen.numel(), dtype=torch.bool)
    seen[visited] = True
    assert torch.equal(res.seen.cpu() != 0, seen), what
    for t in _tensors(res):      # rows not visited hold NaN, visited rows are finite
        flat = t.reshape(2, t.shape[1], -1).cpu()
        assert bool(torch.isnan(flat[:, ~seen]).all()) and bool(torch.isfinite(flat[:, seen]).all()), what


@pytest.mark.parametrize("mode,inplace", [("fp32", True), ("fp32", False), ("bf16", True)])
def test_eval_epoch_bit_for_bit_against_the_forward_on_padded_copies(env, mode, inplace):
    """1. preds and the four embeddings of both streams, at rows idx, hold the bits engine.NetCall gives on store.batch(idx); seen is
    exactly the visited set (here: all 37; a 29-row subset epoch leaves the other rows NaN and unseen)."""
    res = env.run(mode, embeddings=True, inplace=inplace)
    torch.cuda.synchronize()
    ev = env.evaluate._evaluator[1]
    assert ev._in_place(env.store[mode]) == inplace and (ev.arena.sets[0].maps is not None) == inplace
    assert res.preds.shape == (2, N_UTT) and res.embeddings["cross_text"].shape == (2, N_UTT, 7, 128)
    _assert_equals_reference(res, env.reference(mode), env.batches, (mode, inplace))
    assert int((res.seen != 0).sum()) == N_UTT
    sub = env.run(mode, batches=env.batches[1:], embeddings=True, inplace=inplace)
    torch.cuda.synchronize()
    _assert_equals_reference(sub, env.reference(mode)[1:], env.batches[1:], (mode, inplace, "subset"))
    assert int((sub.seen != 0).sum()) == N_UTT - 8
    # without embeddings: the same predictions, two scatter segments
    plain = env.run(mode, inplace=inplace)
    torch.cuda.synchronize()
    assert plain.embeddings is None and torch.equal(plain.preds, res.preds) and torch.equal(plain.seen, res.seen)


def test_eval_epoch_against_the_cpu_oracle(env):
    """2. fp32 storage, in place (the gathered epoch holds the same bits by test 1): preds and embeddings against oracle.sdumc_oracle's
    eval forward of each padded batch at the output bar of tests/test_gpu_net.py's forward parity tests, 2e-5.  (bf16 storage rounds
    the features and projected frames to 8 bits of mantissa: no 2e-5 statement exists for it in the suite, and none is made here.)"""
    O = env.O
    res = env.run("fp32", embeddings=True)
    torch.cuda.synchronize()
    store, P = env.store["fp32"], {k: v.double() for k, v in env.P["fp32"].items()}
    for ix in env.batches:
        b = store.batch(ix)[0]
        audio, video = b["audios"].cpu().double(), b["videos"].cpu().double()
        for s, tk in enumerate(("texts", "feat4s")):
            y, (z, r, th, ct) = O.forward(P, audio, b[tk].cpu().double(), video, O.DropCtx("eval", 0, s))
            for name, got, want in zip(NAMES, _tensors(res), (y, z, r, th, ct)):
                _close(got[s][ix.cuda()].reshape(ix.numel(), -1), want.detach().reshape(ix.numel(), -1), 2e-5, f"{name} stream {s}")


@pytest.mark.parametrize("mode,inplace", [("fp32", True), ("fp32", False), ("bf16", True)])
def test_key_padding_reaches_the_poolings(env, mode, inplace):
    """3. key_padding=True equals NetCall(lengths = the batch's valid frame counts) bit for bit, and differs from the default on this
    ragged store."""
    res = env.run(mode, embeddings=True, key_padding=True, inplace=inplace)
    off = env.run(mode, embeddings=True, inplace=inplace)
    torch.cuda.synchronize()
    _assert_equals_reference(res, env.reference(mode, key_padding=True), env.batches, (mode, inplace, "key padding"))
    assert not torch.equal(res.preds, off.preds) and not torch.equal(res.embeddings["fused"], off.embeddings["fused"])


def test_training_is_untouched_by_evaluation_epochs(env):
    """4. two run_epoch calls with eval_epoch over a second store between and after them: parameters, Adam moments, hyper, the losses of
    every step and the dropout call counter are torch.equal to the run without evaluation (fp32, in place)."""
    from sdumc_amd.data import DeviceFeatureStore
    E, dims = env.engine, DIMS["fp32"]
    train_store = env.store["fp32"]
    eval_store = DeviceFeatureStore.synthetic(21, TCAP, dims, seed=9, min_frac=0.25, planes=True)
    eval_batches = _batches(4, sizes=(8, 8, 5), n=21)
    runs = []
    for with_eval in (False, True):
        flat = env.flat["fp32"].clone()
        tr = E.FusedTrainer(flat, dims, lr=1e-3, seed=11, capacity=(8, TCAP))
        plan = train_store.plan_epoch(env.batches)
        ls, evals = [], []
        for _ in range(2):
            tr.run_epoch(train_store, plan, on_step=lambda i, l: ls.append(l.clone()))
            if with_eval:
                evals.append(tr.eval_epoch(eval_store, eval_batches, embeddings=True))
        torch.cuda.synchronize()
        assert tr._in_place(train_store)
        runs.append((flat, tr.state.adam_m, tr.state.adam_v, tr.state.hyper, ls, tr.state.rng.call))
        if with_eval:      # the evaluations themselves ran: all rows seen, finite, and the second one saw the updated parameters
            for r in evals:
                assert int((r.seen != 0).sum()) == 21 and bool(torch.isfinite(r.preds).all())
            assert not torch.equal(evals[0].preds, evals[1].preds)
            assert tr._evaluator.arena.workspace.data_ptr() != tr.arena.workspace.data_ptr()
    a, b = runs
    for x, y, what in zip(a[:4], b[:4], ("parameters", "adam_m", "adam_v", "hyper")):
        assert torch.equal(x, y), what
    assert len(a[4]) == len(b[4]) == 10 and all(torch.equal(x, y) for x, y in zip(a[4], b[4]))
    assert a[5] == b[5] == 20
    assert not torch.equal(a[0], env.flat["fp32"])      # (the run trained)


def test_a_second_epoch_reuses_the_result_and_the_arena_grows(env):
    """5. out=first over another plan of the same store: the same tensors, seen and the NaN fill reset, the bits of a fresh call; a later
    plan with a larger B than any before runs (the arena grows) and still equals the per-batch forward."""
    first = env.run("fp32", embeddings=True)
    ptrs = [t.data_ptr() for t in _tensors(first)] + [first.seen.data_ptr()]
    other = _batches(2)[:3]      # another order, 24 of the 37 rows
    again = env.run("fp32", batches=other, embeddings=True, out=first)
    assert again is first and [t.data_ptr() for t in _tensors(first)] + [first.seen.data_ptr()] == ptrs
    fresh = env.run("fp32", batches=other, embeddings=True)
    torch.cuda.synchronize()
    assert int((first.seen != 0).sum()) == 24 and torch.equal(first.seen, fresh.seen)
    for x, y in zip(_tensors(first), _tensors(fresh)):
        assert torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))
    assert bool(torch.isnan(first.preds[:, first.seen == 0]).all())
    ev = env.evaluate._evaluator[1]
    arena, b_before = ev.arena, ev.arena.B
    big = _batches(6, sizes=(13, 11, 13))
    res = env.run("fp32", batches=big, embeddings=True)
    torch.cuda.synchronize()
    assert b_before == 8 and ev.arena is not arena and ev.arena.B == 13
    store = env.store["fp32"]
    for ix in big:
        b = store.batch(ix)[0]
        ref = env.engine.NetCall(env.flat["fp32"], b["audios"], [b["texts"], b["feat4s"]], b["videos"], False, None, planes=True).forward()
        for got, want in zip(_tensors(res), ref):
            for s in range(2):
                assert torch.equal(got[s][ix.cuda()].reshape(ix.numel(), -1), want[s * ix.numel():(s + 1) * ix.numel()].reshape(ix.numel(), -1))


def test_refusals_come_before_any_launch(env):
    """6. a duplicate index within the epoch, an empty batch list, an index out of range: SdumcError, and the out= result's tensors are
    what they were (nothing ran, not even the NaN fill)."""
    SdumcError = env._lib.SdumcError
    out = env.run("fp32", embeddings=True)
    torch.cuda.synchronize()
    before = [t.clone() for t in _tensors(out)] + [out.seen.clone()]
    dup = [b.clone() for b in env.batches]
    dup[3][2] = dup[0][5]
    oor = [b.clone() for b in env.batches]
    oor[1][0] = N_UTT
    for bad in (dup, [], oor, [env.batches[0], torch.zeros(0, dtype=torch.int64)]):
        with pytest.raises(SdumcError):
            env.run("fp32", batches=bad, embeddings=True, out=out)
    with pytest.raises(SdumcError):      # a result without embeddings cannot take an epoch that collects them
        env.run("fp32", embeddings=True, out=env.evaluate.EvalResult.empty(N_UTT, "cuda", False))
    with pytest.raises(SdumcError):      # a plan made for a larger store names rows this one does not have
        from sdumc_amd.data import DeviceFeatureStore
        bigger = DeviceFeatureStore.synthetic(N_UTT + 3, TCAP, DIMS["fp32"], seed=5, planes=True)
        env.run("fp32", batches=bigger.plan_epoch([torch.arange(N_UTT - 2, N_UTT + 3)]), embeddings=True, out=out)
    torch.cuda.synchronize()
    for t, b in zip(_tensors(out) + [out.seen], before):
        assert torch.equal(t, b)


def test_results_dictionary_matches_the_module_route(env):
    """7. results(store): keys and array shapes of checkpoint.run_inference on model.get_models over the same batches; values at the bar
    of test 2 (the module route runs single-stream plans with the in-kernel split: other bits); the MSE entries are the numpy means."""
    from sdumc_amd.checkpoint import run_inference
    from sdumc_amd.model import get_models
    store, dims = env.store["fp32"], DIMS["fp32"]
    model = get_models(types.SimpleNamespace(input_dims=dims, model="wengnet_mosei_mult_views_text_missing"))
    model.load_state_dict({"model." + k: v for k, v in env.P["fp32"].items()})
    model = model.cuda()
    want = run_inference(model, [store.batch(ix) for ix in env.batches])
    res = env.run("fp32", embeddings=True)
    got = res.results(store)
    assert set(got) == set(want) | {"val_mse_full"}
    order = np.argsort(torch.cat(env.batches).numpy(), kind="stable")      # the module route is in visiting order, the results in store order
    assert got["names"] == store.names and [want["names"][i] for i in order] == got["names"]
    for k, w in want.items():
        if isinstance(w, np.ndarray):
            assert got[k].shape == w.shape and got[k].dtype == w.dtype, k
            _close(got[k], w[order], 2e-5, k)
    lab = got["val_labels"].reshape(-1)
    assert np.array_equal(lab, store.vals.cpu().numpy())
    assert got["val_mse"] == got["val_mse_full"] == float(np.mean((lab - got["val_preds_full"].reshape(-1)) ** 2))
    assert got["val_mse_missing"] == float(np.mean((lab - got["val_preds_missing"].reshape(-1)) ** 2))
    m = res.metrics(store)
    assert set(m) == {"full", "missing"} and m["full"]["n"] == N_UTT and abs(m["full"]["mse"] - got["val_mse"]) < 1e-6
    # predictions only: no embedding keys
    assert set(env.run("fp32").results(store)) == {"val_preds_full", "val_preds_missing", "val_labels", "names", "val_mse",
                                                   "val_mse_full", "val_mse_missing"}
