"""The record of a training epoch (FusedTrainer.train_epoch -> record.TrainRecord; one sdumc_epoch_record call per step,
csrc/epoch_record.hip): the step's train-mode outputs in store order, its loss vector, batch size and learning rate in a log row, the
L2 norm and the non-finite count of its raw gradient bucket -- read-only towards the training run.

The fixture is the one of tests/test_gpu_eval_epoch.py: 37 synthetic utterances, frame maxima (40, 6, 24, 5), min_frac 0.25, batches of
8, 8, 8, 8, 5 in a shuffled order; widths (64, 128, 64, 128) in fp32 storage (a store with planes), (128, 128, 128, 128) in bf16 storage;
FusedTrainer(..., lr=1e-3, seed=11, capacity=(8, TCAP)).  The reference runs (run_epoch with on_step clones) are made once per mode.

The gradient-norm bar (tests 3 and 4) is derived, not measured: the kernel accumulates n < 2^24 non-negative fp64 terms, which is off
by at most n 2^-53 relative -- far below half an fp32 ulp -- and rounds once to fp32, as torch.linalg.vector_norm(x.double()).float()
does; the two can differ only where the exact value sits on a rounding boundary: one fp32 ulp, relative 2^-23.
A bucket whose norm is beyond the fp32 range (4099 elements of 3e38: 1.9e40, finite in fp64) comes out as +Inf -- the one rounding to
fp32 -- which include/sdumc_hip.h states and test 4 asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_UTT, TCAP = 37, (40, 6, 24, 5)
DIMS = {"fp32": (64, 128, 64, 128), "bf16": (128, 128, 128, 128)}
NAMES = ("vals", "fused", "rnc", "text_hidden", "cross_text")
WIDTHS = (1, 128, 64, 256, 7 * 128)
ULP = 2.0 ** -23
ROUTES = [("fp32", True), ("fp32", False), ("bf16", True)]


def _batches(seed, sizes=(8, 8, 8, 8, 5), n=N_UTT):
    p = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    out, o = [], 0
    for b in sizes:
        out.append(p[o:o + b].clone())
        o += b
    return out


class _Env:
    def __init__(self):
        from oracle import sdumc_oracle as O
        from sdumc_amd import engine, record, _lib
        from sdumc_amd.data import DeviceFeatureStore
        self.engine, self.record, self._lib = engine, record, _lib
        self.flat, self.store = {}, {}
        for mode, dims in DIMS.items():
            P = O.init_params(dims, seed=8)
            lay = engine.ParamLayout.get(*dims[:3])
            flat = torch.zeros(lay.total)
            for k, v in lay.views(flat).items():
                v.copy_(P[k])
            self.flat[mode] = flat.cuda()
            self.store[mode] = DeviceFeatureStore.synthetic(N_UTT, TCAP, dims, seed=5, min_frac=0.25, bf16=mode == "bf16",
                                                            planes=mode == "fp32")
        self.batches = _batches(1)
        self._runs = {}

    def trainer(self, mode, inplace=True):
        kw = {"bf16": True} if mode == "bf16" else {}
        tr = self.engine.FusedTrainer(self.flat[mode].clone(), DIMS[mode], lr=1e-3, seed=11, capacity=(8, TCAP), inplace=inplace, **kw)
        return tr

    def runs(self, mode, inplace):
        """once per route: (the per-step clones of a run_epoch reference -- losses and the arena's five outs[:2 B w] --, the record of
        train_epoch(embeddings=True, grad_norm=True) on a second trainer from the same parameters and seed, that trainer)"""
        key = (mode, inplace)
        if key not in self._runs:
            store, ref = self.store[mode], []
            a = self.trainer(mode, inplace)

            def keep(i, l):
                B = self.batches[i].numel()
                ref.append((l.clone(), [o[:2 * B * w].clone() for o, w in zip(a.arena.outs, WIDTHS)]))
            assert a.run_epoch(store, self.batches, on_step=keep) == len(self.batches)
            b = self.trainer(mode, inplace)
            rec = b.train_epoch(store, self.batches, embeddings=True, grad_norm=True)
            torch.cuda.synchronize()
            assert a._in_place(store) == b._in_place(store) == inplace
            self._runs[key] = (ref, rec, b)
        return self._runs[key]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return _Env()


def _tensors(rec):
    return [rec.preds.unsqueeze(-1)] + [rec.embeddings[n] for n in NAMES[1:]]


def _same(x, y):
    """bit equality with NaN == NaN"""
    return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))


def _assert_record_equals_clones(rec, ref, batches, what):
    assert rec.steps == len(batches) == len(ref), what
    lr = torch.tensor(1e-3, dtype=torch.float32)
    for i, (ix, (losses, outs)) in enumerate(zip(batches, ref)):
        B = ix.numel()
        assert torch.equal(rec.log[i, 0:8], losses), (what, "losses", i)
        assert float(rec.log[i, 10]) == B and torch.equal(rec.log[i, 11].cpu(), lr), (what, "B / lr", i)
        for name, got, want in zip(NAMES, _tensors(rec), outs):
            for s in range(2):
                assert torch.equal(got[s][ix.cuda()].reshape(B, -1), want.reshape(2 * B, -1)[s * B:(s + 1) * B]), (what, name, s, i)
    seen = torch.zeros(N_UTT, dtype=torch.bool)
    seen[torch.cat(batches)] = True
    assert torch.equal(rec.seen.cpu() != 0, seen), what
    for t in _tensors(rec):      # rows not visited hold NaN, visited rows are finite
        flat = t.reshape(2, N_UTT, -1).cpu()
        assert bool(torch.isnan(flat[:, ~seen]).all()) and bool(torch.isfinite(flat[:, seen]).all()), what
    assert bool(torch.isnan(rec.log[rec.steps:]).all()) and bool(torch.isfinite(rec.log[:rec.steps]).all()), what


@pytest.mark.parametrize("mode,inplace", ROUTES)
def test_record_holds_the_bits_the_steps_left(env, mode, inplace):
    """1. log[i, 0:8] = the losses run_epoch's step i wrote, preds / embeddings at rows idx = rows [s B, (s + 1) B) of the arena's outputs
    after step i, log[i, 10] = B_i, log[i, 11] = 1e-3, seen = the visited set -- bit for bit; then a 29-row subset epoch into the same
    record: the other rows NaN and unseen, the log row beyond `steps` NaN."""
    ref, rec, tr = env.runs(mode, inplace)
    assert rec.preds.shape == (2, N_UTT) and rec.embeddings["cross_text"].shape == (2, N_UTT, 7, 128) and rec.log.shape == (5, 12)
    _assert_record_equals_clones(rec, ref, env.batches, (mode, inplace))
    assert int((rec.seen != 0).sum()) == N_UTT
    # a second epoch of the reference run and of the recorded run over batches[1:]: 4 steps into the 5-row record
    a, store, ref2 = env.trainer(mode, inplace), env.store[mode], []
    a.run_epoch(store, env.batches)

    def keep(i, l):
        B = env.batches[1 + i].numel()
        ref2.append((l.clone(), [o[:2 * B * w].clone() for o, w in zip(a.arena.outs, WIDTHS)]))
    a.run_epoch(store, env.batches[1:], on_step=keep)
    sub = tr.train_epoch(store, env.batches[1:], embeddings=True, grad_norm=True, out=rec)
    torch.cuda.synchronize()
    try:
        assert sub is rec and rec.steps == 4 and int((rec.seen != 0).sum()) == N_UTT - 8
        _assert_record_equals_clones(rec, ref2, env.batches[1:], (mode, inplace, "subset"))
    finally:
        env._runs.pop((mode, inplace))      # (the shared record now holds the subset epoch: the next user makes its own)


def test_training_is_untouched_by_the_record(env):
    """2. two epochs: parameters, both Adam moments, hyper and the dropout call counter are torch.equal between run_epoch and
    train_epoch(embeddings=True, grad_norm=True) (fp32, in place)."""
    store, runs = env.store["fp32"], []
    for recorded in (False, True):
        tr = env.trainer("fp32")
        plan = store.plan_epoch(env.batches)
        for _ in range(2):
            if recorded:
                rec = tr.train_epoch(store, plan, embeddings=True, grad_norm=True)
            else:
                assert tr.run_epoch(store, plan) == 5
        torch.cuda.synchronize()
        runs.append((tr.params, tr.state.adam_m, tr.state.adam_v, tr.state.hyper, tr.state.rng.call))
    a, b = runs
    for x, y, what in zip(a[:4], b[:4], ("parameters", "adam_m", "adam_v", "hyper")):
        assert torch.equal(x, y), what
    assert a[4] == b[4] == 20
    assert not torch.equal(a[0], env.flat["fp32"]) and float(a[3][1]) == 10.0      # (the run trained: ten Adam steps)
    assert rec.steps == 5 and int((rec.seen != 0).sum()) == N_UTT and bool(torch.isfinite(rec.log).all())


def test_gradient_norm_of_every_step(env):
    """3. log[i, 8] against torch.linalg.vector_norm(bucket.double()).float() of the bucket cloned in on_step: within one fp32 ulp
    (the module docstring derives the bar); log[i, 9] == 0."""
    tr, store, buckets = env.trainer("fp32"), env.store["fp32"], []
    rec = tr.train_epoch(store, env.batches, grad_norm=True, on_step=lambda i, l: buckets.append(next(iter(tr._steps.values())).grads.clone()))
    torch.cuda.synchronize()
    live = env.engine.ParamLayout.get(*DIMS["fp32"][:3]).live
    assert rec.embeddings is None and len(buckets) == 5 and buckets[0].numel() == live and rec.n_grads == live
    for i, g in enumerate(buckets):
        want = float(torch.linalg.vector_norm(g.double()).float())
        got = float(rec.log[i, 8])
        print(f"step {i}: grad_norm {got!r} reference {want!r} rel {abs(got - want) / want:.3e}")
        assert want > 0 and abs(got - want) <= ULP * want, i
        assert float(rec.log[i, 9]) == 0.0, i
    assert not torch.equal(buckets[0], buckets[1])
    s = rec.summary()
    assert s["grad_norm_max"] == float(rec.log[:, 8].max()) and s["grad_norm_last"] == float(rec.log[4, 8]) and s["nonfinite_steps"] == []


def _entry(env, log_row, losses, hyper, grads=None, n=0, scratch=None, B=0):
    r = env._lib.EpochRec()
    r.nseg, r.B, r.losses, r.hyper, r.log_row = 0, B, losses.data_ptr(), hyper.data_ptr(), log_row.data_ptr()
    if grads is not None:
        r.grads, r.n_grads, r.scratch = grads.data_ptr(), n, scratch.data_ptr()
    return env._lib.lib.sdumc_epoch_record(C.byref(r), env._lib.current_stream())


def test_the_entry_alone_on_buffers_of_many_sizes(env):
    """4. nseg = 0, buffers the test owns: n = 1, 3, 255, 256, 257, 4099, 1 048 579 from an aligned base and from one 4 bytes further,
    N(0, 1) * 1e-3 -- the ulp bar of test 3, two launches the same bits; 4099 elements of 3e38 -> +Inf (the norm, 1.9e40, is finite in
    fp64 and beyond fp32: one rounding); a NaN, a +Inf and a -Inf at the first, a middle and the last element -> count 3, norm
    non-finite; ONE scratch serves all of these calls."""
    lib = env._lib.lib
    sizes = (1, 3, 255, 256, 257, 4099, 1048579)
    g = torch.Generator(device="cuda").manual_seed(4)
    big = torch.randn(max(sizes) + 1, device="cuda", generator=g) * 1e-3
    scratch = torch.zeros(lib.sdumc_epoch_record_scratch_bytes(max(sizes)), dtype=torch.uint8, device="cuda")
    losses = torch.arange(8, device="cuda", dtype=torch.float32) + 0.5
    hyper = torch.tensor([3e-4, 7.0, 0.0, 0.0], device="cuda")
    cases = [(n, off, big[off:off + n]) for n in sizes for off in (0, 1)]
    huge = torch.full((4099,), 3e38, device="cuda")
    bad = big[:4099].clone()
    bad[0], bad[2000], bad[4098] = float("nan"), float("inf"), float("-inf")
    cases += [(4099, "3e38", huge), (4099, "nan/inf", bad), (4099, "after", big[:4099])]      # (the last: the scratch is still ready)
    log = torch.full((2, len(cases), 12), -7.0, device="cuda")
    for rep in range(2):
        for k, (n, off, x) in enumerate(cases):
            assert x.data_ptr() % 16 == (4 if off == 1 else 0)
            assert _entry(env, log[rep, k], losses, hyper, x, n, scratch, B=k) == 0
    torch.cuda.synchronize()
    assert torch.equal(torch.nan_to_num(log[0], nan=-1.0), torch.nan_to_num(log[1], nan=-1.0)) and torch.equal(torch.isnan(log[0]), torch.isnan(log[1]))
    rows = log[0].cpu()
    for k, (n, what, x) in enumerate(cases):
        row = rows[k]
        assert torch.equal(row[0:8], losses.cpu()) and float(row[10]) == k and torch.equal(row[11], hyper[0].cpu()), (n, what)
        if what in ("3e38", "nan/inf"):
            continue
        want = float(torch.linalg.vector_norm(x.double()).float())
        got = float(row[8])
        print(f"n {n} offset {what}: norm {got!r} reference {want!r} rel {abs(got - want) / want:.3e}")
        assert want > 0 and abs(got - want) <= ULP * want, (n, what)
        assert float(row[9]) == 0.0, (n, what)
    k = len(cases) - 3
    ref64 = float(torch.linalg.vector_norm(huge.double()))
    assert np.isfinite(ref64) and ref64 > 3.4028235e38 and float(rows[k][8]) == float("inf") and float(rows[k][9]) == 0.0
    assert float(torch.linalg.vector_norm(huge.double()).float()) == float("inf")
    assert float(rows[k + 1][9]) == 3.0 and not np.isfinite(float(rows[k + 1][8]))
    # without a bucket: NaN and 0, the rest of the row as before
    plain = torch.full((12,), -7.0, device="cuda")
    assert _entry(env, plain, losses, hyper, B=6) == 0
    torch.cuda.synchronize()
    assert torch.equal(plain[0:8], losses) and bool(torch.isnan(plain[8])) and plain[9:].tolist() == [0.0, 6.0, float(hyper[0])]


def test_a_record_is_reused_across_epochs_and_refusals_come_first(env):
    """5. out= over two epochs with different plans (5 steps, then 3): the same tensors, reset, and the bits of a fresh record; a record
    that does not fit raises before anything is enqueued; a plan with a repeated index raises and leaves `out` untouched."""
    SdumcError, store = env._lib.SdumcError, env.store["fp32"]
    other = _batches(2)[:3]
    a, b = env.trainer("fp32"), env.trainer("fp32")
    first = a.train_epoch(store, env.batches, embeddings=True, grad_norm=True)
    ptrs = [t.data_ptr() for t in _tensors(first) + [first.seen, first.log, first.scratch]]
    again = a.train_epoch(store, other, embeddings=True, grad_norm=True, out=first)
    b.train_epoch(store, env.batches, embeddings=True, grad_norm=True)
    fresh = b.train_epoch(store, other, embeddings=True, grad_norm=True)
    torch.cuda.synchronize()
    assert again is first and [t.data_ptr() for t in _tensors(first) + [first.seen, first.log, first.scratch]] == ptrs
    assert first.steps == fresh.steps == 3 and first.log.shape == (5, 12) and fresh.log.shape == (3, 12)
    assert torch.equal(first.log[:3], fresh.log) and bool(torch.isnan(first.log[3:]).all()) and bool(torch.isfinite(fresh.log).all())
    assert int((first.seen != 0).sum()) == 24 and torch.equal(first.seen, fresh.seen)
    for x, y in zip(_tensors(first), _tensors(fresh)):
        assert _same(x, y)
    assert bool(torch.isnan(first.preds[:, first.seen == 0]).all())
    # refusals: nothing runs -- the record, the step count and the dropout counter are what they were
    before = [t.clone() for t in _tensors(first) + [first.seen, first.log]]
    state = (float(a.state.hyper[1]), a.state.rng.call)
    dup = [x.clone() for x in env.batches]
    dup[3][2] = dup[0][5]
    with pytest.raises(SdumcError):
        a.train_epoch(store, dup, embeddings=True, grad_norm=True, out=first)
    with pytest.raises(SdumcError):      # a record without embeddings cannot take an epoch that keeps them
        a.train_epoch(store, other, embeddings=True, out=env.record.TrainRecord.empty(N_UTT, 3, "cuda"))
    with pytest.raises(SdumcError):      # ... nor one without the reduce's scratch an epoch with grad_norm
        a.train_epoch(store, other, grad_norm=True, out=env.record.TrainRecord.empty(N_UTT, 3, "cuda"))
    with pytest.raises(SdumcError):      # ... nor a log of 5 rows an epoch of 6 steps
        a.train_epoch(store, _batches(3, sizes=(6, 6, 6, 6, 6, 7)), embeddings=True, grad_norm=True, out=first)
    torch.cuda.synchronize()
    for t, w in zip(_tensors(first) + [first.seen, first.log], before):
        assert _same(t.float(), w.float())
    assert (float(a.state.hyper[1]), a.state.rng.call) == state and first.steps == 3


def test_summary_and_results_agree_on_the_mse(env):
    """6. the B-weighted mse_full / mse_missing of summary() against results()'s val_mse_full / val_mse_missing, rtol 1e-6: both are fp32
    roundings of fp64 sums over the same vals (1e-6 = 16 roundings of 2^-24)."""
    _, rec, _ = env.runs("fp32", True)
    s, r = rec.summary(), rec.results(env.store["fp32"])
    assert r["names"] == env.store["fp32"].names and r["val_preds_full"].shape == (N_UTT, 1) and "full_rep" in r
    for a, b in (("mse_full", "val_mse_full"), ("mse_missing", "val_mse_missing")):
        print(f"{a} {s[a]!r} {b} {r[b]!r} rel {abs(s[a] - r[b]) / r[b]:.3e}")
        np.testing.assert_allclose(s[a], r[b], rtol=1e-6)
    assert s["steps"] == 5 and s["samples"] == N_UTT and s["nonfinite_steps"] == []


def test_refused_arguments_launch_nothing(env):
    """7. SDUMC_EINVAL for each rejected argument, and the poisoned log row stays poisoned."""
    lib, EpochRec = env._lib.lib, env._lib.EpochRec
    B, n = 5, 11
    src, dst = torch.randn(2 * B, 64, device="cuda"), torch.full((n, 64), -7.0, device="cuda")
    idx = torch.arange(B, device="cuda")
    losses, hyper = torch.zeros(8, device="cuda"), torch.zeros(4, device="cuda")
    grads, scratch = torch.ones(64, device="cuda"), torch.zeros(lib.sdumc_epoch_record_scratch_bytes(64), dtype=torch.uint8, device="cuda")
    log = torch.full((12,), -7.0, device="cuda")

    def call(seg=None, **kw):
        r = EpochRec()
        r.nseg, r.B, r.idx = 1, B, idx.data_ptr()
        r.losses, r.hyper, r.log_row = losses.data_ptr(), hyper.data_ptr(), log.data_ptr()
        r.grads, r.n_grads, r.scratch = grads.data_ptr(), 64, scratch.data_ptr()
        good = (src.data_ptr(), dst.data_ptr(), B, 64, n)
        for k in range(2):
            sg = r.seg[k]
            sg.src, sg.dst, sg.rows, sg.cols, sg.dst_rows = good if (seg is None or k == 0) else seg
        for k, v in kw.items():
            setattr(r, k, v)
        return lib.sdumc_epoch_record(C.byref(r), env._lib.current_stream())

    s, d = src.data_ptr(), dst.data_ptr()
    bad = {"log_row NULL": call(log_row=None), "losses NULL": call(losses=None), "hyper NULL": call(hyper=None),
           "nseg < 0": call(nseg=-1), "nseg > max": call(nseg=env._lib.SCATTER_MAX_SEGS + 1), "idx NULL": call(idx=None),
           "B < 1": call(B=0), "n_grads < 1": call(n_grads=0), "scratch NULL": call(scratch=None),
           "desc NULL": lib.sdumc_epoch_record(None, env._lib.current_stream())}
    for what, seg in (("src NULL", (None, d, B, 64, n)), ("dst NULL", (s, None, B, 64, n)), ("rows < 1", (s, d, 0, 64, n)),
                      ("cols < 1", (s, d, B, 0, n)), ("rows % B", (s, d, B + 1, 64, n)), ("dst_rows < 1", (s, d, B, 64, 0)),
                      ("misaligned", (s + 2, d, B, 64, n))):
        bad[what] = call(seg=seg, nseg=2)
    torch.cuda.synchronize()
    assert all(rc == -1 for rc in bad.values()), bad
    assert bool((log == -7.0).all()) and bool((dst == -7.0).all()) and int(scratch.sum()) == 0
    assert call() == 0      # (the same descriptor with nothing wrong runs: one segment, the log row, the norm of 64 ones)
    torch.cuda.synchronize()
    assert torch.equal(dst[:B], src[:B]) and bool((dst[B:] == -7.0).all()) and float(log[8]) == 8.0 and float(log[10]) == B
