"""The training record by tensor (sdumc_tensor_norms, csrc/tensor_norms.hip; FusedTrainer.train_epoch(by_tensor=True | 'updates') ->
record.TensorNorms; record.tensor_norms for a loop that keeps per-parameter .grad tensors): per tensor and step the L2 norm and the
non-finite count of the raw gradient, the weight norm after the step and the norm of the step's actual update -- read-only towards
the training run.

The bar is the one of tests/test_gpu_epoch_record.py, by the same argument: the kernel accumulates n < 2^24 non-negative fp64 terms
(squares of fp32 values, or of fp32 differences taken exactly in fp64) in a fixed order, which is off by at most n 2^-53 relative --
far below half an fp32 ulp -- and rounds once to fp32, as torch.linalg.vector_norm(x.double()).float() does; the two can differ only
where the exact value sits on a rounding boundary: one fp32 ulp, relative 2^-23.

Epoch fixtures: 33 synthetic utterances, frame maxima (40, 6, 24, 5), min_frac 0.25, ragged batches of 7, 6, 7, 6, 7 in a shuffled
order, FusedTrainer(lr=1e-3, seed=11, capacity=(8, TCAP)), 5 steps: 'tiny' = widths (48, 32, 40, 32) in fp32 storage (these widths
are no whole k-tiles: the store has no planes and the batches are gathered), 'fp32' = (64, 128, 64, 128) read in place from a store
with planes, 'bf16' = (128, 128, 128, 128) in bf16 storage, in place."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
N_UTT, TCAP, SIZES = 33, (40, 6, 24, 5), (7, 6, 7, 6, 7)
DIMS = {"tiny": (48, 32, 40, 32), "fp32": (64, 128, 64, 128), "bf16": (128, 128, 128, 128)}
COUNTS = (1, 3, 4, 5, 4095, 4096, 4097, 1048577)


def _ref(x):
    return float(torch.linalg.vector_norm(x.double()).float())


def _bits(t):
    return t.view(torch.int32)


def _call(lib_mod, xs, ys=None, norm=None, bad=None, diff=None, scratch=None, nbytes=None):
    """sdumc_tensor_norms over the tensors xs (ys: their snapshots or None) -> (rc, norm, nonfinite, diff_norm)"""
    lib, n = lib_mod.lib, len(xs)
    segs = (lib_mod.NormSeg * n)()
    for i, s in enumerate(segs):
        s.x, s.count = xs[i].data_ptr(), xs[i].numel()
        s.y = ys[i].data_ptr() if ys is not None and ys[i] is not None else None
    need = lib.sdumc_tensor_norms_scratch_bytes(segs, n)
    norm = torch.full((n,), -7.0, device="cuda") if norm is None else norm
    bad = torch.full((n,), -7, dtype=torch.int32, device="cuda") if bad is None else bad
    diff = torch.full((n,), -7.0, device="cuda") if diff is None else diff
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda") if scratch is None else scratch
    rc = lib.sdumc_tensor_norms(segs, n, norm.data_ptr(), bad.data_ptr(), diff.data_ptr(), scratch.data_ptr(),
                                need if nbytes is None else nbytes, lib_mod.current_stream())
    return rc, norm, bad, diff


def _carve(buf, counts, first=1):
    """views of `counts` floats at ODD float offsets of buf (4 bytes past every alignment), 1 or 3 floats apart"""
    out, o = [], first
    for k, c in enumerate(counts):
        out.append(buf[o:o + c])
        o += c + (2 if (o + c) % 2 else 1) + 2 * (k % 2)
        assert o % 2 == 1
    return out


@pytest.fixture(scope="module")
def lib_mod():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def carved(lib_mod):
    g = torch.Generator(device="cuda").manual_seed(3)
    total = sum(COUNTS) + 64
    buf = torch.randn(total, generator=g, device="cuda") * 1e-3
    other = torch.randn(total + 2, generator=g, device="cuda") * 1e-3
    return buf, other


def test_entry_alone_norms_diff_norms_and_the_rolling_snapshot(lib_mod, carved):
    """1. every norm within one ulp of the fp64 reference, for segments of 1 .. 1 048 577 floats at odd float offsets; the same for
    diff_norm against a snapshot of other values -- once with y sitting like x within 16 bytes (16-byte loads of both) and once two
    floats off (the one-float-per-lane route) --; afterwards y equals x bit for bit, a second call gives diff_norm == 0 and the same
    norms, and two calls give identical bits."""
    buf, other = carved
    xs = _carve(buf, COUNTS)
    assert all(x.data_ptr() % 8 == 4 for x in xs)
    rc, norm, bad, diff = _call(lib_mod, xs)
    assert rc == 0
    for x, got in zip(xs, norm.tolist()):
        want = _ref(x)
        print(f"n {x.numel()}: norm {got!r} reference {want!r} rel {abs(got - want) / want:.3e}")
        assert want > 0 and abs(got - want) <= ULP * want, x.numel()
    assert not bool(bad.any()) and bool((diff == -7.0).all())      # (no snapshot: diff_norm is left as it is)
    rc, norm2, bad2, _ = _call(lib_mod, xs)
    assert rc == 0 and torch.equal(_bits(norm), _bits(norm2)) and torch.equal(bad, bad2)
    for shift, what in ((0, "aligned alike"), (2, "two floats off")):
        snap = other.clone()
        ys = _carve(snap[shift:], COUNTS)
        assert all((x.data_ptr() - y.data_ptr()) % 16 == (0 if shift == 0 else 8) for x, y in zip(xs, ys))
        wants = [_ref(x.double() - y.double()) for x, y in zip(xs, ys)]
        rc, n3, b3, d3 = _call(lib_mod, xs, ys)
        assert rc == 0 and torch.equal(_bits(n3), _bits(norm)) and not bool(b3.any()), what
        for x, got, want in zip(xs, d3.tolist(), wants):
            print(f"n {x.numel()} {what}: diff_norm {got!r} reference {want!r} rel {abs(got - want) / want:.3e}")
            assert want > 0 and abs(got - want) <= ULP * want, (x.numel(), what)
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(xs, ys)), what
        # nothing but the segments was written: the floats between and around them are the ones of `other`
        keep = torch.ones_like(snap, dtype=torch.bool)
        for y in ys:
            o = (y.data_ptr() - snap.data_ptr()) // 4
            keep[o:o + y.numel()] = False
        assert torch.equal(_bits(snap[keep]), _bits(other[keep])), what
        rc, n4, _, d4 = _call(lib_mod, xs, ys)
        assert rc == 0 and bool((d4 == 0).all()) and torch.equal(_bits(n4), _bits(norm)), what
    # a mixed table: a snapshot for every other segment only
    ys = [y if k % 2 else None for k, y in enumerate(_carve(other.clone(), COUNTS))]
    rc, n5, _, d5 = _call(lib_mod, xs, ys)
    assert rc == 0 and torch.equal(_bits(n5), _bits(norm))
    assert all((d > 0) if y is not None else (d == -7.0) for d, y in zip(d5.tolist(), ys))


def test_nonfinite_values_stay_in_their_segment(lib_mod, carved):
    """2. a NaN and an Inf planted in two segments: their counts exact, their norms NaN / Inf as torch gives, every other segment's
    norm unchanged bit for bit; 4099 values of 3e38 give +Inf in fp32 (1.9e40 in fp64) with count 0"""
    buf, _ = carved
    work = buf.clone()
    xs = _carve(work, COUNTS)
    rc, clean, _, _ = _call(lib_mod, xs)
    assert rc == 0
    xs[4][4094] = float("nan")          # the last element of the 4095 segment
    xs[4][0] = float("nan")
    xs[7][8192 * 77 + 5] = float("-inf")
    xs[7][1048576] = float("inf")       # the last element of all
    xs[7][3] = float("inf")
    rc, norm, bad, _ = _call(lib_mod, xs)
    assert rc == 0 and bad.tolist() == [0, 0, 0, 0, 2, 0, 0, 3]
    for k, x in enumerate(xs):
        want = torch.linalg.vector_norm(x.double()).float()
        if k == 4:
            assert bool(torch.isnan(want)) and bool(torch.isnan(norm[k]))
        elif k == 7:
            assert float(want) == float("inf") and float(norm[k]) == float("inf")
        else:
            assert torch.equal(_bits(norm[k]), _bits(clean[k])), k
    xs[7][9] = float("nan")             # NaN beside Inf: NaN, as torch
    rc, norm, bad, _ = _call(lib_mod, xs)
    assert rc == 0 and bool(torch.isnan(norm[7])) and int(bad[7]) == 4
    assert bool(torch.isnan(torch.linalg.vector_norm(xs[7].double())))
    huge = torch.full((4099 + 1,), 3e38, device="cuda")[1:]
    rc, norm, bad, diff = _call(lib_mod, [xs[0], huge, xs[1]], [None, torch.zeros(4100, device="cuda")[1:], None])
    assert rc == 0 and float(norm[1]) == float("inf") and float(diff[1]) == float("inf") and bad.tolist() == [0, 0, 0]
    assert np.isfinite(float(torch.linalg.vector_norm(huge.double())))
    assert torch.equal(_bits(norm[0]), _bits(clean[0])) and torch.equal(_bits(norm[2]), _bits(clean[1]))


def test_refusals_on_the_device_leave_the_outputs_poisoned(lib_mod, carved):
    """3. SDUMC_EINVAL before any launch: the poisoned outputs and the snapshot are as they were after a synchronisation"""
    buf, other = carved
    xs = _carve(buf, COUNTS[:5])
    snap = other.clone()
    ys = _carve(snap, COUNTS[:5])
    lib, n = lib_mod.lib, len(xs)
    segs = (lib_mod.NormSeg * n)()
    for s, x, y in zip(segs, xs, ys):
        s.x, s.y, s.count = x.data_ptr(), y.data_ptr(), x.numel()
    need = lib.sdumc_tensor_norms_scratch_bytes(segs, n)
    norm = torch.full((n,), -7.0, device="cuda")
    bad = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    diff = torch.full((n,), -7.0, device="cuda")
    scratch = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    st = lib_mod.current_stream()
    P = lambda t: t.data_ptr()
    assert lib.sdumc_tensor_norms(segs, n, P(norm), P(bad), P(diff), P(scratch), need - 1, st) == -1      # a short scratch
    assert lib.sdumc_tensor_norms(segs, n, P(norm), P(bad), P(diff), P(scratch) + 8, need, st) == -1      # scratch not 16-byte aligned
    assert lib.sdumc_tensor_norms(segs, n, P(norm), P(bad), None, P(scratch), need, st) == -1             # snapshots, no diff_norm
    assert lib.sdumc_tensor_norms(segs, n, P(norm) + 2, P(bad), P(diff), P(scratch), need, st) == -1
    assert lib.sdumc_tensor_norms(segs, n, None, P(bad), P(diff), P(scratch), need, st) == -1
    assert lib.sdumc_tensor_norms(segs, 0, P(norm), P(bad), P(diff), P(scratch), need, st) == -1
    assert lib.sdumc_tensor_norms(None, n, P(norm), P(bad), P(diff), P(scratch), need, st) == -1
    segs[2].count = -1
    assert lib.sdumc_tensor_norms(segs, n, P(norm), P(bad), P(diff), P(scratch), need, st) == -1
    segs[2].count, segs[3].x = xs[2].numel(), xs[3].data_ptr() + 2
    assert lib.sdumc_tensor_norms(segs, n, P(norm), P(bad), P(diff), P(scratch), need, st) == -1
    segs[3].x = xs[3].data_ptr()
    many = (lib_mod.NormSeg * (lib_mod.TENSOR_NORMS_MAX_SEGS + 1))()
    for s in many:
        s.x, s.count = xs[0].data_ptr(), 1
    assert lib.sdumc_tensor_norms(many, len(many), P(norm), P(bad), P(diff), P(scratch), 1 << 20, st) == -1
    torch.cuda.synchronize()
    assert bool((norm == -7.0).all()) and bool((bad == -7).all()) and bool((diff == -7.0).all())
    assert torch.equal(_bits(snap), _bits(other))
    # and the table as it stands again is accepted
    assert lib.sdumc_tensor_norms(segs, n, P(norm), P(bad), P(diff), P(scratch), need, st) == 0
    torch.cuda.synchronize()
    assert bool((norm > 0).all()) and not bool(bad.any()) and bool((diff > 0).all())


def _batches(seed=1):
    p = torch.randperm(N_UTT, generator=torch.Generator().manual_seed(seed))
    out, o = [], 0
    for b in SIZES:
        out.append(p[o:o + b].clone())
        o += b
    return out


class _Env:
    def __init__(self):
        from sdumc_amd import engine, record
        self.engine, self.record = engine, record
        self.batches, self._made, self._runs = _batches(), {}, {}

    def setup(self, mode):
        if mode not in self._made:
            from oracle import sdumc_oracle as O
            from sdumc_amd.data import DeviceFeatureStore
            dims = DIMS[mode]
            P = O.init_params(dims, seed=8)
            lay = self.engine.ParamLayout.get(*dims[:3])
            flat = torch.zeros(lay.total)
            for k, v in lay.views(flat).items():
                v.copy_(P[k])
            store = DeviceFeatureStore.synthetic(N_UTT, TCAP, dims, seed=5, min_frac=0.25, bf16=mode == "bf16", planes=mode == "fp32")
            self._made[mode] = (flat.cuda(), store, lay)
        return self._made[mode]

    def trainer(self, mode):
        flat, store, lay = self.setup(mode)
        kw = {"bf16": True} if mode == "bf16" else {}
        tr = self.engine.FusedTrainer(flat.clone(), DIMS[mode], lr=1e-3, seed=11, capacity=(8, TCAP), **kw)
        return tr, store, lay

    def state(self, tr):
        m, v, step = tr.optimizer_state()
        return [tr.params.clone(), m.clone(), v.clone(), tr.state.hyper.clone(), tr.state.rng.t.clone(), tr.state.losses.clone()], step

    def run(self, mode):
        """once per mode: train_epoch(grad_norm=True, by_tensor='updates') with the bucket and the parameters cloned behind every step
        -> (record, buckets, thetas (thetas[0] = before the first step), the final state, the trainer)"""
        if mode not in self._runs:
            tr, store, lay = self.trainer(mode)
            buckets, thetas = [], [tr.params.clone()]

            def keep(i, losses):
                buckets.append(next(iter(tr._steps.values())).grads.clone())
                thetas.append(tr.params.clone())
            rec = tr.train_epoch(store, self.batches, grad_norm=True, by_tensor="updates", on_step=keep)
            torch.cuda.synchronize()
            assert tr._in_place(store) == (mode != "tiny")
            self._runs[mode] = (rec, buckets, thetas, self.state(tr), tr)
        return self._runs[mode]


@pytest.fixture(scope="module")
def env(lib_mod):
    return _Env()


def _assert_rows(what, got_rows, refs, names):
    worst = 0.0
    for i, (row, ref) in enumerate(zip(got_rows, refs)):
        for k, (got, want) in enumerate(zip(row.tolist(), ref)):
            assert abs(got - want) <= ULP * want, (what, i, names[k], got, want)
            worst = max(worst, abs(got - want) / want if want else 0.0)
    print(f"{what}: {len(refs)} steps x {len(names)} tensors, worst rel {worst:.3e} (bar {ULP:.3e})")


@pytest.mark.parametrize("mode", ["tiny", "fp32"])
def test_epoch_by_tensor_against_the_cloned_buckets_and_parameters(env, mode):
    """4. grad_norm[i] against the per-tensor fp64 norms of the bucket cloned behind step i, update_norm[i] against the norms of
    (theta_after - theta_before).double() with theta cloned around every step, param_norm[i] against theta_after's: one ulp each;
    sqrt(sum of grad_norm[i]^2) against log[i, 8] at rtol 1e-6; names = ParamLayout.live_names(); rows beyond `steps` NaN / 0."""
    rec, buckets, thetas, _, tr = env.run(mode)
    lay = env.setup(mode)[2]
    bt, n_steps = rec.by_tensor, len(SIZES)
    names = lay.live_names()
    assert list(bt.names) == names and len(names) == 83 and rec.steps == bt.steps == n_steps == len(buckets)
    assert bt.grad_norm.shape == (n_steps, 83) and bt.grad_norm.dtype == torch.float32 and bt.grad_nonfinite.dtype == torch.int32
    if mode == "tiny":
        assert {1, 3, 7} <= set(bt.counts)
    cut = lambda flat: [flat[o:o + c] for o, c in zip(bt.offsets, bt.counts)]
    _assert_rows(mode + " grad_norm", bt.grad_norm, [[_ref(x) for x in cut(b)] for b in buckets], names)
    _assert_rows(mode + " update_norm", bt.update_norm,
                 [[_ref(x) for x in cut((thetas[i + 1] - thetas[i]).double())] for i in range(n_steps)], names)
    _assert_rows(mode + " param_norm", bt.param_norm, [[_ref(x) for x in cut(thetas[i + 1])] for i in range(n_steps)], names)
    assert not bool(bt.grad_nonfinite.any()) and not bool(bt.param_nonfinite.any()) and bt.first_nonfinite() is None
    assert rec.summary()["first_nonfinite"] is None
    assert not torch.equal(buckets[0], buckets[1]) and bool((bt.update_norm > 0).sum() >= 42 * n_steps)      # (not vacuous: most tensors move on every step)
    total = bt.grad_norm.double().square().sum(1).sqrt().cpu().numpy()
    np.testing.assert_allclose(total, rec.log[:n_steps, 8].double().cpu().numpy(), rtol=1e-6)
    r = bt.update_ratio()
    assert r.shape == (n_steps, 83) and r.dtype == np.float64
    with np.errstate(divide="ignore", invalid="ignore"):
        np.testing.assert_array_equal(r, bt.update_norm.cpu().numpy().astype(np.float64) / bt.param_norm.cpu().numpy().astype(np.float64))
    # a shorter epoch into the same record: the rows beyond its steps are NaN / 0 again
    sub = tr.train_epoch(env.setup(mode)[1], env.batches[:3], grad_norm=True, by_tensor="updates", out=rec)
    torch.cuda.synchronize()
    assert sub is rec and rec.steps == bt.steps == 3
    assert bool(torch.isnan(bt.grad_norm[3:]).all()) and bool(torch.isnan(bt.update_norm[3:]).all()) and bool(torch.isnan(bt.param_norm[3:]).all())
    assert not bool(bt.grad_nonfinite[3:].any()) and bool(torch.isfinite(bt.grad_norm[:3]).all())
    env._runs.pop(mode)      # (the record was reused: the next test of this mode makes its own)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "tiny"])
def test_by_tensor_is_read_only_towards_the_run(env, mode):
    """5. parameters, moments, step count, Philox counter, losses and predictions are torch.equal between
    train_epoch(grad_norm=True) and train_epoch(grad_norm=True, by_tensor='updates') from the same seed (by_tensor=True too), in fp32
    and in bf16 storage; a record reused with out= across two epochs equals a fresh one."""
    rec, _, _, (state, step), _ = env.run(mode)
    a, store, lay = env.trainer(mode)
    plain = a.train_epoch(store, env.batches, grad_norm=True)
    torch.cuda.synchronize()
    sa, step_a = env.state(a)
    assert plain.by_tensor is None and step_a == step == len(SIZES)
    assert all(torch.equal(x, y) for x, y in zip(sa, state))
    same = lambda x, y: torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))
    assert same(plain.log, rec.log) and same(plain.preds, rec.preds) and torch.equal(plain.seen, rec.seen)
    b, _, _ = env.trainer(mode)
    g = b.train_epoch(store, env.batches, grad_norm=True, by_tensor=True)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(env.state(b)[0], state))
    assert g.by_tensor.update_norm is None and g.by_tensor.param_norm is None and g.by_tensor.snapshot is None
    assert torch.equal(_bits(g.by_tensor.grad_norm), _bits(rec.by_tensor.grad_norm)) and same(g.log, rec.log)
    # two epochs: a record reused with out= against fresh ones
    c, _, _ = env.trainer(mode)
    d, _, _ = env.trainer(mode)
    other = _batches(2)
    r1 = c.train_epoch(store, env.batches, grad_norm=True, by_tensor="updates")
    r2 = c.train_epoch(store, other, grad_norm=True, by_tensor="updates", out=r1)
    d.train_epoch(store, env.batches, grad_norm=True, by_tensor="updates")
    f2 = d.train_epoch(store, other, grad_norm=True, by_tensor="updates")
    torch.cuda.synchronize()
    assert r2 is r1 and all(torch.equal(x, y) for x, y in zip(env.state(c)[0], env.state(d)[0]))
    for name in ("grad_norm", "update_norm", "param_norm", "grad_nonfinite", "param_nonfinite"):
        assert torch.equal(_bits(getattr(r2.by_tensor, name)), _bits(getattr(f2.by_tensor, name))), name
    assert same(r2.log, f2.log) and same(r2.preds, f2.preds)
    assert bool((r2.by_tensor.update_norm > 0).sum() >= 42 * len(SIZES))
    # a record made for other options is refused before anything is enqueued
    before = env.state(c)[0]
    for kw in ({"by_tensor": True}, {}, {"by_tensor": "updates", "embeddings": True}):
        with pytest.raises(env.engine._lib.SdumcError):
            c.train_epoch(store, env.batches, grad_norm=True, out=r1, **kw)
    with pytest.raises(env.engine._lib.SdumcError):
        c.train_epoch(store, env.batches, grad_norm=True, by_tensor="updates", out=plain)
    with pytest.raises(env.engine._lib.SdumcError):
        c.train_epoch(store, env.batches, by_tensor="nonsense")
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(env.state(c)[0], before))


def test_tensor_norms_helper_on_a_model_grad_list(lib_mod):
    """6. record.tensor_norms on the .grad list of a drop-in model against torch, one ulp; its refusals"""
    import types
    from sdumc_amd import record
    from sdumc_amd.model import get_models
    torch.manual_seed(5)
    model = get_models(types.SimpleNamespace(input_dims=(64, 32, 48, 32), model="wengnet_mosei_mult_views_text_missing")).cuda()
    net = model.model
    gen = torch.Generator().manual_seed(11)
    for name in net._live_names:
        p = net._get(name)
        p.grad = (torch.randn(p.shape, generator=gen) * 1e-2).to(p.device)
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert len(grads) == len(net._live_names) == 83
    norms, bad = record.tensor_norms(grads)
    assert norms.shape == (83,) and norms.dtype == torch.float32 and norms.is_cuda and bad.dtype == torch.int32 and bad.is_cuda
    for g, got in zip(grads, norms.tolist()):
        want = _ref(g)
        assert want > 0 and abs(got - want) <= ULP * want, tuple(g.shape)
    assert not bool(bad.any())
    grads[7].view(-1)[0] = float("inf")
    n2, b2 = record.tensor_norms(grads)
    assert float(n2[7]) == float("inf") and int(b2[7]) == 1 and int(b2.sum()) == 1
    assert torch.equal(_bits(n2[:7]), _bits(norms[:7])) and torch.equal(_bits(n2[8:]), _bits(norms[8:]))
    # more tensors than one call's table holds: two calls, the same numbers
    many = [grads[k % 83] for k in range(2 * lib_mod.TENSOR_NORMS_MAX_SEGS + 5)]
    n3, b3 = record.tensor_norms(many)
    assert torch.equal(_bits(n3), _bits(torch.stack([n2[k % 83] for k in range(len(many))])))
    assert torch.equal(b3, torch.stack([b2[k % 83] for k in range(len(many))]))
    for wrong in ([grads[0].cpu()], [grads[0].double()], [grads[1].t()] if grads[1].dim() == 2 else [grads[0].cpu()], [], [None]):
        with pytest.raises(lib_mod.SdumcError):
            record.tensor_norms(wrong)
