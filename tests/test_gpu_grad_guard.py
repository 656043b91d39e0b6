"""Gradient-norm clipping and the non-finite step guard on the device (sdumc_grad_guard / sdumc_grad_guard_multi,
csrc/grad_guard.hip; TrainStep / FusedTrainer(clip_norm=, skip_nonfinite=); TrainRecord.guard; optim.clip_grad_norm_).

Bars, all derived:
  norm         the kernel accumulates n < 2^24 non-negative fp64 terms in a fixed order (off by at most n 2^-53 relative, far below
               half an fp32 ulp) and rounds once to fp32, as torch.linalg.vector_norm(x.double()).float() does: the two differ only
               where the exact value sits on a rounding boundary -- one fp32 ulp, relative 2^-23 (the bar of test_gpu_tensor_norms.py).
  coefficient  min(1, max_norm / (norm + 1e-6)) in float64 from the fp64 norm, rounded once: equality with numpy's evaluation.
  bucket       one fp32 multiply per element: bit equality with torch's g * coef; untouched (bit equality with the input) at coef 1.
  fp64 torch   torch.nn.utils.clip_grad_norm_ on fp64 copies: our element = g coef64 (1 + e1)(1 + e2), |e1|, |e2| <= 2^-24 (the
               coefficient's rounding to fp32, the fp32 multiply): relative 2^-23 (1 + 2^-20) covers both and the fp64 noise.
  fused step   bit equality throughout (torch.equal): the guard adds launches between the backward and Adam and changes no
               arithmetic of either.
Fused-step fixtures: B = 4, T = (13, 5, 9, 3), lr 1e-3, seed 3; one warm-up step gives the state S1 (non-zero moments, t = 1) every
compared step resumes from (load_optimizer_state), the guarded and the unguarded ones alike."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
SIZES = (1, 3, 255, 4099, 3 * 8192 + 5)
MULTI = (1, 3, 255, 4099, 70000)
B, T = 4, (13, 5, 9, 3)
# the smallest shape in both settings of the storage switch (at these widths bf16=True rounds the GEMM operands and keeps
# fp32 storage: engine.bf16_mode), and widths of whole k-tiles where bf16=True is bf16 STORAGE
MODES = {"fp32": ((48, 32, 40, 32), False), "bf16": ((48, 32, 40, 32), True), "bf16-storage": ((128, 128, 128, 128), True)}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _coef(norm64, max_norm):
    """the contract's formula in numpy float64 from the fp64 norm, the max_norm the kernel saw (fp32), one rounding"""
    return np.float32(min(1.0, np.float64(np.float32(max_norm)) / (np.float64(norm64) + 1e-6)))


@pytest.fixture(scope="module")
def lib_mod():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import _lib
    return _lib


def _values(n, seed):
    """n values of magnitude 2^-20 .. 2^20 and both signs; from 3 elements on with -0.0 and two subnormals among them"""
    g = torch.Generator().manual_seed(seed)
    v = torch.exp2(torch.rand(n, generator=g) * 40 - 20) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    if n >= 3:
        v[0], v[1] = -0.0, 1e-40
    if n >= 255:
        v[n // 2], v[n - 1] = -3e-42, -0.0
    return v


def _odd(v, pad=8.5):
    """v on the device at a base address 4 bytes past 16-byte alignment, `pad` in the floats around it -> (buffer, view)"""
    buf = torch.full((v.numel() + 9,), pad, device="cuda")
    x = buf[1:1 + v.numel()]
    x.copy_(v)
    assert x.data_ptr() % 16 == 4
    return buf, x


def _guard(lib_mod, x, max_norm, skip=0, hyper=None):
    lib = lib_mod.lib
    nb = lib.sdumc_grad_guard_scratch_bytes(x.numel())
    assert nb >= 16
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    guard = torch.full((4,), -7.0, device="cuda")
    rc = lib.sdumc_grad_guard(x.data_ptr(), x.numel(), max_norm, skip, lib_mod.ptr(hyper), scratch.data_ptr(), guard.data_ptr(),
                              lib_mod.current_stream())
    assert rc == 0
    return guard


@pytest.mark.parametrize("n", SIZES)
def test_kernel_norm_coefficient_and_bucket(lib_mod, n):
    """1. per size: the norm within one ulp, the coefficient equal to the formula, the bucket bit-equal to g * coef and nothing
    around it written; max_norm above the norm, and max_norm 0, leave the bucket's bits alone with coef 1; the same call twice gives
    the same guard bits"""
    v = _values(n, 10 + n)
    buf, x = _odd(v)
    g0 = x.clone()
    norm64 = float(torch.linalg.vector_norm(g0.double()))
    want = float(np.float32(norm64))
    # above the norm, and no clipping at all: untouched
    for max_norm in (2.0 * want + 1.0, 0.0):      # (+ 1: twice a norm below 1e-6 would still clip, the formula's 1e-6)
        guard = _guard(lib_mod, x, max_norm, skip=1)
        got = guard.tolist()
        print(f"n {n} max_norm {max_norm!r}: guard {got!r} reference norm {want!r}")
        assert want > 0 and abs(got[0] - want) <= ULP * want
        assert got[1:] == [1.0, 0.0, 0.0]
        assert torch.equal(_bits(x), _bits(g0))
    first = guard.clone()
    max_norm = 0.37 * want
    guard = _guard(lib_mod, x, max_norm)
    got = guard.tolist()
    coef = _coef(norm64, max_norm)
    print(f"n {n} max_norm {max_norm!r}: guard {got!r} reference norm {want!r} coef {coef!r}")
    assert torch.equal(_bits(guard[0:1]), _bits(first[0:1]))      # the same input, the same norm bits
    assert np.float32(got[1]) == coef and 0 < coef < 1 and got[2:] == [0.0, 0.0]
    assert torch.equal(_bits(x), _bits(g0 * guard[1]))
    assert float(buf[0]) == 8.5 and bool((buf[1 + n:] == 8.5).all())


def test_kernel_norm_beyond_fp32_is_no_reason_to_skip(lib_mod):
    """2. 4099 elements of 3e38: the fp64 norm (1.9e40) is finite, so the coefficient is a tiny finite number taken from it while
    guard[0] reads +Inf in fp32; no element is non-finite and the step is not skipped"""
    buf, x = _odd(torch.full((4099,), 3e38))
    g0 = x.clone()
    hyper = torch.tensor([1e-3, 5.0, 0.25, 0.5], device="cuda")
    norm64 = float(torch.linalg.vector_norm(g0.double()))
    guard = _guard(lib_mod, x, 1.0, skip=1, hyper=hyper)
    got, coef = guard.tolist(), _coef(norm64, 1.0)
    print(f"guard {got!r} fp64 norm {norm64!r} coef {coef!r}")
    assert np.isfinite(norm64) and got[0] == float("inf") and got[2:] == [0.0, 0.0]
    assert np.float32(got[1]) == coef and coef > 0
    assert torch.equal(_bits(x), _bits(g0 * guard[1])) and bool(torch.isfinite(x).all())
    assert hyper.tolist() == [np.float32(1e-3), 5.0, 0.25, 0.5]


def test_kernel_nonfinite_bucket_is_counted_skipped_and_left_alone(lib_mod):
    """3. two NaN and one -Inf: count 3, skipped 1, the bucket untouched, hyper[1] back by one and nothing else of hyper written;
    without skip_nonfinite the same bucket is counted but not skipped and hyper stays"""
    v = _values(4099, 5)
    v[0], v[2050], v[4098] = float("nan"), float("-inf"), float("nan")
    buf, x = _odd(v)
    g0 = x.clone()
    hyper = torch.tensor([1e-3, 5.0, 0.25, 0.5], device="cuda")
    guard = _guard(lib_mod, x, 1.0, skip=1, hyper=hyper)
    got = guard.tolist()
    print(f"skip: guard {got!r}")
    assert np.isnan(got[0]) and got[2:] == [3.0, 1.0]
    assert torch.equal(_bits(x), _bits(g0))
    assert hyper.tolist() == [np.float32(1e-3), 4.0, 0.25, 0.5]
    assert _guard(lib_mod, x, 1.0, skip=1, hyper=None).tolist()[2:] == [3.0, 1.0]      # (hyper is optional)
    guard = _guard(lib_mod, x, 0.0, skip=0, hyper=hyper)
    got = guard.tolist()
    print(f"no skip: guard {got!r}")
    assert np.isnan(got[0]) and got[1:] == [1.0, 3.0, 0.0]
    assert torch.equal(_bits(x), _bits(g0)) and float(hyper[1]) == 4.0


def _carve(buf, counts, first=1):
    """views of `counts` floats at ODD float offsets of buf (4 bytes past every alignment), 1 or 3 floats apart"""
    out, o = [], first
    for k, c in enumerate(counts):
        out.append(buf[o:o + c])
        o += c + (2 if (o + c) % 2 else 1) + 2 * (k % 2)
        assert o % 2 == 1
    return out


def _multi(lib_mod, xs, max_norm):
    lib, n = lib_mod.lib, len(xs)
    segs = (lib_mod.NormSeg * n)()
    for s, x in zip(segs, xs):
        s.x, s.y, s.count = x.data_ptr(), None, x.numel()
    nb = lib.sdumc_grad_guard_multi_scratch_bytes(segs, n)
    assert nb >= 16
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    guard = torch.full((4,), -7.0, device="cuda")
    rc = lib.sdumc_grad_guard_multi(segs, n, max_norm, scratch.data_ptr(), nb, guard.data_ptr(), lib_mod.current_stream())
    assert rc == 0
    return guard


def test_multi_segment_entry_against_the_formula_and_torch_in_float64(lib_mod):
    """4. five tensors of 1 .. 70 000 floats at odd offsets: ONE norm over all of them within an ulp, the formula's coefficient,
    every tensor bit-equal to g * coef, the floats between them untouched, coef 1 leaves every bit; and against
    torch.nn.utils.clip_grad_norm_ on fp64 copies: its returned norm within an ulp, its clipped gradients within 2^-23 relative"""
    vals = _values(sum(MULTI), 21)
    buf = torch.full((sum(MULTI) + 64,), 8.5, device="cuda")
    xs = _carve(buf, MULTI)
    assert all(x.data_ptr() % 8 == 4 for x in xs)
    o = 0
    for x in xs:
        x.copy_(vals[o:o + x.numel()])
        o += x.numel()
    before = buf.clone()
    g0 = [x.clone() for x in xs]
    norm64 = float(torch.linalg.vector_norm(torch.cat(g0).double()))
    want = float(np.float32(norm64))
    guard = _multi(lib_mod, xs, 3.0 * want)
    assert abs(float(guard[0]) - want) <= ULP * want and guard.tolist()[1:] == [1.0, 0.0, 0.0]
    assert torch.equal(_bits(buf), _bits(before))
    max_norm = 0.25 * want
    guard = _multi(lib_mod, xs, max_norm)
    got, coef = guard.tolist(), _coef(norm64, max_norm)
    print(f"guard {got!r} reference norm {want!r} coef {coef!r}")
    assert abs(got[0] - want) <= ULP * want and np.float32(got[1]) == coef and got[2:] == [0.0, 0.0]
    keep = torch.ones_like(buf, dtype=torch.bool)
    for x, g in zip(xs, g0):
        assert torch.equal(_bits(x), _bits(g * guard[1])), x.numel()
        k = (x.data_ptr() - buf.data_ptr()) // 4
        keep[k:k + x.numel()] = False
    assert bool((buf[keep] == 8.5).all())
    # torch on fp64 copies
    ps = [torch.nn.Parameter(torch.zeros(g.numel(), dtype=torch.float64, device="cuda")) for g in g0]
    for p, g in zip(ps, g0):
        p.grad = g.double()
    total = float(torch.nn.utils.clip_grad_norm_(ps, float(np.float32(max_norm))))
    assert abs(got[0] - total) <= ULP * total
    worst = 0.0
    for p, x in zip(ps, xs):
        ref = p.grad
        big = ref.abs() >= 2.0 ** -100      # (a subnormal fp32 product has no relative bound: the planted zeros and subnormals)
        rel = ((x.double() - ref).abs()[big] / ref.abs()[big]).max().item() if bool(big.any()) else 0.0
        worst = max(worst, rel)
        assert bool(((x.double() - ref).abs()[~big] <= 2.0 ** -149).all())
    print(f"worst relative difference to torch's fp64 clip: {worst:.3e}")
    assert worst <= ULP * (1 + 2.0 ** -20)


# ------------------------------------------------------------------------------------------------------------------ the fused step
class _Fused:
    def __init__(self, mode):
        from oracle import sdumc_oracle as O
        from sdumc_amd import engine
        self.engine = engine
        self.dims, self.bf16 = MODES[mode]
        P = O.init_params(self.dims, seed=1)
        self.lay = lay = engine.ParamLayout.get(*self.dims[:3])
        flat = torch.zeros(lay.total)
        for k, v in lay.views(flat).items():
            v.copy_(P[k])
        self.batch = [t.cuda() for t in O.synthetic_batch(B, T, self.dims, seed=2)]
        warm = self._step(flat.cuda())
        warm.set_batch(*self.batch)
        warm.run()
        torch.cuda.synchronize()
        assert warm.optimizer_state()[2] == 1 and warm.rng.call == 2
        self.S1 = types.SimpleNamespace(params=warm.params.clone(), m=warm.adam_m.clone(), v=warm.adam_v.clone())
        ref = self.resume()
        ref.run()
        self.ref = self.state(ref)
        self.ref_grads = ref.grads.clone()

    def _step(self, flat, **kw):
        return self.engine.TrainStep(flat, B, T, self.dims, lr=1e-3, seed=3, bf16=self.bf16, **kw)

    def resume(self, call=None, nan_label=False, **kw):
        """a fresh step at the state S1 (t = 1, dropout counter 2 or `call`) with the fixture's batch installed"""
        ts = self._step(self.S1.params.clone(), **kw)
        ts.load_optimizer_state(self.S1.m, self.S1.v, 1)
        if call is not None:
            ts.rng.set_call(call)
        self.install(ts, nan_label)
        return ts

    def install(self, ts, nan_label):
        labels = self.batch[4].clone()
        if nan_label:
            labels[1] = float("nan")
        ts.set_batch(*self.batch[:4], labels)

    @staticmethod
    def state(ts):
        torch.cuda.synchronize()
        return {"params": ts.params.clone(), "adam_m": ts.adam_m.clone(), "adam_v": ts.adam_v.clone(), "losses": ts.losses.clone(),
                "hyper": ts.hyper.clone(), "call": ts.rng.call}


_fused = {}


@pytest.fixture
def fused(request, lib_mod):
    mode = request.param
    if mode not in _fused:
        _fused[mode] = _Fused(mode)
    return _fused[mode]


def _same_state(a, b, what, keys=("params", "adam_m", "adam_v", "losses", "hyper", "call")):
    for k in keys:
        same = a[k] == b[k] if k == "call" else torch.equal(_bits(a[k]), _bits(b[k]))
        assert same, (what, k)


@pytest.mark.parametrize("fused", list(MODES), indirect=True)
def test_step_with_a_guard_that_never_clips_is_the_unguarded_step(fused):
    """5a. clip_norm = 1e30: parameters, both moments, losses, hyper and the dropout counter equal the unguarded step's from the
    same state, bit for bit; guard = {the bucket's norm within an ulp, 1, 0, 0} and the bucket is the unguarded one"""
    ts = fused.resume(clip_norm=1e30, skip_nonfinite=True)
    assert ts.guard is not None and ts.guard.shape == (4,) and ts.guard.is_cuda
    ts.run()
    _same_state(fused.state(ts), fused.ref, "clip_norm=1e30")
    want = float(torch.linalg.vector_norm(fused.ref_grads.double()).float())
    got = ts.guard.tolist()
    print(f"guard {got!r} reference norm {want!r}")
    assert want > 0 and abs(got[0] - want) <= ULP * want and got[1:] == [1.0, 0.0, 0.0]
    assert torch.equal(_bits(ts.grads), _bits(fused.ref_grads))
    assert bool(torch.isfinite(fused.ref["params"]).all())
    plain = fused.resume()
    assert plain.guard is None and plain.cfg.guard is None and plain.cfg.clip_norm == 0.0 and plain.cfg.skip_nonfinite == 0


@pytest.mark.parametrize("fused", list(MODES), indirect=True)
def test_clipped_step_is_the_multiplied_bucket_through_todays_adam(fused):
    """5b. clip_norm at half the measured norm: parameters and moments equal sdumc_adam_step applied by the test to the unguarded
    step's bucket times guard[1]; the coefficient is the formula's; the step's bucket holds the scaled gradients"""
    from sdumc_amd import ops
    norm32 = torch.linalg.vector_norm(fused.ref_grads.double()).float()
    clip = 0.5 * float(norm32)
    ts = fused.resume(clip_norm=clip)
    ts.run()
    got = fused.state(ts)
    guard = ts.guard.clone()
    coef = _coef(float(torch.linalg.vector_norm(fused.ref_grads.double())), clip)
    print(f"guard {guard.tolist()!r} clip_norm {clip!r} coef {coef!r}")
    assert np.float32(float(guard[1])) == coef and 0.49 < coef < 0.51 and guard.tolist()[2:] == [0.0, 0.0]
    scaled = fused.ref_grads * guard[1]
    assert torch.equal(_bits(ts.grads), _bits(scaled))
    live = fused.lay.live
    p, m, v = fused.S1.params.clone(), fused.S1.m.clone(), fused.S1.v.clone()
    hyper = torch.tensor([1e-3, 1.0, 0.0, 0.0], device="cuda")
    ops.adam_step(p[:live], scaled, m, v, hyper)
    torch.cuda.synchronize()
    want = {"params": p, "adam_m": m, "adam_v": v, "hyper": hyper, "losses": fused.ref["losses"], "call": fused.ref["call"]}
    _same_state(got, want, "clip at half the norm")
    assert not torch.equal(got["params"], fused.ref["params"])      # (the clip did change the step)


@pytest.mark.parametrize("fused", list(MODES), indirect=True)
def test_nan_label_is_skipped_and_the_run_goes_on_as_if_nothing_happened(fused):
    """5c. one NaN label with skip_nonfinite: parameters, moments and the step count are bit-identical to before, the dropout
    counter has advanced by 2, guard[3] == 1; the NEXT step with finite labels equals the step an unguarded trainer makes from
    that state and that counter"""
    ts = fused.resume(nan_label=True, skip_nonfinite=True)
    ts.run()
    got = fused.state(ts)
    guard = ts.guard.tolist()
    print(f"guard {guard!r} losses {got['losses'].tolist()!r}")
    assert guard[3] == 1.0 and guard[2] > 0 and guard[1] == 1.0
    for k, want in (("params", fused.S1.params), ("adam_m", fused.S1.m), ("adam_v", fused.S1.v)):
        assert torch.equal(_bits(got[k]), _bits(want)), k
    assert float(got["hyper"][1]) == 1.0 and ts.optimizer_state()[2] == 1 and got["call"] == 4
    assert float(got["losses"][7]) == 0.0      # (the cluster-failure flag is not the guard's)
    fused.install(ts, nan_label=False)
    ts.run()
    after = fused.state(ts)
    assert ts.guard.tolist()[1:] == [1.0, 0.0, 0.0]
    plain = fused.resume(call=4)
    plain.run()
    _same_state(after, fused.state(plain), "the step after a skipped one")
    assert float(after["hyper"][1]) == 2.0 and after["call"] == 6 and bool(torch.isfinite(after["params"]).all())


@pytest.mark.parametrize("fused", list(MODES), indirect=True)
def test_nan_label_without_the_guard_poisons_the_parameters(fused):
    """5d. the behaviour the option exists to prevent: the same NaN label, guard off -> NaN in the parameters and both moments"""
    ts = fused.resume(nan_label=True)
    ts.run()
    got = fused.state(ts)
    assert bool(torch.isnan(got["params"]).any()) and bool(torch.isnan(got["adam_m"]).any()) and bool(torch.isnan(got["adam_v"]).any())
    assert float(got["hyper"][1]) == 2.0 and got["call"] == 4
    # ... and clipping alone does not save it either (torch's clip_grad_norm_ with error_if_nonfinite=False: a NaN coefficient)
    ts = fused.resume(nan_label=True, clip_norm=1.0)
    ts.run()
    assert bool(torch.isnan(fused.state(ts)["params"]).any()) and ts.guard.tolist()[2] > 0 and ts.guard.tolist()[3] == 0.0


def test_step_refuses_what_is_out_of_scope(lib_mod):
    """6. capture() of a guarded step raises; sdumc_train_step refuses guard options without a guard vector, and a guard without
    scratch, before anything is enqueued (the state is untouched)"""
    f = _fused.get("fp32") or _fused.setdefault("fp32", _Fused("fp32"))
    ts = f.resume(clip_norm=1.0)
    with pytest.raises(lib_mod.SdumcError, match="capture"):
        ts.capture()
    plain = f.resume()
    before = f.state(plain)
    for field, value in (("clip_norm", 1.0), ("skip_nonfinite", 1), ("guard_scratch", ts.guard_scratch.data_ptr())):
        setattr(plain.cfg, field, value)
        with pytest.raises(lib_mod.SdumcError, match="SDUMC_EINVAL"):
            plain.launch()
        setattr(plain.cfg, field, 0 if field != "guard_scratch" else None)
    plain.cfg.guard = ts.guard.data_ptr()      # a guard vector, no scratch
    with pytest.raises(lib_mod.SdumcError, match="SDUMC_EINVAL"):
        plain.launch()
    plain.cfg.guard = None
    _same_state(f.state(plain), before, "refused launches")
    plain.run()
    _same_state(f.state(plain), f.ref, "the step after the refusals")


# ------------------------------------------------------------------------------------------------------------ record and drop-in
def test_train_epoch_keeps_the_guard_of_every_step(lib_mod):
    """7. FusedTrainer.train_epoch over three ragged batches with a NaN label in the second: rec.guard [3, 4], skipped_steps() == [1],
    the run's step count 2 and dropout counter 6, finite parameters; the unclipped steps' guard norm is the record's own grad_norm
    (two fp64 reduces of the same bucket, each rounded once: one ulp)"""
    from oracle import sdumc_oracle as O
    from sdumc_amd import engine
    from sdumc_amd.data import DeviceFeatureStore
    dims, tcap, n = (48, 32, 40, 32), (40, 6, 24, 5), 20
    P = O.init_params(dims, seed=8)
    lay = engine.ParamLayout.get(*dims[:3])
    flat = torch.zeros(lay.total)
    for k, v in lay.views(flat).items():
        v.copy_(P[k])
    store = DeviceFeatureStore.synthetic(n, tcap, dims, seed=5, min_frac=0.25)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    batches = [perm[0:7].clone(), perm[7:13].clone(), perm[13:20].clone()]
    store.vals[int(batches[1][2])] = float("nan")
    tr = engine.FusedTrainer(flat.cuda(), dims, lr=1e-3, seed=11, capacity=(8, tcap), clip_norm=1e30, skip_nonfinite=True)
    assert tr.guard is not None and tr.guard.shape == (4,)
    rec = tr.train_epoch(store, batches, grad_norm=True)
    torch.cuda.synchronize()
    g = rec.guard.cpu().numpy()
    log = rec.log.cpu().numpy()
    print(f"guard\n{g!r}\nlog grad_norm {log[:, 8]!r} nonfinite {log[:, 9]!r}")
    assert rec.guard.shape == (3, 4) and rec.steps == 3 and rec.skipped_steps() == [1]
    assert g[:, 3].tolist() == [0.0, 1.0, 0.0] and g[0, 1] == 1.0 and g[2, 1] == 1.0
    assert np.isnan(g[1, 0]) and np.isnan(g[1, 1])      # (a NaN norm and, with a clip_norm, torch's NaN coefficient: nothing was scaled)
    assert g[0, 2] == 0 and g[2, 2] == 0 and g[1, 2] > 0 and g[1, 2] == log[1, 9]
    for i in (0, 2):
        assert g[i, 0] > 0 and abs(float(g[i, 0]) - float(log[i, 8])) <= ULP * float(log[i, 8])
    assert tr.optimizer_state()[2] == 2 and tr.state.rng.call == 6
    assert bool(torch.isfinite(tr.params).all()) and bool(torch.isfinite(tr.state.adam_v).all())
    assert torch.equal(rec.guard[2], tr.guard)
    # the record is reusable as out= and a trainer without the options keeps no column
    again = tr.train_epoch(store, [batches[0]], grad_norm=True, out=rec)
    torch.cuda.synchronize()
    assert again is rec and rec.steps == 1 and rec.skipped_steps() == [] and bool(torch.isnan(rec.guard[1:]).all())


def test_clip_grad_norm_on_the_dropin_modules_gradients(lib_mod):
    """8. optim.clip_grad_norm_ over the drop-in module's .grad tensors: a 0-dim device tensor with the total norm within an ulp,
    every gradient bit-equal to g * coef with the formula's coefficient, dead parameters still without a gradient; a max_norm above
    the norm leaves every bit"""
    from sdumc_amd import optim
    from sdumc_amd.model import get_models
    torch.manual_seed(5)
    model = get_models(types.SimpleNamespace(input_dims=(64, 32, 48, 32), model="wengnet_mosei_mult_views_text_missing")).cuda()
    net = model.model
    gen = torch.Generator().manual_seed(11)
    g0 = {}
    for name in net._live_names:
        p = net._get(name)
        p.grad = (torch.randn(p.shape, generator=gen) * 1e-2).to(p.device)
        g0[name] = p.grad.clone()
    norm64 = float(torch.linalg.vector_norm(torch.cat([g.reshape(-1) for g in g0.values()]).double()))
    want = float(np.float32(norm64))
    total = optim.clip_grad_norm_(model.parameters(), 10.0 * want)
    assert total.dim() == 0 and total.is_cuda and total.dtype == torch.float32
    assert abs(float(total) - want) <= ULP * want
    assert all(torch.equal(_bits(net._get(k).grad), _bits(g)) for k, g in g0.items())
    max_norm = 0.5 * want
    total = optim.clip_grad_norm_(model.parameters(), max_norm, norm_type=2, foreach=True)
    coef = torch.tensor(_coef(norm64, max_norm), device="cuda")
    print(f"total {float(total)!r} reference {want!r} coef {float(coef)!r}; {len(g0)} gradient tensors")
    assert abs(float(total) - want) <= ULP * want and 0.49 < float(coef) < 0.51
    for k, g in g0.items():
        assert torch.equal(_bits(net._get(k).grad), _bits(g * coef)), k
    n_dead = sum(1 for p in model.parameters() if p.grad is None)
    assert n_dead == len(list(model.parameters())) - len(g0)
