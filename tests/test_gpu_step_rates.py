"""Per-tensor learning rates, decay and frozen tensors in the fused step (TrainStep / FusedTrainer: freeze=, lr_scale=, decay_scale=;
sdumc_step_cfg.rates; csrc/engine.hip, csrc/adam.hip).

Everything is bit equality (torch.equal on the bits) against the PARENT's own kernels, which are the semantics:
  freeze   a plain TrainStep on a copy, whose frozen tensors' parameters and moments are put back to their initial bits after every
           step (torch's requires_grad = False);
  scales   sdumc_adam_step applied by the test, tensor by tensor, to the plain step's bucket with that tensor's learning rate
           fp32(lr 2^k) and decay fp32(wd) * fp32(s) (exact by construction: tests/test_gpu_adam_rates.py);
  guard    the norm within one fp32 ulp of torch.linalg.vector_norm in fp64 (the reduce's documented accuracy,
           tests/test_gpu_grad_guard.py), everything else bit equality.

Shapes, each in fp32 and with bf16=True, train mode with Philox masks and one seed on both sides:
  lens    dims (128, 128, 128, 128), B = 4, T = (70, 9, 33, 6) with the key-padding lengths of tests/test_gpu_bf16_edges.py (its case 6)
  ragged  dims (64, 192, 64, 192), B = 3, T = (65, 1, 64, 2) (its case 2)
  tiny    dims (48, 32, 40, 32), B = 4, T = (13, 5, 9, 3)
  odd     dims (37, 32, 42, 32), B = 4, T = (13, 5, 9, 3): audio and video widths that are no multiples of 4
The frame dW routes plan_backward can choose: the grouped launch in fp32 storage (lens, ragged and tiny in fp32), the grouped launch in
bf16 storage (lens and ragged with bf16=True), the per-stream GEMMs for every modality (tiny and odd with bf16=True: these widths are no
whole k-tiles, so bf16=True rounds operands and keeps fp32 storage, where the grouped launch is not used), and the MIXED schedule of
odd in fp32: audio's and video's frame dW go per stream (their rows are not 16-byte aligned) while text's is a problem of the grouped
launch behind the join -- frozen, one kind is skipped and the other is not, and the trailing launch may or may not have a problem left.

Every step starts from the state S0: the initial parameters, random moments (second moment >= 0), step count 3, dropout counter 6."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
LR, WD, SEED, T0 = 1e-3, 1e-2, 3, 3
LENS = ([70, 12, 65, 1], [9, 3, 1, 8], [33, 33, 2, 17], [6, 1, 4, 5])
#         dims                  B  T                lengths
SHAPES = {"lens": ((128, 128, 128, 128), 4, (70, 9, 33, 6), True),
          "ragged": ((64, 192, 64, 192), 3, (65, 1, 64, 2), False),
          "tiny": ((48, 32, 40, 32), 4, (13, 5, 9, 3), False),
          "odd": ((37, 32, 42, 32), 4, (13, 5, 9, 3), False)}
CONFIGS = [(s, b) for s in SHAPES for b in (False, True)]
FREEZE = ("frame_dim_reshape_*", "cross_fc_att.weight")
KEYS = ("params", "adam_m", "adam_v", "losses", "hyper", "call")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _state(ts):
    torch.cuda.synchronize()
    return {"params": ts.params.clone(), "adam_m": ts.adam_m.clone(), "adam_v": ts.adam_v.clone(), "losses": ts.losses.clone(),
            "hyper": ts.hyper.clone(), "call": ts.rng.call, "grads": ts.grads.clone()}


def _same(a, b, what, keys=KEYS):
    for k in keys:
        same = a[k] == b[k] if k == "call" else torch.equal(_bits(a[k]), _bits(b[k]))
        assert same, (what, k)


def _profiled(lib_mod, call):
    """{variant: (launches, flops)} of what `call` launched through the GEMM entry points (sdumc_profile_report, the launch report
    tests/test_gpu_gemm_parity.py reads)"""
    lib = lib_mod.lib
    torch.cuda.synchronize()
    lib.sdumc_profile_enable(1)
    try:
        call()
        torch.cuda.synchronize()
        arr = (lib_mod.ProfEntry * 64)()
        n = lib.sdumc_profile_report(arr, 64)
    finally:
        lib.sdumc_profile_enable(0)
    assert n > 0
    return {arr[i].name.decode(): (int(arr[i].launches), float(arr[i].total_flops)) for i in range(n) if arr[i].launches}


class _Run:
    """One (shape, storage) setting: the inputs, S0, and three steps of the plain TrainStep from it (state and bucket after each)"""

    def __init__(self, shape, bf16):
        from oracle import sdumc_oracle as O
        from sdumc_amd import _lib, engine
        self.engine, self.lib_mod = engine, _lib
        self.dims, self.B, self.T, with_lengths = SHAPES[shape]
        self.bf16 = bf16
        P = O.init_params(self.dims, seed=21)
        self.lay = lay = engine.ParamLayout.get(*self.dims[:3])
        flat = torch.zeros(lay.total)
        for k, v in lay.views(flat).items():
            v.copy_(P[k])
        self.flat = flat.cuda()
        batch = list(O.synthetic_batch(self.B, self.T, self.dims, seed=41))
        self.lens = None
        if with_lengths:
            self.lens = [torch.tensor(l, dtype=torch.int32) for l in LENS]
            for t, l in zip(batch[:4], self.lens):
                for b in range(self.B):
                    t[b, int(l[b]):] = 0
        self.batch = [t.cuda() for t in batch]
        g = torch.Generator().manual_seed(5)
        self.m0 = (torch.randn(lay.live, generator=g) * 1e-3).cuda()
        self.v0 = (torch.rand(lay.live, generator=g) * 1e-6).cuda()
        # the modalities whose frame dW goes per stream (the docstring): all of them where bf16=True rounds operands, else the ones
        # whose width is no multiple of 4
        self.per_stream = [m for m in range(3) if (bf16 and engine.bf16_mode(bf16, self.dims) == 1) or self.dims[m] % 4]
        self.segs = {name: (lay.entries[name][0], int(np.prod(lay.entries[name][1]))) for name in lay.live_names()}
        ref = self.step()
        self.S0 = _state(ref)
        self.plain, self.plain_launches = [], None
        for k in range(3):
            if k == 0:
                self.plain_launches = _profiled(_lib, ref.run)
            else:
                ref.run()
            self.plain.append(_state(ref))

    def step(self, nan_label=False, **kw):
        ts = self.engine.TrainStep(self.flat.clone(), self.B, self.T, self.dims, lr=LR, weight_decay=WD, seed=SEED, bf16=self.bf16, **kw)
        ts.load_optimizer_state(self.m0, self.v0, T0)
        labels = self.batch[4].clone()
        if nan_label:
            labels[1] = float("nan")
        ts.set_batch(*self.batch[:4], labels)
        if self.lens is not None:
            ts.set_lengths(self.lens)
        return ts

    def mask(self, names):
        m = torch.zeros(self.lay.live, dtype=torch.bool)
        for name in names:
            off, n = self.segs[name]
            m[off:off + n] = True
        return m.cuda()

    def frame_dw_flops(self, mods):
        """the frame_dim_reshape dW products of the modalities `mods`: 2 * 256 * width * rows, rows = B * T (text: both streams)"""
        Ta, Tt, Tv, T4 = self.T
        rows = (self.B * Ta, self.B * (Tt + T4), self.B * Tv)
        return sum(2.0 * 256 * self.dims[m] * rows[m] for m in mods)

    def adam_by_tensor(self, rates, bucket):
        """sdumc_adam_step applied tensor by tensor to `bucket` from S0, with each tensor's own learning rate and decay (frozen: left
        alone) -> (params[:live], m, v)"""
        from sdumc_amd import ops
        p, m, v = self.S0["params"][:self.lay.live].clone(), self.m0.clone(), self.v0.clone()
        for name, ls, ws, fr in zip(rates.names, rates.lr_scale, rates.decay_scale, rates.frozen):
            if fr:
                continue
            off, n = self.segs[name]
            lr = float(np.float32(LR) * np.float32(ls))
            assert lr == float(np.float32(LR)) * float(ls)      # a power of two (or one): exact
            pi, gi, mi, vi = (x[off:off + n].clone() for x in (p, bucket, m, v))
            hyper = torch.tensor([lr, float(T0), 0.0, 0.0], device="cuda")
            ops.adam_step(pi, gi, mi, vi, hyper, weight_decay=float(np.float32(WD) * np.float32(ws)))
            p[off:off + n], m[off:off + n], v[off:off + n] = pi, mi, vi
        torch.cuda.synchronize()
        return p, m, v


_runs = {}


@pytest.fixture
def run(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if request.param not in _runs:
        _runs[request.param] = _Run(*request.param)
    return _runs[request.param]


both = pytest.mark.parametrize("run", CONFIGS, indirect=True, ids=[f"{s}-{'bf16' if b else 'fp32'}" for s, b in CONFIGS])


@both
def test_an_explicit_table_of_ones_is_the_plain_step(run):
    """1. lr_scale = decay_scale = {'*': 1.0}: the rates launch in Adam's place; parameters, both moments, losses, the dropout counter,
    hyper and the bucket equal the plain step's after each of three steps"""
    ts = run.step(lr_scale={"*": 1.0}, decay_scale={"*": 1.0})
    assert ts.rates is not None and bool(ts.cfg.rates) and ts.cfg.rates.contents.n == 83 and not ts.rates.frozen.any()
    plain = run.step()
    assert plain.rates is None and not bool(plain.cfg.rates)
    for k in range(3):
        ts.run()
        _same(_state(ts), run.plain[k], f"step {k}", KEYS + ("grads",))
    assert run.plain[2]["call"] == 2 * T0 + 6 and float(run.plain[2]["hyper"][1]) == T0 + 3
    assert not torch.equal(run.plain[2]["params"], run.S0["params"])


def _check_freeze(run, freeze, skipped_mods):
    """three steps with `freeze` against the plain step with the frozen tensors put back after every step; skipped_mods: the
    modalities whose frame dW must not have run"""
    ts, ref = run.step(freeze=freeze), run.step()
    frozen = [n for n, f in zip(ts.rates.names, ts.rates.frozen) if f]
    assert frozen and set(frozen) < set(run.segs)
    fmask = run.mask(frozen)
    live = run.lay.live
    for k in range(3):
        if k == 0:
            launches = _profiled(run.lib_mod, ts.run)
        else:
            ts.run()
        ref.run()
        torch.cuda.synchronize()
        ref.params[:live][fmask] = run.S0["params"][:live][fmask]
        ref.adam_m[fmask], ref.adam_v[fmask] = run.m0[fmask], run.v0[fmask]
        got, want = _state(ts), _state(ref)
        _same(got, want, f"{freeze} step {k}")
        assert bool((_bits(got["grads"])[fmask] == 0).all()), f"{freeze} step {k}: a frozen segment of the bucket is not +0.0"
        assert torch.equal(_bits(got["grads"][~fmask]), _bits(want["grads"][~fmask])), f"{freeze} step {k}: a neighbour's gradient"
        assert bool((want["grads"][fmask] != 0).any())      # (the plain step does compute them)
    for name in frozen:
        off, n = run.segs[name]
        for key, init in (("params", run.S0["params"]), ("adam_m", run.m0), ("adam_v", run.v0)):
            assert torch.equal(_bits(got[key][off:off + n]), _bits(init[off:off + n])), (name, key)
    # the launch report: the GEMM products of the first step differ from the plain step's by exactly the skipped frame dW
    plain = run.plain_launches
    flops = lambda rep: sum(f for _, f in rep.values())
    count = lambda rep: sum(n for n, _ in rep.values())
    want_flops = run.frame_dw_flops(skipped_mods)
    print(f"{freeze}: GEMM launches {count(plain)} -> {count(launches)}, flops {flops(plain):.6g} -> {flops(launches):.6g} "
          f"(frame dW of modalities {skipped_mods}: {want_flops:.6g})")
    assert abs((flops(plain) - flops(launches)) - want_flops) <= 1e-9 * flops(plain)
    # one GEMM per stream of a skipped per-stream modality; the grouped launch behind the join (in halves where its slab is short)
    # goes when every modality it serves is skipped
    gone = sum(2 if m == 1 else 1 for m in skipped_mods if m in run.per_stream)
    grouped = [m for m in range(3) if m not in run.per_stream]
    fewer = count(plain) - count(launches)
    assert fewer == gone if not grouped else fewer >= gone + all(m in skipped_mods for m in grouped)
    assert set(launches) <= set(plain)
    return got


@both
def test_frozen_frame_projections_and_one_utterance_level_tensor(run):
    """2. freeze frame_dim_reshape_* and cross_fc_att.weight: every tensor's parameters and moments and the losses of all three steps
    equal the reference's; the frozen segments of .grads are +0.0 and every other segment is the reference's; no frame dW ran"""
    got = _check_freeze(run, FREEZE, (0, 1, 2))
    assert not torch.equal(got["params"], run.S0["params"])      # (the rest did train)


@both
def test_one_modality_frozen_and_its_weight_alone(run):
    """3. only the text projection frozen: the other two frame dW run; only its weight frozen: the dW still runs (the bias needs its
    column sum) and the weight segment is zeroed afterwards"""
    _check_freeze(run, ("frame_dim_reshape_1.*",), (1,))
    _check_freeze(run, ("frame_dim_reshape_1.weight",), ())


def _same_by_tensor(run, got, want):
    """every live tensor of the state `got` equals (params, m, v) = `want`; the alignment padding between tensors -- zero gradient, the
    default update -- is the plain step's; the parameters that never get a gradient are untouched"""
    live = run.lay.live
    for name, (off, n) in run.segs.items():
        for key, b in zip(("params", "adam_m", "adam_v"), want):
            assert torch.equal(_bits(got[key][off:off + n]), _bits(b[off:off + n])), (name, key)
    pad = ~run.mask(run.segs)
    assert 0 < int(pad.sum()) < 4 * len(run.segs)
    for key in ("params", "adam_m", "adam_v"):
        assert torch.equal(_bits(got[key][:live][pad]), _bits(run.plain[0][key][:live][pad])), (key, "padding")
    assert torch.equal(_bits(got["params"][live:]), _bits(run.S0["params"][live:]))


SCALES = dict(lr_scale={"cross_*": 0.5, "fc_out_v.*": 2.0, "frame_dim_reshape_*": 0.25, "fra2utt_1.*": 4.0},
              decay_scale={"*.bias": 0.0, "*.attention_context_vector": 0.0, "fc_att.weight": 0.3})


@both
def test_scales_are_adam_tensor_by_tensor(run):
    """4. power-of-two lr_scale on some tensors, decay_scale 0 on biases and context vectors (and 0.3 on one weight), one step: each
    tensor equals sdumc_adam_step applied to the plain step's bucket with that tensor's lr and decay"""
    ts = run.step(**SCALES)
    ts.run()
    got = _state(ts)
    _same(got, run.plain[0], "scales", ("losses", "hyper", "call", "grads"))
    _same_by_tensor(run, got, run.adam_by_tensor(ts.rates, run.plain[0]["grads"]))
    assert not torch.equal(got["params"], run.plain[0]["params"])


@both
def test_with_the_guard(run):
    """5. clip_norm and skip_nonfinite beside freeze and scales: guard[0] is the norm of the plain step's bucket with the frozen
    segments zeroed (one ulp); the bucket is that one times guard[1]; the update is item 4's rule on the scaled bucket.  A NaN label:
    every parameter and moment bit-unchanged, step count kept, the dropout counter advanced by 2."""
    opts = dict(freeze=FREEZE, lr_scale={"cross_*": 0.5, "fc_out_v.*": 2.0}, decay_scale={"*.bias": 0.0})
    probe = run.step(**opts)
    zeroed = run.plain[0]["grads"].clone()
    zeroed[run.mask([n for n, f in zip(probe.rates.names, probe.rates.frozen) if f])] = 0.0
    norm64 = float(torch.linalg.vector_norm(zeroed.double()))
    want = float(np.float32(norm64))
    full = float(torch.linalg.vector_norm(run.plain[0]["grads"].double()).float())
    clip = 0.37 * want
    ts = run.step(clip_norm=clip, skip_nonfinite=True, **opts)
    ts.run()
    got, guard = _state(ts), ts.guard.tolist()
    coef = np.float32(min(1.0, np.float64(np.float32(clip)) / (np.float64(norm64) + 1e-6)))
    print(f"guard {guard!r}: norm of the zeroed bucket {want!r} (of the whole bucket {full!r}), coefficient {coef!r}")
    assert want > 0 and abs(guard[0] - want) <= ULP * want and abs(full - want) > 4 * ULP * want      # (the frozen tensors do weigh)
    assert np.float32(guard[1]) == coef and 0 < coef < 1 and guard[2:] == [0.0, 0.0]
    scaled = zeroed * ts.guard[1]
    assert torch.equal(_bits(got["grads"]), _bits(scaled))
    _same_by_tensor(run, got, run.adam_by_tensor(ts.rates, scaled))
    _same(got, run.plain[0], "clipped", ("losses", "hyper", "call"))
    # a non-finite step
    ts = run.step(nan_label=True, clip_norm=clip, skip_nonfinite=True, **opts)
    ts.run()
    got, guard = _state(ts), ts.guard.tolist()
    assert guard[3] == 1.0 and guard[2] > 0
    for key, init in (("params", run.S0["params"]), ("adam_m", run.m0), ("adam_v", run.v0)):
        assert torch.equal(_bits(got[key]), _bits(init)), key
    assert float(got["hyper"][1]) == T0 and got["call"] == 2 * T0 + 2 and float(got["losses"][7]) == 0.0


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_fused_trainer_over_a_ragged_store(bf16):
    """6. FusedTrainer(freeze=, lr_scale=, decay_scale=) over a tiny ragged store, two batch shapes: run_epoch equals the chain of
    TrainSteps that share one state and the trainer's TensorRates; train_epoch(by_tensor='updates') shows update_norm == 0 and
    grad_norm == 0 exactly for the frozen tensors and > 0 for the others, in the order of trainer.rates.names"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle import sdumc_oracle as O
    from sdumc_amd import engine as E
    from sdumc_amd.data import DeviceFeatureStore
    dims = (128, 128, 128, 128) if bf16 else (64, 128, 64, 128)
    tcap, n = (40, 9, 24, 8), 20
    P = O.init_params(dims, seed=8)
    lay = E.ParamLayout.get(*dims[:3])
    flat0 = torch.zeros(lay.total)
    for k, v in lay.views(flat0).items():
        v.copy_(P[k])
    store = DeviceFeatureStore.synthetic(n, tcap, dims, seed=5, min_frac=0.25, **({"bf16": True} if bf16 else {"planes": True}))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    batches = [perm[0:6].clone(), perm[6:10].clone(), perm[10:16].clone()]
    assert len({store.batch_shape(ix) for ix in batches}) >= 2
    opts = dict(freeze=FREEZE, lr_scale={"cross_*": 0.5}, decay_scale={"*.bias": 0.0})

    def trainer():
        return E.FusedTrainer(flat0.clone().cuda(), dims, lr=LR, seed=11, capacity=(6, tcap), weight_decay=WD, bf16=bf16, **opts)

    tr, ls = trainer(), []
    assert isinstance(tr.rates, E.TensorRates) and tr.rates.names == lay.live_names()
    tr.run_epoch(store, batches, on_step=lambda i, l: ls.append(l.clone()))
    torch.cuda.synchronize()
    assert all(ts.rates is tr.rates for ts in tr._steps.values()) and len(tr._steps) >= 2
    # the chain
    flat = flat0.clone().cuda()
    state, chain = E._RunState(flat, lay.live, LR, 11), []
    for ix in batches:
        b, _, _, vals, _ = store.batch(ix)
        ts = E.TrainStep(flat, *store.batch_shape(ix), dims, share=state, weight_decay=WD, bf16=bf16, bits_next=False, rates=tr.rates,
                         **({} if bf16 else {"planes": True}))
        ts.set_batch(b["audios"], b["texts"], b["videos"], b["feat4s"], vals)
        chain.append(ts.run().clone())
        torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(ls, chain)):
        assert torch.equal(_bits(x), _bits(y)), (i, x.tolist(), y.tolist())
    assert torch.equal(_bits(tr.params), _bits(flat)) and torch.equal(_bits(tr.state.adam_m), _bits(state.adam_m))
    assert torch.equal(_bits(tr.state.adam_v), _bits(state.adam_v))
    # the record by tensor
    tr = trainer()
    rec = tr.train_epoch(store, batches, by_tensor="updates")
    torch.cuda.synchronize()
    bt = rec.by_tensor
    assert tuple(bt.names) == tuple(tr.rates.names)
    frozen = torch.from_numpy(tr.rates.frozen)
    gn, un = bt.grad_norm[:rec.steps].cpu(), bt.update_norm[:rec.steps].cpu()
    assert rec.steps == 3 and frozen.sum() == 7
    assert bool((gn[:, frozen] == 0).all()) and bool((un[:, frozen] == 0).all())
    assert bool((gn[:, ~frozen] > 0).all()) and bool((un[:, ~frozen] > 0).all())
    assert torch.equal(_bits(tr.params), _bits(flat))      # (the record only reads)


def test_capture_of_a_step_with_rates_raises_and_the_step_still_runs():
    """7. capture() raises for each of the three options; the step then runs eagerly, as the one that was never asked"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    key = ("tiny", False)
    run = _runs.get(key) or _runs.setdefault(key, _Run(*key))
    for opts in ({"freeze": ("frame_dim_reshape_*",)}, {"lr_scale": {"cross_*": 0.5}}, {"decay_scale": {"*.bias": 0.0}}):
        ts = run.step(**opts)
        with pytest.raises(run.lib_mod.SdumcError, match="capture"):
            ts.capture()
        assert ts.graph is None
        ts.run()
        again = run.step(**opts)
        again.run()
        _same(_state(ts), _state(again), str(opts), KEYS + ("grads",))
        assert bool(torch.isfinite(ts.params).all()) and not torch.equal(ts.params, run.S0["params"])
