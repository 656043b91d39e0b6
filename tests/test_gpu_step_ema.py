"""Averaged weights in the fused step (TrainStep / FusedTrainer: ema_decay=, ema_warmup=; sdumc_step_cfg.ema; csrc/engine.hip,
csrc/adam.hip): the EMA form of the step's last launch.

The four shapes of tests/test_gpu_step_rates.py (lens, ragged, tiny, odd), each in fp32 and with bf16=True, three steps from that
file's state S0 (its _Run: the inputs, random moments, step count 3, dropout counter 6, and three steps of the plain TrainStep), train
mode, one seed on both sides.

  read-only   parameters, both moments, losses, hyper, the dropout counter and the gradient bucket are bit-equal after every step to the
              plain TrainStep on a copy -- also with freeze= / lr_scale= on both sides;
  the rule    the EMA after step k from the EMA before step k and the parameters AFTER step k (both snapshotted around the step):
              torch.lerp's bits for w in {0.25, 0.5, 1}, within 2 * 2^-23 * max(|a|, |p|) of the fp64 rule otherwise
              (tests/ema_ref.py); the parameters BEFORE the step miss that bound, so the check cannot pass for the wrong reason."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ema_ref  # noqa: E402
from tests import test_gpu_step_rates as R  # noqa: E402      (its shapes, its S0 and its plain steps: one cache of them per session)

pytestmark = pytest.mark.gpu

CONFIGS = R.CONFIGS
KEYS = R.KEYS + ("grads",)
_bits, _state, _same = R._bits, R._state, R._same


@pytest.fixture
def run(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if request.param not in R._runs:
        R._runs[request.param] = R._Run(*request.param)
    return R._runs[request.param]


both = pytest.mark.parametrize("run", CONFIGS, indirect=True, ids=[f"{s}-{'bf16' if b else 'fp32'}" for s, b in CONFIGS])


def _ema(ts):
    torch.cuda.synchronize()
    return ts.ema_params.clone()


def _check_rule(run, before, after, params_after, w, what, skip=None):
    """the EMA over the live bucket by the rule (skip: a mask of elements that must keep their bits instead); the tail of parameters
    that never get a gradient keeps the initial bits"""
    live = run.lay.live
    a0, a1, p = before[:live], after[:live], params_after[:live]
    keep = torch.zeros(live, dtype=torch.bool, device="cuda") if skip is None else skip
    ratio = ema_ref.check(a1[~keep], a0[~keep], p[~keep], w, what)
    assert torch.equal(_bits(a1[keep]), _bits(a0[keep])), f"{what}: an average that must not move did"
    assert torch.equal(_bits(after[live:]), _bits(run.S0["params"][live:])), f"{what}: the tail of dead parameters"
    return ratio


@both
def test_the_run_is_the_plain_run_and_the_average_obeys_the_rule(run):
    """decay 0.9 and 0.999 (the bound), 0.75 and 0.5 (bit equality): three steps each"""
    live = run.lay.live
    for decay in (0.9, 0.999, 0.75, 0.5):
        ts = run.step(ema_decay=decay)
        assert ts.ema_params is not None and ts.ema_params.numel() == run.lay.total and ts.ema_params.data_ptr() != ts.params.data_ptr()
        assert bool(ts.cfg.ema) and ts.cfg.ema_decay == np.float32(decay) and ts.cfg.ema_warmup == 0
        assert torch.equal(_bits(_ema(ts)), _bits(run.S0["params"]))      # the average starts as a copy
        w, worst = ema_ref.weight(decay), 0.0
        for k in range(3):
            before, p_before = _ema(ts), ts.params.clone()
            ts.run()
            got = _state(ts)
            _same(got, run.plain[k], f"decay {decay}, step {k}", KEYS)
            after = _ema(ts)
            worst = max(worst, _check_rule(run, before, after, got["params"], w, f"decay {decay}, step {k}"))
            if decay == 0.9:
                # the reading that must fail: the parameters before the update
                wrong = ema_ref.worst(after[:live], before[:live], p_before[:live], w)
                print(f"decay 0.9, step {k}: the pre-update reading is {wrong:.1f} units of the bound off")
                assert wrong > 1.0
        print(f"decay {decay}: worst ratio to the bound over three steps {worst:.4f}")
    plain = run.step()
    assert plain.ema_params is None and not bool(plain.cfg.ema) and plain.cfg.ema_decay == 0.0


@both
def test_decay_zero_holds_the_parameters_bits(run):
    ts = run.step(ema_decay=0)
    live = run.lay.live
    for k in range(3):
        ts.run()
        got, a = _state(ts), _ema(ts)
        _same(got, run.plain[k], f"step {k}", KEYS)
        assert torch.equal(_bits(a[:live]), _bits(got["params"][:live])), k
        assert torch.equal(_bits(a[live:]), _bits(run.S0["params"][live:])), k
    assert not torch.equal(a[:live], run.S0["params"][:live])


@both
def test_with_frozen_and_scaled_tensors_on_both_sides(run):
    """freeze= / lr_scale= / decay_scale= on both sides: the run is the rates run, bit for bit; a frozen tensor's average keeps its
    initial bits over the three steps; an lr_scale = 0 tensor is updated by the rule (its parameter stays, so its average stays)"""
    opts = dict(freeze=R.FREEZE, lr_scale={"cross_*": 0.5, "fc_out_v.*": 0}, decay_scale={"*.bias": 0.0})
    ts, ref = run.step(ema_decay=0.9, **opts), run.step(**opts)
    frozen = [n for n, f in zip(ts.rates.names, ts.rates.frozen) if f]
    fmask = run.mask(frozen)
    w = ema_ref.weight(0.9)
    for k in range(3):
        before = _ema(ts)
        ts.run()
        ref.run()
        got = _state(ts)
        _same(got, _state(ref), f"step {k}", KEYS)
        _check_rule(run, before, _ema(ts), got["params"], w, f"rates, step {k}", skip=fmask)
    a = _ema(ts)
    for name in frozen:
        off, n = run.segs[name]
        assert torch.equal(_bits(a[off:off + n]), _bits(run.S0["params"][off:off + n])), name
    for name in ("fc_out_v.weight", "fc_out_v.bias"):
        off, n = run.segs[name]
        assert torch.equal(_bits(a[off:off + n]), _bits(run.S0["params"][off:off + n])), name
        assert torch.equal(_bits(got["params"][off:off + n]), _bits(run.S0["params"][off:off + n])), name
    assert not torch.equal(a[:run.lay.live][~fmask], run.S0["params"][:run.lay.live][~fmask])


@both
def test_a_skipped_step_leaves_the_average_alone_and_the_warmup_follows_the_count_the_guard_left(run):
    """skip_nonfinite=True with one NaN label: the skipped step leaves the EMA bit-identical; the next, finite step updates it by the
    rule, with the warm-up weight of step count T0 + 1 -- the count the guard took back -- and not of T0 + 2"""
    for warm in (True, False):
        ts = run.step(nan_label=True, skip_nonfinite=True, ema_decay=0.999, ema_warmup=warm)
        start = _ema(ts)
        ts.run()
        got = _state(ts)
        assert ts.guard.tolist()[3] == 1.0 and float(got["hyper"][1]) == R.T0
        assert torch.equal(_bits(_ema(ts)), _bits(start)) and torch.equal(_bits(got["params"]), _bits(run.S0["params"]))
        ts.set_batch(*run.batch[:4], run.batch[4])      # the same batch with its finite labels
        ts.run()
        got, after = _state(ts), _ema(ts)
        assert ts.guard.tolist()[3] == 0.0 and float(got["hyper"][1]) == R.T0 + 1
        assert not torch.equal(got["params"], run.S0["params"])
        w = ema_ref.weight(0.999, R.T0 + 1, warmup=warm)
        _check_rule(run, start, after, got["params"], w, f"the step after the skipped one, warm-up {warm}")
        if warm:
            live = run.lay.live
            assert w == float(np.float32(1.0 - (1.0 + R.T0 + 1) / (10.0 + R.T0 + 1)))
            assert ema_ref.worst(after[:live], start[:live], got["params"][:live], ema_ref.weight(0.999, R.T0 + 2, warmup=True)) > 1.0
            # ... and a guarded run without a skipped step is three steps of the schedule
            ts = run.step(skip_nonfinite=True, ema_decay=0.999, ema_warmup=True)
            for k in range(3):
                before = _ema(ts)
                ts.run()
                got = _state(ts)
                _same(got, run.plain[k], f"guarded, step {k}", ("params", "adam_m", "adam_v", "hyper", "call", "grads"))
                _check_rule(run, before, _ema(ts), got["params"], ema_ref.weight(0.999, R.T0 + 1 + k, warmup=True), f"warm-up, step {k}")


@both
def test_resume_and_reset(run):
    """load_ema, then a step, equals an uninterrupted run's EMA bit for bit; reset_ema gives the parameters' bits"""
    whole = run.step(ema_decay=0.9, ema_warmup=True)
    whole.run()
    torch.cuda.synchronize()
    saved = {"params": whole.params.clone(), "m": whole.adam_m.clone(), "v": whole.adam_v.clone(), "ema": whole.ema_params.cpu().clone()}
    whole.run()
    # the resumed run: the state after one step, the average installed from the host copy
    from sdumc_amd import _lib
    ts = run.engine.TrainStep(saved["params"].clone(), run.B, run.T, run.dims, lr=R.LR, weight_decay=R.WD, seed=R.SEED, bf16=run.bf16,
                              ema_decay=0.9, ema_warmup=True)
    ts.load_optimizer_state(saved["m"], saved["v"], R.T0 + 1)
    ts.load_ema(saved["ema"])
    ts.set_batch(*run.batch[:5])
    if run.lens is not None:
        ts.set_lengths(run.lens)
    ts.run()
    torch.cuda.synchronize()
    assert torch.equal(_bits(ts.params), _bits(whole.params))
    assert torch.equal(_bits(ts.ema_params), _bits(whole.ema_params))
    assert not torch.equal(ts.ema_params, ts.params)
    for bad in (saved["ema"][:-1], saved["ema"].double(), None):
        with pytest.raises(_lib.SdumcError, match="load_ema"):
            ts.load_ema(bad)
    ts.reset_ema()
    torch.cuda.synchronize()
    assert torch.equal(_bits(ts.ema_params), _bits(ts.params))
    with pytest.raises(_lib.SdumcError, match="keeps no averaged weights"):
        run.step().reset_ema()


def _trainer_env(bf16):
    from oracle import sdumc_oracle as O
    from sdumc_amd import engine as E
    from sdumc_amd.data import DeviceFeatureStore
    dims = (128, 128, 128, 128) if bf16 else (64, 128, 64, 128)
    tcap, n = (40, 9, 24, 8), 12
    P = O.init_params(dims, seed=8)
    lay = E.ParamLayout.get(*dims[:3])
    flat0 = torch.zeros(lay.total)
    for k, v in lay.views(flat0).items():
        v.copy_(P[k])
    store = DeviceFeatureStore.synthetic(n, tcap, dims, seed=5, min_frac=0.25, **({"bf16": True} if bf16 else {"planes": True}))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    batches = [perm[0:5].clone(), perm[5:8].clone(), perm[8:12].clone()]
    assert len({store.batch_shape(ix) for ix in batches}) >= 2

    def trainer(**kw):
        return E.FusedTrainer(flat0.clone().cuda(), dims, lr=R.LR, seed=11, capacity=(5, tcap), weight_decay=R.WD, bf16=bf16, **kw)

    return E, lay, dims, store, batches, flat0, trainer


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_one_average_across_the_shapes_of_a_fused_trainer(bf16):
    """FusedTrainer(capacity=) over a 12-utterance store, two batch shapes: one ema_params tensor across the shapes; run_epoch leaves
    the same EMA bits as the same batches through step_from_store, and each step obeys the rule"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    E, lay, dims, store, batches, flat0, trainer = _trainer_env(bf16)
    opts = dict(ema_decay=0.9, ema_warmup=True, freeze=("frame_dim_reshape_1.*",))
    tr = trainer(**opts)
    assert tr.ema_params is tr.state.ema_params and tr.ema_params.numel() == lay.total
    assert torch.equal(_bits(tr.ema_params), _bits(flat0.cuda())) and tr.ema_params.data_ptr() != tr.params.data_ptr()
    tr.run_epoch(store, batches)
    torch.cuda.synchronize()
    assert len(tr._steps) >= 2 and all(ts.ema_params is tr.ema_params for ts in tr._steps.values())
    one = trainer(**opts)
    frozen = torch.zeros(lay.live, dtype=torch.bool)
    for name, fr in zip(one.rates.names, one.rates.frozen):
        if fr:
            off, shape, _ = lay.entries[name]
            frozen[off:off + int(np.prod(shape))] = True
    frozen = frozen.cuda()
    for k, ix in enumerate(batches):
        before = one.ema_params.clone()
        one.step_from_store(store, ix)
        torch.cuda.synchronize()
        a, p = one.ema_params[:lay.live], one.params[:lay.live]
        ema_ref.check(a[~frozen], before[:lay.live][~frozen], p[~frozen], ema_ref.weight(0.9, k + 1, warmup=True), f"batch {k}")
        assert torch.equal(_bits(a[frozen]), _bits(flat0.cuda()[:lay.live][frozen]))
    assert torch.equal(_bits(tr.params), _bits(one.params))
    assert torch.equal(_bits(tr.ema_params), _bits(one.ema_params))
    # ... and the option off is the trainer without it
    off_tr = trainer(freeze=("frame_dim_reshape_1.*",))
    off_tr.run_epoch(store, batches)
    torch.cuda.synchronize()
    assert off_tr.ema_params is None and torch.equal(_bits(off_tr.params), _bits(tr.params))
    from sdumc_amd import _lib
    with pytest.raises(_lib.SdumcError, match="without averaged weights"):
        off_tr.eval_epoch(store, batches, weights="ema")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_evaluation_and_saliency_over_the_average(bf16):
    """eval_epoch(weights='ema') is bit-equal to evaluate.eval_epoch over a clone of the average and differs from weights='params';
    saliency_epoch(weights='ema') likewise, in fp32 storage; neither call changes any training state"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import evaluate, saliency
    E, lay, dims, store, batches, flat0, trainer = _trainer_env(bf16)
    tr = trainer(ema_decay=0.5)
    tr.run_epoch(store, batches)
    torch.cuda.synchronize()
    assert not torch.equal(tr.ema_params, tr.params)

    def snapshot():
        torch.cuda.synchronize()
        s = tr.state
        return [t.clone() for t in (tr.params, tr.ema_params, s.adam_m, s.adam_v, s.hyper, s.losses)] + [s.rng.call]

    state = snapshot()
    by_ema = tr.eval_epoch(store, batches, weights="ema", embeddings=True)
    by_params = tr.eval_epoch(store, batches, embeddings=True)
    want = evaluate.eval_epoch(tr.ema_params.clone(), dims, store, batches, bf16=bf16, embeddings=True)
    torch.cuda.synchronize()
    assert bool(by_ema.seen.bool().all())
    assert torch.equal(_bits(by_ema.preds), _bits(want.preds)) and not torch.equal(by_ema.preds, by_params.preds)
    for key in by_ema.embeddings:
        assert torch.equal(_bits(by_ema.embeddings[key]), _bits(want.embeddings[key])), key
    assert tr._evaluator is not tr._evaluator_ema and tr._evaluator_ema.params is tr.ema_params
    # the second evaluator reads the average as it is when the call runs: another epoch moves it, the kept evaluator follows
    kept, first = tr._evaluator_ema, by_ema.preds.clone()
    for a, b in zip(state, snapshot()):
        assert a == b if isinstance(a, int) else torch.equal(_bits(a), _bits(b))
    tr.run_epoch(store, batches)
    later = tr.eval_epoch(store, batches, weights="ema")
    want = evaluate.eval_epoch(tr.ema_params.clone(), dims, store, batches, bf16=bf16)
    torch.cuda.synchronize()
    assert tr._evaluator_ema is kept and torch.equal(_bits(later.preds), _bits(want.preds))
    assert not torch.equal(later.preds, first)
    if bf16:
        return
    state = snapshot()
    sal = tr.saliency_epoch(store, batches, weights="ema")
    sal_params = tr.saliency_epoch(store, batches)
    want = saliency.saliency_epoch(tr.ema_params.clone(), dims, store, batches)
    torch.cuda.synchronize()
    assert torch.equal(_bits(sal.preds), _bits(want.preds)) and not torch.equal(sal.preds, sal_params.preds)
    for s, mods in sal.maps.items():
        for m, t in mods.items():
            assert torch.equal(_bits(t), _bits(want.maps[s][m])), (s, m)
            assert not torch.equal(t, sal_params.maps[s][m]), (s, m)
    for a, b in zip(state, snapshot()):
        assert a == b if isinstance(a, int) else torch.equal(_bits(a), _bits(b))


def test_capture_of_a_step_with_an_average_raises_and_the_step_still_runs():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    key = ("tiny", False)
    run = R._runs.get(key) or R._runs.setdefault(key, R._Run(*key))
    ts = run.step(ema_decay=0.999)
    with pytest.raises(run.lib_mod.SdumcError, match="capture"):
        ts.capture()
    assert ts.graph is None
    ts.run()
    _same(_state(ts), run.plain[0], "after the refused capture", KEYS)
