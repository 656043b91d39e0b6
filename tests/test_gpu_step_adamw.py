"""Decoupled weight decay in the fused step (TrainStep / FusedTrainer: decoupled_decay=True; sdumc_step_cfg.decoupled_decay;
csrc/engine.hip, csrc/adam.hip).

Everything is bit equality against the code that was there before.  The reference of ONE step: the reference state is copied into a
plain TrainStep, which runs for its losses, its dropout counter and its gradient bucket; its update is discarded, and the rule of
tests/test_gpu_adamw.py is applied by the test to the pre-step state with that bucket --
    no table   p.mul_(dk) by torch, dk = fp32(1 - fp32(lr) * fp32(wd)) computed by the test, then ops.adam_step(weight_decay=0);
    a table    the same tensor by tensor with lr * lr_scale and dk = fp32(1 - (lr * lr_scale) * (wd * decay_scale)), frozen tensors
               left alone, the alignment padding between tensors as without a table.
Three steps per case, the learning rate changed before the second and the third (set_lr: the factor follows hyper[0]).

Shapes and start state are those of tests/test_gpu_step_rates.py: `tiny`, `odd`, `ragged`, `lens` (with key-padding lengths), each in
fp32 and with bf16=True, train mode with Philox masks; every run starts from S0: the initial parameters, random moments (second
moment >= 0), step count 3, dropout counter 6."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import adamw_ref  # noqa: E402
import ema_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
LRS, WD, SEED, T0 = (1e-3, 4e-4, 2e-3), 1e-2, 3, 3
LENS = ([70, 12, 65, 1], [9, 3, 1, 8], [33, 33, 2, 17], [6, 1, 4, 5])
#         dims                  B  T                lengths
SHAPES = {"lens": ((128, 128, 128, 128), 4, (70, 9, 33, 6), True),
          "ragged": ((64, 192, 64, 192), 3, (65, 1, 64, 2), False),
          "tiny": ((48, 32, 40, 32), 4, (13, 5, 9, 3), False),
          "odd": ((37, 32, 42, 32), 4, (13, 5, 9, 3), False)}
CONFIGS = [(s, b) for s in SHAPES for b in (False, True)]
KEYS = ("params", "adam_m", "adam_v", "losses", "hyper", "call")
RATES = dict(freeze=("frame_dim_reshape_1.*",), lr_scale={"cross_*": 0.5, "fc_out_v.*": 2.0, "fra2utt_1.*": 0.25},
             decay_scale={"*.bias": 0.0, "*.attention_context_vector": 0.0, "fc_att.weight": 0.5})


def _bits(t):
    return t.contiguous().view(torch.int32)


def _state(ts):
    torch.cuda.synchronize()
    return {"params": ts.params.clone(), "adam_m": ts.adam_m.clone(), "adam_v": ts.adam_v.clone(), "losses": ts.losses.clone(),
            "hyper": ts.hyper.clone(), "call": ts.rng.call, "grads": ts.grads.clone()}


def _same(a, b, what, keys=KEYS):
    for k in keys:
        if k == "call":
            assert a[k] == b[k], (what, k, a[k], b[k])
            continue
        bad = torch.nonzero(_bits(a[k]) != _bits(b[k])).flatten()
        assert bad.numel() == 0, (what, k, f"{bad.numel()} of {a[k].numel()} elements differ, the first at {bad[:6].tolist()}")


class _Run:
    """One (shape, storage) setting: the inputs, S0, and the reference chains the cases share"""

    def __init__(self, shape, bf16):
        from oracle import sdumc_oracle as O
        from sdumc_amd import _lib, engine, ops
        self.engine, self.lib_mod, self.ops = engine, _lib, ops
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
        self.segs = {name: (lay.entries[name][0], int(np.prod(lay.entries[name][1]))) for name in lay.live_names()}
        self.S0 = _state(self.step())
        self._chains = {}

    def step(self, nan_label=False, **kw):
        ts = self.engine.TrainStep(self.flat.clone(), self.B, self.T, self.dims, lr=LRS[0], weight_decay=WD, seed=SEED, bf16=self.bf16,
                                   **kw)
        ts.load_optimizer_state(self.m0, self.v0, T0)
        self.labels(ts, nan_label)
        if self.lens is not None:
            ts.set_lengths(self.lens)
        return ts

    def labels(self, ts, nan_label):
        labels = self.batch[4].clone()
        if nan_label:
            labels[1] = float("nan")
        ts.set_batch(*self.batch[:4], labels)

    def mask(self, names):
        m = torch.zeros(self.lay.live, dtype=torch.bool)
        for name in names:
            off, n = self.segs[name]
            m[off:off + n] = True
        return m.cuda()

    def rule(self, pre, bucket, lr, rates=None):
        """the rule applied to the pre-step state (params, adam_m, adam_v, hyper) with `bucket`: -> (params, m, v), whole buffers"""
        ops, live = self.ops, self.lay.live
        t = float(pre["hyper"][1])

        def one(p, g, m, v, lr_i, dk):
            p.mul_(torch.tensor(dk, dtype=torch.float32, device="cuda"))
            ops.adam_step(p, g, m, v, torch.tensor([lr_i, t, 0.0, 0.0], device="cuda"), weight_decay=0.0)

        p, m, v = pre["params"][:live].clone(), pre["adam_m"].clone(), pre["adam_v"].clone()
        dk = np.float32(1 - float(np.float32(lr)) * float(np.float32(WD)))
        assert dk == adamw_ref.decay_factor(lr, WD) and dk < 1
        one(p, bucket.clone(), m, v, lr, dk)
        if rates is not None:      # (the padding between tensors keeps what the whole-bucket rule just gave it)
            for name, ls, ws, fr in zip(rates.names, rates.lr_scale, rates.decay_scale, rates.frozen):
                off, n = self.segs[name]
                src = (pre["params"], pre["adam_m"], pre["adam_v"])
                pi, mi, vi = (x[off:off + n].clone() for x in src)
                if not fr:
                    lr_i = float(np.float32(lr) * np.float32(ls))
                    assert lr_i == float(np.float32(lr)) * float(ls)      # a power of two (or one): exact
                    one(pi, bucket[off:off + n].clone(), mi, vi, lr_i, adamw_ref.decay_factor(lr, WD, ls, ws))
                p[off:off + n], m[off:off + n], v[off:off + n] = pi, mi, vi
        params = pre["params"].clone()
        params[:live] = p
        torch.cuda.synchronize()
        return params, m, v

    def chain(self, key, rates=None, coef=None):
        """three reference steps from S0 (cached under `key`): [(state after the step, the plain step's bucket)]; coef: per step, the
        factor the guard scaled the bucket by"""
        if key in self._chains:
            return self._chains[key]
        ref = self.step()
        pre, out = dict(self.S0), []
        for k, lr in enumerate(LRS):
            ref.params.copy_(pre["params"]), ref.adam_m.copy_(pre["adam_m"]), ref.adam_v.copy_(pre["adam_v"])
            ref.set_lr(lr)
            ref.run()
            got = _state(ref)
            bucket = got["grads"]
            if rates is not None:
                bucket = bucket.clone()
                bucket[self.mask([n for n, f in zip(rates.names, rates.frozen) if f])] = 0.0
            if coef is not None:
                bucket = bucket * coef[k]
            pre_k = dict(pre, hyper=torch.tensor([lr, T0 + k, 0.0, 0.0], device="cuda"))
            p, m, v = self.rule(pre_k, bucket, lr, rates)
            pre = dict(got, params=p, adam_m=m, adam_v=v, grads=bucket)
            out.append(pre)
        self._chains[key] = out
        return out


_runs = {}


@pytest.fixture
def run(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if request.param not in _runs:
        _runs[request.param] = _Run(*request.param)
    return _runs[request.param]


both = pytest.mark.parametrize("run", CONFIGS, indirect=True, ids=[f"{s}-{'bf16' if b else 'fp32'}" for s, b in CONFIGS])


def _three(ts, want, what, keys=KEYS + ("grads",)):
    for k, lr in enumerate(LRS):
        ts.set_lr(lr)
        ts.run()
        _same(_state(ts), want[k], f"{what} step {k}", keys)


@both
def test_decoupled_alone(run):
    """1. parameters, both moments, hyper, losses, the dropout counter and the bucket match the reference after each of three steps"""
    ts = run.step(decoupled_decay=True)
    assert ts.decoupled_decay is True and ts.cfg.decoupled_decay == 1 and ts.rates is None and ts.guard is None
    want = run.chain("plain")
    _three(ts, want, "decoupled")
    assert want[2]["call"] == 2 * T0 + 6 and float(want[2]["hyper"][1]) == T0 + 3
    assert float(want[2]["hyper"][0]) == float(np.float32(LRS[2]))
    # ... which the coupled step is not
    coupled = run.step()
    coupled.run()
    assert not torch.equal(_state(coupled)["params"], want[0]["params"])
    _same(_state(coupled), want[0], "the coupled step's forward and backward", ("losses", "call", "grads"))


@both
def test_with_freeze_and_scales(run):
    """2. freeze + lr_scale + decay_scale (power-of-two scales, '*.bias': 0.0, a frozen frame projection): each tensor matches the rule
    with its own scales; a frozen tensor is untouched and its segment of the bucket is +0.0"""
    ts = run.step(decoupled_decay=True, **RATES)
    rates = ts.rates
    frozen = [n for n, f in zip(rates.names, rates.frozen) if f]
    assert len(frozen) == 2 and any(s == 0.0 for s in rates.decay_scale) and {0.25, 0.5, 2.0} <= set(float(s) for s in rates.lr_scale)
    want = run.chain("rates", rates=rates)
    _three(ts, want, "rates")
    got = _state(ts)
    for name in frozen:
        off, n = run.segs[name]
        for key, init in (("params", run.S0["params"]), ("adam_m", run.m0), ("adam_v", run.v0)):
            assert torch.equal(_bits(got[key][off:off + n]), _bits(init[off:off + n])), (name, key)
    assert not torch.equal(got["params"], run.chain("plain")[2]["params"])


@both
def test_with_clipping(run):
    """3. clip_norm small enough that every step clips: the bucket is the plain step's times guard[1], then the rule"""
    first = run.chain("plain")[0]["grads"]
    clip = 0.05 * float(torch.linalg.vector_norm(first.double()))
    ts = run.step(decoupled_decay=True, clip_norm=clip)
    # the coefficients come from the step under test (its norm is tests/test_gpu_grad_guard.py's matter); the reference chain needs
    # them step by step, so both advance together
    ref, pre = run.step(), dict(run.S0)
    for k, lr in enumerate(LRS):
        ts.set_lr(lr)
        ts.run()
        got = _state(ts)
        coef = ts.guard[1].clone()
        assert 0.0 < float(coef) < 1.0 and ts.guard[2:].tolist() == [0.0, 0.0]
        ref.params.copy_(pre["params"]), ref.adam_m.copy_(pre["adam_m"]), ref.adam_v.copy_(pre["adam_v"])
        ref.set_lr(lr)
        ref.run()
        plain = _state(ref)
        bucket = plain["grads"] * coef
        p, m, v = run.rule(dict(pre, hyper=torch.tensor([lr, T0 + k, 0.0, 0.0], device="cuda")), bucket, lr)
        pre = dict(plain, params=p, adam_m=m, adam_v=v, grads=bucket)
        _same(got, pre, f"clipped step {k}", KEYS + ("grads",))


@both
def test_a_skipped_step_decays_nothing(run):
    """4. skip_nonfinite=True and a NaN label: state and step count bit for bit unchanged, the dropout counter advances; the next step
    equals the unguarded decoupled step from that state"""
    ts = run.step(nan_label=True, decoupled_decay=True, skip_nonfinite=True)
    ts.run()
    got, guard = _state(ts), ts.guard.tolist()
    assert guard[3] == 1.0 and guard[2] > 0
    for key, init in (("params", run.S0["params"]), ("adam_m", run.m0), ("adam_v", run.v0)):
        assert torch.equal(_bits(got[key]), _bits(init)), key
    assert float(got["hyper"][1]) == T0 and got["call"] == 2 * T0 + 2 and float(got["losses"][7]) == 0.0
    run.labels(ts, False)
    ts.run()
    plain = run.step(decoupled_decay=True)
    plain.rng.set_call(2 * T0 + 2)
    plain.run()
    assert ts.guard.tolist()[2:] == [0.0, 0.0]
    _same(_state(ts), _state(plain), "the step behind a skipped one", KEYS + ("grads",))
    assert not torch.equal(ts.params, run.S0["params"])


@both
def test_with_the_average(run):
    """5. ema_decay=0.75, ema_warmup=True: the average follows tests/ema_ref.py's rule on the post-step parameters; parameters and
    moments are those of case 1; a skipped step leaves the average alone"""
    ts = run.step(decoupled_decay=True, ema_decay=0.75, ema_warmup=True, skip_nonfinite=True)
    want, live = run.chain("plain"), run.lay.live
    assert torch.equal(_bits(ts.ema_params), _bits(run.S0["params"]))
    for k, lr in enumerate(LRS):
        before = ts.ema_params.clone()
        ts.set_lr(lr)
        ts.run()
        _same(_state(ts), want[k], f"with an average, step {k}", KEYS + ("grads",))
        w = ema_ref.weight(0.75, T0 + k + 1, True)
        ema_ref.check(ts.ema_params[:live], before[:live], ts.params[:live], w, f"step {k}")
        assert torch.equal(_bits(ts.ema_params[live:]), _bits(before[live:]))
    assert ema_ref.weight(0.75, T0 + 3, True) > ema_ref.weight(0.75, T0 + 30, True) == 0.25      # (these steps are inside the warm-up)
    run.labels(ts, True)
    before, p_before = ts.ema_params.clone(), ts.params.clone()
    ts.run()
    torch.cuda.synchronize()
    assert ts.guard.tolist()[3] == 1.0
    assert torch.equal(_bits(ts.ema_params), _bits(before)) and torch.equal(_bits(ts.params), _bits(p_before))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_fused_trainer_over_a_ragged_store(bf16):
    """6. FusedTrainer(decoupled_decay=True) over a four-batch ragged epoch of two shapes: run_epoch equals the same steps made one by
    one through TrainSteps sharing one state.  train_epoch(by_tensor='updates'): update_norm is the norm of theta_after - theta_before
    of that chain within the record's one ulp; on the first step a tensor with decay_scale 0 has, bit for bit, the update_norm of a
    run with weight_decay=0 (dk == 1), a tensor with decay has another."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle import sdumc_oracle as O
    from sdumc_amd import engine as E
    from sdumc_amd.data import DeviceFeatureStore
    dims = (128, 128, 128, 128) if bf16 else (64, 128, 64, 128)
    tcap, n, lr = (40, 9, 24, 8), 20, LRS[0]
    P = O.init_params(dims, seed=8)
    lay = E.ParamLayout.get(*dims[:3])
    flat0 = torch.zeros(lay.total)
    for k, v in lay.views(flat0).items():
        v.copy_(P[k])
    store = DeviceFeatureStore.synthetic(n, tcap, dims, seed=5, min_frac=0.25, **({"bf16": True} if bf16 else {"planes": True}))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    batches = [perm[0:6].clone(), perm[6:10].clone(), perm[10:16].clone(), perm[16:20].clone()]
    assert len({store.batch_shape(ix) for ix in batches}) >= 2
    opts = dict(decay_scale={"*.bias": 0.0})

    def trainer(wd=0.1):
        return E.FusedTrainer(flat0.clone().cuda(), dims, lr=lr, seed=11, capacity=(6, tcap), weight_decay=wd, bf16=bf16,
                              decoupled_decay=True, **opts)

    tr, ls = trainer(), []
    assert tr.decoupled_decay is True
    tr.run_epoch(store, batches, on_step=lambda i, l: ls.append(l.clone()))
    torch.cuda.synchronize()
    assert all(ts.decoupled_decay and ts.cfg.decoupled_decay == 1 for ts in tr._steps.values()) and len(tr._steps) >= 2
    # the chain
    flat = flat0.clone().cuda()
    state, chain, thetas = E._RunState(flat, lay.live, lr, 11), [], [flat.clone()]
    for ix in batches:
        b, _, _, vals, _ = store.batch(ix)
        ts = E.TrainStep(flat, *store.batch_shape(ix), dims, share=state, weight_decay=0.1, bf16=bf16, bits_next=False, rates=tr.rates,
                         decoupled_decay=True, **({} if bf16 else {"planes": True}))
        ts.set_batch(b["audios"], b["texts"], b["videos"], b["feat4s"], vals)
        chain.append(ts.run().clone())
        torch.cuda.synchronize()
        thetas.append(flat.clone())
    for i, (x, y) in enumerate(zip(ls, chain)):
        assert torch.equal(_bits(x), _bits(y)), (i, x.tolist(), y.tolist())
    assert torch.equal(_bits(tr.params), _bits(flat)) and torch.equal(_bits(tr.state.adam_m), _bits(state.adam_m))
    assert torch.equal(_bits(tr.state.adam_v), _bits(state.adam_v))
    # the record by tensor
    tr = trainer()
    bt = tr.train_epoch(store, batches, by_tensor="updates").by_tensor
    none = trainer(wd=0.0).train_epoch(store, batches, by_tensor="updates").by_tensor
    torch.cuda.synchronize()
    assert torch.equal(_bits(tr.params), _bits(flat)) and bt.steps == 4
    un = bt.update_norm[:4].cpu()
    for i in range(4):
        d = thetas[i + 1] - thetas[i]
        for k, (o, c) in enumerate(zip(bt.offsets, bt.counts)):
            want = float(torch.linalg.vector_norm(d[o:o + c].double()))
            assert abs(float(un[i, k]) - want) <= ULP * want, (i, bt.names[k], float(un[i, k]), want)
    no_decay = torch.tensor([s == 0.0 for s in tr.rates.decay_scale])
    assert 0 < int(no_decay.sum()) < len(bt.names)
    first, first_none = _bits(bt.update_norm[0].cpu()), _bits(none.update_norm[0].cpu())
    assert torch.equal(first[no_decay], first_none[no_decay])
    differ = (first[~no_decay] != first_none[~no_decay]).float().mean()      # (a tensor that starts at zero has nothing to decay)
    assert float(differ) > 0.5, float(differ)


def _launch_names(lib_mod, call):
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
    return {arr[i].name.decode(): (int(arr[i].launches), float(arr[i].total_flops)) for i in range(n) if arr[i].launches}


@both
def test_the_option_off_is_the_step_that_was_there(run):
    """7. decoupled_decay=False: the launch report's list and every bit are those of a step built without the keyword -- and the
    option on changes no launch of that list either (the last launch is no GEMM)"""
    off, without, on = run.step(decoupled_decay=False), run.step(), run.step(decoupled_decay=True)
    assert off.cfg.decoupled_decay == 0 and off.decoupled_decay is False
    reports = []
    for ts in (off, without, on):
        reports.append(_launch_names(run.lib_mod, ts.run))
    assert reports[0] == reports[1] == reports[2] and reports[0]
    for k in range(2):
        _same(_state(off), _state(without), f"option off, step {k}", KEYS + ("grads",))
        off.run(), without.run()
    assert not torch.equal(_state(on)["params"], _state(off)["params"])


def test_capture_raises_and_launches_nothing():
    """8. capture() of a decoupled step raises "not built" before anything is enqueued: the state is S0's, and the step then runs
    eagerly as one that was never asked"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    key = ("tiny", False)
    run = _runs.get(key) or _runs.setdefault(key, _Run(*key))
    ts = run.step(decoupled_decay=True)
    with pytest.raises(run.lib_mod.SdumcError, match="capture: a step with decoupled_decay is not captured \\(not built\\)"):
        ts.capture()
    assert ts.graph is None
    _same(_state(ts), run.S0, "after the refused capture")
    ts.run()
    _same(_state(ts), run.chain("plain")[0], "eager after the refused capture")
