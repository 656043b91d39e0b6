"""What an epoch over a resident store enqueues per batch (sdumc_amd/epoch.py: the one loop under FusedTrainer.run_epoch / train_epoch,
Evaluator.eval_epoch and Saliency.saliency_epoch), against the same batches as fixed-shape calls made by hand -- engine.NetCall on
store.batch's padded copies, engine.TrainStep.set_batch + run, the way the "composition bit for bit" tests build them.

Two records of one run, both taken from the run itself: the library's own {GEMM kernel: launches} report (sdumc_profile_enable /
sdumc_profile_report: every GEMM of every forward, backward and step) and the number of calls of each entry point of the C ABI the
loops use.  An epoch must launch the GEMMs of its composition, kernel for kernel, and call its entries plus exactly the documented
per-batch extras: one gather (batch 0's by sdumc_gather_batch, every later one carried by the previous call: sdumc_net_io.prefetch),
one scatter, one export with attention, one reduce per stream; train_epoch is run_epoch plus the record's calls.
The fixture is tests/test_gpu_saliency.py's: 7 ragged utterances at widths (256, 512, 256, 512), a store with planes, batches of 3."""
import collections

import pytest
import torch

from tests.test_gpu_saliency import BATCHES, SHAPES, _Env

pytestmark = pytest.mark.gpu

KEY = "kernel"
ENTRIES = ("sdumc_gather_batch", "sdumc_net_forward", "sdumc_net_backward", "sdumc_net_export_attention", "sdumc_scatter_rows_multi",
           "sdumc_frame_saliency", "sdumc_train_step", "sdumc_epoch_record", "sdumc_tensor_norms")
CARRIED = "gather carried by a forward / step"


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    e = _Env()
    e.two = e.batches[:2]
    assert len({e.store[KEY].batch_shape(ix) for ix in e.two}) == 2      # two batches, two padded shapes
    return e


def _enqueued(fn):
    """({GEMM kernel name: launches}, {entry point: calls}) of fn(), one lane"""
    from sdumc_amd import _lib
    lib, calls, real = _lib.lib, collections.Counter(), {}

    def counted(name):
        def call(*args):
            calls[name] += 1
            if name in ("sdumc_net_forward", "sdumc_train_step") and args[1]._obj.prefetch:
                calls[CARRIED] += 1
            return real[name](*args)
        return call

    torch.cuda.synchronize()
    try:
        for name in ENTRIES:
            real[name] = getattr(lib, name)
            setattr(lib, name, counted(name))
        lib.sdumc_set_concurrency(0)
        lib.sdumc_profile_enable(1)
        fn()
        torch.cuda.synchronize()
        arr = (_lib.ProfEntry * 32)()
        n = lib.sdumc_profile_report(arr, 32)
    finally:
        lib.sdumc_profile_enable(0)
        lib.sdumc_set_concurrency(1)
        for name, f in real.items():
            setattr(lib, name, f)
    assert n > 0, "sdumc_profile_report failed"
    gemms = {arr[i].name.decode(): int(arr[i].launches) for i in range(n) if arr[i].launches}
    assert gemms, "no GEMM launch was recorded"
    return gemms, dict(calls)


def _hand_forwards(env, backward_stream=None):
    """one NetCall per batch on the padded copies: a forward, and for backward_stream = s the feature-gradient backward of stream s"""
    store, flat = env.store[KEY], env.flat[KEY]
    for ix in env.two:
        b = store.batch(ix)[0]
        B = ix.numel()
        nc = env.E.NetCall(flat, b["audios"], [b["texts"], b["feat4s"]], b["videos"], False, None, planes=True)
        nc.forward()
        if backward_stream is not None:
            s = backward_stream
            seed = torch.zeros(2 * B, 1, device="cuda")
            seed[s * B:(s + 1) * B] = 1.0
            nc.backward(seed, None, None, None, None, feature_grads=(True, s == 0, s == 1, True))


def _plus(calls, extras):
    out = collections.Counter(calls)
    out.update(extras)
    return {k: v for k, v in out.items() if v}


def _compare(what, epoch, hand, extras):
    (g_epoch, c_epoch), (g_hand, c_hand) = epoch, hand
    print(f"{what}: GEMM launches of the epoch {g_epoch}\n{what}: GEMM launches by hand     {g_hand}")
    print(f"{what}: entry calls of the epoch {c_epoch}\n{what}: entry calls by hand     {c_hand}, extras {extras}")
    assert g_epoch == g_hand, what
    assert c_epoch == _plus(c_hand, extras), what


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("attention", [False, True])
def test_eval_epoch_enqueues_its_forwards_and_the_documented_extras(env, attention, inplace):
    n = len(env.two)
    ev = env.evaluate.Evaluator(env.flat[KEY], SHAPES[KEY], inplace=inplace)
    ev.eval_epoch(env.store[KEY], env.two, attention=attention)      # (the arena and the per-shape dims exist: the counted epoch builds nothing)
    epoch = _enqueued(lambda: ev.eval_epoch(env.store[KEY], env.two, attention=attention))
    assert ev._in_place(env.store[KEY]) == inplace
    extras = {"sdumc_gather_batch": 1, CARRIED: n - 1, "sdumc_scatter_rows_multi": n}
    if attention:
        extras["sdumc_net_export_attention"] = n
    _compare(f"eval_epoch(attention={attention}, inplace={inplace})", epoch, _enqueued(lambda: _hand_forwards(env)), extras)


@pytest.mark.parametrize("inplace", [True, False])
def test_saliency_epoch_with_one_stream_enqueues_one_backward_and_one_reduce_per_batch(env, inplace):
    n = len(env.two)
    sal = env.S.Saliency(env.flat[KEY], SHAPES[KEY], inplace=inplace)
    sal.saliency_epoch(env.store[KEY], env.two, streams=("missing",))
    epoch = _enqueued(lambda: sal.saliency_epoch(env.store[KEY], env.two, streams=("missing",)))
    extras = {"sdumc_gather_batch": 1, CARRIED: n - 1, "sdumc_scatter_rows_multi": n, "sdumc_frame_saliency": n}
    _compare(f"saliency_epoch('missing', inplace={inplace})", epoch, _enqueued(lambda: _hand_forwards(env, backward_stream=1)), extras)


def _trainer(env, inplace=True):
    tcap = tuple(int(env.store[KEY].length[m].max()) for m in env.store[KEY].MODS)
    return env.E.FusedTrainer(env.flat[KEY].clone(), SHAPES[KEY], lr=1e-3, seed=11, capacity=(max(len(b) for b in BATCHES), tcap),
                              inplace=inplace)


@pytest.mark.parametrize("inplace", [True, False])
def test_run_epoch_enqueues_its_steps_and_one_gather_per_batch(env, inplace):
    n = len(env.two)
    store, dims = env.store[KEY], SHAPES[KEY]
    tr = _trainer(env, inplace)
    tr.run_epoch(store, env.two)      # (every per-shape step exists)
    epoch = _enqueued(lambda: tr.run_epoch(store, env.two))
    assert tr._in_place(store) == inplace

    def by_hand():      # tests/test_gpu_configs.py's "plain" route: store.batch() tensors installed with set_batch(planes=True)
        flat = env.flat[KEY].clone()
        state = env.E._RunState(flat, env.E.ParamLayout.get(*dims[:3]).live, 1e-3, 11)
        for ix in env.two:
            b, _, _, vals, _ = store.batch(ix)
            ts = env.E.TrainStep(flat, *store.batch_shape(ix), dims, share=state, planes=True, bits_next=False)
            ts.set_batch(b["audios"], b["texts"], b["videos"], b["feat4s"], vals)
            ts.run()

    _compare(f"run_epoch(inplace={inplace})", epoch, _enqueued(by_hand), {"sdumc_gather_batch": 1, CARRIED: n - 1})


@pytest.mark.parametrize("options,record", [({}, ("sdumc_epoch_record",)),
                                            ({"grad_norm": True, "by_tensor": True}, ("sdumc_epoch_record", "sdumc_tensor_norms"))])
def test_train_epoch_is_run_epoch_plus_the_records_calls(env, options, record):
    n = len(env.two)
    store = env.store[KEY]
    tr = _trainer(env)
    rec = tr.train_epoch(store, env.two, **options)
    plain = _enqueued(lambda: tr.run_epoch(store, env.two))
    kept = _enqueued(lambda: tr.train_epoch(store, env.two, out=rec, **options))
    _compare(f"train_epoch({options})", kept, plain, {name: n for name in record})
