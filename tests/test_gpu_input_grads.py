"""Input-feature gradients (sdumc_net_grads.d_audio / d_text / d_video; csrc/frame_dx.hip): the backward of the frame projections
frame_dim_reshape_{0,1,2} (model :193-195, :282-284) through their INPUT.

Kernel level: sdumc_frame_dx against an fp64 product in both arithmetic forms (the split form must be as close to fp64 as the fp32
MFMAs: tests/test_gpu_split.py's judge), every element written, nothing written outside, launches repeatable bit for bit, the row
zeroing exact.  Network level: the three (four) feature gradients against the fp64 oracle with the inputs as leaves, at the project's
gradient bar -- 2e-4 of each tensor's own norm and 2e-4 element-wise (tests/test_gpu_net.py's close) --, the parameter bucket untouched
by the request, key padding, one stream, subsets, a row-mapped batch, the refusals, and the nn.Module route."""
import ctypes as C
import types

import pytest
import torch

from tests.test_gpu_distill import close_norm
from tests.test_gpu_net import close, flat_from
from tests.test_gpu_split import both, judge

pytestmark = pytest.mark.gpu

BAR = 2e-4


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import ops, _lib
    return ops, _lib


@pytest.fixture(scope="module")
def E(env):
    from sdumc_amd import engine
    return engine


# ---------------------------------------------------------------- 3. the kernel against fp64, both arithmetic forms
@pytest.mark.parametrize("M,N", [(1, 256), (63, 256), (64, 256), (65, 256), (200, 4096), (5003, 1024)])
def test_kernel_against_fp64_in_both_arithmetic_forms(env, M, N):
    ops, _lib = env
    g = torch.Generator(device="cuda").manual_seed(1000 * M + N)
    dz = torch.randn(M, 256, device="cuda", generator=g)
    W = torch.randn(256, N, device="cuda", generator=g) / 16
    ref = dz.double() @ W.double()
    ldc, tail = N + 64, 4096      # a guard region behind every row and behind the tensor
    buf = torch.empty(M * ldc + tail, device="cuda")
    Cv = buf[:M * ldc].view(M, ldc)

    def run():
        buf.fill_(float("nan"))
        ops.frame_dx(dz, W, C_out=Cv[:, :N])
        assert not bool(torch.isnan(Cv[:, :N]).any()), "an element of C was not written"
        assert bool(torch.isnan(Cv[:, N:]).all()) and bool(torch.isnan(buf[M * ldc:]).all()), "a store outside C"
        return [Cv[:, :N]]

    f32, split = both(_lib.lib, run)
    judge(f32, split, [ref], f"frame_dx {M}x{N}")
    again = run()[0]
    assert torch.equal(again, split[0]), "two launches differ"
    # the weight packed ahead of the call (W_frag) instead of by it: the same bits
    assert torch.equal(ops.frame_dx(dz, W, W_frag=ops.p3_split_frag_t(W)), split[0])


def test_transposed_packer_is_the_packer_of_the_transpose(env):
    ops, _lib = env
    W = torch.randn(256, 512, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    assert torch.equal(ops.p3_split_frag_t(W), ops.p3_split_frag(W.t().contiguous()))
    wide = torch.randn(256, 640, device="cuda")      # a row stride above N
    assert torch.equal(ops.p3_split_frag_t(wide[:, :512]), ops.p3_split_frag(wide[:, :512].t().contiguous()))


# ---------------------------------------------------------------- 4. row zeroing
@pytest.mark.parametrize("mask", [15, 0])
def test_row_zeroing_is_exact(env, mask):
    ops, _lib = env
    T, N = 11, 512
    lens = [11, 0, 1, 10, 5, 11]
    M = len(lens) * T
    g = torch.Generator(device="cuda").manual_seed(9)
    dz = torch.randn(M, 256, device="cuda", generator=g)
    W = -torch.rand(256, N, device="cuda", generator=g)
    lengths = torch.tensor(lens, dtype=torch.int32, device="cuda")
    pad = (torch.arange(T, device="cuda")[None, :] >= lengths[:, None]).reshape(-1)
    try:
        _lib.lib.sdumc_set_split_(mask)
        plain = ops.frame_dx(dz, W)
        poisoned = dz.clone()
        poisoned[pad] = float("nan")      # padded rows are not multiplied: whatever they hold, the result is +0
        poisoned[T] = 1.0                  # (a row whose product is negative everywhere: -0 would show)
        got = ops.frame_dx(poisoned, W, lengths=lengths, T=T)
    finally:
        _lib.lib.sdumc_set_split_(15)
    assert int(pad.sum()) == 28
    assert bool((got[pad].view(torch.int32) == 0).all()), "a padded row is not +0.0 bit for bit"
    assert torch.equal(got[~pad], plain[~pad])


# ---------------------------------------------------------------- network level
def _douts(V, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(V, 1, generator=g), torch.randn(V, 128, generator=g), torch.randn(V, 64, generator=g),
            torch.randn(V, 256, generator=g), torch.randn(V, 7, 128, generator=g)]


def _oracle(P, audio, texts, video, mode, seed, call0, douts, lengths=None):
    """tests/test_gpu_net.py's _oracle_grads with the inputs as fp64 leaves too: (parameter gradients, d_audio, [d_text], d_video);
    lengths = (audio, text, video[, feat4]) or None"""
    from oracle import sdumc_oracle as O
    leaves = {k: v.double().requires_grad_(not O.is_dead(k)) for k, v in P.items()}
    a, v = audio.double().requires_grad_(), video.double().requires_grad_()
    tx = [t.double().requires_grad_() for t in texts]
    total = 0
    for s, t in enumerate(tx):
        d = O.DropCtx("eval" if mode == "eval" else "philox", seed, call0 + s)
        ls = None if lengths is None else (lengths[0], lengths[1 if s == 0 else 3], lengths[2])
        y, (z, r, th, ct) = O.forward(leaves, a, t, v, d, lengths=ls)
        B = y.shape[0]
        for o, do in zip((y, z, r, th, ct), douts):
            total = total + (o * do[s * B:(s + 1) * B].double().reshape(o.shape)).sum()
    total.backward()
    return {k: p.grad for k, p in leaves.items() if p.grad is not None}, a.grad, [t.grad for t in tx], v.grad


def _hold(got, want, what):
    close_norm(got, want, BAR, what)
    close(got, want, BAR, what)


def _batch(dims, B, Tn, seed=5):
    from oracle import sdumc_oracle as O
    audio, text, video, feat4, _ = O.synthetic_batch(B, Tn, dims, seed=seed)
    audio[1, Tn[0] * 4 // 7:] = 0      # zero-padded (ragged) samples take part in the softmax like in the reference
    video[B - 1, Tn[2] // 3:] = 0
    return audio, text, video, feat4


SHAPES = {"generic": ((48, 32, 40, 32), 5, (70, 9, 33, 4)),          # widths the kernel does not take: the NN GEMM
          "kernel": ((256, 512, 256, 512), 3, (66, 5, 33, 2))}        # sdumc_frame_dx: M = 198 / 15 / 99 / 6


@pytest.fixture(scope="module")
def params():
    from oracle import sdumc_oracle as O
    return {k: O.init_params(v[0], seed=11) for k, v in SHAPES.items()}


@pytest.mark.parametrize("equal_T", [True, False])
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_feature_gradients_against_the_oracle(E, params, shape, mode, equal_T):
    dims, B, Tn = SHAPES[shape]
    if equal_T:
        Tn = Tn[:3] + (Tn[1],)
    P = params[shape]
    flat, lay = flat_from(E, P, dims)
    audio, text, video, feat4 = _batch(dims, B, Tn)
    seed, call0 = 99, 4
    douts = _douts(2 * B)
    _, wa, wt, wv = _oracle(P, audio, [text, feat4], video, mode, seed, call0, douts)
    rng = E.RngState(seed, "cuda", call=call0)
    call = E.NetCall(flat, audio.cuda(), [text.cuda(), feat4.cuda()], video.cuda(), mode == "train", rng)
    dev = [d.cuda().contiguous() for d in douts]
    call.forward()
    plain = call.backward(*dev).clone()
    assert call.d_inputs == (None, [None, None], None)
    call.forward()
    bucket = call.backward(*dev, feature_grads=True).clone()
    da, dt, dv = call.d_inputs
    _hold(da, wa, "d_audio")
    _hold(dt[0], wt[0], "d_text[0]")
    _hold(dt[1], wt[1], "d_text[1]")
    _hold(dv, wv, "d_video")
    assert torch.equal(bucket, plain), "asking for the feature gradients changed the parameter bucket"
    call.forward()
    call.backward(*dev, feature_grads=True)
    for a, b in zip((da, *dt, dv), (call.d_inputs[0], *call.d_inputs[1], call.d_inputs[2])):
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b), "a second forward / backward gives other feature gradients"


# ---------------------------------------------------------------- 6. key padding
@pytest.mark.parametrize("shape", list(SHAPES))
def test_key_padding_rows_are_exact_zeros(E, params, shape):
    dims, B, Tn = SHAPES[shape]
    P = params[shape]
    flat, _ = flat_from(E, P, dims)
    audio, text, video, feat4 = _batch(dims, B, Tn, seed=8)
    g = torch.Generator().manual_seed(4)
    lens = [torch.randint(1, T + 1, (B,), generator=g) for T in (Tn[0], Tn[1], Tn[2], Tn[3])]
    lens[0][0], lens[2][1] = Tn[0], 1
    douts = _douts(2 * B, seed=6)
    _, wa, wt, wv = _oracle(P, audio, [text, feat4], video, "train", 7, 2, douts, lengths=[l.tolist() for l in lens])
    call = E.NetCall(flat, audio.cuda(), [text.cuda(), feat4.cuda()], video.cuda(), True, E.RngState(7, "cuda", call=2),
                     lengths=tuple(lens[i] for i in (0, 1, 2, 3)))
    call.forward()
    call.backward(*[d.cuda().contiguous() for d in douts], feature_grads=True)
    da, dt, dv = call.d_inputs
    for got, want, l, what in ((da, wa, lens[0], "d_audio"), (dt[0], wt[0], lens[1], "d_text[0]"), (dt[1], wt[1], lens[3], "d_text[1]"),
                               (dv, wv, lens[2], "d_video")):
        pad = torch.arange(got.shape[1])[None, :] >= l[:, None]
        assert bool((want[pad] == 0).all()), "the oracle's padded rows are zero"
        assert bool((got.cpu()[pad].view(torch.int32) == 0).all()), f"{what}: a padded row is not exactly zero"
        _hold(got, want, what)


# ---------------------------------------------------------------- 7. one stream, subsets
def test_one_stream_and_subsets(E, params):
    dims, B, Tn = SHAPES["kernel"]
    P = params["kernel"]
    flat, _ = flat_from(E, P, dims)
    audio, text, video, feat4 = _batch(dims, B, Tn, seed=12)
    seed, call0 = 21, 6
    douts = _douts(2 * B, seed=3)
    one = [[d[s * B:(s + 1) * B].contiguous() for d in douts] for s in range(2)]
    want1 = [_oracle(P, audio, [t], video, "train", seed, call0 + s, one[s]) for s, t in enumerate((text, feat4))]
    # streams == 1, everything asked for
    c1 = E.NetCall(flat, audio.cuda(), [feat4.cuda()], video.cuda(), True, E.RngState(seed, "cuda", call=call0 + 1))
    c1.forward()
    c1.backward(*[d.cuda() for d in one[1]], feature_grads=True)
    _hold(c1.d_inputs[0], want1[1][1], "one stream: d_audio")
    _hold(c1.d_inputs[1][0], want1[1][2][0], "one stream: d_text")
    _hold(c1.d_inputs[2], want1[1][3], "one stream: d_video")
    # a subset: only audio of a two-stream call; the other outputs are not even allocated
    c2 = E.NetCall(flat, audio.cuda(), [text.cuda(), feat4.cuda()], video.cuda(), True, E.RngState(seed, "cuda", call=call0))
    dev = [d.cuda().contiguous() for d in douts]
    c2.forward()
    c2.backward(*dev, feature_grads=(True, False, False, False))
    da, dt, dv = c2.d_inputs
    assert dt == [None, None] and dv is None
    # the same through the C ABI in two phases: phase 0 ignores the fields (a pointer phase 1 would refuse passes), phase 1 writes
    # d_audio alone -- every element -- and the poisoned buffers that were not handed over stay as they were
    _lib, lib = E._lib, E._lib.lib
    outs = c2.forward()
    poison = [torch.full(t.shape, float("nan"), device="cuda") for t in (audio, text, feat4, video)]
    bucket = torch.zeros(c2.layout.live, device="cuda")
    ng = _lib.NetGrads()
    ng.d_vals, ng.d_fused, ng.d_rnc, ng.d_text_hidden, ng.d_cross_text = (t.data_ptr() for t in dev)
    ng.grads, ng.d_audio = bucket.data_ptr(), poison[0].data_ptr() + 4
    args = (C.byref(c2.dims), C.byref(c2.io), C.byref(ng))
    assert lib.sdumc_net_backward_phase(*args, 0, _lib.current_stream()) == 0
    assert lib.sdumc_net_backward_phase(*args, 1, _lib.current_stream()) == -1
    ng.d_audio = poison[0].data_ptr()
    scratch = torch.empty(lib.sdumc_net_feature_grad_scratch_bytes(C.byref(c2.dims)), dtype=torch.uint8, device="cuda")
    ng.feat_scratch, ng.feat_scratch_bytes = scratch.data_ptr(), scratch.numel()
    assert lib.sdumc_net_backward_phase(*args, 1, _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(poison[0], da), "the phased backward gives other bits than the single call"
    assert all(bool(torch.isnan(p).all()) for p in poison[1:])
    # audio of the two-stream call = the sum over the two one-stream calls (one tensor feeds both)
    _hold(da, want1[0][1] + want1[1][1], "two streams: d_audio is the sum over the streams")
    with pytest.raises(E._lib.SdumcError):
        c2.backward(*dev, feature_grads=(True, False))
    with pytest.raises(E._lib.SdumcError):
        c1.backward(*[d.cuda() for d in one[1]], feature_grads=(True, True, True, True))


# ---------------------------------------------------------------- 8. a row-mapped batch
@pytest.mark.parametrize("streams", [1, 2])
def test_row_mapped_batch_gives_the_padded_copys_bits(E, streams):
    from tests.test_gpu_rowmap import _flat_params, _map_io, _net_call, _resident_batch
    rb = _resident_batch(streams, 70)
    flat = _flat_params()
    call = _net_call(flat, rb, streams, True, E.ExecContext())
    outs = call.forward()
    g = torch.Generator(device="cuda").manual_seed(2)
    og = [torch.randn(t.shape, device="cuda", generator=g) for t in outs]
    call.backward(*og, feature_grads=True)
    want = call.d_inputs
    _map_io(call, rb)
    call.forward()
    call.backward(*og, feature_grads=True)
    got = call.d_inputs
    for a, b in zip((want[0], *want[1], want[2]), (got[0], *got[1], got[2])):
        assert float(a.abs().max()) > 0 and a.data_ptr() != b.data_ptr() and torch.equal(a, b)


# ---------------------------------------------------------------- 9. refusals on the device
def test_refusals_leave_everything_untouched(E, env, params):
    ops, _lib = env
    lib = _lib.lib
    dims, B, Tn = SHAPES["kernel"]
    flat, lay = flat_from(E, params["kernel"], dims)
    audio, text, video, feat4 = (t.cuda() for t in _batch(dims, B, Tn))

    def attempt(call, spoil, want_rc, what):
        outs = call.forward()
        og = [torch.ones_like(t) for t in outs]
        grads = torch.full((call.layout.live,), -77.0, device="cuda")
        nb = lib.sdumc_net_feature_grad_scratch_bytes(C.byref(call.dims)) or 4096
        scratch = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        poison = [torch.full((B * T * d + 4,), float("nan"), device="cuda") for T, d in zip(Tn, (dims[0], dims[1], dims[2], dims[3]))]
        ng = _lib.NetGrads()
        ng.d_vals, ng.d_fused, ng.d_rnc, ng.d_text_hidden, ng.d_cross_text = (t.data_ptr() for t in og)
        ng.grads = grads.data_ptr()
        ng.d_audio, ng.d_video = poison[0].data_ptr(), poison[2].data_ptr()
        ng.d_text[0] = poison[1].data_ptr()
        if call.S == 2:
            ng.d_text[1] = poison[3].data_ptr()
        ng.feat_scratch, ng.feat_scratch_bytes = scratch.data_ptr(), nb
        spoil(ng, poison)
        torch.cuda.synchronize()
        args = (C.byref(call.dims), C.byref(call.io), C.byref(ng))
        for fn in (lambda: lib.sdumc_net_backward(*args, _lib.current_stream()),
                   lambda: lib.sdumc_net_backward_phase(*args, 1, _lib.current_stream())):
            assert fn() == want_rc, what
            torch.cuda.synchronize()
            assert bool((grads == -77.0).all()), f"{what}: the refused call wrote the gradient bucket"
            assert all(bool(torch.isnan(p).all()) for p in poison), f"{what}: the refused call wrote an output"

    two = E.NetCall(flat, audio, [text, feat4], video, False, None)
    attempt(two, lambda ng, p: setattr(ng, "d_video", p[2].data_ptr() + 4), -1, "a misaligned output")
    attempt(two, lambda ng, p: setattr(ng, "feat_scratch_bytes", ng.feat_scratch_bytes - 1), -3, "a short scratch")
    attempt(two, lambda ng, p: setattr(ng, "feat_scratch", None), -3, "no scratch")
    one = E.NetCall(flat, audio, [text], video, False, None)
    attempt(one, lambda ng, p: ng.d_text.__setitem__(1, p[3].data_ptr()), -1, "streams == 1 with d_text[1]")
    half = E.NetCall(flat, audio, [text, feat4], video, False, None, bf16=True)
    assert half.dims.bf16 == 2 and lib.sdumc_net_feature_grad_scratch_bytes(C.byref(half.dims)) == 0
    attempt(half, lambda ng, p: None, -1, "bf16 storage")
    outs = half.forward()
    with pytest.raises(_lib.SdumcError):
        half.backward(*[torch.ones_like(t) for t in outs], feature_grads=True)
    half.backward(*[torch.ones_like(t) for t in outs])      # (without the request the bf16-storage backward runs as before)
    # the refused calls left no lane forked: the two-stream call still gives the gradients of a fresh one
    fresh = E.NetCall(flat, audio, [text, feat4], video, False, None)
    res = []
    for c in (two, fresh):
        og = [torch.ones_like(t) for t in c.forward()]
        res.append((c.backward(*og, feature_grads=True).clone(), c.d_inputs))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1][0], res[1][1][0]) and torch.equal(res[0][1][2], res[1][1][2])


# ---------------------------------------------------------------- 10. the nn.Module route
def _module(dims, P):
    from sdumc_amd.model import get_models
    model = get_models(types.SimpleNamespace(input_dims=dims, model="wengnet_mosei_mult_views_text_missing"))
    model.load_state_dict({"model." + k: v for k, v in P.items()})
    model = model.cuda()
    model.model.seed, model.model._calls = 31, 6
    return model


@pytest.fixture(scope="module")
def module_case(params):
    dims = (48, 32, 40)
    from oracle import sdumc_oracle as O
    P = O.init_params(dims + (32,), seed=11)
    B, Tn = 4, (13, 5, 9, 3)
    audio, text, video, feat4 = _batch(dims + (32,), B, Tn, seed=15)
    vals = torch.linspace(-2, 2, B)
    return dims, P, (audio, text, video, feat4, vals)


def test_adapter_in_front_of_audio_trains_through_the_reference_loop(env, module_case):
    """main :119-150 with sdumc_amd.loss and an nn.Linear adapter on the audio features that feeds both model calls"""
    from oracle import sdumc_oracle as O
    from sdumc_amd.loss import MSELoss, RMSELoss, RnCLoss
    dims, P, (audio, text, video, feat4, vals) = module_case
    model = _module(dims, P)
    torch.manual_seed(2)
    adapter = torch.nn.Linear(48, 48)
    Wd, bd = adapter.weight.detach().double().requires_grad_(), adapter.bias.detach().double().requires_grad_()
    adapter = adapter.cuda()
    w = (1.0, 1.0, 0.5, 0.5, 0.5, 0.1)
    model.train()
    a = adapter(audio.cuda())
    v0, (z0, r0, t0, q0) = model([a, text.cuda(), video.cuda(), False])
    v1, (z1, r1, t1, q1) = model([a, feat4.cuda(), video.cuda(), True])
    mse, rmse, rnc = MSELoss().cuda(), RMSELoss().cuda(), RnCLoss().cuda()
    y = vals.cuda()
    terms = [mse(v0, y), mse(v1, y), rmse(t1, t0.detach()), rmse(q1, q0.detach()), rmse(z1, z0),
             rnc(torch.stack((r0, r1), dim=1), y.unsqueeze(1))]
    loss = sum(wi * t for wi, t in zip(w, terms))
    loss.backward()
    assert adapter.weight.grad is not None and adapter.bias.grad is not None
    leaves = {k: p.double().requires_grad_(not O.is_dead(k)) for k, p in P.items()}
    want, _, _ = O.step_loss(leaves, audio.double() @ Wd.t() + bd, text.double(), video.double(), feat4.double(), vals.double(), w,
                             "philox", 31, 3)
    want.backward()
    assert abs(float(loss.detach()) - float(want.detach())) < 1e-4 * max(1.0, abs(float(want.detach())))
    _hold(adapter.weight.grad, Wd.grad, "adapter.weight.grad")
    _hold(adapter.bias.grad, bd.grad, "adapter.bias.grad")
    _hold(model.model._get("frame_dim_reshape_0.weight").grad, leaves["frame_dim_reshape_0.weight"].grad, "frame_dim_reshape_0.weight.grad")


def test_leaf_inputs_train_and_eval_mode(E, env, module_case, monkeypatch):
    from oracle import sdumc_oracle as O
    dims, P, (audio, text, video, feat4, vals) = module_case
    asked = []
    real = E.NetCall.backward

    def spy(self, *a, **k):
        out = real(self, *a, **k)
        asked.append(self.d_inputs)
        return out
    monkeypatch.setattr(E.NetCall, "backward", spy)
    model = _module(dims, P)
    # train mode: a leaf video gets .grad, and only it was asked of the engine
    model.train()
    vid = video.cuda().requires_grad_()
    y, emb = model([audio.cuda(), text.cuda(), vid, False])
    (y.sum() + sum(e.sum() for e in emb)).backward()
    assert vid.grad is not None and asked[-1][0] is None and asked[-1][1] == [None] and asked[-1][2] is not None
    B = y.shape[0]
    ones = [torch.ones(B, 1), torch.ones(B, 128), torch.ones(B, 64), torch.ones(B, 256), torch.ones(B, 7, 128)]
    _, _, _, wv = _oracle(P, audio, [text], video, "train", 31, 6, ones)
    _hold(vid.grad, wv, "video.grad (train mode)")
    with_input = {k: p.grad.clone() for k, p in model.model.named_parameters() if p.grad is not None}
    # no input requires grad: nothing is asked of the engine, and the parameter gradients are the same bits
    model.zero_grad(set_to_none=True)
    model.model._calls = 6
    y, emb = model([audio.cuda(), text.cuda(), video.cuda(), False])
    (y.sum() + sum(e.sum() for e in emb)).backward()
    assert asked[-1] == (None, [None], None)
    without = {k: p.grad for k, p in model.model.named_parameters() if p.grad is not None}
    assert set(without) == set(with_input) and all(torch.equal(without[k], with_input[k]) for k in without)
    # eval mode: the reference's eval-mode outputs are autograd-connected; so are these
    model.eval()
    leaves = [t.cuda().requires_grad_() for t in (audio, text, video)]
    model(leaves + [False])[0].sum().backward()
    zero = [torch.zeros_like(o) for o in ones[1:]]
    _, wa, wt, wv = _oracle(P, audio, [text], video, "eval", 0, 0, [ones[0]] + zero)
    _hold(leaves[0].grad, wa, "audio.grad (eval mode)")
    _hold(leaves[1].grad, wt[0], "text.grad (eval mode)")
    _hold(leaves[2].grad, wv, "video.grad (eval mode)")
    # every other eval call takes the plain path: no autograd node, the same values
    with torch.no_grad():
        y0 = model([audio.cuda(), text.cuda(), video.cuda(), False])[0]
    y1 = model([audio.cuda(), text.cuda(), video.cuda(), False])[0]
    y2 = model(leaves + [False])[0]
    assert not y1.requires_grad and y2.requires_grad and torch.equal(y0, y1) and torch.equal(y0, y2.detach())
