"""Batches read IN PLACE from a resident feature store (include/sdumc_hip.h: sdumc_net_io.row_map, sdumc_gemm_p3.a_map,
sdumc_gemm_b1.a_map, sdumc_gg_problem.b_map; sdumc_gather_batch's map_out).  The two products that read features -- the frame
projections frame_dim_reshape_m (model :282-284) and their weight gradients (autograd of the same Linear) -- must give, through a row
map into the packed store, BIT FOR BIT what they give on the padded copy of the batch that the reference's collater builds
(toolkit/utils/read_data.py:223-248, toolkit/data/feat_data.py:232-253); the whole-step / whole-epoch form of the same statement is
tests/test_gpu_configs.py::test_run_epoch_*."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import _lib, ops
    return _lib, ops


def _store(n_utt, T, d, seed):
    """packed [sum T + 1, d] with a trailing zero row, per-utterance starts / lengths (ragged)"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(max(1, T // 4), T + 1, (n_utt,), generator=g)
    rows = int(lens.sum())
    X = torch.zeros(rows + 1, d)
    X[:rows] = torch.randn(rows, d, generator=g)
    starts = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)[:-1]])
    return X.cuda(), starts, lens, rows


def _batch_map(starts, lens, zero_row, B, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(len(lens), generator=g)[:B]
    Tp = int(lens[idx].max())
    m = torch.full((B, Tp), zero_row, dtype=torch.int32)
    for b, e in enumerate(idx.tolist()):
        n = int(lens[e])
        m[b, :n] = torch.arange(int(starts[e]), int(starts[e]) + n, dtype=torch.int32)
    return m.reshape(-1), idx, Tp


def _padded(x):      # int32 map -> device, with the 64 spare entries the bf16 weight-gradient kernel may read past a batch's last row
    return torch.cat([x, torch.zeros(64, dtype=torch.int32)]).cuda()


def test_gather_batch_writes_the_row_maps_the_host_would(env):
    """sdumc_gather_batch(map_out): entry (b, t) = start of utterance idx[b] + t for a valid frame, the store's zero row for padding;
    labels and valid frame counts ride along; a padded copy through the map equals the gathered padded copy."""
    _lib, ops = env
    from sdumc_amd.data import DeviceFeatureStore
    dims, Tcap = (64, 128, 64, 128), (23, 7, 15, 6)
    store = DeviceFeatureStore.synthetic(30, Tcap, dims, seed=3, planes=True)
    idx = torch.tensor([4, 29, 0, 17, 11], dtype=torch.int64)
    B, T = store.batch_shape(idx)
    maps = [torch.full((B * T[i] + 64,), -7, dtype=torch.int32, device="cuda") for i in range(4)]
    labels = torch.empty(B, device="cuda")
    lens = [torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(4)]
    idx_d = idx.cuda()
    g = store.gather_desc(idx_d.data_ptr(), B, T, None, labels, lens, maps_out=maps)
    _lib.check(_lib.lib.sdumc_gather_batch(C.byref(g), 0, _lib.current_stream()), "sdumc_gather_batch")
    bd, pads, emos, vals, names = store.batch(idx)
    assert torch.equal(labels, vals)
    for i, (m, key) in enumerate(zip(store.MODS, ("audios", "texts", "videos", "feat4s"))):
        zr = store.packed[m].shape[0] - 1
        want = torch.full((B, T[i]), zr, dtype=torch.int32)
        for b, e in enumerate(idx.tolist()):
            n = int(store.length[m][e])
            want[b, :n] = torch.arange(int(store.start[m][e]), int(store.start[m][e]) + n, dtype=torch.int32)
        assert torch.equal(maps[i][:B * T[i]].cpu(), want.reshape(-1))
        assert torch.equal(maps[i][B * T[i]:].cpu(), torch.full((64,), -7, dtype=torch.int32)), "wrote past the batch's rows"
        assert torch.equal(lens[i].cpu(), store.length[m][idx].clamp(max=T[i]))
        assert float(store.packed[m][zr].abs().max()) == 0.0 and int(store.packed_p3[m][zr].max()) == 0      # the zero rows
        assert torch.equal(store.packed[m][maps[i][:B * T[i]].long()].view(B, T[i], -1), bd[key])          # map == the collater's padding


@pytest.mark.parametrize("shape", [(33, 128, 1), (70, 256, 1), (9, 1024, 4)])
def test_frame_projection_through_a_row_map_equals_the_padded_copy(env, shape):
    """sdumc_gemm_p3_nt / sdumc_gemm_b1_nt with a_map (descriptor form via a_map_rows, and the 64-bit form), one tensor and two (the
    text slot's two streams: A2 / a2_map), split-K included: bit for bit the product on the padded copy."""
    _lib, ops = env
    T, d, sk = shape
    B = 6
    X, starts, lens, rows = _store(20, T, d, 5)
    X2, starts2, lens2, rows2 = _store(20, T, d, 6)
    g = torch.Generator(device="cuda").manual_seed(9)
    W = torch.randn(256, d, device="cuda", generator=g) / d ** 0.5
    bias = torch.randn(256, device="cuda", generator=g)
    amap, _, Tp = _batch_map(starts, lens, rows, B, 1)
    M = B * Tp
    Xb = X[amap.cuda().long()].contiguous()
    X3, Xb3, W3 = ops.p3_split(X), ops.p3_split(Xb), ops.p3_split_frag(W)
    amap_d = _padded(amap)
    want = ops.gemm_p3_nt(Xb3, W3, M, 256, d, bias=bias, splitk=sk)
    for rows_hint in (X.shape[0], 0):
        got = ops.gemm_p3_nt(X3, W3, M, 256, d, bias=bias, splitk=sk, a_map=amap_d, a_map_rows=rows_hint)
        assert torch.equal(got, want), f"gemm_p3 mapped (a_map_rows={rows_hint})"
    # two tensors in one launch: rows [0, M2) from X through its map, rows [M2, 2 M2) from X2 through its own (M2 a multiple of 64)
    B2 = 64
    m1 = torch.randint(0, rows + 1, (B2 * 2,), dtype=torch.int32)
    m2 = torch.randint(0, rows2 + 1, (B2 * 2,), dtype=torch.int32)
    Xc = torch.cat([X[m1.cuda().long()], X2[m2.cuda().long()]]).contiguous()
    want2 = ops.gemm_p3_nt(ops.p3_split(Xc), W3, 4 * B2, 256, d, bias=bias, splitk=sk)
    got2 = ops.gemm_p3_nt(X3, W3, 4 * B2, 256, d, bias=bias, splitk=sk, A3_second=ops.p3_split(X2), second_row0=2 * B2,
                          a_map=_padded(m1), a2_map=_padded(m2), a_map_rows=max(X.shape[0], X2.shape[0]))
    assert torch.equal(got2, want2), "gemm_p3 mapped, two tensors"
    # bf16 storage
    if d % 128 == 0:
        Xh, Xbh, Wb = X.bfloat16(), Xb.bfloat16(), ops.b1_frag(W)
        wanth = ops.gemm_b1_nt(Xbh, Wb, M, 256, d, bias=bias, splitk=sk)
        for rows_hint in (X.shape[0], 0):
            goth = ops.gemm_b1_nt(Xh, Wb, M, 256, d, bias=bias, splitk=sk, a_map=amap_d, a_map_rows=rows_hint)
            assert torch.equal(goth, wanth), f"gemm_b1 mapped (a_map_rows={rows_hint})"


@pytest.mark.parametrize("shape", [(33, 128), (70, 256), (21, 1024)])
def test_frame_weight_gradient_through_a_row_map_equals_the_padded_copy(env, shape):
    """sdumc_gemm_group_tn / _bf16 with b_map: C = dx^T . features with the features' k-rows fetched through the map (K not a multiple
    of the k-tile, two K segments = the two text streams from two packed tensors): weight AND bias gradient bit for bit."""
    _lib, ops = env
    T, d = shape
    B = 5
    X, starts, lens, rows = _store(20, T, d, 7)
    X2, starts2, lens2, rows2 = _store(20, T, d, 8)
    g = torch.Generator(device="cuda").manual_seed(3)
    amap, _, Tp = _batch_map(starts, lens, rows, B, 2)
    amap2, _, Tp2 = _batch_map(starts2, lens2, rows2, B, 3)
    K, K2 = B * Tp, B * Tp2
    Xb, Xb2 = X[amap.cuda().long()].contiguous(), X2[amap2.cuda().long()].contiguous()
    dx, dx2 = torch.randn(K, 256, device="cuda", generator=g), torch.randn(K2, 256, device="cuda", generator=g)
    for hf in (False, True):
        if hf and d % 8:
            continue
        cv = (lambda t: t.bfloat16()) if hf else (lambda t: t)
        p0 = [dict(A=cv(dx), B=cv(Xb), colsum=torch.empty(256, device="cuda")),
              dict(A=cv(dx), B=cv(Xb), A1=cv(dx2), B1=cv(Xb2), colsum=torch.empty(256, device="cuda"))]
        p1 = [dict(A=cv(dx), B=cv(X), b_map=_padded(amap), K=K, colsum=torch.empty(256, device="cuda")),
              dict(A=cv(dx), B=cv(X), b_map=_padded(amap), K=K, A1=cv(dx2), B1=cv(X2), b_map1=_padded(amap2), K1=K2,
                   colsum=torch.empty(256, device="cuda"))]
        ops.gemm_group_tn(p0)
        ops.gemm_group_tn(p1)
        torch.cuda.synchronize()
        for a, b in zip(p0, p1):
            assert torch.equal(a["C"], b["C"]) and torch.equal(a["colsum"], b["colsum"]), f"grouped dW mapped (bf16={hf})"


def test_row_map_argument_contract(env):
    """SDUMC_EINVAL where a map cannot be honoured: with a_row_mod / keep-bits / an explicit tile height on the plane GEMM, a2_map
    without A2, b_row_mod beside b_map, and on the fp32-MFMA form of the grouped kernel (sdumc_set_split_(0))."""
    _lib, ops = env
    lib = _lib.lib
    X = torch.randn(129, 128, device="cuda")
    X[-1] = 0
    W = torch.randn(256, 128, device="cuda")
    X3, W3 = ops.p3_split(X), ops.p3_split_frag(W)
    amap = _padded(torch.randint(0, 129, (64,), dtype=torch.int32))
    bits = torch.randint(0, 16, (64, 32), device="cuda", dtype=torch.uint8)
    for kw in (dict(a_row_mod=32), dict(bits=bits, scale=2.0), dict(tile_m=64), dict(a2_map=amap)):
        with pytest.raises(_lib.SdumcError):
            ops.gemm_p3_nt(X3, W3, 64, 256, 128, a_map=amap, **kw)
    dx = torch.randn(64, 256, device="cuda")
    with pytest.raises(_lib.SdumcError):
        ops.gemm_group_tn([dict(A=dx, B=X, b_map=amap, K=64, b_row_mod=32)])
    prev = lib.sdumc_get_split_()
    try:
        lib.sdumc_set_split_(0)
        with pytest.raises(_lib.SdumcError):
            ops.gemm_group_tn([dict(A=dx, B=X, b_map=amap, K=64)])
    finally:
        lib.sdumc_set_split_(prev)


# ---- a row-mapped batch the backward's schedule cannot serve (plan_backward's rc) is rejected before anything of the call runs ----
# The frame projections' weight gradient fetches mapped rows only in the grouped launch, and the grouped launch takes 16-byte aligned
# operands: a packed fp32 audio tensor at a float-aligned but not 16-byte-aligned address is a batch check_io accepts (the forward reads
# the planes, never the fp32 tensor) and the backward cannot run.  So is, in fp32 storage, a context whose split option keeps the plane
# GEMMs of the forward (SDUMC_SPLIT_WIDE) and turns the grouped launch's split arithmetic off (SDUMC_SPLIT_GROUP): only that kernel of
# the grouped launch reads maps.
_REASONS = ("misaligned", "split")
_SPLIT_NO_GROUP = 14      # every family but the grouped weight-gradient launch


def _unservable(streams, seed, reason, ctx):
    """the batch and context state of `reason`; returns (batch, undo)"""
    if reason == "split":
        ctx.set_option("split", _SPLIT_NO_GROUP)
        return _resident_batch(streams, seed), lambda: ctx.set_option("split", None)
    return _resident_batch(streams, seed, misalign_audio=True), lambda: None
_RB, _RT, _RD = 2, (9, 5, 7, 6), (64, 128, 64, 128)      # B; padded frames and widths of audio, text, video, feat4


def _resident_batch(streams, seed, misalign_audio=False):
    """the (audio, text, video[, feat4]) slots of one batch: packed store tensors with planes and row maps, and the padded copies"""
    from sdumc_amd import engine
    n = 3 if streams == 1 else 4
    out = dict(packed=[], planes=[], maps=[], rows=[], padded=[])
    for i in range(n):
        X, starts, lens, rows = _store(5, _RT[i], _RD[i], seed + i)
        amap, _, Tp = _batch_map(starts, lens, rows, _RB, seed + 10 + i)
        amap = torch.cat([amap.view(_RB, Tp), torch.full((_RB, _RT[i] - Tp), rows, dtype=torch.int32)], 1).reshape(-1)
        out["padded"].append(X[amap.cuda().long()].view(_RB, _RT[i], _RD[i]).contiguous())
        out["planes"].append(engine.p3_split_into(X, engine._planes_buffer(X.shape[0], _RD[i], X.device)))
        if i == 0 and misalign_audio:
            buf = torch.zeros(X.numel() + 4, device=X.device)
            Xm = buf[1:1 + X.numel()].view_as(X)
            Xm.copy_(X)
            if Xm.data_ptr() % 16 != 4:
                pytest.fail("test set-up: the allocator returned a block that is not 16-byte aligned")
            X = Xm
        out["packed"].append(X)
        out["maps"].append(_padded(amap))
        out["rows"].append(int(X.shape[0]))
    return out


def _flat_params():
    from oracle import sdumc_oracle as O
    from sdumc_amd import engine
    lay = engine.ParamLayout.get(*_RD[:3])
    flat = torch.zeros(lay.total)
    P = O.init_params(_RD, seed=1)
    for k, v in lay.views(flat).items():
        v.copy_(P[k])
    return flat.cuda()


def _bind_store(step, rb, seed):
    from sdumc_amd import engine
    labels = torch.randn(_RB, generator=torch.Generator().manual_seed(seed)).cuda()
    step._bind(engine._Source(tuple(rb["packed"]), tuple(rb["planes"]), rb["maps"], tuple(rb["rows"]), labels))


def _map_io(call, rb):
    """points a NetCall built on the padded copies at the packed store tensors, their planes and the row maps"""
    io, ptr = call.io, torch.Tensor.data_ptr
    io.audio, io.text[0], io.video = ptr(rb["packed"][0]), ptr(rb["packed"][1]), ptr(rb["packed"][2])
    io.audio_p3, io.text_p3[0], io.video_p3 = ptr(rb["planes"][0]), ptr(rb["planes"][1]), ptr(rb["planes"][2])
    if len(rb["packed"]) == 4:
        io.text[1], io.text_p3[1] = ptr(rb["packed"][3]), ptr(rb["planes"][3])
    for i, (m, r) in enumerate(zip(rb["maps"], rb["rows"])):
        io.row_map[i], io.store_rows[i] = ptr(m), r


def _net_call(flat, rb, streams, train, ctx):
    from sdumc_amd import engine
    rng = engine.RngState(5, flat.device) if train else None
    pad = rb["padded"]
    return engine.NetCall(flat, pad[0], [pad[1]] + ([pad[3]] if streams == 2 else []), pad[2], train, rng, planes=True, ctx=ctx)


@pytest.mark.parametrize("reason", _REASONS)
def test_unservable_row_mapped_train_step_is_rejected_before_anything_runs_and_the_context_stays_usable(env, reason):
    """sdumc_train_step on a row-mapped batch whose frame dW cannot take the grouped launch: SDUMC_EINVAL with the outputs, the loss
    record, the whole step workspace (gradient bucket included), the parameters, the Adam state and the dropout counter untouched --
    no forward, no loss stage, no fork.  The same context then runs a valid row-mapped step bit for bit like a context that never saw
    the rejected call (no lane left forked, no event left recorded)."""
    _lib, ops = env
    from sdumc_amd import engine
    good = _resident_batch(2, 40)
    steps = []
    for rejected_first in (True, False):
        flat = _flat_params()
        ctx = engine.ExecContext()
        step = engine.TrainStep(flat, _RB, _RT, _RD, seed=3, planes=True, ctx=ctx)
        if rejected_first:
            bad, undo = _unservable(2, 40, reason, ctx)
            _bind_store(step, bad, 7)
            outs = (step.vals, step.fused, step.rnc, step.text_hidden, step.cross_text, step.losses, step.grads)
            for t in outs:
                t.fill_(-77.0)
            step.adam_m.fill_(0.25)
            step.adam_v.fill_(0.5)
            state = (flat, step.adam_m, step.adam_v, step.hyper, step.rng.t, step.workspace)
            before = [t.clone() for t in state]
            torch.cuda.synchronize()
            with pytest.raises(_lib.SdumcError, match="SDUMC_EINVAL"):
                step.launch()
            torch.cuda.synchronize()
            for t in outs:
                assert bool((t == -77.0).all()), "a launch of the rejected step wrote an output"
            for t, b in zip(state, before):
                assert torch.equal(t, b), "the rejected step changed state"
            undo()
            step.adam_m.zero_()
            step.adam_v.zero_()
            step.grads.zero_()
        _bind_store(step, good, 7)
        losses = step.run().clone()
        torch.cuda.synchronize()
        steps.append((losses, flat, step.adam_m, step.adam_v, step.hyper))
    assert bool(torch.isfinite(steps[0][0]).all()) and float(steps[0][2].abs().max()) > 0
    for a, b in zip(*steps):
        assert torch.equal(a, b), "a step after the rejected call differs from one on a fresh context"


@pytest.mark.parametrize("reason", _REASONS)
@pytest.mark.parametrize("streams", [1, 2])
def test_unservable_row_mapped_backward_is_rejected_before_anything_runs(env, streams, reason):
    """sdumc_net_backward, and BOTH phases of sdumc_net_backward_phase (the rejection is a property of the frame-level part, and the
    first phase already returns it), after a successful forward: SDUMC_EINVAL, gradient bucket and workspace untouched."""
    _lib, ops = env
    from sdumc_amd import engine
    lib = _lib.lib
    ctx = engine.ExecContext()
    rb, undo = _unservable(streams, 50, reason, ctx)
    flat = _flat_params()
    call = _net_call(flat, rb, streams, True, ctx)
    _map_io(call, rb)
    outs = call.forward()
    g = torch.Generator(device="cuda").manual_seed(2)
    og = [torch.randn(t.shape, device="cuda", generator=g) for t in outs]
    grads = torch.full((call.layout.live,), -77.0, device="cuda")
    ng = _lib.NetGrads()
    ng.d_vals, ng.d_fused, ng.d_rnc, ng.d_text_hidden, ng.d_cross_text = (t.data_ptr() for t in og)
    ng.grads = grads.data_ptr()
    torch.cuda.synchronize()
    ws = call.workspace.clone()
    args = (C.byref(call.dims), C.byref(call.io), C.byref(ng))
    calls = [lambda: lib.sdumc_net_backward(*args, _lib.current_stream()),
             lambda: lib.sdumc_net_backward_phase(*args, 0, _lib.current_stream()),
             lambda: lib.sdumc_net_backward_phase(*args, 1, _lib.current_stream())]
    for fn in calls:
        with pytest.raises(_lib.SdumcError, match="SDUMC_EINVAL"):
            _lib.check(fn(), "backward")
        torch.cuda.synchronize()
        assert bool((grads == -77.0).all()) and torch.equal(call.workspace, ws), "a launch of the rejected backward ran"
    # the context is usable: the aligned form of the same batch runs, and its bucket is finite and non-trivial
    undo()
    ok = _resident_batch(streams, 50)
    _map_io(call, ok)
    call.forward()
    _lib.check(calls[0](), "sdumc_net_backward")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grads).all()) and float(grads.abs().max()) > 0


@pytest.mark.parametrize("reason", _REASONS)
@pytest.mark.parametrize("streams", [1, 2])
def test_forward_still_accepts_the_batch_the_backward_rejects(env, streams, reason):
    """eval-mode sdumc_net_forward reads the planes through the maps and never the fp32 tensors: on the batch the backward rejects it
    gives, bit for bit, the outputs of the padded copy of the same batch."""
    _lib, ops = env
    from sdumc_amd import engine
    ctx = engine.ExecContext()
    rb, _ = _unservable(streams, 60, reason, ctx)
    flat = _flat_params()
    call = _net_call(flat, rb, streams, False, ctx)
    want = [t.clone() for t in call.forward()]
    _map_io(call, rb)
    for t in (call.vals, call.fused, call.rnc, call.text_hidden, call.cross_text):
        t.fill_(-77.0)
    got = call.forward()
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ---- a row-mapped batch the FORWARD's schedule cannot serve (plan_forward's rc) is refused before anything of the call runs ----
# Only the plane GEMM (fp32 storage) and the fragment-major bf16 GEMM fetch their A rows through a map.  A context whose split option
# turns the wide-tile family's split arithmetic off (SDUMC_SPLIT_WIDE) has no plane route; the grouped weight-gradient launch keeps its
# own (SDUMC_SPLIT_GROUP), so the backward's schedule accepts the batch and the refusal is the forward's.
_SPLIT_NO_WIDE = 13      # every family but the wide-tile one
_LENS = tuple((t, max(1, t // 2)) for t in _RT)      # key-padding lengths per modality (audio, text, video, feat4), _RB samples


def _refused_forward(_lib, streams, rejected_first):
    """one train-mode sdumc_net_forward of the servable batch; with rejected_first the same context and call object saw the refused
    call before"""
    from sdumc_amd import engine
    ctx = engine.ExecContext()
    flat = _flat_params()
    rb = _resident_batch(streams, 70)
    call = _net_call(flat, rb, streams, True, ctx)
    _map_io(call, rb)
    call.set_lengths(_LENS[:3] if streams == 1 else _LENS)
    if rejected_first:
        ctx.set_option("split", _SPLIT_NO_WIDE)
        outs = (call.vals, call.fused, call.rnc, call.text_hidden, call.cross_text)
        for t in outs:
            t.fill_(-77.0)
        rng = call._keep[4]
        state = (call.workspace, flat, rng.t)
        before = [t.clone() for t in state]
        torch.cuda.synchronize()
        with pytest.raises(_lib.SdumcError, match="SDUMC_EINVAL"):
            call.forward()
        torch.cuda.synchronize()
        for t in outs:
            assert bool((t == -77.0).all()), "a launch of the refused forward wrote an output"
        for name, t, b in zip(("workspace", "parameters", "dropout counter"), state, before):
            assert torch.equal(t, b), f"the refused forward changed the {name}"
        ctx.set_option("split", None)
    got = [t.clone() for t in call.forward()]
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("streams", [1, 2])
def test_row_mapped_forward_without_a_plane_route_is_refused_before_anything_runs(env, streams):
    """sdumc_net_forward with row maps, key-padding lengths and no plane route: SDUMC_EINVAL with the five outputs, the whole
    workspace (the expanded lengths included), the parameters and the dropout counter untouched; the same context then runs the
    batch bit for bit like a context that never saw the refused call."""
    _lib, ops = env
    after, fresh = _refused_forward(_lib, streams, True), _refused_forward(_lib, streams, False)
    assert bool(torch.isfinite(fresh[0]).all())
    for a, b in zip(after, fresh):
        assert torch.equal(a, b), "a forward after the refused call differs from one on a fresh context"


def test_row_mapped_train_step_without_a_plane_route_is_refused_before_anything_runs(env):
    """sdumc_train_step on the same batch and context: the backward's schedule accepts it, the forward's does not -- SDUMC_EINVAL
    with the outputs, the loss record, the whole step workspace, the parameters, the Adam state and the dropout counter untouched;
    the same context then runs the step bit for bit like a fresh one."""
    _lib, ops = env
    from sdumc_amd import engine
    rb = _resident_batch(2, 70)
    steps = []
    for rejected_first in (True, False):
        flat = _flat_params()
        ctx = engine.ExecContext()
        step = engine.TrainStep(flat, _RB, _RT, _RD, seed=3, planes=True, ctx=ctx)
        _bind_store(step, rb, 7)
        step.set_lengths(_LENS)
        if rejected_first:
            ctx.set_option("split", _SPLIT_NO_WIDE)
            outs = (step.vals, step.fused, step.rnc, step.text_hidden, step.cross_text, step.losses, step.grads)
            for t in outs:
                t.fill_(-77.0)
            step.adam_m.fill_(0.25)
            step.adam_v.fill_(0.5)
            state = (step.workspace, flat, step.adam_m, step.adam_v, step.hyper, step.rng.t)
            before = [t.clone() for t in state]
            torch.cuda.synchronize()
            with pytest.raises(_lib.SdumcError, match="SDUMC_EINVAL"):
                step.launch()
            torch.cuda.synchronize()
            for t in outs:
                assert bool((t == -77.0).all()), "a launch of the refused step wrote an output"
            for name, t, b in zip(("workspace", "parameters", "adam_m", "adam_v", "hyper", "dropout counter"), state, before):
                assert torch.equal(t, b), f"the refused step changed the {name}"
            ctx.set_option("split", None)
            step.adam_m.zero_()
            step.adam_v.zero_()
            step.grads.zero_()
        losses = step.run().clone()
        torch.cuda.synchronize()
        steps.append((losses, flat, step.adam_m, step.adam_v, step.hyper))
    assert bool(torch.isfinite(steps[0][0]).all()) and float(steps[0][2].abs().max()) > 0
    for a, b in zip(*steps):
        assert torch.equal(a, b), "a step after the refused call differs from one on a fresh context"
