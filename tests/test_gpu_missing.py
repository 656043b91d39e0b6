"""The random-missing protocol on the device (DeviceFeatureStore.with_missing -> data.MissingView; sdumc_gather_batch's miss_* fields,
csrc/elementwise.hip gather_batch_kernel): frames and whole modalities dropped while a batch's row maps / padded copies are written.

The fixture is tests/test_gpu_eval_epoch.py's, rebuilt here: 37 synthetic utterances, frame maxima (40, 6, 24, 5), min_frac 0.25, batches
of 8, 8, 8, 8, 5 in a shuffled order; widths (64, 128, 64, 128) in fp32 storage with planes, (128, 128, 128, 128) in bf16 storage.
Spec A: frame = {audio .3, text .5, video 1.0}, modality = {audio .25}, seed 1234.

Every expectation is built HERE from oracle/philox.py and torch indexing -- never from missing_keep, materialized or anything else under
test: which packed rows are absent (rule_rows), and the MATERIALISED store (a clone of the packed tensors with those rows zeroed, planes
split again).  A view must give the bits the materialised store gives: a zero row is a zero row on both sides, so no tolerance appears."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.philox import philox4x32_10, drop_threshold

pytestmark = pytest.mark.gpu

N_UTT, TCAP = 37, (40, 6, 24, 5)
DIMS = {"fp32": (64, 128, 64, 128), "bf16": (128, 128, 128, 128)}
MODS = ("audio", "text", "video", "feat4")
NAMES = ("fused", "rnc", "text_hidden", "cross_text")
SPEC_A = dict(frame={"audio": .3, "text": .5, "video": 1.0}, modality={"audio": .25}, seed=1234)


def _batches(seed, sizes=(8, 8, 8, 8, 5), n=N_UTT):
    p = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    out, o = [], 0
    for b in sizes:
        out.append(p[o:o + b].clone())
        o += b
    return out


def rule_rows(store, frame=None, modality=None, seed=0, draw=0):
    """{modality: bool numpy [packed rows without the zero row], True = absent} -- the rule of include/sdumc_hip.h from the oracle's
    Philox: word(c0) = philox(c0, e, 0x4D530000 + m, draw, seed lo, seed hi)[0]; absent iff word(t) < floor(frame rate * 2^32) or
    word(0xFFFFFFFF) < floor(modality rate * 2^32), compared in 64 bits (a rate of 1 has the threshold 2^32)"""
    frame, modality, out = frame or {}, modality or {}, {}
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for m, name in enumerate(MODS):
        lens = store.length[name].numpy().astype(np.int64)
        starts = store.start[name].numpy()
        e = np.repeat(np.arange(lens.size), lens)
        t = np.arange(int(lens.sum())) - np.repeat(starts, lens)
        c2 = np.uint32(0x4D530000 + m)
        w_t = philox4x32_10(t.astype(np.uint32), e.astype(np.uint32), c2, np.uint32(draw), k0, k1)[0].astype(np.uint64)
        w_u = philox4x32_10(np.uint32(0xFFFFFFFF), e.astype(np.uint32), c2, np.uint32(draw), k0, k1)[0].astype(np.uint64)
        out[name] = (w_t < np.uint64(drop_threshold(frame.get(name, 0.0)))) | (w_u < np.uint64(drop_threshold(modality.get(name, 0.0))))
    return out


def materialise(store, absent):
    """the test-built reference store: packed tensors cloned, absent rows zeroed, planes split again"""
    new = copy.copy(store)
    new.packed = {m: t.clone() for m, t in store.packed.items()}
    for m in MODS:
        rows = torch.from_numpy(np.flatnonzero(absent[m])).cuda()
        new.packed[m][rows] = 0
    new.packed_p3 = None
    if store.packed_p3 is not None:
        new.make_planes()
    return new


def _same(x, y):
    """bit equality with NaN == NaN"""
    return x.shape == y.shape and torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))


class _Env:
    def __init__(self):
        from oracle import sdumc_oracle as O
        from sdumc_amd import engine, evaluate, saliency, data, _lib
        self.engine, self.evaluate, self.saliency, self.data, self._lib = engine, evaluate, saliency, data, _lib
        self.flat, self.store = {}, {}
        for mode, dims in DIMS.items():
            P = O.init_params(dims, seed=8)
            lay = engine.ParamLayout.get(*dims[:3])
            flat = torch.zeros(lay.total)
            for k, v in lay.views(flat).items():
                v.copy_(P[k])
            self.flat[mode] = flat.cuda()
            self.store[mode] = data.DeviceFeatureStore.synthetic(N_UTT, TCAP, dims, seed=5, min_frac=0.25, bf16=mode == "bf16",
                                                                 planes=mode == "fp32")
        self.batches = _batches(1)
        self._mat = {}

    def view(self, mode, draw=0, **spec):
        return self.store[mode].with_missing(**(spec or SPEC_A), draw=draw)

    def absent(self, mode, draw=0, **spec):
        return rule_rows(self.store[mode], draw=draw, **(spec or SPEC_A))

    def mat(self, mode, draw=0):
        """the materialised store of spec A at `draw` (built once, never changed)"""
        if (mode, draw) not in self._mat:
            self._mat[mode, draw] = materialise(self.store[mode], self.absent(mode, draw))
        return self._mat[mode, draw]

    def maps(self, store, ix, T=None, max_workgroups=0, lengths=True, poison=None):
        """gather_desc(maps_out=...) + sdumc_gather_batch -> (four int32 [B, T_m] maps, four int32 [B] lengths, the call's code)"""
        _lib = self._lib
        B, T0 = store.batch_shape(ix)
        T = T0 if T is None else T
        idx_d = torch.as_tensor(ix, dtype=torch.int64).cuda()
        maps = [torch.full((B, t), -7, dtype=torch.int32, device="cuda") for t in T]
        lens = [torch.full((B,), -7, dtype=torch.int32, device="cuda") for _ in T] if lengths else None
        labels = torch.empty(B, device="cuda")
        g = store.gather_desc(idx_d.data_ptr(), B, T, None, labels, lens, maps_out=maps)
        if poison is not None:
            poison(g)
        rc = _lib.lib.sdumc_gather_batch(C.byref(g), max_workgroups, _lib.current_stream())
        torch.cuda.synchronize()
        return maps, lens, rc

    def expected_maps(self, store, absent, ix, T=None):
        B, T0 = store.batch_shape(ix)
        T = T0 if T is None else T
        out = []
        for m, t in zip(MODS, T):
            zero_row = int(store.packed[m].shape[0]) - 1
            want = torch.full((B, t), zero_row, dtype=torch.int32)
            for b, e in enumerate(torch.as_tensor(ix).tolist()):
                s, n = int(store.start[m][e]), min(int(store.length[m][e]), t)
                rows = torch.arange(s, s + n, dtype=torch.int32)
                rows[torch.from_numpy(absent[m][s:s + n])] = zero_row
                want[b, :n] = rows
            out.append(want)
        return out


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return _Env()


def test_spec_a_drops_what_it_should(env):
    """the fixture itself: under spec A some audio and text frames go and some stay, every video frame goes, no feat4 frame does; a
    quarter or so of the utterances lose their audio entirely -- so the comparisons below have something to compare"""
    a = env.absent("fp32")
    st = env.store["fp32"]
    view = env.view("fp32")
    assert isinstance(view, env.data.MissingView) and view.base is st and view.spec == env.data.MissingSpec(**SPEC_A)
    assert view.packed is st.packed and view.packed_p3 is st.packed_p3 and view.start_d is st.start_d      # a view shares, it does not copy
    assert 0 < a["audio"].sum() < a["audio"].size and 0 < a["text"].sum() < a["text"].size
    assert a["video"].all() and not a["feat4"].any()
    whole = [bool(a["audio"][int(st.start["audio"][e]):int(st.start["audio"][e]) + int(st.length["audio"][e])].all()) for e in range(N_UTT)]
    assert 2 <= sum(whole) <= 20
    assert not torch.equal(env.mat("fp32").packed["audio"], st.packed["audio"])
    assert torch.equal(env.mat("fp32").packed["feat4"], st.packed["feat4"])


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("max_workgroups", [0, 1])
def test_maps(env, mode, max_workgroups):
    """1. every map entry = start + t for a present frame, zero_row for an absent or padded one; len_out is the plain store's -- for a
    batch of 8, the batch of 5 and a batch of 1, in one pass and on the strided one-workgroup grid"""
    store, view, absent = env.store[mode], env.view(mode), env.absent(mode)
    n_absent = 0
    for ix in (env.batches[0], env.batches[4], env.batches[2][3:4]):
        maps, lens, rc = env.maps(view, ix, max_workgroups=max_workgroups)
        assert rc == 0
        _, plain_lens, rc = env.maps(store, ix, max_workgroups=max_workgroups)
        assert rc == 0
        for k, (m, got, want) in enumerate(zip(MODS, maps, env.expected_maps(store, absent, ix))):
            assert torch.equal(got.cpu(), want), (m, ix.tolist())
            assert torch.equal(lens[k], plain_lens[k]) and torch.equal(lens[k].cpu(), store.length[m][ix].clamp(max=got.shape[1])), m
            n_absent += int(sum((want[b, :int(store.length[m][e])] == store.packed[m].shape[0] - 1).sum() for b, e in enumerate(ix.tolist())))
    assert n_absent > 20


def test_copies(env):
    """2. batch_into with planes (fp32: eight segments, the descriptor's maximum) and the bf16 rows hold the materialised store's bits;
    so does view.batch, which goes through batch_into (the materialised store's batch is the old sdumc_gather_pad route)"""
    for mode in ("fp32", "bf16"):
        view, mat, store = env.view(mode), env.mat(mode), env.store[mode]
        dtype = store.packed["audio"].dtype
        for ix in (env.batches[1], env.batches[4]):
            B, T = store.batch_shape(ix)
            got, want = [], []
            for s in (view, mat):
                outs = [torch.full((B, t, d), 7.0, dtype=dtype, device="cuda") for t, d in zip(T, DIMS[mode])]
                planes = [torch.full((B * t * 6 * d,), 7, dtype=torch.uint8, device="cuda") for t, d in zip(T, DIMS[mode])] if mode == "fp32" else None
                labels, lens = torch.empty(B, device="cuda"), [torch.empty(B, dtype=torch.int32, device="cuda") for _ in T]
                s.batch_into(ix, outs, labels, lens, planes_out=planes)
                torch.cuda.synchronize()
                (got if s is view else want).append((outs, planes, labels, lens))
            (go, gp, gl, gn), (wo, wp, wl, wn) = got[0], want[0]
            for k, m in enumerate(MODS):
                assert torch.equal(go[k], wo[k]), (mode, m, "rows")
                assert torch.equal(gn[k], wn[k]) and torch.equal(gl, wl), (mode, m, "lengths / labels")
                if gp is not None:
                    assert torch.equal(gp[k], wp[k]), (mode, m, "planes")
            assert not bool(go[2].any()) and bool(go[3].any())      # video: every frame absent; feat4: untouched
            vb, mb = view.batch(ix), mat.batch(ix)
            for key in ("audios", "texts", "videos", "feat4s"):
                assert torch.equal(vb[0][key], mb[0][key]), (mode, key)
            assert vb[1] == mb[1] and torch.equal(vb[3], mb[3]) and vb[4] == mb[4]


def test_invariance(env):
    """3. one utterance in two batches of different composition, position and Tmax loses the same frames (the rule's); another draw
    loses different ones"""
    store, view, absent = env.store["fp32"], env.view("fp32"), env.absent("fp32")
    lens_a = store.length["audio"]
    u = int(max(env.batches[0].tolist(), key=lambda e: int(lens_a[e])))      # the longest audio of the first batch
    pos_a = env.batches[0].tolist().index(u)
    other = torch.tensor([u] + env.batches[3][:2].tolist())
    T_b = tuple(t + 3 for t in store.batch_shape(torch.cat([env.batches[0], other]))[1])      # (a padded shape neither batch has)
    ma, _, _ = env.maps(view, env.batches[0])
    mb, _, _ = env.maps(view, other, T=T_b)
    mc, _, _ = env.maps(env.view("fp32", draw=1), env.batches[0])
    assert pos_a != 0 or len(other) != len(env.batches[0])
    differs = False
    for k, m in enumerate(MODS):
        s, n = int(store.start[m][u]), int(store.length[m][u])
        zero_row = store.packed[m].shape[0] - 1
        pa, pb, pc = (ma[k][pos_a, :n] == zero_row).cpu(), (mb[k][0, :n] == zero_row).cpu(), (mc[k][pos_a, :n] == zero_row).cpu()
        assert ma[k].shape[1] != mb[k].shape[1]
        assert torch.equal(pa, pb) and torch.equal(pa, torch.from_numpy(absent[m][s:s + n])), m
        differs |= not torch.equal(pa, pc)
    assert differs
    d1 = env.absent("fp32", draw=1)
    assert all(torch.equal(g.cpu(), w) for g, w in zip(mc, env.expected_maps(store, d1, env.batches[0])))


def _assert_eval_equal(a, b, what):
    assert torch.equal(a.seen, b.seen) and _same(a.preds, b.preds), what
    for n in NAMES:
        assert _same(a.embeddings[n], b.embeddings[n]), (what, n)
    for s, d in a.attention.items():
        for m, t in d.items():
            assert _same(t, b.attention[s][m]), (what, s, m)


@pytest.mark.parametrize("mode,inplace,key_padding", [("fp32", True, False), ("fp32", False, False), ("bf16", True, False), ("fp32", True, True)])
def test_evaluation(env, mode, inplace, key_padding):
    """4. eval_epoch(view) = eval_epoch(materialised): predictions, embeddings and attention maps, bit for bit"""
    kw = dict(bf16=mode == "bf16", inplace=inplace, key_padding=key_padding, embeddings=True, attention=True)
    got = env.evaluate.eval_epoch(env.flat[mode], DIMS[mode], env.view(mode), env.batches, **kw)
    torch.cuda.synchronize()
    assert env.evaluate._evaluator[1]._in_place(env.view(mode)) == inplace
    want = env.evaluate.eval_epoch(env.flat[mode], DIMS[mode], env.mat(mode), env.batches, **kw)
    plain = env.evaluate.eval_epoch(env.flat[mode], DIMS[mode], env.store[mode], env.batches, **kw)
    torch.cuda.synchronize()
    _assert_eval_equal(got, want, (mode, inplace, key_padding))
    assert int((got.seen != 0).sum()) == N_UTT and bool(torch.isfinite(got.preds).all())
    assert not torch.equal(got.preds, plain.preds)      # (and the spec does change the predictions)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_training(env, mode):
    """5. two trainers from the same parameters and seed: run_epoch over view.redrawn(0), view.redrawn(1) against the two materialised
    stores -- parameters, both Adam moments, the step count; then train_epoch's record on the view against the materialised store's"""
    kw = {"bf16": True} if mode == "bf16" else {}
    a, b = (env.engine.FusedTrainer(env.flat[mode].clone(), DIMS[mode], lr=1e-3, seed=11, capacity=(8, TCAP), **kw) for _ in range(2))
    view = env.view(mode)
    for draw in (0, 1):
        assert a.run_epoch(view.redrawn(draw), env.batches) == len(env.batches)
        assert b.run_epoch(env.mat(mode, draw), env.batches) == len(env.batches)
    torch.cuda.synchronize()
    assert a._in_place(view) and b._in_place(env.mat(mode))
    (ma, va, ta), (mb, vb, tb) = a.optimizer_state(), b.optimizer_state()
    assert ta == tb == 2 * len(env.batches)
    assert torch.equal(a.params, b.params) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(a.state.hyper, b.state.hyper)
    assert not torch.equal(a.params, env.flat[mode])
    ra = a.train_epoch(view.redrawn(0), env.batches)
    rb = b.train_epoch(env.mat(mode, 0), env.batches)
    torch.cuda.synchronize()
    assert ra.steps == rb.steps == len(env.batches) and torch.equal(ra.seen, rb.seen)
    assert _same(ra.preds, rb.preds) and _same(ra.log, rb.log) and bool(torch.isfinite(ra.preds).all())
    assert torch.equal(a.params, b.params)
    # the draw matters: a third trainer on draw 0 twice ends elsewhere
    c = env.engine.FusedTrainer(env.flat[mode].clone(), DIMS[mode], lr=1e-3, seed=11, capacity=(8, TCAP), **kw)
    c.run_epoch(view.redrawn(0), env.batches)
    c.run_epoch(view.redrawn(0), env.batches)
    c.train_epoch(view.redrawn(0), env.batches)
    torch.cuda.synchronize()
    assert not torch.equal(c.params, a.params)


def test_step_from_store_on_a_view(env):
    """5b. the single-step route assembles through the same descriptor"""
    a, b = (env.engine.FusedTrainer(env.flat["fp32"].clone(), DIMS["fp32"], lr=1e-3, seed=11, capacity=(8, TCAP)) for _ in range(2))
    for ix in env.batches[:2]:
        a.step_from_store(env.view("fp32"), ix)
        b.step_from_store(env.mat("fp32"), ix)
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params) and torch.equal(a.state.adam_m, b.state.adam_m)


def test_edges(env):
    """6. an all-zero spec is the plain store (descriptor bytes and results); modality = {text: 1} is a store whose text rows are all
    zero; missing_curve's rate-0 entry is the plain metrics and its rate-1 entry the all-zero audio and video store's"""
    mode = "fp32"
    store, flat, dims = env.store[mode], env.flat[mode], DIMS[mode]
    ev = lambda s, **kw: env.evaluate.eval_epoch(flat, dims, s, env.batches, embeddings=True, attention=True, **kw)
    zero = store.with_missing(frame={"audio": 0.0}, modality={"video": 0}, seed=99, draw=5)
    idx_d = env.batches[0].cuda()
    B, T = store.batch_shape(env.batches[0])
    maps = [torch.empty(B * t, dtype=torch.int32, device="cuda") for t in T]
    labels = torch.empty(B, device="cuda")
    assert bytes(zero.gather_desc(idx_d.data_ptr(), B, T, None, labels, None, maps_out=maps)) == \
        bytes(store.gather_desc(idx_d.data_ptr(), B, T, None, labels, None, maps_out=maps))
    plain = ev(store)
    torch.cuda.synchronize()
    _assert_eval_equal(ev(zero), plain, "all-zero spec")
    # a whole modality
    no_text = materialise(store, {m: np.full(int(store.length[m].sum()), m == "text") for m in MODS})
    assert not bool(no_text.packed["text"].any()) and not bool(no_text.packed_p3["text"].any())
    got = ev(store.with_missing(modality={"text": 1.0}, seed=3))
    want = ev(no_text)
    torch.cuda.synchronize()
    _assert_eval_equal(got, want, "modality text = 1")
    assert torch.equal(got.preds[1], plain.preds[1]) and not torch.equal(got.preds[0], plain.preds[0])      # the missing stream reads feat4
    # the curve
    runner = env.evaluate.Evaluator(flat, dims)
    curve = env.evaluate.missing_curve(runner, store, env.batches, (0, .5, 1), seed=1234, draw=2)
    assert [c["rate"] for c in curve] == [0.0, 0.5, 1.0] and all(set(c) == {"rate", "full", "missing"} for c in curve)
    assert {k: curve[0][k] for k in ("full", "missing")} == plain.metrics(store)
    ends = []
    for rate in (.5, 1.0):
        m = materialise(store, rule_rows(store, frame={"audio": rate, "video": rate}, seed=1234, draw=2))
        ends.append(runner.eval_epoch(m, env.batches).metrics(store))
    assert {k: curve[1][k] for k in ("full", "missing")} == ends[0]
    assert {k: curve[2][k] for k in ("full", "missing")} == ends[1]
    assert curve[2]["full"] != curve[0]["full"]
    # kind='modality' on a trainer: whole utterances lose audio and video
    tr = env.engine.FusedTrainer(flat.clone(), dims, capacity=(8, TCAP))
    cm = env.evaluate.missing_curve(tr, store, env.batches, (0.5,), kind="modality", seed=7)
    m = materialise(store, rule_rows(store, modality={"audio": .5, "video": .5}, seed=7))
    assert {k: cm[0][k] for k in ("full", "missing")} == runner.eval_epoch(m, env.batches).metrics(store)
    with pytest.raises(env._lib.SdumcError):
        env.evaluate.missing_curve(runner, store, env.batches, (0.5, 1.5))
    with pytest.raises(env._lib.SdumcError):
        env.evaluate.missing_curve(runner, store, env.batches, (0.5,), kind="frames")


def test_materialized_is_the_test_built_store(env):
    """view.materialized(): a new ordinary store holding the bits of the store this file builds by hand, planes included"""
    for mode in ("fp32", "bf16"):
        got, want = env.view(mode).materialized(), env.mat(mode)
        assert type(got) is env.data.DeviceFeatureStore and got is not env.store[mode]
        for m in MODS:
            assert torch.equal(got.packed[m], want.packed[m]) and got.packed[m].data_ptr() != env.store[mode].packed[m].data_ptr()
            if mode == "fp32":
                assert torch.equal(got.packed_p3[m], want.packed_p3[m])
        assert (got.packed_p3 is None) == (mode == "bf16") and len(got) == N_UTT and got.get_featdim() == env.store[mode].get_featdim()
    assert env.view("fp32").materialized(planes=False).packed_p3 is None
    # the host rule of the view agrees row by row
    for m in MODS:
        np.testing.assert_array_equal(env.view("fp32").absent_rows(m), env.absent("fp32")[m])


@pytest.mark.parametrize("inplace", [True, False])
def test_saliency(env, inplace):
    """7. saliency_epoch(view) = saliency_epoch(materialised), bit for bit; gradient x input of an absent frame is exactly 0"""
    mode = "fp32"
    run = lambda s: env.saliency.saliency_epoch(env.flat[mode], DIMS[mode], s, env.batches, inplace=inplace)
    got = run(env.view(mode))
    want = run(env.mat(mode))
    torch.cuda.synchronize()
    assert _same(got.preds, want.preds) and torch.equal(got.seen, want.seen)
    absent = env.absent(mode)
    for name, d in got.maps.items():
        for m, t in d.items():
            assert _same(t, want.maps[name][m]), (name, m)
            assert bool(torch.isfinite(t).all())
            rows = torch.from_numpy(absent[m]).cuda()
            assert not bool(t[rows, 0].any()), (name, m)      # (+0 or -0)
            if m in ("audio", "text"):
                assert bool((t[~rows, 0] != 0).any()) and bool((t[rows, 1] > 0).any())      # present frames have one; the gradient itself does not vanish


def test_errors_before_launch(env):
    """8. view.resampled raises; a descriptor with the spec enabled and a modality index of 4 is SDUMC_EINVAL and nothing is written"""
    view = env.view("fp32")
    with pytest.raises(env._lib.SdumcError, match="pool first"):
        view.resampled(2)
    assert isinstance(env.store["fp32"].resampled(2).with_missing(**SPEC_A), env.data.MissingView)      # pool first, then view

    def bad_mod(g):
        assert g.miss_enable == 1 and [g.seg[k].miss_mod for k in range(4)] == [0, 1, 2, 3]
        g.seg[3].miss_mod = 4
    maps, lens, rc = env.maps(view, env.batches[0], poison=bad_mod)
    assert rc == -1
    assert all(bool((t == -7).all()) for t in maps + lens)

    def bad_flag(g):
        g.seg[0].miss_all = 4
    assert env.maps(view, env.batches[0], poison=bad_flag)[2] == -1

    def off(g):      # the same fields with the spec switched off: today's behaviour, whatever they hold
        g.seg[3].miss_mod = 4
        g.miss_enable = 0
    maps, _, rc = env.maps(view, env.batches[0], poison=off)
    plain, _, _ = env.maps(env.store["fp32"], env.batches[0])
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(maps, plain))
