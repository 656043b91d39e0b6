"""Saliency maps (sdumc_amd/saliency.py; sdumc_frame_saliency, csrc/frame_saliency.hip): per stream, modality and frame the
gradient x input (column 0) and the gradient norm (column 1) of the eval-mode prediction, in store order.

Kernel level: against fp64 at six (B, T, d), through padded features and through a row map, with the bound one fp32 rounding of an
fp64 sum of at most 4096 exact products leaves:
    |got0 - s| <= 2^-23 sum_c |g_c x_c| + 2^-149          |got1 - r| <= 2^-23 r + 2^-149
nothing written outside the rows the contract names, launches repeatable, bits independent of batch order and padded length,
non-finite values confined to their row, refusals that launch nothing.
Epoch level: every stream and modality against the fp64 reference model with the inputs as leaves (the route of
tests/test_gpu_input_grads.py::_oracle, eval mode, one-hot d_vals) at the project's gradient bar BAR = 2e-4: with G the reference's
feature gradient of the padded batch and X its features, over the exported frames of a batch
    ||got0 - want0||_2 <= BAR ||G||_F max_row ||X_row||_2    (Cauchy-Schwarz on the bar d_feat is held to)
    ||got1 - want1||_2 <= BAR ||want1||_2
then the composition bit for bit against engine.NetCall + the kernel by hand, in place = gathered, out= reuse, one stream alone,
predictions = eval_epoch's, a training run untouched, the refusals, and the nn.Module route."""
import ctypes as C

import pytest
import torch

from tests.test_gpu_input_grads import BAR, _module, _oracle
from tests.test_gpu_net import flat_from

pytestmark = pytest.mark.gpu

POISON = -77.0
STREAMS = (("full", ("audio", "text", "video")), ("missing", ("audio", "feat4", "video")))
MODS = ("audio", "text", "video", "feat4")
TINY = 2.0 ** -149


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import _lib
    return _lib


def _desc_array(L, items):
    arr = (L.SaliencyDesc * len(items))()
    for p, it in zip(arr, items):
        for k, v in it.items():
            setattr(p, k, v.data_ptr() if torch.is_tensor(v) else v)
    return arr


def _launch(L, items, idx):
    rc = L.lib.sdumc_frame_saliency(_desc_array(L, items), len(items), idx.data_ptr(), L.current_stream())
    torch.cuda.synchronize()
    return rc


# ---------------------------------------------------------------- 1. the kernel against fp64
def _lengths(T):
    return [T, 1, 0, max(1, T // 2), T, min(T, 2), max(1, T - 1)]      # seven utterances: lengths T, 1 and 0 among them


class _Case:
    """One kernel problem: a 7-utterance store-shaped destination, a batch of B valid samples (a permuted subset of the utterances)
    plus ONE sample whose index is out of range, padded features and the same features packed behind a row map (some VALID frames'
    entries name the trailing zero row, some lie outside the packed tensor: both read as a zero row)."""

    def __init__(self, B, T, d, seed=0):
        g = torch.Generator().manual_seed(1000 * T + d + seed)
        lens = _lengths(T)
        self.lens, self.n_utt, self.T, self.d = lens, len(lens), T, d
        self.start = [sum(lens[:i]) for i in range(7)]
        self.rows = sum(lens)
        valid = [0, 2, 1, 4, 3][:B][::-1]
        bad = (7, -1)[B % 2]
        self.idx = valid[:B // 2] + [bad] + valid[B // 2:]
        self.B = B + 1
        self.grad = torch.randn(self.B, T, d, generator=g)
        self.feat = torch.randn(self.B, T, d, generator=g) * 3
        # the packed copy: the valid frames of every in-range sample in batch order, then the zero row
        packed, rmap, self.feat_eff = [], torch.zeros(self.B, T, dtype=torch.int32), self.feat.clone()
        n = 0
        for b, e in enumerate(self.idx):
            ln = lens[e] if 0 <= e < 7 else 0
            for t in range(ln):
                packed.append(self.feat[b, t])
                rmap[b, t] = n
                n += 1
        self.store_rows = n + 1
        for b in range(self.B):
            for t in range(T):
                e = self.idx[b]
                ln = lens[e] if 0 <= e < 7 else 0
                if t >= ln:
                    rmap[b, t] = n                        # a padded frame: the zero row
                elif (b + t) % 5 == 3:
                    rmap[b, t] = n                        # a valid frame reading the zero row
                    self.feat_eff[b, t] = 0
                elif (b + t) % 5 == 4:
                    rmap[b, t] = (n + 4, -1)[t % 2]       # ... and one outside the packed tensor
                    self.feat_eff[b, t] = 0
        self.packed = torch.cat([torch.stack(packed) if packed else torch.zeros(0, d), torch.zeros(1, d)])
        self.rmap = rmap.reshape(-1)

    def expected(self, feat):
        """{destination row: (s, sum |g x|, r)} in fp64"""
        out = {}
        for b, e in enumerate(self.idx):
            if not 0 <= e < 7:
                continue
            for t in range(self.lens[e]):
                gx = self.grad[b, t].double() * feat[b, t].double()
                out[self.start[e] + t] = (float(gx.sum()), float(gx.abs().sum()), float(self.grad[b, t].double().pow(2).sum().sqrt()))
        return out

    def device(self):
        dev = {k: getattr(self, k).cuda() for k in ("grad", "feat", "packed", "rmap")}
        dev["idx"] = torch.tensor(self.idx, dtype=torch.int64).cuda()
        dev["start"] = torch.tensor(self.start, dtype=torch.int64).cuda()
        dev["length"] = torch.tensor(self.lens, dtype=torch.int32).cuda()
        return dev

    def items(self, dev, dst_pad, dst_map):
        common = dict(grad=dev["grad"], start=dev["start"], length=dev["length"], n_utt=7, dst_rows=self.rows, B=self.B, T=self.T, d=self.d)
        return [dict(common, feat=dev["feat"], dst=dst_pad), dict(common, feat=dev["packed"], row_map=dev["rmap"], store_rows=self.store_rows, dst=dst_map)]


GUARD = 16


def _check(case, got, feat, what):
    want = case.expected(feat)
    got = got.cpu()
    worst = [0.0, 0.0]
    for row in range(case.rows + GUARD):
        if row not in want:
            assert float(got[row, 0]) == POISON and float(got[row, 1]) == POISON, f"{what}: row {row} was written"
            continue
        s, a, r = want[row]
        e0, e1 = abs(float(got[row, 0].double()) - s), abs(float(got[row, 1].double()) - r)
        b0, b1 = 2.0 ** -23 * a + TINY, 2.0 ** -23 * r + TINY
        worst = [max(worst[0], e0 / b0), max(worst[1], e1 / b1)]
        assert e0 <= b0 and e1 <= b1, f"{what}: row {row}: |got0 - s| = {e0:.3e} (bound {b0:.3e}), |got1 - r| = {e1:.3e} (bound {b1:.3e})"
    print(f"{what}: worst error / bound = {worst[0]:.3f} (column 0), {worst[1]:.3f} (column 1); {len(want)} rows")


@pytest.mark.parametrize("B,T,d", [(1, 1, 4), (1, 3, 6), (3, 5, 20), (2, 70, 48), (3, 66, 256), (2, 9, 4096)])
def test_kernel_against_fp64(L, B, T, d):
    case = _Case(B, T, d)
    dev = case.device()
    dst = [torch.full((case.rows + GUARD, 2), POISON, device="cuda") for _ in range(2)]
    assert len(case.expected(case.feat)) == sum(case.lens[e] for e in case.idx if 0 <= e < 7) > 0
    assert _launch(L, case.items(dev, *dst), dev["idx"]) == 0
    _check(case, dst[0], case.feat, f"({B}, {T}, {d}) padded features")
    _check(case, dst[1], case.feat_eff, f"({B}, {T}, {d}) row-mapped features")
    if T >= 5:
        assert not torch.equal(case.feat_eff, case.feat)      # (some valid frames did read the zero row)
    # a destination shorter than the store's frames: the rows beyond it are skipped, the others are the same bits
    cut = case.rows - 1
    if cut >= 1:
        short = torch.full((case.rows + GUARD, 2), POISON, device="cuda")
        items = case.items(dev, short, short)[:1]
        items[0]["dst_rows"] = cut
        assert _launch(L, items, dev["idx"]) == 0
        assert torch.equal(short[:cut], dst[0][:cut]) and bool((short[cut:] == POISON).all())


# ---------------------------------------------------------------- 2. repeatability, layout independence
@pytest.mark.parametrize("d", [48, 70, 256, 1028])
def test_repeatable_and_independent_of_the_batch_layout(L, d):
    g = torch.Generator().manual_seed(d)
    lens = [5, 1, 7, 3]
    start = [0, 5, 6, 13]
    G = [torch.randn(n, d, generator=g) for n in lens]
    X = [torch.randn(n, d, generator=g) for n in lens]
    tables = dict(start=torch.tensor(start, dtype=torch.int64).cuda(), length=torch.tensor(lens, dtype=torch.int32).cuda(), n_utt=4,
                  dst_rows=sum(lens))

    def run(order, T):
        grad, feat = torch.randn(len(order), T, d, generator=g), torch.randn(len(order), T, d, generator=g)      # (noise in the padding)
        for b, e in enumerate(order):
            grad[b, :lens[e]], feat[b, :lens[e]] = G[e], X[e]
        dst = torch.full((sum(lens), 2), POISON, device="cuda")
        item = dict(tables, grad=grad.cuda(), feat=feat.cuda(), dst=dst, B=len(order), T=T, d=d)
        idx = torch.tensor(order, dtype=torch.int64).cuda()
        assert _launch(L, [item], idx) == 0
        again = torch.full_like(dst, POISON)
        assert _launch(L, [dict(item, dst=again)], idx) == 0
        assert torch.equal(dst, again), "two launches differ"
        return dst

    one = run([0, 1, 2], 7)
    other = run([2, 3, 0, 1], 12)
    assert bool((one[:13] != POISON).all()) and bool((one[13:] == POISON).all()) and bool((other != POISON).all())
    assert torch.equal(one[:13], other[:13]), "the same grad / feat rows gave other bits in another batch order and padded length"


# ---------------------------------------------------------------- 3. non-finite values
def test_non_finite_values_stay_in_their_row(L):
    case = _Case(3, 5, 20, seed=1)
    dev = case.device()
    clean = torch.full((case.rows, 2), POISON, device="cuda")
    assert _launch(L, case.items(dev, clean, clean)[:1], dev["idx"]) == 0
    b = case.idx.index(0)      # utterance 0 has every frame
    grad = case.grad.clone()
    grad[b, 2, 3], grad[b, 2, 11] = float("nan"), float("inf")
    dirty = torch.full((case.rows, 2), POISON, device="cuda")
    items = case.items(dict(dev, grad=grad.cuda()), dirty, dirty)[:1]
    assert _launch(L, items, dev["idx"]) == 0
    row = case.start[0] + 2
    assert not bool(torch.isfinite(dirty[row]).any())
    keep = torch.ones(case.rows, dtype=torch.bool, device="cuda")
    keep[row] = False
    assert torch.equal(dirty[keep], clean[keep]) and bool(torch.isfinite(clean[clean[:, 0] != POISON]).all())


# ---------------------------------------------------------------- 4. refusals launch nothing
def test_refusals_launch_nothing(L):
    case = _Case(2, 9, 48)
    dev = case.device()
    dst = [torch.full((case.rows + GUARD, 2), POISON, device="cuda") for _ in range(2)]
    idx = dev["idx"]

    def attempt(spoil, k=1, n=2, idx_ptr=idx.data_ptr(), none=False):
        arr = _desc_array(L, case.items(dev, *dst))
        spoil(arr[k])
        rc = L.lib.sdumc_frame_saliency(None if none else arr, n, idx_ptr, L.current_stream())
        torch.cuda.synchronize()
        return rc

    bad = {"descs NULL": attempt(lambda p: None, none=True), "idx NULL": attempt(lambda p: None, idx_ptr=None),
           "n = 0": attempt(lambda p: None, n=0), "n = 5": attempt(lambda p: None, n=5)}
    for f in ("grad", "feat", "start", "length", "dst"):
        bad[f + " NULL"] = attempt(lambda p: setattr(p, f, None))
    for f in ("B", "T", "d", "n_utt", "dst_rows"):
        bad[f + " = 0"] = attempt(lambda p: setattr(p, f, 0))
    bad["another B"] = attempt(lambda p: setattr(p, "B", 1))
    bad["row_map with store_rows = 0"] = attempt(lambda p: setattr(p, "store_rows", 0))
    bad["misaligned grad"] = attempt(lambda p: setattr(p, "grad", p.grad + 4))
    bad["misaligned dst"] = attempt(lambda p: setattr(p, "dst", p.dst + 8))
    bad["misaligned feat, d % 4 == 0"] = attempt(lambda p: setattr(p, "feat", p.feat + 4), k=0)
    assert all(rc == -1 for rc in bad.values()), bad
    assert all(bool((t == POISON).all()) for t in dst)
    assert attempt(lambda p: None) == 0 and not bool((dst[0] == POISON).all()) and not bool((dst[1] == POISON).all())
    # d % 4 != 0: a feature tensor at any 4-byte address is taken (the scalar path)
    odd = _Case(1, 3, 6)
    od = odd.device()
    shifted = torch.zeros(od["feat"].numel() + 1, device="cuda")
    shifted[1:] = od["feat"].reshape(-1)
    a, b = (torch.full((odd.rows, 2), POISON, device="cuda") for _ in range(2))
    assert _launch(L, odd.items(od, a, a)[:1], od["idx"]) == 0
    assert _launch(L, odd.items(dict(od, feat=shifted[1:]), b, b)[:1], od["idx"]) == 0
    assert torch.equal(a, b)


# ---------------------------------------------------------------- the epoch
SHAPES = {"generic": (48, 32, 40, 32), "kernel": (256, 512, 256, 512)}
LEN7 = {"audio": (70, 9, 33, 1, 66, 40, 17), "text": (9, 2, 5, 1, 7, 3, 4), "video": (33, 12, 1, 20, 7, 30, 5), "feat4": (4, 1, 2, 3, 1, 4, 2)}
BATCHES = ((4, 0, 2), (6, 1, 5), (3,))


class _Env:
    def __init__(self):
        from oracle import sdumc_oracle as O
        from sdumc_amd import engine, evaluate, saliency
        from sdumc_amd.data import DeviceFeatureStore
        self.O, self.E, self.evaluate, self.S = O, engine, evaluate, saliency
        self.P, self.flat, self.store = {}, {}, {}
        for key, dims in SHAPES.items():
            self.P[key] = O.init_params(dims, seed=11)
            self.flat[key] = flat_from(engine, self.P[key], dims)[0]
            g = torch.Generator().manual_seed(5)
            inst = [{"emo": 0, "val": 0.5 * i - 1.5, "name": f"s{i}", **{m: torch.randn(LEN7[m][i], d, generator=g) for m, d in zip(MODS, dims)}}
                    for i in range(7)]
            self.store[key] = DeviceFeatureStore(inst, device="cuda", planes=key == "kernel")
        self.batches = [torch.tensor(b, dtype=torch.int64) for b in BATCHES]
        self._refs = {}

    def run(self, key, batches=None, **kw):
        return self.S.saliency_epoch(self.flat[key], SHAPES[key], self.store[key], self.batches if batches is None else batches, **kw)

    def reference(self, key, key_padding):
        """per batch: [stream] -> ((G_audio, G_textslot, G_video), (X_audio, X_textslot, X_video)), fp64 on the padded batch"""
        k = (key, key_padding)
        if k not in self._refs:
            store, outs = self.store[key], []
            for ix in self.batches:
                b = store.batch(ix)[0]
                audio, text, video, feat4 = (b[n].cpu() for n in ("audios", "texts", "videos", "feat4s"))
                B = ix.numel()
                lens = [store.length[m][ix].tolist() for m in MODS] if key_padding else None
                per = []
                for s in range(2):
                    dv = torch.zeros(2 * B, 1)
                    dv[s * B:(s + 1) * B] = 1.0
                    douts = [dv, torch.zeros(2 * B, 128), torch.zeros(2 * B, 64), torch.zeros(2 * B, 256), torch.zeros(2 * B, 7, 128)]
                    _, ga, gt, gv = _oracle(self.P[key], audio, [text, feat4], video, "eval", 0, 0, douts, lengths=lens)
                    per.append(((ga, gt[s], gv), (audio.double(), (text, feat4)[s].double(), video.double())))
                outs.append(per)
            self._refs[k] = outs
        return self._refs[k]


@pytest.fixture(scope="module")
def env(L):
    return _Env()


def _maps(res):
    torch.cuda.synchronize()
    return {s: {m: t.cpu() for m, t in d.items()} for s, d in res.maps.items()}


def _exported(store, m, ix, t_bt2):
    """[B, T, 2] of a padded batch -> the rows of its exported frames, in batch order"""
    return torch.cat([t_bt2[b, :int(store.length[m][i])] for b, i in enumerate(ix.tolist())])


def _rows_of(store, m, ix, packed):
    return torch.cat([packed[int(store.start[m][i]):int(store.start[m][i]) + int(store.length[m][i])] for i in ix.tolist()])


def _hold(got, G, X, want, what):
    """the two bounds of the module docstring over one batch's exported frames of one (stream, modality)"""
    got, want = got.double(), want.double()
    e0, e1 = float((got[:, 0] - want[:, 0]).norm()), float((got[:, 1] - want[:, 1]).norm())
    b0, b1 = BAR * float(G.double().norm()) * float(X.double().norm(dim=-1).max()), BAR * float(want[:, 1].norm())
    print(f"{what}: column 0 error / bound = {e0 / b0:.3e}, column 1 error / bound = {e1 / b1:.3e} ({got.shape[0]} frames)")
    assert bool(torch.isfinite(got).all()) and e0 <= b0 and e1 <= b1, f"{what}: {e0:.3e} vs {b0:.3e}, {e1:.3e} vs {b1:.3e}"


@pytest.mark.parametrize("key_padding", [False, True])
@pytest.mark.parametrize("key", list(SHAPES))
def test_epoch_against_the_fp64_reference(env, key, key_padding):
    store = env.store[key]
    res = env.run(key, key_padding=key_padding)
    assert env.S._saliency[1]._in_place(store) == (key == "kernel")
    maps = _maps(res)
    assert int((res.seen != 0).sum()) == 7 and all(bool(torch.isfinite(t).all()) for d in maps.values() for t in d.values())
    for ix, ref in zip(env.batches, env.reference(key, key_padding)):
        for s, (name, mods) in enumerate(STREAMS):
            for j, m in enumerate(mods):
                G, X = ref[s][0][j], ref[s][1][j]
                want = _exported(store, m, ix, env.S.frame_scores(G, X))
                _hold(_rows_of(store, m, ix, maps[name][m]), G, X, want, f"{key} key_padding={key_padding} batch {ix.tolist()} {name}/{m}")


def _by_hand(env, L, key, key_padding):
    """the maps of an epoch over env.batches from engine.NetCall on store.batch's padded copies (a forward in front of every backward)
    and sdumc_frame_saliency by hand"""
    store, flat = env.store[key], env.flat[key]
    rows = env.S.frame_rows(store)
    out = {name: {m: torch.full((rows[m], 2), float("nan"), device="cuda") for m in mods} for name, mods in STREAMS}
    for ix in env.batches:
        b = store.batch(ix)[0]
        feats = {"audio": b["audios"], "text": b["texts"], "video": b["videos"], "feat4": b["feat4s"]}
        B = ix.numel()
        lengths = [store.length[m][ix] for m in MODS] if key_padding else None
        nc = env.E.NetCall(flat, feats["audio"], [feats["text"], feats["feat4"]], feats["video"], False, None, planes=key == "kernel",
                           lengths=lengths)
        idx = ix.cuda()
        for s, (name, mods) in enumerate(STREAMS):
            seed = torch.zeros(2 * B, 1, device="cuda")
            seed[s * B:(s + 1) * B] = 1.0
            nc.forward()
            nc.backward(seed, None, None, None, None, feature_grads=(True, s == 0, s == 1, True))
            da, dt, dv = nc.d_inputs
            items = [dict(grad=g, feat=feats[m], start=store.start_d[m], length=store.length_d[m], n_utt=7, dst=out[name][m],
                          dst_rows=rows[m], B=B, T=g.shape[1], d=g.shape[2]) for m, g in zip(mods, (da, dt[s], dv))]
            assert _launch(L, items, idx) == 0
    return out


@pytest.mark.parametrize("key_padding", [False, True])
@pytest.mark.parametrize("key", list(SHAPES))
def test_composition_bit_for_bit(env, L, key, key_padding):
    hand = _by_hand(env, L, key, key_padding)
    gathered = env.run(key, key_padding=key_padding, inplace=False)
    torch.cuda.synchronize()
    assert not env.S._saliency[1]._in_place(env.store[key])
    for name, mods in STREAMS:
        for m in mods:
            assert torch.equal(gathered.maps[name][m], hand[name][m]), (name, m)
    inplace = env.run(key, key_padding=key_padding)
    ptrs = [t.data_ptr() for d in inplace.maps.values() for t in d.values()]
    one = env.run(key, key_padding=key_padding, streams=("missing",))
    sub = env.run(key, key_padding=key_padding, batches=env.batches[:1])
    torch.cuda.synchronize()
    assert tuple(one.maps) == ("missing",) and int((sub.seen != 0).sum()) == 3
    for name, mods in STREAMS:
        for m in mods:
            assert torch.equal(inplace.maps[name][m], gathered.maps[name][m]), (name, m)
            if name == "missing":
                assert torch.equal(one.maps[name][m], gathered.maps[name][m]), m
    assert torch.equal(one.preds, gathered.preds) and torch.equal(one.seen, gathered.seen)
    # out= reuse, after an epoch over other rows left NaN in it
    again = env.run(key, key_padding=key_padding, out=sub)
    torch.cuda.synchronize()
    assert again is sub and all(torch.equal(sub.maps[n][m], gathered.maps[n][m]) for n, mods in STREAMS for m in mods)
    assert [t.data_ptr() for d in inplace.maps.values() for t in d.values()] == ptrs
    # a subset epoch: the other utterances' rows stay NaN, of() serves the visited ones only
    store = env.store[key]
    part = env.run(key, key_padding=key_padding, batches=env.batches[1:])
    torch.cuda.synchronize()
    for i in range(7):
        visited = i not in BATCHES[0]
        for name, mods in STREAMS:
            for m in mods:
                t = part.maps[name][m][int(store.start[m][i]):int(store.start[m][i]) + int(store.length[m][i])]
                assert bool(torch.isfinite(t).all()) if visited else bool(torch.isnan(t).all()), (i, name, m)
    assert part.of(store, "s6")["missing"]["feat4"].shape == (LEN7["feat4"][6], 2)
    with pytest.raises(L.SdumcError):
        part.of(store, BATCHES[0][0])


def _snapshot(res):
    torch.cuda.synchronize()
    return [res.preds.clone(), res.seen.float()] + [t.clone() for d in res.maps.values() for t in d.values()]


@pytest.mark.parametrize("key", list(SHAPES))
def test_a_later_epoch_grows_the_arena_and_an_earlier_plan_reuses_it(env, key):
    """ONE Saliency object and ONE result (out= throughout) over an epoch of small batches, then over one whose largest batch has more
    samples and a longer T in every modality: the arena gives way to a larger one and the epoch holds the bits of a fresh object's;
    a third epoch over the first plan runs in the grown arena (the same workspace) and reproduces the first bit for bit."""
    store, flat, dims = env.store[key], env.flat[key], SHAPES[key]
    small = [torch.tensor(b, dtype=torch.int64) for b in ((3,), (6, 1))]
    large = [torch.tensor(b, dtype=torch.int64) for b in ((4, 0, 2, 5), (6, 1, 3))]
    sal = env.S.Saliency(flat, dims)
    out = sal.saliency_epoch(store, small)
    one, first = _snapshot(out), sal.arena
    assert first.B == 2 and int((out.seen != 0).sum()) == 3 and bool(torch.isnan(out.maps["full"]["audio"]).any())
    assert sal.saliency_epoch(store, large, out=out) is out
    two, grown = _snapshot(out), sal.arena
    assert grown is not first and grown.B == 4 and all(t > c for t, c in zip(grown.T, first.T))
    fresh = _snapshot(env.S.Saliency(flat, dims).saliency_epoch(store, large))
    assert int((out.seen != 0).sum()) == 7 and len(two) == len(fresh) == 8      # (every row visited: no NaN to step around)
    for x, y in zip(two, fresh):
        assert torch.equal(x, y)
    ws = grown.workspace.data_ptr()
    assert sal.saliency_epoch(store, small, out=out) is out
    three = _snapshot(out)
    assert sal.arena is grown and sal.arena.workspace.data_ptr() == ws and (sal.arena.B, sal.arena.T) == (4, grown.T)
    for x, y in zip(three, one):
        assert torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))
    assert bool(torch.isnan(three[0][:, [0, 2, 4, 5]]).all()) and bool(torch.isfinite(three[0][:, [1, 3, 6]]).all())


@pytest.mark.parametrize("key", list(SHAPES))
def test_predictions_are_eval_epochs(env, key):
    for kp in (False, True):
        for inplace in (True, False):
            sal = env.run(key, key_padding=kp, inplace=inplace)
            ev = env.evaluate.eval_epoch(env.flat[key], SHAPES[key], env.store[key], env.batches, key_padding=kp, inplace=inplace)
            torch.cuda.synchronize()
            assert torch.equal(sal.preds, ev.preds) and torch.equal(sal.seen, ev.seen) and bool(torch.isfinite(sal.preds).all())


def test_a_training_run_is_untouched(env):
    key = "kernel"
    dims, store = SHAPES[key], env.store[key]
    cap = (3, tuple(max(LEN7[m]) for m in MODS))
    runs = []
    for with_saliency in (False, True):
        flat = env.flat[key].clone()
        tr = env.E.FusedTrainer(flat, dims, lr=1e-3, seed=11, capacity=cap)
        plan = store.plan_epoch(env.batches)
        tr.run_epoch(store, plan)
        if with_saliency:
            torch.cuda.synchronize()
            before = [flat.clone(), tr.state.adam_m.clone(), tr.state.adam_v.clone(), tr.state.hyper.clone(), tr.state.rng.t.clone()]
            res = tr.saliency_epoch(store, env.batches)
            torch.cuda.synchronize()
            after = [flat, tr.state.adam_m, tr.state.adam_v, tr.state.hyper, tr.state.rng.t]
            for x, y, what in zip(before, after, ("parameters", "adam_m", "adam_v", "step count", "dropout counter")):
                assert torch.equal(x, y), what
            assert int((res.seen != 0).sum()) == 7 and all(bool(torch.isfinite(t).all()) for d in res.maps.values() for t in d.values())
            assert isinstance(res, env.S.SaliencyResult) and tr.saliency_epoch(store, env.batches, out=res) is res
        tr.run_epoch(store, plan)
        torch.cuda.synchronize()
        runs.append((flat, tr.state.adam_m, tr.state.adam_v, tr.state.hyper, tr.state.rng.t))
    for x, y, what in zip(runs[0], runs[1], ("parameters", "adam_m", "adam_v", "hyper", "rng")):
        assert torch.equal(x, y), what
    assert not torch.equal(runs[0][0], env.flat[key])


def test_refusals_before_any_launch(env, L):
    key = "kernel"
    store, flat, dims = env.store[key], env.flat[key], SHAPES[key]
    out = env.run(key)
    torch.cuda.synchronize()
    for t in [out.preds] + [t for d in out.maps.values() for t in d.values()]:
        t.fill_(5.0)
    out.seen.fill_(1)

    def untouched():
        torch.cuda.synchronize()
        return bool((out.preds == 5.0).all()) and bool((out.seen == 1).all()) and all(bool((t == 5.0).all()) for d in out.maps.values() for t in d.values())

    with pytest.raises(L.SdumcError, match="fp32 storage only"):      # bf16 storage
        env.E.FusedTrainer(flat, dims, bf16=True).saliency_epoch(store, env.batches, out=out)
    with pytest.raises(L.SdumcError, match="more than once"):
        env.run(key, batches=[torch.tensor([0, 1]), torch.tensor([1, 2])], out=out)
    with pytest.raises(L.SdumcError, match="out of range"):
        env.run(key, batches=[torch.tensor([0, 7])], out=out)
    with pytest.raises(L.SdumcError, match="feature widths"):
        env.S.saliency_epoch(flat, dims, env.store["generic"], env.batches, out=out)
    with pytest.raises(L.SdumcError, match="unknown stream"):
        env.run(key, streams=("full", "text"), out=out)
    with pytest.raises(L.SdumcError, match="out="):      # a result of other streams, of another store's size, of another type
        env.run(key, streams=("missing",), out=out)
    with pytest.raises(L.SdumcError, match="out="):
        env.run(key, batches=env.batches[:1], out=env.S.SaliencyResult.empty(6, "cuda", env.S.frame_rows(store)))
    with pytest.raises(L.SdumcError, match="out="):
        env.run(key, out=env.evaluate.EvalResult.empty(7, "cuda"))
    assert untouched()
    assert env.run(key, out=out) is out and not untouched()


def test_module_route(env):
    """model.eval() with leaf inputs, vals.sum().backward() for the full stream: frame_scores(audio.grad, audio) against the epoch's
    'full' audio map of the same batch, at the two bounds with G = the module's gradient"""
    key = "generic"
    store, ix = env.store[key], env.batches[0]
    model = _module(SHAPES[key][:3], env.P[key])
    model.eval()
    b = store.batch(ix)[0]
    audio, text, video = (b[n].clone().requires_grad_() for n in ("audios", "texts", "videos"))
    model([audio, text, video, False])[0].sum().backward()
    want = env.S.frame_scores(audio.grad, audio.detach(), store.length["audio"][ix].cuda())
    assert LEN7["audio"][int(ix[0])] < audio.shape[1] and bool((want[0, LEN7["audio"][int(ix[0])]:] == 0).all())
    res = env.run(key, batches=[ix])
    got = _rows_of(store, "audio", ix, _maps(res)["full"]["audio"])
    _hold(got, audio.grad.cpu(), audio.detach().cpu(), _exported(store, "audio", ix, want.cpu()), "module route, full/audio")
