"""Attention maps from evaluation epochs (evaluate.eval_epoch(..., attention=True); sdumc_net_export_attention, csrc/attn_export.hip):
the softmax-over-time weights of the six poolings of both streams (vector_attention of FRA2UTT_new / Cross_Attention, model :68, :95),
per frame and in store order -- EvalResult.attention[stream][modality] is [frames of the store, 8]: column 0 FRA2UTT_new's weight,
columns 1..7 Cross_Attention's.

Fixture A is tests/test_gpu_eval_epoch.py's: 37 synthetic utterances, frame maxima (40, 6, 24, 5), min_frac 0.25, shuffled batches of
8, 8, 8, 8, 5 -- single-chunk sites, text and feat4 padded to different lengths (two text runs), a short last batch; widths
(64, 128, 64, 128) in fp32 storage with planes, (128, 128, 128, 128) in bf16 storage.
Fixture B is built from explicit instances: 24 utterances, batch k = the utterances i with i % 3 == k (store neighbours are never in
one batch).  Audio lengths ragged up to 150 with at least one >= 96 per batch (padded T = 100 / 150 / 149: several 64-frame chunks,
the last partial, and the K3 route in fp32), video ragged up to 70, text and feat4 exactly 32 frames (one merged text run: the shape
the clustered fold accepts), utterance 0 has ONE audio frame; two batchings put it first and last in its batch.

The bar against the oracle: max |error| <= 2e-5 of the largest weight of the compared tensor -- the project's output bar (README
"Parity: outputs 2e-5") applied to the tensor's own scale, not to max(1, .), which would be vacuous for weights of order 1 / T.  The
tensor here is ONE utterance's [T_i, 8] map of one (stream, modality): the smallest scale the bar can be read for.  The references
(oracle.sdumc_oracle.forward in fp64 on store.batch's padded copies, return_attn=True) are computed once and shared.
bf16 storage rounds features, projected frames and keys to 8 bits of mantissa: its maps are held to the documented bf16 activation
bar, 2e-2, on the same scale.  Every test prints the worst ratio it saw."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

N_A, TCAP_A = 37, (40, 6, 24, 5)
DIMS = {"fp32": (64, 128, 64, 128), "bf16": (128, 128, 128, 128)}
STREAMS = (("full", ("audio", "text", "video")), ("missing", ("audio", "feat4", "video")))
BAR, BAR_BF16 = 2e-5, 2e-2
B_AUDIO = (1, 150, 17, 64, 65, 128, 96, 5, 63, 33, 2, 149, 90, 77, 31, 100, 130, 12, 64, 97, 45, 8, 129, 70)
B_VIDEO = (70, 3, 25, 64, 1, 65, 40, 13, 9, 70, 33, 2, 64, 50, 21, 66, 7, 69, 30, 1, 58, 64, 15, 44)
N_B, B_TEXT = len(B_AUDIO), 32


def _batches_a(seed, sizes=(8, 8, 8, 8, 5)):
    p = torch.randperm(N_A, generator=torch.Generator().manual_seed(seed))
    out, o = [], 0
    for b in sizes:
        out.append(p[o:o + b].clone())
        o += b
    return out


def _batches_b(first):
    """batch k = utterances k, k + 3, ...; utterance 0 (one audio frame) first or last in batch 0, the others in two fixed orders"""
    out = []
    for k in range(3):
        ix = list(range(k, N_B, 3))
        if k == 0 and not first:
            ix = ix[1:] + ix[:1]
        elif k and not first:
            ix = ix[::-1]
        out.append(torch.tensor(ix, dtype=torch.int64))
    return out


class _Env:
    def __init__(self):
        from oracle import sdumc_oracle as O
        from sdumc_amd import engine, evaluate, _lib
        from sdumc_amd.data import DeviceFeatureStore
        self.O, self.engine, self.evaluate, self._lib = O, engine, evaluate, _lib
        self.P, self.flat, self.store, self.batches = {}, {}, {}, {}
        for mode, dims in DIMS.items():
            self.P[mode] = O.init_params(dims, seed=8)
            lay = engine.ParamLayout.get(*dims[:3])
            flat = torch.zeros(lay.total)
            for k, v in lay.views(flat).items():
                v.copy_(self.P[mode][k])
            self.flat[mode] = flat.cuda()
            self.store["A", mode] = DeviceFeatureStore.synthetic(N_A, TCAP_A, dims, seed=5, min_frac=0.25, bf16=mode == "bf16",
                                                                 planes=mode == "fp32")
        g = torch.Generator().manual_seed(21)
        d = DIMS["fp32"]
        inst = [{"audio": torch.randn(B_AUDIO[i], d[0], generator=g), "text": torch.randn(B_TEXT, d[1], generator=g),
                 "video": torch.randn(B_VIDEO[i], d[2], generator=g), "feat4": torch.randn(B_TEXT, d[3], generator=g),
                 "emo": 0, "val": 0.25 * i - 3.0, "name": f"b{i:02d}"} for i in range(N_B)]
        self.store["B", "fp32"] = DeviceFeatureStore(inst, device="cuda", planes=True)
        self.batches["A"], self.batches["A2"] = _batches_a(1), _batches_a(2, sizes=(5, 8, 8, 8, 8))
        self.batches["B"], self.batches["B2"] = _batches_b(True), _batches_b(False)
        sa, sb = self.store["A", "fp32"], self.store["B", "fp32"]
        assert len({sa.batch_shape(ix) for ix in self.batches["A"]}) == 5
        assert all(sa.batch_shape(ix)[1][1] != sa.batch_shape(ix)[1][3] for ix in self.batches["A"])      # two text runs in every batch
        for ix in self.batches["B"]:
            T = sb.batch_shape(ix)[1]
            assert T[0] >= 96 and T[0] % 64 and T[1] == T[3] == 32
        assert sb.batch_shape(self.batches["B"][0])[1][2] == 70 and int(sb.length["audio"][0]) == 1
        assert int(self.batches["B"][0][0]) == 0 and int(self.batches["B2"][0][-1]) == 0
        self._refs = {}

    def reference(self, fixture, mode, key_padding):
        """per batch of self.batches[fixture]: [stream][modality slot] -> [B, T, 8] fp64 (column 0 from 'fra', 1..7 from 'cross') of the
        fp64 oracle on the padded batch the epoch evaluates (store.batch)"""
        key = (fixture, mode, key_padding)
        if key not in self._refs:
            O, store = self.O, self.store[fixture[0], mode]
            P = {k: v.double() for k, v in self.P[mode].items()}
            outs = []
            for ix in self.batches[fixture]:
                b = store.batch(ix)[0]
                audio, video = b["audios"].cpu().double(), b["videos"].cpu().double()
                per = []
                for s, (tk, tm) in enumerate((("texts", "text"), ("feat4s", "feat4"))):
                    lens = tuple(store.length[m][ix] for m in ("audio", tm, "video")) if key_padding else None
                    with torch.no_grad():
                        _, _, att = O.forward(P, audio, b[tk].cpu().double(), video, O.DropCtx("eval", 0, s), return_attn=True, lengths=lens)
                    per.append([torch.cat([att["fra"][m], att["cross"][m]], dim=2) for m in range(3)])
                outs.append(per)
            self._refs[key] = outs
        return self._refs[key]

    def run(self, fixture, mode="fp32", batches=None, **kw):
        return self.evaluate.eval_epoch(self.flat[mode], DIMS[mode], self.store[fixture[0], mode],
                                        self.batches[fixture] if batches is None else batches, bf16=mode == "bf16", **kw)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return _Env()


def _host(res):
    torch.cuda.synchronize()
    return {s: {m: t.cpu() for m, t in d.items()} for s, d in res.attention.items()}


def _utt(att, store, s, m, i):
    a, n = int(store.start[m][i]), int(store.length[m][i])
    return att[s][m][a:a + n]


def _hold_to_reference(att, store, batches, refs, bar, what):
    """every utterance, every one of the six tensors: max |got - want| <= bar * max |want| over that utterance's [T_i, 8] map"""
    worst = 0.0
    for ix, ref in zip(batches, refs):
        for s, (sname, mods) in enumerate(STREAMS):
            for mi, m in enumerate(mods):
                for b, i in enumerate(ix.tolist()):
                    got = _utt(att, store, sname, m, i).double()
                    want = ref[s][mi][b, :got.shape[0]]
                    assert got.shape == want.shape == (int(store.length[m][i]), 8)
                    ratio = float((got - want).abs().max() / want.abs().max())
                    worst = max(worst, ratio)
                    assert ratio <= bar, (what, sname, m, i, ratio)
    print(f"{what}: worst max|err| / max|weight| = {worst:.3e} (bar {bar:g})")
    return worst


@pytest.mark.parametrize("key_padding", [False, True])
@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("fixture", ["A", "B"])
def test_maps_against_the_oracle(env, fixture, inplace, key_padding):
    """1. fp32 storage: all six maps of every utterance against the fp64 oracle on the same padded batch, truncated to the utterance."""
    res = env.run(fixture, inplace=inplace, key_padding=key_padding, attention=True)
    att = _host(res)
    ev = env.evaluate._evaluator[1]
    assert ev._in_place(env.store[fixture, "fp32"]) == inplace and res.embeddings is None
    _hold_to_reference(att, env.store[fixture, "fp32"], env.batches[fixture], env.reference(fixture, "fp32", key_padding), BAR,
                       f"fixture {fixture} inplace={inplace} key_padding={key_padding}")


@pytest.mark.parametrize("cluster", [1, 0])
def test_fixture_b_with_the_clustered_stages_on_and_off(env, cluster):
    """1b. fixture B takes the clustered stages' fold (partial-only pooling passes, fold_combine normalises the stored weights) when they
    are on and the combine launches when they are off: both are held to the oracle; they are not required to be bit-equal."""
    lib = env._lib.lib
    # the routes this pair is about depend on: the clustered kernels fitting V = 2 * 8 = 16 (the fold additionally on one run per modality
    # and <= 32 chunks: the fixture's shapes), the utterance-level chain (V <= 512, SDUMC_CHAIN not 0), K3 on (SDUMC_K3 not 0, T >= 96)
    assert lib.sdumc_chain_cluster_fits_(16) == 1
    assert os.environ.get("SDUMC_CHAIN", "1") != "0" and os.environ.get("SDUMC_K3", "1") != "0"
    try:
        lib.sdumc_set_chain_cluster(cluster)
        res = env.run("B", attention=True)
        att = _host(res)
    finally:
        e = os.environ.get("SDUMC_CHAIN_CLUSTER")
        lib.sdumc_set_chain_cluster(int(e) if e else 1)
    _hold_to_reference(att, env.store["B", "fp32"], env.batches["B"], env.reference("B", "fp32", False), BAR, f"fixture B cluster={cluster}")


def _plan_offsets(_lib, dims):
    need = -_lib.lib.sdumc_debug_plan_table(C.byref(dims), None, 0)
    buf = C.create_string_buffer(need)
    assert _lib.lib.sdumc_debug_plan_table(C.byref(dims), buf, need) > 0
    return {l.split()[0]: (int(l.split()[1]), int(l.split()[2])) for l in buf.value.decode().splitlines()}


def _workspace_maps(env, mode, ix, key_padding=False):
    """[stream][modality slot] -> [B, T, 8]: the weights an eval-mode engine.NetCall on store.batch(ix) leaves in its workspace, found
    through sdumc_debug_plan_table.  Layout per run [V, T, nq], v = s * B + b; the text slot is two runs (the second behind the first)
    when the two streams' padded lengths differ."""
    store = env.store["A", mode]
    b = store.batch(ix)[0]
    lengths = [store.length[m][ix] for m in store.MODS] if key_padding else None
    nc = env.engine.NetCall(env.flat[mode], b["audios"], [b["texts"], b["feat4s"]], b["videos"], False, None, planes=True,
                            bf16=mode == "bf16", lengths=lengths)
    nc.forward()
    torch.cuda.synchronize()
    ws = nc.workspace.view(torch.float32)
    offs = _plan_offsets(env._lib, nc.dims)
    B = ix.numel()
    T = {"a": (b["audios"].shape[1],) * 2, "t": (b["texts"].shape[1], b["feat4s"].shape[1]), "v": (b["videos"].shape[1],) * 2}
    out = [[None] * 3 for _ in range(2)]
    for mi, mk in enumerate("atv"):
        (o0, n0), (o1, n1) = offs["attn0" + mk], offs["attn1" + mk]
        assert n0 == B * (T[mk][0] + T[mk][1]) and n1 == 7 * n0
        for s in range(2):
            r0, Ts = s * B * T[mk][0], T[mk][s]
            w0 = ws[o0 + r0:o0 + r0 + B * Ts].reshape(B, Ts, 1)
            w1 = ws[o1 + 7 * r0:o1 + 7 * (r0 + B * Ts)].reshape(B, Ts, 7)
            out[s][mi] = torch.cat([w0, w1], dim=2).cpu()
    return out


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_exported_rows_are_the_forwards_own_workspace_bit_for_bit(env, mode):
    """2. fixture A, in place: the exported rows equal, bitwise, what an eval-mode engine.NetCall on the same padded batch leaves in
    attn0{a,t,v} / attn1{a,t,v} -- pins stream, run, row0 and chunk-edge indexing in bf16 storage too; bf16 storage is additionally
    held to the oracle at the bf16 activation bar."""
    store = env.store["A", mode]
    res = env.run("A", mode, attention=True)
    att = _host(res)
    for ix in env.batches["A"]:
        ws = _workspace_maps(env, mode, ix)
        for s, (sname, mods) in enumerate(STREAMS):
            for mi, m in enumerate(mods):
                for b, i in enumerate(ix.tolist()):
                    got = _utt(att, store, sname, m, i)
                    assert torch.equal(got, ws[s][mi][b, :got.shape[0]]), (mode, sname, m, i)
    if mode == "bf16":
        _hold_to_reference(att, store, env.batches["A"], env.reference("A", "bf16", False), BAR_BF16, "fixture A bf16 storage")


def _column_sums(att, store, batches):
    """[visited utterances, 6 tensors, 8 columns] fp64 sums over each utterance's frames, and whether the utterance was padded"""
    sums, padded = [], []
    for ix in batches:
        T = store.batch_shape(ix)[1]
        for i in ix.tolist():
            sums.append(torch.stack([_utt(att, store, s, m, i).double().sum(0) for s, mods in STREAMS for m in mods]))
            padded.append(torch.tensor([int(store.length[m][i]) < T[store.MODS.index(m)] for s, mods in STREAMS for m in mods]))
    return torch.stack(sums), torch.stack(padded)


def test_properties_of_the_maps(env):
    """3. key_padding=True: every column of every visited utterance sums to 1 within 1e-5, and another batching of fixture A gives the
    same maps within test 1's bar; key_padding=False: the sums are at most 1 + 1e-5 and strictly below 1 where an utterance was
    padded."""
    store = env.store["A", "fp32"]
    on = _host(env.run("A", key_padding=True, attention=True))
    sums, _ = _column_sums(on, store, env.batches["A"])
    assert sums.shape == (N_A, 6, 8) and float((sums - 1).abs().max()) <= 1e-5, float((sums - 1).abs().max())
    on2 = _host(env.run("A2", key_padding=True, attention=True))
    assert {store.batch_shape(ix) for ix in env.batches["A"]} != {store.batch_shape(ix) for ix in env.batches["A2"]}
    worst = 0.0
    for i in range(N_A):
        for s, mods in STREAMS:
            for m in mods:
                x, y = _utt(on, store, s, m, i).double(), _utt(on2, store, s, m, i).double()
                worst = max(worst, float((x - y).abs().max() / x.abs().max()))
    print(f"two batchings, key_padding=True: worst max|diff| / max|weight| = {worst:.3e} (bar {BAR:g})")
    assert worst <= BAR
    off = _host(env.run("A", attention=True))
    sums, padded = _column_sums(off, store, env.batches["A"])
    assert float(sums.max()) <= 1 + 1e-5 and bool(padded.any())
    assert bool((sums[padded] < 1).any())      # (the padded frames took the rest)
    assert float((sums[~padded] - 1).abs().max()) <= 1e-5


def test_bookkeeping_unvisited_rows_neighbours_and_reuse(env):
    """4. a 29-utterance subset epoch leaves the rows of the eight others NaN and every visited row finite; in fixture B store neighbours
    are never in one batch, so after an epoch over batch 0 alone the row behind every visited utterance's last frame (the next
    utterance's first) is still NaN -- with the one-frame utterance first and last in its batch -- and after a full epoch it holds the
    next utterance's values (test 1 holds those to the oracle); out= reuse and a second identical epoch give the same bits."""
    store = env.store["A", "fp32"]
    sub = env.run("A", batches=env.batches["A"][1:], attention=True)
    att = _host(sub)
    seen = sub.seen.cpu() != 0
    assert int(seen.sum()) == N_A - 8
    for i in range(N_A):
        for s, mods in STREAMS:
            for m in mods:
                t = _utt(att, store, s, m, i)
                assert bool(torch.isfinite(t).all()) if seen[i] else bool(torch.isnan(t).all()), (s, m, i)
    with pytest.raises(env._lib.SdumcError):
        sub.attention_of(store, int(env.batches["A"][0][0]))
    got = sub.attention_of(store, store.names[int(env.batches["A"][1][0])])
    assert torch.equal(got["missing"]["feat4"].cpu(), _utt(att, store, "missing", "feat4", int(env.batches["A"][1][0])))
    sb = env.store["B", "fp32"]
    for fx in ("B", "B2"):
        one = _host(env.run(fx, batches=env.batches[fx][:1], attention=True))
        full = _host(env.run(fx, attention=True))
        for i in env.batches[fx][0].tolist():
            for s, mods in STREAMS:
                for m in mods:
                    end = int(sb.start[m][i]) + int(sb.length[m][i])
                    assert end == int(sb.start[m][i + 1])      # (i + 1 is in another batch)
                    assert bool(torch.isfinite(_utt(one, sb, s, m, i)).all()) and bool(torch.isnan(one[s][m][end]).all()), (fx, s, m, i)
                    assert bool(torch.isfinite(full[s][m][end]).all())
                    assert torch.equal(full[s][m][end], _utt(full, sb, s, m, i + 1)[0])
                    assert torch.equal(_utt(full, sb, s, m, i), _utt(one, sb, s, m, i))
    # the other order within the batches (the one-frame utterance last): held to the oracle like test 1's
    _hold_to_reference(_host(env.run("B2", attention=True)), sb, env.batches["B2"], env.reference("B2", "fp32", False), BAR, "fixture B2")
    # out= reuse (after an epoch over other rows) and a second identical epoch
    first = env.run("A", batches=env.batches["A2"][:3], attention=True, embeddings=True)
    ptrs = [t.data_ptr() for d in first.attention.values() for t in d.values()]
    again = env.run("A", attention=True, embeddings=True, out=first)
    fresh = env.run("A", attention=True, embeddings=True)
    second = env.run("A", attention=True, embeddings=True)
    torch.cuda.synchronize()
    assert again is first and [t.data_ptr() for d in first.attention.values() for t in d.values()] == ptrs
    for s, mods in STREAMS:
        for m in mods:
            assert torch.equal(first.attention[s][m], fresh.attention[s][m]) and torch.equal(second.attention[s][m], fresh.attention[s][m])
            assert bool(torch.isfinite(fresh.attention[s][m]).all())
    with pytest.raises(env._lib.SdumcError):      # a result without attention maps cannot take an epoch that keeps them, and vice versa
        env.run("A", attention=True, out=env.evaluate.EvalResult.empty(N_A, "cuda"))
    with pytest.raises(env._lib.SdumcError):
        env.run("A", out=env.run("A", attention=True))
    with pytest.raises(env._lib.SdumcError):      # ... nor one sized for another store's frames
        env.run("B", attention=True, out=env.run("A", attention=True))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_the_option_changes_nothing_else_of_the_epoch(env, mode):
    """5a. preds, seen and the four embeddings with attention=True equal, bit for bit, those with attention=False."""
    off = env.run("A", mode, embeddings=True)
    on = env.run("A", mode, embeddings=True, attention=True)
    torch.cuda.synchronize()
    assert off.attention is None and on.attention is not None
    assert torch.equal(off.preds, on.preds) and torch.equal(off.seen, on.seen) and int((on.seen != 0).sum()) == N_A
    for k in off.embeddings:
        assert torch.equal(off.embeddings[k], on.embeddings[k]), k
    assert set(on.results(env.store["A", mode])) == set(off.results(env.store["A", mode]))


def test_training_is_untouched_by_an_attention_epoch(env):
    """5b. FusedTrainer: run_epoch -> eval_epoch(attention=True) -> run_epoch leaves the parameters, the Adam moments and the dropout
    counter of the same two training epochs without evaluation."""
    E, dims = env.engine, DIMS["fp32"]
    train_store, eval_store = env.store["A", "fp32"], env.store["B", "fp32"]
    runs = []
    for with_eval in (False, True):
        flat = env.flat["fp32"].clone()
        tr = E.FusedTrainer(flat, dims, lr=1e-3, seed=11, capacity=(8, TCAP_A))
        plan = train_store.plan_epoch(env.batches["A"])
        tr.run_epoch(train_store, plan)
        if with_eval:
            res = tr.eval_epoch(eval_store, env.batches["B"], attention=True)
        tr.run_epoch(train_store, plan)
        torch.cuda.synchronize()
        runs.append((flat, tr.state.adam_m, tr.state.adam_v, tr.state.hyper, tr.state.rng.call))
        if with_eval:
            assert int((res.seen != 0).sum()) == N_B and all(bool(torch.isfinite(t).all()) for d in res.attention.values() for t in d.values())
            assert set(res.attention_of(eval_store, "b00")["full"]) == {"audio", "text", "video"}
    for x, y, what in zip(runs[0][:4], runs[1][:4], ("parameters", "adam_m", "adam_v", "hyper")):
        assert torch.equal(x, y), what
    assert runs[0][4] == runs[1][4] == 20 and not torch.equal(runs[0][0], env.flat["fp32"])


def test_abi_argument_errors_leave_the_destination_untouched(env):
    """6. every SDUMC_EINVAL case of include/sdumc_hip.h returns before anything is launched: a poisoned destination stays as it is
    (and the same descriptor, unspoilt, does write it).  Invalid ARGUMENTS only -- every pointer that is passed is a live allocation."""
    _lib, store = env._lib, env.store["A", "fp32"]
    ix = env.batches["A"][0]
    b = store.batch(ix)[0]
    nc = env.engine.NetCall(env.flat["fp32"], b["audios"], [b["texts"], b["feat4s"]], b["videos"], False, None, planes=True)
    one = env.engine.NetCall(env.flat["fp32"], b["audios"], [b["texts"]], b["videos"], False, None, planes=True)
    nc.forward()
    one.forward()
    idx = ix.cuda()
    rows = env.evaluate.attention_rows(store)
    POISON = 7.0
    dst = [[torch.full((rows[m], 8), POISON, device="cuda") for m in mods] for _, mods in STREAMS]

    def desc():
        e = _lib.AttnExport()
        e.idx, e.n_utt = idx.data_ptr(), len(store)
        for k, m in enumerate(store.MODS):
            e.start[k], e.length[k] = store.start_d[m].data_ptr(), store.length_d[m].data_ptr()
        for s in range(2):
            for j in range(3):
                e.dst[s][j], e.dst_rows[s][j] = dst[s][j].data_ptr(), dst[s][j].shape[0]
        return e

    def call(call_obj, e, dims=None, io=None):
        return _lib.lib.sdumc_net_export_attention(C.byref(dims if dims is not None else call_obj.dims), C.byref(io if io is not None else call_obj.io),
                                                  C.byref(e), _lib.current_stream())

    def copy_of(struct):
        c = type(struct)()
        C.memmove(C.byref(c), C.byref(struct), C.sizeof(struct))
        return c

    bad = []
    e = desc(); e.idx = None; bad.append(("idx", call(nc, e)))
    e = desc(); e.n_utt = 0; bad.append(("n_utt", call(nc, e)))
    e = desc(); e.start[3] = None; bad.append(("start table", call(nc, e)))
    e = desc(); e.length[0] = None; bad.append(("length table", call(nc, e)))
    e = desc(); e.dst[1][1] = None; bad.append(("destination", call(nc, e)))
    e = desc(); e.dst[0][2] = dst[0][2].data_ptr() + 8; bad.append(("alignment", call(nc, e)))
    e = desc(); e.dst_rows[1][0] = 0; bad.append(("dst_rows", call(nc, e)))
    io = copy_of(nc.io); io.workspace = None; bad.append(("workspace", call(nc, desc(), io=io)))
    d0 = copy_of(nc.dims); d0.B = 0; bad.append(("refused dims", call(nc, desc(), dims=d0)))
    bad.append(("streams == 1 with a stream-1 destination", call(one, desc())))
    lib = _lib.lib
    bad.append(("d NULL", lib.sdumc_net_export_attention(None, C.byref(nc.io), C.byref(desc()), _lib.current_stream())))
    bad.append(("io NULL", lib.sdumc_net_export_attention(C.byref(nc.dims), None, C.byref(desc()), _lib.current_stream())))
    bad.append(("e NULL", lib.sdumc_net_export_attention(C.byref(nc.dims), C.byref(nc.io), None, _lib.current_stream())))
    torch.cuda.synchronize()
    assert all(rc == -1 for _, rc in bad), bad
    assert all(bool((t == POISON).all()) for row in dst for t in row)
    # the unspoilt descriptor writes the batch's rows and nothing else; a one-stream call with stream 1's destinations NULL writes stream 0's
    assert call(nc, desc()) == 0
    e = desc()
    for j in range(3):
        e.dst[1][j] = None
    assert call(one, e) == 0
    torch.cuda.synchronize()
    visited = set(ix.tolist())
    for s, (_, mods) in enumerate(STREAMS):
        for j, m in enumerate(mods):
            t = dst[s][j].cpu()
            for i in range(N_A):
                rows_i = t[int(store.start[m][i]):int(store.start[m][i]) + int(store.length[m][i])]
                assert bool((rows_i != POISON).all()) if i in visited else bool((rows_i == POISON).all()), (s, m, i)
