"""Temporal pre-compression of the resident store on the device: sdumc_pool_frames (csrc/resample.hip) behind
DeviceFeatureStore.resampled(feat_scale, feat_type) = the reference's --feat_scale / --feat_type (func_mapping_feature,
feature_scale_compress, align_to_text, align_to_utt: read_data.py:120-200), against tests/golden/resample.npz (recorded from the
reference by tests/golden/make_resample_goldens.py) and against the host route sdumc_amd.data.map_feature / resample_instances.

Bars.  Kernel and golden (and kernel and map_feature) both round ONE float64 quotient of a float64 sum taken in frame order: they can
differ only if the sums do, so every element is held to 1 float32 ulp of the reference value and bit-equality is expected (the count
of unequal elements is printed).  A row that is all zero in the reference must be bit-zero.  The 'utt' route against the
reference's float32 pairwise mean: the recorded gap |ref32 - fp32(ref64)| plus 1 ulp.  bf16 stores: 1 bf16 ulp (2^-8 relative)
against a bf16 store of the host-resampled instances (the same two roundings: float64 -> float32 -> bf16)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODS = ("audio", "text", "video", "feat4")


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import _lib
    from sdumc_amd.data import DeviceFeatureStore
    return _lib, DeviceFeatureStore


def split(a, lens):
    out, o = [], 0
    for n in lens:
        out.append(a[o:o + int(n)])
        o += int(n)
    assert o == a.shape[0]
    return out


def ceil_div(lens, k):
    return [-(-int(n) // k) for n in lens]


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def golden_instances(g):
    lens = g["lens"]
    cols = {m: split(g[f"in_{m}"], lens[:, k]) for k, m in enumerate(MODS)}
    return [{m: cols[m][i] for m in MODS} | {"emo": 0, "val": 0.25 * i - 1.0, "name": f"u{i}"} for i in range(lens.shape[0])]


def utterances(store, m):
    """the utterances of one modality of a store as host float32 arrays, and its trailing row"""
    packed = store.packed[m].float().cpu().numpy()
    start, length = store.start[m].numpy(), store.length[m].numpy()
    assert packed.shape[0] == int(length.sum()) + 1 and np.array_equal(start, np.concatenate([[0], np.cumsum(length)[:-1]]))
    return [packed[s:s + n] for s, n in zip(start, length)], packed[-1]


def hold(got, want, bar, what, tally):
    """got within `bar` of want element by element; rows that are all zero in want are bit-zero in got"""
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    tally[0] += int((got.view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).sum())
    tally[1] += got.size
    assert (err <= bar).all(), (what, float((err / np.maximum(bar, 1e-300)).max()))
    zero = ~want.any(axis=1)
    assert not got[zero].view(np.uint32).any(), (what, "a zero row of the reference is not bit-zero")


def random_instances(lens4, d, seed, bf16=False):
    """lens4: [N, 4] frame counts -> instances with N(0, 1) features of width d (rounded to bf16-representable values on request)"""
    rs = np.random.RandomState(seed)
    out = []
    for i, row in enumerate(lens4):
        inst = {"emo": 0, "val": float(rs.uniform(-3, 3)), "name": f"s{i}"}
        for m, L in zip(MODS, row):
            x = rs.standard_normal((int(L), d)).astype(np.float32)
            inst[m] = torch.from_numpy(x).to(torch.bfloat16).float().numpy() if bf16 else x
        out.append(inst)
    return out


def permuted_lengths(seed):
    """five utterances, lengths {1, 2, 7, 33, 75} permuted per modality; utterance 0 has audio (2) shorter than text (7)"""
    rs = np.random.RandomState(seed)
    lens = np.stack([rs.permutation([1, 2, 7, 33, 75]) for _ in MODS], axis=1)
    for k, want in enumerate((2, 7, 33, 1)):
        j = int(np.nonzero(lens[:, k] == want)[0][0])
        lens[[0, j], k] = lens[[j, 0], k]
    return lens


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the reference's own outputs
# ---------------------------------------------------------------------------------------------------------------------------------
def test_kernel_against_the_reference_golden_every_mode(cuda, golden):
    _, Store = cuda
    g = golden("resample")
    lens = g["lens"]
    store = Store(golden_instances(g))
    tally = [0, 0]
    for k in (2, 3, 4):
        res = store.resampled(feat_scale=k)
        for c, m in enumerate(MODS):
            got, last = utterances(res, m)
            assert not last.view(np.uint32).any()
            for i, (a, w) in enumerate(zip(got, split(g[f"scale{k}_{m}"], ceil_div(lens[:, c], k)))):
                hold(a, w, ulp32(w), (f"scale{k}", m, i), tally)
    res = store.resampled(feat_type="frm_align")
    for m in MODS:
        want = split(g[f"align_{m}"], lens[:, 1]) if m != "feat4" else split(g["in_feat4"], lens[:, 3])
        for i, (a, w) in enumerate(zip(utterances(res, m)[0], want)):
            hold(a, w, ulp32(w), ("frm_align", m, i), tally)
    print(f"fp64 routes against the golden: {tally[0]} of {tally[1]} elements unequal (0 expected)")
    res = store.resampled(feat_type="utt")
    t64, worst = [0, 0], 0.0
    for m in MODS:
        got = np.stack(utterances(res, m)[0])
        assert got.shape == (9, 1, 8)
        hold(got[:, 0], g[f"utt64_{m}"].astype(np.float32), ulp32(g[f"utt64_{m}"]), ("utt, fp64 rule", m), t64)
        err = np.abs(got[:, 0].astype(np.float64) - g[f"utt_{m}"].astype(np.float64))
        bar = g[f"uttgap_{m}"] + ulp32(g[f"utt_{m}"])
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), ("utt against align_to_utt", m, float((err / bar).max()))
    print(f"utt route: {t64[0]} of {t64[1]} unequal to fp32(fp64 mean); worst error / bar against align_to_utt {worst:.3f}")


def test_both_options_scale_first_then_align(cuda, golden):
    """feat_scale is applied first, so frm_align aligns to the compressed text length: equal to the two calls one after the other and
    to the host route, bit for bit; against the reference's chain (which keeps float64 between the passes, where a store holds
    float32) within 2^-24 of the pooled magnitude of the intermediate plus 1 ulp -- the bar derived in tests/test_resample_cpu.py."""
    from sdumc_amd.data import map_feature, resample_instances
    _, Store = cuda
    g = golden("resample")
    inst = golden_instances(g)
    store = Store(inst)
    res = store.resampled(feat_scale=2, feat_type="frm_align")
    two = store.resampled(feat_scale=2).resampled(feat_type="frm_align")
    host = resample_instances(inst, feat_scale=2, feat_type="frm_align")
    mid = resample_instances(inst, feat_scale=2)
    tl = ceil_div(g["lens"][:, 1], 2)
    tally, ref = [0, 0], [0, 0]
    for m in MODS:
        assert torch.equal(res.packed[m], two.packed[m]) and torch.equal(res.length[m], two.length[m])
        got = utterances(res, m)[0]
        for i, a in enumerate(got):
            hold(a, host[i][m], ulp32(host[i][m]), ("host route", m, i), tally)
        if m != "feat4":
            assert res.length[m].tolist() == tl
            for i, (a, w) in enumerate(zip(got, split(g[f"scale2_align_{m}"], tl))):
                bar = 2.0 ** -24 * map_feature(np.abs(mid[i][m]), tl[i]).astype(np.float64) * (1 + 2.0 ** -23) + ulp32(w)
                hold(a, w, bar, ("reference chain", m, i), ref)
    print(f"scale 2 + frm_align: {tally[0]} of {tally[1]} unequal to the host route, {ref[0]} of {ref[1]} to the reference's chain")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. shapes where the indexing can go wrong, against map_feature
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 260, 1024])
def test_widths_and_permuted_lengths_against_the_host_route(cuda, d):
    """d = 4: one chunk per row; 260: 65 chunks, one more than a wave stride; 1024: the workload's width.  Lengths {1, 2, 7, 33, 75}
    permuted per modality: the first and the last utterance of the binary search own rows of every pool size."""
    from sdumc_amd.data import resample_instances
    _, Store = cuda
    inst = random_instances(permuted_lengths(d), d, seed=100 + d)
    store = Store(inst)
    tally = [0, 0]
    for kw in (dict(feat_scale=2), dict(feat_scale=3), dict(feat_type="frm_align"), dict(feat_type="utt"),
               dict(feat_scale=3, feat_type="frm_align")):
        res, host = store.resampled(**kw), resample_instances(inst, **kw)
        for m in MODS:
            got, last = utterances(res, m)
            assert not last.view(np.uint32).any() and res.dim[m] == d
            assert res.length[m].tolist() == [h[m].shape[0] for h in host]
            for i, a in enumerate(got):
                hold(a, host[i][m], ulp32(host[i][m]), (kw, m, i), tally)
    print(f"d = {d}: {tally[0]} of {tally[1]} elements unequal to map_feature (0 expected)")


@pytest.mark.parametrize("kw", [dict(feat_scale=2), dict(feat_scale=3), dict(feat_type="frm_align"), dict(feat_type="utt")])
def test_one_utterance_store(cuda, kw):
    from sdumc_amd.data import resample_instances
    _, Store = cuda
    inst = random_instances([[5, 9, 75, 1]], 12, seed=7)      # audio shorter than text: the L < n branch
    res, host = Store(inst).resampled(**kw), resample_instances(inst, **kw)
    tally = [0, 0]
    for m in MODS:
        got, last = utterances(res, m)
        assert len(got) == 1 and not last.view(np.uint32).any()
        hold(got[0], host[0][m], ulp32(host[0][m]), (kw, m), tally)
    assert tally[0] == 0, tally


@pytest.mark.parametrize("d", [8, 264])
def test_bf16_store(cuda, d):
    """bf16 rows in, float64 sums, the quotient rounded to float32 and then to bf16: what DeviceFeatureStore(bf16=True) makes of the
    host-resampled instances, to 1 bf16 ulp (2^16 float32 ulps of the bf16 value)."""
    from sdumc_amd.data import resample_instances
    _, Store = cuda
    inst = random_instances(permuted_lengths(d), d, seed=200 + d, bf16=True)
    store = Store(inst, bf16=True)
    unequal = total = 0
    for kw in (dict(feat_scale=2), dict(feat_scale=3), dict(feat_type="frm_align"), dict(feat_type="utt")):
        res = store.resampled(**kw)
        want = Store(resample_instances(inst, **kw), bf16=True)
        for m in MODS:
            assert res.packed[m].dtype == torch.bfloat16 and res.packed[m].shape == want.packed[m].shape
            assert torch.equal(res.length[m], want.length[m]) and torch.equal(res.start[m], want.start[m])
            a, w = res.packed[m].float().cpu().numpy(), want.packed[m].float().cpu().numpy()
            err = np.abs(a.astype(np.float64) - w.astype(np.float64))
            assert (err <= ulp32(w) * 65536).all(), (kw, m, float(err.max()))
            assert not a[~w.any(axis=1)].view(np.uint32).any()
            unequal, total = unequal + int((a != w).sum()), total + a.size
    print(f"bf16, d = {d}: {unequal} of {total} elements unequal (0 expected)")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. structure of the result
# ---------------------------------------------------------------------------------------------------------------------------------
def test_structure_tables_planes_and_untouched_source(cuda):
    _lib, Store = cuda
    lens = permuted_lengths(3)
    inst = random_instances(lens, 64, seed=3)
    src = Store(inst, planes=True)
    before = {m: (src.packed[m].clone(), src.packed_p3[m].clone(), src.start[m].clone(), src.length[m].clone()) for m in MODS}
    assert src.resampled() is src and src.resampled(feat_scale=1, feat_type="frm_unalign") is src and src.resampled(1.0) is src
    res = src.resampled(feat_scale=2)
    torch.cuda.synchronize()
    assert res is not src and res.names == src.names and res.names is not src.names and res.device == src.device
    assert torch.equal(res.vals, src.vals) and torch.equal(res.emos, src.emos) and len(res) == len(src)
    assert res.get_featdim() == src.get_featdim()
    for k, m in enumerate(MODS):
        want = torch.tensor(ceil_div(lens[:, k], 2), dtype=torch.int32)
        assert res.length[m].dtype == torch.int32 and torch.equal(res.length[m], want)
        assert res.start[m].dtype == torch.int64 and torch.equal(res.start[m], torch.cumsum(want.long(), 0) - want.long())
        assert torch.equal(res.length_d[m].cpu(), res.length[m]) and torch.equal(res.start_d[m].cpu(), res.start[m])
        assert res.length_d[m].device == src.packed[m].device and res.packed[m].dtype == torch.float32
        assert res.packed[m].shape == (int(want.sum()) + 1, 64) and not bool(res.packed[m][-1].any())      # the trailing zero row
        assert res.packed[m].data_ptr() != src.packed[m].data_ptr()
        # the planes of the result are sdumc_p3_split of its rows, bit for bit
        p3 = torch.empty(res.packed[m].shape[0], 6 * 64, dtype=torch.uint8, device="cuda")
        _lib.check(_lib.lib.sdumc_p3_split(_lib.ptr(res.packed[m]), 64, _lib.ptr(p3), 6 * 64, res.packed[m].shape[0], 64,
                                           _lib.current_stream()), "sdumc_p3_split")
        assert res.packed_p3 is not None and torch.equal(res.packed_p3[m], p3)
        for a, b in zip(before[m], (src.packed[m], src.packed_p3[m], src.start[m], src.length[m])):      # the source: untouched
            assert torch.equal(a, b)
    assert res.batch_shape([0, 1, 2, 3, 4]) == (5, tuple(int(-(-lens[:, k].max() // 2)) for k in range(4)))
    assert src.resampled(feat_scale=2, planes=False).packed_p3 is None
    bare = Store(inst)
    assert bare.resampled(feat_type="utt").packed_p3 is None and bare.resampled(feat_type="utt", planes=True).packed_p3 is not None
    # a batch of the result = collate() of the host-resampled instances
    from sdumc_amd.data import collate, resample_instances
    got = res.batch([4, 0, 2])
    host = resample_instances(inst, feat_scale=2)
    want = collate([host[4], host[0], host[2]])
    for key in ("audios", "texts", "videos", "feat4s"):
        assert torch.equal(got[0][key].cpu(), want[0][key]), key
    assert got[1] == want[1] and got[4] == want[4]


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. end to end: evaluation and training on the compressed store
# ---------------------------------------------------------------------------------------------------------------------------------
def test_eval_and_train_epochs_on_the_resampled_store(cuda):
    """12 utterances, widths 64 (planes allowed, so the epochs read the store in place through row maps), T up to 40 / 8 / 30 / 8,
    feat_scale = 2: store.resampled(...) against a store built from resample_instances(...).  The packed tensors must compare equal;
    the predictions of eval_epoch and the losses of two run_epoch steps are then the same computation on the same bits and must be
    equal bit for bit.  (Were the packed tensors to differ in a last bit, the suite's 2e-5 output bar would apply instead.)"""
    from oracle import sdumc_oracle as O
    from sdumc_amd import engine
    from sdumc_amd.data import resample_instances
    _, Store = cuda
    dims, tcap = (64, 64, 64, 64), (40, 8, 30, 8)
    rs = np.random.RandomState(12)
    lens = np.stack([rs.randint(max(1, t // 4), t + 1, size=12) for t in tcap], axis=1)
    lens[0], lens[11] = tcap, (11, 1, 9, 3)
    inst = random_instances(lens, 64, seed=13)
    dev = Store(inst, planes=True).resampled(feat_scale=2)
    host = Store(resample_instances(inst, feat_scale=2), planes=True)
    same = all(torch.equal(dev.packed[m], host.packed[m]) and torch.equal(dev.packed_p3[m], host.packed_p3[m]) for m in MODS)
    assert same, "the device-resampled store differs from the host-resampled one: the bit-for-bit checks below rest on their equality"
    P = O.init_params(dims, seed=8)
    lay = engine.ParamLayout.get(*dims[:3])
    flat0 = torch.zeros(lay.total)
    for k, v in lay.views(flat0).items():
        v.copy_(P[k])
    batches = [torch.tensor([3, 0, 7, 10, 5, 1]), torch.tensor([11, 2, 9, 4, 8, 6])]
    cap = (6, tuple(-(-t // 2) for t in tcap))
    runs = []
    for store in (dev, host):
        tr = engine.FusedTrainer(flat0.clone().cuda(), dims, lr=1e-3, seed=11, capacity=cap)
        ev0 = tr.eval_epoch(store, batches).preds.clone()
        losses = []
        assert tr.run_epoch(store, batches, on_step=lambda i, l: losses.append(l.clone())) == 2
        ev1 = tr.eval_epoch(store, batches).preds.clone()
        torch.cuda.synchronize()
        assert tr._in_place(store)
        runs.append([ev0.cpu(), ev1.cpu()] + [l.cpu() for l in losses])
    for name, a, b in zip(("preds before", "preds after two steps", "losses of step 0", "losses of step 1"), *runs):
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), name
        if same:
            assert torch.equal(a, b), (name, float((a - b).abs().max()))
        else:
            scale = max(1.0, float(b.abs().max()))
            np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=2e-5, atol=2e-5 * scale, err_msg=name)
    assert not torch.equal(runs[0][0], runs[0][1])      # the two steps moved the parameters


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(feat_scale=0), dict(feat_scale=-1), dict(feat_scale=2.5), dict(feat_scale="2"),
                                dict(feat_type="frame"), dict(feat_type=None), dict(feat_scale=2, planes=True)])
def test_bad_arguments_raise_before_anything_is_enqueued(cuda, kw):
    _lib, Store = cuda
    store = Store(random_instances([[3, 2, 4, 1], [6, 1, 2, 2]], 8, seed=1))      # widths of 8: planes are not allowed
    with pytest.raises(_lib.SdumcError):
        store.resampled(**kw)


def test_c_entry_refuses_without_launching(cuda):
    _lib, _ = cuda
    EINVAL = -1
    src = torch.randn(8, 8, device="cuda")
    dst = torch.full((5, 8), 7.0, device="cuda")
    s0, sl = torch.tensor([0, 3], device="cuda"), torch.tensor([3, 4], dtype=torch.int32, device="cuda")
    d0, dl = torch.tensor([0, 2], device="cuda"), torch.tensor([2, 2], dtype=torch.int32, device="cuda")

    def desc(**over):
        p = _lib.PoolFrames()
        p.src, p.dst, p.src_start, p.src_len, p.dst_start, p.dst_len = (t.data_ptr() for t in (src, dst, s0, sl, d0, dl))
        p.src_rows, p.dst_rows, p.n_utts, p.cols, p.bf16 = 7, 4, 2, 8, 0
        for k, v in over.items():
            setattr(p, k, v)
        return p

    call = lambda p, wg=0: _lib.lib.sdumc_pool_frames(C.byref(p) if p is not None else None, wg, _lib.current_stream())
    assert call(None) == EINVAL
    for k in ("src", "dst", "src_start", "src_len", "dst_start", "dst_len"):
        assert call(desc(**{k: None})) == EINVAL, k
    assert call(desc(src=src.data_ptr() + 4)) == EINVAL and call(desc(dst=dst.data_ptr() + 8)) == EINVAL      # not 16-byte aligned
    for cols in (0, -4, 6, 2):
        assert call(desc(cols=cols)) == EINVAL, cols
    assert call(desc(cols=4, bf16=1)) == EINVAL and call(desc(bf16=2)) == EINVAL      # bf16 rows: whole 8-element chunks
    for k in ("n_utts", "src_rows", "dst_rows"):
        assert call(desc(**{k: 0})) == EINVAL and call(desc(**{k: -1})) == EINVAL, k
    assert call(desc(), -1) == EINVAL
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())      # nothing was launched
    assert call(desc()) == 0 and call(desc(), 1) == 0      # the same descriptor, unmodified, is accepted (also on ONE workgroup)
    torch.cuda.synchronize()
    x = src.double()
    want = torch.stack([x[0] / 2, (x[1] + x[2]) / 2, (x[3] + x[4]) / 2, (x[5] + x[6]) / 2, torch.zeros_like(x[0])]).float()
    assert torch.equal(dst, want)
