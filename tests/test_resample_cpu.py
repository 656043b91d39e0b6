"""CPU: the host route of the temporal pre-compression (sdumc_amd.data.map_feature, resample_instances = the reference's
--feat_scale / --feat_type: func_mapping_feature, feature_scale_compress, align_to_text, align_to_utt of read_data.py:120-200)
against tests/golden/resample.npz, which tests/golden/make_resample_goldens.py recorded from the reference itself.

Bars: the float64 routes (everything but align_to_utt) are BIT-EQUAL to the golden -- both sides sum in float64 in frame order,
divide once and round once.  The 'utt' route is held to the recorded gap |ref32 - fp32(ref64)| of each element plus one float32
ulp of the value: the reference's align_to_utt sums pairwise in float32, ours keeps the float64 rule, and fp32(ref64) is what ours
must give exactly (asserted too)."""
import numpy as np
import pytest

MODS = ("audio", "text", "video", "feat4")


def split(a, lens):
    out, o = [], 0
    for n in lens:
        out.append(a[o:o + int(n)])
        o += int(n)
    assert o == a.shape[0]
    return out


def golden_instances(g):
    lens = g["lens"]
    cols = {m: split(g[f"in_{m}"], lens[:, k]) for k, m in enumerate(MODS)}
    return [{m: cols[m][i] for m in MODS} | {"emo": 0, "val": 0.25 * i - 1.0, "name": f"u{i}"} for i in range(lens.shape[0])]


def ceil_div(lens, k):
    return [-(-int(n) // k) for n in lens]


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def g(golden):
    return golden("resample")


def test_map_feature_bit_equal_on_the_pair_table(g):
    from sdumc_amd.data import map_feature
    ins = dict(zip(g["map_ls"].tolist(), split(g["map_in"], g["map_ls"])))
    outs = split(g["map_out"], g["pairs"][:, 1])
    kinds = set()
    for (L, n), want in zip(g["pairs"].tolist(), outs):
        got = map_feature(ins[L], n)
        assert got.dtype == np.float32 and got.shape == (n, 8) and got.flags.c_contiguous
        assert bits_equal(got, want), (L, n, np.abs(got - want).max())
        q, r = divmod(L, n)
        kinds.add("short" if L < n else "same" if L == n else "utt" if n == 1 else "even" if r == 0 else "ragged")
        if L > n and r and n - r >= q + 1:
            kinds.add("zero rows")
            assert not got[:(n - r) // (q + 1)].any()
    assert kinds == {"short", "same", "utt", "even", "ragged", "zero rows"}      # the table covers every branch


def test_map_feature_quirks_by_hand():
    """L = 7, n = 5: pool 2, three zero frames in FRONT -- row 0 is zero, row 1 is x[0] / 2 (the divisor is the pool, not the count
    of real frames); L < n: zero rows behind; the input is not modified and the result never aliases it."""
    from sdumc_amd.data import map_feature
    x = np.arange(1, 29, dtype=np.float32).reshape(7, 4)
    keep = x.copy()
    y = map_feature(x, 5)
    assert not y[0].any() and np.array_equal(y[1], x[0] / 2) and np.array_equal(y[2], (x[1] + x[2]) / 2)
    assert np.array_equal(y[4], (x[5] + x[6]) / 2)
    z = map_feature(x, 9)
    assert z.shape == (9, 4) and np.array_equal(z[:7], x) and not z[7:].any()
    same = map_feature(x, 7)
    assert np.array_equal(same, x) and not np.shares_memory(same, x) and np.array_equal(x, keep)
    assert np.array_equal(map_feature(x.astype(np.float64), 1)[0], x.astype(np.float64).sum(0) / 7)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_feat_scale_bit_equal(g, k):
    from sdumc_amd.data import resample_instances
    inst = golden_instances(g)
    out = resample_instances(inst, feat_scale=k)
    for c, m in enumerate(MODS):
        want = split(g[f"scale{k}_{m}"], ceil_div(g["lens"][:, c], k))
        for i, w in enumerate(want):
            assert bits_equal(out[i][m], w), (k, m, i)
    assert [o["name"] for o in out] == [i["name"] for i in inst] and [o["val"] for o in out] == [i["val"] for i in inst]
    for j, i in enumerate(inst):      # the source instances are left as they were
        assert [i[m].shape[0] for m in MODS] == g["lens"][j].tolist()


def test_frm_align_bit_equal_and_feat4_keeps_its_length(g):
    from sdumc_amd.data import resample_instances
    out = resample_instances(golden_instances(g), feat_type="frm_align")
    tl = g["lens"][:, 1]
    for m in MODS[:3]:
        for i, w in enumerate(split(g[f"align_{m}"], tl)):
            assert bits_equal(out[i][m], w), (m, i)
    for i, w in enumerate(split(g["in_feat4"], g["lens"][:, 3])):
        assert bits_equal(out[i]["feat4"], w)
    assert g["lens"][0, 0] < g["lens"][0, 1]      # the fixture holds audio shorter than text: the L < n branch was taken


def test_feat_scale_is_applied_before_feat_type(g):
    """feat_data.py:117-126: frm_align aligns to the COMPRESSED text length.  Both options = the two passes one after the other, bit for
    bit.  Against the reference's chain the bar is derived, not bit-equality: the reference hands the float64 result of
    feature_scale_compress to align_to_text unrounded, while an instance (and a store) holds float32 between the passes.  That rounding
    moves an intermediate element y by <= 2^-24 |y|, the second pass averages `pool` of them (mean |y| over the pool, which
    map_feature(|y|, n) gives), and both sides then round once: |got - ref| <= 2^-24 mean|y| (1 + 2^-23) + ulp32(ref)."""
    from sdumc_amd.data import map_feature, resample_instances
    inst = golden_instances(g)
    out = resample_instances(inst, feat_scale=2, feat_type="frm_align")
    mid = resample_instances(inst, feat_scale=2)
    tl = ceil_div(g["lens"][:, 1], 2)
    worst, unequal = 0.0, 0
    for m in MODS[:3]:
        for i, w in enumerate(split(g[f"scale2_align_{m}"], tl)):
            assert out[i][m].shape == w.shape and out[i][m].dtype == np.float32
            err = np.abs(out[i][m].astype(np.float64) - w.astype(np.float64))
            bar = 2.0 ** -24 * map_feature(np.abs(mid[i][m]), tl[i]).astype(np.float64) * (1 + 2.0 ** -23) + ulp32(w)
            worst, unequal = max(worst, float((err / bar).max())), unequal + int((err != 0).sum())
            assert (err <= bar).all(), (m, i, float((err / bar).max()))
    print(f"feat_scale=2 + frm_align against the reference's unrounded chain: {unequal} unequal elements, worst error / bar {worst:.3f}")
    for i, w in enumerate(split(g["scale2_feat4"], ceil_div(g["lens"][:, 3], 2))):
        assert bits_equal(out[i]["feat4"], w)
    two = resample_instances(mid, feat_type="frm_align")
    assert all(bits_equal(a[m], b[m]) for a, b in zip(out, two) for m in MODS)
    swapped = resample_instances(resample_instances(inst, feat_type="frm_align"), feat_scale=2)      # the other order: the same lengths, other values
    assert [o["audio"].shape[0] for o in out] == tl and [o["audio"].shape[0] for o in swapped] == ceil_div(g["lens"][:, 1], 2)
    assert any(not bits_equal(a["audio"], b["audio"]) for a, b in zip(out, swapped))


def test_utt_route_holds_the_fp64_rule_within_the_reference_gap(g):
    from sdumc_amd.data import resample_instances
    out = resample_instances(golden_instances(g), feat_type="utt")
    worst = 0.0
    for m in MODS:
        got = np.stack([o[m] for o in out])
        assert got.dtype == np.float32 and got.shape == (9, 1, 8)
        got = got[:, 0]
        assert bits_equal(got, g[f"utt64_{m}"].astype(np.float32)), m
        err = np.abs(got.astype(np.float64) - g[f"utt_{m}"].astype(np.float64))
        bar = g[f"uttgap_{m}"] + ulp32(g[f"utt_{m}"])
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), (m, float((err - bar).max()))
    print(f"utt route: worst error / bar = {worst:.3f}")


def test_identity_shapes_and_collate(g):
    import torch
    from sdumc_amd.data import collate, resample_instances
    inst = golden_instances(g)
    same = resample_instances(inst)
    assert all(bits_equal(a[m], b[m]) for a, b in zip(same, inst) for m in MODS)
    assert bits_equal(resample_instances([{**inst[0], "audio": inst[0]["audio"][0]}])[0]["audio"], inst[0]["audio"][:1])      # 1-D -> [1, d]
    out = resample_instances([{**i, "text": torch.from_numpy(i["text"])} for i in inst], feat_scale=3)
    batch, pads, emos, vals, names = collate(out)
    for c, (key, m) in enumerate(zip(("audios", "texts", "videos", "feat4s"), MODS)):
        lens = ceil_div(g["lens"][:, c], 3)
        assert batch[key].shape == (9, max(lens), 8) and batch[key].dtype == torch.float32
        assert pads[c] == [max(lens) - n for n in lens]
    assert names == [f"u{i}" for i in range(9)]


@pytest.mark.parametrize("kw", [dict(feat_scale=0), dict(feat_scale=-2), dict(feat_scale=1.5), dict(feat_scale="2"),
                                dict(feat_scale=True), dict(feat_scale=float("nan")), dict(feat_type="frame"),
                                dict(feat_type=None), dict(feat_scale=2, feat_type="utterance")])
def test_bad_arguments_raise(g, kw):
    from sdumc_amd._lib import SdumcError
    from sdumc_amd.data import resample_instances
    with pytest.raises(SdumcError):
        resample_instances(golden_instances(g), **kw)


def test_map_feature_refuses_bad_input():
    from sdumc_amd._lib import SdumcError
    from sdumc_amd.data import map_feature
    for x, n in ((np.zeros((3, 4), np.float32), 0), (np.zeros((3, 4), np.float32), -1), (np.zeros(4, np.float32), 2)):
        with pytest.raises(SdumcError):
            map_feature(x, n)


def test_golden_is_data_only_and_small():
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample.npz")
    assert os.path.getsize(path) < 100 << 10
    with np.load(path, allow_pickle=False) as z:
        assert all(z[k].dtype.kind in "fi" for k in z.files)


def test_pool_descriptor_mirrors_the_header_and_null_is_refused():
    """the ctypes mirror of sdumc_pool_desc against the C compiler's view of include/sdumc_hip.h (size and every field offset); a NULL
    descriptor comes back as SDUMC_EINVAL from the host-side checks (no device needed)."""
    import ctypes as C
    import os
    import subprocess
    import tempfile
    from sdumc_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f[0] for f in _lib.PoolFrames._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sdumc_hip.h"\nint main(){printf("%zu", sizeof(sdumc_pool_desc));\n' + \
          "".join(f'printf(" %zu", offsetof(sdumc_pool_desc, {f}));\n' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), os.path.join(td, "t.c"), "-o", os.path.join(td, "t")])
        want = [int(v) for v in subprocess.check_output([os.path.join(td, "t")]).split()]
    assert [C.sizeof(_lib.PoolFrames)] + [getattr(_lib.PoolFrames, f).offset for f in fields] == want
    assert _lib.lib.sdumc_pool_frames(None, 0, None) == -1
