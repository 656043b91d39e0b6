#!/usr/bin/env python
"""Generate tests/golden/resample.npz from the REAL reference's temporal pre-compression (toolkit/utils/read_data.py:120-200).

    python tests/golden/make_resample_goldens.py <path of the reference checkout>

Imports toolkit/utils/read_data.py of the reference by path (never copies it) and runs func_mapping_feature,
feature_scale_compress, align_to_text and align_to_utt on seeded float32 inputs.  The module's imports that the functions do not
use (prefetch_generator, cv2, torchaudio, lmdb, toolkit.utils.chatgpt) are stubbed in sys.modules where they are not installed.
Data only (np.savez_compressed, loadable with allow_pickle=False); every reference output is recorded cast to float32, which is
what the reference's torch.FloatTensor(...) makes of it.

Per-utterance arrays are recorded CONCATENATED along the frame axis, utterance 0 first (their lengths follow from `lens`).

  map_ls           int32 [9]: the distinct source lengths; map_in float32 [sum map_ls, 8]: one input per length, in that order
  pairs            int32 [P, 2]: (L, n) of func_mapping_feature(input of length L, n): L < n, L == n, r == 0, r != 0, n == 1 and
                   pad >= pool (leading all-zero rows); map_out float32 [sum n, 8]: the outputs in pair order
  lens             int32 [N, 4]: frames of utterance i in audio, text, video, feat4 (N = 9; a permutation of map_ls per modality)
  in_<m>           float32 [sum L, 8], m in audio / text / video / feat4
  scale<k>_<m>     feature_scale_compress with k in 2, 3, 4: ceil(L / k) frames each (feat4 by the same call on a list of its own)
  align_<m>        align_to_text, m in audio / text / video: the text length each
  scale2_align_<m> feature_scale_compress(2) and align_to_text after it (the order of feat_data.py:117-126): ceil(L_text / 2) each
  utt_<m>          float32 [N, 8]: align_to_utt (np.mean of the float32 array); utt64_<m> float64 [N, 8]: the mean in float64, frame
                   order; uttgap_<m> float64 [N, 8]: |utt - fp32(utt64)|, the reference's own float32 rounding on this route
"""
import importlib
import math
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
MODS = ("audio", "text", "video", "feat4")
LS = (1, 2, 3, 5, 7, 10, 16, 33, 75)
D = 8
# (7, 5), (10, 7), (5, 4): pad >= pool, so the leading output rows are all zero
PAIRS = [(3, 5), (1, 4), (7, 7), (1, 1), (10, 5), (16, 4), (75, 25), (7, 5), (10, 3), (33, 5), (75, 38), (16, 9), (10, 7), (5, 4),
         (33, 17), (2, 1), (7, 1), (33, 1), (75, 1)]


def load_reference_read_data(ref):
    for name in ("prefetch_generator", "cv2", "torchaudio", "lmdb"):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["prefetch_generator"], "BackgroundGenerator"):
        sys.modules["prefetch_generator"].BackgroundGenerator = object
    chat = types.ModuleType("toolkit.utils.chatgpt")
    chat.get_translate_eng2chi = chat.get_translate_chi2eng = None
    sys.modules["toolkit.utils.chatgpt"] = chat
    sys.path.insert(0, ref)
    return importlib.import_module("toolkit.utils.read_data")


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    R = load_reference_read_data(os.path.abspath(sys.argv[1]))
    rs = np.random.RandomState(20241019)
    d = {"pairs": np.array(PAIRS, dtype=np.int32), "map_ls": np.array(LS, dtype=np.int32)}
    map_in = {L: rs.standard_normal((L, D)).astype(np.float32) for L in LS}
    d["map_in"] = np.concatenate([map_in[L] for L in LS])
    outs = [f32(R.func_mapping_feature(map_in[L].copy(), n)) for L, n in PAIRS]
    assert all(o.shape == (n, D) for o, (_, n) in zip(outs, PAIRS))
    d["map_out"] = np.concatenate(outs)
    N = len(LS)
    lens = np.stack([rs.permutation(LS) for _ in MODS], axis=1).astype(np.int32)
    for k, want in enumerate((3, 7, 5, 2)):      # utterance 0: audio shorter than text, the L < n branch of align_to_text
        j = int(np.nonzero(lens[:, k] == want)[0][0])
        lens[[0, j], k] = lens[[j, 0], k]
    d["lens"] = lens
    feats = {m: [rs.standard_normal((int(lens[i, k]), D)).astype(np.float32) for i in range(N)] for k, m in enumerate(MODS)}
    for m in MODS:
        d[f"in_{m}"] = np.concatenate(feats[m])
    fresh = lambda m: [x.copy() for x in feats[m]]

    def put(prefix, names, lists, want_lens):
        for m, xs in zip(names, lists):
            xs = [f32(x) for x in xs]
            assert [x.shape[0] if x.ndim == 2 else -1 for x in xs] == list(want_lens(m)), (prefix, m)
            d[f"{prefix}_{m}"] = np.concatenate(xs) if xs[0].ndim == 2 else np.stack(xs)

    col = lambda m: lens[:, MODS.index(m)].tolist()
    for k in (2, 3, 4):
        ceil_k = lambda m: [math.ceil(L / k) for L in col(m)]
        put(f"scale{k}", MODS[:3], R.feature_scale_compress(fresh("audio"), fresh("text"), fresh("video"), k), ceil_k)
        put(f"scale{k}", MODS[3:], R.feature_scale_compress(fresh("feat4"), fresh("feat4"), fresh("feat4"), k)[:1], ceil_k)
    put("align", MODS[:3], R.align_to_text(fresh("audio"), fresh("text"), fresh("video")), lambda m: col("text"))
    put("scale2_align", MODS[:3], R.align_to_text(*R.feature_scale_compress(fresh("audio"), fresh("text"), fresh("video"), 2)),
        lambda m: [math.ceil(L / 2) for L in col("text")])
    put("utt", MODS[:3], R.align_to_utt(fresh("audio"), fresh("text"), fresh("video")), lambda m: [-1] * N)      # 1-D rows
    put("utt", MODS[3:], R.align_to_utt(fresh("feat4"), fresh("feat4"), fresh("feat4"))[:1], lambda m: [-1] * N)
    worst = 0.0
    for m in MODS:
        assert d[f"utt_{m}"].dtype == np.float32 and d[f"utt_{m}"].shape == (N, D)
        u64 = np.zeros((N, D), dtype=np.float64)
        for i in range(N):
            for row in feats[m][i]:
                u64[i] += row.astype(np.float64)
            u64[i] /= len(feats[m][i])
        d[f"utt64_{m}"] = u64
        d[f"uttgap_{m}"] = np.abs(d[f"utt_{m}"].astype(np.float64) - u64.astype(np.float32).astype(np.float64))
        worst = max(worst, float(d[f"uttgap_{m}"].max()))
    print(f"{len(PAIRS)} (L, n) pairs, {N} utterances x {len(MODS)} modalities; largest align_to_utt gap {worst:.3e}")
    path = os.path.join(OUT, "resample.npz")
    np.savez_compressed(path, **d)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
