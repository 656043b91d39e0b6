"""The feature-tensor (dataloader) contract of the hot path:

  data = (batch_dict, pads, emos, vals, names)       toolkit/data/feat_data.py:232-253
  batch_dict['audios'|'texts'|'videos'|'feat4s']     float32 [B, maxT_m, d_m], RIGHT-zero-padded per
                                                     modality to the batch max (read_data.py:139-151,223-248)
  pads   4 lists of per-sample pad lengths (unused downstream), emos/vals float [B], names list[str]
  on disk: <feat_root>/<feature_name>/<utt>.npy of shape [T, d] (squeezed; 1-D promoted to [1, d])
           (read_data.py:22-49)

Padded frames are NOT masked anywhere on the reference's path: they take part in the softmax over time.
This module reproduces the contract (not the reference's 12-process loader)."""
import os

import numpy as np
import torch

KEYS = ('audios', 'texts', 'videos', 'feat4s')


def read_feature(feature_root, name):
    """[T, d] float32 from <root>/<name>.npy or a directory of per-frame .npy files (read_data.py:22-49)."""
    path = os.path.join(feature_root, name + '.npy')
    if os.path.exists(path):
        feat = np.load(path).squeeze()
    elif os.path.isdir(os.path.join(feature_root, name)):
        d = os.path.join(feature_root, name)
        feat = np.array([np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))]).squeeze()
    else:
        raise FileNotFoundError(path)
    if feat.ndim == 1:
        feat = feat[np.newaxis, :]
    return np.ascontiguousarray(feat, dtype=np.float32)


def pad_right(feats):
    """list of [T_i, d] tensors -> ([B, maxT, d], pad_lens)  (pad_to_maxlen_pre_modality_tensor_4)"""
    lens = [int(f.shape[0]) for f in feats]
    mx = max(lens)
    out = torch.zeros(len(feats), mx, feats[0].shape[1], dtype=torch.float32)
    for i, f in enumerate(feats):
        out[i, :lens[i]] = torch.as_tensor(f, dtype=torch.float32)
    return out, [mx - n for n in lens]


def collate(instances):
    """instances: dicts with 'audio','text','video','feat4' ([T,d]), 'emo','val','name'
    (Data_Feat_MOSEI_EmoVal_4F.__getitem__, feat_data.py:218-229) -> the reference's batch tuple."""
    batch, pads = {}, []
    for key, src in zip(KEYS, ('audio', 'text', 'video', 'feat4')):
        batch[key], p = pad_right([inst[src] for inst in instances])
        pads.append(p)
    emos = torch.FloatTensor([inst['emo'] for inst in instances])
    vals = torch.FloatTensor([inst['val'] for inst in instances])
    names = [inst['name'] for inst in instances]
    return batch, pads, emos, vals, names


def lengths_from_pads(data):
    """Valid frame counts (audio, text, video, feat4) of one batch tuple = maxT_m - pad_len (the `pads` the reference's
    collater returns and never uses, feat_data.py:244-253): what `lengths=` of the key-padding extension takes."""
    b, pads = data[0], data[1]
    return tuple(torch.tensor([b[k].shape[1] - int(p) for p in pad], dtype=torch.int32) for k, pad in zip(KEYS, pads))


def unpack(data, device):
    """What train_or_eval_model reads from one batch tuple (main :94-109), moved to `device`."""
    b = data[0]
    return (b['audios'].to(device, non_blocking=True), b['texts'].to(device, non_blocking=True),
            b['videos'].to(device, non_blocking=True), b['feat4s'].to(device, non_blocking=True),
            data[-2].float().to(device, non_blocking=True), data[-1])


FEAT_TYPES = ('utt', 'frm_align', 'frm_unalign')      # --feat_type (main_frame_val_text_missing.py:225)
_SRC = ('audio', 'text', 'video', 'feat4')


def map_feature(feature, dst_len):
    """[L, d] -> float32 [dst_len, d]: the reference's func_mapping_feature (read_data.py:120-137), quirks included.
    L <= dst_len: the rows, then zero rows (frames from then on).  L > dst_len: q, r = divmod(L, dst_len); pool = q and no padding if
    r == 0, else pool = q + 1 and dst_len - r zero frames in FRONT; row j = the sum of frames [j pool, (j + 1) pool) of the padded
    sequence divided by pool (never by the count of real frames).  Summed in float64 in frame order, one division, one rounding to
    float32: what the reference's float64 promotion (its np.zeros padding) followed by torch.FloatTensor computes, bit for bit."""
    x = np.asarray(feature)
    n = int(dst_len)
    if x.ndim != 2 or n < 1:
        from ._lib import SdumcError
        raise SdumcError(f"map_feature: a [T, d] feature and dst_len >= 1, not shape {x.shape} and {dst_len!r}")
    L, d = x.shape
    if L <= n:
        out = np.zeros((n, d), dtype=np.float32)
        out[:L] = x
        return out
    q, r = divmod(L, n)
    pool, pad = (q, 0) if r == 0 else (q + 1, n - r)
    xp = np.concatenate([np.zeros((pad, d)), x.astype(np.float64)]).reshape(n, pool, d)
    acc = xp[:, 0, :].copy()
    for t in range(1, pool):
        acc += xp[:, t, :]
    return (acc / pool).astype(np.float32)


def _resample_steps(feat_scale, feat_type):
    """Validated (feat_scale, feat_type) -> the passes in the reference's order (feat_data.py:117-126: feat_scale first, feat_type
    after it, so frm_align aligns to the COMPRESSED text length).  A pass is an integer k > 1, 'frm_align' or 'utt'."""
    from ._lib import SdumcError
    if isinstance(feat_scale, bool) or not isinstance(feat_scale, (int, float, np.integer, np.floating)) \
            or not np.isfinite(feat_scale) or feat_scale != int(feat_scale) or feat_scale < 1:
        raise SdumcError(f"feat_scale must be an integer >= 1, not {feat_scale!r}")
    if feat_type not in FEAT_TYPES:
        raise SdumcError(f"feat_type must be one of {FEAT_TYPES}, not {feat_type!r}")
    steps = [int(feat_scale)] if int(feat_scale) > 1 else []
    if feat_type != 'frm_unalign':
        steps.append(feat_type)
    return steps


def _target_lengths(lens, step):
    """lens: the four modalities' frame counts (audio, text, video, feat4), integer arrays [N] -> the same after one pass."""
    lens = [np.asarray(l, dtype=np.int64) for l in lens]
    if step == 'utt':
        return [np.ones_like(l) for l in lens]
    if step == 'frm_align':
        return [lens[1], lens[1], lens[1], lens[3]]      # audio, text, video to the text length; feat4 keeps its own
    return [-(-l // step) for l in lens]                  # ceil(L / k), every modality on its own


def resample_instances(instances, feat_scale=1, feat_type='frm_unalign'):
    """The reference's --feat_scale / --feat_type on the host: feature_scale_compress, then align_to_text or align_to_utt
    (read_data.py:178-200, applied in that order by the dataset constructors, feat_data.py:117-126) -> new instance dicts that
    collate() and DeviceFeatureStore(...) accept (float32 [T', d] arrays; every other key is carried over).
    feat_scale = k: every modality to ceil(T / k) frames, feat4 (the text slot of stream 1) by the same rule.  'frm_align': audio,
    text and video to the utterance's text length, feat4 keeps its own.  'utt': one frame per modality.  'frm_unalign': nothing.
    Every route is map_feature's float64 rule.  That includes 'utt', which stays [1, d]: the reference's align_to_utt is np.mean of
    the float32 array (pairwise float32 sums, a 1-D float32 result) and so LESS exact than this route; the two agree to the
    reference's own float32 rounding.  With both options the result of the first pass is rounded to float32 before the second (an
    instance, like a store, holds float32), where the reference hands its float64 arrays on unrounded: at most 2^-24 of the pooled
    magnitude apart.  DeviceFeatureStore.resampled computes the same on the device."""
    steps = _resample_steps(feat_scale, feat_type)
    out = [dict(inst) for inst in instances]
    for inst in out:
        for m in _SRC:
            x = np.asarray(inst[m], dtype=np.float32)
            inst[m] = x[np.newaxis, :] if x.ndim == 1 else x
    for step in steps:
        for inst in out:
            tgt = _target_lengths([[inst[m].shape[0]] for m in _SRC], step)
            for m, n in zip(_SRC, tgt):
                inst[m] = map_feature(inst[m], int(n[0]))
    return out


# ---- the random-missing protocol: frame and modality drops, decided per (seed, draw, modality, utterance, frame) ----------------------
# The rule (include/sdumc_hip.h states it beside sdumc_gather_batch, whose kernel evaluates it while it writes a batch's row maps):
#   word(c0) = philox4x32_10(ctr = (c0, e, MISSING_SITE + m, draw), key = (seed & 0xffffffff, seed >> 32))[0]
#   frame t of modality m (index in MODS) of utterance e (index in the store) is ABSENT
#       iff word(t) < floor(frame[m] * 2^32)  or  word(MISSING_UTT) < floor(modality[m] * 2^32)
# -- the dropout sites' "dropped when word < threshold" convention; a rate >= 1 makes every frame absent (its threshold does not fit
# 32 bits: a flag), a rate of 0 none.  An absent frame is a ZERO FEATURE ROW THAT STILL COUNTS AS A FRAME (the reference's
# audio_feat * mask, main_frame_val_text_missing.py:123-129, no rescale): lengths are unchanged, the row takes part in the softmaxes.
MISSING_SITE = 0x4D530000      # + m: counter word 2, disjoint from every dropout site (small integers) under the same seed
MISSING_UTT = 0xFFFFFFFF       # counter word 0 of the utterance-level draw (a frame index never reaches it)
_SPEC_MODS = ('audio', 'text', 'video', 'feat4')


def _philox_word0(c0, c1, c2, c3, k0, k1):
    """word 0 of Philox4x32-10 (Salmon et al., SC'11) for broadcastable uint32 counters: csrc/common.h's philox4x32_10 on the host"""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)])
    k0, k1, mask = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF, np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = c0 * np.uint64(0xD2511F53), c2 * np.uint64(0xCD9E8D57)      # (32 x 32 bits: exact in 64)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0.astype(np.uint32)


class MissingSpec:
    """A validated missing spec: frame / modality = four rates in MODS order ('audio', 'text', 'video', 'feat4'), seed < 2^64,
    draw < 2^32 (the epoch number in training, a fixed number in evaluation).  Bad values raise SdumcError, on the host."""
    __slots__ = ('frame', 'modality', 'seed', 'draw')

    def __init__(self, frame=None, modality=None, seed=0, draw=0):
        from ._lib import SdumcError

        def rates(arg, what):
            arg = {} if arg is None else arg
            if not hasattr(arg, 'items'):
                raise SdumcError(f"missing spec: {what} is a mapping from modality name to rate, not {arg!r}")
            out = [0.0] * 4
            for name, r in arg.items():
                if name not in _SPEC_MODS:
                    raise SdumcError(f"missing spec: unknown modality {name!r} in {what} (one of {_SPEC_MODS})")
                if isinstance(r, bool) or not isinstance(r, (int, float, np.integer, np.floating)) or not 0.0 <= float(r) <= 1.0:
                    raise SdumcError(f"missing spec: {what}[{name!r}] must be a rate in [0, 1], not {r!r}")
                out[_SPEC_MODS.index(name)] = float(r)
            return tuple(out)

        def integer(v, bits, what):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < 2 ** bits:
                raise SdumcError(f"missing spec: {what} must be an integer in [0, 2^{bits}), not {v!r}")
            return int(v)

        object.__setattr__(self, 'frame', rates(frame, 'frame'))
        object.__setattr__(self, 'modality', rates(modality, 'modality'))
        object.__setattr__(self, 'seed', integer(seed, 64, 'seed'))
        object.__setattr__(self, 'draw', integer(draw, 32, 'draw'))

    def __setattr__(self, name, value):
        raise AttributeError("a MissingSpec does not change: with_missing(...) / redrawn(draw) make a new one")

    def __repr__(self):
        f = {m: r for m, r in zip(_SPEC_MODS, self.frame) if r}
        u = {m: r for m, r in zip(_SPEC_MODS, self.modality) if r}
        return f"MissingSpec(frame={f}, modality={u}, seed={self.seed}, draw={self.draw})"

    def __eq__(self, other):
        return isinstance(other, MissingSpec) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    def __hash__(self):
        return hash((self.frame, self.modality, self.seed, self.draw))

    @property
    def enabled(self):
        """False: no rate above 0 -- nothing is ever absent, and a view's descriptors are the plain store's"""
        return any(r > 0.0 for r in self.frame + self.modality)

    def with_draw(self, draw):
        return MissingSpec(dict(zip(_SPEC_MODS, self.frame)), dict(zip(_SPEC_MODS, self.modality)), self.seed, draw)

    def thresholds(self, k):
        """modality index k -> (frame threshold, modality threshold, flags): the sdumc_gather_seg fields.  threshold =
        floor(rate * 2^32) where that fits 32 bits; a rate of 1 sets the flag instead (bit 0: frame level, bit 1: modality level)."""
        out, flags = [], 0
        for bit, rate in enumerate((self.frame[k], self.modality[k])):
            thr = int(rate * 4294967296.0)
            if thr > 0xFFFFFFFF:
                thr, flags = 0xFFFFFFFF, flags | (1 << bit)
            out.append(thr)
        return out[0], out[1], flags


def _as_spec(spec):
    if isinstance(spec, MissingSpec):
        return spec
    if hasattr(spec, 'keys'):
        from ._lib import SdumcError
        if set(spec.keys()) - set(MissingSpec.__slots__):
            raise SdumcError(f"missing spec: unknown fields {sorted(set(spec.keys()) - set(MissingSpec.__slots__))}")
        return MissingSpec(**dict(spec))
    from ._lib import SdumcError
    raise SdumcError(f"a missing spec is a MissingSpec or a mapping with frame / modality / seed / draw, not {spec!r}")


def _modality_index(modality):
    if isinstance(modality, str) and modality in _SPEC_MODS:
        return _SPEC_MODS.index(modality)
    if not isinstance(modality, (bool, str)) and isinstance(modality, (int, np.integer)) and 0 <= int(modality) < 4:
        return int(modality)
    from ._lib import SdumcError
    raise SdumcError(f"unknown modality {modality!r}: one of {_SPEC_MODS}, or its index 0..3")


def _missing_absent(spec, k, utt, t):
    """the rule for modality index k at broadcastable utterance indices `utt` and frame indices `t` -> bool array, True = absent"""
    ft, ut, flags = spec.thresholds(k)
    utt, t = np.asarray(utt, dtype=np.uint64) & np.uint64(0xFFFFFFFF), np.asarray(t, dtype=np.uint64)
    k0, k1 = spec.seed & 0xFFFFFFFF, spec.seed >> 32
    absent = np.zeros(np.broadcast(utt, t).shape, dtype=bool)
    if flags:
        absent[...] = True
        return absent
    if ft:
        absent |= _philox_word0(t, utt, MISSING_SITE + k, spec.draw, k0, k1) < np.uint32(ft)
    if ut:
        absent |= np.broadcast_to(_philox_word0(MISSING_UTT, utt, MISSING_SITE + k, spec.draw, k0, k1) < np.uint32(ut), absent.shape)
    return absent


def missing_keep(spec, modality, utt, length):
    """bool [length]: which of the `length` frames of modality `modality` (a name of ('audio', 'text', 'video', 'feat4') or its index)
    of utterance `utt` (its index in the store / dataset) are PRESENT under `spec` (a MissingSpec, or a mapping with its fields) --
    the rule above on the host, for a loader loop that masks its own batches: feat[~missing_keep(...)] = 0.  The same bits
    store.with_missing(...) applies on the device, whatever the batch."""
    from ._lib import SdumcError
    spec, k = _as_spec(spec), _modality_index(modality)
    if isinstance(utt, bool) or not isinstance(utt, (int, np.integer)) or not 0 <= int(utt) < 2 ** 32:
        raise SdumcError(f"missing_keep: utt is the utterance's index in the store, 0 <= utt < 2^32, not {utt!r}")
    if isinstance(length, bool) or not isinstance(length, (int, np.integer)) or not 0 <= int(length) < 0xFFFFFFFF:
        raise SdumcError(f"missing_keep: length must be a frame count, not {length!r}")
    return ~_missing_absent(spec, k, int(utt), np.arange(int(length), dtype=np.uint64))


class EpochPlan:
    """The batches of one epoch as the device sees them: ONE index tensor uploaded once (no per-batch host -> device copy inside the
    loop -- a pageable upload per step costs the host a synchronisation with the previous step), the host-side offsets into it and the
    padded shape (B, (T_audio, T_text, T_video, T_feat4)) of every batch."""

    def __init__(self, idx_d, offsets, shapes, idx_h=None):
        self.idx_d, self.offsets, self.shapes = idx_d, offsets, shapes
        self.idx_h = idx_h      # the same indices on the host, when the plan's maker kept them (host-side checks read these)

    def __len__(self):
        return len(self.shapes)

    def idx_ptr(self, i):
        return self.idx_d.data_ptr() + 8 * self.offsets[i]


class DeviceFeatureStore:
    """All pre-extracted features of a split, packed per modality into ONE device tensor [sum T, d]
    (MOSEI train at WavLM/Vicuna/MANet widths is tens of GB: it fits the 288 GB of one MI355X many times).
    `batch(indices)` assembles the reference's batch tuple on the GPU with a HIP gather/pad kernel
    (sdumc_gather_pad), so no feature bytes cross PCIe inside the training loop.  Replaces the roles of
    Data_Feat_MOSEI_EmoVal_4F.collater + pad_to_maxlen_pre_modality_tensor_4 (feat_data.py:232-253,
    read_data.py:223-248) for the hot path; the on-disk format is the reference's (read_feature).

    Every packed tensor ends in ONE all-zero row: a step can then read a batch IN PLACE through a row map (sdumc_net_io.row_map; entry
    of a padded frame = that row) instead of from a padded copy -- gather_desc(maps_out=...) writes the maps, 4 bytes per frame.

    planes=True (fp32 storage): every utterance is ALSO held as P3 planes (sdumc_p3_split of the packed tensor, three bf16 parts per
    value, 6 d bytes per row) -- split ONCE per dataset, where the reference re-reads the feature files every epoch; the store then
    takes 2.5x the fp32 bytes (the fp32 rows the weight gradients read + 1.5x for the planes the frame projections read).  A batch's
    planes are gathered like its fp32 rows (a padded row is zero in both, so this equals splitting the gathered batch bit for bit)."""

    MODS = ('audio', 'text', 'video', 'feat4')

    def __init__(self, instances, device='cuda', bf16=False, planes=False):
        """instances: iterable of dicts with 'audio','text','video','feat4' ([T, d] arrays), 'emo', 'val', 'name'.
        bf16=True holds the features as bf16 (half the HBM; what the engine's bf16-storage mode reads; widths % 8 == 0)."""
        import ctypes as C
        from . import _lib
        self._C, self._lib = C, _lib
        instances = list(instances)
        self.device = torch.device(device)
        self.names = [inst['name'] for inst in instances]
        self.vals = torch.tensor([float(inst['val']) for inst in instances], dtype=torch.float32, device=self.device)
        self.emos = torch.tensor([float(inst['emo']) for inst in instances], dtype=torch.float32, device=self.device)
        self.packed, self.start, self.length, self.dim = {}, {}, {}, {}
        for m in self.MODS:
            lens = [int(inst[m].shape[0]) for inst in instances]
            d = int(instances[0][m].shape[1])
            if d % 4:
                raise _lib.SdumcError(f"feature width {d} of '{m}' must be a multiple of 4")
            starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
            host = torch.zeros(sum(lens) + 1, d, dtype=torch.float32)      # (+ one all-zero row: what a padded frame's row-map entry names)
            for s, n, inst in zip(starts, lens, instances):
                host[s:s + n] = torch.as_tensor(inst[m], dtype=torch.float32)
            self.packed[m] = host.to(self.device).to(torch.bfloat16 if bf16 else torch.float32)
            if bf16 and d % 8:
                raise _lib.SdumcError(f"bf16 feature width {d} of '{m}' must be a multiple of 8")
            self.start[m] = torch.from_numpy(starts)
            self.length[m] = torch.tensor(lens, dtype=torch.int32)
            self.dim[m] = d
        self._device_tables()
        self.packed_p3 = None
        if planes:
            self.make_planes()

    def _device_tables(self):
        # store-wide tables on the device: a batch is then named by its index vector alone (sdumc_gather_batch)
        self.start_d = {m: self.start[m].to(self.device) for m in self.MODS}
        self.length_d = {m: self.length[m].to(self.device) for m in self.MODS}
        self._len_np = {m: self.length[m].numpy() for m in self.MODS}

    def make_planes(self):
        """The P3 planes of every packed tensor (fp32 storage, widths in whole 64-element k-tiles: what csrc/gemm_p3.hip reads)."""
        _lib = self._lib
        if any(t.dtype != torch.float32 for t in self.packed.values()):
            raise _lib.SdumcError("planes: the store holds bf16 features (the bf16-storage step reads them as they are)")
        if any(self.dim[m] % 64 for m in self.MODS):
            raise _lib.SdumcError("planes: feature widths must be multiples of 64")
        self.packed_p3 = {}
        for m in self.MODS:
            src, d = self.packed[m], self.dim[m]
            dst = torch.empty(src.shape[0], 6 * d, dtype=torch.uint8, device=self.device)
            _lib.check(_lib.lib.sdumc_p3_split(_lib.ptr(src), d, _lib.ptr(dst), 6 * d, src.shape[0], d, _lib.current_stream()), "sdumc_p3_split")
            self.packed_p3[m] = dst
        return self

    def resampled(self, feat_scale=1, feat_type='frm_unalign', planes=None):
        """The reference's --feat_scale / --feat_type (feature_scale_compress, align_to_text, align_to_utt: read_data.py:178-200,
        applied in the dataset constructors, feat_data.py:117-126) on the resident store: a NEW store with fewer (or aligned) frames
        per utterance, pooled on the device by sdumc_pool_frames -- one HBM-bound pass per modality, no feature byte crosses PCIe.
        Semantics and arithmetic are resample_instances': feat_scale first, feat_type after it (two passes when both are given).
        Same names, vals, emos, device and storage dtype; new packed / start / length tables (computed on the host, uploaded once).
        planes: None = as the source (rebuilt with make_planes()), True / False overrides.  The source is left untouched;
        feat_scale == 1 with 'frm_unalign' returns self.  Bad arguments raise SdumcError before anything is enqueued."""
        _lib = self._lib
        steps = _resample_steps(feat_scale, feat_type)
        if not steps:
            return self
        want_planes = (self.packed_p3 is not None) if planes is None else bool(planes)
        if want_planes and any(t.dtype != torch.float32 for t in self.packed.values()):
            raise _lib.SdumcError("planes: the store holds bf16 features (the bf16-storage step reads them as they are)")
        if want_planes and any(self.dim[m] % 64 for m in self.MODS):
            raise _lib.SdumcError("planes: feature widths must be multiples of 64")
        store = self
        for step in steps:
            store = store._pooled(_target_lengths([store._len_np[m] for m in self.MODS], step))
        if want_planes:
            store.make_planes()
        return store

    def _pooled(self, targets):
        """A new store (no planes) whose modality m holds targets[k][e] frames of utterance e: one sdumc_pool_frames launch each."""
        C, _lib = self._C, self._lib
        new = type(self).__new__(type(self))
        new._C, new._lib, new.device = C, _lib, self.device
        new.names, new.vals, new.emos = list(self.names), self.vals, self.emos
        new.packed, new.start, new.length, new.dim = {}, {}, {}, dict(self.dim)
        new.packed_p3 = None
        for m, tgt in zip(self.MODS, targets):
            tgt = np.asarray(tgt, dtype=np.int64)
            rows = int(tgt.sum())
            if tgt.shape != self._len_np[m].shape or int(tgt.min()) < 1 or rows >= 2 ** 31 - 1:
                raise _lib.SdumcError(f"resample: bad target lengths for '{m}'")
            new.start[m] = torch.from_numpy(np.concatenate([[0], np.cumsum(tgt)[:-1]]).astype(np.int64))
            new.length[m] = torch.from_numpy(tgt.astype(np.int32))
        new._device_tables()
        for m in self.MODS:
            src = self.packed[m]
            rows = int(new.length[m].sum())
            dst = torch.empty(rows + 1, self.dim[m], dtype=src.dtype, device=self.device)
            p = _lib.PoolFrames()
            p.src, p.dst = _lib.ptr(src), _lib.ptr(dst)
            p.src_start, p.src_len = _lib.ptr(self.start_d[m]), _lib.ptr(self.length_d[m])
            p.dst_start, p.dst_len = _lib.ptr(new.start_d[m]), _lib.ptr(new.length_d[m])
            p.src_rows, p.dst_rows = int(src.shape[0]) - 1, rows
            p.n_utts, p.cols, p.bf16 = len(self), self.dim[m], int(src.dtype == torch.bfloat16)
            _lib.check(_lib.lib.sdumc_pool_frames(C.byref(p), 0, _lib.current_stream()), "sdumc_pool_frames")
            new.packed[m] = dst
        return new

    def with_missing(self, frame=None, modality=None, seed=0, draw=0):
        """The random-missing protocol on this store: a VIEW (MissingView) that shares every tensor and table and whose batches lose
        frames -- frame = {modality name: rate} drops single frames, modality = {name: rate} drops the modality of a whole utterance;
        the rule is stated above missing_keep and in include/sdumc_hip.h.  An absent frame is a zero feature row that still counts as
        a frame: the reference's audio_feat * mask (main_frame_val_text_missing.py:123-129), no rescale, lengths unchanged.  Which
        frames go depends on (seed, draw, modality, utterance's index in the store, frame) alone: pass draw=epoch for a fresh draw per
        training epoch (view.redrawn(epoch)), a fixed draw for a reproducible corrupted test set.  No device work, no allocation:
        the gather launch that writes a batch's row maps (or padded copies) redirects the absent frames to the store's zero row, so
        the view goes wherever a store goes -- run_epoch, train_epoch, step_from_store, eval_epoch, saliency_epoch, batch_into, batch.
        'text' and 'feat4' are separate modalities (the two streams degrade independently); 'audio' and 'video' are shared by both
        streams.  Bad rates, names, seed or draw raise SdumcError here, on the host."""
        return MissingView(self, MissingSpec(frame, modality, seed, draw))

    @property
    def nbytes(self):
        n = sum(t.numel() * t.element_size() for t in self.packed.values())
        if self.packed_p3 is not None:
            n += sum(t.numel() for t in self.packed_p3.values())
        return n

    @classmethod
    def synthetic(cls, n, T, dims, seed=1234, device='cuda', min_frac=0.25, bf16=False, planes=False):
        """n utterances with per-sample lengths ~ U{ceil(min_frac * T_m) .. T_m} and N(0, 1) features, generated on the device
        (SURVEY §8d's variable-length synthetic inputs; no host copy of the tens of GB a real split holds)."""
        import ctypes as C
        from . import _lib
        self = cls.__new__(cls)
        self._C, self._lib = C, _lib
        self.device = torch.device(device)
        g = torch.Generator().manual_seed(seed)
        gd = torch.Generator(device=self.device).manual_seed(seed)
        self.names = [f"utt{i:06d}" for i in range(n)]
        self.vals = (torch.rand(n, generator=g) * 6 - 3).to(self.device)
        self.emos = torch.zeros(n, device=self.device)
        self.packed, self.start, self.length, self.dim = {}, {}, {}, {}
        for m, Tm, d in zip(self.MODS, T, dims):
            lo = max(1, int(np.ceil(Tm * min_frac)))
            lens = torch.randint(lo, Tm + 1, (n,), generator=g, dtype=torch.int32)
            starts = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens.to(torch.int64), 0)[:-1]])
            rows = int(lens.sum())
            self.packed[m] = torch.zeros(rows + 1, d, device=self.device, dtype=torch.bfloat16 if bf16 else torch.float32)      # (+ the zero row)
            self.packed[m][:rows] = torch.randn(rows, d, device=self.device, generator=gd)
            self.start[m], self.length[m], self.dim[m] = starts, lens, int(d)
        self._device_tables()
        self.packed_p3 = None
        if planes:
            self.make_planes()
        return self

    def batch_shape(self, indices):
        """(B, (T_audio, T_text, T_video, T_feat4)) of the padded batch -- host-side table lookups only."""
        idx = self._checked(indices)
        return int(idx.numel()), tuple(int(self.length[m][idx].max()) for m in self.MODS)

    def _checked(self, indices):
        """host-side range check: the gather kernel indexes device tables with these values"""
        idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
        n = len(self)
        if idx.numel() == 0 or int(idx.min()) < 0 or int(idx.max()) >= n:
            raise self._lib.SdumcError(f"sample index out of range [0, {n})")
        return idx

    def plan_epoch(self, batches):
        """batches: the epoch's index vectors (what a BatchSampler yields) -> EpochPlan: every index range-checked, one upload."""
        idxs = [self._checked(b) for b in batches]
        if not idxs:
            raise self._lib.SdumcError("plan_epoch: no batches")
        offsets = np.concatenate([[0], np.cumsum([i.numel() for i in idxs])]).astype(np.int64)
        shapes = []
        for i in idxs:
            ii = i.numpy()
            shapes.append((int(ii.size), tuple(int(self._len_np[m][ii].max()) for m in self.MODS)))
        idx_h = torch.cat(idxs)
        return EpochPlan(idx_h.to(self.device), [int(o) for o in offsets[:-1]], shapes, idx_h)

    def gather_desc(self, idx_ptr, B, T, outs, labels_out, lengths_out=None, planes_out=None, maps_out=None):
        """The sdumc_gather_batch descriptor of one batch: idx_ptr = device address of its int64 [B] index vector, T its padded frame
        counts, outs = 4 device buffers of >= B * T_m * d_m elements (fp32, or bf16 for a bf16 store), planes_out = 4 uint8 buffers of
        >= B * T_m * 6 d_m bytes (needs the store's planes), labels_out [>= B], lengths_out = optional 4 int32 [>= B].
        maps_out = 4 int32 buffers of >= B * T_m entries INSTEAD of outs / planes_out (pass outs=None): no padded copy is made, the
        step reads the store in place through these row maps (sdumc_net_io.row_map)."""
        _lib = self._lib
        if planes_out is not None and self.packed_p3 is None:
            raise _lib.SdumcError("this store holds no planes (DeviceFeatureStore(planes=True))")
        if (outs is None) == (maps_out is None):
            raise _lib.SdumcError("gather_desc: padded copies (outs) or row maps (maps_out), one of the two")
        g = _lib.GatherBatch()
        n = 0      # (the miss_* fields stay zero: no frame is absent; MissingView.gather_desc fills them)
        for k, m in enumerate(self.MODS):
            if maps_out is not None:
                sg = g.seg[n]
                sg.start_all, sg.len_all = _lib.ptr(self.start_d[m]), _lib.ptr(self.length_d[m])
                sg.map_out, sg.zero_row = _lib.ptr(maps_out[k]), int(self.packed[m].shape[0]) - 1
                sg.len_out = _lib.ptr(lengths_out[k]) if lengths_out is not None else None
                sg.Tmax, sg.d4 = int(T[k]), 0
                n += 1
                continue
            srcs = [(self.packed[m], outs[k], self.dim[m] * self.packed[m].element_size() // 16)]
            if planes_out is not None:
                srcs.append((self.packed_p3[m], planes_out[k], 6 * self.dim[m] // 16))
            for j, (src, dst, d4) in enumerate(srcs):
                sg = g.seg[n]
                sg.packed, sg.start_all, sg.len_all = _lib.ptr(src), _lib.ptr(self.start_d[m]), _lib.ptr(self.length_d[m])
                sg.out = _lib.ptr(dst)
                sg.len_out = _lib.ptr(lengths_out[k]) if (lengths_out is not None and j == 0) else None
                sg.Tmax, sg.d4 = int(T[k]), int(d4)
                n += 1
        g.nseg, g.B, g.idx = n, int(B), idx_ptr
        g.labels_all, g.labels_out = _lib.ptr(self.vals), _lib.ptr(labels_out)
        return g

    def batch_into(self, indices, outs, labels_out, lengths_out=None, planes_out=None):
        """Assembles the batch `indices` into caller-owned buffers: outs = 4 device tensors [B, Tmax_m, d_m] (e.g. the input
        buffers of an engine.TrainStep), labels_out [B]; lengths_out = optional 4 int32 device tensors (>= B) that receive the
        valid frame counts; planes_out = optional 4 uint8 tensors (>= B * Tmax_m * 6 d_m bytes) that receive the batch's P3 planes.
        One index-vector upload, ONE gather launch, nothing else."""
        _lib = self._lib
        idx = self._checked(indices)
        B = idx.numel()
        idx_d = idx.to(self.device, non_blocking=True)
        for k, m in enumerate(self.MODS):
            dst = outs[k]
            if dst.shape[0] != B or dst.shape[2] != self.dim[m] or not dst.is_contiguous() or dst.dtype != self.packed[m].dtype:
                raise _lib.SdumcError("batch_into: output buffer does not match the batch (shape / dtype)")
            if planes_out is not None and (planes_out[k].dtype != torch.uint8 or planes_out[k].numel() < B * dst.shape[1] * 6 * self.dim[m]):
                raise _lib.SdumcError("batch_into: planes buffer too small")
        g = self.gather_desc(idx_d.data_ptr(), B, [o.shape[1] for o in outs], outs, labels_out, lengths_out, planes_out)
        _lib.check(_lib.lib.sdumc_gather_batch(self._C.byref(g), 0, _lib.current_stream()), "sdumc_gather_batch")
        self._keep_idx = idx_d
        return lengths_out

    def __len__(self):
        return len(self.names)

    def get_featdim(self):
        return tuple(self.dim[m] for m in self.MODS)          # (adim, tdim, vdim, f4dim), feat_data.py:256-258

    def batch(self, indices):
        """-> (batch_dict, pads, emos, vals, names) with device tensors, identical to collate() of the same samples."""
        C, _lib = self._C, self._lib
        idx = torch.as_tensor(indices, dtype=torch.int64)
        B = idx.numel()
        out, pads = {}, []
        for key, m in zip(KEYS, self.MODS):
            lens = self.length[m][idx]
            tmax = int(lens.max())
            start_d = self.start[m][idx].to(self.device)
            len_d = lens.to(self.device)
            dst = torch.empty(B, tmax, self.dim[m], dtype=self.packed[m].dtype, device=self.device)
            dw = self.dim[m] if dst.dtype == torch.float32 else self.dim[m] // 2
            _lib.check(_lib.lib.sdumc_gather_pad(_lib.ptr(self.packed[m]), _lib.ptr(start_d), _lib.ptr(len_d), B, tmax,
                                                 dw, _lib.ptr(dst), _lib.current_stream()), "sdumc_gather_pad")
            out[key] = dst
            pads.append((tmax - lens).tolist())
        idx_d = idx.to(self.device)
        return out, pads, self.emos[idx_d], self.vals[idx_d], [self.names[i] for i in idx.tolist()]


class MissingView(DeviceFeatureStore):
    """store.with_missing(...): the store under a missing spec.  Holds nothing of its own but `base`, `spec` and the spec's descriptor
    fields: every tensor and table is the base store's (attribute reads fall through to it, so planes made later on the base are seen
    here too), and making a view does no device work -- one per epoch (view.redrawn(epoch)) rebuilds no arena, no cached step and no planes.  The one thing that
    differs is gather_desc, which fills the descriptor's miss_* fields: every consumer assembles its batches through it."""

    def __init__(self, base, spec):
        if isinstance(base, MissingView):      # a spec REPLACES the view's, it does not compose
            base = base.base
        self.base, self.spec = base, spec
        # the descriptor's fields, worked out once: (seed lo, seed hi, draw), per modality (frame threshold, modality threshold, flags);
        # None when every rate is 0 -- the view's descriptors are then the plain store's, bit for bit
        self._miss = ((spec.seed & 0xFFFFFFFF, spec.seed >> 32, spec.draw), tuple(spec.thresholds(k) for k in range(4))) if spec.enabled else None

    def __getattr__(self, name):      # (only reached for what the view does not hold itself)
        if name in ('base', 'spec', '_miss'):
            raise AttributeError(name)
        return getattr(self.base, name)

    def gather_desc(self, idx_ptr, B, T, outs, labels_out, lengths_out=None, planes_out=None, maps_out=None):
        """the store's descriptor with the protocol's fields filled in: every segment of a modality -- its rows and, in a padded copy with
        planes, its planes -- carries that modality's index and thresholds, so both lose the same frames"""
        g = DeviceFeatureStore.gather_desc(self, idx_ptr, B, T, outs, labels_out, lengths_out, planes_out, maps_out)
        if self._miss is not None:
            (g.miss_seed_lo, g.miss_seed_hi, g.miss_draw), per = self._miss[0], g.nseg // 4      # (segments are laid out modality by modality)
            g.miss_enable = 1
            for j in range(g.nseg):
                sg, k = g.seg[j], j // per
                sg.miss_mod = k
                sg.miss_frame_thr, sg.miss_utt_thr, sg.miss_all = self._miss[1][k]
        return g

    def with_missing(self, frame=None, modality=None, seed=0, draw=0):
        return self.base.with_missing(frame, modality, seed, draw)

    def redrawn(self, draw):
        """the same spec at another draw (the epoch number: a fresh mask per epoch, the same one whenever that epoch is replayed)"""
        return MissingView(self.base, self.spec.with_draw(draw))

    def make_planes(self):
        self.base.make_planes()
        return self

    def resampled(self, feat_scale=1, feat_type='frm_unalign', planes=None):
        from ._lib import SdumcError
        raise SdumcError("resampled: not on a with_missing view (the mask is defined on the frames of the store it was made on) -- "
                         "pool first, then view: store.resampled(...).with_missing(...)")

    def batch(self, indices):
        """as DeviceFeatureStore.batch, through batch_into (the one launch that knows the protocol): absent frames are zero rows"""
        idx = self._checked(indices)
        B, T = self.batch_shape(idx)
        outs = [torch.empty(B, T[k], self.dim[m], dtype=self.packed[m].dtype, device=self.device) for k, m in enumerate(self.MODS)]
        labels = torch.empty(B, dtype=torch.float32, device=self.device)
        self.batch_into(idx, outs, labels)
        pads = [(T[k] - self.length[m][idx]).tolist() for k, m in enumerate(self.MODS)]
        idx_d = idx.to(self.device)
        return dict(zip(KEYS, outs)), pads, self.emos[idx_d], self.vals[idx_d], [self.names[i] for i in idx.tolist()]

    def absent_rows(self, modality):
        """bool numpy [frames of the store]: True where the packed row (start[e] + t, store order, without the trailing zero row) of
        `modality` is absent under the spec -- the rule on the host, for every frame at once"""
        k = _modality_index(modality)
        lens = self._len_np[self.MODS[k]].astype(np.int64)
        utt = np.repeat(np.arange(lens.size, dtype=np.int64), lens)
        t = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(self.start[self.MODS[k]].numpy(), lens)
        return _missing_absent(self.spec, k, utt, t)

    def materialized(self, planes=None):
        """A NEW ordinary store with the spec burnt in: the packed tensors cloned, the absent rows zeroed (torch indexing on the device),
        the planes split again -- a fixed corrupted test set to share or checkpoint.  Shares the base's labels, names and tables.
        planes: None = as the base, True / False overrides.  Its batches hold the bits this view's batches hold."""
        base, _lib = self.base, self._lib
        want_planes = (base.packed_p3 is not None) if planes is None else bool(planes)
        new = DeviceFeatureStore.__new__(DeviceFeatureStore)
        new._C, new._lib, new.device = base._C, _lib, base.device
        new.names, new.vals, new.emos = list(base.names), base.vals, base.emos
        new.start, new.length, new.dim = dict(base.start), dict(base.length), dict(base.dim)
        new.start_d, new.length_d, new._len_np = dict(base.start_d), dict(base.length_d), dict(base._len_np)
        new.packed, new.packed_p3 = {}, None
        for m in self.MODS:
            t = base.packed[m].clone()
            rows = np.flatnonzero(self.absent_rows(m))
            if rows.size:
                t[torch.from_numpy(rows).to(base.device)] = 0
            new.packed[m] = t
        if want_planes:
            new.make_planes()
        return new
