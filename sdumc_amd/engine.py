"""Thin Python host over the network-level C ABI (include/sdumc_hip.h, engine.hip).

PyTorch-ROCm is used for device memory and streams only.  Everything numeric
happens in libsdumc_hip.so; there is no CPU or torch fallback.
"""
import collections
import ctypes as C

import torch

from . import _lib, epoch
from ._lib import lib, check, ptr

D, H, NQ, RNC_DIM = _lib.D, _lib.H, _lib.NQ, _lib.RNC_DIM
P_FRAME, P_MLP = 0.5, 0.3        # model :54,:77 / model :187 (constructor default; --dropout is never forwarded)
DEFAULT_WEIGHTS = (0.5, 0.5, 0.1, 0.7, 0.1, 0.8)      # main :234-239
PUBLISHED_WEIGHTS = (0.5, 0.5, 0.0, 0.0, 0.13, 0.5)   # shell/main_text_missing_icassp.sh:6


class ParamLayout:
    """name -> (offset, shape, live) of the flat parameter buffer for feature widths (da, dt, dv)."""

    _cache = {}

    def __init__(self, da, dt, dv):
        self.dims = (int(da), int(dt), int(dv))
        need = -lib.sdumc_param_table(*self.dims, None, 0)
        buf = C.create_string_buffer(need)
        n = lib.sdumc_param_table(*self.dims, buf, need)
        if n < 0:
            raise _lib.SdumcError("sdumc_param_table failed")
        self.entries = {}
        self.order = []
        for line in buf.value.decode().splitlines():
            name, off, rows, cols, live = line.split()
            shape = (int(rows), int(cols)) if int(cols) else (int(rows),)
            self.entries[name] = (int(off), shape, bool(int(live)))
            self.order.append(name)
        self.total = lib.sdumc_param_count(*self.dims)
        self.live = lib.sdumc_param_live_count(*self.dims)
        # [0, early): utterance-level layers (gradients final after backward phase 0), [early, live): frame-level
        self.early = lib.sdumc_param_early_count(*self.dims)

    @classmethod
    def get(cls, da, dt, dv):
        key = (int(da), int(dt), int(dv))
        if key not in cls._cache:
            cls._cache[key] = cls(*key)
        return cls._cache[key]

    def views(self, flat):
        """dict name -> view of `flat` (no copies)."""
        out = {}
        for name in self.order:
            off, shape, _ = self.entries[name]
            n = 1
            for s in shape:
                n *= s
            out[name] = flat[off:off + n].view(shape)
        return out

    def live_names(self):
        return [n for n in self.order if self.entries[n][2]]


class TensorRates:
    """Per-tensor learning-rate scale, decay scale and frozen flag of the fused step (TrainStep / FusedTrainer: lr_scale=, decay_scale=,
    freeze=), resolved ONCE on the host: torch.optim.Adam with one parameter group per tensor and one shared step count.
    lr_scale / decay_scale: dicts {fnmatch pattern over ParamLayout's names: a finite Python number >= 0}, applied in order -- a later
    match overrides an earlier one; freeze: patterns of the tensors that are torch's requires_grad = False.  A pattern that matches no
    name of the layout raises; one that matches only parameters that never get a gradient is accepted and changes nothing; an entry
    whose pattern reaches frozen tensors ONLY raises (frozen and scaled contradict each other), while a wider one ('*.bias') scales the
    others and leaves the frozen ones among its matches frozen, their scales at 1.
    .names / .lr_scale / .decay_scale / .frozen: one entry per live tensor, in sdumc_param_table order (layout.live_names());
    .c: the same as the sdumc_tensor_rates every step's cfg.rates points at."""

    def __init__(self, layout, lr_scale=None, decay_scale=None, freeze=None):
        import fnmatch
        import math
        import numpy as np
        self.layout = layout
        self.names = layout.live_names()
        n = len(self.names)
        if n > _lib.RATES_MAX_SEGS:
            raise _lib.SdumcError(f"TensorRates: {n} live tensors, the table holds {_lib.RATES_MAX_SEGS}")
        index = {name: i for i, name in enumerate(self.names)}

        def matches(pattern, what):
            if not isinstance(pattern, str):
                raise _lib.SdumcError(f"{what}: patterns are strings, not {pattern!r}")
            hit = [name for name in layout.order if fnmatch.fnmatchcase(name, pattern)]
            if not hit:
                raise _lib.SdumcError(f"{what}: pattern {pattern!r} matches no parameter of the layout")
            return [index[name] for name in hit if name in index]      # (dead parameters: accepted, nothing to scale)

        self.frozen = np.zeros(n, dtype=bool)
        if freeze is not None:
            if isinstance(freeze, str) or not isinstance(freeze, (tuple, list)):
                raise _lib.SdumcError(f"freeze must be a tuple or list of patterns or None, not {freeze!r}")
            for pattern in freeze:
                self.frozen[matches(pattern, "freeze")] = True

        def scales(table, what):
            out = np.ones(n, dtype=np.float32)
            if table is None:
                return out
            if not isinstance(table, dict):
                raise _lib.SdumcError(f"{what} must be a dict {{pattern: scale}} or None, not {table!r}")
            for pattern, s in table.items():
                hit = matches(pattern, what)
                if isinstance(s, bool) or not isinstance(s, (int, float)) or not math.isfinite(s) or s < 0 \
                        or not math.isfinite(C.c_float(s).value):
                    raise _lib.SdumcError(f"{what}[{pattern!r}] must be a finite number >= 0, not {s!r}")
                free = [i for i in hit if not self.frozen[i]]
                if hit and not free:
                    raise _lib.SdumcError(f"{what}[{pattern!r}] names frozen tensors only: {[self.names[i] for i in hit]} are frozen "
                                          "AND given a scale")
                out[free] = s
            return out

        self.lr_scale = scales(lr_scale, "lr_scale")
        self.decay_scale = scales(decay_scale, "decay_scale")
        self.c = _lib.TensorRates()
        self.c.n = n
        for i in range(n):
            self.c.lr_scale[i], self.c.wd_scale[i], self.c.frozen[i] = float(self.lr_scale[i]), float(self.decay_scale[i]), int(self.frozen[i])

    @staticmethod
    def wanted(lr_scale, decay_scale, freeze):
        return lr_scale is not None or decay_scale is not None or freeze is not None

    def segments(self):
        """(offset, n, lr_scale, decay_scale, frozen) per live tensor: the table ops.adam_step_rates / ops.zero_segments take"""
        out = []
        for i, name in enumerate(self.names):
            off, shape, _ = self.layout.entries[name]
            n = 1
            for s in shape:
                n *= s
            out.append((off, n, float(self.lr_scale[i]), float(self.decay_scale[i]), bool(self.frozen[i])))
        return out


def _require_cuda(*tensors, dtypes=(torch.float32,)):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.SdumcError("sdumc_amd runs on the GPU only: got a CPU tensor (there is no CPU fallback)")
        if t.dtype not in dtypes or not t.is_contiguous():
            raise _lib.SdumcError("expected contiguous " + " / ".join(str(d).replace("torch.", "") for d in dtypes) + " tensors")


def bf16_mode(bf16, dims):
    """sdumc_net_dims.bf16 for the Python-level switch: False -> 0 (fp32); True -> 2 = bf16 STORAGE of features, projected
    frames, keys and frame-level gradients (BASELINE configs[2] / [4]) when the feature widths are whole 64-element k-tiles,
    else 1; "operands" -> 1 = fp32 storage, frame-level GEMM operands rounded to bf16 on their way to the matrix cores."""
    if not bf16:
        return 0
    if bf16 == "operands" or (not isinstance(bf16, bool) and bf16 == 1):
        return 1
    return 2 if all(int(d) % 64 == 0 for d in dims[:3]) else 1


def planes_wanted(planes, dims, bf16):
    """Whether a step / call keeps bf16-plane copies of its fp32 features (sdumc_net_io.*_p3; csrc/gemm_p3.hip: the frame and key
    projections then run on operands split once per tensor).  OPT-IN (planes=True): the caller states that the installed batch is
    RESIDENT -- run many times, or assembled from a DeviceFeatureStore(planes=True) whose planes were split once per dataset.  A loop
    that installs a fresh batch per step (set_batch per step) would re-split ~224 MB per step at C2 for one use,
    ~0.15-0.2 ms against the ~0.015 ms the planes save: there the default (False = the in-kernel split of csrc/gemm_wide.hip) is the
    faster path.  None: the environment's SDUMC_P3 (A/B runs), else False.  Needs fp32 storage and widths in whole 64-element k-tiles;
    costs 1.5x the features' bytes on top of them."""
    import os
    if planes is None:
        planes = os.environ.get("SDUMC_P3", "0") == "1"
    return bool(planes) and bf16_mode(bf16, dims) == 0 and all(int(d) % 64 == 0 for d in dims[:3])


def p3_split_into(src, dst):
    """src fp32 [..., d] contiguous -> dst uint8 [rows, 6 d]: the three bf16 planes of every value (exact: they sum to it)"""
    d = src.shape[-1]
    rows = src.numel() // d
    check(lib.sdumc_p3_split(ptr(src), d, ptr(dst), 6 * d, rows, d, _lib.current_stream()), "sdumc_p3_split")
    return dst


def _planes_buffer(rows, d, device):
    """uninitialised uint8 [rows, 6 d]: where the three bf16 planes of an fp32 [rows, d] tensor go (p3_split_into, the store's gather)"""
    return torch.empty(rows, 6 * d, dtype=torch.uint8, device=device)


def make_dims(B, streams, Ta, Tv, Tt, dims, train, sample0=0, p_mlp=P_MLP, bf16=False):
    d = _lib.NetDims()
    d.B, d.streams, d.Ta, d.Tv = B, streams, Ta, Tv
    d.Tt[0] = Tt[0]
    d.Tt[1] = Tt[1] if len(Tt) > 1 else Tt[0]
    d.da, d.dt, d.dv = dims[0], dims[1], dims[2]
    d.train = 1 if train else 0
    d.sample0 = sample0
    d.p_frame, d.p_mlp = P_FRAME, p_mlp
    d.bf16 = bf16_mode(bf16, dims)
    return d


class ExecContext:
    """A caller-owned execution context of the C ABI (sdumc_ctx_create): its own internal side streams and event ring.
    Steps driven concurrently from several host threads (each on its own torch stream) take one context each; without one,
    every call on a device shares that device's default context and must come from one thread at a time."""

    def __init__(self):
        h = C.c_void_p()
        check(lib.sdumc_ctx_create(C.byref(h)), "sdumc_ctx_create")
        self.handle = h

    OPTIONS = {"concurrency": 0, "background_lane": 1, "chain_cluster": 2, "split": 3}

    def set_option(self, name, value):
        """Schedule options of THIS context only (sdumc_ctx_set_option): 'concurrency' 0 | 1, 'background_lane' 0 | 2 | 3,
        'chain_cluster' 0 | 1, 'split' 0..15 (which fp32 GEMM kernel families multiply on the bf16 matrix pipe: sdumc_hip.h,
        sdumc_set_split_); None (or a negative value) returns the option to the process-wide default."""
        check(lib.sdumc_ctx_set_option(self.handle, self.OPTIONS[name], -1 if value is None else int(value)), "sdumc_ctx_set_option")

    def close(self):
        if self.handle:
            lib.sdumc_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def backward_schedule(call, phases=3):
    """Debug: the record the backward pass of `call` (a NetCall or TrainStep: its .dims and .io, the context's options included) would
    take -- {field: int} of sdumc_debug_backward_schedule; phases 3 = the single call (NetCall.backward, the fused step), 1 / 2 =
    sdumc_net_backward_phase 0 / 1.  A TrainStep's frozen frame projections (freeze=: weight AND bias) are passed as the step passes
    them.  Launches nothing."""
    frozen = 0
    rates = getattr(call, "rates", None)
    if rates is not None:
        is_frozen = dict(zip(rates.names, rates.frozen))
        for m in range(3):
            if is_frozen.get(f"frame_dim_reshape_{m}.weight") and is_frozen.get(f"frame_dim_reshape_{m}.bias"):
                frozen |= 1 << m
    args = (C.byref(call.dims), C.byref(call.io), int(phases), frozen, _lib.current_stream())
    need = -lib.sdumc_debug_backward_schedule(*args, None, 0)
    if need <= 0:
        raise _lib.SdumcError("sdumc_debug_backward_schedule: arguments the call itself would refuse")
    buf = C.create_string_buffer(need)
    if lib.sdumc_debug_backward_schedule(*args, buf, need) <= 0:
        raise _lib.SdumcError("sdumc_debug_backward_schedule failed")
    return {k: int(v) for k, v in (line.split() for line in buf.value.decode().splitlines())}


class RngState:
    """Device-resident {seed_lo, seed_hi, call}: lets captured graphs draw fresh masks per replay."""

    def __init__(self, seed, device, call=0):
        self.t = torch.tensor([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, call], dtype=torch.int64,
                              device="cpu").to(torch.int32).to(device)

    def set_call(self, call):
        self.t[2] = call

    @property
    def call(self):
        return int(self.t[2].item()) & 0xFFFFFFFF


def _lengths_arg(lengths, B, n, device):
    """(audio, text, video[, feat4]) valid-frame counts -> n contiguous cuda int32 tensors of B entries."""
    if lengths is None:
        return None
    lengths = list(lengths)
    if len(lengths) != n:
        raise _lib.SdumcError(f"lengths: expected {n} per-modality tensors (audio, text, video" + (", feat4)" if n == 4 else ")"))
    out = []
    for l in lengths:
        t = torch.as_tensor(l, dtype=torch.int32).reshape(-1).to(device).contiguous()
        if t.numel() != B:
            raise _lib.SdumcError("lengths: one entry per sample of the batch")
        out.append(t)
    return out


def _copy_lengths(io, own, new, B):
    """set_lengths of a NetCall / TrainStep: `new` (_lengths_arg's tensors, or None = extension off) is copied into the object's OWN
    [B] int32 buffers `own` -- allocated on first use, the same addresses from then on (a captured graph keeps reading them) -- and
    io.lengths points at them (None: at nothing).  Returns the own buffers."""
    for i in range(4):
        io.lengths[i] = None
    if new is None:
        return own
    if own is None:
        own = [torch.empty(B, dtype=torch.int32, device=t.device) for t in new]
    for i, (dst, src) in enumerate(zip(own, new)):
        io.lengths[i] = ptr(dst)
        dst.copy_(src, non_blocking=True)
    return own


class NetCall:
    """One network invocation (1 or 2 streams): owns workspace + outputs, supports backward.
    `lengths` (extension, default None = the reference's behaviour): per-modality valid frame counts
    (audio, text[, feat4 when two streams], video -> given as (audio, text, video) or (audio, text, video, feat4));
    padded frames are then masked out of the six attention poolings."""

    def __init__(self, flat_params, audio, texts, video, train, rng, sample0=0, p_mlp=P_MLP, bf16=False, lengths=None,
                 ctx=None, planes=None, bits_next=False):
        texts = list(texts)
        _require_cuda(flat_params)
        _require_cuda(audio, video, *texts, dtypes=(torch.float32, torch.bfloat16))
        S = len(texts)
        B, Ta, da = audio.shape
        store = torch.bfloat16 if bf16_mode(bf16, (da, texts[0].shape[2], video.shape[2])) == 2 else torch.float32
        # bf16-storage mode reads bf16 features (a DeviceFeatureStore(bf16=True) hands them over as such; fp32 inputs are
        # converted once, here); the other modes read fp32
        audio, video = audio.to(store), video.to(store)
        texts = [t.to(store) for t in texts]
        Tv, dv = video.shape[1], video.shape[2]
        dt = texts[0].shape[2]
        for t in texts:
            if t.shape[0] != B or t.shape[2] != dt:
                raise _lib.SdumcError("text-slot inputs must share batch and width (SURVEY §8b: feat4 width == text width)")
        if video.shape[0] != B:
            raise _lib.SdumcError("batch mismatch")
        self.dims = make_dims(B, S, Ta, Tv, [t.shape[1] for t in texts], (da, dt, dv), train, sample0, p_mlp, bf16)
        self.layout = ParamLayout.get(da, dt, dv)
        if flat_params.numel() != self.layout.total:
            raise _lib.SdumcError("flat parameter buffer has the wrong size")
        dev = audio.device
        nbytes = lib.sdumc_net_workspace_bytes(C.byref(self.dims))
        if nbytes == 0:
            raise _lib.SdumcError("invalid network dimensions")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        V = B * S
        self.V, self.B, self.S = V, B, S
        self.vals = torch.empty(V, 1, device=dev)
        self.fused = torch.empty(V, H, device=dev)
        self.rnc = torch.empty(V, RNC_DIM, device=dev)
        self.text_hidden = torch.empty(V, D, device=dev)
        self.cross_text = torch.empty(V, NQ, H, device=dev)
        self._keep = (flat_params, audio, texts, video, rng)
        io = _lib.NetIO()
        io.audio, io.video = ptr(audio), ptr(video)
        io.text[0] = ptr(texts[0])
        io.text[1] = ptr(texts[1]) if S == 2 else None
        io.params = ptr(flat_params)
        io.rng_state = ptr(rng.t) if rng is not None else None
        io.workspace, io.workspace_bytes = ptr(self.workspace), nbytes
        io.vals, io.fused, io.rnc = ptr(self.vals), ptr(self.fused), ptr(self.rnc)
        io.text_hidden, io.cross_text = ptr(self.text_hidden), ptr(self.cross_text)
        self._lengths = _lengths_arg(lengths, B, 4 if S == 2 else 3, dev)
        if self._lengths is not None:
            for i, t in enumerate(self._lengths):
                io.lengths[i] = ptr(t)
        self._ctx = ctx
        io.ctx = ctx.handle if ctx is not None else None
        self._planes = None
        if planes_wanted(planes, (da, dt, dv), bf16):      # bf16-plane copies of the features, split once for the life of this call object
            mk = lambda t: _planes_buffer(t.shape[0] * t.shape[1], t.shape[2], dev)
            self._planes = (mk(audio), mk(video), [mk(t) for t in texts])
            io.audio_p3, io.video_p3 = ptr(self._planes[0]), ptr(self._planes[1])
            for i, t in enumerate(self._planes[2]):
                io.text_p3[i] = ptr(t)
        # fp32 train-mode calls that are repeated step after step on this object (the data-parallel backend): the NEXT call's frame-level
        # keep-bits are generated in this call's middle (sdumc_net_io.bits_next; the Philox counter must advance by 2 between calls,
        # as HipBackend.adam and sdumc_train_step do) -- bit-identical masks, tagged; any other sequence regenerates at the head
        self._bits_next = None
        if bits_next and train and rng is not None:
            nb = lib.sdumc_net_bits_next_bytes(C.byref(self.dims))
            if nb:
                self._bits_next = torch.zeros(nb, dtype=torch.uint8, device=dev)
                io.bits_next = ptr(self._bits_next)
        self.io = io
        self._feat_scratch = None
        self.d_inputs = (None, [None] * S, None)
        self.refresh_planes()

    def refresh_planes(self):
        """Re-split the feature tensors this call object was built on (a caller that overwrites them in place -- the data-parallel
        backend's resident batch buffers -- calls this after every new batch)."""
        if self._planes is None:
            return
        _, audio, texts, video, _ = self._keep
        p3_split_into(audio, self._planes[0])
        p3_split_into(video, self._planes[1])
        for t, dst in zip(texts, self._planes[2]):
            p3_split_into(t, dst)

    def set_lengths(self, lengths):
        """Key-padding extension for the next forward: per-modality valid frame counts, or None = the reference's behaviour."""
        new = _lengths_arg(lengths, self.B, 4 if self.S == 2 else 3, self.vals.device)
        self._lengths = _copy_lengths(self.io, self._lengths, new, self.B)

    def forward(self):
        check(lib.sdumc_net_forward(C.byref(self.dims), C.byref(self.io), _lib.current_stream()), "sdumc_net_forward")
        return self.vals, self.fused, self.rnc, self.text_hidden, self.cross_text

    def next_call(self):
        """After the step that this forward / backward pair belongs to (the caller has advanced the Philox counter by 2): the next
        forward reads the keep-bits set this one filled."""
        if self._bits_next is not None:
            self.io.bits_phase ^= 1

    def backward(self, d_vals, d_fused, d_rnc, d_text_hidden, d_cross_text, grads=None, feature_grads=None):
        """Returns the flat gradient bucket [live] (allocated zeroed when not given).
        feature_grads: None = parameters only.  True, or one boolean per input in the order (audio, *texts, video), also asks for the
        gradients with respect to those feature tensors: afterwards self.d_inputs == (d_audio, [d_text ...], d_video), fresh fp32
        tensors shaped like the inputs, None where not asked (with two streams d_audio / d_video are the sum over both)."""
        _require_cuda(d_vals, d_fused, d_rnc, d_text_hidden, d_cross_text)
        if grads is None:
            grads = torch.zeros(self.layout.live, device=self.vals.device)
        g = _lib.NetGrads()
        g.d_vals, g.d_fused, g.d_rnc = ptr(d_vals), ptr(d_fused), ptr(d_rnc)
        g.d_text_hidden, g.d_cross_text = ptr(d_text_hidden), ptr(d_cross_text)
        g.grads = ptr(grads)
        self.d_inputs = (None, [None] * self.S, None)
        if feature_grads is not None and feature_grads is not False:
            want = (True,) * (2 + self.S) if feature_grads is True else tuple(bool(w) for w in feature_grads)
            if len(want) != 2 + self.S:
                raise _lib.SdumcError("feature_grads: True, or one boolean per input (audio, *texts, video)")
            if any(want):
                if self.dims.bf16 == 2:
                    raise _lib.SdumcError("feature gradients are not available in bf16 storage")
                _, audio, texts, video, _ = self._keep
                if self._feat_scratch is None:      # the packed transposed frame weights: once per call object
                    nb = lib.sdumc_net_feature_grad_scratch_bytes(C.byref(self.dims))
                    self._feat_scratch = torch.empty(nb, dtype=torch.uint8, device=self.vals.device)
                g.feat_scratch, g.feat_scratch_bytes = ptr(self._feat_scratch), self._feat_scratch.numel()
                mk = lambda t, w: torch.empty(t.shape, dtype=torch.float32, device=t.device) if w else None
                d_audio, d_video = mk(audio, want[0]), mk(video, want[-1])
                d_texts = [mk(t, w) for t, w in zip(texts, want[1:-1])]
                g.d_audio, g.d_video = ptr(d_audio), ptr(d_video)
                for i, t in enumerate(d_texts):
                    g.d_text[i] = ptr(t)
                self.d_inputs = (d_audio, d_texts, d_video)
        check(lib.sdumc_net_backward(C.byref(self.dims), C.byref(self.io), C.byref(g), _lib.current_stream()),
              "sdumc_net_backward")
        return grads


class _OptStateMixin:
    """Optimiser / RNG state of one training run: .adam_m .adam_v [live], .hyper = device {lr, step count t, lr/(1-b1^t),
    sqrt(1-b2^t)} (the last two are recomputed from t by every step), .rng = device Philox {seed, call}."""

    def optimizer_state(self):
        """(exp_avg, exp_avg_sq, step) -- what checkpoint.adam_state_from_flat takes."""
        return self.adam_m, self.adam_v, int(round(float(self.hyper[1].item())))

    def load_optimizer_state(self, adam_m, adam_v, step):
        """Resume (main_frame_val_text_missing.py:375 saves 'optimizer'; checkpoint.flat_from_adam_state gives the flat
        moments): installs the Adam moments, the step count that drives the bias correction, and the dropout call
        counter (two forward calls per step), so that the next step continues the interrupted run exactly."""
        if adam_m.numel() != self.adam_m.numel() or adam_v.numel() != self.adam_v.numel():
            raise _lib.SdumcError("load_optimizer_state: moment buffers must have layout.live elements")
        step = int(step)
        self.adam_m.copy_(adam_m.reshape(-1).to(self.adam_m.device))
        self.adam_v.copy_(adam_v.reshape(-1).to(self.adam_v.device))
        self.hyper[1] = float(step)
        self.rng.set_call(2 * step)

    ema_params = None      # with ema_decay: the averaged weights, a flat tensor laid out like .params (ParamLayout.total)
    decoupled_decay = False      # True: decoupled weight decay, the decoupled form of the step's last launch (sdumc_adamw_step)

    def load_ema(self, flat):
        """Resume: installs a saved average (checkpoint.load_ema gives the flat tensor) -- ParamLayout.total elements, copied to the
        run's device; the next step continues an uninterrupted run's average bit for bit."""
        if self.ema_params is None:
            raise _lib.SdumcError("load_ema: this run keeps no averaged weights (ema_decay=)")
        if not torch.is_tensor(flat) or flat.dtype != torch.float32 or flat.numel() != self.ema_params.numel():
            raise _lib.SdumcError(f"load_ema: expected a flat fp32 tensor of {self.ema_params.numel()} elements (ParamLayout.total)")
        if flat.device.type not in ("cpu", "cuda") or (flat.is_cuda and flat.device != self.ema_params.device):
            raise _lib.SdumcError(f"load_ema: the average lives on {self.ema_params.device}, not on {flat.device}")
        self.ema_params.copy_(flat.reshape(-1))

    def reset_ema(self):
        """The average starts again from the current parameters (a copy of their bits)."""
        if self.ema_params is None:
            raise _lib.SdumcError("reset_ema: this run keeps no averaged weights (ema_decay=)")
        self.ema_params.copy_(self.params)


_NO4 = (None,) * 4


def _guard_buffers(live, dev):
    """(guard float[4], scratch) of sdumc_grad_guard over a bucket of `live` floats"""
    nb = int(lib.sdumc_grad_guard_scratch_bytes(int(live)))
    return torch.zeros(4, device=dev), torch.empty(nb, dtype=torch.uint8, device=dev)

# One input source of a TrainStep (TrainStep._bind): feats = the (audio, text, video, feat4) tensors the step reads -- padded [B, T, d]
# batches, or a store's packed [rows, d] tensors when maps is given --, planes = their four bf16-plane tensors or None, maps = four
# int32 row maps or None, store_rows = the packed tensors' row counts (0 without maps), labels [B].  The record's references are what
# keeps a borrowed batch alive.
_Source = collections.namedtuple("_Source", "feats planes maps store_rows labels")


def _bind_source(io, src):
    """Points the inputs of `io` (an sdumc_net_io) at `src` (a _Source; None = at nothing).  The ONLY code that writes its feature,
    plane, row-map and store_rows fields."""
    feats, planes, maps, rows = src[:4] if src is not None else (_NO4, None, None, (0,) * 4)
    io.audio, io.text[0], io.video, io.text[1] = (ptr(t) for t in feats)
    io.audio_p3, io.text_p3[0], io.video_p3, io.text_p3[1] = (ptr(t) for t in planes or _NO4)
    for i, m in enumerate(maps or _NO4):
        io.row_map[i] = ptr(m)
        io.store_rows[i] = rows[i]


def _store_source(store, st, labels):
    """`store` read in place through the row maps of input set `st`: its packed tensors, and their planes where it holds some"""
    feats = tuple([store.packed[m] for m in store.MODS])
    planes = tuple([store.packed_p3[m] for m in store.MODS]) if store.packed_p3 is not None else None
    return _Source(feats, planes, st.ensure_maps(), tuple([t.shape[0] for t in feats]), labels)


class TrainStep(_OptStateMixin):
    """The fused two-stream self-distillation step (main :119-150) on one GPU:
    forward(both streams) -> 6 losses -> backward -> Adam, ~150 launches on one stream,
    optionally captured into a hipGraph (torch.cuda.CUDAGraph) and replayed.

    Inputs: the step reads ONE bound source at a time, installed by set_batch (a copy into the step's writable home), use_set (an input
    set of the arena), use_store (a DeviceFeatureStore in place, through row maps) or use_batch (the caller's tensors, zero-copy); whether
    planes are read is a property of what is bound.  The home is the step's own buffers, or with an arena the padded views of the set
    last named by use_set / use_store (set 0 at first); set_batch binds it first when something else is bound, and splits its planes when
    it has some.  A step without an arena starts bound to its own buffers; an arena step starts unbound (no padded buffer is touched) and
    launch() refuses until a batch is installed.  set_lengths copies into step-owned buffers, use_lengths points at the caller's: neither
    writes through the other's tensors."""

    _teacher = _teacher_rows = _teacher_idx = None      # (teacher=: a stored teacher and the rows of the next launch)

    def __init__(self, flat_params, B, T, dims, weights=DEFAULT_WEIGHTS, lr=1e-4, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=1e-5, seed=0, train=True, sample0=0, bf16=False, share=None, arena=None, ctx=None, planes=None,
                 bits_next=True, distill='rmse', contrast='rnc', contrast_temperature=None, contrast_classes='eq', clip_norm=None,
                 skip_nonfinite=False, freeze=None, lr_scale=None, decay_scale=None, rates=None, ema_decay=None, ema_warmup=False,
                 decoupled_decay=False, regress='mse', regress_delta=1.0, teacher=None):
        """teacher (None = today's step, through the entry it always took): a teacher.TeacherTargets -- distillation targets from a
        STORED teacher.  For every pair it holds a table of (text_hidden, cross_text, fused; losses[3:6]) the target of sample b is
        table row idx[b] instead of stream 0's row b, a constant: stream 0 gets no gradient from that pair -- for `fused` too, the one
        pair self-distillation does not detach.  The loss stage's kernels read the tables through the index vector (a workgroup reads its
        chunk's indices, at most 32, once into LDS): no further launch, nothing on the host per step; tables that hold bit copies of stream 0's rows give the
        default step's bits.  .teacher is settable between launches (a TeacherTargets or None); use_teacher_rows(idx) names the rows
        of the NEXT launches (a device int64 [B] tensor, checked on the host against the tables and their `seen`; None: the tables
        are [B, ...] in batch order).  Combines with distill / regress / contrast, clip_norm / skip_nonfinite (a NaN table row is a
        NaN loss: the guard skips the step), freeze / lr_scale / decay_scale, ema_decay, decoupled_decay and bf16 storage.  A step with
        a teacher is not captured (capture() raises: a graph would replay one index vector's address).
        regress ('mse' = today's step, launch for launch and bit for bit): the criterion of the two regression terms (main :137-138;
        losses[1:3], the seed of the backward): 'l1' (torch.nn.L1Loss), 'huber' (torch.nn.HuberLoss(delta=regress_delta)), both under
        MSELoss's reduction (sum over rows / B), or 'ccc' (1 - the concordance correlation coefficient of the batch, moments in
        double).  Computed by the workgroups of the loss stage that held the MSE terms: no further launch, so it combines with
        everything behind the loss stage (guard, rates, freeze, EMA, AdamW, bf16 storage, capture()).  regress_delta: a positive finite
        number, read by 'huber' alone (anything but 1.0 beside another criterion raises).
        decoupled_decay (False = today's step, launch for launch; a bool): torch.optim.AdamW's decoupled weight decay in place of
        the coupled L2 -- the decoupled form of the step's last launch (sdumc_adamw_step has the rule): every updated parameter is
        first multiplied by fp32(1 - lr * lr_scale_i * weight_decay * decay_scale_i), one fp32 multiply of its own with the factor
        derived on the device from the lr the launch reads (set_lr is followed), then updated as with weight_decay = 0.  Combines
        with clip_norm / skip_nonfinite (a skipped step decays nothing), freeze / lr_scale / decay_scale and ema_decay / ema_warmup.
        A decoupled step is not captured (capture() raises).
        ema_decay (None = today's step, launch for launch) / ema_warmup: averaged weights, an exponential moving average of the
        parameters kept by the step's last launch (Adam's, or the rates launch) at the cost of one more read-and-write stream in it: no
        further launch, nothing on the host per step.  .ema_params is a flat tensor laid out like the parameters (the run's, through
        share, or this step's own), a copy of them at construction; after every update ema <- torch.lerp(ema, params, w), w = fp32(1 -
        fp32(ema_decay)), on params[:live] -- parameters that never get a gradient keep their copy.  ema_warmup=True: the decay is
        min(ema_decay, (1 + t) / (10 + t)), t = the step count after the step (the timm / torch-ema warm-up), derived on the device.
        ema_decay=0: the average holds the parameters' bits.  A step the guard skips leaves the average bit for bit alone; a frozen
        tensor's average is never touched.  load_ema / reset_ema install a saved average / start over.  A step with an average is not
        captured (capture() raises).
        freeze / lr_scale / decay_scale (all None = today's step, launch for launch): per-tensor learning rates, decay and frozen
        tensors -- TensorRates has the patterns and their resolution.  Tensor i is updated with lr * lr_scale_i and coupled L2
        weight_decay * decay_scale_i (set_lr multiplies every tensor alike; lr_scale_i == 0: the parameter stays, the moments
        advance) by ONE launch in Adam's place.  A frozen tensor is torch's requires_grad = False: parameter and both moments stay bit
        for bit, and its segment of .grads is +0.0 to everyone who reads the bucket after the backward -- the guard's norm, the epoch
        record.  frame_dim_reshape_m with weight and bias frozen: that modality's frame dW (at C2 the step's largest GEMM) is not
        computed; every other frozen tensor's gradient is computed and then zeroed.  rates: a TensorRates built before (FusedTrainer
        hands its one to every step) instead of the three.  .rates is the resolved object (None with all off).  A step with rates is
        not captured (capture() raises).
        clip_norm (None or a positive number) / skip_nonfinite: gradient-norm clipping and the non-finite guard, on the device
        between the backward and Adam (sdumc_grad_guard: three launches, no synchronisation).  With either on, .guard is the device
        float[4] the step writes -- the bucket's L2 norm before clipping, the coefficient min(1, clip_norm / (norm + 1e-6)) the
        bucket was scaled by in place (1 without clip_norm), its number of NaN / Inf elements, and 1 when skip_nonfinite skipped the
        step: parameters, moments and step count then stay as they were, the dropout counter advances as for any step.  Both off
        (the default): .guard is None and the step is launch for launch the one without them.  A step with a guard is not
        captured (capture() raises).
        contrast: the contrastive criterion over the [2B, 64] rnc rows (losses[6]): 'rnc' (Rank-N-Contrast, main :140 as it
        stands) or 'supcon' (SupConLoss, loss.py:143-240: the two streams are the two views of a sample, rows L2-normalised in
        the kernel, positives = samples of one class: contrast_classes 'eq' equal labels, 'round' equal rint(label));
        contrast_temperature: None = the criterion's own default (2.0 / 0.07).
        distill: the criterion of the three distillation pairs (text_hidden, cross_text, fused; main :148): 'rmse' (the
        reference's line as it stands), 'cosine' (CosineSimilarityLoss4Seq) or 'kl' (KLLoss); losses[3:6] hold its values.
        share: an object with .params .rng .adam_m .adam_v .hyper .losses (another TrainStep over the SAME flat_params, or
        FusedTrainer's run state) whose optimiser state this step uses instead of allocating its own -- steps of different
        (B, T) shapes then continue one training run.
        arena: a _StepArena sized for the largest batch of the run: workspace, input and output buffers are views into it
        instead of fresh allocations (a C2 step owns ~1.2 GB of workspace: one arena per run, not one per batch shape); the arena
        decides about planes and owns the keep-bits buffer (its shapes change from step to step: use_set / launch(next_step=)).
        planes=True: the batch installed by set_batch is RESIDENT (run many times): its bf16 planes are split once, there (planes_wanted)."""
        Ta, Tt, Tv, T4 = T
        distill_code = _lib.distill_code(distill)
        self.distill = distill
        regress_code, regress_d = _lib.regress_args(regress, regress_delta)
        self.regress, self.regress_delta = regress, regress_d
        self.decoupled_decay = bool(_lib.decoupled_arg(decoupled_decay))
        clip, skip = _lib.guard_args(clip_norm, skip_nonfinite)
        if (clip or skip) and not _lib.GUARD_ABI:
            raise _lib.SdumcError("clip_norm / skip_nonfinite: the library named by SDUMC_LIB is from before sdumc_grad_guard")
        self.clip_norm, self.skip_nonfinite, self.guard = clip_norm, bool(skip), None
        ema_on, ema_d, ema_w = _lib.ema_args(ema_decay, ema_warmup)
        if ema_on and not _lib.EMA_ABI:
            raise _lib.SdumcError("ema_decay: the library named by SDUMC_LIB is from before sdumc_adam_step_ema")
        self.ema_decay, self.ema_warmup = ema_decay, bool(ema_w)
        _lib.contrast_cfg(_lib.StepCfg(), contrast, contrast_temperature, contrast_classes)      # (rejected before any device work)
        self.contrast, self.contrast_temperature, self.contrast_classes = contrast, contrast_temperature, contrast_classes
        self.layout = ParamLayout.get(dims[0], dims[1], dims[2])
        if rates is not None and TensorRates.wanted(lr_scale, decay_scale, freeze):
            raise _lib.SdumcError("rates= is the resolved form of freeze / lr_scale / decay_scale: give one or the other")
        if rates is None and TensorRates.wanted(lr_scale, decay_scale, freeze):
            rates = TensorRates(self.layout, lr_scale, decay_scale, freeze)
        if rates is not None and (not isinstance(rates, TensorRates) or rates.layout is not self.layout):
            raise _lib.SdumcError("rates: a TensorRates over this step's ParamLayout")
        if rates is not None and not _lib.RATES_ABI:
            raise _lib.SdumcError("freeze / lr_scale / decay_scale: the library named by SDUMC_LIB is from before sdumc_adam_step_rates")
        self.rates = rates
        dev = flat_params.device
        _require_cuda(flat_params)
        self.params = flat_params
        from .teacher import teacher_arg
        self._teacher = teacher_arg(teacher, dev, "TrainStep")
        self._teacher_rows = self._teacher_idx = None      # the index tensor (kept alive) / its device address; None: row b
        self.dims = make_dims(B, 2, Ta, Tv, (Tt, T4), dims, train, sample0, bf16=bf16)
        nbytes = lib.sdumc_step_workspace_bytes(C.byref(self.dims))
        if nbytes == 0:
            raise _lib.SdumcError("invalid step dimensions")
        if share is not None and share.params.data_ptr() != flat_params.data_ptr():
            raise _lib.SdumcError("share: both steps must update the same flat parameter buffer")
        self.rng = share.rng if share is not None else RngState(seed, dev)
        V = 2 * B
        self.B, self.V, self.T = B, V, (Ta, Tt, Tv, T4)
        self._fdims = (dims[0], dims[1], dims[2], dims[1])
        fdt = torch.bfloat16 if self.dims.bf16 == 2 else torch.float32      # dtype the features are held in
        self.feature_dtype = fdt
        self._arena = arena
        self._lengths = None      # set_lengths' own [B] int32 buffers, allocated on first use
        io = _lib.NetIO()
        self.io = io
        cfg = _lib.StepCfg()
        self.cfg = cfg
        self._bits_next = None
        if arena is not None:
            if arena.feature_dtype != fdt:
                raise _lib.SdumcError("arena and step disagree on the feature dtype")
            if not arena.fits(B, T, nbytes):
                raise _lib.SdumcError("arena too small for this batch shape")
            self.workspace = arena.workspace
            nbytes = arena.workspace.numel()
            self.vals = arena.outs[0][:V].view(V, 1)
            self.fused = arena.outs[1][:V * H].view(V, H)
            self.rnc = arena.outs[2][:V * RNC_DIM].view(V, RNC_DIM)
            self.text_hidden = arena.outs[3][:V * D].view(V, D)
            self.cross_text = arena.outs[4][:V * NQ * H].view(V, NQ, H)
            # the home is named, not built: (set, planes wanted) -> _Source on first need (_set_source keeps them); nothing is bound yet
            self._home, self._sources = (0, True), {}
            self._bind(None)
            if arena.bits is not None and train:
                io.bits_next, io.bits_next_bytes = ptr(arena.bits), arena.bits.numel()
        else:
            self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            feats = tuple(torch.empty(B, t, d, device=dev, dtype=fdt) for t, d in zip(self.T, self._fdims))
            self.vals = torch.empty(V, 1, device=dev)
            self.fused = torch.empty(V, H, device=dev)
            self.rnc = torch.empty(V, RNC_DIM, device=dev)
            self.text_hidden = torch.empty(V, D, device=dev)
            self.cross_text = torch.empty(V, NQ, H, device=dev)
            # fp32 storage, a RESIDENT batch (planes=True): bf16-plane copies of the four feature tensors, split once by set_batch --
            # 1.5x the features' bytes on top of them
            own_planes = None
            if planes_wanted(planes, dims, bf16):
                own_planes = [_planes_buffer(B * t, d, dev) for t, d in zip(self.T, self._fdims)]
            self._home = _Source(feats, own_planes, None, (0,) * 4, torch.empty(B, device=dev))      # the step's own buffers
            self._bind(self._home)
            # fp32 train steps: a buffer of its own for the NEXT step's keep-bits (generated in this step's idle middle, found at the next
            # step's head under its {seed, call, shape} tag; bit-identical masks) -- not in the workspace: it must survive whatever else
            # runs between two steps of this shape
            nb = lib.sdumc_net_bits_next_bytes(C.byref(self.dims)) if bits_next else 0
            self._bits_next = torch.zeros(nb, dtype=torch.uint8, device=dev) if nb else None
            if self._bits_next is not None:
                io.bits_next = ptr(self._bits_next)
        if share is not None:
            self.adam_m, self.adam_v, self.hyper, self.losses = share.adam_m, share.adam_v, share.hyper, share.losses
        else:
            self.adam_m = torch.zeros(self.layout.live, device=dev)
            self.adam_v = torch.zeros(self.layout.live, device=dev)
            self.hyper = torch.tensor([lr, 0.0, 0.0, 0.0], device=dev)
            self.losses = torch.zeros(8, device=dev)
        io.params, io.rng_state = ptr(flat_params), ptr(self.rng.t)
        io.workspace, io.workspace_bytes = ptr(self.workspace), nbytes
        io.vals, io.fused, io.rnc = ptr(self.vals), ptr(self.fused), ptr(self.rnc)
        io.text_hidden, io.cross_text = ptr(self.text_hidden), ptr(self.cross_text)
        self._ctx = ctx       # ExecContext or None (= the device's default lanes)
        io.ctx = ctx.handle if ctx is not None else None
        for i, w in enumerate(weights):
            cfg.weights[i] = w
        _lib.contrast_cfg(cfg, contrast, contrast_temperature, contrast_classes)      # (temperature: 2.0 unless asked otherwise)
        cfg.beta1, cfg.beta2, cfg.eps, cfg.weight_decay = betas[0], betas[1], eps, weight_decay
        if self.decoupled_decay:
            cfg.decoupled_decay = 1
        cfg.adam_m, cfg.adam_v = ptr(self.adam_m), ptr(self.adam_v)
        cfg.hyper, cfg.losses = ptr(self.hyper), ptr(self.losses)
        cfg.distill = distill_code
        if regress_code:      # (a zeroed pair of fields = MSE: the struct of the default step is written as it always was)
            cfg.regress, cfg.regress_delta = regress_code, regress_d
        if clip or skip:
            # the guard vector and the reduce's scratch: the run's (share.guard, one vector for every shape of a FusedTrainer) or its own
            if getattr(share, "guard", None) is not None:
                self.guard, self.guard_scratch = share.guard, share.guard_scratch
            else:
                self.guard, self.guard_scratch = _guard_buffers(self.layout.live, dev)
            cfg.clip_norm, cfg.skip_nonfinite = clip, skip
            cfg.guard, cfg.guard_scratch = ptr(self.guard), ptr(self.guard_scratch)
        if rates is not None:
            cfg.rates = C.pointer(rates.c)      # (host memory, read during every call: self.rates keeps it alive)
        if ema_on:
            # the run's average (share.ema_params: one tensor for every shape of a FusedTrainer) or its own, a copy of the parameters
            self.ema_params = getattr(share, "ema_params", None)
            if self.ema_params is None:
                self.ema_params = flat_params.clone()
            cfg.ema, cfg.ema_decay, cfg.ema_warmup = ptr(self.ema_params), ema_d, ema_w
        self.graph = None
        goff = lib.sdumc_step_grads_offset(C.byref(self.dims))      # the same for every shape: the bucket leads the workspace
        self.grads = self.workspace[goff:goff + 4 * self.layout.live].view(torch.float32)
        if arena is None:
            self.grads.zero_()      # alignment padding between tensors is never written by the kernels (an arena zeroes it once)

    def _bind(self, src):
        """Installs `src` (a _Source; None = nothing: launch() then refuses) as what the step reads.  The ONLY code that writes the
        label pointer of cfg and the step's .audio .text .video .feat4 .labels; io's pointers are _bind_source's."""
        self._src = src
        self.audio, self.text, self.video, self.feat4 = src.feats if src is not None else _NO4
        self.labels = src.labels if src is not None else None
        _bind_source(self.io, src)
        self.cfg.labels = ptr(self.labels)

    @property
    def _planes(self):
        """the plane tensors the step reads now (None: the bound source has none)"""
        return self._src.planes if self._src is not None else None

    def _set_source(self, k, planes):
        """Arena steps: input set `k` as a source -- its padded buffers viewed at this step's shape, with the set's planes when they
        are wanted and exist.  Built once per (set, planes): set_batch tells by identity whether its home is what is bound."""
        st = self._arena.sets[k]
        key = (k, bool(planes) and st.planes is not None)
        src = self._sources.get(key)
        if src is None:
            B, T, fd = self.B, self.T, self._fdims
            feats = tuple(st.inputs[i][:B * T[i] * fd[i]].view(B, T[i], fd[i]) for i in range(4))
            src = self._sources[key] = _Source(feats, st.planes if key[1] else None, None, (0,) * 4, st.labels[:B])
        return src

    def use_set(self, k, planes=True):
        """Arena steps: read the batch held in input set `k` of the arena (FusedTrainer alternates two sets -- the next batch is
        assembled in the other one while this step runs; bench.py rotates K resident batches).  planes=False: this batch has no
        planes in the set (fresh tensors handed to step(): splitting them for one use costs more than it saves).  Pointers only."""
        if self._arena is None:
            raise _lib.SdumcError("use_set: this step owns its input buffers (no arena)")
        self._home = (k, planes)
        self._bind(self._set_source(k, planes))
        return self

    def use_store(self, store, k):
        """Arena steps in fp32 storage: read the batch IN PLACE from a DeviceFeatureStore(planes=True) through the row maps held in
        input set `k` (written by the store's gather_desc(maps_out=...) launch): the step's feature pointers are the store's packed
        tensors, no padded copy of the batch exists.  Labels / lengths come from the set as with use_set."""
        a = self._arena
        if a is None or store.packed['audio'].dtype != self.feature_dtype \
                or not epoch.in_place(True, self.feature_dtype, a._planes_ok, self._fdims, store):
            raise _lib.SdumcError("use_store: an arena step in fp32 storage with a store that holds planes, or in bf16 storage with a bf16 store")
        self._home = (k, True)
        self._bind(_store_source(store, a.sets[k], a.sets[k].labels[:self.B]))
        return self

    def set_batch(self, audio, text, video, feat4, labels):
        """Copies one batch into the step's writable home (shapes are fixed per TrainStep; the class docstring says what the home
        is), binding it first when the step reads something else; in bf16-storage mode the buffers are bf16 and fp32 inputs are rounded
        by the copy.  With planes (a resident batch) the bf16 planes are split here."""
        home = self._home if self._arena is None else self._set_source(*self._home)
        if self._src is not home:
            self._bind(home)
        for dst, src in zip(home.feats, (audio, text, video, feat4)):
            dst.copy_(src, non_blocking=True)
        home.labels.copy_(labels.reshape(-1), non_blocking=True)
        if home.planes is not None:
            for src, dst in zip(home.feats, home.planes):
                p3_split_into(src, dst)

    def use_batch(self, audio, text, video, feat4, labels):
        """Zero-copy hand-over of one batch: the step reads the caller's device tensors where they are (no 224 MB device copy per
        batch: what `for data in loader: step.use_batch(*unpack(data, 'cuda')[:5]); step.run()` saves over set_batch).  The tensors
        must have the step's shapes and feature dtype, be contiguous and 16-byte aligned, and stay alive and unchanged until the step
        has run (the step keeps references until the next hand-over); labels [B] fp32.  Returns False -- and copies, as set_batch --
        when a tensor does not qualify (fp32 features handed to a bf16-storage step are rounded by the copy).  Not for captured
        steps (a graph replays the addresses it was recorded with)."""
        if self.graph is not None:
            raise _lib.SdumcError("use_batch: the captured hipGraph reads the step's own buffers (set_batch)")
        ts = (audio, text, video, feat4)
        ok = labels.is_cuda and labels.dtype == torch.float32 and labels.is_contiguous() and labels.numel() == self.B
        for t, T, d in zip(ts, self.T, self._fdims):
            ok = ok and t.is_cuda and t.dtype == self.feature_dtype and t.is_contiguous() and tuple(t.shape) == (self.B, T, d) \
                and t.data_ptr() % 16 == 0
        if not ok:
            self.set_batch(audio, text, video, feat4, labels)
            return False
        self._bind(_Source(ts, None, None, (0,) * 4, labels.reshape(-1)))      # (a fresh batch: no planes to split for one use)
        return True

    def set_lengths(self, lengths):
        """Key-padding extension: (audio, text, video, feat4) valid frame counts of the current batch, or None to go back
        to the reference's behaviour (padded frames take part in the softmax)."""
        new = _lengths_arg(lengths, self.B, 4, self.params.device)
        on = self.io.lengths[0] is not None
        if self.graph is not None and (new is None) == on:
            raise _lib.SdumcError("the captured hipGraph was recorded with the key-padding extension "
                                  + ("on" if on else "off") + ": switch it before capture()")
        self._lengths = _copy_lengths(self.io, self._lengths, new, self.B)

    def use_lengths(self, tensors):
        """Arena steps: the key-padding lengths as four device int32 buffers the batch's assembly already filled (or None = off).
        Pointers only: the step never writes these."""
        for i in range(4):
            self.io.lengths[i] = ptr(tensors[i]) if tensors is not None else None

    def set_lr(self, lr):
        self.hyper[0] = lr

    @property
    def teacher(self):
        """the teacher.TeacherTargets the next launch reads its distillation targets from; None: stream 0, as always"""
        return self._teacher

    @teacher.setter
    def teacher(self, targets):
        from .teacher import teacher_arg
        targets = teacher_arg(targets, self.params.device, "TrainStep.teacher")
        if self.graph is not None and targets is not None and targets.active:
            raise _lib.SdumcError("teacher: the captured hipGraph was recorded without one")
        self._teacher = targets
        self._teacher_rows = self._teacher_idx = None      # (rows named for another table are not carried over)

    def use_teacher_rows(self, idx):
        """The rows of the teacher's tables the NEXT launches read: a device int64 [B] tensor (row idx[b] is the target of sample b),
        or None (row b: the tables are [B, ...] in batch order).  Checked on the host -- range and the teacher's `seen` -- before
        anything is enqueued; the step keeps the tensor alive."""
        t = self._teacher
        if idx is None or t is None or not t.active:
            self._teacher_rows = self._teacher_idx = None
            return self
        if not (torch.is_tensor(idx) and idx.dtype == torch.int64 and idx.device == self.params.device and idx.is_contiguous()
                and idx.numel() == self.B):
            raise _lib.SdumcError(f"use_teacher_rows: a contiguous int64 [{self.B}] tensor on {self.params.device}, or None")
        t.check_rows(idx, "use_teacher_rows")
        self._teacher_rows, self._teacher_idx = idx, idx.data_ptr()
        return self

    def _use_teacher_ptr(self, targets, idx_ptr):
        """FusedTrainer's launches: the run's teacher and the device address of this batch's index vector (both checked by the
        trainer, once per epoch or batch, against the tables; the trainer keeps the indices alive)"""
        self._teacher, self._teacher_rows, self._teacher_idx = targets, None, idx_ptr

    def _step_entry(self):
        """(entry, its arguments behind dims and io, its name): sdumc_train_step, or with a teacher that holds a table
        sdumc_train_step_teacher and this launch's record"""
        t = self._teacher
        if t is None or not t.active:
            return lib.sdumc_train_step, (C.byref(self.cfg),), "sdumc_train_step"
        if self._teacher_idx is None:
            t.check_batch(self.B, "launch")
        self._teacher_rec = t.record(self._teacher_idx)      # (host memory, read during the call)
        return lib.sdumc_train_step_teacher, (C.byref(self.cfg), C.byref(self._teacher_rec)), "sdumc_train_step_teacher"

    def launch(self, stream=None, next_step=None, prefetch=None, pregen=True):
        """Enqueues the step.  next_step: the TrainStep that runs NEXT in this arena (its dims decide how this step's middle lays out
        the next keep-bits set); prefetch: the sdumc_gather_batch descriptor of the next batch, issued by the step beside its middle
        and backward; pregen=False: no keep-bits for a next step this time (the caller does not expect a step of a known shape to follow)."""
        if self._src is None:
            raise _lib.SdumcError("launch: no batch is installed (set_batch, use_set, use_store or use_batch first)")
        st = _lib.current_stream() if stream is None else stream
        entry, args, name = self._step_entry()      # (what a teacher's host checks refuse: before any field of io is touched)
        io = self.io
        a = self._arena
        shared = a is not None and a.bits is not None and io.bits_next
        if shared:
            io.bits_phase = a.bits_phase
        saved = io.bits_next
        if not pregen and self.graph is None:
            io.bits_next = None
        io.bits_next_dims = C.addressof(next_step.dims) if next_step is not None else None
        io.prefetch_workgroups = a.prefetch_workgroups if a is not None else 0
        try:
            check(epoch.with_prefetch(io, prefetch, entry, C.byref(self.dims), C.byref(io), *args, st), name)
        finally:
            io.bits_next, io.bits_next_dims = saved, None
        if pregen or self.graph is not None:
            if shared:
                a.bits_phase ^= 1
            else:
                io.bits_phase ^= 1      # (the next step reads the keep-bits set this one filled in its middle: sdumc_net_io.bits_next)

    def capture(self):
        """Capture one step into a hipGraph; run() then replays it.  For embedding the step in a captured region, not for speed:
        the capture records a plain three-lane fork/join (no background lane, chain.hip instead of the clustered kernels) and
        measured slower than the eager four-lane launches, which are the production path."""
        if self.guard is not None:
            raise _lib.SdumcError("capture: a step with clip_norm / skip_nonfinite is not captured (not built)")
        if self.rates is not None:
            raise _lib.SdumcError("capture: a step with freeze / lr_scale / decay_scale is not captured (not built)")
        if self.ema_params is not None:
            raise _lib.SdumcError("capture: a step with ema_decay is not captured (not built)")
        if self.decoupled_decay:
            raise _lib.SdumcError("capture: a step with decoupled_decay is not captured (not built)")
        if self._teacher is not None and self._teacher.active:
            raise _lib.SdumcError("capture: a step with a teacher is not captured (not built)")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        # the capture itself does not execute; state (params, Adam, rng) is untouched by it
        self.io.bits_next = None      # (a replayed graph cannot alternate the two keep-bits sets: every replay generates its own)
        with torch.cuda.graph(g, stream=s):
            self.launch()
        self.graph = g

    def run(self):
        if self.graph is not None:
            self.graph.replay()
        else:
            self.launch()
        return self.losses


class _RunState(_OptStateMixin):
    """Optimiser state of one training run, shared by the per-shape TrainSteps of a FusedTrainer (and by the per-shape
    backends of trainer.DataParallelStep)."""

    def __init__(self, flat_params, live, lr, seed):
        dev = flat_params.device
        self.params = flat_params
        self.rng = RngState(seed, dev)
        self.adam_m = torch.zeros(live, device=dev)
        self.adam_v = torch.zeros(live, device=dev)
        self.hyper = torch.tensor([lr, 0.0, 0.0, 0.0], device=dev)
        self.losses = torch.zeros(8, device=dev)


class _InputSet:
    """One resident batch slot of an arena: the four feature buffers (flat, capacity-sized), their P3 planes (fp32 storage, planes on),
    the labels and the valid frame counts."""

    def __init__(self, n, B, dtype, dev, rows):
        self._n, self._dtype, self._inputs = n, dtype, None      # (the padded copies' buffers exist only once something is copied)
        self.planes = None    # (_StepArena.ensure_planes)
        self.labels = torch.empty(B, device=dev)
        self.lengths = [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(4)]
        self.maps = None      # row maps (int32 per frame): a batch read in place from a DeviceFeatureStore (ensure_maps)
        self._rows = rows

    @property
    def inputs(self):
        if self._inputs is None:
            self._inputs = [torch.empty(k, device=self.labels.device, dtype=self._dtype) for k in self._n]
        return self._inputs

    def ensure_maps(self):
        if self.maps is None:
            # (+ 64 entries: the bf16 weight-gradient kernel fetches map entries four at a time, past a batch's last row)
            self.maps = [torch.zeros(r + 64, dtype=torch.int32, device=self.labels.device) for r in self._rows]
        return self.maps


class _Arena:
    """Device memory of epochs over a store, sized for the largest batch (B, (T_audio, T_text, T_video, T_feat4)) seen so far: the
    workspace, the five [2 B, w] outputs, and `sets` input sets the batches are assembled in (row maps, labels, lengths; padded input
    buffers and planes only once a batch is gathered) -- two sets let the NEXT batch be assembled while a call runs."""

    def __init__(self, dev, B, T, fdims, dtype, nbytes, sets=2):
        self.B, self.T = int(B), tuple(int(t) for t in T)
        self._fdims = tuple(fdims)
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.outs = [torch.empty(2 * self.B * w, device=dev) for w in epoch.OUT_WIDTHS]
        rows = [self.B * t for t in self.T]
        self.sets = [_InputSet([r * d for r, d in zip(rows, self._fdims)], self.B, dtype, dev, rows) for _ in range(max(1, int(sets)))]

    @property
    def nbytes(self):
        """the byte sizes of the buffers that grow with the batch shape beside the sets: what fits takes after (B, T)"""
        return (self.workspace.numel(),)

    def fits(self, B, T, nbytes=0):
        return B <= self.B and all(t <= c for t, c in zip(T, self.T)) and nbytes <= self.workspace.numel()

    def ensure_planes(self):
        """The plane buffers of every input set (1.5x the fp32 input bytes each), allocated on first need"""
        for st in self.sets:
            if st.planes is None:
                st.planes = [_planes_buffer(r, d, self.workspace.device) for r, d in zip(st._rows, self._fdims)]
        return True


class _StepArena(_Arena):
    """Device memory of one training run, sized once for its largest batch: an _Arena over the step workspace (whose leading gradient
    bucket is zeroed here, once) -- DeviceFeatureStore gathers straight into its input sets --, and (fp32 train steps) the two keep-bits
    sets every shape of the run shares (their tags name the shape they were laid out for)."""

    def __init__(self, flat_params, B, T, dims, bf16=False, sets=1, planes=False, bits_next=True, prefetch_workgroups=0):
        self.dims = tuple(dims)
        d = make_dims(int(B), 2, int(T[0]), int(T[2]), (int(T[1]), int(T[3])), dims, True, 0, bf16=bf16)
        nbytes = lib.sdumc_step_workspace_bytes(C.byref(d))
        if nbytes == 0:
            raise _lib.SdumcError("invalid arena dimensions")
        self.feature_dtype = torch.bfloat16 if d.bf16 == 2 else torch.float32
        super().__init__(flat_params.device, B, T, (dims[0], dims[1], dims[2], dims[1]), self.feature_dtype, nbytes, sets)
        goff = lib.sdumc_step_grads_offset(C.byref(d))
        self.workspace[goff:goff + 4 * ParamLayout.get(dims[0], dims[1], dims[2]).live].zero_()
        # planes: True = the input sets carry P3 planes from the start; None = as soon as a store with planes (or a resident batch)
        # asks for them (ensure_planes); False = never
        self._planes_ok = planes is not False and planes_wanted(True, dims, bf16)
        if planes is True:
            self.ensure_planes()
        nb = lib.sdumc_net_bits_next_bytes(C.byref(d)) if bits_next else 0
        self.bits = torch.zeros(nb, dtype=torch.uint8, device=flat_params.device) if nb else None
        self.bits_phase = 0
        self.prefetch_workgroups = int(prefetch_workgroups)

    def ensure_planes(self):
        """False when the arena's mode has no planes (bf16 storage, widths that are not whole k-tiles, planes=False)"""
        return self._planes_ok and super().ensure_planes()


StepArena = _StepArena      # (public name: bench.py and callers that rotate resident batches build one directly)


class FusedTrainer:
    """The fused step for the reference's REAL batches, whose (B, T_audio, T_text, T_video, T_feat4) change from batch to
    batch (every modality is padded to its batch maximum, read_data.py:223-248; the last batch of an epoch is short):
    one TrainStep per shape, created on first use, all sharing one optimiser state, so `step()` over a data loader is one
    continuous run of main_frame_val_text_missing.py:119-150.  At most `max_cached` shapes keep their workspace (least
    recently used first out); a shape seen again after eviction is simply rebuilt.  `step()` hands each batch over zero-copy
    (TrainStep.use_batch), holds the caller's tensors itself in one slot until the next `step()`, and unbinds the per-shape step after the
    launch: a cached step keeps no batch alive, and a stray launch() on it raises instead of reading freed memory.

    With capacity= and a DeviceFeatureStore, `run_epoch` is the replacement for the reference's loop over its DataLoader
    (main :89-109 over feat_data.py:232-253): the epoch's index vectors are uploaded once, every batch is assembled on the device
    straight into one of the arena's two input sets -- by the PREVIOUS step, beside its latency-bound middle and its backward
    (sdumc_net_io.prefetch) -- and every step tells the engine the next batch's shape, so that the next keep-bits are laid out for it."""

    guard = None      # with clip_norm / skip_nonfinite: the run's device float[4] every step writes (sdumc_grad_guard)
    teacher = None    # a teacher.TeacherTargets: the stored teacher every step reads its distillation targets from (set_teacher)

    def __init__(self, flat_params, dims, max_cached=8, lr=1e-4, seed=0, capacity=None, planes=None, sets=2, prefetch_workgroups=0,
                 inplace=True, distill='rmse', contrast='rnc', contrast_temperature=None, contrast_classes='eq', clip_norm=None,
                 skip_nonfinite=False, freeze=None, lr_scale=None, decay_scale=None, ema_decay=None, ema_warmup=False,
                 decoupled_decay=False, regress='mse', regress_delta=1.0, teacher=None, **step_kwargs):
        """teacher: a teacher.TeacherTargets (or None; set_teacher changes it between launches, refresh_teacher installs the eval-mode
        embeddings of the run's own parameters or averaged weights) -- distillation targets from a stored teacher in every step
        (TrainStep has the semantics).  The tables are in STORE order: step_from_store / run_epoch / train_epoch hand step i the index
        vector of batch i; step(..., teacher_rows=) takes the rows of a batch the caller brings.  Read at every launch: a cached
        step never runs with a table that is no longer the trainer's.
        distill: 'rmse' | 'cosine' | 'kl', the distillation criterion of every step of this trainer (TrainStep).
        regress: 'mse' | 'l1' | 'huber' | 'ccc' with regress_delta, the regression criterion of every step (TrainStep); columns 1-2 of
        train_epoch's record hold its values.
        decoupled_decay (a bool): torch.optim.AdamW's decoupled weight decay in every step of the run (TrainStep has the rule).
        ema_decay / ema_warmup: averaged weights (TrainStep has the rule): .ema_params is the run's ONE average, a flat tensor laid out
        like the parameters that every step updates whatever its shape (None when off); eval_epoch / saliency_epoch(weights='ema')
        read it, load_ema / reset_ema install a saved one / start over.  The average is not part of train_epoch's record.
        freeze / lr_scale / decay_scale: per-tensor learning rates, decay and frozen tensors of every step (TrainStep, TensorRates):
        resolved once, here; .rates is the ONE TensorRates every step of the run reads (None with all three off).
        clip_norm / skip_nonfinite: gradient-norm clipping and the non-finite guard of every step (TrainStep); .guard is the run's
        ONE device float[4] {norm, coefficient, non-finite count, skipped}, rewritten by every step whatever its shape (None with
        both off); train_epoch keeps a copy per step.
        contrast: 'rnc' | 'supcon', contrast_temperature, contrast_classes: its contrastive criterion (TrainStep).
        capacity = (B_max, (T_audio, T_text, T_video, T_feat4) maxima) of the run: ONE arena then backs every batch shape
        (no per-shape workspace, the per-shape step is a few ctypes structs and tensor views: cache as many as you like) and
        `step_from_store` / `run_epoch` assemble batches straight into it.  Without it every cached shape owns its workspace.
        planes (arena only): None (default) = follow the store -- batches assembled from a DeviceFeatureStore(planes=True) bring their
        P3 planes along (the same gather as the fp32 rows) and the step's frame projections read them; False = never.
        inplace (default True): with such a store the batches are not gathered at all -- the step reads the store's packed tensors
        through per-batch row maps (4 bytes per frame; sdumc_net_io.row_map)."""
        _lib.distill_code(distill)
        self.distill = distill
        self.regress = (regress, _lib.regress_args(regress, regress_delta)[1])
        self.decoupled_decay = bool(_lib.decoupled_arg(decoupled_decay))
        clip, skip = _lib.guard_args(clip_norm, skip_nonfinite)
        ema_on = _lib.ema_args(ema_decay, ema_warmup)[0]
        if ema_on and not _lib.EMA_ABI:
            raise _lib.SdumcError("ema_decay: the library named by SDUMC_LIB is from before sdumc_adam_step_ema")
        _lib.contrast_cfg(_lib.StepCfg(), contrast, contrast_temperature, contrast_classes)
        self.contrast = (contrast, contrast_temperature, contrast_classes)
        _require_cuda(flat_params)
        self.params, self.dims, self.max_cached = flat_params, tuple(dims), max(1, int(max_cached))
        self.teacher = None
        self.set_teacher(teacher)
        self._teacher_res = None      # refresh_teacher's result, kept and reused
        self.kw = dict(step_kwargs, lr=lr, seed=seed, distill=distill, contrast=contrast, contrast_temperature=contrast_temperature,
                       contrast_classes=contrast_classes, clip_norm=clip_norm, skip_nonfinite=skip_nonfinite)
        if ema_on:      # (off: the steps are built with the keywords they always were)
            self.kw.update(ema_decay=ema_decay, ema_warmup=ema_warmup)
        if self.decoupled_decay:
            self.kw.update(decoupled_decay=True)
        if regress != 'mse':
            self.kw.update(regress=regress, regress_delta=regress_delta)
        lay = ParamLayout.get(dims[0], dims[1], dims[2])
        self.rates = TensorRates(lay, lr_scale, decay_scale, freeze) if TensorRates.wanted(lr_scale, decay_scale, freeze) else None
        if self.rates is not None and not _lib.RATES_ABI:
            raise _lib.SdumcError("freeze / lr_scale / decay_scale: the library named by SDUMC_LIB is from before sdumc_adam_step_rates")
        self.kw["rates"] = self.rates
        self.state = _RunState(flat_params, lay.live, lr, seed)     # (params, rng, adam_m, adam_v, hyper, losses)
        self.guard = None
        if clip or skip:
            self.guard, self.state.guard_scratch = _guard_buffers(lay.live, flat_params.device)
        self.state.guard = self.guard
        if ema_on:
            self.state.ema_params = flat_params.clone()      # the average starts as a copy: no bias correction exists
        self._steps = {}          # shape -> TrainStep, insertion order = recency
        self.arena = None
        self._arena_kw = dict(bf16=step_kwargs.get("bf16", False), sets=sets, planes=planes,
                              bits_next=step_kwargs.get("bits_next", True), prefetch_workgroups=prefetch_workgroups)
        self._last_shape = None
        self._batch = None        # the caller's tensors of step()'s zero-copy hand-over, until the next step()
        # inplace (fp32 storage, a store with planes): batches are read from the store through row maps, no padded copy (use_store);
        # False: every batch is gathered into the arena's input sets (fp32 rows + plane rows)
        self.inplace = bool(inplace)
        if capacity is not None:
            self.arena = _StepArena(flat_params, capacity[0], capacity[1], dims, **self._arena_kw)
            self.max_cached = max(self.max_cached, 4096)
        else:
            # per-shape steps own their buffers and see a fresh batch per step: no planes to re-split, and no keep-bits set kept per
            # shape (the next step is usually another shape with another buffer: its tag would never match)
            self.kw.update(planes=False, bits_next=False)

    def _get(self, B, T):
        # the criteria are part of the key: one cache never mixes them
        key = (B,) + tuple(T) + self.regress + self.contrast + (self.distill,)
        ts = self._steps.pop(key, None)
        if ts is None:
            while len(self._steps) >= self.max_cached:
                del self._steps[next(iter(self._steps))]
            self._fit_arena(B, T)
            kw = {k: v for k, v in self.kw.items() if not (self.arena is not None and k in ("planes", "bits_next"))}
            ts = TrainStep(self.params, B, T, self.dims, share=self.state, arena=self.arena, **kw)
        self._steps[key] = ts
        return ts

    def _fit_arena(self, B, T):
        """a batch beyond the arena's capacity: a larger arena takes its place (every cached step pointed into the old one: they go)"""
        a = self.arena
        if a is None or a.fits(B, T):
            return
        self.arena = _StepArena(self.params, max(B, a.B), tuple(max(t, c) for t, c in zip(T, a.T)), self.dims, **self._arena_kw)
        self._steps.clear()

    def set_lr(self, lr):
        self.state.hyper[0] = lr

    def load_optimizer_state(self, adam_m, adam_v, step):
        self.state.load_optimizer_state(adam_m, adam_v, step)

    def optimizer_state(self):
        return self.state.optimizer_state()

    @property
    def ema_params(self):
        """the run's averaged weights (ema_decay=): a flat tensor laid out like the parameters; None when off"""
        return self.state.ema_params

    def load_ema(self, flat):
        self.state.load_ema(flat)

    def reset_ema(self):
        self.state.reset_ema()

    def _weights(self, weights, what):
        """the flat tensor eval_epoch / saliency_epoch(weights=) read: 'params' the trainer's parameters, 'ema' its averaged weights"""
        if weights == "params":
            return self.params
        if weights != "ema":
            raise _lib.SdumcError(f"{what}: weights must be 'params' or 'ema', not {weights!r}")
        if self.ema_params is None:
            raise _lib.SdumcError(f"{what}: weights='ema' on a trainer without averaged weights (ema_decay=)")
        return self.ema_params

    def set_teacher(self, targets):
        """The stored teacher of every step from now on (a teacher.TeacherTargets), or None: self-distillation"""
        from .teacher import teacher_arg
        self.teacher = teacher_arg(targets, self.params.device, "FusedTrainer")

    def _teacher_on(self):
        return self.teacher is not None and self.teacher.active

    def _check_teacher_epoch(self, store, indices):
        """an epoch's indices against the teacher's tables, on the host, before anything is enqueued"""
        self.teacher.check_store(len(store), "epoch")
        self.teacher.check_rows(indices, "epoch")

    def refresh_teacher(self, store, batches, weights="params", key_padding=False, stream="full", pairs=("text_hidden", "cross_text", "fused")):
        """One evaluation pass (eval_epoch(embeddings=True), into a result the trainer keeps and reuses) over `batches` of `store`
        with the trainer's parameters, or with weights='ema' its averaged weights, whose embeddings of `stream` ('full' | 'missing')
        become the teacher's tables for `pairs` -> the EvalResult.  Between epochs with weights='ema': a mean teacher at epoch
        granularity.  Utterances the pass did not visit hold NaN: an epoch that names one is refused on the host."""
        from .teacher import TeacherTargets
        out = self._teacher_res
        if out is not None and not out.fits(len(store), self.params.device, True):
            out = None
        res = self.eval_epoch(store, batches, key_padding=key_padding, embeddings=True, out=out, weights=weights)
        self._teacher_res = res
        self.set_teacher(TeacherTargets.from_eval(res, stream, pairs))
        return res

    def _launch(self, ts, next_step=None, prefetch=None, teacher_idx=None):
        # keep-bits for a next step only when its shape is known (run_epoch) or has been repeating (a static-shape loader)
        ts._use_teacher_ptr(self.teacher, teacher_idx)
        key = (ts.B,) + ts.T
        pregen = next_step is not None or key == self._last_shape
        self._last_shape = key
        ts.launch(next_step=next_step, prefetch=prefetch, pregen=pregen)
        return ts.losses

    def _store_planes(self, store):
        return store.packed_p3 is not None and self.arena.ensure_planes()

    def _in_place(self, store):
        """fp32 storage and a store with planes, or bf16 storage and a bf16 store (widths in whole 128-element tiles): batches are not
        copied at all -- the step reads the store's packed tensors through row maps."""
        return epoch.in_place(self.inplace, self.arena.feature_dtype, self.arena._planes_ok, self.dims, store)

    def step_from_store(self, store, indices, key_padding=False):
        """One optimisation step on the batch `indices` of a data.DeviceFeatureStore: the padded batch is assembled by the
        gather/pad kernel DIRECTLY in the step's input buffers (no intermediate batch tensors, no 224 MB device copy);
        key_padding=True also hands the valid frame counts to the kernels (extension, default off = the reference).
        (One batch at a time: the assembly runs in front of the step.  run_epoch overlaps it with the previous step.)"""
        if self.arena is None:
            raise _lib.SdumcError("step_from_store needs FusedTrainer(capacity=...)")
        B, T = store.batch_shape(indices)
        teacher_idx = None
        if self._teacher_on():      # (refused here, before the batch's assembly is enqueued)
            self.teacher.check_store(len(store), "step_from_store")
            self._keep_rows = self.teacher.check_rows(indices, "step_from_store").to(self.params.device)
            teacher_idx = self._keep_rows.data_ptr()
        ts = self._get(B, T)
        st = self.arena.sets[0]
        if self._in_place(store):
            # (one upload of the batch's indices: the row maps' gather and the teacher read the same vector)
            idx_d = self._keep_rows if teacher_idx is not None else store._checked(indices).to(store.device, non_blocking=True)
            g = epoch.gather_desc(store, idx_d.data_ptr(), B, T, st, key_padding, True, True)
            check(lib.sdumc_gather_batch(C.byref(g), 0, _lib.current_stream()), "sdumc_gather_batch")
            self._keep_idx = idx_d
            ts.use_store(store, 0)
        else:
            planes = self._store_planes(store)
            ts.use_set(0, planes=planes)
            store.batch_into(indices, (ts.audio, ts.text, ts.video, ts.feat4), ts.labels, st.lengths if key_padding else None,
                             st.planes if planes else None)
        ts.use_lengths(st.lengths if key_padding else None)
        return self._launch(ts, teacher_idx=teacher_idx)

    def run_epoch(self, store, batches, key_padding=False, on_step=None):
        """Every batch of `batches` (index vectors into `store`, or a data.EpochPlan), in order: main :89-150's loop.  The first batch
        is assembled in front of the first step; from then on step i assembles batch i + 1 in the other input set while it runs.
        on_step(i, losses) is called after step i has been ENQUEUED (losses = the device vector the step will write: clone it to keep
        it).  Returns the number of steps.  (train_epoch is the same loop with the epoch's record kept.)"""
        self._need_sets("run_epoch")
        from .data import EpochPlan
        return self._epoch(store, batches if isinstance(batches, EpochPlan) else store.plan_epoch(batches), key_padding, on_step)

    def _need_sets(self, what):
        if self.arena is None or len(self.arena.sets) < 2:
            raise _lib.SdumcError(f"{what} needs FusedTrainer(capacity=..., sets=2)")

    def _epoch(self, store, plan, key_padding, on_step, record=None, teacher_checked=False):
        """The loop of run_epoch and train_epoch over a data.EpochPlan.  record(i, ts) is called right after step i has been enqueued
        (ts = the step that ran it), before on_step.  teacher_checked: the caller has held the epoch's indices against the teacher."""
        # the arena must hold the epoch's largest batch BEFORE the first descriptor is built (growing it invalidates every cached step)
        launch = self._launch
        if self._teacher_on():
            # the epoch's indices against the tables, once, on the host; then step i reads ITS batch's index vector (the same step
            # prefetches batch i + 1 through another pointer)
            if not teacher_checked:
                self._check_teacher_epoch(store, plan.idx_h if getattr(plan, "idx_h", None) is not None else plan.idx_d)
            batch_no = iter(range(len(plan)))

            def launch(ts, nxt, pf):
                return self._launch(ts, nxt, pf, plan.idx_ptr(next(batch_no)))
        self._fit_arena(max(B for B, _ in plan.shapes), tuple(max(T[i] for _, T in plan.shapes) for i in range(4)))
        sets, inplace = self.arena.sets, self._in_place(store)
        planes = inplace or self._store_planes(store)

        def bind(ts, k):
            ts = ts.use_store(store, k) if inplace else ts.use_set(k, planes=planes)
            ts.use_lengths(sets[k].lengths if key_padding else None)
            return ts

        def both(i, ts):
            if record is not None:
                record(i, ts)
            on_step(i, ts.losses)

        return epoch.run(self, store, plan, sets, key_padding, planes, inplace, self._get, bind, launch,
                         record if on_step is None else both)

    def train_epoch(self, store, batches, key_padding=False, on_step=None, embeddings=False, grad_norm=False, out=None, by_tensor=False):
        """run_epoch with the epoch's record kept -> record.TrainRecord: what the reference's training pass returns (main :156-178: the
        train-mode predictions of both streams in store order and their MSE; embeddings=True: the four embeddings too) and a log row
        per step (the loss vector, B, the learning rate; grad_norm=True: the L2 norm of the step's raw gradient bucket -- without
        Adam's coupled L2 term -- and its number of non-finite elements).  The same launches as run_epoch plus one per step, two with
        grad_norm (sdumc_epoch_record), which only read what the step left: parameters, moments and dropout counter are those of run_epoch.
        The epoch must not visit an utterance twice (checked on the host before anything is enqueued; `out` is untouched if it
        does).  out= reuses a record (TrainRecord.fits: this store, at least this many steps, the same options).
        by_tensor=True: one more call per step (sdumc_tensor_norms, two launches) cuts the same raw bucket at ParamLayout's offsets ->
        rec.by_tensor (record.TensorNorms): every live tensor's gradient norm and non-finite count per step.  by_tensor='updates': a
        second such call over the flat parameters against a snapshot the record owns (one device copy in front of the first step) adds
        each tensor's weight norm after the step and the norm of the step's actual update.  Both only read what the step left.
        A trainer with clip_norm / skip_nonfinite: rec.guard [steps, 4] keeps every step's guard vector (one asynchronous device copy
        per step; rec.skipped_steps()).  The record reads the bucket as the step LEFT it: with clipping on, the log's grad_norm column
        and the record by tensor see the gradients AFTER scaling -- rec.guard[:, 0] is the norm before.  A skipped step's bucket is
        unscaled, its non-finite elements are counted by both."""
        self._need_sets("train_epoch")
        from .record import NormTable, TrainRecord, by_tensor_mode
        by_tensor = by_tensor_mode(by_tensor)
        dev, n_store = self.params.device, len(store)
        plan, batches = epoch.checked_plan(batches, n_store)
        if self._teacher_on():      # (before the record is made or reset)
            host = torch.cat(batches) if plan is None else (plan.idx_h if getattr(plan, "idx_h", None) is not None else plan.idx_d)
            self._check_teacher_epoch(store, host)
        n = len(plan if plan is not None else batches)
        lay = ParamLayout.get(*self.dims[:3])
        n_grads = lay.live if grad_norm else 0
        guard = self.guard is not None
        if out is not None and not (isinstance(out, TrainRecord) and out.fits(n_store, n, dev, embeddings, n_grads, by_tensor, lay, guard)):
            raise _lib.SdumcError("train_epoch: out= is not a record of this store's size and device, these many steps and these options")
        if plan is None:
            plan = store.plan_epoch(batches)
        rec = (out if out is not None else TrainRecord.empty(n_store, n, dev, embeddings, n_grads, by_tensor, lay, guard)).reset()
        descs, st = {}, _lib.current_stream()
        bt, tables = rec.by_tensor, {}
        if by_tensor == "updates":
            # the snapshot: the view of the record's buffer that sits like the parameters within 16 bytes (16-byte loads of both),
            # filled once here; every step's call then rolls it forward itself
            k = ((self.params.data_ptr() - bt.snapshot.data_ptr()) >> 2) & 3
            snap = bt.snapshot[k:k + lay.live]
            snap.copy_(self.params[:lay.live])
            base = self.params.data_ptr()
            tables["params"] = NormTable((base + 4 * o, snap.data_ptr() + 4 * o, c) for o, c in zip(bt.offsets, bt.counts))

        def record_by_tensor(i, ts):
            g = ts.grads.data_ptr()
            tb = tables.get(g)      # (one bucket per arena: a table per address it has had)
            if tb is None:
                tb = tables[g] = NormTable((g + 4 * o, None, c) for o, c in zip(bt.offsets, bt.counts))
            row = 4 * len(bt.names) * i
            tb.launch(bt.grad_norm.data_ptr() + row, bt.grad_nonfinite.data_ptr() + row, 0, bt.scratch, st)
            if by_tensor == "updates":
                tables["params"].launch(bt.param_norm.data_ptr() + row, bt.param_nonfinite.data_ptr() + row,
                                        bt.update_norm.data_ptr() + row, bt.scratch, st)

        def record(i, ts):
            d = descs.get(ts.B)
            if d is None or d[1] is not self.arena:
                d = descs[ts.B] = (self._record_desc(rec, ts, embeddings, grad_norm), self.arena)
            r = d[0]
            r.idx, r.log_row = plan.idx_ptr(i), rec.log.data_ptr() + 4 * _lib.LOG_COLS * i
            check(lib.sdumc_epoch_record(C.byref(r), st), "sdumc_epoch_record")
            if by_tensor:
                record_by_tensor(i, ts)
            if guard:
                rec.guard[i].copy_(self.guard, non_blocking=True)

        rec.steps = self._epoch(store, plan, key_padding, on_step, record, teacher_checked=True)
        return rec

    def _record_desc(self, rec, ts, embeddings, grad_norm):
        """sdumc_epoch_record's descriptor for steps of ts.B samples (idx and log_row are set per step): rows [0, B) of the arena's
        outputs to stream 0's tensors of the record, rows [B, 2 B) to stream 1's"""
        r = _lib.EpochRec()
        for k, sg in enumerate(epoch.scatter_segments(self.arena.outs, rec, ts.B, embeddings)):
            r.seg[k] = sg
        r.nseg, r.B, r.mark = k + 1, ts.B, ptr(rec.seen)
        r.losses, r.hyper = ptr(self.state.losses), ptr(self.state.hyper)
        if grad_norm:
            r.grads, r.n_grads, r.scratch = ptr(ts.grads), ts.grads.numel(), ptr(rec.scratch)
        return r

    def eval_epoch(self, store, batches, key_padding=False, embeddings=False, out=None, attention=False, weights="params"):
        """One evaluation pass (main :151-166: both streams, eval mode) over `batches` of `store` with the trainer's parameters, in its
        storage mode and with its inplace / planes choices -> evaluate.EvalResult in store order.  Evaluation owns its memory
        (evaluate.Evaluator, made on first use and kept): it touches nothing of the training run but reads the parameters.
        attention=True also keeps the per-frame attention maps (EvalResult.attention; evaluate.eval_epoch has the semantics).
        weights='ema': the same pass over the averaged weights (ema_decay=), through a second Evaluator made on first use and kept; it
        reads the average as it is when the call runs."""
        flat = self._weights(weights, "eval_epoch")
        attr = "_evaluator" if weights == "params" else "_evaluator_ema"
        if getattr(self, attr, None) is None:
            from .evaluate import Evaluator
            kw = self._arena_kw
            setattr(self, attr, Evaluator(flat, self.dims, bf16=kw["bf16"], inplace=self.inplace, planes=kw["planes"],
                                          prefetch_workgroups=kw["prefetch_workgroups"]))
        return getattr(self, attr).eval_epoch(store, batches, key_padding=key_padding, embeddings=embeddings, out=out, attention=attention)

    def saliency_epoch(self, store, batches, key_padding=False, streams=("full", "missing"), out=None, weights="params"):
        """One saliency pass (saliency.saliency_epoch has the semantics) over `batches` of `store` with the trainer's parameters and its
        inplace / planes choices -> saliency.SaliencyResult in store order: per stream and modality the gradient x input and the gradient
        norm of the eval-mode prediction per frame.  Like eval_epoch it owns its memory (saliency.Saliency, made on first use and
        kept) and only reads the parameters.  fp32 storage only: a bf16-storage trainer raises.
        weights='ema': the same pass over the averaged weights (ema_decay=), through a second Saliency made on first use and kept."""
        flat = self._weights(weights, "saliency_epoch")
        attr = "_saliency" if weights == "params" else "_saliency_ema"
        if getattr(self, attr, None) is None:
            from .saliency import Saliency
            kw = self._arena_kw
            setattr(self, attr, Saliency(flat, self.dims, bf16=kw["bf16"], inplace=self.inplace, planes=kw["planes"],
                                         prefetch_workgroups=kw["prefetch_workgroups"]))
        return getattr(self, attr).saliency_epoch(store, batches, key_padding=key_padding, streams=streams, out=out)

    def step(self, audio, text, video, feat4, labels, lengths=None, teacher_rows=None):
        """One optimisation step on one batch of any shape; returns the device loss vector
        [total, mse_full, mse_missing, rmse_text, rmse_query, rmse_fused, rnc, 0].
        teacher_rows (a trainer with a teacher): the [B] rows of the teacher's tables this batch's samples have (indices, on the host
        or the device; checked on the host), or None: the tables are [B, ...] in this batch's order."""
        teacher_idx = None
        if self._teacher_on():
            if teacher_rows is None:
                self.teacher.check_batch(audio.shape[0], "step")
            else:
                rows = self.teacher.check_rows(teacher_rows, "step")
                if rows.numel() != audio.shape[0]:
                    raise _lib.SdumcError(f"step: teacher_rows has {rows.numel()} entries for a batch of {audio.shape[0]}")
                self._keep_rows = rows.to(self.params.device)
                teacher_idx = self._keep_rows.data_ptr()
        ts = self._get(audio.shape[0], (audio.shape[1], text.shape[1], video.shape[1], feat4.shape[1]))
        if self.arena is not None:
            ts.use_set(0, planes=False)      # (fresh tensors: a split for one use costs more than the planes save)
        # the caller's device tensors are read where they are when they qualify (no 224 MB copy per batch); else copied.  The trainer
        # holds them, in ONE slot, until the next step(); the cached per-shape step is unbound again and keeps nothing alive
        batch = (audio, text, video, feat4, labels.reshape(-1) if torch.is_tensor(labels) else labels)
        self._batch = batch if ts.use_batch(*batch) else None
        ts.set_lengths(lengths)
        losses = self._launch(ts, teacher_idx=teacher_idx)
        ts._bind(None)
        return losses
