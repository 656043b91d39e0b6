"""Saliency maps from evaluation epochs over a resident feature store: which frames of which modality moved the eval-mode prediction,
per frame and in store order -- the gradient-based half of what the attention maps (evaluate.eval_epoch(..., attention=True)) are
plotted for.

For stream s (0 = full, 1 = text-missing), modality m of that stream (audio, text slot, video; stream 1's text slot is feat4),
utterance i and frame t < length_m[i], with g = d vals_out_s[i] / d feat_m[i, t, :] (the gradient of the eval-mode prediction, model
:282-284 through :364, with respect to the frame's input feature row):
    column 0 ('grad_x_input')  sum_c g[c] * feat_m[i, t, c]      gradient x input, signed
    column 1 ('grad_norm')     sqrt(sum_c g[c]^2)                gradient norm

`saliency_epoch` is evaluate.Evaluator.eval_epoch's loop (epoch.run has its definition) with the feature-gradient backwards between
the forward (sdumc_net_forward, eval mode, both streams) and the scatter.  In eval mode the samples of a batch do
not interact, so ONE backward (sdumc_net_backward) seeded with d_vals = 1 on the rows of stream s, 0 on the other stream's rows and
every other output gradient NULL gives all per-sample feature gradients of that stream at once (the other stream adds exact zeros to
the summed d_audio / d_video).  Per batch: one forward; per requested stream one backward with exactly the feature-gradient pointers
that stream reads and ONE sdumc_frame_saliency launch that reduces the three padded [B, T, d] gradients against the features to
[rows, 2] tensors in store order; then the sdumc_scatter_rows_multi launch for the predictions and the visited set.  The backward
reads the forward's workspace and writes only its own buffers of the plan, so both streams' backwards follow ONE forward.

As with the attention maps: with key_padding=False (the reference) the padded frames take part in the softmax and an utterance's map
depends on the batch it was evaluated in; with key_padding=True it does not.  Only frames t < length are exported.

The epoch owns its device memory (_SaliencyArena) and reads the flat parameters and nothing else of a training run: parameters, Adam
moments, step count and dropout counter are untouched.  Feature gradients exist in fp32 storage only.

`frame_scores` applies the same rule with torch ops in fp64 on any device: for users of the drop-in module (audio.grad after
vals.sum().backward() under model.eval())."""
import ctypes as C

import torch

from . import _lib, engine
from ._lib import lib, check, ptr
from .epoch import MODS, StoreOrdered, rows_dict
from .evaluate import ATTENTION as STREAMS, Evaluator, attention_rows

COLUMNS = ("grad_x_input", "grad_norm")
NCOL = _lib.SALIENCY_COLS
frame_rows = attention_rows      # {modality: packed rows of a store}, from its host tables


def frame_scores(grad, feat, lengths=None):
    """grad, feat [..., T, d] (any float dtype, any device) -> [..., T, 2] fp64: column 0 = sum_c grad * feat, column 1 =
    sqrt(sum_c grad^2), both formed in fp64.  lengths ([...] valid frame counts): rows t >= length are zero in the result."""
    g, x = grad.double(), feat.double()
    out = torch.stack(((g * x).sum(-1), (g * g).sum(-1).sqrt()), dim=-1)
    if lengths is not None:
        T = out.shape[-2]
        n = torch.as_tensor(lengths, device=out.device).reshape(out.shape[:-2] + (1,))
        pad = torch.arange(T, device=out.device).expand(out.shape[:-1]) >= n
        out = out.masked_fill(pad.unsqueeze(-1), 0.0)
    return out


def _stream_names(streams):
    names = [s for s, _ in STREAMS]
    if isinstance(streams, str):
        streams = (streams,)
    streams = tuple(streams)
    for s in streams:
        if s not in names:
            raise _lib.SdumcError(f"saliency_epoch: unknown stream {s!r} (one or both of {tuple(names)})")
    if not streams:
        raise _lib.SdumcError("saliency_epoch: no stream asked for")
    return tuple(s for s in names if s in streams)


class SaliencyResult(StoreOrdered):
    """Results of one saliency epoch in STORE order: preds [2, N] (row 0 the full stream, row 1 the text-missing one), seen [N]
    (uint8: visited this epoch), maps {'full': {'audio', 'text', 'video'}, 'missing': {'audio', 'feat4', 'video'}} -- the requested
    streams only -- of [rows_m, 2] fp32 tensors, rows_m = the frames of all utterances of that modality in store order (row start[i] + t
    = frame t of utterance i; columns = COLUMNS).  Rows not visited hold NaN.  Device or CPU tensors."""

    COLUMNS = COLUMNS

    def __init__(self, preds, seen, maps):
        self.preds, self.seen, self.maps = preds, seen, maps

    @classmethod
    def empty(cls, n, device, rows, streams=("full", "missing")):
        """rows = frame_rows(store) (or the four row counts, audio / text / video / feat4)"""
        rows, streams = rows_dict(rows), _stream_names(streams)
        maps = {s: {m: torch.empty(rows[m], NCOL, device=device) for m in mods} for s, mods in STREAMS if s in streams}
        return cls(*cls._empty(n, device)[:2], maps)

    def fits(self, n, device, rows, streams=("full", "missing")):
        rows, streams = rows_dict(rows), _stream_names(streams)
        return (self._fits(n, device) and tuple(self.maps) == streams
                and self._frames_fit(self.maps, [(s, mods) for s, mods in STREAMS if s in streams], rows, NCOL, device))

    def reset(self):
        """NaN everywhere, nothing seen: once per epoch, in front of its first batch"""
        return self._reset(*(t for d in self.maps.values() for t in d.values()))

    def of(self, store, i):
        """The maps of ONE utterance -- i = its index in the store, or its name -- as views: {stream: {modality: [T_i, 2]}}, sliced by
        the store's start / length tables.  Raises when the utterance is unknown or was not visited in this epoch."""
        return self._frames_of(store, i, self.maps)


class _SaliencyArena(engine._Arena):
    """Device memory of saliency epochs, sized for the largest batch seen so far: what evaluation holds (the eval workspace, the
    forward's five outputs, two input sets) plus the packed frame weights' scratch of the feature-gradient backward, a zeroed gradient
    bucket that backward may overwrite, the four padded d_feat buffers and two d_vals seed vectors per batch size."""

    def __init__(self, dev, B, T, fdims, nbytes, scratch_bytes, live):
        super().__init__(dev, B, T, fdims, torch.float32, nbytes)
        self.feat_scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        self.bucket = torch.zeros(live, device=dev)
        self.d_feat = [torch.empty(self.B * t * d, device=dev) for t, d in zip(self.T, fdims)]
        self._seeds = {}

    @property
    def nbytes(self):
        return (self.workspace.numel(), self.feat_scratch.numel())

    def fits(self, B, T, nbytes, scratch_bytes):
        return super().fits(B, T, nbytes) and scratch_bytes <= self.feat_scratch.numel()

    def seeds(self, B):
        """[2, 2 B]: row s = d_vals of a two-stream batch of B with ones on stream s's rows"""
        t = self._seeds.get(B)
        if t is None:
            t = self._seeds[B] = torch.zeros(2, 2 * B, device=self.bucket.device)
            t[0, :B] = 1.0
            t[1, B:] = 1.0
        return t


class Saliency(Evaluator):
    """The state `saliency_epoch` keeps across epochs for one parameter buffer: the arena and the per-shape dims."""

    def __init__(self, flat_params, dims, bf16=False, inplace=True, planes=None, prefetch_workgroups=0):
        super().__init__(flat_params, dims, bf16=bf16, inplace=inplace, planes=planes, prefetch_workgroups=prefetch_workgroups)
        self._live = engine.ParamLayout.get(*self.dims[:3]).live
        self._scratch = {}      # (B, T) -> bytes of the feature-gradient scratch

    def _scratch_bytes(self, shape):
        nb = self._scratch.get(shape)
        if nb is None:
            nb = self._scratch[shape] = int(lib.sdumc_net_feature_grad_scratch_bytes(C.byref(self._shape(shape)[0])))
        return nb

    def _grads(self, s, B):
        """sdumc_net_grads of stream s for batches of B: the one-hot d_vals, every other output gradient NULL, and exactly the feature
        gradients that stream reads"""
        a = self.arena
        g = _lib.NetGrads()
        g.d_vals = a.seeds(B).data_ptr() + 4 * s * 2 * B
        g.grads = ptr(a.bucket)
        g.d_audio, g.d_video = ptr(a.d_feat[0]), ptr(a.d_feat[2])
        g.d_text[s] = ptr(a.d_feat[1 if s == 0 else 3])
        g.feat_scratch, g.feat_scratch_bytes = ptr(a.feat_scratch), a.feat_scratch.numel()
        return g

    def _saliency_descs(self, store, res, name, s, k, B, T, inplace):
        """sdumc_frame_saliency's descriptors of stream s for one batch in input set k: the three modalities that stream reads"""
        a, st = self.arena, self.arena.sets[k]
        descs = (_lib.SaliencyDesc * 3)()
        for j, m in enumerate(STREAMS[s][1]):
            slot = MODS.index(m)
            p = descs[j]
            p.grad = ptr(a.d_feat[slot])
            if inplace:
                p.feat, p.row_map, p.store_rows = ptr(store.packed[m]), ptr(st.maps[slot]), int(store.packed[m].shape[0])
            else:
                p.feat = ptr(st.inputs[slot])
            p.start, p.length, p.n_utt = ptr(store.start_d[m]), ptr(store.length_d[m]), len(store)
            p.dst, p.dst_rows = ptr(res.maps[name][m]), int(res.maps[name][m].shape[0])
            p.B, p.T, p.d = B, T[slot], self._fdims[slot]
        return descs

    def _reduce(self, descs, idx_ptr, st):
        """one stream's three feature gradients -> its maps (tools/saliency_bench.py times the epoch without this launch)"""
        check(lib.sdumc_frame_saliency(descs, len(descs), idx_ptr, st), "sdumc_frame_saliency")

    def _bytes(self, shapes):
        scratch = max(self._scratch_bytes(s) for s in shapes)
        if scratch < 1:
            raise _lib.SdumcError("saliency_epoch: the engine has no feature gradients for these dims")
        return super()._bytes(shapes) + (scratch,)

    def _new_arena(self, B, T, nbytes, scratch_bytes):
        return _SaliencyArena(self.params.device, B, T, self._fdims, nbytes, scratch_bytes, self._live)

    def saliency_epoch(self, store, batches, key_padding=False, streams=("full", "missing"), out=None):
        # ---- saliency's own refusals, then the pre-flight it shares with eval_epoch ----
        streams = _stream_names(streams)
        if self.feature_dtype != torch.float32 or store.packed['audio'].dtype != torch.float32:
            raise _lib.SdumcError("saliency_epoch: feature gradients exist in fp32 storage only (not in bf16 storage, not from a bf16 store)")
        rows = frame_rows(store)
        if min(rows.values()) < 1:
            raise _lib.SdumcError("saliency_epoch: needs a store with at least one frame per modality")
        plan, res, inplace, planes = self._prepare("saliency_epoch", store, batches, out, SaliencyResult, (rows, streams),
                                                   "frames and streams")
        wanted = [(s, name) for s, (name, _) in enumerate(STREAMS) if name in streams]
        for B in {B for B, _ in plan.shapes}:
            self.arena.seeds(B)

        def backwards(i, k, d, io, st):      # (the backward leaves the forward's part of the workspace as it is: one forward serves both)
            B, T = plan.shapes[i]
            for s, name in wanted:
                ng = self._grads(s, B)
                check(lib.sdumc_net_backward(C.byref(d), C.byref(io), C.byref(ng), st), "sdumc_net_backward")
                self._reduce(self._saliency_descs(store, res, name, s, k, B, T, inplace), plan.idx_ptr(i), st)
        return self._run(store, plan, res, inplace, planes, key_padding, False, backwards)


_saliency = None      # saliency_epoch's state: ONE object (the last parameter buffer asked for), so its arena is kept across epochs


def saliency_epoch(flat_params, dims, store, batches, *, key_padding=False, streams=("full", "missing"), inplace=True, out=None):
    """One saliency pass over `batches` (index vectors into `store`, or a data.EpochPlan -- any subset of the store, any order, no index
    twice) with the parameters `flat_params`: both streams in eval mode, one feature-gradient backward per requested stream ->
    SaliencyResult in store order (preds and seen as evaluate.eval_epoch gives them; maps[stream][modality] [frames of the store, 2]:
    gradient x input and gradient norm of the stream's prediction per frame).
    key_padding=True hands the valid frame counts to the attention poolings (extension, default off = the reference: the padded
    frames take part in the softmax and an utterance's map depends on the batch it was evaluated in); streams: one or both of 'full',
    'missing' (one stream: half the backwards); inplace=False gathers padded copies even where the store could be read in place;
    out= reuses a previous result's tensors.  fp32 storage only."""
    global _saliency
    dims = tuple(int(d) for d in dims)
    key = (flat_params.data_ptr(), flat_params.device, dims, bool(inplace))
    if _saliency is None or _saliency[0] != key:
        _saliency = (key, Saliency(flat_params, dims, inplace=inplace))
    return _saliency[1].saliency_epoch(store, batches, key_padding=key_padding, streams=streams, out=out)
