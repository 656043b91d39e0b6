"""Saliency maps from evaluation epochs over a resident feature store: which frames of which modality moved the eval-mode prediction,
per frame and in store order -- the gradient-based half of what the attention maps (evaluate.eval_epoch(..., attention=True)) are
plotted for.

For stream s (0 = full, 1 = text-missing), modality m of that stream (audio, text slot, video; stream 1's text slot is feat4),
utterance i and frame t < length_m[i], with g = d vals_out_s[i] / d feat_m[i, t, :] (the gradient of the eval-mode prediction, model
:282-284 through :364, with respect to the frame's input feature row):
    column 0 ('grad_x_input')  sum_c g[c] * feat_m[i, t, c]      gradient x input, signed
    column 1 ('grad_norm')     sqrt(sum_c g[c]^2)                gradient norm

`saliency_epoch` has the shape of evaluate.Evaluator.eval_epoch: the epoch's index vectors are uploaded once, forward i
(sdumc_net_forward, eval mode, both streams) carries the assembly of batch i + 1 (sdumc_net_io.prefetch), batches are read in place
through row maps where the store allows it, and nothing crosses to the host inside the loop.  In eval mode the samples of a batch do
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
from .evaluate import ATTENTION as STREAMS, MODS, Evaluator, _EvalArena, attention_rows, checked_plan

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


def _rows_dict(rows):
    if not isinstance(rows, dict):
        rows = dict(zip(MODS, rows))
    return {m: int(rows[m]) for m in MODS}


class SaliencyResult:
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
        rows, streams = _rows_dict(rows), _stream_names(streams)
        maps = {s: {m: torch.empty(rows[m], NCOL, device=device) for m in mods} for s, mods in STREAMS if s in streams}
        return cls(torch.empty(2, n, device=device), torch.empty(n, dtype=torch.uint8, device=device), maps)

    def fits(self, n, device, rows, streams=("full", "missing")):
        rows, streams, device = _rows_dict(rows), _stream_names(streams), torch.device(device)
        ok = (self.preds.shape == (2, n) and self.preds.device == device and self.seen.numel() == n
              and self.seen.element_size() == 1 and tuple(self.maps) == streams)
        return ok and all(m in self.maps[s] and self.maps[s][m].shape == (rows[m], NCOL) and self.maps[s][m].device == device
                          and self.maps[s][m].dtype == torch.float32 and self.maps[s][m].is_contiguous()
                          for s, mods in STREAMS if s in streams for m in mods)

    def reset(self):
        """NaN everywhere, nothing seen: once per epoch, in front of its first batch"""
        self.preds.fill_(float("nan"))
        self.seen.zero_()
        for d in self.maps.values():
            for t in d.values():
                t.fill_(float("nan"))
        return self

    def of(self, store, i):
        """The maps of ONE utterance -- i = its index in the store, or its name -- as views: {stream: {modality: [T_i, 2]}}, sliced by
        the store's start / length tables.  Raises when the utterance is unknown or was not visited in this epoch."""
        if isinstance(i, str):
            try:
                i = store.names.index(i)
            except ValueError:
                raise _lib.SdumcError(f"SaliencyResult: no utterance named {i!r} in the store") from None
        i = int(i)
        if not 0 <= i < self.seen.numel():
            raise _lib.SdumcError(f"SaliencyResult: utterance index {i} out of range [0, {self.seen.numel()})")
        if int(self.seen.reshape(-1)[i]) == 0:
            raise _lib.SdumcError(f"SaliencyResult: utterance {i} was not visited in this epoch")
        out = {}
        for s, d in self.maps.items():
            out[s] = {}
            for m, t in d.items():
                a, n = int(store.start[m][i]), int(store.length[m][i])
                out[s][m] = t[a:a + n]
        return out


class _SaliencyArena(_EvalArena):
    """Device memory of saliency epochs, sized for the largest batch seen so far: what evaluation holds (the eval workspace, the
    forward's five outputs, two input sets) plus the packed frame weights' scratch of the feature-gradient backward, a zeroed gradient
    bucket that backward may overwrite, the four padded d_feat buffers and two d_vals seed vectors per batch size."""

    def __init__(self, dev, B, T, fdims, nbytes, scratch_bytes, live):
        super().__init__(dev, B, T, fdims, torch.float32, nbytes)
        self.feat_scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        self.bucket = torch.zeros(live, device=dev)
        self.d_feat = [torch.empty(self.B * t * d, device=dev) for t, d in zip(self.T, fdims)]
        self._seeds = {}

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

    def saliency_epoch(self, store, batches, key_padding=False, streams=("full", "missing"), out=None):
        n_store = len(store)
        # ---- host-side checks: nothing is enqueued (and nothing of `out` is touched) before all of them have passed ----
        streams = _stream_names(streams)
        plan, batches = checked_plan(batches, n_store)
        if self.feature_dtype != torch.float32 or store.packed['audio'].dtype != torch.float32:
            raise _lib.SdumcError("saliency_epoch: feature gradients exist in fp32 storage only (not in bf16 storage, not from a bf16 store)")
        if store.packed['audio'].device != self.params.device:
            raise _lib.SdumcError("saliency_epoch: the store and the parameters live on different devices")
        if tuple(store.get_featdim()) != self._fdims:
            raise _lib.SdumcError(f"saliency_epoch: the store's feature widths {store.get_featdim()} are not {self._fdims}")
        rows = frame_rows(store)
        if min(rows.values()) < 1:
            raise _lib.SdumcError("saliency_epoch: needs a store with at least one frame per modality")
        if out is not None and not (isinstance(out, SaliencyResult) and out.fits(n_store, self.params.device, rows, streams)):
            raise _lib.SdumcError("saliency_epoch: out= is not a result of this store's size, device, frames and streams")
        inplace = self._in_place(store)
        if plan is None:
            plan = store.plan_epoch(batches)
        shapes = set(plan.shapes)
        need = max(self._shape(s)[1] for s in shapes)
        scratch = max(self._scratch_bytes(s) for s in shapes)
        if scratch < 1:
            raise _lib.SdumcError("saliency_epoch: the engine has no feature gradients for these dims")
        Bmax, Tmax = max(B for B, _ in shapes), tuple(max(T[i] for _, T in shapes) for i in range(4))
        # ---- memory ----
        a = self.arena
        if a is None or not a.fits(Bmax, Tmax, need, scratch):
            if a is not None:
                Bmax, Tmax = max(Bmax, a.B), tuple(max(t, c) for t, c in zip(Tmax, a.T))
                need, scratch = max(need, a.workspace.numel()), max(scratch, a.feat_scratch.numel())
            a = self.arena = _SaliencyArena(self.params.device, Bmax, Tmax, self._fdims, need, scratch, self._live)
        planes = False
        if not inplace and store.packed_p3 is not None and self._planes_ok:
            a.ensure_planes()
            planes = True
        res = (out if out is not None else SaliencyResult.empty(n_store, self.params.device, rows, streams)).reset()
        ios = [self._io(store, k, inplace, planes, key_padding) for k in range(2)]
        wanted = [(s, name) for s, (name, _) in enumerate(STREAMS) if name in streams]
        for B in {B for B, _ in shapes}:
            a.seeds(B)
        segs, mark, st = {}, ptr(res.seen), _lib.current_stream()
        # ---- the epoch: no host synchronisation from here on ----
        n = len(plan)
        g = self._desc(store, plan, 0, inplace, planes, key_padding)
        check(lib.sdumc_gather_batch(C.byref(g), 0, st), "sdumc_gather_batch")
        nxt = self._shape(plan.shapes[0])[0]
        for i in range(n):
            d, io, (B, T) = nxt, ios[i & 1], plan.shapes[i]
            sg = segs.get(B)
            if sg is None:
                sg = segs[B] = self._segments(res, B, False)
            pf = None
            if i + 1 < n:
                nxt = self._shape(plan.shapes[i + 1])[0]
                pf = self._desc(store, plan, i + 1, inplace, planes, key_padding)
            io.prefetch = C.addressof(pf) if pf is not None else None
            try:
                check(lib.sdumc_net_forward(C.byref(d), C.byref(io), st), "sdumc_net_forward")
            finally:
                io.prefetch = None
            for s, name in wanted:      # (the backward leaves the forward's part of the workspace as it is: one forward serves both)
                ng = self._grads(s, B)
                check(lib.sdumc_net_backward(C.byref(d), C.byref(io), C.byref(ng), st), "sdumc_net_backward")
                self._reduce(self._saliency_descs(store, res, name, s, i & 1, B, T, inplace), plan.idx_ptr(i), st)
            check(lib.sdumc_scatter_rows_multi(sg, len(sg), plan.idx_ptr(i), B, mark, st), "sdumc_scatter_rows_multi")
        self._keep_plan = plan      # (the index tensor must outlive the enqueued gathers and scatters)
        return res


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
