"""Evaluation epochs over a resident feature store: the validation and test passes of the reference driver
(main_frame_val_text_missing.py:333-353 calls train_or_eval_model three times per epoch; :151-166 is the eval branch -- both streams,
no_grad, model.eval(); main_frame_val_text_missing_inference.py:100-215 is the same loop with the embeddings kept).

`eval_epoch` is to those passes what FusedTrainer.run_epoch is to the training pass: the epoch's index vectors are uploaded once, the
first batch is assembled in front of the first forward, and forward i (sdumc_net_forward, train = 0, both streams in one call: the
audio / video frame projections run once) carries the assembly of batch i + 1 on its background lane (sdumc_net_io.prefetch).  With a
store the training epoch would read in place, no padded copy of a batch exists: the forward reads the packed tensors through row maps.
After every forward ONE launch (sdumc_scatter_rows_multi) moves the batch's stream-major outputs to the rows its utterances have in
the store, so the results line up with store.names / store.vals whatever order the sampler used, and nothing crosses to the host
inside the loop.  The metrics stay on the host (metric.py): [N] vectors cross once per epoch.

Evaluation owns its device memory (_EvalArena): workspace, outputs, two sets of row maps / labels / lengths (and input buffers when
batches are gathered).  It reads the flat parameters and nothing else of a training run -- no step workspace, no keep-bits, no
Philox counter (rng_state = NULL) -- so a training run is bit for bit the same with or without evaluation epochs in between.

attention=True keeps what the reference's inference pass plots per utterance (vector_attention of FRA2UTT_new / Cross_Attention,
model :68, :95; attention_masks, model :291; main_frame_val_text_missing_inference.py:176-181): ONE more launch per batch
(sdumc_net_export_attention, between the forward and the scatter) copies the six poolings' normalised softmax-over-time weights of
both streams out of the forward's workspace to per-frame tensors in store order (EvalResult.attention)."""
import ctypes as C

import numpy as np
import torch

from . import _lib, engine
from ._lib import lib, check, ptr

D, H, NQ, RNC_DIM = _lib.D, _lib.H, _lib.NQ, _lib.RNC_DIM
# the forward's outputs beside vals, in sdumc_net_io's order: name, trailing shape, (full, missing) keys of checkpoint.run_inference
EMBEDDINGS = (("fused", (H,), ("full_rep", "missing_rep")),
              ("rnc", (RNC_DIM,), ("full_rnc", "missing_rnc")),
              ("text_hidden", (D,), ("text_rep_query_full", "text_rep_query_missing")),
              ("cross_text", (NQ, H), ("text_rep_full", "text_rep_missing")))
# the attention maps: per stream, the modalities its three pooling pairs read (stream 1's text slot is feat4); every tensor
# [packed rows of that modality, ATTN_COLS]: column 0 FRA2UTT_new's weight, columns 1..7 Cross_Attention's in multi_query order
ATTENTION = (("full", ("audio", "text", "video")), ("missing", ("audio", "feat4", "video")))
ATTN_COLS = 1 + NQ
MODS = ("audio", "text", "video", "feat4")


def attention_rows(store):
    """{modality: packed rows (frames of all utterances, without the trailing zero row)} of a store -- from its host tables"""
    return {m: int(torch.as_tensor(store.length[m]).sum()) for m in MODS}


def _rows_dict(rows):
    if rows is None:
        raise _lib.SdumcError("EvalResult: attention=True needs rows= (evaluate.attention_rows(store), or the four row counts)")
    if not isinstance(rows, dict):
        rows = dict(zip(MODS, rows))
    return {m: int(rows[m]) for m in MODS}


def check_epoch_indices(batches, n):
    """Host-side check of an epoch's index vectors against a store of n utterances: every index in [0, n) and none visited twice
    (the scatter writes every result row once; a second visit would race with the first).  Returns the concatenated int64 tensor."""
    idxs = [torch.as_tensor(b, dtype=torch.int64).reshape(-1).cpu() for b in batches]
    if not idxs or any(i.numel() == 0 for i in idxs):
        raise _lib.SdumcError("eval_epoch: no batches, or an empty batch")
    flat = torch.cat(idxs)
    if int(flat.min()) < 0 or int(flat.max()) >= n:
        raise _lib.SdumcError(f"eval_epoch: sample index out of range [0, {n})")
    u, counts = torch.unique(flat, return_counts=True)
    if u.numel() != flat.numel():
        raise _lib.SdumcError(f"eval_epoch: index {int(u[counts > 1][0])} appears more than once in the epoch")
    return flat


def checked_plan(batches, n):
    """check_epoch_indices over `batches` -- index vectors, or a data.EpochPlan (its host copy of the indices when it kept one) -- before
    anything is uploaded or enqueued -> (the plan or None, the batches as int64 tensors or None)."""
    from .data import EpochPlan
    if isinstance(batches, EpochPlan):
        host = getattr(batches, "idx_h", None)
        host = batches.idx_d.cpu() if host is None else host
        bounds = list(batches.offsets) + [int(host.numel())]
        check_epoch_indices([host[a:b] for a, b in zip(bounds, bounds[1:])], n)
        return batches, None
    batches = [torch.as_tensor(b, dtype=torch.int64).reshape(-1) for b in batches]
    check_epoch_indices(batches, n)
    return None, batches


class EvalResult:
    """Results of one evaluation epoch in STORE order (row i = utterance i of the store): preds [2, N] (row 0 the full stream, row 1
    the text-missing one), seen [N] (uint8 / bool: visited this epoch), embeddings None or {'fused' [2, N, 128], 'rnc' [2, N, 64],
    'text_hidden' [2, N, 256], 'cross_text' [2, N, 7, 128]}, attention None or {'full': {'audio', 'text', 'video'}, 'missing':
    {'audio', 'feat4', 'video'}} of [rows_m, 8] tensors, rows_m = the frames of all utterances of that modality in store order
    (row start[i] + t = frame t of utterance i; column 0 the FRA2UTT_new weight, columns 1..7 the Cross_Attention weights in
    multi_query order: fused, at, tv, av, audio, text, video).  Rows not visited hold NaN.  Device or CPU tensors."""

    def __init__(self, preds, seen, embeddings=None, attention=None):
        self.preds, self.seen, self.embeddings, self.attention = preds, seen, embeddings, attention

    @classmethod
    def empty(cls, n, device, embeddings=False, attention=False, rows=None):
        """attention=True: rows = attention_rows(store) (or the four row counts, audio / text / video / feat4)"""
        emb = att = None
        if embeddings:
            emb = {name: torch.empty((2, n) + shape, device=device) for name, shape, _ in EMBEDDINGS}
        if attention:
            rows = _rows_dict(rows)
            att = {s: {m: torch.empty(rows[m], ATTN_COLS, device=device) for m in mods} for s, mods in ATTENTION}
        return cls(torch.empty(2, n, device=device), torch.empty(n, dtype=torch.uint8, device=device), emb, att)

    def fits(self, n, device, embeddings, attention=False, rows=None):
        ok = (self.preds.shape == (2, n) and self.preds.device == torch.device(device) and self.seen.numel() == n
              and self.seen.element_size() == 1 and (self.embeddings is not None) == bool(embeddings)
              and (self.attention is not None) == bool(attention))
        if ok and attention:
            rows = _rows_dict(rows)
            ok = all(s in self.attention and m in self.attention[s] and self.attention[s][m].shape == (rows[m], ATTN_COLS)
                     and self.attention[s][m].device == torch.device(device) and self.attention[s][m].dtype == torch.float32
                     and self.attention[s][m].is_contiguous() for s, mods in ATTENTION for m in mods)
        return ok

    def reset(self):
        """NaN everywhere, nothing seen: once per epoch, in front of its first batch"""
        self.preds.fill_(float("nan"))
        self.seen.zero_()
        for t in (self.embeddings or {}).values():
            t.fill_(float("nan"))
        for d in (self.attention or {}).values():
            for t in d.values():
                t.fill_(float("nan"))
        return self

    def attention_of(self, store, i):
        """The attention maps of ONE utterance -- i = its index in the store, or its name -- as views: {'full': {'audio' [T_a, 8],
        'text' [T_t, 8], 'video' [T_v, 8]}, 'missing': {'audio', 'feat4' [T_f4, 8], 'video'}}, sliced by the store's start / length
        tables.  Raises when the epoch kept no attention maps or did not visit the utterance."""
        if self.attention is None:
            raise _lib.SdumcError("EvalResult: this epoch kept no attention maps (eval_epoch(..., attention=True))")
        if isinstance(i, str):
            try:
                i = store.names.index(i)
            except ValueError:
                raise _lib.SdumcError(f"EvalResult: no utterance named {i!r} in the store") from None
        i = int(i)
        if not 0 <= i < self.seen.numel():
            raise _lib.SdumcError(f"EvalResult: utterance index {i} out of range [0, {self.seen.numel()})")
        if int(self.seen.reshape(-1)[i]) == 0:
            raise _lib.SdumcError(f"EvalResult: utterance {i} was not visited in this epoch")
        out = {}
        for s, mods in ATTENTION:
            out[s] = {}
            for m in mods:
                a, n = int(store.start[m][i]), int(store.length[m][i])
                out[s][m] = self.attention[s][m][a:a + n]
        return out

    def _visited(self):
        rows = np.flatnonzero(self.seen.cpu().numpy().reshape(-1) != 0)
        if rows.size == 0:
            raise _lib.SdumcError("EvalResult: no row was visited")
        return rows

    def results(self, store):
        """The dictionary checkpoint.run_inference returns (same keys, array shapes and embedding names), over the visited rows in
        store order, names from store.names, labels from store.vals; plus val_mse_full (main :170; = val_mse).  One device -> host
        copy per tensor."""
        rows = self._visited()
        preds = self.preds.cpu().numpy()
        labels = torch.as_tensor(store.vals).cpu().numpy().astype(np.float32).reshape(-1)[rows]
        out = {"val_preds_full": preds[0][rows].reshape(-1, 1), "val_preds_missing": preds[1][rows].reshape(-1, 1),
               "val_labels": labels}
        for name, _, keys in EMBEDDINGS if self.embeddings is not None else ():
            t = self.embeddings[name].cpu().numpy()
            out[keys[0]], out[keys[1]] = t[0][rows], t[1][rows]
        out["names"] = [store.names[i] for i in rows.tolist()]
        out["val_mse"] = float(np.mean((labels - out["val_preds_full"].reshape(-1)) ** 2))
        out["val_mse_full"] = out["val_mse"]
        out["val_mse_missing"] = float(np.mean((labels - out["val_preds_missing"].reshape(-1)) ** 2))
        return out

    def metrics(self, store):
        """{'full': eval_mosei_metric(...), 'missing': ...} of the visited rows (main :366-367), on the host."""
        from .metric import eval_mosei_metric
        rows = self._visited()
        preds = self.preds.cpu().numpy()
        labels = torch.as_tensor(store.vals).cpu().numpy().reshape(-1)[rows]
        names = [store.names[i] for i in rows.tolist()]
        return {"full": eval_mosei_metric(preds[0][rows], labels, names), "missing": eval_mosei_metric(preds[1][rows], labels, names)}


class _EvalArena:
    """Device memory of evaluation, sized for the largest batch seen so far: the eval workspace, the forward's five [2 B, w] outputs
    and two engine._InputSet (row maps, labels, lengths; padded input buffers and planes only once a batch is gathered)."""

    def __init__(self, dev, B, T, fdims, dtype, nbytes):
        self.B, self.T = int(B), tuple(int(t) for t in T)
        self._fdims = fdims
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        V = 2 * self.B
        self.outs = [torch.empty(V * k, device=dev) for k in (1, H, RNC_DIM, D, NQ * H)]
        rows = [self.B * t for t in self.T]
        self.sets = [engine._InputSet([r * d for r, d in zip(rows, fdims)], self.B, dtype, dev, rows) for _ in range(2)]

    def fits(self, B, T, nbytes):
        return B <= self.B and all(t <= c for t, c in zip(T, self.T)) and nbytes <= self.workspace.numel()

    def ensure_planes(self):
        for st in self.sets:
            if st.planes is None:
                st.planes = [engine._planes_buffer(r, d, self.workspace.device) for r, d in zip(st._rows, self._fdims)]


class Evaluator:
    """The state `eval_epoch` keeps across epochs for one parameter buffer: the arena and the per-shape dims."""

    def __init__(self, flat_params, dims, bf16=False, inplace=True, planes=None, prefetch_workgroups=0):
        engine._require_cuda(flat_params)
        self.params, self.dims, self.bf16 = flat_params, tuple(int(d) for d in dims), bf16
        lay = engine.ParamLayout.get(*self.dims[:3])
        if flat_params.numel() != lay.total:
            raise _lib.SdumcError("flat parameter buffer has the wrong size")
        self.inplace = bool(inplace)
        self.prefetch_workgroups = int(prefetch_workgroups)
        self._fdims = (self.dims[0], self.dims[1], self.dims[2], self.dims[1])
        self.feature_dtype = torch.bfloat16 if engine.bf16_mode(bf16, self.dims) == 2 else torch.float32
        self._planes_ok = planes is not False and engine.planes_wanted(True, self.dims, bf16)
        self.arena = None
        self._dims = {}       # (B, T) -> (sdumc_net_dims, workspace bytes)

    def _in_place(self, store):
        """as FusedTrainer._in_place: fp32 storage and a store with planes, or bf16 storage and a bf16 store (widths % 128 == 0)"""
        if not self.inplace:
            return False
        if self.feature_dtype == torch.bfloat16:
            return store.packed['audio'].dtype == torch.bfloat16 and all(d % 128 == 0 for d in self.dims[:3])
        return store.packed_p3 is not None and self._planes_ok

    def _shape(self, shape):
        """eval dims of one (B, T) and the workspace they need; a shape the engine refuses raises"""
        e = self._dims.get(shape)
        if e is None:
            B, T = shape
            d = engine.make_dims(B, 2, T[0], T[2], (T[1], T[3]), self.dims, False, 0, bf16=self.bf16)
            nb = lib.sdumc_net_workspace_bytes(C.byref(d))
            if nb == 0:
                raise _lib.SdumcError(f"eval_epoch: the engine refuses the batch shape B={B}, T={T}")
            e = self._dims[shape] = (d, int(nb))
        return e

    def _io(self, store, k, inplace, planes, key_padding):
        a, st = self.arena, self.arena.sets[k]
        io = _lib.NetIO()
        if inplace:
            feats = [store.packed[m] for m in store.MODS]
            p3 = [store.packed_p3[m] for m in store.MODS] if self.feature_dtype == torch.float32 else None
            for i, m in enumerate(st.ensure_maps()):
                io.row_map[i], io.store_rows[i] = ptr(m), int(feats[i].shape[0])
        else:
            feats, p3 = st.inputs, (st.planes if planes else None)
        io.audio, io.text[0], io.video, io.text[1] = (ptr(t) for t in feats)
        if p3 is not None:
            io.audio_p3, io.text_p3[0], io.video_p3, io.text_p3[1] = (ptr(t) for t in p3)
        io.params, io.rng_state = ptr(self.params), None
        io.workspace, io.workspace_bytes = ptr(a.workspace), a.workspace.numel()
        io.vals, io.fused, io.rnc, io.text_hidden, io.cross_text = (ptr(t) for t in a.outs)
        if key_padding:
            for i, t in enumerate(st.lengths):
                io.lengths[i] = ptr(t)
        io.prefetch_workgroups = self.prefetch_workgroups
        return io

    def _desc(self, store, plan, i, inplace, planes, key_padding):
        st = self.arena.sets[i & 1]
        B, T = plan.shapes[i]
        lens = st.lengths if key_padding else None
        if inplace:
            return store.gather_desc(plan.idx_ptr(i), B, T, None, st.labels, lens, maps_out=st.ensure_maps())
        return store.gather_desc(plan.idx_ptr(i), B, T, st.inputs, st.labels, lens, st.planes if planes else None)

    def _segments(self, res, B, embeddings):
        """the scatter's segment table for batches of B: rows [0, B) of every output to stream 0's result, rows [B, 2 B) to stream 1's"""
        pairs = [(self.arena.outs[0], res.preds, 1)]
        if embeddings:
            pairs += [(self.arena.outs[j + 1], res.embeddings[name], int(np.prod(shape))) for j, (name, shape, _) in enumerate(EMBEDDINGS)]
        n = res.preds.shape[1]
        segs = (_lib.ScatterSeg * (2 * len(pairs)))()
        for j, (src, dst, w) in enumerate(pairs):
            for s in range(2):
                sg = segs[2 * j + s]
                sg.src, sg.dst = src.data_ptr() + 4 * s * B * w, dst.data_ptr() + 4 * s * n * w
                sg.rows, sg.cols, sg.dst_rows = B, w, n
        return segs

    def _export(self, store, res):
        """the export's descriptor for one epoch (idx is set per batch): the store's device tables, the result's six tensors"""
        e = _lib.AttnExport()
        for k, m in enumerate(MODS):
            e.start[k], e.length[k] = ptr(store.start_d[m]), ptr(store.length_d[m])
        e.n_utt = len(store)
        for s, (name, mods) in enumerate(ATTENTION):
            for j, m in enumerate(mods):
                t = res.attention[name][m]
                e.dst[s][j], e.dst_rows[s][j] = ptr(t), int(t.shape[0])
        return e

    def eval_epoch(self, store, batches, key_padding=False, embeddings=False, out=None, attention=False):
        n_store = len(store)
        # ---- host-side checks: nothing is enqueued (and nothing of `out` is touched) before all of them have passed ----
        plan, batches = checked_plan(batches, n_store)
        if store.packed['audio'].device != self.params.device:
            raise _lib.SdumcError("eval_epoch: the store and the parameters live on different devices")
        inplace = self._in_place(store)
        if not inplace and store.packed['audio'].dtype != self.feature_dtype:
            raise _lib.SdumcError("eval_epoch: gathering needs a store that holds the features in the storage mode's dtype "
                                  "(a bf16 store for bf16 storage, an fp32 store otherwise)")
        if tuple(store.get_featdim()) != self._fdims:
            raise _lib.SdumcError(f"eval_epoch: the store's feature widths {store.get_featdim()} are not {self._fdims}")
        rows = attention_rows(store) if attention else None
        if attention and min(rows.values()) < 1:
            raise _lib.SdumcError("eval_epoch: attention=True needs a store with at least one frame per modality")
        if out is not None and not (isinstance(out, EvalResult) and out.fits(n_store, self.params.device, embeddings, attention, rows)):
            raise _lib.SdumcError("eval_epoch: out= is not a result of this store's size, device, embeddings and attention setting")
        if plan is None:
            plan = store.plan_epoch(batches)
        shapes = set(plan.shapes)
        need = max(self._shape(s)[1] for s in shapes)
        Bmax, Tmax = max(B for B, _ in shapes), tuple(max(T[i] for _, T in shapes) for i in range(4))
        # ---- memory ----
        a = self.arena
        if a is None or not a.fits(Bmax, Tmax, need):
            if a is not None:
                Bmax, Tmax, need = max(Bmax, a.B), tuple(max(t, c) for t, c in zip(Tmax, a.T)), max(need, a.workspace.numel())
            a = self.arena = _EvalArena(self.params.device, Bmax, Tmax, self._fdims, self.feature_dtype, need)
        planes = False
        if not inplace and store.packed_p3 is not None and self._planes_ok:
            a.ensure_planes()
            planes = True
        res = (out if out is not None else EvalResult.empty(n_store, self.params.device, embeddings, attention, rows)).reset()
        ios = [self._io(store, k, inplace, planes, key_padding) for k in range(2)]
        exp = self._export(store, res) if attention else None
        segs, mark, st = {}, ptr(res.seen), _lib.current_stream()
        # ---- the epoch: no host synchronisation from here on ----
        n = len(plan)
        g = self._desc(store, plan, 0, inplace, planes, key_padding)
        check(lib.sdumc_gather_batch(C.byref(g), 0, st), "sdumc_gather_batch")
        nxt = self._shape(plan.shapes[0])[0]
        for i in range(n):
            d, io, B = nxt, ios[i & 1], plan.shapes[i][0]
            sg = segs.get(B)
            if sg is None:
                sg = segs[B] = self._segments(res, B, embeddings)
            pf = None
            if i + 1 < n:
                nxt = self._shape(plan.shapes[i + 1])[0]
                pf = self._desc(store, plan, i + 1, inplace, planes, key_padding)
            io.prefetch = C.addressof(pf) if pf is not None else None
            try:
                check(lib.sdumc_net_forward(C.byref(d), C.byref(io), st), "sdumc_net_forward")
            finally:
                io.prefetch = None
            if exp is not None:      # (the workspace holds this batch's weights until the next forward into it)
                exp.idx = plan.idx_ptr(i)
                check(lib.sdumc_net_export_attention(C.byref(d), C.byref(io), C.byref(exp), st), "sdumc_net_export_attention")
            check(lib.sdumc_scatter_rows_multi(sg, len(sg), plan.idx_ptr(i), B, mark, st), "sdumc_scatter_rows_multi")
        self._keep_plan = plan      # (the index tensor must outlive the enqueued gathers and scatters)
        return res


_evaluator = None      # eval_epoch's state: ONE evaluator (the last parameter buffer / mode asked for), so its arena is kept across epochs


def eval_epoch(flat_params, dims, store, batches, *, bf16=False, key_padding=False, embeddings=False, inplace=True, out=None,
               prefetch_workgroups=0, attention=False):
    """One evaluation pass over `batches` (index vectors into `store`, or a data.EpochPlan -- any subset of the store, any order, no
    index twice) with the parameters `flat_params`: both streams in eval mode, -> EvalResult in store order.
    bf16: the storage mode, as engine.TrainStep; key_padding=True hands the valid frame counts to the attention poolings (extension,
    default off = the reference); embeddings=True also keeps the four embeddings of each stream; inplace=False gathers padded copies
    even where the store could be read in place; out= reuses a previous result's tensors.
    attention=True also keeps the attention maps (EvalResult.attention, EvalResult.attention_of): per stream and modality one
    [frames of the store, 8] tensor -- column 0 FRA2UTT_new's softmax-over-time weight of the frame, columns 1..7 Cross_Attention's
    seven (fused, at, tv, av, audio, text, video) -- written by one more launch per batch; with attention=False the epoch enqueues
    exactly what it did without the option.  With key_padding=False (the reference) the softmax runs over the batch's PADDED
    length and the padded frames take part: an utterance's weights then depend on the batch it was evaluated in and sum to at most
    1 over its valid frames -- what the reference's vector_attention[:, :len] would show.  With key_padding=True they sum to 1 and
    do not depend on the batch."""
    global _evaluator
    dims = tuple(int(d) for d in dims)
    key = (flat_params.data_ptr(), flat_params.device, dims, engine.bf16_mode(bf16, dims), bool(inplace), int(prefetch_workgroups))
    if _evaluator is None or _evaluator[0] != key:
        _evaluator = (key, Evaluator(flat_params, dims, bf16=bf16, inplace=inplace, prefetch_workgroups=prefetch_workgroups))
    return _evaluator[1].eval_epoch(store, batches, key_padding=key_padding, embeddings=embeddings, out=out, attention=attention)


def missing_curve(runner, store, batches, rates, modalities=('audio', 'video'), kind='frame', seed=0, draw=0, key_padding=False):
    """The random-missing evaluation protocol: the metrics of both streams at every rate of `rates`, with the frames (kind='frame') or
    the whole utterances (kind='modality') of `modalities` absent at that rate -- one eval_epoch per rate over store.with_missing views
    of the SAME store (no second copy of it, no feature byte rewritten; data.DeviceFeatureStore.with_missing has the rule).
    runner: a FusedTrainer or an Evaluator (anything with their eval_epoch).  -> [{'rate', 'full': metrics, 'missing': metrics}, ...]
    in the order of `rates` (EvalResult.metrics); the entry of rate 0 is eval_epoch on the plain store.  The same (seed, draw) at every
    rate: a frame absent at one rate is absent at every higher one."""
    if kind not in ('frame', 'modality'):
        raise _lib.SdumcError(f"missing_curve: kind must be 'frame' or 'modality', not {kind!r}")
    if isinstance(modalities, str):
        modalities = (modalities,)
    base = getattr(store, 'base', store)
    views = [base.with_missing(**{kind: {m: r for m in modalities}}, seed=seed, draw=draw) for r in rates]      # (validated up front)
    from .data import EpochPlan
    plan = batches if isinstance(batches, EpochPlan) else base.plan_epoch(batches)      # (one upload for all the rates)
    curve, res = [], None
    for rate, view in zip(rates, views):
        res = runner.eval_epoch(view, plan, key_padding=key_padding, out=res)
        curve.append({'rate': float(rate), **res.metrics(base)})
    return curve
