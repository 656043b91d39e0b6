"""Evaluation epochs over a resident feature store: the validation and test passes of the reference driver
(main_frame_val_text_missing.py:333-353 calls train_or_eval_model three times per epoch; :151-166 is the eval branch -- both streams,
no_grad, model.eval(); main_frame_val_text_missing_inference.py:100-215 is the same loop with the embeddings kept).

`eval_epoch` is to those passes what FusedTrainer.run_epoch is to the training pass, and runs the same loop (epoch.run has its
definition): the call of batch i is forward i (sdumc_net_forward, train = 0, both streams in one call: the audio / video frame
projections run once).  After every forward ONE launch (sdumc_scatter_rows_multi) moves the batch's stream-major outputs to the rows
its utterances have in the store, so the results line up with store.names / store.vals whatever order the sampler used.  The metrics
stay on the host (metric.py): [N] vectors cross once per epoch.

Evaluation owns its device memory (an engine._Arena): workspace, outputs, two sets of row maps / labels / lengths (and input buffers
when batches are gathered).  It reads the flat parameters and nothing else of a training run -- no step workspace, no keep-bits, no
Philox counter (rng_state = NULL) -- so a training run is bit for bit the same with or without evaluation epochs in between.

attention=True keeps what the reference's inference pass plots per utterance (vector_attention of FRA2UTT_new / Cross_Attention,
model :68, :95; attention_masks, model :291; main_frame_val_text_missing_inference.py:176-181): ONE more launch per batch
(sdumc_net_export_attention, between the forward and the scatter) copies the six poolings' normalised softmax-over-time weights of
both streams out of the forward's workspace to per-frame tensors in store order (EvalResult.attention)."""
import ctypes as C

import torch

from . import _lib, engine, epoch
from ._lib import lib, check, ptr
from .epoch import EMBEDDINGS, MODS, NQ, check_epoch_indices, checked_plan      # (callers reach these through evaluate too)

# the attention maps: per stream, the modalities its three pooling pairs read (stream 1's text slot is feat4); every tensor
# [packed rows of that modality, ATTN_COLS]: column 0 FRA2UTT_new's weight, columns 1..7 Cross_Attention's in multi_query order
ATTENTION = (("full", ("audio", "text", "video")), ("missing", ("audio", "feat4", "video")))
ATTN_COLS = 1 + NQ


def attention_rows(store):
    """{modality: packed rows (frames of all utterances, without the trailing zero row)} of a store -- from its host tables"""
    return {m: int(torch.as_tensor(store.length[m]).sum()) for m in MODS}


class EvalResult(epoch.StoreOrdered):
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
        att = None
        if attention:
            rows = epoch.rows_dict(rows)
            att = {s: {m: torch.empty(rows[m], ATTN_COLS, device=device) for m in mods} for s, mods in ATTENTION}
        return cls(*cls._empty(n, device, embeddings), att)

    def fits(self, n, device, embeddings, attention=False, rows=None):
        return (self._fits(n, device) and (self.embeddings is not None) == bool(embeddings)
                and (self.attention is not None) == bool(attention)
                and (not attention or self._frames_fit(self.attention, ATTENTION, epoch.rows_dict(rows), ATTN_COLS, device)))

    def reset(self):
        """NaN everywhere, nothing seen: once per epoch, in front of its first batch"""
        return self._reset(*(t for d in (self.attention or {}).values() for t in d.values()))

    def attention_of(self, store, i):
        """The attention maps of ONE utterance -- i = its index in the store, or its name -- as views: {'full': {'audio' [T_a, 8],
        'text' [T_t, 8], 'video' [T_v, 8]}, 'missing': {'audio', 'feat4' [T_f4, 8], 'video'}}, sliced by the store's start / length
        tables.  Raises when the epoch kept no attention maps or did not visit the utterance."""
        if self.attention is None:
            raise _lib.SdumcError("EvalResult: this epoch kept no attention maps (eval_epoch(..., attention=True))")
        return self._frames_of(store, i, {s: {m: self.attention[s][m] for m in mods} for s, mods in ATTENTION})

    def results(self, store):
        """The dictionary checkpoint.run_inference returns (same keys, array shapes and embedding names), over the visited rows in
        store order, names from store.names, labels from store.vals; plus val_mse_full (main :170; = val_mse).  One device -> host
        copy per tensor."""
        out = super().results(store)
        out["val_mse"] = out["val_mse_full"]
        return out

    def metrics(self, store):
        """{'full': eval_mosei_metric(...), 'missing': ...} of the visited rows (main :366-367), on the host."""
        from .metric import eval_mosei_metric
        rows = self._visited()
        preds = self.preds.cpu().numpy()
        labels = torch.as_tensor(store.vals).cpu().numpy().reshape(-1)[rows]
        names = [store.names[i] for i in rows.tolist()]
        return {"full": eval_mosei_metric(preds[0][rows], labels, names), "missing": eval_mosei_metric(preds[1][rows], labels, names)}


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
        return epoch.in_place(self.inplace, self.feature_dtype, self._planes_ok, self.dims, store)

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

    def _bytes(self, shapes):
        """the byte sizes an arena for batches of `shapes` needs, in the order of the arena's .nbytes and of _new_arena"""
        return (max(self._shape(s)[1] for s in shapes),)

    def _new_arena(self, B, T, nbytes):
        return engine._Arena(self.params.device, B, T, self._fdims, self.feature_dtype, nbytes)

    def _io(self, store, k, inplace, planes, key_padding):
        a, st = self.arena, self.arena.sets[k]
        io = _lib.NetIO()
        if inplace:
            engine._bind_source(io, engine._store_source(store, st, st.labels))
        else:
            engine._bind_source(io, engine._Source(st.inputs, st.planes if planes else None, None, (0,) * 4, st.labels))
        io.params, io.rng_state = ptr(self.params), None
        io.workspace, io.workspace_bytes = ptr(a.workspace), a.workspace.numel()
        io.vals, io.fused, io.rnc, io.text_hidden, io.cross_text = (ptr(t) for t in a.outs)
        if key_padding:
            for i, t in enumerate(st.lengths):
                io.lengths[i] = ptr(t)
        io.prefetch_workgroups = self.prefetch_workgroups
        return io

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

    def _prepare(self, what, store, batches, out, cls, spec, spec_text):
        """The pre-flight of a read-only epoch `what` (the caller's name, for the messages): every host-side check, then the memory ->
        (plan, result after reset, read in place?, planes gathered?).  cls / spec: the result's class and what its fits / empty take
        after (n, device).  Nothing is enqueued and nothing of `out` is touched before all the checks have passed."""
        n_store, dev = len(store), self.params.device
        plan, batches = checked_plan(batches, n_store)
        if store.packed['audio'].device != dev:
            raise _lib.SdumcError(f"{what}: the store and the parameters live on different devices")
        inplace = self._in_place(store)
        if not inplace and store.packed['audio'].dtype != self.feature_dtype:
            raise _lib.SdumcError(f"{what}: gathering needs a store that holds the features in the storage mode's dtype "
                                  "(a bf16 store for bf16 storage, an fp32 store otherwise)")
        if tuple(store.get_featdim()) != self._fdims:
            raise _lib.SdumcError(f"{what}: the store's feature widths {store.get_featdim()} are not {self._fdims}")
        if out is not None and not (isinstance(out, cls) and out.fits(n_store, dev, *spec)):
            raise _lib.SdumcError(f"{what}: out= is not a result of this store's size, device, {spec_text}")
        if plan is None:
            plan = store.plan_epoch(batches)
        shapes = set(plan.shapes)
        nbytes = self._bytes(shapes)
        Bmax, Tmax = max(B for B, _ in shapes), tuple(max(T[i] for _, T in shapes) for i in range(4))
        # ---- memory: an arena too small for this epoch gives way to one that holds both (it never shrinks) ----
        a = self.arena
        if a is None or not a.fits(Bmax, Tmax, *nbytes):
            if a is not None:
                Bmax, Tmax = max(Bmax, a.B), tuple(max(t, c) for t, c in zip(Tmax, a.T))
                nbytes = tuple(max(x, y) for x, y in zip(nbytes, a.nbytes))
            a = self.arena = self._new_arena(Bmax, Tmax, *nbytes)
        planes = not inplace and store.packed_p3 is not None and self._planes_ok and a.ensure_planes()
        res = (out if out is not None else cls.empty(n_store, dev, *spec)).reset()
        return plan, res, inplace, planes

    def _run(self, store, plan, res, inplace, planes, key_padding, embeddings, middle=None):
        """epoch.run for a read-only epoch: per batch one forward, middle(i, k, d, io, stream) when given, one scatter of the forward's
        outputs to the store's rows of `res`.  No host synchronisation inside."""
        a = self.arena
        ios = [self._io(store, k, inplace, planes, key_padding) for k in range(2)]
        segs, mark, st = {}, ptr(res.seen), _lib.current_stream()

        def forward(cur, nxt, pf):
            _, d, io = cur
            check(epoch.with_prefetch(io, pf, lib.sdumc_net_forward, C.byref(d), C.byref(io), st), "sdumc_net_forward")

        def tail(i, cur):
            B = plan.shapes[i][0]
            sg = segs.get(B)
            if sg is None:
                sg = segs[B] = epoch.scatter_segments(a.outs, res, B, embeddings)
            if middle is not None:
                middle(i, *cur, st)
            check(lib.sdumc_scatter_rows_multi(sg, len(sg), plan.idx_ptr(i), B, mark, st), "sdumc_scatter_rows_multi")

        epoch.run(self, store, plan, a.sets, key_padding, planes, inplace, lambda B, T: self._shape((B, T))[0],
                  lambda d, k: (k, d, ios[k]), forward, tail)
        return res

    def eval_epoch(self, store, batches, key_padding=False, embeddings=False, out=None, attention=False):
        rows = attention_rows(store) if attention else None
        if attention and min(rows.values()) < 1:
            raise _lib.SdumcError("eval_epoch: attention=True needs a store with at least one frame per modality")
        plan, res, inplace, planes = self._prepare("eval_epoch", store, batches, out, EvalResult, (embeddings, attention, rows),
                                                   "embeddings and attention setting")
        middle = None
        if attention:
            exp = self._export(store, res)

            def middle(i, k, d, io, st):      # (the workspace holds this batch's weights until the next forward into it)
                exp.idx = plan.idx_ptr(i)
                check(lib.sdumc_net_export_attention(C.byref(d), C.byref(io), C.byref(exp), st), "sdumc_net_export_attention")
        return self._run(store, plan, res, inplace, planes, key_padding, embeddings, middle)


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
