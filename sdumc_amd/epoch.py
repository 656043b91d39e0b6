"""An epoch over a resident data.DeviceFeatureStore: the ONE definition of what the training pass (engine.FusedTrainer.run_epoch /
train_epoch), the evaluation pass (evaluate.Evaluator.eval_epoch) and the saliency pass (saliency.Saliency.saliency_epoch) share.

The loop (`run`): the epoch's index vectors are uploaded once (data.EpochPlan), batch 0 is assembled in front of the first call, and
from then on the call of batch i -- a fused step or a forward -- carries the assembly of batch i + 1 into the other of two input sets
on its background lane (sdumc_net_io.prefetch, `with_prefetch`).  With a store that can be read in place (`in_place`) no padded copy of
a batch exists: the assembly writes row maps only (`gather_desc`).  Nothing crosses to the host inside the loop.

Around it: the host-side check of an epoch's indices (`checked_plan`), the scatter table that moves a batch's stream-major outputs to
the rows its utterances have in the store (`scatter_segments`), and the base of the results kept in store order (`StoreOrdered`)."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import lib, check

D, H, NQ, RNC_DIM = _lib.D, _lib.H, _lib.NQ, _lib.RNC_DIM
# the forward's outputs beside vals, in sdumc_net_io's order: name, trailing shape, (full, missing) keys of checkpoint.run_inference
EMBEDDINGS = (("fused", (H,), ("full_rep", "missing_rep")),
              ("rnc", (RNC_DIM,), ("full_rnc", "missing_rnc")),
              ("text_hidden", (D,), ("text_rep_query_full", "text_rep_query_missing")),
              ("cross_text", (NQ, H), ("text_rep_full", "text_rep_missing")))
OUT_WIDTHS = (1,) + tuple(math.prod(shape) for _, shape, _ in EMBEDDINGS)      # floats per row of the five outputs
MODS = ("audio", "text", "video", "feat4")


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


def in_place(inplace, feature_dtype, planes_ok, dims, store):
    """Whether batches of `store` are read in place -- not copied at all: the call reads the store's packed tensors through row maps.
    fp32 storage and a store with planes (planes_ok: the reader's mode has planes), or bf16 storage and a bf16 store (widths in whole
    128-element tiles); never with inplace=False."""
    if not inplace:
        return False
    if feature_dtype == torch.bfloat16:
        return store.packed['audio'].dtype == torch.bfloat16 and all(int(d) % 128 == 0 for d in dims[:3])
    return store.packed_p3 is not None and planes_ok


def gather_desc(store, idx_ptr, B, T, st, key_padding, planes, inplace):
    """The sdumc_gather_batch descriptor that assembles the batch (idx_ptr, B, T) in input set `st` (engine._InputSet): its row maps
    when the store is read in place, else its padded copies (and their planes); labels always, valid frame counts with key_padding."""
    lens = st.lengths if key_padding else None
    if inplace:
        return store.gather_desc(idx_ptr, B, T, None, st.labels, lens, maps_out=st.ensure_maps())
    return store.gather_desc(idx_ptr, B, T, st.inputs, st.labels, lens, st.planes if planes else None)


def with_prefetch(io, desc, call, *args):
    """call(*args) -- the entry that reads `io` -- with io.prefetch naming `desc` (a gather_desc, or None) for that call alone: the
    ONLY code that writes the field (the descriptor lives as long as the caller's reference: the field holds a bare address)."""
    io.prefetch = C.addressof(desc) if desc is not None else None
    try:
        return call(*args)
    finally:
        io.prefetch = None


def run(owner, store, plan, sets, key_padding, planes, inplace, per_shape, bind, enqueue, tail):
    """Every batch of `plan` (a data.EpochPlan), in order, alternating between the two input sets `sets`.
    per_shape(B, T) -> what the caller keeps per batch shape (a TrainStep, an sdumc_net_dims), made ONE batch ahead: the host runs
    ahead of the device anyway, so a shape seen for the first time costs no device time; bind(that, k) -> the same bound to input set k;
    enqueue(bound, next, desc): the call of the batch, which carries `desc`, the assembly of the next one (next = its per-shape
    object; both None after the last batch); tail(i, bound), or None: whatever else the caller enqueues for batch i.  -> the number
    of batches.  `owner` keeps the plan: the index tensor must outlive the enqueued gathers and scatters.
    (The callables are called as they are, once per batch each: a bound method costs the host less than a closure around it.)"""
    n = len(plan)
    nxt = per_shape(*plan.shapes[0])
    g = gather_desc(store, plan.idx_ptr(0), *plan.shapes[0], sets[0], key_padding, planes, inplace)
    check(lib.sdumc_gather_batch(C.byref(g), 0, _lib.current_stream()), "sdumc_gather_batch")
    for i in range(n):
        cur = bind(nxt, i & 1)
        nxt = pf = None
        if i + 1 < n:
            nxt = per_shape(*plan.shapes[i + 1])
            pf = gather_desc(store, plan.idx_ptr(i + 1), *plan.shapes[i + 1], sets[(i + 1) & 1], key_padding, planes, inplace)
        enqueue(cur, nxt, pf)
        if tail is not None:
            tail(i, cur)
    owner._keep_plan = plan
    return n


def scatter_segments(outs, res, B, embeddings):
    """The store-ordered scatter table of batches of B: rows [0, B) of the outputs `outs` (an arena's five [2 B, w] buffers) to stream
    0's rows of res.preds (and, with embeddings, of res.embeddings), rows [B, 2 B) to stream 1's -> an array of sdumc_scatter_seg."""
    dsts = [res.preds] + ([res.embeddings[name] for name, _, _ in EMBEDDINGS] if embeddings else [])
    n = res.preds.shape[1]
    segs = (_lib.ScatterSeg * (2 * len(dsts)))()
    for j, (src, dst, w) in enumerate(zip(outs, dsts, OUT_WIDTHS)):
        for s in range(2):
            sg = segs[2 * j + s]
            sg.src, sg.dst = src.data_ptr() + 4 * s * B * w, dst.data_ptr() + 4 * s * n * w
            sg.rows, sg.cols, sg.dst_rows = B, w, n
    return segs


def rows_dict(rows):
    """{modality: packed rows} from such a dictionary or from the four row counts (audio / text / video / feat4)"""
    if rows is None:
        raise _lib.SdumcError("EvalResult: attention=True needs rows= (evaluate.attention_rows(store), or the four row counts)")
    if not isinstance(rows, dict):
        rows = dict(zip(MODS, rows))
    return {m: int(rows[m]) for m in MODS}


class StoreOrdered:
    """Base of the results kept in STORE order (row i = utterance i of the store): preds [2, N] (row 0 the full stream, row 1 the
    text-missing one), seen [N] (uint8 / bool: visited this epoch), embeddings None or the four tensors of EMBEDDINGS [2, N, ...].
    Rows not visited hold NaN.  Error messages carry the subclass's name."""

    embeddings = None

    @staticmethod
    def _empty(n, device, embeddings=False):
        """(preds, seen, embeddings or None), uninitialised"""
        emb = {name: torch.empty((2, n) + shape, device=device) for name, shape, _ in EMBEDDINGS} if embeddings else None
        return torch.empty(2, n, device=device), torch.empty(n, dtype=torch.uint8, device=device), emb

    def _fits(self, n, device):
        return (self.preds.shape == (2, n) and self.preds.device == torch.device(device) and self.seen.numel() == n
                and self.seen.element_size() == 1)

    def _frames_fit(self, maps, streams, rows, cols, device):
        """maps {stream: {modality: tensor}} holds a contiguous fp32 [rows[m], cols] on `device` for every (stream, modalities) pair"""
        return all(s in maps and m in maps[s] and maps[s][m].shape == (rows[m], cols) and maps[s][m].device == torch.device(device)
                   and maps[s][m].dtype == torch.float32 and maps[s][m].is_contiguous() for s, mods in streams for m in mods)

    def _reset(self, *more):
        """NaN in preds, the embeddings and the tensors `more`, nothing seen"""
        self.seen.zero_()
        for t in (self.preds, *(self.embeddings or {}).values(), *more):
            t.fill_(float("nan"))
        return self

    def _visited(self):
        rows = np.flatnonzero(self.seen.cpu().numpy().reshape(-1) != 0)
        if rows.size == 0:
            raise _lib.SdumcError(f"{type(self).__name__}: no row was visited")
        return rows

    def _frames_of(self, store, i, maps):
        """The rows of ONE visited utterance -- i = its index in the store, or its name -- of every per-frame tensor of `maps`
        {stream: {modality: [rows_m, c]}}, as views sliced by the store's start / length tables."""
        who = type(self).__name__
        if isinstance(i, str):
            try:
                i = store.names.index(i)
            except ValueError:
                raise _lib.SdumcError(f"{who}: no utterance named {i!r} in the store") from None
        i = int(i)
        if not 0 <= i < self.seen.numel():
            raise _lib.SdumcError(f"{who}: utterance index {i} out of range [0, {self.seen.numel()})")
        if int(self.seen.reshape(-1)[i]) == 0:
            raise _lib.SdumcError(f"{who}: utterance {i} was not visited in this epoch")
        return {s: {m: t[int(store.start[m][i]):int(store.start[m][i]) + int(store.length[m][i])] for m, t in d.items()}
                for s, d in maps.items()}

    def results(self, store):
        """The dictionary the reference's passes return (main :168-175) over the visited rows in store order: val_mse_full,
        val_mse_missing, val_preds_full [n, 1], val_preds_missing [n, 1], val_labels, names (from store.names; labels from store.vals);
        with embeddings also checkpoint.run_inference's embedding keys.  One device -> host copy per tensor."""
        rows = self._visited()
        preds = self.preds.cpu().numpy()
        labels = torch.as_tensor(store.vals).cpu().numpy().astype(np.float32).reshape(-1)[rows]
        out = {"val_preds_full": preds[0][rows].reshape(-1, 1), "val_preds_missing": preds[1][rows].reshape(-1, 1),
               "val_labels": labels}
        for name, _, keys in EMBEDDINGS if self.embeddings is not None else ():
            t = self.embeddings[name].cpu().numpy()
            out[keys[0]], out[keys[1]] = t[0][rows], t[1][rows]
        out["names"] = [store.names[i] for i in rows.tolist()]
        out["val_mse_full"] = float(np.mean((labels - out["val_preds_full"].reshape(-1)) ** 2))
        out["val_mse_missing"] = float(np.mean((labels - out["val_preds_missing"].reshape(-1)) ** 2))
        return out
