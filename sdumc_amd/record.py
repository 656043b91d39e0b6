"""The record of a training epoch over a resident feature store (FusedTrainer.train_epoch): what the reference's training pass returns
beside the updated model.  main_frame_val_text_missing.py:333-353 runs train_or_eval_model three times per epoch; the training pass is
the same function as the evaluation passes: it appends every batch's TRAIN-mode predictions of both streams (:156-158), returns them
with their MSE (:160-178) and the driver prints train_val_mse_full / train_val_mse_missing once per epoch (:348).  The inference variant
keeps the four embeddings in either mode (main_frame_val_text_missing_inference.py:166-175).

After every step ONE call (sdumc_epoch_record, csrc/epoch_record.hip: one launch, two with grad_norm) files the step away: its stream-major outputs go to the rows
the batch's utterances have in the store (as evaluate.eval_epoch's scatter does), and a 12-float log row takes the step's loss vector,
the L2 norm of its raw gradient bucket and the number of non-finite gradient elements (grad_norm=True), the batch size and the learning
rate.  Nothing crosses to the host inside the loop and nothing of the step is written: a run is bit for bit the same with or without
the record.  The metrics stay on the host (TrainRecord.results / .summary): [N] vectors and the [steps, 12] log cross once per epoch.

BY TENSOR (train_epoch(by_tensor=True | 'updates'), TensorNorms): the one norm says that a step went bad, not where -- the bucket holds
83 tensors from 1 element to 256 x 4096, and the frame projections dominate its norm.  One more call per step (sdumc_tensor_norms,
csrc/tensor_norms.hip: two launches, fp64, fixed order, no atomics) cuts the same raw bucket at ParamLayout's offsets: a gradient norm
and a non-finite count per tensor and step.  'updates': a second call over the flat parameters against a snapshot the record owns (one
device copy in front of the first step, rolled forward by the call itself) gives each tensor's weight norm after the step and the norm
of the step's actual update, Adam's coupled L2 term included.  Read-only towards the step like the rest of the record.
tensor_norms(tensors) is the same entry for a loop that keeps per-parameter .grad tensors."""
import numpy as np
import torch

from . import _lib
from ._lib import lib
from .epoch import StoreOrdered

LOG_COLS = _lib.LOG_COLS
# columns 0..7 of a log row: the step's loss vector (sdumc_step_cfg.losses).  Entries 3..5 hold the chosen distillation criterion's
# values for the text_hidden, cross_text and fused pairs, entry 6 the chosen contrastive criterion's, entry 7 is not used by the step.
# Entries 1..2 ("mse_full", "mse_missing": the names stay) hold the chosen regression criterion's values (regress='mse' | 'l1' | 'huber'
# | 'ccc'); train_val_mse_* are computed from the predictions and are the MSE whatever the criterion.
LOSS_NAMES = ("total", "mse_full", "mse_missing", "distill_text", "distill_query", "distill_fused", "contrast", "unused")
COL_GRAD_NORM, COL_NONFINITE, COL_B, COL_LR = 8, 9, 10, 11


BY_TENSOR_MODES = (False, True, "updates")


def by_tensor_mode(by_tensor):
    """False | True | 'updates' as given, or SdumcError: the one place the option's values are checked"""
    if by_tensor is None:
        by_tensor = False
    if not any(by_tensor is m for m in BY_TENSOR_MODES[:2]) and by_tensor != "updates":
        raise _lib.SdumcError(f"by_tensor={by_tensor!r}: expected False, True or 'updates'")
    return by_tensor


def layout_segments(layout):
    """(names, offsets, counts) of the live tensors of an engine.ParamLayout, in table order: the segments of a gradient bucket or of
    the first layout.live floats of the flat parameters.  The offsets are READ from the table, not supposed to be multiples of 4."""
    names = tuple(layout.live_names())
    offs = tuple(int(layout.entries[k][0]) for k in names)
    counts = tuple(int(np.prod(layout.entries[k][1], dtype=np.int64)) for k in names)
    if any(o < 0 or o + c > layout.live for o, c in zip(offs, counts)):
        raise _lib.SdumcError("ParamLayout: a live tensor lies outside the first `live` floats")
    return names, offs, counts


class NormTable:
    """The host tables of sdumc_tensor_norms over tensors given as (x address, y address or None, count): calls of at most
    TENSOR_NORMS_MAX_SEGS segments each (one call for a ParamLayout's 83), kept by a caller that measures the same tensors again and
    again.  scratch_bytes: what the largest call needs (the calls are stream-ordered: they share one scratch)."""

    def __init__(self, triples):
        triples = list(triples)
        if not triples:
            raise _lib.SdumcError("tensor norms: no tensor given")
        cap = _lib.TENSOR_NORMS_MAX_SEGS
        self.n, self.calls, self.scratch_bytes = len(triples), [], 0
        for c0 in range(0, self.n, cap):
            part = triples[c0:c0 + cap]
            segs = (_lib.NormSeg * len(part))()
            for sg, (x, y, count) in zip(segs, part):
                sg.x, sg.y, sg.count = x or None, y or None, int(count)
            nb = int(lib.sdumc_tensor_norms_scratch_bytes(segs, len(part)))
            if nb == 0:
                raise _lib.SdumcError("sdumc_tensor_norms_scratch_bytes refused the segment table (a negative count, a misaligned address)")
            self.calls.append((segs, len(part), c0))
            self.scratch_bytes = max(self.scratch_bytes, nb)

    def launch(self, norm_ptr, nonfinite_ptr, diff_ptr, scratch, stream):
        """the rows at norm_ptr / nonfinite_ptr / diff_ptr (addresses of n consecutive fp32 / int32 / fp32; diff_ptr 0 without a y)"""
        for segs, n, c0 in self.calls:
            _lib.check(lib.sdumc_tensor_norms(segs, n, norm_ptr + 4 * c0, nonfinite_ptr + 4 * c0, diff_ptr + 4 * c0 if diff_ptr else None,
                                              _lib.ptr(scratch), scratch.numel(), stream), "sdumc_tensor_norms")


def tensor_norms(tensors):
    """The L2 norm and the non-finite count of every tensor of a list of fp32 CUDA tensors on one device, e.g.
    [p.grad for p in model.parameters() if p.grad is not None] -> (norms [n] fp32, nonfinite [n] int32), device tensors.  Two launches
    on the current stream for up to 96 tensors (two more per further 96), no synchronisation; fp64 inside, the same bits on every call
    (sdumc_tensor_norms).  CPU tensors, other dtypes and non-contiguous tensors raise SdumcError: there is no fallback."""
    tensors = list(tensors)
    if not tensors:
        raise _lib.SdumcError("tensor_norms: no tensor given")
    for t in tensors:
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.SdumcError("tensor_norms: expected contiguous fp32 CUDA tensors (there is no CPU fallback)")
        if t.device != tensors[0].device:
            raise _lib.SdumcError("tensor_norms: the tensors are on different devices")
    dev = tensors[0].device
    table = NormTable((t.data_ptr(), None, t.numel()) for t in tensors)
    with torch.cuda.device(dev):
        norms = torch.empty(table.n, device=dev)
        bad = torch.empty(table.n, dtype=torch.int32, device=dev)
        scratch = torch.empty(table.scratch_bytes, dtype=torch.uint8, device=dev)
        table.launch(norms.data_ptr(), bad.data_ptr(), 0, scratch, _lib.current_stream())
    return norms, bad


class TensorNorms:
    """TrainRecord.by_tensor: the epoch's record by tensor.  names = ParamLayout.live_names() (offsets / counts: where each lies in the
    bucket); row i = step i of grad_norm [capacity, n] fp32 (the L2 norm of each tensor's raw gradient) and grad_nonfinite
    [capacity, n] int32 (its NaN / Inf elements); with 'updates' also param_norm (each tensor's weights AFTER the step), update_norm
    (the step's actual update, theta_after - theta_before, Adam's coupled L2 term included) and param_nonfinite, else None.  Rows
    from `steps` on hold NaN (0 for the counts).  The record owns the reduce's scratch and the parameter snapshot; no step memory is
    written.  Device or CPU tensors."""

    def __init__(self, names, offsets, counts, grad_norm, grad_nonfinite, param_norm=None, update_norm=None, param_nonfinite=None,
                 steps=0, scratch=None, snapshot=None):
        self.names, self.offsets, self.counts = tuple(names), tuple(offsets), tuple(counts)
        self.grad_norm, self.grad_nonfinite = grad_norm, grad_nonfinite
        self.param_norm, self.update_norm, self.param_nonfinite = param_norm, update_norm, param_nonfinite
        self.steps, self.scratch, self.snapshot = int(steps), scratch, snapshot

    @property
    def mode(self):
        return "updates" if self.update_norm is not None else True

    @classmethod
    def empty(cls, layout, n_steps, device, updates=False):
        names, offs, counts = layout_segments(layout)
        n, cap = len(names), int(n_steps)
        nb = NormTable((8, None, c) for c in counts).scratch_bytes      # (the scratch depends on the counts alone)
        f = lambda: torch.empty(cap, n, device=device)
        i = lambda: torch.empty(cap, n, dtype=torch.int32, device=device)
        extra = (f(), f(), i()) if updates else (None, None, None)
        # 4 floats more than the parameters: train_epoch takes the view that sits like the parameters within 16 bytes
        snap = torch.empty(layout.live + 4, device=device) if updates else None
        return cls(names, offs, counts, f(), i(), *extra, 0, torch.empty(nb, dtype=torch.uint8, device=device), snap)

    def fits(self, layout, n_steps, device, updates):
        dev = torch.device(device)
        ts = [self.grad_norm, self.grad_nonfinite] + ([self.param_norm, self.update_norm, self.param_nonfinite] if updates else [])
        return ((self.update_norm is not None) == bool(updates) and (self.names, self.offsets, self.counts) == layout_segments(layout)
                and all(t is not None and t.dim() == 2 and t.shape[1] == len(self.names) and t.shape[0] >= n_steps
                        and t.device == dev and t.is_contiguous() for t in ts)
                and self.scratch is not None and self.scratch.device == dev
                and (not updates or (self.snapshot is not None and self.snapshot.numel() == layout.live + 4)))

    def reset(self):
        for t in (self.grad_norm, self.param_norm, self.update_norm):
            if t is not None:
                t.fill_(float("nan"))
        for t in (self.grad_nonfinite, self.param_nonfinite):
            if t is not None:
                t.zero_()
        self.steps = 0
        return self

    def update_ratio(self):
        """update_norm / param_norm of rows [0, steps), float64 on the host [steps, n]: is each layer's update a sane fraction of its
        weights?  (a tensor of all-zero weights gives inf, or NaN where its update is zero too)"""
        if self.update_norm is None:
            raise _lib.SdumcError("TensorNorms.update_ratio: the epoch ran without by_tensor='updates'")
        u = self.update_norm[:self.steps].cpu().numpy().astype(np.float64)
        p = self.param_norm[:self.steps].cpu().numpy().astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return u / p

    def first_nonfinite(self):
        """(step, tensor name) of the first gradient tensor, in step and then table order, that held a NaN / Inf element or whose norm
        is not finite (an overflow of the fp32 range); None when every recorded step is clean"""
        g = self.grad_norm[:self.steps].cpu().numpy()
        bad = (self.grad_nonfinite[:self.steps].cpu().numpy() != 0) | ~np.isfinite(g)
        hit = np.argwhere(bad)
        return None if hit.shape[0] == 0 else (int(hit[0, 0]), self.names[int(hit[0, 1])])


class TrainRecord(StoreOrdered):
    """One training epoch's record.  log [capacity, 12]: row i = step i (columns 0..7 the loss vector as the step wrote it, 8 grad_norm,
    9 non-finite gradient elements, 10 B, 11 learning rate; 8 is NaN and 9 is 0 when the epoch ran without grad_norm); steps = the rows
    the last epoch filled.  In STORE order, as evaluate.EvalResult: preds [2, N] (row 0 the full stream, row 1 the text-missing one,
    train-mode values: dropout on, parameters as they were BEFORE the step's update), seen [N], embeddings None or the four tensors of
    evaluate.EMBEDDINGS.  Rows not visited, and log rows from `steps` on, hold NaN.  Device or CPU tensors.
    scratch: the gradient reduce's device scratch (None without grad_norm): the record owns it, no step workspace is written.
    by_tensor: None, or the TensorNorms of an epoch that ran with by_tensor=True | 'updates'.
    guard: None, or [capacity, 4] of a trainer with clip_norm / skip_nonfinite: row i = step i's guard vector (sdumc_grad_guard: the
    bucket's L2 norm BEFORE clipping, the clip coefficient, its non-finite elements, 1 when the step was skipped).  With clipping on,
    the log's grad_norm column and by_tensor see the bucket AFTER scaling."""

    def __init__(self, log, preds, seen, embeddings=None, steps=0, scratch=None, n_grads=0, by_tensor=None, guard=None):
        self.guard = guard
        self.log, self.preds, self.seen, self.embeddings = log, preds, seen, embeddings
        self._steps, self.scratch, self.n_grads, self.by_tensor = int(steps), scratch, int(n_grads), by_tensor
        self.steps = steps

    @property
    def steps(self):
        return self._steps

    @steps.setter
    def steps(self, k):      # (the rows the last epoch filled: of the log and of the record by tensor alike)
        self._steps = int(k)
        if self.by_tensor is not None:
            self.by_tensor.steps = int(k)

    @classmethod
    def empty(cls, n, n_steps, device, embeddings=False, n_grads=0, by_tensor=False, layout=None, guard=False):
        """n utterances, room for n_steps steps; n_grads > 0: with the scratch of a gradient bucket of that many floats;
        by_tensor=True | 'updates' (with layout, the run's engine.ParamLayout): with the record by tensor (TensorNorms);
        guard=True: with the [n_steps, 4] guard column"""
        scratch = bt = None
        mode = by_tensor_mode(by_tensor)
        if mode:
            if layout is None:
                raise _lib.SdumcError("TrainRecord.empty: by_tensor needs layout= (the run's ParamLayout)")
            bt = TensorNorms.empty(layout, n_steps, device, updates=mode == "updates")
        if n_grads > 0:
            scratch = torch.zeros(int(lib.sdumc_epoch_record_scratch_bytes(int(n_grads))), dtype=torch.uint8, device=device)
        return cls(torch.empty(int(n_steps), LOG_COLS, device=device), *cls._empty(n, device, embeddings), 0, scratch,
                   n_grads if n_grads > 0 else 0, bt,
                   torch.empty(int(n_steps), 4, device=device) if guard else None)

    def fits(self, n, n_steps, device, embeddings, n_grads=0, by_tensor=False, layout=None, guard=False):
        dev = torch.device(device)
        if (self.guard is not None) != bool(guard):
            return False
        if guard and not (self.guard.dim() == 2 and self.guard.shape[1] == 4 and self.guard.shape[0] >= n_steps
                          and self.guard.device == dev and self.guard.is_contiguous() and self.guard.dtype == torch.float32):
            return False
        mode = by_tensor_mode(by_tensor)
        if (self.by_tensor is not None) != bool(mode):
            return False
        if mode and (layout is None or not self.by_tensor.fits(layout, n_steps, device, mode == "updates")):
            return False
        return (self._fits(n, dev)
                and self.log.dim() == 2 and self.log.shape[1] == LOG_COLS and self.log.shape[0] >= n_steps and self.log.device == dev
                and self.log.is_contiguous() and (self.embeddings is not None) == bool(embeddings)
                and max(0, int(n_grads)) == self.n_grads)

    def reset(self):
        """NaN everywhere -- unused log rows included --, nothing seen, no step filled: once per epoch, in front of its first step"""
        self._reset(self.log, *(() if self.guard is None else (self.guard,)))
        if self.by_tensor is not None:
            self.by_tensor.reset()
        self.steps = 0
        return self

    def skipped_steps(self):
        """The steps the non-finite guard skipped (guard[:, 3] != 0 over rows [0, steps)), a list of step indices; one device -> host copy"""
        if self.guard is None:
            raise _lib.SdumcError("TrainRecord.skipped_steps: the epoch ran without clip_norm / skip_nonfinite")
        return np.flatnonzero(self.guard[:self.steps, 3].cpu().numpy() != 0).tolist()

    def summary(self):
        """The epoch in a few numbers, float64 on the host from log[:steps] (one copy): the B-weighted mean of each of the 8 loss entries
        under LOSS_NAMES (the MSE entries are batch means, so their weighted means are the epoch's means over utterances),
        grad_norm_max and grad_norm_last (NaN when the epoch ran without grad_norm; a NaN norm propagates into the maximum),
        nonfinite_steps (the steps whose gradient bucket held a NaN / Inf or whose loss entries are not all finite), steps, samples;
        with the record by tensor also first_nonfinite (TensorNorms.first_nonfinite: (step, tensor name) or None)."""
        if self.steps < 1:
            raise _lib.SdumcError("TrainRecord: no step was recorded")
        log = self.log[:self.steps].cpu().numpy().astype(np.float64)
        w = log[:, COL_B]
        out = {name: float((log[:, k] * w).sum() / w.sum()) for k, name in enumerate(LOSS_NAMES)}
        norms = log[:, COL_GRAD_NORM]
        out["grad_norm_max"], out["grad_norm_last"] = float(np.max(norms)), float(norms[-1])
        bad = (log[:, COL_NONFINITE] != 0) | ~np.isfinite(log[:, :8]).all(axis=1)
        out["nonfinite_steps"] = np.flatnonzero(bad).tolist()
        out["steps"], out["samples"] = self.steps, int(w.sum())
        if self.by_tensor is not None:
            out["first_nonfinite"] = self.by_tensor.first_nonfinite()
        return out
