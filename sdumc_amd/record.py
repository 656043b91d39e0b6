"""The record of a training epoch over a resident feature store (FusedTrainer.train_epoch): what the reference's training pass returns
beside the updated model.  main_frame_val_text_missing.py:333-353 runs train_or_eval_model three times per epoch; the training pass is
the same function as the evaluation passes: it appends every batch's TRAIN-mode predictions of both streams (:156-158), returns them
with their MSE (:160-178) and the driver prints train_val_mse_full / train_val_mse_missing once per epoch (:348).  The inference variant
keeps the four embeddings in either mode (main_frame_val_text_missing_inference.py:166-175).

After every step ONE call (sdumc_epoch_record, csrc/epoch_record.hip: one launch, two with grad_norm) files the step away: its stream-major outputs go to the rows
the batch's utterances have in the store (as evaluate.eval_epoch's scatter does), and a 12-float log row takes the step's loss vector,
the L2 norm of its raw gradient bucket and the number of non-finite gradient elements (grad_norm=True), the batch size and the learning
rate.  Nothing crosses to the host inside the loop and nothing of the step is written: a run is bit for bit the same with or without
the record.  The metrics stay on the host (TrainRecord.results / .summary): [N] vectors and the [steps, 12] log cross once per epoch."""
import numpy as np
import torch

from . import _lib
from ._lib import lib
from .evaluate import EMBEDDINGS

LOG_COLS = _lib.LOG_COLS
# columns 0..7 of a log row: the step's loss vector (sdumc_step_cfg.losses).  Entries 3..5 hold the chosen distillation criterion's
# values for the text_hidden, cross_text and fused pairs, entry 6 the chosen contrastive criterion's, entry 7 is not used by the step.
LOSS_NAMES = ("total", "mse_full", "mse_missing", "distill_text", "distill_query", "distill_fused", "contrast", "unused")
COL_GRAD_NORM, COL_NONFINITE, COL_B, COL_LR = 8, 9, 10, 11


class TrainRecord:
    """One training epoch's record.  log [capacity, 12]: row i = step i (columns 0..7 the loss vector as the step wrote it, 8 grad_norm,
    9 non-finite gradient elements, 10 B, 11 learning rate; 8 is NaN and 9 is 0 when the epoch ran without grad_norm); steps = the rows
    the last epoch filled.  In STORE order, as evaluate.EvalResult: preds [2, N] (row 0 the full stream, row 1 the text-missing one,
    train-mode values: dropout on, parameters as they were BEFORE the step's update), seen [N], embeddings None or the four tensors of
    evaluate.EMBEDDINGS.  Rows not visited, and log rows from `steps` on, hold NaN.  Device or CPU tensors.
    scratch: the gradient reduce's device scratch (None without grad_norm): the record owns it, no step workspace is written."""

    def __init__(self, log, preds, seen, embeddings=None, steps=0, scratch=None, n_grads=0):
        self.log, self.preds, self.seen, self.embeddings = log, preds, seen, embeddings
        self.steps, self.scratch, self.n_grads = int(steps), scratch, int(n_grads)

    @classmethod
    def empty(cls, n, n_steps, device, embeddings=False, n_grads=0):
        """n utterances, room for n_steps steps; n_grads > 0: with the scratch of a gradient bucket of that many floats"""
        emb = scratch = None
        if embeddings:
            emb = {name: torch.empty((2, n) + shape, device=device) for name, shape, _ in EMBEDDINGS}
        if n_grads > 0:
            scratch = torch.zeros(int(lib.sdumc_epoch_record_scratch_bytes(int(n_grads))), dtype=torch.uint8, device=device)
        return cls(torch.empty(int(n_steps), LOG_COLS, device=device), torch.empty(2, n, device=device),
                   torch.empty(n, dtype=torch.uint8, device=device), emb, 0, scratch, n_grads if n_grads > 0 else 0)

    def fits(self, n, n_steps, device, embeddings, n_grads=0):
        dev = torch.device(device)
        return (self.preds.shape == (2, n) and self.preds.device == dev and self.seen.numel() == n and self.seen.element_size() == 1
                and self.log.dim() == 2 and self.log.shape[1] == LOG_COLS and self.log.shape[0] >= n_steps and self.log.device == dev
                and self.log.is_contiguous() and (self.embeddings is not None) == bool(embeddings)
                and max(0, int(n_grads)) == self.n_grads)

    def reset(self):
        """NaN everywhere -- unused log rows included --, nothing seen, no step filled: once per epoch, in front of its first step"""
        self.log.fill_(float("nan"))
        self.preds.fill_(float("nan"))
        self.seen.zero_()
        for t in (self.embeddings or {}).values():
            t.fill_(float("nan"))
        self.steps = 0
        return self

    def _visited(self):
        rows = np.flatnonzero(self.seen.cpu().numpy().reshape(-1) != 0)
        if rows.size == 0:
            raise _lib.SdumcError("TrainRecord: no row was visited")
        return rows

    def results(self, store):
        """The dictionary the reference's training pass returns (main :168-175) over the visited rows in store order: val_mse_full,
        val_mse_missing, val_preds_full [n, 1], val_preds_missing [n, 1], val_labels, names -- the MSE as EvalResult.results takes it;
        with embeddings also EvalResult.results' embedding keys.  One device -> host copy per tensor."""
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

    def summary(self):
        """The epoch in a few numbers, float64 on the host from log[:steps] (one copy): the B-weighted mean of each of the 8 loss entries
        under LOSS_NAMES (the MSE entries are batch means, so their weighted means are the epoch's means over utterances),
        grad_norm_max and grad_norm_last (NaN when the epoch ran without grad_norm; a NaN norm propagates into the maximum),
        nonfinite_steps (the steps whose gradient bucket held a NaN / Inf or whose loss entries are not all finite), steps, samples."""
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
        return out
