"""Distillation targets from a STORED teacher (include/sdumc_hip.h, sdumc_teacher).

main :148 pulls the text-missing stream towards the full stream of the same step.  A TeacherTargets holds up to three device tables
in store order -- 'text_hidden' [n_rows, 256], 'cross_text' [n_rows, 7, 128], 'fused' [n_rows, 128] -- that take stream 0's place as
the target of their pair: the eval-mode embeddings of a trained full-modality checkpoint (a fixed teacher), or of the run's own averaged
weights refreshed once per epoch (a mean teacher; engine.FusedTrainer.refresh_teacher).  The loss stage's kernels read the tables
through the batch's index vector: no further launch, nothing on the host per step.

This module is the host side only: validation of the tables, and the checks of an index vector against them (`check_rows`) that every
host path runs before anything is enqueued -- the kernels answer an index outside the tables with NaN, never with a read."""
import ctypes as C

import numpy as np
import torch

from . import _lib

PAIRS = ("text_hidden", "cross_text", "fused")      # the order of losses[3:6] and of sdumc_teacher's table pointers
SHAPES = {"text_hidden": (_lib.D,), "cross_text": (_lib.NQ, _lib.H), "fused": (_lib.H,)}
STREAMS = {"full": 0, "missing": 1}


def check_rows(idx, n_rows, seen=None, what="teacher"):
    """Host-side check of an index vector (anything torch.as_tensor takes; a device tensor is copied to the host) against tables of
    n_rows rows: every index in [0, n_rows), and -- with seen, a host bool array [n_rows] -- none that names a row the teacher's
    evaluation pass did not visit (its rows hold NaN).  Raises SdumcError; returns the indices as a host int64 tensor."""
    idx = torch.as_tensor(idx).reshape(-1)
    if idx.dtype != torch.int64:
        if idx.dtype.is_floating_point or idx.dtype == torch.bool:
            raise _lib.SdumcError(f"{what}: row indices must be integers, not {idx.dtype}")
        idx = idx.to(torch.int64)
    idx = idx.cpu()
    if idx.numel() == 0:
        raise _lib.SdumcError(f"{what}: no row indices")
    lo, hi = int(idx.min()), int(idx.max())
    if lo < 0 or hi >= n_rows:
        raise _lib.SdumcError(f"{what}: row index {lo if lo < 0 else hi} outside the teacher's tables [0, {n_rows})")
    if seen is not None:
        missed = idx[torch.from_numpy(~np.asarray(seen, dtype=bool))[idx]]
        if missed.numel():
            raise _lib.SdumcError(f"{what}: utterance {int(missed[0])} was not visited by the teacher's evaluation pass "
                                  f"(its rows are NaN; {int(missed.numel())} such rows in this batch or epoch)")
    return idx


class TeacherTargets:
    """Up to three teacher tables and, optionally, which of their rows are valid.

    text_hidden / cross_text / fused: None (that pair keeps stream 0 as its target, as the step always had it) or a contiguous fp32
    tensor [n_rows, 256] / [n_rows, 7, 128] / [n_rows, 128]; every table given has the same n_rows and sits on one device.  seen:
    None (every row valid) or n_rows booleans (a tensor or array; kept on the host), False = that row holds no teacher output --
    an epoch or batch that names such a row is refused on the host.  No table at all is a valid object: a step given it runs as the
    step without a teacher, launch for launch."""

    def __init__(self, text_hidden=None, cross_text=None, fused=None, seen=None):
        self.tables = {}
        self.n_rows, self.device = None, None
        for name, t in zip(PAIRS, (text_hidden, cross_text, fused)):
            if t is None:
                continue
            if not torch.is_tensor(t) or t.dtype != torch.float32:
                raise _lib.SdumcError(f"teacher: {name} must be a float32 tensor")
            if t.dim() != 1 + len(SHAPES[name]) or tuple(t.shape[1:]) != SHAPES[name] or t.shape[0] < 1:
                raise _lib.SdumcError(f"teacher: {name} must be [n_rows, {', '.join(str(k) for k in SHAPES[name])}] with n_rows >= 1, "
                                      f"not {tuple(t.shape)}")
            if not t.is_contiguous():
                raise _lib.SdumcError(f"teacher: {name} must be contiguous")
            if self.n_rows is not None and t.shape[0] != self.n_rows:
                raise _lib.SdumcError(f"teacher: every table has the same n_rows ({name} has {t.shape[0]}, another {self.n_rows})")
            if self.device is not None and t.device != self.device:
                raise _lib.SdumcError(f"teacher: every table sits on one device ({name} on {t.device}, another on {self.device})")
            self.n_rows, self.device = int(t.shape[0]), t.device
            self.tables[name] = t
        self.seen = None
        if seen is not None:
            s = seen.detach().cpu().numpy() if torch.is_tensor(seen) else np.asarray(seen)
            s = s.reshape(-1) != 0
            if self.n_rows is not None and s.size != self.n_rows:
                raise _lib.SdumcError(f"teacher: seen has {s.size} entries for tables of {self.n_rows} rows")
            self.seen = None if bool(s.all()) else s

    @classmethod
    def from_tensors(cls, text_hidden=None, cross_text=None, fused=None, seen=None):
        return cls(text_hidden, cross_text, fused, seen)

    @classmethod
    def from_eval(cls, res, stream="full", pairs=PAIRS):
        """The tables of an evaluation pass: views (not copies) of res.embeddings[name][0] ('full') or [1] ('missing') for the pairs
        named -- res = an evaluate.EvalResult made with embeddings=True; a later pass into the same result refreshes the teacher in
        place.  res.seen is read to the host once, here."""
        if stream not in STREAMS:
            raise _lib.SdumcError(f"teacher: stream must be 'full' or 'missing', not {stream!r}")
        pairs = tuple(pairs)
        if not pairs or any(p not in PAIRS for p in pairs) or len(set(pairs)) != len(pairs):
            raise _lib.SdumcError(f"teacher: pairs must name some of {PAIRS}, each once, not {pairs!r}")
        if getattr(res, "embeddings", None) is None:
            raise _lib.SdumcError("teacher: this result kept no embeddings (eval_epoch(..., embeddings=True))")
        s = STREAMS[stream]
        return cls(**{p: res.embeddings[p][s] for p in pairs}, seen=res.seen)

    @property
    def active(self):
        return bool(self.tables)

    def check_rows(self, idx, what="teacher"):
        return check_rows(idx, self.n_rows, self.seen, what)

    def check_store(self, n_store, what="teacher"):
        if self.active and self.n_rows != n_store:
            raise _lib.SdumcError(f"{what}: the teacher's tables have {self.n_rows} rows, the store {n_store} utterances")

    def check_batch(self, B, what="teacher"):
        """a launch without an index vector: row b of the tables is sample b"""
        if self.n_rows != B:
            raise _lib.SdumcError(f"{what}: without row indices the teacher's tables are [B, ...] in batch order "
                                  f"({self.n_rows} rows for a batch of {B})")
        if self.seen is not None:
            self.check_rows(np.arange(B), what)

    def record(self, idx_ptr=None):
        """sdumc_teacher over these tables and the device int64 [B] index vector at address idx_ptr (None: row b = sample b)"""
        t = _lib.Teacher()
        for name in PAIRS:
            setattr(t, name, _lib.ptr(self.tables.get(name)))
        t.idx, t.n_rows = idx_ptr, self.n_rows or 0
        return t


def teacher_arg(teacher, device=None, what="teacher"):
    """TrainStep / FusedTrainer (teacher=) -> the TeacherTargets to use, or None: nothing else is accepted, the tables sit on the
    step's device, and a library from before the entries that take one raises."""
    if teacher is None:
        return None
    if not isinstance(teacher, TeacherTargets):
        raise _lib.SdumcError(f"{what}: a teacher.TeacherTargets or None, not {type(teacher).__name__}")
    if teacher.active:
        if not _lib.TEACHER_ABI:
            raise _lib.SdumcError("teacher: the library named by SDUMC_LIB is from before sdumc_train_step_teacher")
        if device is not None and teacher.device != torch.device(device):
            raise _lib.SdumcError(f"{what}: the teacher's tables sit on {teacher.device}, the step on {device}")
    return teacher
