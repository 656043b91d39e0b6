"""CPU-only: the host side of gradient-norm clipping and the non-finite step guard (sdumc_grad_guard, csrc/grad_guard.hip;
TrainStep / FusedTrainer(clip_norm=, skip_nonfinite=); optim.clip_grad_norm_): the validators, the ctypes mirror of the new
sdumc_step_cfg fields, the record's guard column, and the entries' refusals, which come back before any HIP call."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_validators_refuse_what_is_no_positive_finite_number():
    from sdumc_amd import _lib
    for bad in (0, 0.0, -1, -0.5, float("nan"), float("inf"), "1.0", True, False, torch.tensor(1.0), [1.0], 1e-60, 1e60):
        with pytest.raises(_lib.SdumcError, match="clip_norm"):
            _lib.guard_args(bad, False)
    for bad in (1, 0, None, "yes", torch.tensor(True)):
        with pytest.raises(_lib.SdumcError, match="skip_nonfinite"):
            _lib.guard_args(None, bad)
    assert _lib.guard_args(None, False) == (0.0, 0)
    assert _lib.guard_args(2, True) == (2.0, 1) and _lib.guard_args(0.5, False) == (0.5, 0)
    assert _lib.guard_args(1e30, False) == (1e30, 0)


def test_step_cfg_mirrors_the_header_and_defaults_to_zero():
    """the four fields sit together behind `losses`, in the header's order and types; a zeroed struct is the step without them"""
    from sdumc_amd import _lib
    names = [f[0] for f in _lib.StepCfg._fields_]
    k = names.index("losses")
    assert names[k + 1:k + 5] == ["clip_norm", "skip_nonfinite", "guard", "guard_scratch"] and names[k + 5] == "B_global"
    types = dict(_lib.StepCfg._fields_)
    assert types["clip_norm"] is C.c_float and types["skip_nonfinite"] is C.c_int32
    assert types["guard"] is C.c_void_p and types["guard_scratch"] is C.c_void_p
    z = _lib.StepCfg()
    assert z.clip_norm == 0.0 and z.skip_nonfinite == 0 and z.guard is None and z.guard_scratch is None
    header = open(os.path.join(ROOT, "include", "sdumc_hip.h")).read()
    body = header[header.index("typedef struct sdumc_step_cfg {"):header.index("} sdumc_step_cfg;")]
    decl = re.findall(r"^  [\w ]+?\*? ?(\w+)(?:\[\d+\])?;", body, flags=re.M)
    k = decl.index("losses")
    assert decl[k + 1:k + 6] == ["clip_norm", "skip_nonfinite", "guard", "guard_scratch", "B_global"]
    assert _lib.GUARD_ABI is True
    assert {"sdumc_grad_guard", "sdumc_grad_guard_scratch_bytes", "sdumc_grad_guard_multi",
            "sdumc_grad_guard_multi_scratch_bytes"} <= set(_lib.EXPORTS)


def test_constructors_take_the_options_and_refuse_bad_values_on_the_host():
    from sdumc_amd import engine, optim, trainer
    from sdumc_amd._lib import SdumcError
    for cls in (engine.TrainStep, engine.FusedTrainer):
        p = inspect.signature(cls.__init__).parameters
        assert p["clip_norm"].default is None and p["skip_nonfinite"].default is False
    flat, dims, T = torch.zeros(4), (48, 32, 40, 32), (13, 5, 9, 3)
    for kw in ({"clip_norm": 0}, {"clip_norm": -1.0}, {"clip_norm": float("nan")}, {"clip_norm": "1"}, {"clip_norm": True},
               {"skip_nonfinite": 1}):
        with pytest.raises(SdumcError, match="clip_norm|skip_nonfinite"):      # (before the CPU tensor is even looked at)
            engine.TrainStep(flat, 4, T, dims, **kw)
        with pytest.raises(SdumcError, match="clip_norm|skip_nonfinite"):
            engine.FusedTrainer(flat, dims, **kw)
    for kw in ({"clip_norm": 1.0}, {"skip_nonfinite": True}):
        with pytest.raises(SdumcError, match="data parallelism"):
            trainer.DataParallelStep(flat, 4, T, dims, **kw)
    assert engine.FusedTrainer.guard is None
    # torch's signature
    sig = inspect.signature(optim.clip_grad_norm_)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [
        ("parameters", inspect.Parameter.empty), ("max_norm", inspect.Parameter.empty), ("norm_type", 2.0),
        ("error_if_nonfinite", False), ("foreach", None)]
    w = torch.nn.Parameter(torch.ones(3))
    w.grad = torch.ones(3)
    for kw in ({"norm_type": 1.0}, {"norm_type": float("inf")}, {"norm_type": "2"}, {"error_if_nonfinite": True}):
        with pytest.raises(SdumcError, match="not built"):
            optim.clip_grad_norm_([w], 1.0, **kw)
    for bad in (0, -2.0, float("nan"), None, "1", True):
        with pytest.raises(SdumcError):
            optim.clip_grad_norm_([w], bad)
    with pytest.raises(SdumcError, match="no fallback"):
        optim.clip_grad_norm_([w], 1.0)      # a CPU gradient
    assert torch.equal(w.grad, torch.ones(3))
    assert float(optim.clip_grad_norm_([torch.nn.Parameter(torch.ones(2))], 1.0)) == 0.0      # no gradient at all: torch's 0


def test_train_record_takes_the_guard_column():
    from sdumc_amd import record
    from sdumc_amd._lib import SdumcError
    rec = record.TrainRecord.empty(9, 3, "cpu", guard=True)
    assert rec.guard.shape == (3, 4) and rec.guard.dtype == torch.float32
    assert rec.fits(9, 3, "cpu", False, guard=True) and rec.fits(9, 2, "cpu", False, guard=True)
    assert not rec.fits(9, 3, "cpu", False) and not rec.fits(9, 4, "cpu", False, guard=True)
    rec.guard.zero_()
    rec.reset()
    assert bool(torch.isnan(rec.guard).all())
    rec.guard.copy_(torch.tensor([[1.0, 1.0, 0.0, 0.0], [float("nan"), float("nan"), 3.0, 1.0], [2.0, 0.5, 0.0, 0.0]]))
    rec.steps = 3
    assert rec.skipped_steps() == [1]
    rec.steps = 1
    assert rec.skipped_steps() == []
    plain = record.TrainRecord.empty(9, 3, "cpu")
    assert plain.guard is None and plain.fits(9, 3, "cpu", False) and not plain.fits(9, 3, "cpu", False, guard=True)
    with pytest.raises(SdumcError, match="skipped_steps"):
        plain.skipped_steps()


def test_entries_refuse_bad_arguments_without_a_device():
    """SDUMC_EINVAL / SDUMC_ENOMEM come back before any HIP call (the pointers here are never dereferenced)"""
    from sdumc_amd import _lib
    lib = _lib.lib
    q = lib.sdumc_grad_guard_scratch_bytes
    assert q(0) == 0 and q(-5) == 0 and q(1) == 16 and q(8192) == 16 and q(8193) == 32
    assert q(3 * 8192 + 5) == 48 and q(8192 * 1024) == q(1 << 40) == 12 * 1024      # (at most 1024 chunks: they grow instead)
    G, S, H, O = 0x7000_0004, 0x7100_0000, 0x7200_0000, 0x7300_0000

    def call(grads=G, n=100, max_norm=1.0, skip=0, hyper=H, scratch=S, guard=O):
        return lib.sdumc_grad_guard(grads, n, max_norm, skip, hyper, scratch, guard, None)
    bad = [call(grads=None), call(n=0), call(n=-1), call(scratch=None), call(guard=None), call(max_norm=float("nan")), call(skip=2),
           call(skip=-1), call(grads=G + 1), call(hyper=H + 2), call(guard=O + 2), call(scratch=S + 8)]
    assert bad == [-1] * len(bad), bad
    segs = (_lib.NormSeg * 2)()
    segs[0].x, segs[0].count, segs[1].x, segs[1].count = G, 5, G + 400, 9000
    need = lib.sdumc_grad_guard_multi_scratch_bytes(segs, 2)
    assert need == 48      # 1 + 2 chunks of 12 bytes, rounded up to 16

    def multi(s=segs, n=2, max_norm=1.0, scratch=S, nbytes=need, guard=O):
        return lib.sdumc_grad_guard_multi(s, n, max_norm, scratch, nbytes, guard, None)
    assert multi(nbytes=need - 1) == -3
    bad = [multi(s=None), multi(n=0), multi(n=_lib.TENSOR_NORMS_MAX_SEGS + 1), multi(scratch=None), multi(guard=None),
           multi(scratch=S + 4), multi(guard=O + 1), multi(max_norm=float("nan"))]
    segs[1].y = G + 800      # a snapshot has no meaning here
    bad.append(multi())
    segs[1].y = None
    segs[1].count = -1
    bad.append(multi())
    assert lib.sdumc_grad_guard_multi_scratch_bytes(segs, 2) == 0
    segs[1].count, segs[1].x = 9000, G + 2
    bad.append(multi())
    assert bad == [-1] * len(bad), bad
