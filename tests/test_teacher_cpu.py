"""CPU-only: distillation targets from a stored teacher (sdumc_teacher; sdumc_distill_teacher_fwd_bwd, sdumc_loss_backward_teacher,
sdumc_train_step_teacher; teacher.TeacherTargets; TrainStep / FusedTrainer(teacher=)) -- the ABI mirror, the refusals that come back
before any HIP call, and the host-side validation.  What needs a device is in tests/test_gpu_teacher.py."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (64, 32, 48)
EINVAL, ENOMEM = -1, -3


def _compiled(exprs, prologue=""):
    """the host C compiler's value of each expression with include/sdumc_hip.h in scope (the helper of tests/test_adamw_cpu.py)"""
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sdumc_hip.h"\n%s\nint main(void){printf("%s\\n", %s); return 0;}\n'
           % (prologue, " ".join(["%zu"] * len(exprs)), ", ".join("(size_t)(%s)" % e for e in exprs)))
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "t.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "t.c"), "-o", os.path.join(td, "t")])
        return [int(v) for v in subprocess.check_output([os.path.join(td, "t")]).split()]


def test_teacher_record_mirrors_the_header_and_the_pinned_structs_stay():
    """1. every field's offsetof and the sizeof of sdumc_teacher from a compiled program against the ctypes mirror; sdumc_step_cfg is
    still 200 bytes and sdumc_net_io what the mirror (unchanged by this feature) says; the three entries are declared, listed and
    bound"""
    from sdumc_amd import _lib
    T = _lib.Teacher
    names = [f[0] for f in T._fields_]
    assert names == ["text_hidden", "cross_text", "fused", "idx", "n_rows"]
    got = _compiled([f"offsetof(sdumc_teacher, {f})" for f in names] +
                    ["sizeof(sdumc_teacher)", "sizeof(sdumc_step_cfg)", "sizeof(sdumc_net_io)"])
    assert got[:5] == [getattr(T, f).offset for f in names] == [0, 8, 16, 24, 32]
    assert got[5] == C.sizeof(T) == 40
    assert got[6] == C.sizeof(_lib.StepCfg) == 200
    assert got[7] == C.sizeof(_lib.NetIO)
    assert [f[0] for f in _lib.StepCfg._fields_][-1] == "distill" and _lib.REGRESS_DELTA_OFFSET == 196
    assert _lib.TEACHER_ABI is True
    header = open(os.path.join(ROOT, "include", "sdumc_hip.h")).read()
    for name, nargs in (("sdumc_distill_teacher_fwd_bwd", 18), ("sdumc_loss_backward_teacher", 8), ("sdumc_train_step_teacher", 5)):
        fn = getattr(_lib.lib, name)
        assert name in _lib.EXPORTS and fn.restype is C.c_int and len(fn.argtypes) == nargs
        assert f"int {name}(" in header
    # the entries without a teacher keep their argument lists
    assert len(_lib.lib.sdumc_train_step.argtypes) == 4 and len(_lib.lib.sdumc_loss_backward.argtypes) == 7
    assert len(_lib.lib.sdumc_distill_fwd_bwd.argtypes) == 16


def _teacher(L, th=0x7000000, ct=0x7100000, fz=0x7200000, idx=0x7300000, n_rows=37):
    t = L.Teacher()
    t.text_hidden, t.cross_text, t.fused, t.idx, t.n_rows = th, ct, fz, idx, n_rows
    return t


# what every entry refuses of a teacher for a batch of B = 4 (B_global / ssd_global: per entry, below)
def _bad_teachers(L):
    return {"n_rows 0": _teacher(L, n_rows=0), "n_rows < 0": _teacher(L, n_rows=-3),
            "no idx and n_rows != B": _teacher(L, idx=None, n_rows=5),
            "no idx and n_rows != B (one table)": _teacher(L, ct=None, fz=None, idx=None, n_rows=3),
            "text_hidden not 4-byte aligned": _teacher(L, th=0x7000002), "cross_text not 4-byte aligned": _teacher(L, ct=0x7100001),
            "fused not 4-byte aligned": _teacher(L, fz=0x7200003), "idx not 8-byte aligned": _teacher(L, idx=0x7300004)}


@pytest.mark.skipif(torch.cuda.is_available(), reason="invented addresses: on a machine with a GPU tests/test_gpu_teacher.py runs "
                    "the entries on live allocations")
def test_the_entries_refuse_a_bad_teacher_before_any_hip_call():
    """2. SDUMC_EINVAL from the three entries, on invented addresses, for: n_rows < 1 with a table, idx NULL with n_rows != B, a
    misaligned table, a teacher beside a B_global different from B, a teacher beside ssd_global.  sdumc_train_step_teacher and
    sdumc_loss_backward_teacher with a GOOD teacher (and with none, and with one that has no table) get as far as the workspace
    check -- SDUMC_ENOMEM, still in front of every HIP call -- so the EINVAL is the teacher's."""
    from sdumc_amd import _lib as L
    from sdumc_amd.engine import make_dims
    lib = L.lib
    B = 4
    d = make_dims(B, 2, 21, 13, (5, 4), DIMS, True)
    io, cfg, g = L.NetIO(), L.StepCfg(), L.NetGrads()
    io.audio, io.video, io.params, io.workspace, io.rng_state = 0x10000, 0x20000, 0x4000000, 0x1000000, 0x60000
    io.text[0], io.text[1] = 0x40000, 0x50000
    io.vals, io.fused, io.rnc, io.text_hidden, io.cross_text = 0x70000, 0x80000, 0x90000, 0xa0000, 0xb0000
    io.workspace_bytes = lib.sdumc_step_workspace_bytes(C.byref(d)) - 1
    cfg.adam_m, cfg.adam_v, cfg.hyper, cfg.losses, cfg.labels = 0x2000000, 0x3000000, 0xc0000, 0xd0000, 0xe0000
    cfg.temperature = 2.0
    g.d_vals, g.d_fused, g.d_rnc, g.d_text_hidden, g.d_cross_text = 0x5000000, 0x5100000, 0x5200000, 0x5300000, 0x5400000

    def step(t):
        return lib.sdumc_train_step_teacher(C.byref(d), C.byref(io), C.byref(cfg), C.byref(t) if t is not None else None, None)

    def loss_bwd(t):
        return lib.sdumc_loss_backward_teacher(C.byref(d), C.byref(io), C.byref(cfg), C.byref(g), C.byref(t) if t is not None else None,
                                               0x6000000, 0, None)

    w5 = (C.c_float * 5)(0.5, 0.5, 0.1, 0.7, 0.1)

    def entry(t, denom=float(B), ssd=None, distill=0):
        return lib.sdumc_distill_teacher_fwd_bwd(B, denom, 0x70000, 0xe0000, 0xa0000, 0xb0000, 0x80000, w5, ssd, 0x5000000, 0x5300000,
                                                 0x5400000, 0x5100000, 0xd0000, 0x6000000, distill, C.byref(t), None)

    good = [None, _teacher(L, th=None, ct=None, fz=None, idx=None, n_rows=0), _teacher(L), _teacher(L, idx=None, n_rows=B),
            _teacher(L, th=None, fz=None), _teacher(L, n_rows=1)]
    for t in good:
        assert step(t) == ENOMEM and loss_bwd(t) == ENOMEM
    assert lib.sdumc_train_step(C.byref(d), C.byref(io), C.byref(cfg), None) == ENOMEM
    for what, t in _bad_teachers(L).items():
        assert step(t) == EINVAL, what
        assert loss_bwd(t) == EINVAL, what
        for distill in (0, 1, 2):
            assert entry(t, distill=distill) == EINVAL, what
    # the data-parallel exchange carries no teacher
    cfg.B_global = 2 * B
    assert step(_teacher(L)) == EINVAL and loss_bwd(_teacher(L)) == EINVAL
    assert step(None) == ENOMEM and step(good[1]) == ENOMEM      # (no table: not a teacher)
    cfg.B_global = B
    assert step(_teacher(L)) == ENOMEM and loss_bwd(_teacher(L)) == ENOMEM
    cfg.B_global = 0
    cfg.ssd_global = 0x8000000
    assert step(_teacher(L)) == EINVAL and loss_bwd(_teacher(L)) == EINVAL
    cfg.ssd_global = None
    assert entry(_teacher(L), denom=float(2 * B)) == EINVAL and entry(_teacher(L), ssd=0x8000000) == EINVAL
    assert entry(_teacher(L), distill=3) == EINVAL


def _tables(n, device="cpu"):
    g = torch.Generator().manual_seed(n)
    return (torch.randn(n, 256, generator=g).to(device), torch.randn(n, 7, 128, generator=g).to(device),
            torch.randn(n, 128, generator=g).to(device))


def test_teacher_targets_validation():
    """3. TeacherTargets on CPU tensors: dtype, shapes, contiguity, one n_rows, seen's length; no table at all is a valid, inactive
    object; from_eval returns views of the result's tensors and reads `seen` once"""
    from sdumc_amd._lib import SdumcError
    from sdumc_amd.teacher import PAIRS, TeacherTargets
    from sdumc_amd.evaluate import EvalResult
    th, ct, fz = _tables(9)
    t = TeacherTargets(th, ct, fz)
    assert t.active and t.n_rows == 9 and t.seen is None and set(t.tables) == set(PAIRS)
    assert t.tables["text_hidden"] is th
    assert TeacherTargets.from_tensors(cross_text=ct).tables == {"cross_text": ct}
    empty = TeacherTargets()
    assert not empty.active and empty.n_rows is None and empty.record().n_rows == 0
    r = t.record(0x1000)
    assert (r.text_hidden, r.cross_text, r.fused, r.idx, r.n_rows) == (th.data_ptr(), ct.data_ptr(), fz.data_ptr(), 0x1000, 9)
    assert TeacherTargets(fused=fz).record().text_hidden is None
    bad = [dict(text_hidden=th.double()), dict(text_hidden=th.half()), dict(text_hidden=th.numpy()), dict(text_hidden=th[:, :255]),
           dict(text_hidden=th.reshape(9, 2, 128)), dict(cross_text=ct.reshape(9, 896)), dict(cross_text=ct[:, :6]),
           dict(fused=fz.t().contiguous().t()), dict(fused=torch.zeros(0, 128)), dict(fused=fz[::2]),
           dict(text_hidden=th, fused=fz[:8]), dict(text_hidden=th, cross_text=_tables(10)[1]),
           dict(text_hidden=th, seen=np.ones(8, dtype=bool)), dict(fused=fz, seen=torch.ones(10, dtype=torch.uint8))]
    for kw in bad:
        with pytest.raises(SdumcError):
            TeacherTargets(**kw)
    seen = np.ones(9, dtype=bool)
    assert TeacherTargets(th, seen=seen).seen is None      # (all visited: nothing to check per batch)
    seen[4] = False
    assert TeacherTargets(th, seen=torch.from_numpy(seen)).seen.tolist() == seen.tolist()
    # from_eval: views, not copies
    res = EvalResult.empty(9, "cpu", embeddings=True).reset()
    res.seen[:] = 1
    res.seen[7] = 0
    for stream, s in (("full", 0), ("missing", 1)):
        te = TeacherTargets.from_eval(res, stream)
        for name in PAIRS:
            assert te.tables[name].data_ptr() == res.embeddings[name][s].data_ptr() and te.tables[name].is_contiguous()
        assert te.n_rows == 9 and te.seen.tolist() == [True] * 7 + [False, True]
    te = TeacherTargets.from_eval(res, pairs=("fused", "text_hidden"))
    assert set(te.tables) == {"fused", "text_hidden"}
    for kw in (dict(stream="both"), dict(pairs=()), dict(pairs=("rnc",)), dict(pairs=("fused", "fused"))):
        with pytest.raises(SdumcError):
            TeacherTargets.from_eval(res, **kw)
    with pytest.raises(SdumcError):
        TeacherTargets.from_eval(EvalResult.empty(9, "cpu").reset())


def test_row_checks_refuse_on_the_host():
    """3. the pure helpers every host path runs before anything is enqueued: an index outside the tables, an utterance the teacher's
    pass did not visit, a store of another size, a batch of another size without indices"""
    from sdumc_amd._lib import SdumcError
    from sdumc_amd.teacher import TeacherTargets, check_rows, teacher_arg
    seen = np.ones(20, dtype=bool)
    seen[[3, 11]] = False
    assert check_rows([0, 19, 5, 5], 20).tolist() == [0, 19, 5, 5]
    assert check_rows(torch.tensor([[1, 2], [4, 0]], dtype=torch.int32), 20, seen).dtype == torch.int64
    for idx in ([0, 20], [-1, 3], [1 << 40], [], torch.tensor([0.0, 1.0]), torch.tensor([True])):
        with pytest.raises(SdumcError):
            check_rows(idx, 20)
    with pytest.raises(SdumcError, match="utterance 11 was not visited"):
        check_rows([0, 11, 4], 20, seen)
    with pytest.raises(SdumcError, match="not visited"):
        check_rows([19, 3], 20, seen)
    th = _tables(20)[0]
    t = TeacherTargets(th, seen=seen)
    assert t.check_rows([0, 1, 2]).tolist() == [0, 1, 2]
    with pytest.raises(SdumcError):
        t.check_rows([2, 3])
    with pytest.raises(SdumcError, match="20 rows, the store 21"):
        t.check_store(21)
    t.check_store(20)
    TeacherTargets().check_store(5)      # (no table: nothing to compare)
    with pytest.raises(SdumcError, match="batch order"):
        t.check_batch(8)
    with pytest.raises(SdumcError):
        t.check_batch(20)      # rows 3 and 11 of a [B, ...] table are marked unvisited
    TeacherTargets(th).check_batch(20)
    # teacher= takes a TeacherTargets or None, on the step's device
    assert teacher_arg(None) is None and teacher_arg(t, "cpu") is t and teacher_arg(TeacherTargets(), "cuda:0") is not None
    for bad in (th, {"text_hidden": th}, "ema", 1):
        with pytest.raises(SdumcError):
            teacher_arg(bad)
    with pytest.raises(SdumcError, match="sit on"):
        teacher_arg(t, "cuda:0")


def test_a_library_from_before_the_entries_refuses_a_teacher(monkeypatch):
    """a library named by SDUMC_LIB that lacks sdumc_train_step_teacher (TEACHER_ABI False): a teacher with a table raises on the host,
    None and a TeacherTargets without tables pass (they take the entry that library has)"""
    from sdumc_amd import _lib
    from sdumc_amd.teacher import TeacherTargets, teacher_arg
    t = TeacherTargets(_tables(4)[0])
    assert teacher_arg(t) is t
    monkeypatch.setattr(_lib, "TEACHER_ABI", False)
    with pytest.raises(_lib.SdumcError, match="from before sdumc_train_step_teacher"):
        teacher_arg(t)
    empty = TeacherTargets()
    assert teacher_arg(None) is None and teacher_arg(empty) is empty


def test_the_python_layers_take_the_argument_and_data_parallel_refuses_it():
    from sdumc_amd import engine, ops, trainer
    from sdumc_amd._lib import SdumcError
    from sdumc_amd.teacher import TeacherTargets
    assert inspect.signature(engine.TrainStep.__init__).parameters["teacher"].default is None
    assert inspect.signature(engine.FusedTrainer.__init__).parameters["teacher"].default is None
    assert inspect.signature(engine.FusedTrainer.step).parameters["teacher_rows"].default is None
    rt = inspect.signature(engine.FusedTrainer.refresh_teacher).parameters
    assert rt["weights"].default == "params" and rt["stream"].default == "full" and rt["key_padding"].default is False
    assert callable(engine.TrainStep.use_teacher_rows) and callable(engine.FusedTrainer.set_teacher)
    assert callable(ops.distill_teacher_fwd_bwd)
    t = TeacherTargets(_tables(4)[0])
    flat = torch.zeros(16)
    with pytest.raises(SdumcError, match="teacher= is not built under data parallelism"):
        trainer.DataParallelStep(flat, 4, (21, 5, 13, 4), (64, 32, 48, 32), teacher=t)
    with pytest.raises(SdumcError, match="teacher= is not built under data parallelism"):
        trainer.HipBackend(flat, 4, (21, 5, 13, 4), (64, 32, 48, 32), (0.5,) * 6, 1e-4, (0.9, 0.999), 1e-8, 1e-5, 0, 0, 4, teacher=t)
