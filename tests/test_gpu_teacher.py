"""GPU: distillation targets from a stored teacher (sdumc_teacher): the stand-alone entry sdumc_distill_teacher_fwd_bwd, the fused step
(TrainStep(teacher=), sdumc_train_step_teacher) and the trainer's epochs (FusedTrainer(teacher=), refresh_teacher).

Chain of evidence: a teacher whose rows are bit copies of stream 0's rows gives the self-distillation's bits (the entry, then the
step), so the arithmetic is the parent's; the indirection is held bit for bit to the same entry on rows gathered by torch; the epoch
loop is held bit for bit to the same batches stepped one by one with pre-gathered rows; and one step with a random teacher equals
the module route (get_models + the loss modules + autograd on table[idx]) at the project's parity bars.

The store of the epoch tests holds no planes: DeviceFeatureStore refuses planes at the toy widths (not multiples of 64)."""
import math

import numpy as np
import pytest
import torch

from tests import teacher_ref as R
from tests.grad_parity import close_norm

pytestmark = pytest.mark.gpu

CRITERIA = ("rmse", "cosine", "kl")
ROWS = (1, 5, 16, 17, 33, 64)      # on and across the 4096-element block edge of each pair (16 / 32 rows; sample 5 of cross_text straddles)
TOY_DIMS, TOY_T = (64, 32, 48, 32), (21, 5, 13, 4)
PAIRS = R.PAIRS


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import engine
    return engine


@pytest.fixture(scope="module")
def L(E):
    from sdumc_amd import _lib
    return _lib


def _stream0(ins, B):
    return {"text_hidden": ins[2][:B].clone(), "cross_text": ins[3][:B].clone(), "fused": ins[4][:B].clone()}


def _self_call(L, B, ins, crit):
    """the self-distillation call through the entries that existed before a teacher did: sdumc_distill_fwd_bwd (RMSE),
    sdumc_distill_crit_reg_ (cosine / KL).  Both now forward to the code the teacher entry runs with no teacher, so what ties the
    no-teacher path to the PARENT's bits is not this file but tests/test_gpu_loss_stage_bits.py and tests/test_gpu_distill.py (goldens
    recorded before this change); here the claim is: tables of stream 0's rows give what that path gives."""
    rc, o = R.entry(L, B, ins, crit, self_entry=True)
    assert rc == 0
    return o


# ---- 4. the entry: teacher rows equal stream 0's rows -------------------------------------------------------------------------------
@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("crit", CRITERIA)
def test_entry_with_copies_of_stream0_gives_the_self_distillation_bits(L, crit, B):
    ins = R.outputs(B, 100 + B)
    base = _self_call(L, B, ins, crit)
    rc, null = R.entry(L, B, ins, crit, teacher=None)      # no teacher, and a record without tables: the same launches
    assert rc == 0
    rc, empty = R.entry(L, B, ins, crit, teacher=R.record(L, {}, None, 0))
    assert rc == 0
    for o in (null, empty):
        assert torch.equal(o.losses.t[1:6], base.losses.t[1:6])
        assert all(torch.equal(o.grads(p), base.grads(p)) for p in PAIRS) and torch.equal(o.d_vals.t, base.d_vals.t)
    s0 = _stream0(ins, B)
    rc, o = R.entry(L, B, ins, crit, teacher=R.record(L, s0, None, B))
    assert rc == 0 and o.intact()
    assert torch.equal(o.losses.t[1:6], base.losses.t[1:6]) and torch.equal(o.d_vals.t, base.d_vals.t)
    assert bool(torch.isfinite(o.losses.t[3:6]).all()) and float(o.losses.t[3:6].min()) > 0
    for p in PAIRS:
        assert torch.equal(o.grads(p)[B:], base.grads(p)[B:]), p
        g0 = o.grads(p)[:B]
        assert bool((g0 == 0).all()) and not bool(torch.signbit(g0).any()), p
    assert bool((base.grads("fused")[:B] != 0).any())      # ... which is where the teacher call differs from the self call
    for p in ("text_hidden", "cross_text"):
        assert torch.equal(base.grads(p)[:B], o.grads(p)[:B])
    # a pair whose table is NULL stays the self call in both halves
    for skip in PAIRS:
        rc, part = R.entry(L, B, ins, crit, teacher=R.record(L, {k: v for k, v in s0.items() if k != skip}, None, B))
        assert rc == 0
        assert torch.equal(part.losses.t[1:6], base.losses.t[1:6])
        for p in PAIRS:
            want = base if p == skip else o
            assert torch.equal(part.grads(p), want.grads(p)), (skip, p)


# ---- 5. the entry: indirection -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("crit", CRITERIA)
def test_entry_indirection_and_an_index_outside_the_tables(L, crit, B):
    n_rows = 37
    ins = R.outputs(B, 200 + B)
    g = torch.Generator().manual_seed(300 + B)
    held = {p: R.NanHeld(0.5 * torch.randn((n_rows,) + R.PER[p], generator=g)) for p in PAIRS}
    tables = {p: h.t for p, h in held.items()}
    idx = torch.randint(0, n_rows, (B,), generator=g)
    if B > 1:
        idx[-1] = idx[0]      # one repeated entry
        assert B < 4 or bool((idx[1:] < idx[:-1]).any())      # not monotonic
    idx_d = idx.cuda()
    rc, o = R.entry(L, B, ins, crit, teacher=R.record(L, tables, idx_d, n_rows))
    assert rc == 0 and o.intact()
    gathered = {p: tables[p][idx_d].contiguous() for p in PAIRS}
    rc, want = R.entry(L, B, ins, crit, teacher=R.record(L, gathered, None, B))
    assert rc == 0
    assert bool(torch.isfinite(o.losses.t[1:6]).all()) and torch.equal(o.losses.t[1:6], want.losses.t[1:6])
    for p in PAIRS:
        assert torch.equal(o.grads(p), want.grads(p)), p
    # one index equal to n_rows: NaN in every pair's value and in that sample's gradient rows; nothing outside the buffers is touched
    k = B // 2
    bad = idx.clone()
    bad[k] = n_rows
    bad_d = bad.cuda()      # (held: the record carries a bare address)
    rc, o2 = R.entry(L, B, ins, crit, teacher=R.record(L, tables, bad_d, n_rows))
    torch.cuda.synchronize()
    assert rc == 0 and o2.intact()
    assert bool(torch.isnan(o2.losses.t[3:6]).all()) and torch.equal(o2.losses.t[1:3], o.losses.t[1:3])
    assert bool((o2.losses.t[[0, 6, 7]] == R.SENTINEL).all())
    keep = torch.ones(B, dtype=torch.bool)
    keep[k] = False
    for p in PAIRS:
        g2 = o2.grads(p)
        assert bool(torch.isnan(g2[B + k]).all()), p
        assert bool((g2[:B] == 0).all()), p
        if crit != "rmse":      # row criteria: every other sample's gradient is what it was (RMSE's gradient carries the NaN value)
            assert torch.equal(g2[B:][keep], o.grads(p)[B:][keep]), p
    # the host path refuses the same index before anything is enqueued
    from sdumc_amd import ops
    from sdumc_amd.teacher import TeacherTargets
    tt = TeacherTargets(**tables)
    with pytest.raises(L.SdumcError, match="outside the teacher's tables"):
        ops.distill_teacher_fwd_bwd(*ins, R.W5, teacher=tt, rows=bad_d, distill=crit)
    got = ops.distill_teacher_fwd_bwd(*ins, R.W5, teacher=tt, rows=idx_d, distill=crit)
    assert torch.equal(got[0][1:6], o.losses.t[1:6]) and torch.equal(got[2], o.grads("text_hidden"))


# ---- 6. / 7. the step ----------------------------------------------------------------------------------------------------------------
BF16_DIMS = (64, 128, 64, 128)      # the toy frame counts at widths in whole 64-element tiles: what bf16 STORAGE needs


def _toy(E, seed_p=0, seed_b=1234, B=4, dims=TOY_DIMS):
    from oracle import sdumc_oracle as O
    P = O.init_params(dims, seed=seed_p)
    batch = [t.cuda() for t in O.synthetic_batch(B, TOY_T, dims, seed=seed_b)]
    return P, batch


def _run_step(E, P, batch, B=4, seed=31, rows=None, dims=TOY_DIMS, **kw):
    flat, lay = R.flat_from(E, P, dims)
    ts = E.TrainStep(flat, B, TOY_T, dims, seed=seed, **kw)
    ts.set_batch(*batch)
    if rows is not None:
        ts.use_teacher_rows(rows)
    losses = ts.run().clone()
    torch.cuda.synchronize()
    return ts, (losses, ts.grads.clone(), flat.clone(), ts.adam_m.clone(), ts.adam_v.clone())


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("crit", CRITERIA)
def test_step_with_a_partial_teacher_of_its_own_rows_is_the_default_step(E, crit, bf16):
    """text_hidden and cross_text from clones of the default step's stream-0 rows, `fused` left to stream 0: losses, bucket, parameters
    and both moments bit for bit -- in batch order, and from a 29-row store-ordered table behind a shuffled index vector.  Also in bf16
    storage (the loss stage reads fp32 outputs in both modes)."""
    from sdumc_amd.teacher import TeacherTargets
    B = 4
    dims = BF16_DIMS if bf16 else TOY_DIMS
    P, batch = _toy(E, dims=dims)
    kw = dict(distill=crit, bf16=bf16, dims=dims)
    ts0, base = _run_step(E, P, batch, **kw)
    assert bool(torch.isfinite(base[0]).all()) and ts0.dims.bf16 == (2 if bf16 else 0)
    th0, ct0 = ts0.text_hidden[:B].clone(), ts0.cross_text[:B].clone()
    ts1, got = _run_step(E, P, batch, teacher=TeacherTargets(th0, ct0), **kw)
    assert ts1.teacher.active and _same(got, base)
    g = torch.Generator().manual_seed(5)
    idx = torch.randperm(29, generator=g)[:B]
    th = torch.randn(29, 256, generator=g).cuda()
    ct = torch.randn(29, 7, 128, generator=g).cuda()
    th[idx.cuda()], ct[idx.cuda()] = th0, ct0
    _, got = _run_step(E, P, batch, teacher=TeacherTargets(th, ct), rows=idx.cuda(), **kw)
    assert _same(got, base)
    # with `fused` from the teacher too the step differs: stream 0 no longer receives that pair's gradient
    _, full = _run_step(E, P, batch, teacher=TeacherTargets(th0, ct0, ts0.fused[:B].clone()), **kw)
    assert torch.equal(full[0][:7], base[0][:7]) and not torch.equal(full[1], base[1])


def test_default_step_is_untouched(E, L):
    """7. teacher=None, a TeacherTargets without tables and a step that never saw the argument: losses, bucket, parameters bit for bit,
    through the entry the step always took"""
    from sdumc_amd.teacher import TeacherTargets
    P, batch = _toy(E)
    ts, never = _run_step(E, P, batch)
    assert ts._step_entry()[2] == "sdumc_train_step"
    for kw in (dict(teacher=None), dict(teacher=TeacherTargets())):
        ts, got = _run_step(E, P, batch, **kw)
        assert ts._step_entry()[2] == "sdumc_train_step" and _same(got, never)
    ts.teacher = TeacherTargets(torch.randn(4, 256).cuda())
    assert ts._step_entry()[2] == "sdumc_train_step_teacher"
    ts.teacher = None
    assert ts._step_entry()[2] == "sdumc_train_step"


# ---- 8. / 9. epochs ------------------------------------------------------------------------------------------------------------------
def _epoch_env(E, **trainer_kw):
    from oracle import sdumc_oracle as O
    from sdumc_amd.data import DeviceFeatureStore
    n = 20
    P = O.init_params(TOY_DIMS, seed=8)
    store = DeviceFeatureStore.synthetic(n, TOY_T, TOY_DIMS, seed=5)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    batches = [perm[0:8].clone(), perm[8:15].clone(), perm[15:20].clone()]
    g = torch.Generator().manual_seed(2)
    tables = {p: (0.5 * torch.randn((n,) + R.PER[p], generator=g)).cuda() for p in PAIRS}

    def trainer(capacity=True, **kw):
        flat, _ = R.flat_from(E, P, TOY_DIMS)
        return E.FusedTrainer(flat, TOY_DIMS, lr=1e-3, seed=11, capacity=(8, TOY_T) if capacity else None, **trainer_kw, **kw)

    return store, batches, tables, trainer


def _state(tr):
    torch.cuda.synchronize()
    return (tr.params.clone(), tr.state.adam_m.clone(), tr.state.adam_v.clone())


def test_epoch_hands_step_i_the_rows_of_batch_i(E):
    from sdumc_amd.teacher import TeacherTargets
    store, batches, tables, trainer = _epoch_env(E)
    tr = trainer(teacher=TeacherTargets(**tables))
    ls = []
    assert tr.run_epoch(store, batches, on_step=lambda i, l: ls.append(l.clone())) == 3
    got = _state(tr)
    # the same batches one by one, each with its pre-gathered [B, ...] rows and no index vector
    one, want_l = trainer(capacity=False), []
    for ix in batches:
        b, _, _, vals, _ = store.batch(ix)
        one.set_teacher(TeacherTargets(**{p: tables[p][ix.cuda()].contiguous() for p in PAIRS}))
        want_l.append(one.step(b["audios"], b["texts"], b["videos"], b["feat4s"], vals, teacher_rows=None).clone())
    want = _state(one)
    for i, (x, y) in enumerate(zip(ls, want_l)):
        assert torch.equal(x, y), (i, x.tolist(), y.tolist())
    assert _same(got, want)
    # ... and through step(teacher_rows=) and step_from_store on the store-ordered tables
    for how in ("step", "step_from_store"):
        tr2 = trainer(capacity=(how == "step_from_store"), teacher=TeacherTargets(**tables))
        for ix in batches:
            if how == "step":
                b, _, _, vals, _ = store.batch(ix)
                tr2.step(b["audios"], b["texts"], b["videos"], b["feat4s"], vals, teacher_rows=ix)
            else:
                tr2.step_from_store(store, ix)
        assert _same(_state(tr2), want), how
    # not the epoch without a teacher
    plain = trainer()
    plain.run_epoch(store, batches)
    assert not torch.equal(_state(plain)[0], got[0])
    # train_epoch's record: columns 3..5 are the values against the teacher
    tr3 = trainer(teacher=TeacherTargets(**tables))
    rec = tr3.train_epoch(store, batches)
    assert _same(_state(tr3), want)
    log = rec.log[:3].cpu()
    for i, l in enumerate(want_l):
        assert torch.equal(log[i, :8], l.cpu()), i
    # set_teacher(None) between epochs: the cached steps run without the tables
    tr3.set_teacher(None)
    tr3.run_epoch(store, batches)
    assert all(ts._step_entry()[2] == "sdumc_train_step" for ts in tr3._steps.values())


def test_refresh_teacher_and_the_host_refusals(E, L):
    from sdumc_amd.teacher import TeacherTargets
    from sdumc_amd.trainer import DataParallelStep
    store, batches, tables, trainer = _epoch_env(E)
    tr = trainer(ema_decay=0.5)
    tr.run_epoch(store, batches)
    assert not torch.equal(tr.ema_params, tr.params)
    for weights in ("params", "ema"):
        res = tr.refresh_teacher(store, batches, weights=weights)
        want = tr.eval_epoch(store, batches, embeddings=True, weights=weights)
        torch.cuda.synchronize()
        assert res is tr._teacher_res and tr.teacher.active and tr.teacher.n_rows == 20 and tr.teacher.seen is None
        for p in PAIRS:
            assert tr.teacher.tables[p].data_ptr() == res.embeddings[p][0].data_ptr()
            assert bool(torch.isfinite(want.embeddings[p][0]).all()) and torch.equal(tr.teacher.tables[p], want.embeddings[p][0]), (weights, p)
    by_params = tr.eval_epoch(store, batches, embeddings=True)
    assert not torch.equal(by_params.embeddings["fused"][0], tr.teacher.tables["fused"])      # (the average is another network)
    kept = tr._teacher_res
    tr.refresh_teacher(store, batches, weights="ema", stream="missing", pairs=("fused",))
    assert tr._teacher_res is kept and set(tr.teacher.tables) == {"fused"}
    assert tr.teacher.tables["fused"].data_ptr() == kept.embeddings["fused"][1].data_ptr()
    tr.run_epoch(store, batches)      # a mean-teacher epoch runs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.state.losses).all()) and bool(torch.isfinite(tr.params).all())
    with pytest.raises(L.SdumcError, match="without averaged weights"):
        trainer().refresh_teacher(store, batches, weights="ema")
    # an epoch that names an utterance the refresh did not visit: refused before anything is enqueued
    tr.refresh_teacher(store, batches[:2])
    assert tr.teacher.seen is not None and int(tr.teacher.seen.sum()) == 15
    before = _state(tr) + (tr.state.hyper.clone(), tr.state.rng.t.clone())
    for run in (lambda: tr.run_epoch(store, batches), lambda: tr.train_epoch(store, batches),
                lambda: tr.step_from_store(store, batches[2])):
        with pytest.raises(L.SdumcError, match="not visited"):
            run()
    assert _same(_state(tr) + (tr.state.hyper, tr.state.rng.t), before)
    tr.run_epoch(store, batches[:2])      # the visited part is fine
    # a store of another size, an index outside the tables
    with pytest.raises(L.SdumcError, match="rows, the store"):
        trainer(teacher=TeacherTargets(tables["text_hidden"][:19].contiguous())).run_epoch(store, batches)
    P, batch = _toy(E)
    t4 = TeacherTargets(tables["text_hidden"][:4].contiguous())
    ft = trainer(capacity=False, teacher=t4)
    with pytest.raises(L.SdumcError, match="outside the teacher's tables"):
        ft.step(*batch, teacher_rows=[0, 1, 2, 4])
    with pytest.raises(L.SdumcError, match="batch order"):
        trainer(capacity=False, teacher=TeacherTargets(tables["text_hidden"])).step(*batch)
    # capture() of a step with a teacher, and data parallelism
    flat, _ = R.flat_from(E, P, TOY_DIMS)
    ts = E.TrainStep(flat, 4, TOY_T, TOY_DIMS, teacher=t4)
    ts.set_batch(*batch)
    with pytest.raises(L.SdumcError, match="capture: a step with a teacher"):
        ts.capture()
    with pytest.raises(L.SdumcError, match="contiguous int64"):
        ts.use_teacher_rows(torch.arange(4, dtype=torch.int32).cuda())
    with pytest.raises(L.SdumcError, match="outside the teacher's tables"):
        ts.use_teacher_rows(torch.tensor([0, 1, 2, 4]).cuda())
    with pytest.raises(L.SdumcError, match="not built under data parallelism"):
        DataParallelStep(flat, 4, TOY_T, TOY_DIMS, teacher=t4)


# ---- 10. the fused step equals the module route --------------------------------------------------------------------------------------
@pytest.mark.parametrize("crit,shape", [("rmse", "toy"), ("cosine", "toy"), ("kl", "toy"), ("rmse", "c1")])
def test_fused_step_equals_module_route(E, crit, shape):
    """One TrainStep(teacher=, distill=crit) against the reference loop on get_models + the loss modules + autograd with table[idx] as
    the three targets, identical parameters, Philox seed and call index: the six terms and the total to 2e-5, every live gradient tensor
    to 2e-4 of its own norm (the project's parity bars)."""
    from oracle import sdumc_oracle as O
    from sdumc_amd.teacher import TeacherTargets
    if shape == "c1":
        dims, B, Tn = (1024, 4096, 1024, 4096), 16, (200, 16, 120, 16)
    else:
        dims, B, Tn = TOY_DIMS, 4, TOY_T
    seed, n_rows = 31, 23
    P = O.init_params(dims, seed=0)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=1234)]
    g = torch.Generator().manual_seed(9)
    tables = {p: (0.5 * torch.randn((n_rows,) + R.PER[p], generator=g)).cuda() for p in PAIRS}
    idx = torch.randperm(n_rows, generator=g)[:B].cuda()
    flat, lay = R.flat_from(E, P, dims)
    ts = E.TrainStep(flat, B, Tn, dims, seed=seed, distill=crit, teacher=TeacherTargets(**tables))
    ts.set_batch(*batch)
    ts.use_teacher_rows(idx)
    got = ts.run().cpu().numpy()
    loss, terms, mod = R.module_route(dims, P, batch, seed, crit, E.DEFAULT_WEIGHTS, tables, idx)
    print(crit, shape, "fused", got[:7], "module", float(loss), [float(t) for t in terms])
    np.testing.assert_allclose(got[0], float(loss), rtol=2e-5)
    np.testing.assert_allclose(got[1:7], [float(t) for t in terms], rtol=2e-5, atol=1e-6)
    gv = lay.views(torch.cat([ts.grads.cpu(), torch.zeros(lay.total - lay.live)]))
    worst = 0.0
    for k in lay.live_names():
        p = mod._get(k)
        assert p.grad is not None, k
        worst = max(worst, close_norm(gv[k], p.grad, 2e-4, k))
    print(crit, shape, "worst relative gradient error", worst)


def test_bf16_storage_step_with_a_teacher_vs_rounding_emulation(E):
    """The bf16-storage step (all three tables, store-ordered, behind an index vector) against the fp64 evaluation that rounds where the
    engine rounds (oracle/bf16_storage.py), restated with table[idx] as the three targets (tests/teacher_ref.oracle_teacher_step), at
    the shape and bars of tests/test_gpu_bf16_edges.py case 3: loss and terms at BF16_EMU_OUT_TOL, every gradient tensor through
    tests/grad_parity.py at BF16_EMU_GRAD_TOL with the emulation's own fp32 evaluation as the second reference (on the CPU its distance
    from the fp64 one is at most 4.5e-4 for every tensor with signal: no in-between raise applies)."""
    from oracle import sdumc_oracle as O
    from oracle.bf16_storage import Bf16Storage
    from sdumc_amd.teacher import TeacherTargets
    from tests import grad_parity as GP
    from tests.test_gpu_fullsize import BF16_EMU_GRAD_TOL, BF16_EMU_OUT_TOL
    dims, B, Tn, seed, n_rows = (128, 256, 128, 256), 5, (70, 9, 33, 4), 9, 23
    P = O.init_params(dims, seed=23)
    batch = list(O.synthetic_batch(B, Tn, dims, seed=43))
    g = torch.Generator().manual_seed(9)
    tables = {p: 0.5 * torch.randn((n_rows,) + R.PER[p], generator=g) for p in PAIRS}
    idx = torch.randperm(n_rows, generator=g)[:B]
    flat, lay = R.flat_from(E, P, dims)
    ts = E.TrainStep(flat, B, Tn, dims, seed=seed, bf16=True, teacher=TeacherTargets(**{p: t.cuda() for p, t in tables.items()}))
    assert ts.dims.bf16 == 2
    ts.set_batch(*[t.cuda() for t in batch])
    ts.use_teacher_rows(idx.cuda())
    losses = ts.run().cpu().numpy()
    gv = lay.views(torch.cat([ts.grads.cpu(), torch.zeros(lay.total - lay.live)]))
    loss64, terms64, hi = R.oracle_teacher_step(P, batch, seed, tables, idx, E.DEFAULT_WEIGHTS, torch.float64, Bf16Storage())
    _, _, lo = R.oracle_teacher_step(P, batch, seed, tables, idx, E.DEFAULT_WEIGHTS, torch.float32, Bf16Storage())
    want = np.array([float(loss64)] + [float(t) for t in terms64])
    assert np.isfinite(want).all()
    print("bf16 teacher step: losses", losses[:7], "emulation", want, "rel. error %.3g" % float(np.abs(losses[:7] - want).max() / np.abs(want).max()))
    np.testing.assert_allclose(losses[0], want[0], rtol=BF16_EMU_OUT_TOL)
    np.testing.assert_allclose(losses[1:7], want[1:], rtol=BF16_EMU_OUT_TOL, atol=1e-5)
    assert set(hi) == set(lay.live_names())
    res = GP.tensor_errors(lay, gv, hi, lo, BF16_EMU_GRAD_TOL, what="bf16 storage, teacher step vs emulation")
    assert len(res) + len(res.nosignal) == 83 and not res.zero


# ---- 11. combination -----------------------------------------------------------------------------------------------------------------
def test_teacher_with_every_other_option_and_a_nan_row_skips_the_step(E):
    from sdumc_amd.teacher import TeacherTargets
    B = 4
    P, batch = _toy(E, seed_p=1, seed_b=2)
    g = torch.Generator().manual_seed(3)
    tables = {p: (0.5 * torch.randn((B,) + R.PER[p], generator=g)).cuda() for p in PAIRS}
    flat, lay = R.flat_from(E, P, TOY_DIMS)
    start = flat.clone()
    ft = E.FusedTrainer(flat, TOY_DIMS, seed=3, teacher=TeacherTargets(**tables), regress="huber", regress_delta=0.5, clip_norm=1.0,
                        skip_nonfinite=True, ema_decay=0.99, decoupled_decay=True, freeze=("frame_dim_reshape_*",))
    l1 = ft.step(*batch).cpu().clone()
    torch.cuda.synchronize()
    guard = ft.guard.cpu()
    assert bool(torch.isfinite(l1).all()) and bool(torch.isfinite(flat).all()) and not torch.equal(start, flat)
    assert guard[3] == 0 and guard[2] == 0 and guard[0] > 0 and 0 < guard[1] <= 1
    off, shape, _ = lay.entries["frame_dim_reshape_0.weight"]
    n = int(np.prod(shape))
    assert torch.equal(flat[off:off + n], start[off:off + n])
    # a NaN row in the table (seen all true, so the host lets it through): the guard skips the step
    tables["cross_text"][2, 3, 17] = float("nan")
    ft.set_teacher(TeacherTargets(**tables, seen=np.ones(B, dtype=bool)))
    before = (flat.clone(), ft.state.adam_m.clone(), ft.state.adam_v.clone(), ft.ema_params.clone())
    l2 = ft.step(*batch).cpu()
    torch.cuda.synchronize()
    assert math.isnan(float(l2[4])) and math.isnan(float(l2[0])) and bool(torch.isfinite(l2[[1, 2, 3, 5, 6]]).all())
    assert float(ft.guard[3]) == 1.0 and float(ft.guard[2]) > 0
    assert _same(before, (flat, ft.state.adam_m, ft.state.adam_v, ft.ema_params))


# ---- 12. reproducible ----------------------------------------------------------------------------------------------------------------
def test_teacher_step_is_bit_reproducible_over_20_runs(E):
    """Twenty teacher steps (B = 33: more than one block per pair, a sample across a block edge) from identical state: losses and
    the gradient bucket bit for bit."""
    from oracle import sdumc_oracle as O
    from sdumc_amd.teacher import TeacherTargets
    B, n_rows = 33, 41
    P = O.init_params(TOY_DIMS, seed=0)
    flat0, lay = R.flat_from(E, P, TOY_DIMS)
    batch = [t.cuda() for t in O.synthetic_batch(B, TOY_T, TOY_DIMS, seed=41)]
    g = torch.Generator().manual_seed(4)
    tables = {p: (0.5 * torch.randn((n_rows,) + R.PER[p], generator=g)).cuda() for p in PAIRS}
    flat = flat0.clone()
    ts = E.TrainStep(flat, B, TOY_T, TOY_DIMS, seed=5, teacher=TeacherTargets(**tables))
    ts.set_batch(*batch)
    ts.use_teacher_rows(torch.randint(0, n_rows, (B,), generator=g).cuda())
    ref, bad = None, []
    for rep in range(20):
        flat.copy_(flat0)
        ts.adam_m.zero_()
        ts.adam_v.zero_()
        ts.hyper[1] = 0.0
        ts.rng.set_call(0)
        torch.cuda.synchronize()
        losses = ts.run().clone()
        out = (losses, ts.grads.clone(), flat.clone())
        torch.cuda.synchronize()
        if ref is None:
            ref = out
            assert bool(torch.isfinite(losses).all()) and float(out[1].abs().max()) > 0 and float(losses[3:6].min()) > 0
        elif not _same(ref, out):
            bad.append(rep)
    assert not bad, f"{len(bad)} of 19 teacher steps differed from the first: runs {bad[:10]}"
