"""The backward pass's schedule (engine.hip: plan_backward -> BwdSchedule, read by backward() and its parts), over the case matrix of
tests/backward_cases.py:

  (a) the route is the record's: the record sdumc_debug_backward_schedule returns for every case equals a row written here from
      reading plan_backward, and over the matrix every field takes every value the public surface can give it (the exceptions by name);
  (b) every route against the reference: each live gradient tensor against its OWN norm (tests/grad_parity.py) -- fp32 and planes
      against the fp64 oracle at the project's 2e-4 with the fp32 oracle as the second reference, bf16 storage against the rounding
      emulation (oracle/bf16_storage.py) at BF16_EMU_GRAD_TOL, TrainStep cases through the oracle's train step with the losses at the
      bars of test_gpu_net.py / test_gpu_bf16_edges.py.  Operands mode (bf16 = 1) has no discriminating reference -- its only oracle bar
      is 4e-2 / 0.2 (test_gpu_net.py::test_bf16_operand_mode_c3) -- so for it only (c) is asserted;
  (c) lanes change nothing: where the record under concurrency 0 equals the record under concurrency 1 in every field but lane placement
      the two gradient buckets are bit for bit equal, and the multi-lane call run twice equals itself.  No bit-equality claim where the
      records differ (the own-lane early route of a phased call): (b) holds those;
  (d) phased calls: after phase 0 alone on a NaN-filled bucket [0, layout.early) is finite on every used element, the late slice is
      still NaN but for the Cross_Attention input_proj gradients the record says leave in phase 0 (ca_dw_grouped), and phase 1 leaves
      the early slice bit-unchanged.

Every tolerance is another test's: 2e-4 (test_gpu_net.py::test_backward_vs_oracle), BF16_EMU_GRAD_TOL / BF16_EMU_OUT_TOL
(test_gpu_fullsize.py), the step's losses rtol 1e-4 / atol 1e-6 (test_gpu_net.py::test_train_step_smallest_batches_vs_oracle) and, in bf16
storage, BF16_EMU_OUT_TOL / atol 1e-5 (test_gpu_bf16_edges.py).  ExecContext options only; every context is closed.

That (b) bites was shown once on scratch builds of engine.hip that change arithmetic only (profiles/grad_parity_by_tensor.txt has the figures):
  * the merged early launch's dX scaled by 1 + 1e-3: the six fp32 / planes TrainStep cases that take that launch fail, naming
    frame_dim_reshape_0 / _2 weight and bias at 9.0e-4 .. 9.9e-4; nothing else fails.  The NetCall cases of the same route do NOT see
    it: under O(1) external gradients the Cross_Attention sites carry under a fifth of dx, so the error stays under 2e-4 -- which is
    why the matrix has the step cases under conc0 / cl0 / split14 and at fold-all.  No bf16-storage case can see it: 1e-3 lies
    under BF16_EMU_GRAD_TOL = 1e-2;
  * the separate mask-sum without its last term: every case with a mask-sum launch fails (83 of 95), naming the frame_dim_reshape
    tensors of the modalities concerned at 0.15 .. 0.97, bf16 storage included; green are exactly the cases without one -- fold-all
    where every modality folds (not its split7 / split0 cases, which fold nothing) and step-freeze-all, whose frame dW is not computed;
  * the per-layer frame dW without audio's problem: the three odd-widths cases fail, naming frame_dim_reshape_0.weight and .bias at
    1.0, and the seven operands-mode cases (worst 1.0 against 0.2); every grouped route stays green."""
import numpy as np
import pytest
import torch

from tests import backward_cases as BC
from tests import grad_parity as GP

pytestmark = pytest.mark.gpu

IDS = [BC.case_id(c) for c in BC.CASES]


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import engine
    return engine


# ---- (a) the table -----------------------------------------------------------------------------------------------------------------
# Written from reading plan_backward / plan_utterance / make_plan, in layers; a later layer overrides an earlier one.  With the
# process-wide switches at their defaults (no SDUMC_* variable set) the record is a function of:
#   bgb         = (background_lane == 3): bit 0 only -- the AUDIO Cross_Attention site is the one early candidate of the option
#   multi       = concurrency
#   dxfold[m]   = every run of m has T >= 63 or T == 32, storage fp32 or bf16 (never operands); dx_sum[m] = dxfold[m] and, in fp32,
#                 the split's rows bit
#   groupable[m]: every SHARED run of m (audio / video under two streams; in bf16 storage in eval mode only) has x_samples * T >= 16
#                 (bf16 storage: 64)
# BASE: fold-av, fp32, the single call, (3, 1, 1, 15).  V = 4 <= 128: chain, clustered; one run per modality and 3 chunks at most: fra_fold.
# fp32: the frame-level dW is grouped (dw_grouped); 3 runs <= 4: pool_grouped; both: batch 1 rides with the input_proj dW (no flush1) and,
# with the frame-level part following, batch 3 rides too (no flush3); gg_utt is always on: no flush2.  bgb and dx_sum of audio AND video:
# both go early (audio_and_video), on lane 3, each folding (dx_sum) with its dW grouped: ONE launch.  Text: T = 6 folds nothing, never early.
BASE = {"rc": 0, "chain": 1, "cluster": 1, "fra_fold": 1, "utterance": 1, "frame": 1, "dw_grouped": 1, "pool_grouped": 1,
        "early_one_launch": 1, "flush1_after_pool": 0, "flush2_after_query": 0, "flush3_after_utt": 0}
for _m, _early, _fold in (("a", 1, 1), ("t", 0, 0), ("v", 1, 1)):
    BASE.update({f"early_{_m}": _early, f"early_lane_{_m}": 3, f"ca_dw_grouped_{_m}": 1, f"fra_dw_grouped_{_m}": 1, f"ca_dw_late_{_m}": 0,
                 f"dw_on_lane3_{_m}": 0, f"dx_sum_{_m}": _fold, f"frame_dw_grouped_{_m}": 1, f"frame_dw_skip_{_m}": 0, f"k1_{_m}": 2 - _early})

# no modality folds: audio alone goes early (bgb), as a launch of its own (no dx_sum: not the merged launch); video waits (k1 = 2)
_NOFOLD = {"dx_sum_a": 0, "dx_sum_v": 0, "early_v": 0, "k1_v": 2, "early_one_launch": 0}
SHAPE = {
    "fold-av": {},
    "fold-av-ne": {"fra_fold": 0},                     # two text runs: the clustered stage does not combine them (four runs: still pool_grouped)
    "fold-all": {"dx_sum_t": 1},                       # text folds too (T = 32); it is still never early
    "fold-av-128": {},
    "no-fold": _NOFOLD,
    # text lengths 5 / 3: two runs, no fra_fold; widths 37 and 42 are no multiples of 4: audio's and video's frame dW go per stream
    "odd-widths": {**_NOFOLD, "fra_fold": 0, "frame_dw_grouped_a": 0, "frame_dw_grouped_v": 0},
    # shared runs of 1 * 6 and 1 * 5 rows < 16: audio's and video's key dW are not groupable (text's runs are not shared); two text runs
    "few-rows": {**_NOFOLD, "fra_fold": 0, "fra_dw_grouped_a": 0, "ca_dw_grouped_a": 0, "fra_dw_grouped_v": 0, "ca_dw_grouped_v": 0},
    # audio folds (T = 2112), video does not: audio alone early, folding, dW grouped: the merged launch with one problem; 33 chunks: no fra_fold
    "long": {"dx_sum_v": 0, "early_v": 0, "k1_v": 2, "fra_fold": 0},
    "wide-V": {**_NOFOLD, "cluster": 0, "fra_fold": 0},                # V = 130: the clustered kernels do not fit; chain.hip
    "no-chain": {**_NOFOLD, "chain": 0, "cluster": 0, "fra_fold": 0},  # V = 514: per layer (flush2 stays off: gg_utt)
    # bf16 storage, eval: audio's shared 40 rows < 64: not groupable -> its per-layer key dW goes to lane 3; video (T = 70) folds, audio
    # (T = 20) does not: audio alone early, not merged; two text runs
    "bf16-few": {"dx_sum_a": 0, "early_v": 0, "k1_v": 2, "early_one_launch": 0, "fra_fold": 0, "fra_dw_grouped_a": 0, "ca_dw_grouped_a": 0,
                 "dw_on_lane3_a": 1},
}
STORAGE = {
    "fp32": {}, "planes": {},      # the planes are the forward's: nothing of the backward's record reads them
    "bf16s": {},                   # grouped like fp32; folds without the split's rows bit; train mode: no run counts as shared
    # operands mode: no grouped frame-level dW (so batches 1 and 3 are flushed where they arise), nothing folds, audio alone early
    "bf16op": {**_NOFOLD, "dx_sum_t": 0, "dw_grouped": 0, "flush1_after_pool": 1, "flush3_after_utt": 1,
               **{f"{f}_{m}": 0 for f in ("ca_dw_grouped", "fra_dw_grouped", "frame_dw_grouped") for m in "atv"}},
}
_NO_EARLY = {"early_a": 0, "early_v": 0, "k1_a": 2, "k1_v": 2, "early_one_launch": 0}      # bgb = 0
_NO_ROWS_BIT = {**_NOFOLD, "dx_sum_t": 0}                                                     # fp32 without the rows bit folds nothing
SETTING = {
    "default": {}, "bg0": _NO_EARLY, "bg2": _NO_EARLY,      # 2 is the forward's background lane only
    "conc0": {"dw_on_lane3_a": 0},                          # one lane: nothing to move to lane 3; the rest of a single call's record stays
    "cl0": {"cluster": 0, "fra_fold": 0},
    "split7": _NO_ROWS_BIT, "split0": _NO_ROWS_BIT,
    "split14": {},                                          # the group bit changes the grouped launch's arithmetic, not the route
    "bg0+conc0": {**_NO_EARLY, "dw_on_lane3_a": 0}, "bg0+cl0": {**_NO_EARLY, "cluster": 0, "fra_fold": 0},
}
FORM = {"net": {}, "s1": {}, "eval": {}, "step": {}, "phased": {},      # (one stream: V = B, no shared run, the same record)
        "step-freeze": {"frame_dw_skip_a": 1}, "step-freeze-all": {"frame_dw_skip_a": 1, "frame_dw_skip_t": 1, "frame_dw_skip_v": 1}}
# phased calls: only a modality that owns a side lane goes early, on that lane (lane 3 cannot carry frame-level work across the phases):
# audio (lane 2) with bgb and real lanes; video sits on the caller's stream.  Never the merged launch.
_PH = {"early_v": 0, "k1_v": 2, "early_one_launch": 0}
PHASED = {"default": {**_PH, "early_a": 1, "early_lane_a": 2, "k1_a": 1},
          "conc0": {**_PH, "early_a": 0, "early_lane_a": 3, "k1_a": 2},
          "bg0": {**_PH, "early_a": 0, "early_lane_a": 3, "k1_a": 2}}
PHASE = {3: {}, 1: {"utterance": 1, "frame": 0, "flush3_after_utt": 1},      # phase 0 ends by flushing batch 3 and joining lane 3
         2: {"utterance": 0, "frame": 1}}


def table_row(c, phases):
    row = {**BASE, **SHAPE[c.shape], **STORAGE[c.storage], **SETTING[c.setting], **FORM[c.form]}
    if c.form == "phased":
        row.update(PHASED[c.setting])
    row.update(PHASE[phases])
    return row


# Values no case can reach through the public surface, and why (asserted: the matrix never shows them):
UNREACHED = {
    ("rc", "nonzero"): "needs row maps (a resident store): tests/test_gpu_rowmap.py holds the refusals",
    ("pool_grouped", 0): "a call never has more than four runs (audio, video, two text runs)",
    ("flush2_after_query", 1): "gg_utt is on unless SDUMC_DW_GROUP=0",
    ("ca_dw_late", 1): "needs pool_grouped = 0",
    ("early_t", 1): "background_lane 3 sets the audio bit alone; audio_and_video adds video, never text",
    ("k1_t", 1): "follows early_t",
    ("early_lane_t", "own"): "follows early_t", ("early_lane_v", "own"): "video's lane is the caller's stream: never an own lane",
    ("dw_on_lane3_t", 1): "audio's alone by construction (m == 0)", ("dw_on_lane3_v", 1): "audio's alone by construction (m == 0)",
}

_records = {}


def _phases_of(c):
    return (1, 2) if c.form == "phased" else (3,)


def records(E, c):
    """{phases: record} of case c from the device library (launches nothing), once per case"""
    if c not in _records:
        ctx = BC.make_ctx(E, c.setting)
        try:
            obj = BC.build(E, c, ctx)
            _records[c] = {ph: E.backward_schedule(BC.schedule_target(obj), ph) for ph in _phases_of(c)}
            torch.cuda.synchronize()
            del obj
        finally:
            ctx.close()
    return _records[c]


@pytest.mark.parametrize("c", BC.CASES, ids=IDS)
def test_record_equals_the_table(E, c):
    for ph, got in records(E, c).items():
        want = table_row(c, ph)
        assert set(got) == set(want)
        diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
        assert not diff, f"{BC.case_id(c)} phases {ph}: (device, table) {diff}"


def test_matrix_reaches_every_value_of_every_field(E):
    seen = {}
    for c in BC.CASES:
        for rec in records(E, c).values():
            for k, v in rec.items():
                seen.setdefault(k, set()).add(v)
    assert seen["rc"] == {0}
    missing = []
    for k, vals in sorted(seen.items()):
        base = k.rsplit("_", 1)[0] if k[-2:] in ("_a", "_t", "_v") else k
        if k == "rc":
            continue
        if base == "k1":
            want = {1, 2}
        elif base == "early_lane":
            want = {3, "own"}
            vals = {3 if v == 3 else "own" for v in vals}
        else:
            want = {0, 1}
        for v in sorted(want - vals, key=str):
            if (k, v) not in UNREACHED and (base, v) not in UNREACHED:
                missing.append((k, v))
        for v in vals & want:
            assert (k, v) not in UNREACHED and (base, v) not in UNREACHED, f"{k} = {v} is reached after all: {UNREACHED.get((k, v))}"
    assert not missing, f"values the matrix never visits: {missing}"
    assert seen["early_lane_a"] == {2, 3}      # lane 3, and audio's own lane (LANE_OF[0] = 2)


# ---- running a case ----------------------------------------------------------------------------------------------------------------
_runs = {}


def _used(lay):
    used = torch.zeros(lay.live, dtype=torch.bool)          # alignment padding between tensors is never written
    for n in lay.live_names():
        off, shape, _ = lay.entries[n]
        used[off:off + int(np.prod(shape))] = True
    return used


def run_case(E, c, cache=True):
    """{"grads": the final bucket on the CPU, "losses": a step's, "phase0": the bucket after phase 0 alone} of case c under its own
    context, which is closed before returning"""
    if cache and c in _runs:
        return _runs[c]
    _, B, _, _, _ = BC.inputs(c.shape, BC.padded_of(c.storage))
    ctx = BC.make_ctx(E, c.setting)
    out = {}
    try:
        obj = BC.build(E, c, ctx)
        if c.form.startswith("step"):
            out["losses"] = obj.run().cpu().numpy().copy()
            out["grads"] = obj.grads.cpu().clone()
        else:
            dout = [d.cuda().contiguous() for d in BC.douts(BC.streams_of(c.form) * B)]
            if c.form == "phased":
                obj.forward()
                for dst, src in zip((obj.d_vals, obj.d_fused, obj.d_rnc, obj.d_text_hidden, obj.d_cross_text), dout):
                    dst.copy_(src)
                obj.grads.fill_(float("nan"))
                obj.backward_phase(0)
                torch.cuda.synchronize()
                out["phase0"] = obj.grads.cpu().clone()
                obj.backward_phase(1)
                torch.cuda.synchronize()
                out["grads"] = obj.grads.cpu().clone()
            else:
                obj.forward()
                out["grads"] = obj.backward(*dout).cpu().clone()
        torch.cuda.synchronize()
        del obj
    finally:
        ctx.close()
    if cache:
        _runs[c] = out
    return out


def _same_bucket(E, c, a, b):
    """bit equality of two buckets on every used element (a phased case's alignment padding keeps its NaN fill)"""
    used = _used(E.ParamLayout.get(*BC.SHAPES[c.shape][0][:3]))
    return torch.equal(a[used], b[used])


def _views(E, c, bucket):
    lay = E.ParamLayout.get(*BC.SHAPES[c.shape][0][:3])
    return lay, lay.views(torch.cat([bucket, torch.zeros(lay.total - lay.live)]))


# ---- (b) every route against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in BC.CASES if BC.has_reference(c)], ids=[i for i, c in zip(IDS, BC.CASES) if BC.has_reference(c)])
def test_route_against_the_reference(E, c):
    got = run_case(E, c)
    ref = BC.reference(c)
    lay, gv = _views(E, c, got["grads"])
    names = lay.live_names()
    assert set(ref["hi"]) == set(names)
    if c.form.startswith("step"):
        want, losses = np.array(ref["losses"]), got["losses"]
        if c.storage == "bf16s":      # test_gpu_bf16_edges.py's bars
            from tests.test_gpu_fullsize import BF16_EMU_OUT_TOL
            np.testing.assert_allclose(losses[0], want[0], rtol=BF16_EMU_OUT_TOL)
            np.testing.assert_allclose(losses[1:7], want[1:], rtol=BF16_EMU_OUT_TOL, atol=1e-5)
        else:                         # test_gpu_net.py::test_train_step_smallest_batches_vs_oracle's bars
            np.testing.assert_allclose(losses[0], want[0], rtol=1e-4)
            np.testing.assert_allclose(losses[1:7], want[1:], rtol=1e-4, atol=1e-6)
        frozen = [n for n in names if BC.FREEZE[c.form] and n.startswith("frame_dim_reshape_")
                  and (c.form == "step-freeze-all" or n.startswith("frame_dim_reshape_0."))]
        assert len(frozen) == {"step": 0, "step-freeze": 2, "step-freeze-all": 6}[c.form]
        for n in frozen:              # a frozen tensor's segment of the bucket is +0.0 to everyone behind the backward
            assert not gv[n].any(), n
        names = [n for n in names if n not in frozen]
    res = GP.tensor_errors(names, gv, ref["hi"], ref["lo"], BC.bar_of(c), zeros=BC.zeros(c.shape, c.form), what="backward route " + BC.case_id(c))
    if not c.form.startswith("step"):
        assert not res.nosignal and len(res) + len(res.zero) == len(names)      # O(1) external gradients: every tensor carries signal


OPERANDS = [c for c in BC.CASES if not BC.has_reference(c)]


@pytest.mark.parametrize("c", OPERANDS, ids=[BC.case_id(c) for c in OPERANDS])
def test_operands_mode_backward_runs_at_every_shape(E, c):
    """Operands mode has no discriminating reference (module docstring), so this is no parity test: the call is accepted, every used
    element is finite and the tensors sit where test_gpu_net.py::test_bf16_operand_mode_c3 puts the mode against the plain oracle
    (own-norm error: median < 4e-2, worst < 0.2) -- a refused, missing or doubled product is far outside that.
    Regression: B * T of a text stream (no-fold: 3 * 6 = 18) or of a text run (fold-av-ne: 2 * 9 = 18) that is no multiple of 4 went to
    the bf16-operand TN kernel, which takes K in whole fours, and sdumc_net_backward came back with SDUMC_EINVAL; such a product now
    multiplies in fp32."""
    got = run_case(E, c)
    lay, gv = _views(E, c, got["grads"])
    assert torch.isfinite(got["grads"][_used(lay)]).all()
    hi = BC.reference(c._replace(storage="fp32"))["hi"]
    errs = {k: float((gv[k].double() - hi[k]).norm() / hi[k].norm()) for k in lay.live_names()}
    worst = max(errs, key=errs.get)
    print("backward route %s vs the plain fp64 oracle: median %.3g, worst %s = %.3g" % (BC.case_id(c), float(np.median(list(errs.values()))), worst, errs[worst]))
    assert float(np.median(list(errs.values()))) < 4e-2 and errs[worst] < 0.2


# ---- (c) lanes change nothing -----------------------------------------------------------------------------------------------------
LANE_PLACEMENT = ("early_lane_a", "early_lane_t", "early_lane_v", "dw_on_lane3_a", "dw_on_lane3_t", "dw_on_lane3_v")
MULTI = [c for c in BC.CASES if BC.options(c.setting)["concurrency"] == 1]


def _one_lane(c):
    """the case with concurrency 0 and everything else the same (backward_cases.py names the one-lane partner of every setting)"""
    one = c._replace(setting=BC.ONE_LANE_PARTNERS[c.setting])
    assert BC.options(one.setting) == {**BC.options(c.setting), "concurrency": 0}
    return one


@pytest.mark.parametrize("c", MULTI, ids=[BC.case_id(c) for c in MULTI])
def test_lanes_change_nothing(E, c):
    """every multi-lane case against the same case on one lane"""
    one = _one_lane(c)
    four = run_case(E, c)
    again = run_case(E, c, cache=False)
    assert _same_bucket(E, c, four["grads"], again["grads"]), "the multi-lane call run twice"
    if "losses" in four:
        assert np.array_equal(four["losses"], again["losses"])
    ra, rb = records(E, c), records(E, one)
    same = all({k: v for k, v in ra[ph].items() if k not in LANE_PLACEMENT} == {k: v for k, v in rb[ph].items() if k not in LANE_PLACEMENT}
               for ph in ra)
    if not same:
        assert c.form == "phased", "only a phased call's route depends on the lanes"      # (its own-lane early dX; (b) holds it)
        return
    got = run_case(E, one)
    assert _same_bucket(E, c, four["grads"], got["grads"]), f"{BC.case_id(c)} against {BC.case_id(one)}"
    if "losses" in four:
        assert np.array_equal(four["losses"], got["losses"])


# ---- (d) phased calls -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in BC.CASES if c.form == "phased"], ids=[BC.case_id(c) for c in BC.CASES if c.form == "phased"])
def test_phase_0_finishes_the_early_slice_and_phase_1_leaves_it(E, c):
    got = run_case(E, c)
    rec = records(E, c)[1]
    lay, _ = _views(E, c, got["grads"])
    used = _used(lay)
    p0, final = got["phase0"], got["grads"]
    early = used[:lay.early]
    assert torch.isfinite(p0[:lay.early][early]).all()
    assert torch.equal(p0[:lay.early][early], final[:lay.early][early])      # bit-unchanged by phase 1
    # the late slice after phase 0: NaN, but for the Cross_Attention input_proj gradients that leave behind phase 0's pooling backward
    pending = used.clone()
    left = []
    for m, suffix in enumerate("atv"):
        if rec[f"ca_dw_grouped_{suffix}"]:
            for w in ("weight", "bias"):
                n = f"cross_att_fra2utt_{m}.input_proj.{w}"
                off, shape, _ = lay.entries[n]
                pending[off:off + int(np.prod(shape))] = False
                left.append((off, int(np.prod(shape))))
    assert not torch.isfinite(p0[lay.early:][pending[lay.early:]]).any()
    for off, n in left:
        assert torch.isfinite(p0[off:off + n]).all() and torch.equal(p0[off:off + n], final[off:off + n])
    assert torch.isfinite(final[used]).all()
