"""The forward pass's schedule (engine.hip: plan_forward -> FwdSchedule, read by forward() and its parts).
  (a) which GEMM kernels one sdumc_net_forward launches, per mode: the {variant: launches} report of sdumc_profile_report against a
      table written here.  The table was recorded ONCE, from the library of the commit before the schedule became a record, and says
      why each count is what it is: a route that moves (another frame-projection kernel, the text slot's two streams in one launch or
      in two, the key projections grouped or one by one) changes a row.
  (b) what the schedule must NOT change: the five outputs of a train-mode forward are bit for bit the same whatever lane carries the
      Cross_Attention key projections (background lane 0 / 2 / 3), with and without real lanes (concurrency 0 / 1), and as the forward
      leg of sdumc_train_step.
B = 2, widths (64, 128, 64, 128); T = (130, 6, 96, 6) and (130, 6, 96, 9): audio (three 64-frame chunks, the third ragged) and video
take the fused projection + pooling kernel at their FRA2UTT site in plain fp32 (T >= 96), text keeps the GEMM + pooling pair; equal
text / feat4 lengths make one run of the text slot, unequal ones two."""
import pytest
import torch

from tests.test_gpu_perlayer import gemm_variants

pytestmark = pytest.mark.gpu

B = 2
DIMS = (64, 128, 64, 128)
DIMS_B1 = (128, 128, 128, 128)      # bf16 storage: the fragment-major weight route needs widths in whole 128-element tiles
T_EQ, T_NE = (130, 6, 96, 6), (130, 6, 96, 9)
DIMS_2K = (64, 2048, 64, 2048)      # a long-K text slot: the few-row / long-K split of the plane and the wide kernel
T_32, T_32_NE = (130, 32, 96, 32), (130, 32, 96, 9)
NAMES = ("vals", "fused", "rnc", "text_hidden", "cross_text")


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import engine
    return engine


_flats, _batches = {}, {}


def _flat(E, dims):
    """the parameters of `dims` (a fresh device copy per caller: a train step updates them)"""
    from oracle import sdumc_oracle as O
    from tests.test_gpu_net import flat_from
    if dims not in _flats:
        _flats[dims] = flat_from(E, O.init_params(dims, seed=1), dims)[0]
    return _flats[dims].clone()


def _batch(T, dims):
    from oracle import sdumc_oracle as O
    if (T, dims) not in _batches:
        _batches[(T, dims)] = tuple(t.cuda() for t in O.synthetic_batch(B, T, dims, seed=2))
    return _batches[(T, dims)]


# storage / arithmetic of a call: (NetCall's bf16, planes, widths)
KINDS = {"planes": (False, True, DIMS), "fp32": (False, False, DIMS), "bf16s": (True, False, DIMS), "bf16s128": (True, False, DIMS_B1),
         "bf16op": ("operands", False, DIMS), "planes2k": (False, True, DIMS_2K), "fp32w2k": (False, False, DIMS_2K)}


def _call(E, kind, T, streams, train, ctx, bits_next=False):
    bf16, planes, dims = KINDS[kind]
    audio, text, video, feat4, _ = _batch(T, dims)
    rng = E.RngState(3, "cuda") if train else None
    return E.NetCall(_flat(E, dims), audio, [text, feat4][:streams], video, train, rng, bf16=bf16, planes=planes, ctx=ctx,
                     bits_next=bits_next)


def _ctx(E, background=None, cluster=None, concurrency=None):
    ctx = E.ExecContext()
    ctx.set_option("background_lane", background)
    ctx.set_option("chain_cluster", cluster)
    ctx.set_option("concurrency", concurrency)
    return ctx


# ---- (a) the route is the record's ---------------------------------------------------------------------------------------------
# mode -> (kind, T, streams, train, background lane, chain_cluster) and the report of one forward.
# Every forward makes, per modality, one frame projection per run of its features (audio / video: one, shared by both streams; the
# text slot: one per stream, or ONE for both when the route takes both in a launch), and one key projection per (site, run of the
# modality's rows) -- minus the FRA2UTT sites that go through the fused projection + pooling kernel, which is no GEMM launch.
ROUTES = {
    "planes-train": ("planes", T_EQ, 2, True, 3, None),
    "planes-eval": ("planes", T_EQ, 2, False, 3, None),
    "planes-train-ne": ("planes", T_NE, 2, True, 3, None),
    "planes-eval-ne": ("planes", T_NE, 2, False, 3, None),
    "planes-train-s1": ("planes", T_EQ, 1, True, 3, None),
    "planes-train-bg0": ("planes", T_EQ, 2, True, 0, None),
    "planes-train-cl0": ("planes", T_EQ, 2, True, 3, 0),
    "planes-train-cl1": ("planes", T_EQ, 2, True, 3, 1),
    "fp32-train": ("fp32", T_EQ, 2, True, 3, None),
    "fp32-eval-ne": ("fp32", T_NE, 2, False, 3, None),
    "fp32-train-bg0": ("fp32", T_EQ, 2, True, 0, None),
    "fp32-train-s1-bg0": ("fp32", T_EQ, 1, True, 0, None),
    "bf16s-train": ("bf16s", T_EQ, 2, True, 3, None),
    "bf16s-eval-ne": ("bf16s", T_NE, 2, False, 3, None),
    "bf16s-train-bg0-cl0": ("bf16s", T_EQ, 2, True, 0, 0),
    "bf16s128-train": ("bf16s128", T_EQ, 2, True, 3, None),
    "bf16s128-eval-ne": ("bf16s128", T_NE, 2, False, 3, None),
    "bf16s128-train-s1-bg0": ("bf16s128", T_EQ, 1, True, 0, None),
    "bf16op-train": ("bf16op", T_EQ, 2, True, 3, None),
    "bf16op-eval-s1-bg0": ("bf16op", T_NE, 1, False, 0, None),
    # the text slot's rule: B * T_text = 64 rows, a whole tile, so a route that takes two tensors in a launch projects both streams at once
    "planes2k-train-t32": ("planes2k", T_32, 2, True, 3, None),
    "planes2k-train-t32-ne": ("planes2k", T_32_NE, 2, True, 3, None),
    "planes-train-t32": ("planes", T_32, 2, True, 3, None),
    "fp32w2k-train-t32": ("fp32w2k", T_32, 2, True, 3, None),
    "bf16s128-train-t32": ("bf16s128", T_32, 2, True, 3, None),
    "bf16s128-eval-t32-ne": ("bf16s128", T_32_NE, 2, False, 3, None),
}
P3, P3M = "gemm_p3_nt_bf16x3", "gemm_p3_nt_masked_bf16x3"
TABLE = {
    # planes: projections audio, video, text, feat4 (128 columns: no split, one launch per stream) = 4 plain; keys with the keep-bits
    # fused on A = masked: text's FRA2UTT site (audio / video: the fused kernel) + the three Cross_Attention sites = 4
    "planes-train": {P3: 4, P3M: 4},
    "planes-eval": {P3: 8},                    # the same eight launches, no mask to fuse
    "planes-train-ne": {P3: 4, P3M: 6},        # two text runs: both text sites twice
    "planes-eval-ne": {P3: 10},
    "planes-train-s1": {P3: 3, P3M: 4},        # one stream: no feat4 projection
    "planes-train-bg0": {P3: 4, P3M: 4},       # no background lane: the plane keys are one launch per site on any lane
    "planes-train-cl0": {P3: 4, P3M: 4},       # chain.hip or the clustered stages: no GEMM launch either way
    "planes-train-cl1": {P3: 4, P3M: 4},
    # fp32 without planes: the generic GEMM picks the tile -- the 4 projections (K = 64 / 128) take the small kernel; the keys with a
    # dropout fused on A (text's FRA2UTT site + 3 Cross_Attention sites) the 64x64 one; no wide-kernel launch at 128 columns
    "fp32-train": {"gemm_nt_64x64": 4, "gemm_small_nt": 4},
    "fp32-eval-ne": {"gemm_nt_64x64": 2, "gemm_small_nt": 8},            # no dropout: text's four 12- / 18-row key launches go small too
    "fp32-train-bg0": {"gemm_nt_64x64": 3, "gemm_small_nt": 4},          # text: both sites' keys as ONE grouped launch
    "fp32-train-s1-bg0": {"gemm_nt_64x64": 3, "gemm_small_nt": 3},       # ... and no feat4 projection
    # bf16 storage at widths that are no whole 128-element tiles: no fragment-major weights, the LDS-staged tiles.  No fused FRA2UTT
    # kernel in bf16: 4 projections + 6 key projections
    "bf16s-train": {"gemm_bf16s_nt": 10},
    "bf16s-eval-ne": {"gemm_bf16s_nt": 12},                              # two text runs
    "bf16s-train-bg0-cl0": {"gemm_bf16s_nt": 7},                         # both sites' keys grouped per modality: 4 + 3
    # bf16 storage on fragment-major weights: gemm_b1 for all ten, none on gemm_bf16's tiles; its keys are never grouped
    "bf16s128-train": {"gemm_b1_nt_bf16": 10},
    "bf16s128-eval-ne": {"gemm_b1_nt_bf16": 12},
    "bf16s128-train-s1-bg0": {"gemm_b1_nt_bf16": 9},
    # bf16 = 1 (operands rounded while staged): the generic GEMM's bf16 tiles, no fused FRA2UTT kernel: 4 + 6; grouped keys: 3 + 3
    "bf16op-train": {"gemm_bf16_nt_64x64": 10},
    "bf16op-eval-s1-bg0": {"gemm_bf16_nt_64x64": 6},
    # planes, text width 2048 and 64 text rows: few rows, long K -> text and feat4 leave as ONE split launch: 3 projections
    "planes2k-train-t32": {P3: 3, P3M: 4},
    "planes2k-train-t32-ne": {P3: 3, P3M: 6},      # ... also when feat4's 18 rows are no whole tile: they follow text's 64
    "planes-train-t32": {P3: 4, P3M: 4},           # 128 columns: no split, so one launch per stream
    # no planes, the same shape: text and feat4 through the wide kernel with K split (one launch per stream), the rest as above
    "fp32w2k-train-t32": {"gemm_nt_64x64": 4, "gemm_small_nt": 2, "gemm_wide_nt_bf16x3": 2},
    "bf16s128-train-t32": {"gemm_b1_nt_bf16": 9},      # gemm_b1 takes both text streams in a launch at any width: 3 + 6
    "bf16s128-eval-t32-ne": {"gemm_b1_nt_bf16": 11},   # ... 3 + 8 with two text runs
}


def route_report(E, mode):
    kind, T, streams, train, background, cluster = ROUTES[mode]
    call = _call(E, kind, T, streams, train, _ctx(E, background, cluster))
    return gemm_variants(call.forward)


@pytest.mark.parametrize("mode", list(ROUTES))
def test_forward_launches_the_kernels_of_its_route(E, mode):
    got = route_report(E, mode)
    print(mode, got)
    assert got == TABLE[mode], mode


# ---- (b) the schedule changes nothing it should not ----------------------------------------------------------------------------
_ref = {}


def _forward_outputs(E, kind, T, background, concurrency):
    call = _call(E, kind, T, 2, True, _ctx(E, background, None, concurrency), bits_next=True)
    outs = [t.clone() for t in call.forward()]
    torch.cuda.synchronize()
    return outs


def _reference(E, kind, T):
    if (kind, T) not in _ref:
        _ref[(kind, T)] = _forward_outputs(E, kind, T, 3, 1)
    return _ref[(kind, T)]


@pytest.mark.parametrize("concurrency", [0, 1])
@pytest.mark.parametrize("background", [0, 2, 3])
@pytest.mark.parametrize("T", [T_EQ, T_NE], ids=["eq", "ne"])
@pytest.mark.parametrize("kind", ["planes", "fp32", "bf16s128"])
def test_outputs_do_not_depend_on_the_lanes(E, kind, T, background, concurrency):
    want = _reference(E, kind, T)
    got = _forward_outputs(E, kind, T, background, concurrency)
    for name, a, b in zip(NAMES, got, want):
        assert torch.equal(a, b), f"{name}: background lane {background}, concurrency {concurrency} against 3 / 1"


@pytest.mark.parametrize("T", [T_EQ, T_NE], ids=["eq", "ne"])
@pytest.mark.parametrize("kind", ["planes", "fp32", "bf16s128"])
def test_forward_leg_of_the_train_step_equals_the_stand_alone_forward(E, kind, T):
    """same parameters, seed and call index: the step's forward writes the five outputs the stand-alone call writes (the step's
    Adam update comes after them)."""
    bf16, planes, dims = KINDS[kind]
    want = _reference(E, kind, T)
    step = E.TrainStep(_flat(E, dims), B, T, dims, seed=3, bf16=bf16, planes=planes, ctx=_ctx(E))
    step.set_batch(*_batch(T, dims))
    step.run()
    torch.cuda.synchronize()
    for name, a, b in zip(NAMES, (step.vals, step.fused, step.rnc, step.text_hidden, step.cross_text), want):
        assert torch.equal(a, b), name
