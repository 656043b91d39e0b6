"""The case matrix of the backward schedule (engine.hip: plan_backward -> BwdSchedule): plain data plus builders, no fixtures, no GPU
at import.  tests/test_gpu_backward_routes.py runs every case on the device; tests/test_backward_routes_cpu.py keeps the reference
side of every case honest without one.

A case is (shape, storage, form, setting):

  shape     SHAPES: widths, B, T (audio, text, video, feat4).  D = 256 is fixed inside the engine.
  storage   fp32 | planes (fp32 with the features also given as bf16 planes) | bf16s (bf16 storage) | bf16op (operands mode)
  form      net     a train-mode NetCall forward + backward, two streams, O(1) external gradients on all five outputs
            s1      the same with one stream
            eval    the same in eval mode (no dropout)
            phased  the same forward, then sdumc_net_backward_phase 0 and 1 through trainer.HipBackend (its d_* buffers filled with the
                    same external gradients: the reference of `net` is the reference of `phased`)
            step / step-freeze / step-freeze-all   one TrainStep (its backward is planned from the forward's record); the freeze forms
                    with freeze=("frame_dim_reshape_0.*",) / ("frame_dim_reshape_*",)
  setting   SETTINGS: what the ExecContext's options are, named by what they change from the default (3, 1, 1, 15) =
            (background_lane, concurrency, chain_cluster, split)

Only the public surface: ExecContext.set_option, the arguments of NetCall / TrainStep / HipBackend, freeze=.  No SDUMC_* environment
switch (statics read once per process), no process-wide setter, no capture.  The two pairs that name the default's own value -- bg3+conc0
and split7+bg3 -- ARE conc0 and split7 under a default that is set explicitly: ALIASES says so, and the matrix runs each once.

The reference of a case depends on (shape, storage's arithmetic, form's graph) only, never on the setting: reference() computes it once
per key -- fp64 and fp32, through oracle/sdumc_oracle.py, for bf16 storage through the rounding emulation oracle/bf16_storage.py -- and
every setting of that key shares it unchanged."""
from collections import namedtuple

import torch

# ---- shapes ---------------------------------------------------------------------------------------------------------------------
# name -> (widths (audio, text, video, feat4), B, T (audio, text, video, feat4)).  What plan_backward / make_plan read off them:
SHAPES = {
    # audio and video in the dxfold set (T >= 63 || T == 32), text not; equal text lengths: one text run
    "fold-av": ((64, 128, 64, 128), 2, (130, 6, 96, 6)),
    "fold-av-ne": ((64, 128, 64, 128), 2, (130, 6, 96, 9)),        # two text runs: no fra_fold; four runs in all
    "fold-all": ((64, 128, 64, 128), 2, (64, 32, 63, 32)),         # every modality folds (64 and 63 on the two sides of a chunk; 32)
    "fold-av-128": ((128, 128, 128, 128), 2, (130, 6, 96, 6)),     # bf16 storage on the fragment-major weights (whole 128-element tiles)
    "no-fold": ((64, 32, 64, 32), 3, (40, 6, 20, 6)),              # dx_sum false everywhere; odd B
    "odd-widths": ((37, 32, 42, 32), 4, (13, 5, 9, 3)),            # audio / video widths & 3 != 0: their frame dW is per stream in fp32
    "few-rows": ((16, 16, 16, 16), 1, (6, 1, 5, 2)),               # shared audio / video runs of 6 and 5 rows (< 16): key dW not groupable
    "long": ((16, 16, 16, 16), 1, (2112, 6, 20, 6)),               # 33 chunks of 64 frames: no fra_fold while clustered
    "wide-V": ((16, 16, 16, 16), 65, (8, 3, 5, 3)),                # V = 130: 65 clusters of 4 workgroups do not fit 256 CUs
    "no-chain": ((16, 16, 16, 16), 257, (4, 2, 3, 2)),             # V = 514 > 512: the per-layer utterance path
    # bf16 storage, eval: audio's shared run has 2 * 20 = 40 rows < 64: its key dW is not groupable, so dw_on_lane3 applies; video folds
    "bf16-few": ((64, 64, 64, 64), 2, (20, 3, 70, 5)),
}
P_SEED, BATCH_SEED, DOUT_SEED, SEED, CALL0 = 31, 17, 5, 99, 0      # (CALL0 = 0: a fresh HipBackend's run state starts there)

# ---- settings -------------------------------------------------------------------------------------------------------------------
DEFAULT = {"background_lane": 3, "concurrency": 1, "chain_cluster": 1, "split": 15}
SETTINGS = {
    "default": {},
    "bg0": {"background_lane": 0},
    "bg2": {"background_lane": 2},
    "conc0": {"concurrency": 0},
    "cl0": {"chain_cluster": 0},
    "split7": {"split": 7},         # no rows bit (8): the rows launches multiply in plain fp32 and fold nothing
    "split14": {"split": 14},       # no group bit (1): the grouped weight-gradient launch in plain fp32
    "split0": {"split": 0},
    "bg0+conc0": {"background_lane": 0, "concurrency": 0},
    "bg0+cl0": {"background_lane": 0, "chain_cluster": 0},
}
# The one-lane partner of every multi-lane setting: what "lanes change nothing" runs it against.  conc0 and bg0+conc0 are settings of the
# matrix; the others are partners only (ONE_LANE): no case is named after them and the route table has no row for them.
ONE_LANE_PARTNERS = {n: ("conc0" if n == "default" else n + "+conc0") for n in SETTINGS if "concurrency" not in SETTINGS[n]}
ONE_LANE = {p: {**SETTINGS[n], "concurrency": 0} for n, p in ONE_LANE_PARTNERS.items() if p not in SETTINGS}
ALIASES = {"bg3+conc0": "conc0", "split7+bg3": "split7"}
SINGLES = ("default", "bg0", "bg2", "conc0", "cl0", "split7", "split14", "split0")
OPTION_VALUES = {"background_lane": (0, 2, 3), "concurrency": (0, 1), "chain_cluster": (0, 1), "split": tuple(range(16))}

STORAGES = {"fp32": (False, False), "planes": (False, True), "bf16s": (True, False), "bf16op": ("operands", False)}   # (bf16=, planes=)
FORMS = ("net", "s1", "eval", "phased", "step", "step-freeze", "step-freeze-all")
FREEZE = {"step": None, "step-freeze": ("frame_dim_reshape_0.*",), "step-freeze-all": ("frame_dim_reshape_*",)}

Case = namedtuple("Case", "shape storage form setting")


def case_id(c):
    return "/".join(c)


def _matrix():
    cases = []
    add = lambda *c: cases.append(Case(*c))
    # the default and the seven single-option settings at the three fold shapes and no-fold
    for shape in ("fold-av", "fold-av-ne", "fold-all", "no-fold"):
        for setting in SINGLES:
            add(shape, "fp32", "net", setting)
    # the remaining settings at fold-av and no-fold: pairs, phased calls, call forms, storages
    for shape in ("fold-av", "no-fold"):
        for setting in ("bg0+conc0", "bg0+cl0"):
            add(shape, "fp32", "net", setting)
        for setting in ("default", "conc0", "bg0"):
            add(shape, "fp32", "phased", setting)
        add(shape, "fp32", "s1", "default")
        add(shape, "fp32", "eval", "default")
        for setting in ("default", "conc0", "bg0"):
            add(shape, "bf16op", "net", setting)
    add("fold-av-ne", "bf16op", "net", "default")      # a text run of 2 * 9 = 18 rows: no multiple of 4 (the per-layer key dW's K)
    # planes and bf16 storage where the storage admits them (widths in whole 64-element tiles)
    for shape in ("fold-av", "fold-av-ne", "fold-all"):
        for setting in ("default", "conc0"):
            add(shape, "planes", "net", setting)
            add(shape, "bf16s", "net", setting)
    for setting in ("default", "conc0", "bg0"):
        add("fold-av-128", "bf16s", "net", setting)
        add("bf16-few", "bf16s", "eval", setting)
    add("fold-av", "bf16s", "phased", "default")
    # the remaining shapes under the default, conc0 and bg0
    for shape in ("odd-widths", "few-rows", "long", "wide-V", "no-chain"):
        for setting in ("default", "conc0", "bg0"):
            add(shape, "fp32", "net", setting)
    # TrainStep: the backward planned from the forward's record
    add("fold-av", "planes", "step", "default")
    add("fold-av", "bf16s", "step", "default")
    # ... and the merged early launch under each setting that keeps it: in a step the Cross_Attention sites carry ~90 % of dx, so the frame
    # dW sees a relative error of the early dX at nearly its full size (under O(1) external gradients their share is under 20 %)
    for setting in ("conc0", "cl0", "split14"):
        add("fold-av", "fp32", "step", setting)
    add("fold-all", "fp32", "step", "default")
    add("fold-av", "fp32", "step-freeze", "default")
    add("fold-av", "fp32", "step-freeze-all", "default")
    return cases


CASES = _matrix()


def options(setting):
    """the four ExecContext options of a setting, every one set explicitly"""
    name = ALIASES.get(setting, setting)
    return {**DEFAULT, **(SETTINGS[name] if name in SETTINGS else ONE_LANE[name])}


def streams_of(form):
    return 1 if form == "s1" else 2


def train_of(form):
    return form != "eval"


# ---- exact zeros and the helper's other classes ------------------------------------------------------------------------------------
def site_tensors(m):
    """the parameters of modality m's two attention sites that only the softmax's gradient reaches (test_gpu_bf16_edges.py): exactly
    zero where every stream's T is 1"""
    return [f"fra2utt_{m}.attention_context_vector", f"fra2utt_{m}.input_proj.weight", f"fra2utt_{m}.input_proj.bias"] + \
           [f"cross_att_fra2utt_{m}.{p}.{w}" for p in ("query_proj", "input_proj") for w in ("weight", "bias")]


def zeros(shape, form):
    """the tensors that are exactly zero in a case's reference, by name (as ZEROS_ONE_FRAME of test_gpu_bf16_edges.py).  few-rows has a
    one-frame text slot, but its second stream (feat4, two frames) reaches the text sites' tensors: with two streams nothing is zero;
    only a one-stream call at that shape would zero site_tensors(1)."""
    T = SHAPES[shape][2]
    ts = (T[1],) if streams_of(form) == 1 else (T[1], T[3])
    z = []
    if T[0] == 1:
        z += site_tensors(0)
    if all(t == 1 for t in ts):
        z += site_tensors(1)
    if T[2] == 1:
        z += site_tensors(2)
    return tuple(z)


# ---- inputs and references -----------------------------------------------------------------------------------------------------------
_inputs, _refs = {}, {}


def inputs(shape, padded=True):
    """(dims, B, T, P, batch): parameters and the synthetic batch of a shape, on the CPU.  padded, where B > 1: sample 1's audio and the
    last sample's video end in zero padding, which takes part in the softmax as in the reference.  Not in bf16 storage (padded_of): a
    run of identical padded frames multiplies ONE flipped bf16 rounding of their common projection by its length, and the emulation's own
    fp32 evaluation then sits 1.5 - 2.8 % from its fp64 one at fold-all (six of video's Cross_Attention tensors) -- a property of the
    reference that says nothing about a route."""
    if (shape, padded) not in _inputs:
        from oracle import sdumc_oracle as O
        dims, B, T = SHAPES[shape]
        P = O.init_params(dims, seed=P_SEED)
        batch = list(O.synthetic_batch(B, T, dims, seed=BATCH_SEED))
        if B > 1 and padded:
            batch[0][1, (T[0] + 1) // 2:] = 0
            batch[2][B - 1, (T[2] + 2) // 3:] = 0
        _inputs[(shape, padded)] = (dims, B, T, P, batch)
    return _inputs[(shape, padded)]


def padded_of(storage):
    return storage != "bf16s"


def douts(V):
    """O(1) external gradients of the five outputs of V virtual samples (test_gpu_net.py::test_backward_vs_oracle)"""
    g = torch.Generator().manual_seed(DOUT_SEED)
    return [torch.randn(V, 1, generator=g), torch.randn(V, 128, generator=g), torch.randn(V, 64, generator=g),
            torch.randn(V, 256, generator=g), torch.randn(V, 7, 128, generator=g)]


def _call_grads(P, audio, texts, video, train, dout, dtype, emulate):
    """parameter gradients of sum(out * dout) over the streams of one call, in `dtype`; emulate: through the bf16-storage rounding
    emulation (one object per evaluation: it shares the projected audio / video frames of the two streams by the input's identity)"""
    from oracle import sdumc_oracle as O
    from oracle.bf16_storage import Bf16Storage
    st = Bf16Storage() if emulate else None
    leaves = {k: v.detach().to(dtype, copy=True).requires_grad_(not O.is_dead(k)) for k, v in P.items()}      # (P itself stays as it is)
    a, v = audio.to(dtype), video.to(dtype)
    total = 0
    for s, tx in enumerate(texts):
        d = O.DropCtx("philox" if train else "eval", SEED, CALL0 + s)
        y, (z, r, th, ct) = O.forward(leaves, a, tx.to(dtype), v, d, st=st)
        B = y.shape[0]
        for o, do in zip((y, z, r, th, ct), dout):
            total = total + (o * do[s * B:(s + 1) * B].to(dtype).reshape(o.shape)).sum()
    total.backward()
    return {k: t.grad for k, t in leaves.items() if t.grad is not None}


def ref_key(c):
    """what a case's reference depends on: the shape, whether the arithmetic is the rounding emulation's, and the graph"""
    graph = "step" if c.form.startswith("step") else ("net" if c.form == "phased" else c.form)
    return (c.shape, c.storage == "bf16s", graph)


def has_reference(c):
    """operands mode (bf16 = 1) has no discriminating reference: its only oracle bar is 4e-2 / 0.2 (test_gpu_net.py::
    test_bf16_operand_mode_c3), which a wrong kernel passes"""
    return c.storage != "bf16op"


def reference(c):
    """{"hi": fp64 gradients, "lo": fp32 gradients[, "losses": the step's total and six terms in fp64]} of a case, computed once per
    ref_key and left unchanged"""
    key = ref_key(c)
    if key not in _refs:
        from oracle import sdumc_oracle as O
        from oracle.bf16_storage import Bf16Storage
        from tests import grad_parity as GP
        shape, emulate, graph = key
        dims, B, T, P, batch = inputs(shape, not emulate)
        audio, text, video, feat4, _ = batch
        if graph == "step":
            st = lambda: Bf16Storage() if emulate else None
            loss, terms, hi, _ = O.train_step({k: v.double() for k, v in P.items()}, {}, *[t.double() for t in batch], mode="philox",
                                              seed=SEED, step=0, st=st())
            lo = GP.oracle_step_grads(P, batch, SEED, dtype=torch.float32, st=st())
            _refs[key] = {"hi": hi, "lo": lo, "losses": [float(loss)] + [float(t) for t in terms]}
        else:
            texts = [text, feat4][:1 if graph == "s1" else 2]
            dout = douts(len(texts) * B)
            hi = _call_grads(P, audio, texts, video, graph != "eval", dout, torch.float64, emulate)
            lo = _call_grads(P, audio, texts, video, graph != "eval", dout, torch.float32, emulate)
            _refs[key] = {"hi": hi, "lo": lo}
    return _refs[key]


def bar_of(c):
    """(own-norm gradient bar, where it comes from): the project's 2e-4 of every fp32 parity test (test_gpu_net.py), BF16_EMU_GRAD_TOL
    of test_gpu_fullsize.py for bf16 storage against its emulation"""
    if c.storage == "bf16s":
        from tests.test_gpu_fullsize import BF16_EMU_GRAD_TOL
        return BF16_EMU_GRAD_TOL
    return 2e-4


# ---- builders (GPU) --------------------------------------------------------------------------------------------------------------------
def make_ctx(E, setting):
    ctx = E.ExecContext()
    for name, value in options(setting).items():
        ctx.set_option(name, value)
    return ctx


def flat_params(E, shape):
    dims, _, _, P, _ = inputs(shape)      # (the parameters do not depend on the padding)
    lay = E.ParamLayout.get(*dims[:3])
    flat = torch.zeros(lay.total)
    for k, v in lay.views(flat).items():
        v.copy_(P[k])
    return flat.cuda(), lay


def build(E, c, ctx):
    """the object that runs case c under the context: a NetCall (net, s1, eval), a HipBackend (phased) or a TrainStep"""
    dims, B, T, P, batch = inputs(c.shape, padded_of(c.storage))
    bf16, planes = STORAGES[c.storage]
    flat, _ = flat_params(E, c.shape)
    audio, text, video, feat4, vals = [t.cuda() for t in batch]
    if c.form in ("net", "s1", "eval"):
        train = train_of(c.form)
        rng = E.RngState(SEED, "cuda", call=CALL0) if train else None
        return E.NetCall(flat, audio, [text, feat4][:streams_of(c.form)], video, train, rng, bf16=bf16, planes=planes, ctx=ctx)
    if c.form == "phased":
        from sdumc_amd.trainer import HipBackend
        be = HipBackend(flat, B, T, dims, E.DEFAULT_WEIGHTS, 1e-4, (0.9, 0.999), 1e-8, 1e-5, SEED, 0, B, bf16=bf16, planes=planes, ctx=ctx)
        be.set_batch(audio, text, video, feat4, vals)
        return be
    ts = E.TrainStep(flat, B, T, dims, seed=SEED, bf16=bf16, planes=planes, ctx=ctx, freeze=FREEZE[c.form])
    ts.set_batch(audio, text, video, feat4, vals)
    return ts


def schedule_target(obj):
    """what engine.backward_schedule reads the record of: the NetCall itself, a HipBackend's call, the TrainStep"""
    return getattr(obj, "call", obj)
