"""The bits of every launch of adam.hip, held to tests/golden/adam_bits.npz: SHA-256 digests of the output bytes, recorded once on an
MI355X from the kernels as they were BEFORE their forms were folded into shared bodies (tests/golden/make_adam_bits.py; the runs are the
functions of this file, so fixture and test cannot drift apart).  The recorder ran every case twice and refused to write unless the two
digests agreed.  What adam.hip promises is bits, not instruction streams: this file is where that promise is pinned.

FLAT BUCKET (sdumc_adam_step, _step_rates, _step_ema, sdumc_adamw_step): n = 2307 = 2 * 1024 + 256 + 3 elements -- three workgroups,
the last one a single wave, and a three-element scalar tail [2304, 2307).  Values drawn like tests/adamw_ref.inputs, moments from
zero, the average from values of its own; three steps with a fresh gradient and hyper[0] = LR * adamw_ref.lr_lambda(step) rewritten
in between, so the decay factor follows the learning rate.  {no table, table} x {no average, w = 0.1, warm-up} x {coupled, decoupled};
decay 0.9 without warm-up is w = 0.1, ema_lerp's w < 0.5 branch; with warm-up w = 1 - min(0.9, (1 + t) / (10 + t)) = 9/11, 3/4, 9/13
>= 0.5 in steps 1 to 3.  The table (TABLE below), a wave being 256 elements and a group 4:
  (0, 300, 2, 1)          wave [0, 256) wholly inside one segment; wave [256, 512) meets a boundary
  padding [300, 341)      the groups [300, 340): 16 bytes wholly inside padding
  (341, 20, .5, 2)        lr_scale = 0.5, wd_scale = 2; group [340, 344) straddles at residue 1, so does [360, 364)
  (362, 100, 0, 1)        lr_scale == 0 (the parameter stays, the moments advance); starts and ends at residue 2
  (463, 200, frozen)      a frozen segment with unaligned ends, residue 3 at both
  (663, 1400, .25, .5)    waves [768, 2048) wholly inside; its start shares the group [660, 664) with the frozen segment
  (2101, 205, 4, .25)     starts at residue 1 and reaches into the scalar tail (2304, 2305); 2306 is trailing padding inside the tail
Digested after step 3: param, exp_avg, exp_avg_sq, ema (where there is one), hyper.

PER-PARAMETER (sdumc_adam_multi, sdumc_adamw_multi, each followed by sdumc_ema_multi): tensors of 1, 3, 1024, 1025 and 2051 elements as
views into one buffer, each at a 16-byte aligned start (lead 0: 16 bytes per lane) and the same views shifted by one element (lead 1: one
float per lane); and 97 tensors of 5 elements, which takes a second launch.  Two steps (learning rates as above); the average takes
w = 0.1 after the first and w = 0.75 after the second.  Digested: the parameter, moment and average buffers whole, and hyper.

FUSED STEP (TrainStep, the scalar tail's weighted total and dropout counter, the guard's hold): smoke()'s shape -- dims (64, 32, 48, 32),
B = 4, T = (21, 5, 13, 4), the oracle's synthetic batch -- two steps, four ways: defaults | clip_norm small enough to clip |
decoupled_decay with freeze=, lr_scale= and ema_decay=0.9 | skip_nonfinite with a NaN label in step 2 only (as tests/test_gpu_grad_guard.py
plants it: nothing faults, the step is held).  Digested: params, adam_m, adam_v, the average, losses, hyper, the dropout counter word.
The recorder would have left a fused case out of the fixture had two runs of it on the recorded library differed; all four reproduced
their bits and are in it.  A case that is not in the fixture fails here (it is never skipped)."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import adamw_ref  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "adam_bits.npz")
LR, WD = 1e-3, 1e-2

# ------------------------------------------------------------------------------------------------------------------ flat bucket
N = 2307
TABLE = [(0, 300, 2.0, 1.0, False), (341, 20, 0.5, 2.0, False), (362, 100, 0.0, 1.0, False), (463, 200, 1.0, 1.0, True),
         (663, 1400, 0.25, 0.5, False), (2101, 205, 4.0, 0.25, False)]
AVERAGES = {"noema": None, "ema": (0.9, False), "emawarm": (0.9, True)}
FLAT = [(table, avg, dec) for table in (False, True) for avg in AVERAGES for dec in (False, True)]
assert N == 2 * 1024 + 256 + 3 and all(a + n <= b for (a, n, *_), (b, *_) in zip(TABLE, TABLE[1:])) and TABLE[-1][0] + TABLE[-1][1] == N - 1
assert {off % 4 for off, *_ in TABLE} == {0, 1, 2, 3} and (N // 4) * 4 < TABLE[-1][0] + TABLE[-1][1] < N


def flat_key(table, avg, dec):
    return f"flat_{'table' if table else 'notable'}_{avg}_{'decoupled' if dec else 'coupled'}"


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def _values(n, gen, steps):
    """like adamw_ref.inputs: p = +-2^U(-4, 4), g = N(0, 1) * 2^U(-6, 2); and an average of p's distribution"""
    def signed():
        sign = torch.randint(0, 2, (n,), generator=gen) * 2.0 - 1.0
        return (sign * torch.exp2(torch.rand(n, generator=gen) * 8 - 4)).float()
    p = signed()
    grads = [(torch.randn(n, generator=gen) * torch.exp2(torch.rand(n, generator=gen) * 8 - 6)).float() for _ in range(steps)]
    return p, grads, signed()


def run_flat(ops, table, avg, dec):
    """three steps of the public entry that names this form -> the tensors to digest"""
    p0, grads, a0 = _values(N, torch.Generator().manual_seed(4100), 3)
    p, a = p0.cuda(), a0.cuda()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    hyper = torch.tensor([LR, 0.0, 0.0, 0.0], device="cuda")
    assert all(x.data_ptr() % 16 == 0 for x in (p, a, m, v))
    segments = TABLE if table else None
    ema = AVERAGES[avg]
    for e, g in enumerate(grads):
        hyper[0] = LR * adamw_ref.lr_lambda(e)
        g = g.cuda()
        if dec:
            kw = dict(ema=a, ema_decay=ema[0], ema_warmup=ema[1]) if ema else {}
            ops.adamw_step(p, g, m, v, hyper, weight_decay=WD, segments=segments, **kw)
        elif ema:
            ops.adam_step_ema(p, g, m, v, hyper, a, ema[0], ema_warmup=ema[1], segments=segments, weight_decay=WD)
        elif table:
            ops.adam_step_rates(p, g, m, v, hyper, segments, weight_decay=WD)
        else:
            ops.adam_step(p, g, m, v, hyper, weight_decay=WD)
    torch.cuda.synchronize()
    assert float(hyper[1]) == 3.0 and bool(torch.isfinite(p).all())
    return [p, m, v] + ([a] if ema else []) + [hyper]


# ------------------------------------------------------------------------------------------------------------------ per-parameter
SIZES = (1, 3, 1024, 1025, 2051)
MULTI = [(dec, shape) for dec in (False, True) for shape in ("lead0", "lead1", "n97")]
EMA_W = (0.1, 0.75)


def multi_key(dec, shape):
    return f"multi_{'adamw' if dec else 'adam'}_{shape}"


def _multi_layout(shape):
    """-> ([(offset, n)], buffer length): the views' places in the buffer"""
    if shape == "n97":
        return [(5 * i, 5) for i in range(97)], 5 * 97 + 3
    lead, segs, cur = int(shape[-1]), [], 0
    for n in SIZES:
        segs.append((cur + lead, n))
        cur += (n + 3) // 4 * 4
    return segs, cur + 4


def run_multi(ops, dec, shape):
    """two steps of sdumc_adam_multi / sdumc_adamw_multi, each followed by sdumc_ema_multi -> the tensors to digest"""
    segs, total = _multi_layout(shape)
    gen = torch.Generator().manual_seed(4200 + len(segs))
    p0, grads, a0 = _values(total, gen, 2)
    P, A = p0.cuda(), a0.cuda()
    M, V = torch.zeros_like(P), torch.zeros_like(P)
    hyper = torch.tensor([LR, 0.0, 0.0, 0.0], device="cuda")
    params, emas, offs = [P[o:o + n] for o, n in segs], [A[o:o + n] for o, n in segs], [o for o, _ in segs]
    if shape == "lead0":
        assert all(x.data_ptr() % 16 == 0 for x in params + emas)
    if shape == "lead1":
        assert all(x.data_ptr() % 16 == 4 for x in params + emas)
    step = ops.adamw_multi if dec else ops.adam_multi
    for e, (g, w) in enumerate(zip(grads, EMA_W)):
        hyper[0] = LR * adamw_ref.lr_lambda(e)
        G = g.cuda()
        step(params, [G[o:o + n] for o, n in segs], M, V, offs, hyper, weight_decay=WD)
        ops.ema_multi(emas, params, w)
    torch.cuda.synchronize()
    assert float(hyper[1]) == 2.0 and bool(torch.isfinite(P).all())
    return [P, M, V, A, hyper]


# ------------------------------------------------------------------------------------------------------------------ fused step
DIMS, B, T = (64, 32, 48, 32), 4, (21, 5, 13, 4)
FUSED = {"defaults": {}, "clip": dict(clip_norm=1e-2),
         "decoupled": dict(decoupled_decay=True, freeze=("frame_dim_reshape_1.*",), lr_scale={"cross_*": 0.5, "fc_out_v.*": 2.0},
                           ema_decay=0.9, weight_decay=1e-2),
         "held": dict(skip_nonfinite=True)}


def fused_key(way):
    return f"fused_{way}"


def run_fused(way):
    """two steps of TrainStep on smoke()'s shape -> the tensors to digest"""
    from oracle import sdumc_oracle as O
    from sdumc_amd import engine
    P = O.init_params(DIMS, seed=1)
    lay = engine.ParamLayout.get(*DIMS[:3])
    flat = torch.zeros(lay.total)
    for k, v in lay.views(flat).items():
        v.copy_(P[k])
    batch = [t.cuda() for t in O.synthetic_batch(B, T, DIMS, seed=2)]
    ts = engine.TrainStep(flat.cuda(), B, T, DIMS, lr=LR, seed=3, **FUSED[way])
    for e in range(2):
        labels = batch[4].clone()
        if way == "held" and e == 1:
            labels[1] = float("nan")
        ts.set_batch(*batch[:4], labels)
        ts.run()
        torch.cuda.synchronize()
    guard = ts.guard.tolist() if ts.guard is not None else None
    if way == "clip":
        assert 0.0 < guard[1] < 1.0, guard
    if way == "held":
        assert guard[3] == 1.0 and float(ts.hyper[1]) == 1.0, guard
    else:
        assert float(ts.hyper[1]) == 2.0
    assert ts.rng.call == 4
    ema = getattr(ts, "ema_params", None)
    return [ts.params, ts.adam_m, ts.adam_v] + ([ema] if ema is not None else []) + [ts.losses, ts.hyper, ts.rng.t[2:3]]


# ------------------------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import ops
    return ops


@pytest.fixture(scope="module")
def bits(golden):
    return golden("adam_bits")


def _hold(bits, key, tensors):
    assert key in bits.files, key + ": not in the fixture"
    got, want = digest(tensors), bits[key]
    print("ADAMBITS", key, got.tobytes().hex()[:16], want.tobytes().hex()[:16])
    assert np.array_equal(got, want), key + ": the outputs' bytes are not the recorded ones"


@pytest.mark.parametrize("table,avg,dec", FLAT)
def test_flat_bits(ops, bits, table, avg, dec):
    _hold(bits, flat_key(table, avg, dec), run_flat(ops, table, avg, dec))


@pytest.mark.parametrize("dec,shape", MULTI)
def test_multi_bits(ops, bits, dec, shape):
    _hold(bits, multi_key(dec, shape), run_multi(ops, dec, shape))


@pytest.mark.parametrize("way", list(FUSED))
def test_fused_bits(ops, bits, way):
    _hold(bits, fused_key(way), run_fused(way))
