"""GPU parity tests of the PER-LAYER utterance path: engine.hip::forward steps 3-7 / 9-12 and the mirror backward, built from
grouped sdumc_gemm_f32 launches and the small kernels of elementwise.hip.  It is taken when plan_utterance()'s `chain` is false: V = streams x B
> 512, or SDUMC_CHAIN=0.  The clustered and the one-launch-per-stage kernels (V <= 128, V <= 512) are held to the oracle all over
the suite; this file holds the third path to the same bars:
  (a) forward + backward with external output gradients on both sides of the switch (V = 512 -> chain.hip, V = 514 / 513 -> per
      layer), outputs at 1e-4, every gradient tensor against its own norm at 2e-4;
  (b) one full fused step at B = 300 against O.train_step;
  (c) the GEMM launch counters prove which path a call took;
  (d) SDUMC_CHAIN=0 in a fresh child process puts the smallest shapes (V = 2, 6, 10) on the per-layer path.
Toy widths (24, 16, 20, 16) throughout: the utterance-level network does not depend on the feature widths."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_gpu_configs import close_norm
from tests.test_gpu_net import NAMES, _oracle_grads, close, flat_from

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (24, 16, 20, 16)
TN = (5, 1, 3, 2)            # unequal text / feat4 lengths: two text runs
OUT_TOL, GRAD_TOL = 1e-4, 2e-4
# the three shapes the forced switch runs: (B, T, index of a fully zero video utterance or None)
FORCED_SHAPES = ((1, (1, 1, 1, 1), None), (3, (65, 1, 64, 2), 2), (5, (70, 9, 33, 4), None))


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import engine
    return engine


def out_err(got, want):
    """`close`'s criterion |got - want| <= tol * |want| + tol * max(1, max|want|) as one number: the smallest tol that passes."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double().reshape(got.shape)
    return float(((got - want).abs() / (want.abs() + max(1.0, float(want.abs().max())))).max())


def norm_err(got, want):
    """`close_norm`'s figure: |got - want| / |want| over the whole tensor."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double().reshape(got.shape)
    return float((got - want).norm()) / float(want.norm())


def gemm_launches(fn):
    """Number of sdumc_gemm_f32 launches `fn` makes (one lane, as bench.py's roofline leg counts them)."""
    return sum(gemm_variants(fn).values())


def gemm_variants(fn):
    """{kernel variant: launches} of the GEMM launches `fn` makes (sdumc_profile_report; one lane)."""
    from sdumc_amd import _lib
    lib = _lib.lib
    torch.cuda.synchronize()
    try:
        lib.sdumc_set_concurrency(0)
        lib.sdumc_profile_enable(1)
        fn()
        torch.cuda.synchronize()
        arr = (_lib.ProfEntry * 32)()
        n = lib.sdumc_profile_report(arr, 32)
    finally:
        lib.sdumc_profile_enable(0)
        lib.sdumc_set_concurrency(1)
    assert n > 0, "sdumc_profile_report failed"
    return {arr[i].name.decode(): int(arr[i].launches) for i in range(n) if arr[i].launches}


def net_case(E, B, Tn, streams, mode, zero_video=None, pseed=11, bseed=5, seed=99, call0=4):
    """Forward and backward of one NetCall with external output gradients against the fp64 oracle.  Returns the worst output figure
    (out_err), the worst per-tensor gradient figure (norm_err) and its tensor; asserts nothing."""
    from oracle import sdumc_oracle as O
    P = O.init_params(DIMS, seed=pseed)
    flat, lay = flat_from(E, P, DIMS)
    audio, text, video, feat4, _ = O.synthetic_batch(B, Tn, DIMS, seed=bseed)
    if zero_video is not None:
        video[zero_video] = 0                 # a fully padded utterance: uniform attention over zero frames
    texts = [text, feat4][:streams]
    V = streams * B
    g = torch.Generator().manual_seed(1)
    douts = [torch.randn(V, 1, generator=g), torch.randn(V, 128, generator=g), torch.randn(V, 64, generator=g),
             torch.randn(V, 256, generator=g), torch.randn(V, 7, 128, generator=g)]
    rng = E.RngState(seed, "cuda", call=call0)
    call = E.NetCall(flat, audio.cuda(), [t.cuda() for t in texts], video.cuda(), mode == "train", rng)
    outs = [o.clone() for o in call.forward()]
    grads = call.backward(*[d.cuda().contiguous() for d in douts])
    gv = lay.views(torch.cat([grads.cpu(), torch.zeros(lay.total - lay.live)]))
    res = {"out": 0.0, "grad": 0.0, "grad_tensor": "", "outs": [], "grads": [], "zero": []}
    Pd = {k: v.double() for k, v in P.items()}
    for s, tx in enumerate(texts):
        d = O.DropCtx("eval" if mode == "eval" else "philox", seed, call0 + s)
        y, (z, r, th, ct) = O.forward(Pd, audio.double(), tx.double(), video.double(), d)
        for name, got, want in zip(NAMES, outs, (y, z, r, th, ct)):
            res["outs"].append((f"{name} stream {s}", got[s * B:(s + 1) * B].cpu(), want))
            e = out_err(got[s * B:(s + 1) * B], want)
            if not e <= res["out"]:           # (a NaN takes the place and stays)
                res["out"] = e
    want = _oracle_grads(P, audio, texts, video, mode, seed, call0, douts)
    assert set(want) == set(lay.live_names())
    for k in lay.live_names():
        res["grads"].append((k, gv[k], want[k]))
        if float(want[k].norm()) == 0.0:      # exactly 0 in the oracle (softmax over ONE frame): close_norm's absolute branch holds it
            res["zero"].append(k)
            continue
        e = norm_err(gv[k], want[k])
        if not e <= res["grad"]:              # (a NaN takes the place and stays)
            res["grad"], res["grad_tensor"] = e, k
    return res


def hold(res, what):
    """The bars of (a): every output at the suite's 1e-4, every gradient tensor at 2e-4 of its own norm."""
    for name, got, want in res["outs"]:
        close(got, want, OUT_TOL, f"{what}: {name}")
    for k, got, want in res["grads"]:
        close_norm(got, want, GRAD_TOL, k, what)
    assert res["out"] <= OUT_TOL and res["grad"] < GRAD_TOL, (what, res["out"], res["grad"], res["grad_tensor"])


_cases = {}


def switch_case(E, mode, B, streams):
    key = (mode, B, streams)
    if key not in _cases:
        _cases[key] = net_case(E, B, TN, streams, mode)
    return _cases[key]


# ---- (a) forward and backward on both sides of the switch ----------------------------------------------------------------------
@pytest.mark.parametrize("B,streams", [(256, 2), (257, 2), (513, 1)])
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_switch_forward_backward_vs_oracle(E, mode, B, streams):
    """V = 512 is the last shape chain.hip takes (the yardstick, same seeds); V = 514 (V % 4 = 2) and V = 513 (one stream, V odd) run
    the per-layer path with a ragged last workgroup in the one-wave-per-sample kernels."""
    res = switch_case(E, mode, B, streams)
    print(f"\n{mode} B={B} streams={streams}: outputs {res['out']:.3e}, worst gradient {res['grad']:.3e} ({res['grad_tensor']})")
    hold(res, f"{mode} B={B} streams={streams}")


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_switch_worst_gradient_errors_on_one_line(E, mode):
    a, b = switch_case(E, mode, 256, 2), switch_case(E, mode, 257, 2)
    print(f"\nworst per-tensor gradient error, {mode}: B=256 (chain.hip) {a['grad']:.3e} ({a['grad_tensor']}) | "
          f"B=257 (per layer) {b['grad']:.3e} ({b['grad_tensor']})")
    assert a["grad"] < GRAD_TOL and b["grad"] < GRAD_TOL


# ---- (b) the full fused step at B = 300 ---------------------------------------------------------------------------------------
def test_full_step_b300_vs_oracle(E):
    """V = 600: loss, the six terms, every gradient and the Adam update of one fused step on the per-layer path.  A gradient may
    count as numerically zero only where the ORACLE's own tensor lies below 1e-6 of its largest one (rms): the RnC head's biases,
    which the translation-invariant RnC loss leaves at rounding noise -- two tensors at the most."""
    from oracle import sdumc_oracle as O
    B = 300
    P = O.init_params(DIMS, seed=3)
    flat, lay = flat_from(E, P, DIMS)
    audio, text, video, feat4, vals = O.synthetic_batch(B, TN, DIMS, seed=7)
    ts = E.TrainStep(flat, B, TN, DIMS, seed=5)
    ts.set_batch(audio.cuda(), text.cuda(), video.cuda(), feat4.cuda(), vals.cuda())
    losses = ts.run().cpu().numpy()
    Pd = {k: v.clone() for k, v in P.items()}
    loss, terms, grads, _ = O.train_step(Pd, {}, audio, text, video, feat4, vals, mode="philox", seed=5, step=0)
    print(f"\nB=300 loss {losses[0]:.7g} vs {float(loss):.7g}; terms {losses[1:7]} vs {[float(t) for t in terms]}")
    np.testing.assert_allclose(losses[0], float(loss), rtol=1e-3)
    np.testing.assert_allclose(losses[1:7], [float(t) for t in terms], rtol=1e-3)
    gv = lay.views(torch.cat([ts.grads.cpu(), torch.zeros(lay.total - lay.live)]))
    assert set(grads) == set(lay.live_names())
    rms = {k: float(grads[k].double().pow(2).mean().sqrt()) for k in grads}
    line = 1e-6 * max(rms.values())
    zero, worst = [], (0.0, "")
    for k in lay.live_names():
        if rms[k] < line:
            zero.append(k)
            continue
        worst = max(worst, (norm_err(gv[k], grads[k]), k))
    print(f"B=300 worst per-tensor gradient error {worst[0]:.3e} ({worst[1]}); numerically zero in the oracle: {zero}")
    assert len(zero) <= 2 and set(zero) <= {"orgin_linear_change.0.bias", "orgin_linear_change.2.bias"}, zero
    for k in lay.live_names():
        if k in zero:
            got = float(gv[k].double().pow(2).mean().sqrt())
            assert got < line, f"{k}: rms {got:.3e} where the oracle has rounding noise (< {line:.3e})"
        else:                                 # close_norm without its absolute "numerically zero" branch
            err = norm_err(gv[k], grads[k])
            assert err < GRAD_TOL, f"{k}: relative error {err:.3e} (oracle rms {rms[k]:.3e})"
    pv = lay.views(flat.cpu())
    for k in ("frame_dim_reshape_0.weight", "cross_att_fra2utt_2.input_proj.weight", "cross_attention_mlp.0.weight"):
        close((pv[k] - P[k]) * 1e4, (Pd[k] - P[k]) * 1e4, 2e-2, k)


# ---- (c) the path under test ran -----------------------------------------------------------------------------------------------
def _forward_launches(E, B, Tn):
    from oracle import sdumc_oracle as O
    flat, _ = flat_from(E, O.init_params(DIMS, seed=11), DIMS)
    audio, text, video, feat4, _ = [t.cuda() for t in O.synthetic_batch(B, Tn, DIMS, seed=5)]
    call = E.NetCall(flat, audio, [text, feat4], video, False, None)
    call.forward()                            # (first call: lazy set-up outside the count)
    return gemm_launches(call.forward)


def test_per_layer_path_launches_the_utterance_gemms(E):
    """chain.hip runs the utterance-level layers inside its own kernels; the per-layer path launches them as sdumc_gemm_f32.  If
    plan_utterance()'s threshold moves, B = 257 stops testing the per-layer path and this assertion says so."""
    n256, n257 = _forward_launches(E, 256, TN), _forward_launches(E, 257, TN)
    print(f"\nsdumc_gemm_f32 launches per forward: B=256 {n256}, B=257 {n257}")
    assert n257 > n256


# ---- (d) the forced switch at the smallest shapes ------------------------------------------------------------------------------
def _forced_child():
    """Runs in a fresh process (SDUMC_CHAIN is read once per process): the three smallest shapes against the oracle, one JSON line."""
    from sdumc_amd import engine
    rep = {"SDUMC_CHAIN": os.environ.get("SDUMC_CHAIN"), "shapes": {}, "failures": []}
    for B, Tn, zero_video in FORCED_SHAPES:
        entry = {"out": 0.0, "grad": 0.0, "grad_tensor": ""}
        for mode in ("eval", "train"):
            res = net_case(engine, B, Tn, 2, mode, zero_video=zero_video, pseed=21, bseed=6, seed=7, call0=2)
            if not res["grad"] <= entry["grad"]:
                entry["grad"], entry["grad_tensor"] = res["grad"], f"{res['grad_tensor']} ({mode})"
            if not res["out"] <= entry["out"]:
                entry["out"] = res["out"]
            try:
                hold(res, f"B={B} T={Tn} {mode}")
            except AssertionError as e:
                rep["failures"].append(str(e)[:400])
        rep["shapes"][f"B={B} T={Tn}"] = entry
    B, Tn, _ = FORCED_SHAPES[-1]
    rep["gemm_launches"] = _forward_launches(engine, B, Tn)
    print(json.dumps(rep))
    sys.stdout.flush()
    sys.exit(1 if rep["failures"] else 0)


def test_forced_per_layer_path_at_the_smallest_shapes(E):
    """SDUMC_CHAIN=0 puts V = 2, 6 and 10 -- shapes the clustered kernels own otherwise -- on the per-layer path: one wave of the
    one-wave-per-sample kernels' only workgroup does work at V = 2, a single text frame, T on both sides of the 64-row pooling
    chunk, a fully zero video utterance."""
    env = dict(os.environ, SDUMC_CHAIN="0")
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_perlayer import _forced_child; _forced_child()"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, f"no report from the child (exit {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    rep = json.loads(lines[-1])
    print("\nSDUMC_CHAIN=0: " + lines[-1])
    assert r.returncode == 0 and not rep["failures"], rep["failures"]
    assert rep["SDUMC_CHAIN"] == "0" and len(rep["shapes"]) == len(FORCED_SHAPES)
    for name, e in rep["shapes"].items():
        assert e["out"] <= OUT_TOL and e["grad"] < GRAD_TOL, (name, e)
    B, Tn, _ = FORCED_SHAPES[-1]
    here = _forward_launches(E, B, Tn)
    print(f"sdumc_gemm_f32 launches per forward at B={B}: {here} in this process, {rep['gemm_launches']} under SDUMC_CHAIN=0")
    assert rep["gemm_launches"] > here, "SDUMC_CHAIN=0 did not take effect in the child"
