"""GPU parity at the batch sizes BASELINE.json STATES, against the CPU oracle (it takes 5-10 s per step at these sizes):
  configs[1]  C2  MOSEI shapes, B = 64, fp32        one full train step vs oracle.train_step (Philox masks)
  configs[2]  C3  the same in bf16 storage           vs the fp32 oracle (activation bar 2e-2) AND vs an fp64 evaluation of the
                                                     same graph with the engine's bf16 rounding points (oracle/bf16_storage.py)
  configs[4]  C5  T = 512 x 3, d = 1024, per-GPU slice B = 32, fp32 and bf16 storage
B = 64 is where the production schedule differs from what the small-batch tests run: V = 128 -> the clustered utterance-level
kernels on 256 workgroups, the stream-K cuts of the grouped weight-gradient launches across 37 problems, the rows GEMM at
M = 48 000.  Reference: main_frame_val_text_missing.py:119-150 (the step), toolkit/models/wengnet_mosei_mult_views_text_missing.py
:275-370 (the network), toolkit/utils/loss.py:19-51, :271-315 (the losses)."""
import numpy as np
import pytest
import torch

from . import grad_parity as GP
from .test_gpu_configs import NAMES, close, flat_from, grad_errors

pytestmark = pytest.mark.gpu

C2 = ((1024, 4096, 1024, 4096), 64, (375, 32, 225, 32))
C5 = ((1024, 1024, 1024, 1024), 32, (512, 512, 512, 512))
# bf16 storage against the fp64 evaluation that rounds where the engine rounds: what is left is fp32 accumulation order, the
# hardware tanh / exp, and bf16 roundings that flip where the two sides differ in the last fp32 bits (a few thousand of the 24 M
# stored frame elements; they show in bias gradients that are sums with heavy cancellation).  Measured on MI355X: median over the
# gradient tensors 1.6e-5 (C5) / ~1e-5 (C3), worst tensor 2.0e-3 (C3: cross_fused_query_mlp.0.bias) and 4.8e-3 (C5:
# video_mlp.0.bias).  A kernel off by 5 % moves every tensor downstream of it to 5e-2.
BF16_EMU_GRAD_TOL = 1e-2          # every tensor
BF16_EMU_GRAD_P90 = 2e-3          # 90th percentile over the tensors
BF16_EMU_GRAD_MEDIAN = 5e-4
BF16_EMU_OUT_TOL = 2e-3
# C2 in bf16 storage: the formerly skipped tensors that the emulation's fp32-parameter evaluation moves by more than
# BF16_EMU_GRAD_TOL / 4 (profiles/grad_parity_by_tensor.txt: e_ref 0.004 for fra2utt_1.input_proj.bias, 0.015 .. 0.035 for the
# others; the next formerly skipped tensor, cross_att_fra2utt_0.input_proj.bias, has 1.8e-3 and is held to the flat bar)
C2_BF16_BETWEEN = ("audio_mlp.0.weight", "audio_mlp.3.weight", "video_mlp.0.weight", "video_mlp.3.weight",
                   "fra2utt_0.attention_context_vector", "fra2utt_0.input_proj.weight", "fra2utt_0.input_proj.bias",
                   "fra2utt_1.input_proj.bias",
                   "fra2utt_2.attention_context_vector", "fra2utt_2.input_proj.weight", "fra2utt_2.input_proj.bias")


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import engine
    return engine


# fp32 at full size: every live gradient tensor by its OWN norm (77 of C2's 83 gradient tensors have max |g| < 1e-3 -- frame weights
# ~1e-5, the smallest 3.5e-10 -- so an absolute tolerance tied to max(1, |g|) passes an all-zero gradient; that was this test until
# round 6).  Measured on MI355X (profiles/r6_fullsize_grad_errors.txt): C2 median 1.0e-6, 90th percentile 1.3e-6, worst 2.5e-5
# (planes) / 5.7e-5 (in-kernel split), both on the RnC head (orgin_linear_change.0: small gradients with heavy cancellation); C5
# median 1.2e-6, worst 4e-6.  A kernel that drops a term moves its tensors to >= 1e-2.
# WHICH tensors are compared is decided on the reference side alone (tests/grad_parity.py): the reference is the fp64 oracle, and a
# tensor is set aside only where the fp32 oracle disagrees with it by more than 10 % of the tensor's norm -- the RnC head's biases,
# zero by translation invariance -- 82 of 83 at C2, 81 of 83 at C5.  (Until this rule, every tensor whose per-element rms was below
# 1e-6 of the largest tensor's was set aside: 26 of C2's 83 and 30 of C5's, the whole backward of the audio and video attention
# sites among them.)  Measured over all of them (profiles/grad_parity_by_tensor.txt): median 1.0e-6, p90 1.4e-6, worst 6.0e-5, still on
# the RnC head; orgin_linear_change.2.weight is the one tensor the two oracles know no better than 5e-5 .. 6e-5 (in between).
FP32_GRAD_TOL = 2e-4


_ORACLE_CACHE = {}


def _oracle_step(cfg, pseed, bseed, seed):
    """(P, batch, Pd after Adam, loss, terms, grads, outs, grads of the fp64 evaluation): 5-10 s of CPU for the fp32 step and about as
    much for the fp64 one at these sizes, shared by the two product paths"""
    from oracle import sdumc_oracle as O
    key = (cfg, pseed, bseed, seed)
    if key not in _ORACLE_CACHE:
        dims, B, Tn = cfg
        P = O.init_params(dims, seed=pseed)
        batch = O.synthetic_batch(B, Tn, dims, seed=bseed)
        Pd = {k: v.clone() for k, v in P.items()}
        _ORACLE_CACHE[key] = (P, batch, Pd) + tuple(O.train_step(Pd, {}, *batch, mode="philox", seed=seed, step=0)) + \
            (GP.oracle_step_grads(P, batch, seed),)
    return _ORACLE_CACHE[key]


def _step_fp32_vs_oracle(E, cfg, pseed, bseed, seed, delta_names, planes):
    """planes=False: the step a set_batch-per-step loop runs (in-kernel operand split, csrc/gemm_wide.hip); planes=True: the step over
    RESIDENT batches -- bench.py's headline and FusedTrainer.run_epoch -- whose frame / key projections read bf16 planes (csrc/gemm_p3.hip)."""
    dims, B, Tn = cfg
    P, batch, Pd, loss, terms, grads, outs, grads64 = _oracle_step(cfg, pseed, bseed, seed)
    flat, lay = flat_from(E, P, dims)
    ts = E.TrainStep(flat, B, Tn, dims, seed=seed, planes=planes)
    assert (ts._planes is not None) == planes
    ts.set_batch(*[t.cuda() for t in batch])
    losses = ts.run().cpu().numpy()
    np.testing.assert_allclose(losses[0], float(loss), rtol=1e-3)              # north-star tolerance: 1e-3
    np.testing.assert_allclose(losses[1:7], [float(t) for t in terms], rtol=1e-3, atol=1e-5)
    for s in range(2):
        for n, got, want in zip(NAMES, (ts.vals, ts.fused, ts.rnc, ts.text_hidden, ts.cross_text), outs[s]):
            close(got[s * B:(s + 1) * B], want, 1e-3, f"{n} stream {s}")
    gv = lay.views(torch.cat([ts.grads.cpu(), torch.zeros(lay.total - lay.live)]))
    assert set(grads) == set(lay.live_names())
    for k in lay.live_names():
        close(gv[k], grads[k], 1e-3, k)           # (the north-star's absolute bar; says little about tensors far below 1e-3 ...)
    # (... so: every tensor relative to its own norm, against the fp64 oracle; the fp32 oracle says how well each can be known)
    errs = GP.tensor_errors(lay, gv, grads64, grads, FP32_GRAD_TOL, what="fp32 %s B = %d, planes=%s" % ("C2" if cfg is C2 else "C5", B, planes))
    assert len(errs) == (82 if cfg is C2 else 81), errs.line
    # (what this test held until now, against the fp32 oracle; the set is now taken from the fp64 gradients' rms where it was taken
    # from the fp32 oracle's: the same tensors unless one sits exactly on 1e-6 G)
    for k in errs.old_compared:
        e = float((gv[k].double() - grads[k].double()).norm()) / float(grads[k].double().norm())
        assert e < FP32_GRAD_TOL, f"{k}: relative gradient error {e:.3e} (|g| = {float(grads[k].norm()):.3e})"
    pv = lay.views(flat.cpu())
    for k in delta_names:          # post-Adam deltas (first step: lr * g / (|g| + eps))
        close((pv[k] - P[k]) * 1e4, (Pd[k] - P[k]) * 1e4, 2e-2, k)


@pytest.mark.parametrize("planes", [True, False])
def test_c2_fp32_step_at_batch_64_vs_oracle(E, planes):
    """BASELINE configs[1] at its stated batch: loss + six terms, five outputs of both streams, EVERY live gradient tensor (relative to
    its own norm) and the post-Adam deltas of three tensors against oracle.train_step(mode="philox"), on both product paths."""
    _step_fp32_vs_oracle(E, C2, 0, 1234, 777,
                         ("frame_dim_reshape_1.weight", "cross_att_fra2utt_0.input_proj.weight", "fc_out_v.weight"), planes)


@pytest.mark.parametrize("planes", [True, False])
def test_c5_fp32_step_at_per_gpu_batch_32_vs_oracle(E, planes):
    """BASELINE configs[4]'s per-GPU slice (B = 32, T = 512 for every modality, d = 1024) in fp32 against the oracle."""
    _step_fp32_vs_oracle(E, C5, 4, 21, 11,
                         ("frame_dim_reshape_0.weight", "cross_att_fra2utt_2.input_proj.weight", "cross_attention_mlp.0.weight"), planes)


def _step_bf16_vs_oracles(E, cfg, pseed, bseed, seed):
    from oracle import sdumc_oracle as O
    from oracle.bf16_storage import Bf16Storage
    dims, B, Tn = cfg
    P = O.init_params(dims, seed=pseed)
    flat, lay = flat_from(E, P, dims)
    batch = O.synthetic_batch(B, Tn, dims, seed=bseed)
    ts = E.TrainStep(flat, B, Tn, dims, seed=seed, bf16=True)
    ts.set_batch(*[t.cuda() for t in batch])
    losses = ts.run().cpu().numpy()
    got_outs = [t.cpu().clone() for t in (ts.vals, ts.fused, ts.rnc, ts.text_hidden, ts.cross_text)]
    gv = lay.views(torch.cat([ts.grads.cpu(), torch.zeros(lay.total - lay.live)]))
    # (a) the fp32 oracle: the activation bar of the bf16 configs (2e-2)
    loss, terms, grads32, outs = O.train_step({k: v.clone() for k, v in P.items()}, {}, *batch, mode="philox", seed=seed, step=0)
    np.testing.assert_allclose(losses[0], float(loss), rtol=2e-2)
    np.testing.assert_allclose(losses[1:7], [float(t) for t in terms], rtol=2e-2, atol=1e-4)
    for s in range(2):
        for n, got, want in zip(NAMES, got_outs, outs[s]):
            close(got[s * B:(s + 1) * B], want, 2e-2, f"bf16 vs fp32 oracle: {n} stream {s}")
    # (b) fp64 evaluation of the same graph on bf16-rounded stored tensors: rounding is reproduced, errors are not
    P64 = {k: v.double() for k, v in P.items()}
    loss64, terms64, grads64, outs64 = O.train_step(P64, {}, *[t.double() for t in batch], mode="philox", seed=seed, step=0,
                                                    st=Bf16Storage())
    np.testing.assert_allclose(losses[0], float(loss64), rtol=BF16_EMU_OUT_TOL)
    np.testing.assert_allclose(losses[1:7], [float(t) for t in terms64], rtol=BF16_EMU_OUT_TOL, atol=1e-5)
    for s in range(2):
        for n, got, want in zip(NAMES, got_outs, outs64[s]):
            close(got[s * B:(s + 1) * B], want, BF16_EMU_OUT_TOL, f"bf16 vs rounding emulation: {n} stream {s}")
    # every tensor at BF16_EMU_GRAD_TOL; where the emulation's OWN fp32-parameter evaluation moves a tensor by more than a quarter of
    # that the bar follows it (grad_parity's in-between rule), for the tensors this test did not compare before.  At C5 there is
    # none and the helper's cap of 2 holds.  At C2 the cap cannot hold: bf16 roundings that flip between the emulation's fp64 and
    # fp32 evaluation move the audio and video branch up to the pooling by e_ref 4e-3 .. 3.5e-2, so the class is pinned to
    # C2_BF16_BETWEEN by name instead; a twelfth tensor in it fails the test.  The device does not need the raise: measured, all 82
    # tensors of C2 within 3.3e-3 (worst frame_dim_reshape_2.weight), all 81 of C5 within 5.9e-3 (fra2utt_2.input_proj.bias).
    lo = GP.oracle_step_grads(P, batch, seed, dtype=torch.float32, st=Bf16Storage())
    errs = GP.tensor_errors(lay, gv, grads64, lo, BF16_EMU_GRAD_TOL, between=C2_BF16_BETWEEN if cfg is C2 else (),
                            what="bf16 storage %s B = %d vs fp64 rounding emulation" % ("C2" if cfg is C2 else "C5", B))
    vals = sorted(errs[k] for k in errs.old_compared)      # (median and p90 over the tensors this test has always compared)
    print("bf16 storage vs fp32 oracle: worst %.3g" % max(grad_errors(lay, gv, grads32).values()))
    assert vals[int(0.9 * len(vals))] < BF16_EMU_GRAD_P90 and float(np.median(vals)) < BF16_EMU_GRAD_MEDIAN, \
        (float(np.median(vals)), vals[int(0.9 * len(vals))])


def test_c3_bf16_step_at_batch_64_vs_oracles(E):
    """BASELINE configs[2] at its stated batch and arithmetic (MOSEI shapes, B = 64, text-missing stream + self-distillation, bf16
    storage): against the fp32 oracle at the bf16 activation bar, and EVERY gradient tensor against the fp64 rounding emulation."""
    _step_bf16_vs_oracles(E, C2, 0, 1234, 777)


def test_c5_bf16_step_at_per_gpu_batch_32_vs_oracles(E):
    """BASELINE configs[4]'s per-GPU slice in its stated bf16 arithmetic."""
    _step_bf16_vs_oracles(E, C5, 4, 21, 11)
