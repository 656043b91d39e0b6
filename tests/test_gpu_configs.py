"""GPU parity tests at the shapes BASELINE.json's `configs` name, beyond the C2 cases of
test_gpu_net.py:
  configs[0]  C1  CMU-MOSI-shaped, B = 16, T = (200, 16, 120, 16): one full step against the oracle
  configs[3]  C4  CMU-MOSEI-shaped, global batch 512: on ONE GPU (the truth the data-parallel run must reproduce:
                  main_frame_val_text_missing.py:119-150 on the whole batch) + two simulated ranks of 256
  configs[4]  C5  long sequences T = 512, d = 1024 in its stated bf16 arithmetic against the fp32 oracle (2e-2)
plus the run-state plumbing of the data-parallel trainer (changing batch shapes, resume)."""
import numpy as np
import pytest
import torch

from tests import grad_parity as GP

pytestmark = pytest.mark.gpu

NAMES = ("vals", "fused", "rnc", "text_hidden", "cross_text")


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import engine
    return engine


def close(got, want, tol=1e-4, msg=""):
    got = got.detach().cpu().double().numpy()
    want = want.detach().cpu().double().numpy() if isinstance(want, torch.Tensor) else np.asarray(want, dtype=np.float64)
    scale = max(1.0, np.abs(want).max())
    np.testing.assert_allclose(got, want.reshape(got.shape), rtol=tol, atol=tol * scale, err_msg=msg)


def flat_from(E, P, dims):
    lay = E.ParamLayout.get(*dims[:3])
    flat = torch.zeros(lay.total)
    for k, v in lay.views(flat).items():
        v.copy_(P[k])
    return flat.cuda(), lay


# Tensor-wise relative error: gradients of this path are 1e-5 and smaller, an absolute tolerance tied to 1.0 says nothing about them.
# The absolute bar below a reference norm of 1e-7 holds for the RnC head's biases alone (analytically zero: the loss is translation
# invariant) -- by name: C2's frame biases have norms of 1.4e-7 and belong with the compared tensors whatever the batch makes of them.
close_norm = GP.close_norm


def test_c1_mosi_shapes_full_step_vs_oracle(E):
    """BASELINE configs[0] (C1): B = 16, T = (200, 16, 120, 16), full feature widths, train mode with Philox masks:
    loss, the six terms, the five outputs of both streams, every gradient and the Adam update against the oracle."""
    from oracle import sdumc_oracle as O
    dims = (1024, 4096, 1024, 4096)
    B, Tn = 16, (200, 16, 120, 16)
    P = O.init_params(dims, seed=0)
    flat, lay = flat_from(E, P, dims)
    audio, text, video, feat4, vals = O.synthetic_batch(B, Tn, dims, seed=1234)
    ts = E.TrainStep(flat, B, Tn, dims, seed=31)
    ts.set_batch(audio.cuda(), text.cuda(), video.cuda(), feat4.cuda(), vals.cuda())
    losses = ts.run().cpu().numpy()
    Pd = {k: v.clone() for k, v in P.items()}
    loss, terms, grads, outs = O.train_step(Pd, {}, audio, text, video, feat4, vals, mode="philox", seed=31, step=0)
    np.testing.assert_allclose(losses[0], float(loss), rtol=1e-3)
    np.testing.assert_allclose(losses[1:7], [float(t) for t in terms], rtol=1e-3, atol=1e-5)
    for s in range(2):
        for n, got, want in zip(NAMES, (ts.vals, ts.fused, ts.rnc, ts.text_hidden, ts.cross_text), outs[s]):
            close(got[s * B:(s + 1) * B], want, 1e-3, f"{n} stream {s}")
    gv = lay.views(torch.cat([ts.grads.cpu(), torch.zeros(lay.total - lay.live)]))
    for k in lay.live_names():
        close(gv[k], grads[k], 1e-3, k)
        close_norm(gv[k], grads[k], 2e-4, k)
    pv = lay.views(flat.cpu())
    for k in ("frame_dim_reshape_0.weight", "cross_att_fra2utt_2.input_proj.weight", "cross_attention_mlp.0.weight"):
        close((pv[k] - P[k]) * 1e4, (Pd[k] - P[k]) * 1e4, 2e-2, k)


@pytest.mark.parametrize("Tn", [(70, 64, 65, 96), (100, 40, 64, 40), (63, 32, 130, 32)])
def test_dx_in_one_pass_over_mixed_run_shapes_vs_oracle(E, Tn):
    """The rows launches that write dx directly (pooling term + mask-sum folded in) are chosen per modality: text streams
    of different lengths (two runs, one launch), a text slot too short for the fold beside audio / video that take it, the 63- and
    32-frame edges.  Every gradient against the oracle."""
    from oracle import sdumc_oracle as O
    dims = (1024, 4096, 1024, 4096)
    B = 6
    P = O.init_params(dims, seed=3)
    flat, lay = flat_from(E, P, dims)
    audio, text, video, feat4, vals = O.synthetic_batch(B, Tn, dims, seed=77)
    ts = E.TrainStep(flat, B, Tn, dims, seed=5)
    ts.set_batch(audio.cuda(), text.cuda(), video.cuda(), feat4.cuda(), vals.cuda())
    losses = ts.run().cpu().numpy()
    Pd = {k: v.clone() for k, v in P.items()}
    loss, terms, grads, outs = O.train_step(Pd, {}, audio, text, video, feat4, vals, mode="philox", seed=5, step=0)
    np.testing.assert_allclose(losses[0], float(loss), rtol=1e-3)
    gv = lay.views(torch.cat([ts.grads.cpu(), torch.zeros(lay.total - lay.live)]))
    for k in lay.live_names():
        close(gv[k], grads[k], 1e-3, k)
        close_norm(gv[k], grads[k], 2e-4, k)


def test_c4_global_batch_512_on_one_gpu_and_two_simulated_ranks(E):
    """BASELINE configs[3] (C4) at its size: the global batch of 512 MOSEI-shaped samples as ONE process on one GPU (what
    the 8-GPU data-parallel run has to equal), size-independent properties, and two simulated ranks of 256 whose summed
    gradients, exchanged losses and Adam update reproduce it."""
    from oracle import sdumc_oracle as O
    from sdumc_amd.trainer import HipBackend
    dims = (1024, 4096, 1024, 4096)
    B, Tn, W, seed = 512, (375, 32, 225, 32), 2, 5
    P = O.init_params(dims, seed=0)
    flat, lay = flat_from(E, P, dims)
    g = torch.Generator(device="cuda").manual_seed(7)
    audio, text, video, feat4 = [torch.randn(B, Tn[i], dims[i], device="cuda", generator=g) for i in range(4)]
    vals = torch.rand(B, device="cuda", generator=g) * 6 - 3
    # eval: the batch equals its two halves (samples are independent)
    full = [t.clone() for t in E.NetCall(flat, audio, [text, feat4], video, False, None).forward()]
    h = B // W
    for lo in (0, h):
        part = E.NetCall(flat, audio[lo:lo + h].contiguous(), [text[lo:lo + h].contiguous(), feat4[lo:lo + h].contiguous()],
                         video[lo:lo + h].contiguous(), False, None).forward()
        for n, f, p in zip(NAMES, full, part):
            for s in range(2):
                close(p[s * h:(s + 1) * h], f[s * B + lo:s * B + lo + h], 1e-5, n)
    del full, part
    # the single-process step on all 512 samples (RnC over n = 1024 rows: the sorted formulation)
    p_full = flat.clone()
    ts = E.TrainStep(p_full, B, Tn, dims, seed=seed)
    ts.set_batch(audio, text, video, feat4, vals)
    ref_losses = ts.run().cpu().clone()
    ref_grads = ts.grads.clone()
    assert torch.isfinite(ref_losses).all() and torch.isfinite(ref_grads).all()
    del ts
    # two ranks of 256 (collectives spelt out), B_global = 512
    bes = []
    for r in range(W):
        be = HipBackend(flat.clone(), h, Tn, dims, E.DEFAULT_WEIGHTS, 1e-4, (0.9, 0.999), 1e-8, 1e-5, seed, r * h, B)
        be.set_batch(*[t[r * h:(r + 1) * h].contiguous() for t in (audio, text, video, feat4, vals)])
        bes.append(be)
    rncs = [be.forward().clone() for be in bes]
    ssd = sum(be.local_ssd().clone() for be in bes)
    feats = torch.cat([p[:h] for p in rncs] + [p[h:] for p in rncs]).contiguous()
    lab = torch.cat([be.labels for be in bes])
    labels2 = torch.cat([lab, lab]).contiguous()
    ls = [be.loss_backward(ssd, feats, labels2, (r * h, W * h + r * h)).cpu().clone() for r, be in enumerate(bes)]
    gsum = sum(be.backward().clone() for be in bes)
    np.testing.assert_allclose((ls[0][1:3] + ls[1][1:3]).numpy(), ref_losses[1:3].numpy(), rtol=1e-4)
    for l in ls:
        np.testing.assert_allclose(l[3:7].numpy(), ref_losses[3:7].numpy(), rtol=1e-4)
    gv, rv = gsum.cpu(), ref_grads.cpu()
    worst, skipped = (0.0, ""), []
    span = {k: (lay.entries[k][0], int(np.prod(lay.entries[k][1]))) for k in lay.live_names()}
    G = max(float(rv[o:o + n].double().norm()) / np.sqrt(n) for o, n in span.values())      # the largest per-element rms of a tensor
    for k, (off, n) in span.items():
        close(gv[off:off + n], rv[off:off + n], 1e-3, k)
        # ... and relative to the tensor's own norm (most gradient tensors are far below the absolute bar: it would pass zeros).  The two
        # sides differ by summation order only (two K ranges of 256 rows against one of 512): measured <= 1e-5
        ref = float(rv[off:off + n].double().norm())
        err = float((gv[off:off + n].double() - rv[off:off + n].double()).norm())
        if k in GP.NO_SIGNAL and ref / np.sqrt(n) < 1e-6 * G:
            # the RnC head's biases, and no other tensor: zero by translation invariance -- rounding noise on both sides.  (There is
            # no oracle at this size; until the rule went by name, every tensor under 1e-6 G was let through here.)
            assert err / np.sqrt(n) < 1e-5 * G, (k, err, G)
            skipped.append(k)
        else:
            assert err / ref < 2e-4, f"{k}: DP(2 x 256) vs single(512) relative gradient error {err / ref:.3e} (|g| = {ref:.3e})"
            worst = max(worst, (err / ref, k))
    print("grad parity C4 DP(2 x 256) vs single process: %d of %d tensors compared, %d no-signal; worst %s = %.3g" %
          (len(span) - len(skipped), len(span), len(skipped), worst[1], worst[0]))
    for be in bes:
        be.grads.copy_(gsum)
        be.adam(1.0)
    torch.cuda.synchronize()
    assert torch.equal(bes[0].params, bes[1].params)
    # the first Adam step is lr * g / (|g| + eps): ill-conditioned where g is rounding noise (|g| ~ eps = 1e-8)
    ok = torch.zeros(lay.total, dtype=torch.bool)
    ok[:lay.live] = rv.abs() > 1e-5
    np.testing.assert_allclose(((bes[0].params - flat) * 1e4).cpu().numpy()[ok.numpy()],
                               ((p_full - flat) * 1e4).cpu().numpy()[ok.numpy()], rtol=5e-2, atol=5e-2)


# bf16 storage against the fp32 step / fp32 oracle: this only bounds the size of the ROUNDING (bf16 carries 8 mantissa bits and the
# step rounds x, keys, dz, dxd, dx: a few per cent on most tensors, up to 0.11 on small biases).  It is not the error check: that
# is tests/test_gpu_fullsize.py, every gradient tensor against an fp64 evaluation that rounds where the engine rounds (4e-3).
C5_BF16_GRAD_MAX = 0.2


def grad_errors(lay, got, ref):
    """norm-wise relative error of every live gradient tensor but orgin_linear_change.{0,2}.bias -- BY NAME (tests/grad_parity.py):
    zero by the translation invariance of RnC, where their per-element rms is below 1e-6 of the largest tensor's they carry no
    signal for a relative error and must be just as small on the device.  (By size alone that rule skipped a third of the tensors.)"""
    rms = {k: float(ref[k].double().norm() / np.sqrt(ref[k].numel())) for k in lay.live_names()}
    G = max(rms.values())
    errs = {}
    for k in lay.live_names():
        d = float((got[k].double() - ref[k].double()).norm())
        if k in GP.NO_SIGNAL and rms[k] < 1e-6 * G:
            assert d / np.sqrt(ref[k].numel()) < 1e-5 * G, (k, d, G)
            continue
        errs[k] = d / float(ref[k].double().norm())
    return errs


def _bf16_full_batch_properties(E, dims, B, Tn, seed):
    """bf16-storage step at a BASELINE batch size: size-independent properties -- the eval-mode forward of the batch equals that
    of its two halves, two runs are bit-identical, every live gradient tensor is finite and non-zero, and the loss terms agree
    with the fp32 step on the same inputs and masks at the bf16 bar (2e-2).  (The comparison with the CPU oracle at these sizes,
    every gradient tensor against an fp64 evaluation with the engine's bf16 rounding points: tests/test_gpu_fullsize.py.)"""
    from oracle import sdumc_oracle as O
    P = O.init_params(dims, seed=0)
    flat, lay = flat_from(E, P, dims)
    g = torch.Generator(device="cuda").manual_seed(seed)
    audio, text, video, feat4 = [torch.randn(B, Tn[i], dims[i], device="cuda", generator=g) for i in range(4)]
    vals = torch.rand(B, device="cuda", generator=g) * 6 - 3
    full = [t.clone() for t in E.NetCall(flat, audio, [text, feat4], video, False, None, bf16=True).forward()]
    h = B // 2
    for lo in (0, h):
        part = E.NetCall(flat, audio[lo:lo + h].contiguous(), [text[lo:lo + h].contiguous(), feat4[lo:lo + h].contiguous()],
                         video[lo:lo + h].contiguous(), False, None, bf16=True).forward()
        for n, f, p in zip(NAMES, full, part):
            for s in range(2):
                close(p[s * h:(s + 1) * h], f[s * B + lo:s * B + lo + h], 1e-5, "bf16 halves " + n)
    del full, part
    runs = []
    for mode in (True, True, False):
        p = flat.clone()
        ts = E.TrainStep(p, B, Tn, dims, seed=seed, bf16=mode)
        ts.set_batch(audio, text, video, feat4, vals)
        losses = ts.run().cpu().clone()
        runs.append((losses, ts.grads.cpu().clone(), p.cpu().clone()))
        del ts
    # two runs of the same step: bit for bit (round 4: the run-to-run differences of this mode were wrong low halves of packed FP32
    # results in the utterance-level kernels when a bf16 MFMA workgroup shared their CU -- those kernels now run without packed
    # FP32 instructions in the bf16 modes: csrc/chain_common.h)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    assert torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all()
    np.testing.assert_allclose(runs[0][0].numpy()[:7], runs[2][0].numpy()[:7], rtol=2e-2, atol=1e-4)
    assert not torch.equal(runs[0][1], runs[2][1]), "bf16 mode is not active"
    gb, gf = lay.views(torch.cat([runs[0][1], torch.zeros(lay.total - lay.live)])), lay.views(torch.cat([runs[2][1], torch.zeros(lay.total - lay.live)]))
    errs = grad_errors(lay, gb, gf)
    worst = max(errs, key=errs.get)
    print("grad parity bf16 storage vs fp32 storage, B = %d, T = %s: %d of %d tensors compared; worst %s = %.3g" %
          (B, Tn, len(errs), len(lay.live_names()), worst, errs[worst]))
    for k, err in errs.items():
        assert float(gb[k].abs().max()) > 0.0, k
        assert err < C5_BF16_GRAD_MAX, (k, err)


def test_c3_bf16_step_at_batch_64_properties(E):
    """BASELINE configs[2] (C3) at its stated batch: MOSEI shapes, B = 64, bf16 storage"""
    _bf16_full_batch_properties(E, (1024, 4096, 1024, 4096), 64, (375, 32, 225, 32), 31)


def test_c5_bf16_step_at_batch_32_properties(E):
    """BASELINE configs[4] (C5) at its per-GPU batch: T = 512 for every modality, d = 1024, B = 32, bf16 storage"""
    _bf16_full_batch_properties(E, (1024, 1024, 1024, 1024), 32, (512, 512, 512, 512), 37)


def test_c5_long_sequence_shapes_in_bf16_vs_fp32_oracle(E):
    """BASELINE configs[4] (C5) in its stated arithmetic: T = 512 for every modality, d = 1024, bf16 mode, one full
    train step against the fp32 oracle at the bf16 bar of SURVEY §8(d) (2e-2), gradients norm-wise."""
    from oracle import sdumc_oracle as O
    dims = (1024, 1024, 1024, 1024)
    B, Tn = 4, (512, 512, 512, 512)
    P = O.init_params(dims, seed=4)
    flat, lay = flat_from(E, P, dims)
    batch = O.synthetic_batch(B, Tn, dims, seed=21)
    dev = [t.cuda() for t in batch]
    f32 = [t.clone() for t in E.NetCall(flat, dev[0], [dev[1], dev[3]], dev[2], False, None).forward()]
    b16 = [t.clone() for t in E.NetCall(flat, dev[0], [dev[1], dev[3]], dev[2], False, None, bf16=True).forward()]
    for n, a, b in zip(NAMES, f32, b16):
        close(b, a, 2e-2, "bf16 " + n)
    assert max(float((a - b).abs().max()) for a, b in zip(f32, b16)) > 1e-6, "bf16 mode is not active"
    ts = E.TrainStep(flat, B, Tn, dims, seed=11, bf16=True)
    ts.set_batch(*dev)
    losses = ts.run().cpu().numpy()
    loss, terms, grads, outs = O.train_step({k: v.clone() for k, v in P.items()}, {}, *batch, mode="philox", seed=11, step=0)
    np.testing.assert_allclose(losses[0], float(loss), rtol=2e-2)
    np.testing.assert_allclose(losses[1:7], [float(t) for t in terms], rtol=2e-2, atol=1e-4)
    gv = lay.views(torch.cat([ts.grads.cpu(), torch.zeros(lay.total - lay.live)]))
    # norm-wise per tensor; tensors whose gradient is (analytically or numerically) negligible next to the largest one --
    # orgin_linear_change.2.bias is exactly zero by the translation invariance of RnC -- carry no signal to compare
    errs = grad_errors(lay, gv, grads)
    vals = sorted(errs[k] for k in GP.old_rule_compared(list(lay.live_names()), grads))      # (median, p90: over the set they were set for)
    worst = max(errs, key=errs.get)
    print("grad parity C5 B = 4 bf16 storage vs fp32 oracle: %d of %d tensors compared; median %.3g, p90 %.3g (both over the %d of the former "
          "rule), worst %s = %.3g" % (len(errs), len(lay.live_names()), float(np.median(vals)), vals[int(0.9 * len(vals))], len(vals), worst, errs[worst]))
    # median 2 %; a few small tensors (a handful of biases whose gradient is a difference of large terms) sit higher; EVERY
    # tensor is bounded (C5_BF16_GRAD_MAX): a tensor of garbage would read >= 1
    assert float(np.median(vals)) < 4e-2 and vals[int(0.9 * len(vals))] < 0.2, (float(np.median(vals)), worst, errs[worst])
    assert errs[worst] < C5_BF16_GRAD_MAX, (worst, errs[worst])


def test_data_parallel_step_over_changing_shapes_and_resume(E):
    """trainer.DataParallelStep on real loader behaviour: batch shapes change from step to step (per-batch padding, short last
    batch) while ONE optimiser state / step count / dropout counter continues (compared with engine.FusedTrainer over the
    same batches), the key-padding lengths are forwarded, and a run resumed through load_optimizer_state equals the
    uninterrupted one bit for bit."""
    from oracle import sdumc_oracle as O
    from sdumc_amd.trainer import DataParallelStep
    dims = (24, 16, 20, 16)
    shapes = [(4, (9, 2, 5, 3)), (3, (7, 4, 6, 1)), (4, (9, 2, 5, 3)), (2, (12, 3, 2, 2))]
    P = O.init_params(dims, seed=8)
    batches = [[t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=100 + i)] for i, (B, Tn) in enumerate(shapes)]
    lens = [[torch.randint(1, T + 1, (B,)) for T in Tn] for (B, Tn) in shapes]

    def run(steps, with_lengths, resume_at=None):
        flat, lay = flat_from(E, P, dims)
        dp = DataParallelStep(flat, shapes[0][0], shapes[0][1], dims, lr=1e-3, seed=17)
        out = []
        for i in steps:
            if resume_at is not None and i == resume_at:
                m, v, t = dp.state.optimizer_state()
                m, v, params = m.clone(), v.clone(), flat.clone()
                flat2 = params                                   # a fresh process: new trainer, restored state
                dp = DataParallelStep(flat2, shapes[i][0], shapes[i][1], dims, lr=1e-3, seed=17)
                dp.load_optimizer_state(m, v, t)
                flat = flat2
            dp.set_batch(*batches[i], lengths=lens[i] if with_lengths else None)
            out.append(dp.step().clone())
        return flat, out, dp

    flat_dp, l_dp, dp = run(range(4), False)
    flat_ft, lay = flat_from(E, P, dims)
    ft = E.FusedTrainer(flat_ft, dims, lr=1e-3, seed=17)
    for i, b in enumerate(batches):
        l = ft.step(*b)
        np.testing.assert_allclose(l_dp[i].cpu().numpy()[1:7], l.cpu().numpy()[1:7], rtol=1e-5, atol=1e-7, err_msg=f"step {i}")
    np.testing.assert_allclose(flat_dp.cpu().numpy(), flat_ft.cpu().numpy(), rtol=0, atol=2e-6)
    assert dp.state.rng.call == 8 and int(dp.state.hyper[1].item()) == 4 and len(dp._bes) == 3
    # resume after two steps == uninterrupted
    flat_rs, l_rs, _ = run(range(4), False, resume_at=2)
    assert torch.equal(flat_rs, flat_dp)
    for a, b in zip(l_dp, l_rs):
        assert torch.equal(a, b)
    # lengths reach the kernels: same batches with the key-padding mask differ from the unmasked run and equal FusedTrainer's
    flat_m, l_m, _ = run(range(4), True)
    flat_f2, _ = flat_from(E, P, dims)
    ft2 = E.FusedTrainer(flat_f2, dims, lr=1e-3, seed=17)
    for i, b in enumerate(batches):
        l = ft2.step(*b, lengths=lens[i])
        np.testing.assert_allclose(l_m[i].cpu().numpy()[1:7], l.cpu().numpy()[1:7], rtol=1e-5, atol=1e-7)
    assert not torch.equal(l_m[0], l_dp[0])


def test_fused_trainer_resume_equals_uninterrupted_run(E):
    """save -> load -> continue through checkpoint.adam_state_from_flat / flat_from_adam_state and
    FusedTrainer.load_optimizer_state: Adam moments, bias-correction step count and dropout counter all continue."""
    from oracle import sdumc_oracle as O
    from sdumc_amd import checkpoint as ck
    dims = (24, 16, 20, 16)
    B, Tn = 4, (9, 2, 5, 3)
    P = O.init_params(dims, seed=9)
    batches = [[t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=200 + i)] for i in range(4)]
    flat_a, lay = flat_from(E, P, dims)
    tr = E.FusedTrainer(flat_a, dims, lr=1e-3, seed=3)
    la = [tr.step(*b).clone() for b in batches]
    flat_b, _ = flat_from(E, P, dims)
    tr1 = E.FusedTrainer(flat_b, dims, lr=1e-3, seed=3)
    lb = [tr1.step(*b).clone() for b in batches[:2]]
    m, v, t = tr1.optimizer_state()
    assert t == 2

    class _Net:        # what checkpoint.* needs of the module: the layout and the parameter order
        _layout = lay
        _pnames = lay.order
    opt = ck.adam_state_from_flat(_Net, m, v, t, lr=1e-3)
    m2, v2, t2 = ck.flat_from_adam_state(_Net, opt, "cuda")
    flat_c = flat_b.clone()
    tr2 = E.FusedTrainer(flat_c, dims, lr=1e-3, seed=3)
    tr2.load_optimizer_state(m2, v2, t2)
    lb += [tr2.step(*b).clone() for b in batches[2:]]
    for a, b in zip(la, lb):
        assert torch.equal(a, b)
    assert torch.equal(flat_a, flat_c)


def test_ragged_epoch_through_store_and_arena_equals_plain_batches(E):
    """F1 + the ragged-epoch path: batches assembled by DeviceFeatureStore.batch_into straight into the arena of a
    capacity-mode FusedTrainer (one workspace for every batch shape, gradient bucket at a fixed offset) reproduce, bit for
    bit, the same epoch run batch by batch through store.batch() + FusedTrainer.step with per-shape workspaces; the
    key-padding lengths produced by the gather kernel equal the host table."""
    from oracle import sdumc_oracle as O
    from sdumc_amd.data import DeviceFeatureStore
    dims = (24, 16, 20, 16)
    Tcap = (19, 6, 11, 5)
    P = O.init_params(dims, seed=8)
    store = DeviceFeatureStore.synthetic(40, Tcap, dims, seed=5)
    g = torch.Generator().manual_seed(1)
    batches = [torch.randperm(40, generator=g)[:B] for B in (6, 6, 4, 6, 3, 6)]
    assert len({store.batch_shape(ix) for ix in batches}) >= 4
    res = []
    for mode in ("arena", "plain", "arena_kp", "plain_kp"):
        flat, lay = flat_from(E, P, dims)
        kp = mode.endswith("_kp")
        tr = E.FusedTrainer(flat, dims, lr=1e-3, seed=11, capacity=(6, Tcap) if mode.startswith("arena") else None)
        ls = []
        for ix in batches:
            if mode.startswith("arena"):
                ls.append(tr.step_from_store(store, ix, key_padding=kp).clone())
            else:
                b, pads, emos, vals, names = store.batch(ix)
                lens = [torch.tensor([b[k].shape[1] - p for p in pad], dtype=torch.int32) for k, pad in zip(("audios", "texts", "videos", "feat4s"), pads)]
                ls.append(tr.step(b["audios"], b["texts"], b["videos"], b["feat4s"], vals, lengths=lens if kp else None).clone())
        res.append((flat.clone(), ls))
        if mode == "arena":
            assert len(tr._steps) == len({store.batch_shape(ix) for ix in batches})
    for a, b in ((0, 1), (2, 3)):
        for x, y in zip(res[a][1], res[b][1]):
            assert torch.equal(x, y)
        assert torch.equal(res[a][0], res[b][0])
    assert not torch.equal(res[0][1][0], res[2][1][0])       # the key-padding mask changes the result


def test_run_epoch_on_a_planes_store_equals_plain_resident_batches_bit_for_bit(E):
    """The production epoch path in fp32 storage -- DeviceFeatureStore(planes=True): every utterance split into bf16 planes ONCE;
    FusedTrainer.run_epoch: index vectors uploaded once, batch i + 1's ROW MAPS (in place, the default: the step reads the store's
    packed tensors through them, sdumc_net_io.row_map) or its padded copy (inplace=False: fp32 rows + plane rows gathered, one launch)
    written into the other input set by step i itself (sdumc_net_io.prefetch), the next keep-bits laid out for batch i + 1's shape
    (bits_next_dims) -- against
      * the same batches one at a time (step_from_store: gather in front of the step, no announced next shape), and
      * plain batches: store.batch() tensors installed with TrainStep.set_batch(planes=True), which SPLITS the padded batch (a padded
        row's planes are zero bytes, so gathering plane rows must equal splitting the gathered batch), keep-bits at the head of each step.
    Losses of every step and the final parameters bit for bit; with and without the key-padding lengths.
    Ref: toolkit/data/feat_data.py:232-253, toolkit/utils/read_data.py:223-248, main_frame_val_text_missing.py:89-109."""
    from oracle import sdumc_oracle as O
    from sdumc_amd.data import DeviceFeatureStore
    from sdumc_amd import _lib
    dims = (64, 128, 64, 128)
    Tcap = (70, 33, 66, 32)
    P = O.init_params(dims, seed=8)
    store = DeviceFeatureStore.synthetic(48, Tcap, dims, seed=5, planes=True)
    assert store.packed_p3 is not None and store.nbytes == sum(t.numel() * 4 for t in store.packed.values()) * 5 // 2
    g = torch.Generator().manual_seed(1)
    batches = [torch.randperm(48, generator=g)[:B] for B in (6, 6, 4, 6, 3, 6, 6)]
    assert len({store.batch_shape(ix) for ix in batches}) >= 4
    # the gathered planes ARE the split of the gathered batch
    B0, T0 = store.batch_shape(batches[0])
    outs = [torch.empty(B0, T0[i], dims[i], device="cuda") for i in range(4)]
    pls = [torch.empty(B0 * T0[i], 6 * dims[i], dtype=torch.uint8, device="cuda") for i in range(4)]
    lab = torch.empty(B0, device="cuda")
    store.batch_into(batches[0], outs, lab, planes_out=pls)
    bd, _, _, vals, _ = store.batch(batches[0])
    for i, k in enumerate(("audios", "texts", "videos", "feat4s")):
        assert torch.equal(outs[i], bd[k])
        assert torch.equal(pls[i], E.p3_split_into(outs[i], torch.empty_like(pls[i])))
    assert torch.equal(lab, vals)
    res = {}
    for mode in ("epoch", "epoch_gather", "one_by_one", "one_by_one_gather", "plain", "epoch_kp", "one_by_one_kp", "epoch_gather_kp"):
        flat, lay = flat_from(E, P, dims)
        kp = mode.endswith("_kp")
        inplace = "gather" not in mode      # in place: the step reads the store through row maps; gather: padded copies (rows + planes)
        ls = []
        if mode.startswith("epoch"):
            tr = E.FusedTrainer(flat, dims, lr=1e-3, seed=11, capacity=(6, Tcap), inplace=inplace)
            n = tr.run_epoch(store, batches, key_padding=kp, on_step=lambda i, l: ls.append(l.clone()))
            assert n == len(batches) and len(tr.arena.sets) == 2
            assert (tr.arena.sets[0].planes is None) == inplace and (tr.arena.sets[0].maps is not None) == inplace
        elif mode.startswith("one_by_one"):
            tr = E.FusedTrainer(flat, dims, lr=1e-3, seed=11, capacity=(6, Tcap), inplace=inplace)
            for ix in batches:
                ls.append(tr.step_from_store(store, ix, key_padding=kp).clone())
        else:
            state = E._RunState(flat, lay.live, 1e-3, 11)
            for ix in batches:
                b, pads, emos, vals, names = store.batch(ix)
                Bn, Tn = store.batch_shape(ix)
                ts = E.TrainStep(flat, Bn, Tn, dims, share=state, planes=True, bits_next=False)
                assert ts._planes is not None
                ts.set_batch(b["audios"], b["texts"], b["videos"], b["feat4s"], vals)
                ls.append(ts.run().clone())
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        res[mode] = (flat.clone(), ls)
    for a, b in (("epoch", "one_by_one"), ("epoch", "plain"), ("epoch", "epoch_gather"), ("epoch", "one_by_one_gather"),
                 ("epoch_kp", "one_by_one_kp"), ("epoch_kp", "epoch_gather_kp")):
        for i, (x, y) in enumerate(zip(res[a][1], res[b][1])):
            assert torch.equal(x, y), (a, b, i, x.tolist(), y.tolist())
        assert torch.equal(res[a][0], res[b][0]), (a, b)
    assert not torch.equal(res["epoch"][1][0], res["epoch_kp"][1][0])
    # a store without planes feeds the same trainer class through the in-kernel split (fp32 rows only): same epoch to rounding
    store2 = DeviceFeatureStore.synthetic(48, Tcap, dims, seed=5)
    flat, lay = flat_from(E, P, dims)
    tr = E.FusedTrainer(flat, dims, lr=1e-3, seed=11, capacity=(6, Tcap))
    ls = []
    tr.run_epoch(store2, batches, on_step=lambda i, l: ls.append(l.clone()))
    assert tr.arena.sets[0].planes is None
    for x, y in zip(ls, res["epoch"][1]):
        np.testing.assert_allclose(x.cpu().numpy()[:7], y.cpu().numpy()[:7], rtol=2e-5, atol=1e-6)
    with pytest.raises(_lib.SdumcError):
        store2.gather_desc(0, 1, (1, 1, 1, 1), [None] * 4, None, planes_out=[None] * 4)


def test_bf16_run_epoch_in_place_equals_gathered_batches_bit_for_bit(E):
    """bf16 storage (BASELINE configs[2] / [4]): a bf16 DeviceFeatureStore read IN PLACE through row maps (gemm_b1's A rows, the bf16
    grouped weight-gradient kernel's B rows; widths in whole 128-element tiles) against the same epoch on gathered padded copies
    (inplace=False) and against one batch at a time: losses of every step and the final parameters bit for bit; ragged shapes incl. a
    short last batch whose row count is not a multiple of four (the weight-gradient kernel fetches map entries four at a time)."""
    from oracle import sdumc_oracle as O
    from sdumc_amd.data import DeviceFeatureStore
    dims = (128, 256, 128, 256)
    Tcap = (70, 33, 66, 32)
    P = O.init_params(dims, seed=8)
    store = DeviceFeatureStore.synthetic(48, Tcap, dims, seed=5, bf16=True)
    g = torch.Generator().manual_seed(1)
    batches = [torch.randperm(48, generator=g)[:B] for B in (6, 6, 4, 6, 3, 6, 5)]
    res = {}
    for mode in ("epoch", "epoch_gather", "one_by_one", "epoch_kp", "epoch_gather_kp"):
        flat, lay = flat_from(E, P, dims)
        kp = mode.endswith("_kp")
        inplace = "gather" not in mode
        ls = []
        tr = E.FusedTrainer(flat, dims, lr=1e-3, seed=11, capacity=(6, Tcap), inplace=inplace, bf16=True)
        if mode.startswith("epoch"):
            tr.run_epoch(store, batches, key_padding=kp, on_step=lambda i, l: ls.append(l.clone()))
            assert (tr.arena.sets[0].maps is not None) == inplace
        else:
            for ix in batches:
                ls.append(tr.step_from_store(store, ix, key_padding=kp).clone())
        torch.cuda.synchronize()
        assert all(torch.isfinite(l).all() for l in ls)
        res[mode] = (flat.clone(), ls)
    for a, b in (("epoch", "epoch_gather"), ("epoch", "one_by_one"), ("epoch_kp", "epoch_gather_kp")):
        for i, (x, y) in enumerate(zip(res[a][1], res[b][1])):
            assert torch.equal(x, y), (a, b, i, x.tolist(), y.tolist())
        assert torch.equal(res[a][0], res[b][0]), (a, b)
    assert not torch.equal(res["epoch"][1][0], res["epoch_kp"][1][0])


def test_zero_copy_hand_over_equals_set_batch(E):
    """TrainStep.use_batch: the step reads the loader's device tensors where they are (what FusedTrainer.step does since round 6
    instead of a 224 MB copy per batch) -- losses, gradients and parameters bit for bit equal to set_batch; tensors that do not
    qualify (not contiguous, fp32 handed to a bf16-storage step) are copied; set_batch after a hand-over writes the step's own
    buffers again; a resident batch (planes=True) survives a hand-over in between.  Ref: main_frame_val_text_missing.py:94-109."""
    from oracle import sdumc_oracle as O
    from sdumc_amd import _lib
    dims, B, Tn = (64, 128, 64, 128), 5, (70, 32, 66, 33)
    P = O.init_params(dims, seed=2)
    b0 = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=60)]
    b1 = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=61)]

    def run(how, **kw):
        flat, lay = flat_from(E, P, dims)
        ts = E.TrainStep(flat, B, Tn, dims, seed=9, lr=1e-3, **kw)
        out = []
        for i, b in enumerate((b0, b1, b0)):
            if how == "set":
                ts.set_batch(*b)
            elif how == "use":
                assert ts.use_batch(*b) is True
            elif how == "mixed":      # hand-over, copy, hand-over
                (ts.set_batch if i == 1 else ts.use_batch)(*b)
            elif how == "strided":    # a non-contiguous view does not qualify: copied, same result
                wide = torch.cat([b[0], b[0]], dim=2)
                assert ts.use_batch(wide[:, :, :dims[0]], *b[1:]) is False
            out.append((ts.run().clone(), ts.grads.clone()))
            torch.cuda.synchronize()
        return out, flat.clone()

    want, wflat = run("set")
    for how in ("use", "mixed", "strided"):
        got, gflat = run(how)
        for (la, ga), (lb, gb) in zip(got, want):
            assert torch.equal(la, lb) and torch.equal(ga, gb), how
        assert torch.equal(gflat, wflat), how
    # a resident batch with planes: a hand-over of another batch in between, then set_batch of the first again
    flat, lay = flat_from(E, P, dims)
    ts = E.TrainStep(flat, B, Tn, dims, seed=9, lr=1e-3, planes=True)
    ts.set_batch(*b0)
    l0 = ts.run().clone()
    ts.use_batch(*b1)
    ts.run()
    ts.set_batch(*b0)
    assert ts._planes is not None and ts.io.audio_p3 == ts._planes[0].data_ptr()
    flat2, _ = flat_from(E, P, dims)
    ts2 = E.TrainStep(flat2, B, Tn, dims, seed=9, lr=1e-3, planes=True)
    ts2.set_batch(*b0)
    assert torch.equal(ts2.run(), l0)
    # bf16 storage: fp32 tensors are rounded by the copy, bf16 tensors are read in place
    flat, lay = flat_from(E, P, dims)
    th = E.TrainStep(flat, B, Tn, dims, seed=9, bf16=True)
    assert th.use_batch(*b0) is False
    la = th.run().clone()
    flat, lay = flat_from(E, P, dims)
    th = E.TrainStep(flat, B, Tn, dims, seed=9, bf16=True)
    assert th.use_batch(*[t.bfloat16() for t in b0[:4]], b0[4]) is True
    assert torch.equal(th.run(), la)


def test_trainer_step_keeps_at_most_one_batch_alive(E):
    """FusedTrainer.step() hands batches over zero-copy; the trainer holds the caller's tensors in ONE slot that the next step()
    replaces, and the cached per-shape steps keep none: over a ragged loader every earlier batch is freed once the following step has
    been enqueued (device memory does not grow with the number of shapes seen), with and without an arena.  A directly used
    TrainStep.use_batch keeps its batch until the next set_batch / use_batch: that contract stands."""
    import gc
    import weakref
    from oracle import sdumc_oracle as O
    dims, Tcap = (64, 128, 64, 128), (70, 33, 66, 33)
    P = O.init_params(dims, seed=2)
    shapes = [(6, Tcap), (4, (66, 31, 64, 32)), (3, (70, 32, 66, 33)), (5, (64, 33, 60, 30)), (6, Tcap)]
    assert len(set(shapes)) >= 4
    for cap in ((6, Tcap), None):
        flat, lay = flat_from(E, P, dims)
        tr = E.FusedTrainer(flat, dims, lr=1e-3, seed=9, capacity=cap)
        refs = []
        for i, (B, Tn) in enumerate(shapes):
            b = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=70 + i)]
            tr.step(*b)
            gc.collect()
            assert all(r() is None for r in refs), (cap, i, [r() is not None for r in refs])
            refs.append(weakref.ref(b[0]))
            del b
        torch.cuda.synchronize()
        gc.collect()
        assert all(r() is None for r in refs[:-1]), cap
        assert torch.isfinite(tr.state.losses).all()
    B, Tn = shapes[1]
    flat, lay = flat_from(E, P, dims)
    ts = E.TrainStep(flat, B, Tn, dims, seed=9)
    for install in (ts.use_batch, ts.set_batch):
        b = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=80)]
        r = weakref.ref(b[0])
        assert ts.use_batch(*b) is True
        del b
        ts.run()
        gc.collect()
        assert r() is not None
        install(*[t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=81)])
        gc.collect()
        assert r() is None, install.__name__
    torch.cuda.synchronize()


def test_launch_without_an_installed_batch_raises(E):
    """An arena step starts unbound, and FusedTrainer.step() leaves its per-shape step unbound: launch() raises SdumcError naming the
    four ways to install a batch instead of reading buffers nobody filled (or a batch the caller has freed)."""
    from oracle import sdumc_oracle as O
    from sdumc_amd import _lib
    dims, B, Tn = (64, 128, 64, 128), 4, (70, 32, 64, 33)
    P = O.init_params(dims, seed=2)
    b = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=60)]
    flat, lay = flat_from(E, P, dims)
    tr = E.FusedTrainer(flat, dims, lr=1e-3, seed=9, capacity=(B, Tn))
    tr.step(*b)
    with pytest.raises(_lib.SdumcError, match="set_batch, use_set, use_store or use_batch"):
        tr._get(B, Tn).launch()
    flat, lay = flat_from(E, P, dims)
    ts = E.TrainStep(flat, B, Tn, dims, seed=9, arena=E.StepArena(flat, B, Tn, dims))
    with pytest.raises(_lib.SdumcError, match="set_batch, use_set, use_store or use_batch"):
        ts.launch()
    assert ts._arena.sets[0]._inputs is None      # (nothing was touched)
    ts.set_batch(*b)                              # an unbound arena step: set 0 is its home
    ts.launch()
    torch.cuda.synchronize()
    assert torch.isfinite(ts.losses).all() and ts.io.audio == ts._arena.sets[0].inputs[0].data_ptr()


def _store_case(E, seed_ix=1, B=4):
    from oracle import sdumc_oracle as O
    from sdumc_amd.data import DeviceFeatureStore
    dims, Tcap = (64, 128, 64, 128), (70, 33, 66, 32)
    store = DeviceFeatureStore.synthetic(48, Tcap, dims, seed=5, planes=True)
    ix = torch.randperm(48, generator=torch.Generator().manual_seed(seed_ix))[:B]
    return O.init_params(dims, seed=8), dims, Tcap, store, ix


def test_set_lengths_after_use_lengths_writes_step_owned_buffers(E):
    """step(lengths=...) after step_from_store(key_padding=True) on the same shape: set_lengths copies into buffers the step owns,
    never into the arena set's capacity-sized length tensors that use_lengths pointed at (B = 4 < B_cap = 6: a shape error before; at
    B = B_cap a silent overwrite of state every cached step shares).  The arena's tensors are untouched, the mask is in force, and the
    two steps equal those of a trainer whose capacity is the batch itself, bit for bit."""
    P, dims, Tcap, store, ix = _store_case(E)
    b, pads, emos, vals, names = store.batch(ix)
    keys = ("audios", "texts", "videos", "feat4s")
    lens = [torch.tensor([b[k].shape[1] - p for p in pad], dtype=torch.int32) for k, pad in zip(keys, pads)]
    assert any(int(l.min()) < b[k].shape[1] for k, l in zip(keys, lens))

    def run(cap_B, masked):
        flat, lay = flat_from(E, P, dims)
        tr = E.FusedTrainer(flat, dims, lr=1e-3, seed=11, capacity=(cap_B, Tcap))
        l0 = tr.step_from_store(store, ix, key_padding=True).clone()
        before = [t.clone() for t in tr.arena.sets[0].lengths]
        l1 = tr.step(*[b[k] for k in keys], vals, lengths=lens if masked else None).clone()
        torch.cuda.synchronize()
        for x, y in zip(before, tr.arena.sets[0].lengths):
            assert torch.equal(x, y)
        return l0, l1, flat.clone()

    got, plain, want = run(6, True), run(6, False), run(4, True)
    assert torch.equal(got[0], plain[0]) and not torch.equal(got[1], plain[1])
    for x, y in zip(got, want):
        assert torch.equal(x, y)


def test_set_batch_after_use_store_trains_on_the_copied_batch(E):
    """set_batch on an arena step that reads a store in place binds the step's home (the padded views of the set use_store named)
    before it copies: the step trains on the batch it was given, not on the store's previous one through row maps left in place.
    Losses and final parameters bit for bit equal to the run that names the set itself (use_set) before the copy."""
    from oracle import sdumc_oracle as O
    P, dims, Tcap, store, ix = _store_case(E)
    B, Tn = store.batch_shape(ix)
    b1 = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=61)]

    def run(name_the_set):
        flat, lay = flat_from(E, P, dims)
        tr = E.FusedTrainer(flat, dims, lr=1e-3, seed=11, capacity=(6, Tcap))
        l0 = tr.step_from_store(store, ix).clone()
        ts = tr._get(B, Tn)
        assert ts.io.row_map[0] is not None      # (the step read the store in place)
        if name_the_set:
            ts.use_set(0)
        ts.set_batch(*b1)
        assert ts.io.row_map[0] is None and ts.io.audio == tr.arena.sets[0].inputs[0].data_ptr()
        ts.launch()
        l1 = ts.losses.clone()
        torch.cuda.synchronize()
        return l0, l1, flat.clone()

    for x, y in zip(run(False), run(True)):
        assert torch.equal(x, y)


def test_in_place_runs_allocate_no_padded_input_buffers(E):
    """_InputSet's padded feature buffers exist only once something is copied into them: an in-place run_epoch / step_from_store
    (row maps into the store) allocates none -- constructing the arena's steps touches no input set --, inplace=False does."""
    P, dims, Tcap, store, ix = _store_case(E)
    g = torch.Generator().manual_seed(1)
    batches = [torch.randperm(48, generator=g)[:B] for B in (6, 4, 6)]
    for inplace in (True, False):
        for epoch in (True, False):
            flat, lay = flat_from(E, P, dims)
            tr = E.FusedTrainer(flat, dims, lr=1e-3, seed=11, capacity=(6, Tcap), inplace=inplace)
            if epoch:
                tr.run_epoch(store, batches)
            else:
                tr.step_from_store(store, ix)
            torch.cuda.synchronize()
            assert torch.isfinite(tr.state.losses).all()
            if inplace:
                assert all(st._inputs is None for st in tr.arena.sets), epoch
            else:
                assert tr.arena.sets[0]._inputs is not None, epoch


def test_keep_bits_sets_are_tagged_with_call_and_shape(E):
    """sdumc_net_io.bits_next: a set is used only under a tag that names THIS call's {seed, call} AND batch shape, and a set regenerated
    at a step's head is re-tagged for that step.  Driven on purpose: (a) the Philox counter rewound to a value a set was once filled for
    while the phase was not flipped in between (stale masks under a matching tag, before the head re-tagged), (b) steps of two shapes
    sharing one arena buffer with and without the next shape announced.  Every variant equals the run that generates its keep-bits at
    the head of each step (bits_next off), bit for bit."""
    from oracle import sdumc_oracle as O
    dims = (64, 128, 64, 128)
    P = O.init_params(dims, seed=2)
    shapes = [(4, (70, 32, 64, 33)), (3, (66, 31, 70, 32))]
    data = {sh: [t.cuda() for t in O.synthetic_batch(sh[0], sh[1], dims, seed=50 + i)] for i, sh in enumerate(shapes)}

    def reference(seq, calls):
        flat, lay = flat_from(E, P, dims)
        state = E._RunState(flat, lay.live, 1e-3, 9)
        out = []
        for sh, call in zip(seq, calls):
            ts = E.TrainStep(flat, sh[0], sh[1], dims, share=state, bits_next=False)
            ts.set_batch(*data[sh])
            if call is not None:
                state.rng.set_call(call)
            out.append(ts.run().clone())
            torch.cuda.synchronize()
        return out, flat.clone()

    # (a) one shape, own buffer: steps at calls 0, 2, then the counter goes back to 2 WITHOUT a phase flip in between
    sh = shapes[0]
    flat, lay = flat_from(E, P, dims)
    ts = E.TrainStep(flat, sh[0], sh[1], dims, seed=9, lr=1e-3)
    assert ts._bits_next is not None
    ts.set_batch(*data[sh])
    got = [ts.run().clone(), ts.run().clone()]      # calls 0, 2; step 1's middle left set 0 = masks(call 4) under tag {4}, phase is 0 again
    ts.rng.set_call(10)            # a jump: step 2 finds set 0 tagged {4}, regenerates masks(call 10) into it -- and must re-tag it {10}
    got.append(ts.run().clone())
    ts.rng.set_call(4)             # back to call 4 ...
    ts.io.bits_phase ^= 1          # ... on set 0 again (phase not flipped): under the old tag {4} it would serve masks(call 10)
    got.append(ts.run().clone())
    ts.rng.set_call(0)             # and a rewind to the very first call on whatever the sets hold now
    got.append(ts.run().clone())
    torch.cuda.synchronize()
    want, wflat = reference([sh] * 5, [None, None, 10, 4, 0])
    for i, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(x, y), (i, x.tolist(), y.tolist())
    assert torch.equal(flat, wflat)
    # (b) two shapes in one arena: announced next shapes (run_epoch's way) and unannounced ones (the tag's shape words must refuse)
    seq = [shapes[0], shapes[1], shapes[1], shapes[0], shapes[0], shapes[1]]
    want, wflat = reference(seq, [None] * len(seq))
    cap = (4, tuple(max(a, b) for a, b in zip(shapes[0][1], shapes[1][1])))
    for announce in (True, False, "wrong"):
        flat, lay = flat_from(E, P, dims)
        tr = E.FusedTrainer(flat, dims, lr=1e-3, seed=9, capacity=cap, sets=1)
        got = []
        for i, shp in enumerate(seq):
            ts = tr._get(*shp).use_set(0)
            ts.set_batch(*data[shp])
            nxt = None
            if announce is True and i + 1 < len(seq):
                nxt = tr._get(*seq[i + 1])
            elif announce == "wrong":
                nxt = tr._get(*seq[i])          # always announces the CURRENT shape: wrong whenever the shape changes
            ts.launch(next_step=nxt, pregen=True)
            got.append(ts.losses.clone())
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip(got, want)):
            assert torch.equal(x, y), (announce, i, x.tolist(), y.tolist())
        assert torch.equal(flat, wflat), announce


def test_two_host_threads_with_their_own_contexts_match_the_sequential_run(E):
    """C-ABI: no state is shared between execution contexts (sdumc_ctx_create / sdumc_net_io.ctx) -- two host threads, each
    with its own context and its own torch stream, run three fused steps concurrently on separate parameter copies; both
    end bit-identical to the same steps run alone on the default context."""
    import threading
    from oracle import sdumc_oracle as O
    dims = (64, 32, 48, 32)
    B, Tn = 6, (70, 6, 30, 5)
    P = O.init_params(dims, seed=3)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=8)]

    def run(ctx, stream, out, k):
        with torch.cuda.stream(stream):
            flat, _ = flat_from(E, P, dims)
            ts = E.TrainStep(flat, B, Tn, dims, seed=5, ctx=ctx)
            ts.set_batch(*batch)
            ls = [ts.run().clone() for _ in range(3)]
            stream.synchronize()
        out[k] = (flat, ls)

    ref = {}
    run(None, torch.cuda.current_stream(), ref, 0)
    torch.cuda.synchronize()
    for _ in range(3):
        res, ths = {}, []
        ctxs = [E.ExecContext(), E.ExecContext()]
        for k in range(2):
            th = threading.Thread(target=run, args=(ctxs[k], torch.cuda.Stream(), res, k))
            th.start()
            ths.append(th)
        for th in ths:
            th.join()
        torch.cuda.synchronize()
        for k in range(2):
            assert torch.equal(res[k][0], ref[0][0])
            for a, b in zip(res[k][1], ref[0][1]):
                assert torch.equal(a, b)
        for c in ctxs:
            c.close()


def test_bf16_forward_is_bit_reproducible_over_200_runs_with_a_busy_neighbour(E):
    """The run-to-run differences of round 3 (2-20 % of bf16-storage forwards differed from the first in a
    few rows of the utterance-level stages' outputs, by up to 1e-2 -- wrong low halves of packed FP32 results next to bf16 MFMA
    workgroups): 200 eval-mode forwards of C3 (B = 64), every one on a freshly allocated workspace, the last 60 with a
    bandwidth-heavy copy loop on another stream beside them; all five outputs bit-identical to the first run's, and the first
    run equal to the fp64 evaluation of the first utterance-level layer from the kernel's own inputs is covered by the oracle
    tests (tests/test_gpu_fullsize.py)."""
    from oracle import sdumc_oracle as O
    dims, B, Tn = (1024, 4096, 1024, 4096), 64, (375, 32, 225, 32)
    P = O.init_params(dims, seed=0)
    flat, lay = flat_from(E, P, dims)
    g = torch.Generator(device="cuda").manual_seed(37)
    audio, text, video, feat4 = [torch.randn(B, Tn[i], dims[i], device="cuda", generator=g) for i in range(4)]
    side = torch.cuda.Stream()
    src, dst = torch.empty(32 << 20, device="cuda"), torch.empty(32 << 20, device="cuda")
    ref, bad = None, 0
    for rep in range(200):
        nc = E.NetCall(flat, audio, [text, feat4], video, False, None, bf16=True)
        torch.cuda.synchronize()
        if rep >= 140:
            with torch.cuda.stream(side):
                for _ in range(4):
                    dst.copy_(src)
        out = [t.clone() for t in nc.forward()]
        torch.cuda.synchronize()
        if ref is None:
            ref = out
        elif not all(torch.equal(a, b) for a, b in zip(ref, out)):
            bad += 1
    assert bad == 0, f"{bad} of 199 bf16-storage forwards differed from the first"


def test_context_options_select_the_schedule_without_touching_process_wide_state(E):
    """sdumc_ctx_set_option (no global state in the C ABI): a context with chain_cluster = 0 / concurrency = 0 runs
    csrc/chain.hip's kernels / one lane -- bit-identical to the same step under the deprecated process-wide setters -- while a step
    on the default context, before and after, still takes the clustered kernels (its gradients differ in the last bits from the
    plain kernels': another summation order)."""
    from oracle import sdumc_oracle as O
    from sdumc_amd import _lib
    dims, B, Tn = (64, 32, 64, 32), 7, (40, 6, 20, 6)
    P = O.init_params(dims, seed=4)
    batch = [t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=6)]

    def run(ctx=None):
        flat, lay = flat_from(E, P, dims)
        ts = E.TrainStep(flat, B, Tn, dims, seed=9, ctx=ctx)
        ts.set_batch(*batch)
        losses = ts.run().clone()
        torch.cuda.synchronize()
        return losses, ts.grads.clone(), flat.clone()

    default_before = run()
    ctx = E.ExecContext()
    ctx.set_option("chain_cluster", 0)
    ctx.set_option("concurrency", 0)
    with_ctx = run(ctx)
    default_after = run()
    try:
        _lib.lib.sdumc_set_chain_cluster(0)
        _lib.lib.sdumc_set_concurrency(0)
        with_globals = run()
    finally:
        _lib.lib.sdumc_set_chain_cluster(1)
        _lib.lib.sdumc_set_concurrency(1)
    for a, b in zip(with_ctx, with_globals):
        assert torch.equal(a, b)
    for a, b in zip(default_before, default_after):
        assert torch.equal(a, b)
    assert not torch.equal(default_before[1], with_ctx[1])          # (the clustered kernels really ran on the default context)
    ctx.set_option("chain_cluster", None)
    ctx.set_option("concurrency", None)
    back = run(ctx)
    for a, b in zip(back, default_before):
        assert torch.equal(a, b)
    ctx.close()
