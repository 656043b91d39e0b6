"""bf16 storage against its discriminating reference -- the fp64 evaluation that rounds where the engine rounds (oracle/bf16_storage.py)
-- at the shapes where kernels break.  tests/test_gpu_fullsize.py holds the mode to that reference at C2 B = 64 and C5 B = 32 only
(aligned T, no lengths); every other bf16-storage test compares against fp32 at 2e-2 / 0.2 or against itself, and the emulation
itself sits 1-4 % from the plain oracle per gradient tensor, so those bars cannot see a wrong kernel.  Here:

  case  dims                  B  T (a, t, v, feat4)
  1     (128, 128, 128, 128)  1  (1, 1, 1, 1)       a single frame: 37 tensors are exactly zero in the reference (softmax over one frame;
                                                    RnC over n = 2 rows), named to the helper
  2     (64, 192, 64, 192)    3  (65, 1, 64, 2)     widths 64 mod 128 (the route without the fragment-major kernels); T across the
                                                    64-frame chunk; a one-frame text slot
  3     (128, 256, 128, 256)  5  (70, 9, 33, 4)     unequal text slots (two text runs), odd B
  4     (64, 64, 64, 64)      2  (130, 3, 129, 5)   two whole chunks + 2 / + 1 frames
  5     (192, 64, 128, 64)    7  (64, 64, 64, 64)   odd B, whole chunks
  6     (128, 128, 128, 128)  4  (70, 9, 33, 6)     key-padding lengths (those of test_train_step_with_lengths_vs_oracle)
  7     (128, 128, 128, 128)  2  (70, 9, 33, 32)    feat4's B T = 64 rows are a whole tile, text's 18 are not: one projection launch per
                                                    stream (the one-launch rule of the text slot is read off stream 0's rows alone)

One TrainStep(bf16=True) in train mode with Philox masks each: the loss and its six terms and the five outputs of both streams at
BF16_EMU_OUT_TOL, every gradient tensor through tests/grad_parity.py at BF16_EMU_GRAD_TOL (the project's numbers:
tests/test_gpu_fullsize.py).  On the CPU the emulation's own fp32-against-fp64 distance at these cases is at most 1.6e-3 for every
tensor with signal (case 4, fra2utt_1.input_proj.bias), below BF16_EMU_GRAD_TOL / 4: no in-between raise applies.  And an eval-mode
NetCall(bf16=True) forward + backward with O(1) random output gradients at cases 2 and 3, one and two streams (emulation's own
distance at most 2.1e-3).
Measured on MI355X (profiles/grad_parity_by_tensor.txt): losses to 1e-7, outputs to 6.5e-5; gradients, median over the tensors 2e-7
(case 1) .. 2e-5, worst tensor of a step 3.3e-3 .. 3.6e-3 in every case but the first -- always a frame_dim_reshape weight, whose
gradient is a product of two bf16-stored tensors (dx and the features) --, worst of a NetCall 3.8e-3 (fra2utt_2.input_proj.bias)."""
import numpy as np
import pytest
import torch

from tests import grad_parity as GP
from tests.test_gpu_configs import NAMES, close, flat_from
from tests.test_gpu_fullsize import BF16_EMU_GRAD_TOL, BF16_EMU_OUT_TOL

pytestmark = pytest.mark.gpu

LENS = ([70, 12, 65, 1], [9, 3, 1, 8], [33, 33, 2, 17], [6, 1, 4, 5])
#        dims                  B  T                  lengths
CASES = {1: ((128, 128, 128, 128), 1, (1, 1, 1, 1), False),
         2: ((64, 192, 64, 192), 3, (65, 1, 64, 2), False),
         3: ((128, 256, 128, 256), 5, (70, 9, 33, 4), False),
         4: ((64, 64, 64, 64), 2, (130, 3, 129, 5), False),
         5: ((192, 64, 128, 64), 7, (64, 64, 64, 64), False),
         6: ((128, 128, 128, 128), 4, (70, 9, 33, 6), True),
         7: ((128, 128, 128, 128), 2, (70, 9, 33, 32), False)}


def site_tensors(m):
    """the parameters of modality m's two attention sites that only the softmax's gradient reaches: zero where T = 1"""
    return [f"fra2utt_{m}.attention_context_vector", f"fra2utt_{m}.input_proj.weight", f"fra2utt_{m}.input_proj.bias"] + \
           [f"cross_att_fra2utt_{m}.{p}.{w}" for p in ("query_proj", "input_proj") for w in ("weight", "bias")]


# case 1: no softmax gradient at any site, so nothing reaches the queries -- but for the text query, which is the distillation's
# text_hidden -- and RnC over the two rows of one sample has one positive and no negative per anchor: its gradient vanishes
ZEROS_ONE_FRAME = sum((site_tensors(m) for m in range(3)), []) + \
    [f"cross_{q}_query_mlp.0.{w}" for q in ("fused", "at", "tv", "av", "audio", "video") for w in ("weight", "bias")] + \
    [f"orgin_linear_change.{i}.{w}" for i in (0, 2) for w in ("weight", "bias")]


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import engine
    return engine


def case_inputs(case):
    from oracle import sdumc_oracle as O
    dims, B, Tn, with_lengths = CASES[case]
    P = O.init_params(dims, seed=20 + case)
    batch = list(O.synthetic_batch(B, Tn, dims, seed=40 + case))
    lens = None
    if with_lengths:
        lens = [torch.tensor(l, dtype=torch.int32) for l in LENS]
        for t, l in zip(batch[:4], lens):
            for b in range(B):
                t[b, int(l[b]):] = 0
    return dims, B, Tn, P, batch, lens


@pytest.mark.parametrize("case", sorted(CASES))
def test_bf16_step_at_the_edges_vs_rounding_emulation(E, case):
    from oracle import sdumc_oracle as O
    from oracle.bf16_storage import Bf16Storage
    assert len(ZEROS_ONE_FRAME) == 37
    dims, B, Tn, P, batch, lens = case_inputs(case)
    seed = 6 + case
    flat, lay = flat_from(E, P, dims)
    ts = E.TrainStep(flat, B, Tn, dims, seed=seed, bf16=True)
    assert ts.dims.bf16 == 2
    ts.set_batch(*[t.cuda() for t in batch])
    if lens is not None:
        ts.set_lengths(lens)
    losses = ts.run().cpu().numpy()
    got_outs = [t.cpu().clone() for t in (ts.vals, ts.fused, ts.rnc, ts.text_hidden, ts.cross_text)]
    gv = lay.views(torch.cat([ts.grads.cpu(), torch.zeros(lay.total - lay.live)]))
    loss64, terms64, hi, outs64 = O.train_step({k: v.double() for k, v in P.items()}, {}, *[t.double() for t in batch], mode="philox",
                                               seed=seed, step=0, lengths=lens, st=Bf16Storage())
    lo = GP.oracle_step_grads(P, batch, seed, dtype=torch.float32, lengths=lens, st=Bf16Storage())
    want = np.array([float(loss64)] + [float(t) for t in terms64])
    assert np.isfinite(want).all()
    worst_out = max(float((got[s * B:(s + 1) * B].double() - w.detach().reshape(got[s * B:(s + 1) * B].shape)).abs().max()) / max(1.0, float(w.detach().abs().max()))
                    for s in range(2) for got, w in zip(got_outs, outs64[s]))
    print("bf16 edges case %d: losses rel. error %.3g, outputs worst |error| / max(1, |want|) %.3g" %
          (case, float(np.abs(losses[:7] - want).max() / np.abs(want).max()), worst_out))
    np.testing.assert_allclose(losses[0], want[0], rtol=BF16_EMU_OUT_TOL)
    np.testing.assert_allclose(losses[1:7], want[1:], rtol=BF16_EMU_OUT_TOL, atol=1e-5)
    for s in range(2):
        for n, got, w in zip(NAMES, got_outs, outs64[s]):
            close(got[s * B:(s + 1) * B], w, BF16_EMU_OUT_TOL, f"case {case}: {n} stream {s}")
    assert set(hi) == set(lay.live_names())
    res = GP.tensor_errors(lay, gv, hi, lo, BF16_EMU_GRAD_TOL, zeros=ZEROS_ONE_FRAME if case == 1 else (),
                           what=f"bf16 edges case {case}, step vs emulation")
    assert len(res.zero) == (37 if case == 1 else 0) and len(res) + len(res.nosignal) + len(res.zero) == 83


def _emulated_call(P, audio, texts, video, douts, lens, dtype):
    """outputs of every stream and the parameter gradients of sum(out * dout) of an eval-mode call through the rounding emulation"""
    from oracle import sdumc_oracle as O
    from oracle.bf16_storage import Bf16Storage
    st = Bf16Storage()
    leaves = {k: v.to(dtype).requires_grad_(not O.is_dead(k)) for k, v in P.items()}
    a, v, txs = audio.to(dtype), video.to(dtype), [t.to(dtype) for t in texts]      # one tensor each: the emulation shares x by identity
    total, outs = 0, []
    for s, tx in enumerate(txs):
        l = None if lens is None else (lens[0], lens[1 + 2 * s], lens[2])
        y, (z, r, th, ct) = O.forward(leaves, a, tx, v, O.DropCtx("eval"), lengths=l, st=st)
        B = y.shape[0]
        outs.append([o.detach() for o in (y, z, r, th, ct)])
        for o, do in zip((y, z, r, th, ct), douts):
            total = total + (o * do[s * B:(s + 1) * B].to(dtype).reshape(o.shape)).sum()
    total.backward()
    return outs, {k: t.grad for k, t in leaves.items() if t.grad is not None}


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("case", [2, 3])
def test_bf16_netcall_forward_backward_vs_rounding_emulation(E, case, streams):
    """eval mode, external output gradients of O(1) on all five outputs (as test_gpu_net.py::test_backward_vs_oracle): the gradients
    are then O(1) too and the RnC head's biases carry signal.  One stream at case 2 has only the one-frame text slot: that modality's
    seven site tensors are exactly zero."""
    dims, B, Tn, P, batch, lens = case_inputs(case)
    audio, text, video, feat4, _ = batch
    texts = [text, feat4][:streams]
    V = streams * B
    g = torch.Generator().manual_seed(case)
    douts = [torch.randn(V, 1, generator=g), torch.randn(V, 128, generator=g), torch.randn(V, 64, generator=g),
             torch.randn(V, 256, generator=g), torch.randn(V, 7, 128, generator=g)]
    flat, lay = flat_from(E, P, dims)
    call = E.NetCall(flat, audio.cuda(), [t.cuda() for t in texts], video.cuda(), False, None, bf16=True)
    outs = [o.cpu().clone() for o in call.forward()]
    grads = call.backward(*[d.cuda().contiguous() for d in douts])
    gv = lay.views(torch.cat([grads.cpu(), torch.zeros(lay.total - lay.live)]))
    outs64, hi = _emulated_call(P, audio, texts, video, douts, lens, torch.float64)
    _, lo = _emulated_call(P, audio, texts, video, douts, lens, torch.float32)
    for s in range(streams):
        for n, got, w in zip(NAMES, outs, outs64[s]):
            close(got[s * B:(s + 1) * B], w, BF16_EMU_OUT_TOL, f"case {case}, {streams} stream(s): {n} stream {s}")
    zeros = site_tensors(1) if (streams == 1 and Tn[1] == 1) else ()
    res = GP.tensor_errors(lay, gv, hi, lo, BF16_EMU_GRAD_TOL, zeros=zeros,
                           what=f"bf16 edges case {case}, NetCall eval, {streams} stream(s) vs emulation")
    assert len(res.zero) == len(zeros) and not res.nosignal
