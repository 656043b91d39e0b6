"""The utterance-level stages (csrc/chain.hip, csrc/chain_cluster.hip) with an ODD number of virtual samples: every workgroup and
every cluster owns R = 2 rows, so V = 3 leaves the last one with one live and one dead row and V = 1 makes the only one ragged.
The sections the two families share (csrc/chain_common.h) are mostly the handling of that dead row: zero-fills in LDS, no write
to HBM.  The rest of the suite drives these kernels with even V only (two streams).

Bars: against the oracle the ones tests/test_gpu_net.py uses (forward 1e-4, gradients 2e-4 of each tensor's scale); plain against
clustered 2e-5 of the largest element, as test_clustered_utterance_level_kernels_equal_the_plain_ones has it (same arithmetic,
different summation order); bf16 storage against fp32 storage the loss bar of tests/test_gpu_configs.py (2e-2)."""
import numpy as np
import pytest
import torch

from tests import grad_parity as GP
from tests.test_gpu_net import NAMES, _oracle_grads, close, flat_from

pytestmark = pytest.mark.gpu

DIMS, TN = (64, 32, 64, 32), (40, 6, 20, 6)
DIMS_BF16 = (64, 64, 64, 64)      # bf16 STORAGE needs feature widths in whole 64-element k-tiles (engine.bf16_mode)
SEED, CALL0 = 13, 6


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import engine
    return engine


def net_inputs(B):
    """parameters, one-stream batch and the five external gradients of a B-sample call"""
    from oracle import sdumc_oracle as O
    P = O.init_params(DIMS, seed=4)
    audio, text, video, _, _ = O.synthetic_batch(B, TN, DIMS, seed=6)
    g = torch.Generator().manual_seed(3)
    douts = [torch.randn(B, 1, generator=g), torch.randn(B, 128, generator=g), torch.randn(B, 64, generator=g),
             torch.randn(B, 256, generator=g), torch.randn(B, 7, 128, generator=g)]
    return P, (audio, text, video), douts


def run_net(E, B, train, cluster, backward=True):
    """One-stream NetCall (V = B) under the given cluster switch -> (the five outputs, gradient bucket or None), on the CPU"""
    from sdumc_amd import _lib
    P, (audio, text, video), douts = net_inputs(B)
    flat, _ = flat_from(E, P, DIMS)
    try:
        _lib.lib.sdumc_set_chain_cluster(cluster)
        call = E.NetCall(flat, audio.cuda(), [text.cuda()], video.cuda(), train, E.RngState(SEED, "cuda", call=CALL0))
        outs = [o.cpu().clone() for o in call.forward()]
        grads = call.backward(*[d.cuda().contiguous() for d in douts]).cpu().clone() if backward else None
        torch.cuda.synchronize()
    finally:                                     # process-wide switch (tests/conftest.py restores it too)
        _lib.lib.sdumc_set_chain_cluster(1)
    assert _lib.lib.sdumc_chain_cluster_error_() == 0
    return outs, grads


def run_bf16_step(E, bf16):
    """One TrainStep at B = 3, both streams (V = 6), plain kernels -> (losses, gradient bucket, updated parameters), on the CPU"""
    from oracle import sdumc_oracle as O
    from sdumc_amd import _lib
    P = O.init_params(DIMS_BF16, seed=4)
    batch = O.synthetic_batch(3, TN, DIMS_BF16, seed=6)
    flat, _ = flat_from(E, P, DIMS_BF16)
    try:
        _lib.lib.sdumc_set_chain_cluster(0)
        ts = E.TrainStep(flat, 3, TN, DIMS_BF16, seed=9, bf16=bf16)
        assert ts.dims.bf16 == (2 if bf16 else 0)
        ts.set_batch(*[t.cuda() for t in batch])
        losses = ts.run().cpu().clone()
        torch.cuda.synchronize()
    finally:
        _lib.lib.sdumc_set_chain_cluster(1)
    assert _lib.lib.sdumc_chain_cluster_error_() == 0
    return losses, ts.grads.cpu().clone(), flat.cpu().clone()


_oracle_cache = {}


def oracle(B, mode, backward=True):
    """fp64 oracle of run_net's call (outputs, gradients) and the fp32 oracle's gradients, computed once per (B, mode)"""
    key = (B, mode)
    if key not in _oracle_cache:
        from oracle import sdumc_oracle as O
        P, (audio, text, video), douts = net_inputs(B)
        d = O.DropCtx("eval" if mode == "eval" else "philox", SEED, CALL0)
        y, (z, r, th, ct) = O.forward({k: v.double() for k, v in P.items()}, audio.double(), text.double(), video.double(), d)
        grads = _oracle_grads(P, audio, [text], video, mode, SEED, CALL0, douts) if backward else None
        grads32 = _oracle_grads(P, audio, [text], video, mode, SEED, CALL0, douts, dtype=torch.float32) if backward else None
        _oracle_cache[key] = ((y, z, r, th, ct), grads, grads32)
    return _oracle_cache[key]


@pytest.mark.parametrize("B", [3, 1])
def test_odd_sample_count_forward_backward_both_families_vs_oracle(E, B):
    """Cases a (V = 3) and b (V = 1): train-mode forward, backward with all five external gradients, plain and clustered."""
    want_outs, want_grads, grads32 = oracle(B, "train")
    lay = E.ParamLayout.get(*DIMS[:3])
    res = [run_net(E, B, True, cluster) for cluster in (0, 1)]
    for cluster, (outs, grads) in enumerate(res):
        for name, got, want in zip(NAMES, outs, want_outs):
            close(got, want, 1e-4, f"{name} cluster={cluster}")
        gv = lay.views(torch.cat([grads, torch.zeros(lay.total - lay.live)]))
        assert set(want_grads) == set(lay.live_names())
        for k in lay.live_names():
            close(gv[k], want_grads[k], 2e-4, f"{k} cluster={cluster}")
        # (that bar is tied to max(1, |g|)) every tensor against its own norm: external gradients of O(1), every tensor carries signal
        own = GP.tensor_errors(lay, gv, want_grads, grads32, 2e-4, what=f"fp32 NetCall train, V = {B}, cluster={cluster}")
        assert len(own) == len(lay.live_names())
    for name, a, b in zip(NAMES, res[0][0], res[1][0]):
        assert float((a - b).abs().max()) < 2e-5 * float(a.abs().max()), name
    gscale = float(res[0][1].abs().max())
    assert float((res[0][1] - res[1][1]).abs().max()) < 2e-5 * gscale
    if B == 3:
        assert not torch.equal(res[0][1], res[1][1])            # (the clustered path really ran)


def test_odd_sample_count_eval_forward_vs_oracle(E):
    """Case c: eval mode (no dropout, relu_scale = 1), V = 3, both families."""
    want_outs = oracle(3, "eval", backward=False)[0]
    for cluster in (0, 1):
        outs, _ = run_net(E, 3, False, cluster, backward=False)
        for name, got, want in zip(NAMES, outs, want_outs):
            close(got, want, 1e-4, f"{name} cluster={cluster}")


def test_bf16_weight_stream_runs_the_shared_sections_reproducibly(E):
    """Case d: a bf16-storage step at B = 3 with the cluster switch off, so that stage A runs chain.hip's bf16-weight kernels over
    the shared sections: two runs from the same state are bit-equal; losses agree with the fp32-storage step at the bf16 bar."""
    a, b, f32 = run_bf16_step(E, True), run_bf16_step(E, True), run_bf16_step(E, False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
    np.testing.assert_allclose(a[0].numpy()[:7], f32[0].numpy()[:7], rtol=2e-2, atol=1e-4)
    assert not torch.equal(a[1], f32[1]), "bf16 mode is not active"
