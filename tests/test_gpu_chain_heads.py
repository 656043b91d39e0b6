"""The heads of the clustered utterance-level stages (csrc/chain_cluster.hip): every request of a head goes out before its first
wait -- chunk statistics, the first batch of partial rows, biases, alpha, saved activations, the first layer's weights -- and the
in-place normalisation of the stored attention weights is finished behind the first layer group.  The shapes are chosen for where a
reordered head can go wrong, not for the workload:

  * B = 7 (the last cluster holds rows beyond V) and B = 1 (V = 2: the one cluster's members see `v >= V` wherever a request is
    clamped instead of branched around);
  * T = (520, 6, 70, 6): audio has 9 chunks -- both branches of the statistics and the second batch of the partial-row pipeline --,
    video 2, text 1;  T = (40, 6, 20, 6): every site is a single chunk.

Clustered against plain compares two summation orders (the plain path combines the chunks in launches of their own), at the bars
of test_gpu_net.test_clustered_utterance_level_kernels_equal_the_plain_ones; the stored weights are a product of one exponential
and one reciprocal per frame in both paths, held to 1e-5 absolute; run-to-run is bit for bit."""
import numpy as np
import pytest
import torch

from tests.test_gpu_eval_attention import _plan_offsets
from tests.test_gpu_net import flat_from

pytestmark = pytest.mark.gpu

DIMS = (64, 32, 64, 32)
SHAPES = [(7, (520, 6, 70, 6)), (7, (40, 6, 20, 6)), (1, (520, 6, 70, 6)), (1, (40, 6, 20, 6))]
IDS = [f"B{B}-T{T[0]}" for B, T in SHAPES]


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import engine
    return engine


def _steps(E, B, Tn, cluster, n):
    """n TrainStep steps (fresh masks each) under the given cluster switch -> (losses per step, gradient bucket, parameters), on the CPU"""
    from oracle import sdumc_oracle as O
    from sdumc_amd import _lib
    flat, _ = flat_from(E, O.init_params(DIMS, seed=4), DIMS)
    try:
        _lib.lib.sdumc_set_chain_cluster(cluster)
        ts = E.TrainStep(flat, B, Tn, DIMS, seed=9)
        ts.set_batch(*[t.cuda() for t in O.synthetic_batch(B, Tn, DIMS, seed=6)])
        ls = [ts.run().cpu().clone() for _ in range(n)]
        torch.cuda.synchronize()
        out = (ls, ts.grads.cpu().clone(), flat.cpu().clone())
    finally:
        _lib.lib.sdumc_set_chain_cluster(1)
    assert _lib.lib.sdumc_chain_cluster_error_() == 0
    return out


@pytest.mark.parametrize("B,Tn", SHAPES, ids=IDS)
def test_clustered_against_plain(E, B, Tn):
    """three steps with fresh masks, clustered against plain: losses, gradients, parameters"""
    from sdumc_amd import _lib
    assert _lib.lib.sdumc_chain_cluster_fits_(2 * B) == 1
    plain, clus = _steps(E, B, Tn, 0, 3), _steps(E, B, Tn, 1, 3)
    gscale = float(plain[1].abs().max())
    print(f"B={B} T={Tn}: max |loss diff| {max(float((a - b).abs().max()) for a, b in zip(plain[0], clus[0])):.3e}  "
          f"max |grad diff| / max |grad| {float((plain[1] - clus[1]).abs().max()) / gscale:.3e}  "
          f"max |param diff| {float((plain[2] - clus[2]).abs().max()):.3e}")
    for a, b in zip(plain[0], clus[0]):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=2e-5, atol=1e-6)
    assert float((plain[1] - clus[1]).abs().max()) < 2e-5 * gscale
    assert not torch.equal(plain[1], clus[1])            # (the clustered path really ran)
    assert float((plain[2] - clus[2]).abs().max()) < 1e-4


def _stored_weights(E, B, Tn, train, cluster):
    """The stored attention weights of both kinds of site after one two-stream NetCall (train: forward + backward; eval: forward),
    read from the call's workspace through sdumc_debug_plan_table: [kind][modality] -> [V, T, nq] on the CPU (kind 0 = FRA2UTT,
    nq = 1; kind 1 = Cross_Attention, nq = 7)."""
    from oracle import sdumc_oracle as O
    from sdumc_amd import _lib
    flat, _ = flat_from(E, O.init_params(DIMS, seed=4), DIMS)
    audio, text, video, feat4, _ = [t.cuda() for t in O.synthetic_batch(B, Tn, DIMS, seed=6)]
    V = 2 * B
    try:
        _lib.lib.sdumc_set_chain_cluster(cluster)
        nc = E.NetCall(flat, audio, [text, feat4], video, train, E.RngState(13, "cuda", call=6) if train else None)
        nc.forward()
        if train:
            g = torch.Generator().manual_seed(3)
            douts = [torch.randn(V, 1, generator=g), torch.randn(V, 128, generator=g), torch.randn(V, 64, generator=g),
                     torch.randn(V, 256, generator=g), torch.randn(V, 7, 128, generator=g)]
            nc.backward(*[d.cuda().contiguous() for d in douts])
        torch.cuda.synchronize()
        ws = nc.workspace.view(torch.float32)
        offs = _plan_offsets(_lib, nc.dims)
        out = []
        for kind, nq in ((0, 1), (1, 7)):
            per = []
            for mk, T in zip("atv", (Tn[0], Tn[1], Tn[2])):
                o, n = offs[f"attn{kind}{mk}"]
                assert n == V * T * nq      # (text and feat4 share their length: one run per modality, the shape the fold accepts)
                per.append(ws[o:o + n].reshape(V, T, nq).cpu().clone())
            out.append(per)
    finally:
        _lib.lib.sdumc_set_chain_cluster(1)
    assert _lib.lib.sdumc_chain_cluster_error_() == 0
    return out


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B,Tn", SHAPES, ids=IDS)
def test_stored_weights_are_normalised(E, B, Tn, train):
    """every (sample, query) row of the stored weights sums to 1 over its frames within 1e-5 and equals the plain path's within the
    same bar: a normalisation deferred past its consumers, or applied with a stale factor, shows here"""
    clus, plain = _stored_weights(E, B, Tn, train, 1), _stored_weights(E, B, Tn, train, 0)
    worst_sum = worst_diff = 0.0
    for kind in range(2):
        for m in range(3):
            c, p = clus[kind][m].double(), plain[kind][m].double()
            worst_sum = max(worst_sum, float((c.sum(1) - 1).abs().max()))
            worst_diff = max(worst_diff, float((c - p).abs().max()))
    print(f"B={B} T={Tn} train={train}: worst |row sum - 1| {worst_sum:.3e}  worst |clustered - plain| {worst_diff:.3e}")
    assert worst_sum <= 1e-5
    assert worst_diff <= 1e-5


def test_run_to_run(E):
    """ten steps at B = 7, T = (520, 6, 70, 6), twice from the same state: losses, gradients and parameters bit for bit"""
    first, second = _steps(E, 7, (520, 6, 70, 6), 1, 10), _steps(E, 7, (520, 6, 70, 6), 1, 10)
    for a, b in zip(first[0], second[0]):
        assert torch.equal(a, b)
    assert torch.equal(first[1], second[1])
    assert torch.equal(first[2], second[2])
