"""Bit-for-bit digests of the utterance-level stages (csrc/chain.hip, csrc/chain_cluster.hip) for comparing two builds of the library:
one SHA-256 per case over everything the case produces (losses, outputs, gradient bucket, updated parameters), one JSON line in all.
Cases: a / b / c / d of tests/test_gpu_chain_tail.py (odd V: a dead row in the last workgroup and cluster; plain and clustered kernels;
the bf16 weight stream) and three TrainStep steps at B = 7 (test_clustered_utterance_level_kernels_equal_the_plain_ones' shape) with
the cluster switch off and on.  Run it once per library, each in a fresh process (SDUMC_LIB=<other build> selects the library); a
refactor of those files must leave every digest equal.
usage: [SDUMC_LIB=path/to/libsdumc_hip.so] python tools/chain_digest.py"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def steps_b7(E, cluster):
    import torch
    from oracle import sdumc_oracle as O
    from sdumc_amd import _lib
    from tests.test_gpu_net import flat_from
    dims, B, Tn = (64, 32, 64, 32), 7, (40, 6, 20, 6)
    flat, _ = flat_from(E, O.init_params(dims, seed=4), dims)
    try:
        _lib.lib.sdumc_set_chain_cluster(cluster)
        ts = E.TrainStep(flat, B, Tn, dims, seed=9)
        ts.set_batch(*[t.cuda() for t in O.synthetic_batch(B, Tn, dims, seed=6)])
        ls = [ts.run().cpu().clone() for _ in range(3)]
        torch.cuda.synchronize()
    finally:
        _lib.lib.sdumc_set_chain_cluster(1)
    return ls + [ts.vals, ts.fused, ts.rnc, ts.text_hidden, ts.cross_text, ts.grads, flat]


def main():
    import torch
    from sdumc_amd import _lib, engine as E
    from tests import test_gpu_chain_tail as T
    torch.cuda.set_device(0)
    out = {"library": os.environ.get("SDUMC_LIB", "tree")}
    for cluster in (0, 1):
        for name, B, train, bwd in (("a", 3, True, True), ("b", 1, True, True), ("c", 3, False, False)):
            outs, grads = T.run_net(E, B, train, cluster, backward=bwd)
            out[f"{name}_cluster{cluster}"] = sha(outs + ([grads] if bwd else []))
        out[f"step_b7_cluster{cluster}"] = sha(steps_b7(E, cluster))
    out["d_bf16"] = sha(T.run_bf16_step(E, True))
    out["cluster_error"] = int(_lib.lib.sdumc_chain_cluster_error_())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
