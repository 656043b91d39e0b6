#!/usr/bin/env python
"""Record tests/golden/loss_stage_bits.npz: SHA-256 digests of what the Rank-N-Contrast launches of loss.hip write, on an MI355X,
from the library that SDUMC_LIB names -- a build of the commit BEFORE the heads of rnc_row_body / rnc_dfeat_body were reordered.

    SDUMC_LIB=<that build's libsdumc_hip.so> python tests/golden/make_loss_stage_bits.py [output path]

The runs are those of tests/test_gpu_loss_stage_bits.py (imported, not restated), so the fixture and the test cannot drift apart.
Per case one uint8[32] array: alone_n<n>_d<dim>[_off4] (dist, G, rowloss, loss, df of sdumc_rnc_fwd_bwd) and fused_n<n>_d<dim>[_off4]
(dist, G, rowloss, losses[1..6], d_rnc, d_vals, d_th, d_ct, d_z, hyper of sdumc_losses_fused_).  Data only."""
import os
import sys

import numpy as np
import torch  # noqa: F401  (before the HIP library: both must share torch's HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    from tests import test_gpu_loss_stage_bits as S
    from sdumc_amd import _lib as L
    out = sys.argv[1] if len(sys.argv) > 1 else S.GOLDEN
    d = {}
    for n, dim, offset in S.ALONE:
        d[S.key("alone", n, dim, offset)] = S.digest(S.alone_outputs(S.run_alone(L, n, dim, offset)))
    for n, dim, offset in S.FUSED:
        d[S.key("fused", n, dim, offset)] = S.digest(S.run_fused(L, n, dim, offset)[1])
    for k, v in d.items():
        print(k, v.tobytes().hex())
    np.savez_compressed(out, **d)
    print("library", L.LIB_PATH)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
