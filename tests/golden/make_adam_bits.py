#!/usr/bin/env python
"""Record tests/golden/adam_bits.npz: SHA-256 digests of what the launches of adam.hip write, on an MI355X, from the library that
SDUMC_LIB names (or the tree's own) -- a build of the commit BEFORE the forms of the Adam kernels were folded into shared bodies.

    SDUMC_LIB=<that build's libsdumc_hip.so> python tests/golden/make_adam_bits.py [output path]

The runs are those of tests/test_gpu_adam_bits.py (imported, not restated), so the fixture and the test cannot drift apart.  Every case
runs TWICE: a flat-bucket or per-parameter case whose two digests differ refuses the whole fixture (exit status 1, nothing written); a
fused-step case whose two digests differ is named and left out (the whole step need not reproduce its bits run to run).  Per case one
uint8[32] array under the key the test asks for.  Data only."""
import os
import sys

import numpy as np
import torch  # noqa: F401  (before the HIP library: both must share torch's HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    from tests import test_gpu_adam_bits as S
    from sdumc_amd import _lib, ops
    out = sys.argv[1] if len(sys.argv) > 1 else S.GOLDEN
    cases = [(S.flat_key(*c), True, lambda c=c: S.run_flat(ops, *c)) for c in S.FLAT]
    cases += [(S.multi_key(*c), True, lambda c=c: S.run_multi(ops, *c)) for c in S.MULTI]
    cases += [(S.fused_key(w), False, lambda w=w: S.run_fused(w)) for w in S.FUSED]
    d, refused = {}, []
    for key, must, run in cases:
        a, b = S.digest(run()), S.digest(run())
        same = np.array_equal(a, b)
        print(key, a.tobytes().hex(), "" if same else "!= second run " + b.tobytes().hex())
        if same:
            d[key] = a
        elif must:
            refused.append(key)
        else:
            print("left out:", key)
    print("library", _lib.LIB_PATH)
    if refused:
        print("NOT written: two runs differ for", refused)
        return 1
    np.savez_compressed(out, **d)
    print("wrote", out, os.path.getsize(out), "bytes,", len(d), "of", len(cases), "cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
