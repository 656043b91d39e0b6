#!/usr/bin/env python
"""Generate tests/golden/input_grads.npz from the REAL reference model.

    python tests/golden/make_input_grad_goldens.py <path of the reference checkout>

Imports toolkit/models/wengnet_mosei_mult_views_text_missing.py of the reference by path (never copies it), loads the oracle's seeded
parameters into it, runs it in float64 and eval mode on a ragged, zero-padded batch -- dims (48, 32, 40), B = 3, T = (7, 3, 5), once
per text-slot input (text, feat4) -- and records the gradients of  vals.sum() + sum(e.sum() for e in embeddings)  with respect to
the three input tensors.  Data only (np.savez_compressed, loadable with allow_pickle=False): the inputs in fp32 (exactly what was
fed, as float64 of these), the parameter seed, the input gradients in float64.
"""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

from oracle import sdumc_oracle as O  # noqa: E402

DIMS, B, T, PSEED = (48, 32, 40, 32), 3, (7, 3, 5, 3), 17
LENS = ((7, 3, 5, 2), (4, 1, 5, 3), (6, 2, 2, 1))      # valid frames of (audio, text, video, feat4) per sample; the rest is zero padding


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    spec = importlib.util.spec_from_file_location(
        "ref_model", os.path.join(sys.argv[1], "toolkit", "models", "wengnet_mosei_mult_views_text_missing.py"))
    ref_model = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_model)
    with contextlib.redirect_stdout(io.StringIO()):
        net = ref_model.WengnetMOSEIMultViewsTextMissing(types.SimpleNamespace(input_dims=DIMS))
    net.load_state_dict(O.init_params(DIMS, seed=PSEED), strict=True)
    net = net.double().eval()
    feats = list(O.synthetic_batch(B, T, DIMS, seed=4321)[:4])
    for i, f in enumerate(feats):
        for b in range(B):
            f[b, LENS[b][i]:] = 0
    d = {"dims": np.array(DIMS), "T": np.array(T), "pseed": np.int64(PSEED), "lens": np.array(LENS)}
    for name, f in zip(("audio", "text", "video", "feat4"), feats):
        d[name] = f.numpy().astype(np.float32)
    audio, text, video, feat4 = feats
    for s, tx in enumerate((text, feat4)):
        leaves = [t.double().clone().requires_grad_() for t in (audio, tx, video)]
        vals, emb = net(leaves + [bool(s)])
        (vals.sum() + sum(e.sum() for e in emb)).backward()
        d[f"vals{s}"] = vals.detach().numpy()
        for n, t in zip(("audio", "text", "video"), leaves):
            d[f"d_{n}{s}"] = t.grad.numpy()
    np.savez_compressed(os.path.join(OUT, "input_grads.npz"), **d)
    print("wrote input_grads.npz:", {k: v.shape for k, v in d.items()})


if __name__ == "__main__":
    main()
