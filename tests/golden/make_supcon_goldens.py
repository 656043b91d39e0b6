#!/usr/bin/env python
"""Generate tests/golden/supcon.npz from the REAL reference's SupConLoss (toolkit/utils/loss.py:143-240).

    python tests/golden/make_supcon_goldens.py <path of the reference checkout>

Imports toolkit/utils/loss.py of the reference by path (never copies it) and runs SupConLoss on the CPU with torch
autograd, in float64 (the recorded value and gradient) and in float32 (only to record the reference's own fp32 rounding:
the bar the kernel is held to).  loss.py:233 calls .cuda() on a fresh tensor; torch.Tensor.cuda is patched to return
self for the run.  Data only (np.savez_compressed, loadable with allow_pickle=False).

Per case <name>:
  <name>_feat    [bsz, n_views, D] float32 inputs (seeded normal draws)
  <name>_labels  [bsz] float32, or <name>_mask [bsz, bsz] float32, or neither (SimCLR)
  <name>_opts    float64 [5]: temperature, base_temperature, contrast_mode == 'all', normalised in the graph, label mode
                 (1: the reference was given rint(labels), the kernel gets the labels as recorded)
  <name>_value   float64 scalar, <name>_grad float64 [bsz, n_views, D]: d value / d feat (through F.normalize where
                 opts[3] is set, so the gradient is with respect to the raw rows)
  <name>_gap     float64 [3]: |value32 - value64|, max |grad32 - grad64|, |grad32 - grad64| / |grad64| (2-norms)
Cases: cls7, simclr, one, mask, v1, odd, t05, prenorm, zero, round (the table in the generator below).
n1024_gap      float64 [5]: the same three gaps, then |value64| and max |grad64|, at bsz 512 x 2 views x 64, 7 classes,
               normalised: the bar for the larger shapes the tests check against their own restatement.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

OUT = os.path.dirname(os.path.abspath(__file__))


def load_reference_losses(ref):
    spec = importlib.util.spec_from_file_location("ref_toolkit_loss", os.path.join(ref, "toolkit", "utils", "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(ref, feat, dtype, norm, labels=None, mask=None, **ctor):
    f = feat.to(dtype).clone().requires_grad_()
    x = F.normalize(f, dim=-1) if norm else f
    crit = ref.SupConLoss(**ctor)
    l = crit(x, labels=None if labels is None else labels.to(dtype), mask=None if mask is None else mask.to(dtype))
    l.backward()
    return l.detach().double(), f.grad.double()


def gaps(ref, feat, norm, **kw):
    l32, g32 = run(ref, feat, torch.float32, norm, **kw)
    l64, g64 = run(ref, feat, torch.float64, norm, **kw)
    assert torch.isfinite(l64) and torch.isfinite(g64).all()
    gap = np.array([abs(float(l32 - l64)), float((g32 - g64).abs().max()), float((g32 - g64).norm() / g64.norm())])
    return l64, g64, gap


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference_losses(sys.argv[1])
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self      # loss.py:233, on the CPU
    try:
        g = torch.Generator().manual_seed(20241018)
        ri = lambda hi, n: torch.randint(0, hi, (n,), generator=g).float()
        asym = (torch.rand(8, 8, generator=g) > 0.5).float()
        assert not torch.equal(asym, asym.T)
        # name, bsz, views, D, normalised in the graph, label mode, call arguments
        cases = [
            ("cls7", 16, 2, 64, True, 0, dict(labels=ri(7, 16))),
            ("simclr", 16, 2, 64, True, 0, dict()),
            ("one", 16, 2, 64, True, 0, dict(labels=ri(3, 16), contrast_mode='one')),
            ("mask", 8, 3, 32, True, 0, dict(mask=asym)),
            ("v1", 6, 1, 16, True, 0, dict(labels=torch.tensor([0., 1, 1, 2, 3, 3]))),
            ("odd", 13, 2, 5, True, 0, dict(labels=ri(4, 13))),
            ("t05", 16, 2, 64, True, 0, dict(labels=ri(7, 16), temperature=0.5)),
            ("prenorm", 16, 2, 64, False, 0, dict(labels=ri(7, 16))),
            ("zero", 8, 2, 16, True, 0, dict(labels=ri(3, 8))),
            ("round", 16, 2, 64, True, 1, dict(labels=torch.rand(16, generator=g) * 6 - 3)),
        ]
        d = {}
        for name, bsz, views, D, norm, mode, kw in cases:
            feat = torch.randn(bsz, views, D, generator=g)
            if name == "prenorm":
                feat = F.normalize(feat, dim=-1)
            if name == "zero":
                feat[3, 1] = 0
            call = dict(kw)
            if mode == 1:
                call["labels"] = torch.round(kw["labels"])      # rint: half to even, as rintf
            l64, g64, gap = gaps(ref, feat, norm, **call)
            d[f"{name}_feat"] = feat.numpy().astype(np.float32)
            for k in ("labels", "mask"):
                if k in kw:
                    d[f"{name}_{k}"] = kw[k].numpy().astype(np.float32)
            d[f"{name}_opts"] = np.array([kw.get("temperature", 0.07), 0.07, kw.get("contrast_mode", "all") == "all", norm, mode],
                                         dtype=np.float64)
            d[f"{name}_value"] = np.float64(l64)
            d[f"{name}_grad"] = g64.numpy()
            d[f"{name}_gap"] = gap
            print(f"{name:8s} value {float(l64):.9f}  gaps: value {gap[0]:.2e} grad max {gap[1]:.2e} rel-norm {gap[2]:.2e}  "
                  f"max|g| {float(g64.abs().max()):.3e}")
        feat = torch.randn(512, 2, 64, generator=g)
        l64, g64, gap = gaps(ref, feat, True, labels=ri(7, 512))
        d["n1024_gap"] = np.concatenate([gap, [abs(float(l64)), float(g64.abs().max())]])
        print("n1024    gaps", d["n1024_gap"])
    finally:
        torch.Tensor.cuda = real_cuda
    path = os.path.join(OUT, "supcon.npz")
    np.savez_compressed(path, **d)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
