#!/usr/bin/env python
"""Generate tests/golden/distill_losses.npz from the REAL reference's loss classes.

    python tests/golden/make_distill_goldens.py <path of the reference checkout>

Imports toolkit/utils/loss.py of the reference by path (never copies it), runs CosineSimilarityLoss4Seq (:100-119),
KLLoss (:74-97) and CELoss (:6-16) on the CPU in fp32 with torch autograd, and records inputs, values and the
gradients to both arguments.  Data only (np.savez_compressed, loadable with allow_pickle=False).

Cases (B = 16, the shapes of the step's three distillation pairs):
  {th,ct,z}_{a,b}      [16,256], [16,7,128], [16,128]    seeded normal inputs, b = a + noise
  {cos,kl}_{th,ct,z}   value, _da / _db gradients of the two criteria on them
  ce                   [16,4] logits + integer targets
  cos_edge             [4,128]: row 0 a = 0, row 1 b = 0, row 2 a == b, row 3 ordinary
  kl_edge              [4,128]: row 0 a == b, row 1 logits of a spread over +-30, row 2 both spread, row 3 ordinary
  kl_edge_gap          max |fp32 - fp64| of the reference's own gradient on kl_edge (what fp32 resolves there)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))


def load_reference_losses(ref):
    spec = importlib.util.spec_from_file_location("ref_toolkit_loss", os.path.join(ref, "toolkit", "utils", "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def np32(t):
    return t.detach().numpy().astype(np.float32)


def run(fn, a, b, dtype=torch.float32):
    a = a.to(dtype).clone().requires_grad_()
    b = b.to(dtype).clone().requires_grad_()
    l = fn(a, b)
    l.backward()
    return l.detach(), a.grad, b.grad


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference_losses(sys.argv[1])
    cos, kl, ce = ref.CosineSimilarityLoss4Seq(), ref.KLLoss(), ref.CELoss()
    g = torch.Generator().manual_seed(20240607)
    B = 16
    d = {}
    shapes = {"th": (B, 256), "ct": (B, 7, 128), "z": (B, 128)}
    for tag, shape in shapes.items():
        a = torch.randn(*shape, generator=g)
        b = a + 0.5 * torch.randn(*shape, generator=g)      # teacher and student are correlated, as in the step
        d.update({f"{tag}_a": np32(a), f"{tag}_b": np32(b)})      # (both criteria read the same inputs)
        for name, fn in (("cos", cos), ("kl", kl)):
            l, da, db = run(fn, a, b)
            d.update({f"{name}_{tag}": np32(l), f"{name}_{tag}_da": np32(da), f"{name}_{tag}_db": np32(db)})
    # CE
    logits = torch.randn(B, 4, generator=g) * 2
    target = torch.randint(0, 4, (B,), generator=g)
    x = logits.clone().requires_grad_()
    l = ce(x, target)
    l.backward()
    d.update({"ce_logits": np32(logits), "ce_target": target.numpy().astype(np.int64), "ce": np32(l), "ce_dlogits": np32(x.grad)})
    # edge rows
    a = torch.randn(4, 128, generator=g)
    b = torch.randn(4, 128, generator=g)
    a[0] = 0
    b[1] = 0
    b[2] = a[2]
    l, da, db = run(cos, a, b)
    d.update({"cos_edge_a": np32(a), "cos_edge_b": np32(b), "cos_edge": np32(l), "cos_edge_da": np32(da), "cos_edge_db": np32(db)})
    a = torch.randn(4, 128, generator=g)
    b = torch.randn(4, 128, generator=g)
    b[0] = a[0]
    a[1] = torch.linspace(-30, 30, 128)[torch.randperm(128, generator=g)]
    a[2] = torch.linspace(-30, 30, 128)[torch.randperm(128, generator=g)]
    b[2] = torch.linspace(-30, 30, 128)[torch.randperm(128, generator=g)]
    l, da, db = run(kl, a, b)
    l64, da64, db64 = run(kl, a, b, torch.float64)
    gap = max(float((da.double() - da64).abs().max()), float((db.double() - db64).abs().max()))
    vgap = float((l.double() - l64).abs())
    d.update({"kl_edge_a": np32(a), "kl_edge_b": np32(b), "kl_edge": np32(l), "kl_edge_da": np32(da), "kl_edge_db": np32(db),
              "kl_edge_gap": np.array([vgap, gap])})
    print("kl_edge: value", float(l), "fp32-fp64 gap of the value", vgap, "of the gradients", gap,
          "max |gradient|", float(da64.abs().max()), float(db64.abs().max()))
    path = os.path.join(OUT, "distill_losses.npz")
    np.savez_compressed(path, **d)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
