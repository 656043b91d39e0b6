#!/usr/bin/env python
"""Generate tests/golden/reg_losses.npz: the regression criteria of the fused step (regress = 'l1' | 'huber' | 'ccc') from torch's own
classes and autograd in float64, on the CPU.

    python tests/golden/make_reg_goldens.py

torch.nn.L1Loss / torch.nn.HuberLoss(delta) with reduction='sum', divided by len(pred) (the reduction of the reference's MSELoss,
toolkit/utils/loss.py:19-33), and 1 - the concordance correlation coefficient written in torch ops with population moments.  Inputs
are recorded as the fp32 values the kernels get; values and gradients are float64 results on exactly those inputs.  Data only
(np.savez_compressed, loadable with allow_pickle=False), a few KB.

Cases (C = l1 | huber | ccc; huber's delta is 1.0 unless the key says otherwise):
  pred [16,1], target [16]          drawn like the step's: labels U(-3, 3), predictions = labels + noise
  C, C_dpred, huber025(_dpred)      value and gradient on them (huber025: delta = 0.25)
  C_gap                             [value, gradient] max |fp32 - fp64| of the same torch expression: what fp32 resolves there
  edge_T_pred / _target, T = d025 | d100 (delta = 0.25 | 1.0): rows with d = pred - target exactly 0 (twice: at 0 and at 1.5),
                                    +-delta, +-(delta + 1 ulp), +-(delta - 1 ulp) in fp32, +-2.5;  edge_T_C, edge_T_C_dpred
  const_pred / _target              all predictions equal (CCC: s_pp = 0, D > 0);  const_C, const_C_dpred
  one_pred / _target                rows = 1;  one_C, one_C_dpred  (CCC: value 1, gradient 0)
"""
import os

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
CRITERIA = ("l1", "huber", "ccc")


def ccc(p, y):
    p, y = p.reshape(-1), y.reshape(-1)
    mp, my = p.mean(), y.mean()
    spp, syy, spy = ((p - mp) ** 2).mean(), ((y - my) ** 2).mean(), ((p - mp) * (y - my)).mean()
    return 1 - 2 * spy / (spp + syy + (mp - my) ** 2)


def criterion(name, delta=1.0):
    if name == "l1":
        return lambda p, y: torch.nn.L1Loss(reduction="sum")(p.reshape(-1), y.reshape(-1)) / len(p)
    if name == "huber":
        return lambda p, y: torch.nn.HuberLoss(reduction="sum", delta=delta)(p.reshape(-1), y.reshape(-1)) / len(p)
    return ccc


def run(fn, pred, target, dtype=torch.float64):
    p = pred.to(dtype).clone().requires_grad_()
    l = fn(p, target.to(dtype))
    l.backward()
    return l.detach(), p.grad


def record(d, prefix, name, fn, pred, target):
    l, dp = run(fn, pred, target)
    d[f"{prefix}{name}"] = np.asarray(l.numpy(), dtype=np.float64)
    d[f"{prefix}{name}_dpred"] = dp.numpy().astype(np.float64)
    return l, dp


def main():
    g = torch.Generator().manual_seed(20241021)
    d = {}
    B = 16
    target = torch.rand(B, generator=g) * 6 - 3
    pred = (target + 0.8 * torch.randn(B, generator=g)).reshape(B, 1)
    d.update(pred=pred.numpy(), target=target.numpy())
    for name in CRITERIA:
        fn = criterion(name)
        l64, g64 = record(d, "", name, fn, pred, target)
        l32, g32 = run(fn, pred, target, torch.float32)
        d[f"{name}_gap"] = np.array([float((l32.double() - l64).abs()), float((g32.double() - g64).abs().max())])
        print(name, "value", float(l64), "fp32-fp64 gap of the value", d[f"{name}_gap"][0], "of the gradient", d[f"{name}_gap"][1])
    record(d, "", "huber025", criterion("huber", 0.25), pred, target)
    # edge rows: d = pred - target exact in fp32 (target 0, or pred == target)
    for tag, delta in (("d025", 0.25), ("d100", 1.0)):
        dl = np.float32(delta)
        up, dn = np.nextafter(dl, np.float32(np.inf)), np.nextafter(dl, np.float32(0))
        dd = np.array([0, 0, dl, -dl, up, -up, dn, -dn, 2.5, -2.5], dtype=np.float32)
        t = np.zeros_like(dd)
        t[1] = 1.5
        p = (t + dd).astype(np.float32)
        assert np.array_equal(p - t, dd)
        ep, et = torch.from_numpy(p).reshape(-1, 1), torch.from_numpy(t)
        d[f"edge_{tag}_pred"], d[f"edge_{tag}_target"] = ep.numpy(), et.numpy()
        for name in CRITERIA:
            record(d, f"edge_{tag}_", name, criterion(name, delta), ep, et)
    d["edge_deltas"] = np.array([0.25, 1.0])
    # all predictions equal
    ct = torch.rand(B, generator=g) * 6 - 3
    cp = torch.full((B, 1), 0.7)
    d.update(const_pred=cp.numpy(), const_target=ct.numpy())
    for name in CRITERIA:
        record(d, "const_", name, criterion(name), cp, ct)
    # rows = 1
    op, ot = torch.tensor([[0.3]]), torch.tensor([-1.1])
    d.update(one_pred=op.numpy(), one_target=ot.numpy())
    for name in CRITERIA:
        record(d, "one_", name, criterion(name), op, ot)
    path = os.path.join(OUT, "reg_losses.npz")
    np.savez_compressed(path, **d)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
