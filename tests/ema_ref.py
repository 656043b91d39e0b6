"""Reference of the averaged weights (sdumc_adam_step_ema, sdumc_ema_multi, TrainStep(ema_decay=)), in torch and fp64, next to
tests/supcon_ref.py.  The rule is torch.lerp(a, p, w)'s own, per element, from the fp32 average `a`, the fp32 parameter `p` AFTER
the step's update and the fp32 weight w:
    w <  0.5:  a' = a + w * (p - a)            w >= 0.5:  a' = p - (p - a) * (1 - w)          (1 - w in fp32: exact there)
w = fp32(1 - d_eff) computed in double and rounded once; d_eff = the decay, or with warm-up min(decay, (1 + t) / (10 + t)) with t =
Adam's step count after the step.  The C entry and the fused step take the decay as an fp32 value (sdumc_step_cfg.ema_decay), so
d there is fp32(decay); sdumc_amd.optim.ema_update_ takes a Python double and rounds 1 - decay once, as torch's own
get_ema_multi_avg_fn does.

THE BOUND.  One update from known fp32 a, p and w lies within 2 * 2^-23 * max(|a|, |p|) of the fp64 value of the rule, element by
element: the subtraction and the final add (or fused multiply-add) round once each, a separate multiply once more, and with
|p - a| <= 2 max that is at most 1.5 * 2^-23 * max; 2 leaves room for either contraction.  Where w is 0.25, 0.5 or 1 the product is
exact, the result does not depend on contraction, and the check is bit equality with torch.lerp(a, p, w) in fp32."""
import numpy as np
import torch

ULP = 2.0 ** -23
EXACT_WEIGHTS = (0.25, 0.5, 1.0)


def weight(decay, t=None, warmup=False, fp32_decay=True):
    """the fp32 weight w as a Python float.  fp32_decay: the decay passes through an fp32 argument first (the C entry, the step)"""
    d = float(np.float32(decay)) if fp32_decay else float(decay)
    if warmup:
        d = min(d, (1.0 + float(t)) / (10.0 + float(t)))
    return float(np.float32(1.0 - d))


def lerp64(a, p, w):
    """the rule in fp64 from fp32 a, p and the fp32 weight w -> fp64 tensor"""
    w = float(np.float32(w))
    a, p = a.double(), p.double()
    d = p - a
    return a + w * d if w < 0.5 else p - d * float(np.float32(1.0) - np.float32(w))


def lerp32(a, p, w):
    """torch.lerp in fp32: what the kernels give bit for bit where w is 0.25, 0.5 or 1"""
    return torch.lerp(a, p, float(np.float32(w)))


def bound(a, p):
    return 2.0 * ULP * torch.maximum(a.abs(), p.abs()).double()


def worst(got, a, p, w):
    """max over elements of |got - rule64| / bound (0 where the bound is 0 and the values agree)"""
    err = (got.double() - lerp64(a, p, w)).abs()
    b = bound(a, p)
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max()) if ratio.numel() else 0.0


def check(got, a, p, w, what=""):
    """bit equality with torch.lerp where the product is exact, the bound elsewhere; returns the worst ratio (0.0 for the bit check)"""
    w = float(np.float32(w))
    if w in EXACT_WEIGHTS:
        want = lerp32(a, p, w)
        bad = torch.nonzero(got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).flatten()
        assert bad.numel() == 0, f"{what}: w = {w}: {bad.numel()} of {got.numel()} elements differ from torch.lerp, first at {bad[:8].tolist()}"
        return 0.0
    r = worst(got, a, p, w)
    assert r <= 1.0, f"{what}: w = {w!r}: worst |ema - rule| / (2 * 2^-23 * max(|a|, |p|)) = {r:.4f}"
    return r
