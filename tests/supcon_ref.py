"""SupConLoss (the reference's toolkit/utils/loss.py:143-240) restated in float64 torch, one anchor at a time: what the
HIP kernel is compared with where no recorded fixture exists.  tests/test_supcon_cpu.py pins it to the fixture recorded
from the reference itself (every value and gradient to 1e-12)."""
import torch


def positives(bsz, labels=None, mask=None, label_mode=0):
    """[bsz, bsz] float64 weights: sample j among the positives of sample i."""
    if labels is not None and mask is not None:
        raise ValueError("labels and mask both given")
    if mask is not None:
        return mask.double()
    if labels is None:
        return torch.eye(bsz, dtype=torch.float64)
    y = labels.reshape(-1)
    if label_mode == 1:
        y = torch.round(y)      # half to even, like rintf
    return (y[:, None] == y[None, :]).double()


def supcon(features, labels=None, mask=None, temperature=0.07, base_temperature=0.07, contrast_mode="all", normalize=False,
           label_mode=0):
    """features [bsz, n_views, D] (any float dtype; computed in float64, differentiable) -> 0-dim float64 value."""
    bsz, views = features.shape[0], features.shape[1]
    x = features.double().reshape(bsz, views, -1)
    if normalize:
        x = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    rows = x.transpose(0, 1).reshape(bsz * views, -1)      # view-major: row v * bsz + b
    n = bsz * views
    anchors = n if contrast_mode == "all" else bsz
    pos = positives(bsz, None if labels is None else labels.to(features.device), mask, label_mode).to(features.device)
    total = x.new_zeros(())
    for i in range(anchors):
        logit = rows @ rows[i] / temperature
        logit = logit - logit.max().detach()               # the maximum runs over every column, the anchor's own too
        others = torch.ones(n, dtype=torch.bool, device=x.device)
        others[i] = False
        log_prob = logit - torch.log(torch.exp(logit[others]).sum())
        w = pos[i % bsz].repeat(views) * others            # the anchor is no positive of itself
        count = w.sum()
        total = total + (w * log_prob).sum() / (count if count >= 1e-6 else 1.0)
    return -(temperature / base_temperature) * total / anchors


def value_and_grad(features, **kw):
    f = features.detach().double().clone().requires_grad_()      # (a float32 leaf would round its gradient)
    v = supcon(f, **kw)
    v.backward()
    return v.detach(), f.grad.double()
