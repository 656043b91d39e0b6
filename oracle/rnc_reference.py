"""Rank-N-Contrast in float64 with its intermediates: the formulas written in sdumc_amd/csrc/loss.hip, one anchor at a time.

    dist_ij    = |f_i - f_j|_2                       e_ij = exp(-dist_ij / t)        (the row maximum is the diagonal's 0)
    member_i(k, j) = j != i and ld_ij >= ld_ik - float32(1e-4)     in FP32 torch: the reference's own operation (loss.py:303)
    D_ik       = sum_j member_i(k, j) e_ij
    rowloss_i  = sum_{k != i} (-dist_ik / t - log D_ik)
    G_ij       = -(1 - e_ij sum_{k != i} member_i(k, j) / D_ik) / (n (n - 1)),   G_ii = 0
    loss       = -sum_i rowloss_i / (n (n - 1))
    df_i       = -(1 / t) sum_j (G_ij + G_ji) (f_i - f_j) / dist_ij              (dist_ij = 0 terms dropped)

One loop over the anchors, all sets of an anchor as one dense 0 / 1 matrix, no sorting: a different algorithm from loss.hip's sorted kernel ON
PURPOSE (and from sdumc_oracle.rnc_loss + autograd, which it is tested against).  Only the label differences and the comparison
are float32; everything else is float64 of the float32 inputs."""
from collections import namedtuple

import torch

RncRef = namedtuple("RncRef", "dist rowloss G loss df D S rows")
RncRef.__doc__ = """dist, rowloss, G: the rows listed in `rows` (all of them without anchors=); loss, df: None with anchors=.
D[a, k] = D_ik and S[a, j] = sum_k member_i(k, j) / D_ik for i = rows[a] (1 resp. 0 on the diagonal): what a caller needs to
bound the rounding error of an fp32 evaluation element by element."""


def rnc_reference(feats_f32, labels_f32, temperature=2.0, anchors=None, flip=None):
    """feats_f32 [n, dim], labels_f32 [n].  anchors: evaluate only these rows of dist / rowloss / G (loss and df need all of them
    and come back None).  flip: {i: (k, j)} inverts member_i(k, j) for those anchors -- for tests that ask whether a comparison
    would notice one wrong membership decision."""
    assert feats_f32.dtype == torch.float32 and labels_f32.dtype == torch.float32
    f = feats_f32.double()
    n, dim = f.shape
    y = labels_f32.reshape(-1)
    assert y.numel() == n and n >= 2
    rows = list(range(n)) if anchors is None else [int(a) for a in anchors]
    t = float(temperature)
    c = 1.0 / (n * (n - 1))
    dist = torch.zeros(len(rows), n, dtype=torch.float64)
    G, D, S = torch.zeros_like(dist), torch.ones_like(dist), torch.zeros_like(dist)
    rowloss = torch.zeros(len(rows), dtype=torch.float64)
    md = torch.empty(n, n, dtype=torch.float64)          # member_i[k, j] as 0.0 / 1.0; row i and column i are taken out below
    for a, i in enumerate(rows):
        d = (f[i] - f).pow(2).sum(1).sqrt()
        d[i] = 0.0
        e = torch.exp(-d / t)
        ld = (y[i] - y).abs()                            # fp32
        thr = ld - 0.0001                                # fp32 tensor - Python scalar: ONE fp32 subtraction of float32(1e-4)
        assert ld.dtype == torch.float32 and thr.dtype == torch.float32
        torch.ge(ld[None, :], thr[:, None], out=md)      # the fp32 comparison, written out as float64 0 / 1
        if flip and i in flip:
            k, j = flip[i]
            assert k != i and j != i
            md[k, j] = 1.0 - md[k, j]
        e_off = e.clone()
        e_off[i] = 0.0                                   # j = i is no member of any set
        Dk = md @ e_off
        Dk[i] = 1.0
        terms = -d / t - torch.log(Dk)
        terms[i] = 0.0
        invD = 1.0 / Dk
        invD[i] = 0.0                                    # k = i is no positive
        Sj = md.t() @ invD
        Sj[i] = 0.0
        g = -c * (1.0 - e * Sj)
        g[i] = 0.0
        dist[a], rowloss[a], G[a], D[a], S[a] = d, terms.sum(), g, Dk, Sj
    if anchors is not None:
        return RncRef(dist, rowloss, G, None, None, D, S, rows)
    loss = -rowloss.sum() * c
    coef = torch.where(dist > 0, (G + G.t()) / dist, torch.zeros_like(dist))
    df = -(1.0 / t) * (coef.sum(1, keepdim=True) * f - coef @ f)
    return RncRef(dist, rowloss, G, loss, df, D, S, rows)


def closest_membership(labels_f32, i):
    """(k, j, margin): the decision member_i(k, j) whose fp32 operands ld_ij and ld_ik - 1e-4 lie closest together."""
    y = labels_f32.reshape(-1).to(torch.float32)
    n = y.numel()
    ld = (y[i] - y).abs()
    thr = ld - 0.0001
    gap = (ld[None, :].double() - thr[:, None].double()).abs()
    gap[:, i] = float("inf")
    gap[i, :] = float("inf")
    p = int(gap.argmin())
    return p // n, p % n, float(gap.reshape(-1)[p])
