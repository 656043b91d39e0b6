"""Rounding-error bars of loss.hip's Rank-N-Contrast kernels, element by element, from the float64 reference's own intermediates
(oracle/rnc_reference.py).  Shared by the CPU test that keeps the bars honest and the GPU tests that apply them; no fixtures here.

The rule is the one of tests/test_gpu_elementwise.py: a sum of n rounded fp32 operations is off by at most n * u * sum|terms|,
u = 2^-24, to first order.  n is counted from the loop lengths of the kernels -- dim for a squared distance, n for a denominator
D_ik or a window sum S_ij (a serial loop in the direct kernel; prefix + suffix of block scans in the sorted one, never more than
n additions deep), n for the final df sum -- plus a stated allowance per library call: sqrtf and division 1 ulp (2u; both are
correctly rounded in this build, 1 ulp leaves room), expf and logf 2 ulp (4u).  Nothing here was tuned against a device result.

  dist_ij      s = sum_c (f_ic - f_jc)^2: u on each difference (2u on its square), u on the product, dim additions of
               non-negative terms: (dim + 3) u on s, half of that after the square root, + 1 ulp:
                   |err dist| <= E_dist * dist,   E_dist = (dim / 2 + 3) u.           dist = 0 (equal rows, diagonal): exact.
  l_ij = -dist_ij / t   1/t rounded once, the product once:   |err l| <= |l| (E_dist + 2u).  The row maximum is l_ii = 0: exact.
  e_ij = expf(l_ij)     relative E_e[j] = |l_ij| (E_dist + 2u) + 4u.
  D_ik                  a sum of at most n non-negative e_ij:   relative E_D = max_j E_e[j] + n u.
  rowloss_i = sum_{k != i} (l_ik - logf(D_ik))   per term |l_ik| (E_dist + 2u) + E_D + 4u |log D_ik| + u |term|; every term is
               <= 0 (k is a member of its own set: D_ik >= e_ik), so the n-term sum adds n u |rowloss_i|.
  G_ij = -c (1 - x),  x = e_ij S_ij,  S_ij = sum_k [member] (1 / D_ik)
               1 / D_ik: E_D + 2u;  the window sum: + n u  ->  E_S = E_D + (n + 2) u;  x: E_e[j] + E_S + u;  the subtraction, c =
               1 / (n (n - 1)) (n (n - 1) < 2^24 is exact in fp32, its reciprocal rounded once) and the product: 4u |G_ij|:
                   |err G_ij| <= c x (E_e[j] + E_S + u) + 4u |G_ij|.                  G_ii = 0 exactly.
  df_ic = -(w / t) sum_j T_j,  T_j = (G_ij + G_ji) (f_ic - f_jc) / dist_ij
               the errors of G_ij and G_ji enter through |f_ic - f_jc| / dist_ij;  T_j itself: E_dist of the divisor + 5u (the sum of
               the two G, the division, the difference, the product, one spare);  the n-term sum and the two scale factors:
               (n + 3) u sum_j |T_j|."""
import numpy as np
import torch

U = 2.0 ** -24


def rnc_row_bars(ref, dim, temperature):
    """(bar_dist, bar_rowloss, bar_G) for the rows of `ref` (an oracle.rnc_reference.RncRef), shapes as ref.dist / ref.rowloss / ref.G."""
    n = ref.dist.shape[1]
    t = float(temperature)
    c = 1.0 / (n * (n - 1))
    e_dist = (dim / 2 + 3) * U
    logit = -ref.dist / t
    e_e = logit.abs() * (e_dist + 2 * U) + 4 * U                     # [rows, n]
    e_D = e_e.max(dim=1, keepdim=True)[0] + n * U                    # [rows, 1]
    logD = torch.log(ref.D)
    term = logit - logD
    diag = torch.zeros_like(ref.dist, dtype=torch.bool)
    diag[torch.arange(len(ref.rows)), torch.tensor(ref.rows)] = True
    per = logit.abs() * (e_dist + 2 * U) + e_D + 4 * U * logD.abs() + U * term.abs()
    per = per.masked_fill(diag, 0.0)
    term = term.masked_fill(diag, 0.0)
    bar_rowloss = per.sum(1) + n * U * term.abs().sum(1)
    x = torch.exp(logit) * ref.S
    e_S = e_D + (n + 2) * U
    bar_G = (c * x * (e_e + e_S + U) + 4 * U * ref.G.abs()).masked_fill(diag, 0.0)
    return e_dist * ref.dist, bar_rowloss, bar_G


def rnc_loss_bar(ref, bar_rowloss):
    """loss = -sum_i rowloss_i / (n (n - 1)) in fp32 against the float64 sum of the reference's rowloss: the rows' own bars, n u for
    the n-term sum, 4u for the negation-free scale (two conversions, one product, one division)."""
    n = ref.dist.shape[1]
    c = 1.0 / (n * (n - 1))
    return float(c * (bar_rowloss.sum() + n * U * ref.rowloss.abs().sum()) + 4 * U * abs(float(ref.loss)))


def rnc_df_ref_and_bar(G, dist, bar_G, feats64, rows, temperature, weight):
    """(df, bar) in float64 for the rows `rows` of df, from the FULL [n, n] G and dist: df_ic = -(w / t) sum_j T_j as above, w the fp32
    value of `weight`.  bar_G: the full matrix of the bars of G, or None when df is judged against the device's own G and dist (then
    only the rounding of the df kernel itself is left).  Rows go through in chunks: [rows, n, dim] in float64 is large at n = 1024."""
    t, w = float(temperature), float(np.float32(weight))
    n, dim = feats64.shape
    e_dist = (dim / 2 + 3) * U
    df, bar = [], []
    for r0 in range(0, len(rows), 32):
        rt = torch.tensor(rows[r0:r0 + 32])
        d = dist[rt]                                                 # [r, n]
        pos = d > 0
        coef = torch.where(pos, (G[rt] + G[:, rt].t()) / d, torch.zeros_like(d))
        delta = feats64[rt][:, None, :] - feats64[None, :, :]       # [r, n, dim]
        T = coef[:, :, None] * delta
        mag = (w / t) * T.abs().sum(1)
        b = (e_dist + 5 * U + (n + 3) * U) * mag
        if bar_G is not None:
            gain = torch.where(pos, (bar_G[rt] + bar_G[:, rt].t()) / d, torch.zeros_like(d))
            b = b + (w / t) * (gain[:, :, None] * delta.abs()).sum(1)
        df.append(-(w / t) * T.sum(1))
        bar.append(b)
    return torch.cat(df), torch.cat(bar)


LABEL_KINDS = ("cont", "ties", "equal", "straddle")


def rnc_case(n, dim, kind, temperature, dup=False, spread=2.0):
    """Deterministic inputs of one Rank-N-Contrast case: feats [n, dim] fp32 scaled so that the largest dist / temperature is `spread`
    (every exp term then matters in its sum), labels [n] fp32.  For even n the labels are one half repeated, as the training step's
    are, so the same case runs through the _rep entry point.  kind: continuous | 7 distinct values | all equal | straddle = round(y, 1) +
    m * 5e-5, m in 0..3 (differences of 5e-5, 1e-4 and 1.5e-4 next to the 1e-4 threshold, where the fp32 subtraction decides).
    dup: rows 1 and 2 identical, and row 0 identical to row n/2 (one sample whose two views coincide): dist = 0 off the diagonal."""
    g = torch.Generator().manual_seed(1000 * n + 10 * dim + LABEL_KINDS.index(kind) + (5 if dup else 0))
    f = torch.randn(n, dim, generator=g)
    half = n // 2 if n % 2 == 0 else n
    y = torch.rand(half, generator=g) * 6 - 3
    if kind == "ties":
        y = y.round()
    elif kind == "equal":
        y = torch.full((half,), 1.3)
    elif kind == "straddle":
        m = torch.randint(0, 4, (half,), generator=g).float()
        y = y.round(decimals=1) + m * 5e-5
    if half != n:
        y = y.repeat(2)
    if dup and n >= 4:
        f[2] = f[1]
        f[n // 2] = f[0]
    dmax = float(torch.cdist(f.double(), f.double()).max())
    f = (f * (spread * float(temperature) / dmax)).contiguous()
    return f, y.float().contiguous()
