"""The regression criteria of the fused step (sdumc_step_cfg.regress: L1 / Huber / CCC beside MSE) as closed forms in float64:
value and the gradient to the prediction, for the tests of sdumc_reg_fwd_bwd, the drop-in modules and the step.  torch only, no
autograd (tests/test_regress_cpu.py holds these forms to torch's autograd and to tests/golden/reg_losses.npz).

    value, dpred = reg_ref(name, pred, target, denom=None, weight=1.0, delta=1.0)

pred / target: tensors of one element count (any shape, any float dtype; taken as flat float64).  denom: B_global (None: the element
count).  d_i = p_i - y_i.
    'mse'    sum d_i^2 / denom                                  2 w d_i / denom
    'l1'     sum |d_i| / denom                                  w sign(d_i) / denom            (sign(0) = 0, NaN stays NaN)
    'huber'  sum h_i / denom, h_i = 0.5 d_i^2 (|d_i| <= delta)   w g_i / denom, g_i = d_i or delta sign(d_i)
                              or delta (|d_i| - 0.5 delta)
    'ccc'    1 - N / D, N = 2 s_py, D = s_pp + s_yy + (m_p - m_y)^2, population moments (/ n)
             dN_i = 2 (y_i - m_y) / n, dD_i = 2 (p_i - m_p) / n + 2 (m_p - m_y) / n,  w (-(dN_i D - N dD_i) / D^2)
"""
import torch

NAMES = ("mse", "l1", "huber", "ccc")


def sign(d):
    """sign(0) = 0 and a NaN stays a NaN (the forms torch.sign has, written out)"""
    one = torch.ones_like(d)
    return torch.where(d > 0, one, torch.where(d < 0, -one, torch.where(d == d, torch.zeros_like(d), d)))


def reg_terms(name, pred, target, delta=1.0):
    """the element terms h_i (non-negative; 'l1' / 'huber' / 'mse') in float64: what the value sums"""
    d = pred.detach().double().reshape(-1) - target.detach().double().reshape(-1)
    if name == "mse":
        return d * d
    if name == "l1":
        return d.abs()
    if name == "huber":
        return torch.where(d.abs() <= delta, 0.5 * d * d, delta * (d.abs() - 0.5 * delta))
    raise ValueError(name)


def reg_ref(name, pred, target, denom=None, weight=1.0, delta=1.0):
    p = pred.detach().double().reshape(-1)
    y = target.detach().double().reshape(-1)
    n = p.numel()
    denom = float(n if denom is None else denom)
    d = p - y
    if name == "ccc":
        mp, my = p.sum() / n, y.sum() / n
        a, b = p - mp, y - my
        spp, syy, spy = (a * a).sum() / n, (b * b).sum() / n, (a * b).sum() / n
        dm = mp - my
        D, N = spp + syy + dm * dm, 2.0 * spy
        dN = 2.0 * b / n
        dD = 2.0 * a / n + 2.0 * dm / n
        return 1.0 - N / D, weight * (-(dN * D - N * dD) / (D * D))
    value = reg_terms(name, p, y, delta).sum() / denom
    if name == "mse":
        g = 2.0 * d
    elif name == "l1":
        g = sign(d)
    else:
        g = torch.where(d.abs() <= delta, d, delta * sign(d))
    return value, weight * g / denom
