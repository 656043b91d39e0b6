"""References of decoupled weight decay (sdumc_adamw_step, sdumc_adamw_multi, sdumc_amd.optim.AdamW, TrainStep(decoupled_decay=True)),
next to tests/ema_ref.py.  Everything here is torch's own: torch.optim.AdamW in fp64 is the truth, torch.optim.AdamW in fp32
(foreach=False, one parameter) gives the error e32 that fp32 arithmetic makes on the same inputs, and the coupled torch.optim.Adam
in fp32 shows how far the rule the step had before lies from that truth.

THE BAR of the tests against torch: max |ours - AdamW fp64| <= 2 * e32, e32 = max |AdamW fp32 - AdamW fp64| on the same inputs.  The
factor 2 is the margin test_semantics_against_torch_adam_in_float64 already gives this project's Adam: our step rounds where torch's
does (the decay multiply, the moments, the quotient, the final subtraction) plus one fused product and bias corrections that are held
in fp32 (torch keeps them as Python doubles), each of which moves a result by a fraction of the ulp that e32 is made of.

Inputs (CPU, seeded): N = 40 000, p = +-2^U(-4, 4), g = N(0, 1) * 2^U(-6, 2), five steps under a LambdaLR that warms up over three
steps and halves at the fifth; (lr, weight_decay) in CASES."""
import numpy as np
import torch

N, STEPS = 40000, 5
CASES = ((1e-3, 1e-2), (1e-4, 1e-2), (1e-2, 0.1))


def lr_lambda(e):
    """warm-up over three steps, one step down at the fifth: 1/3, 2/3, 1, 1, 1/2"""
    return min(1.0, (e + 1) / 3.0) * (0.5 if e >= 4 else 1.0)


def inputs(seed=2024):
    """-> (p fp32 [N], [g fp32 [N]] * STEPS), CPU tensors that nobody writes to"""
    gen = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, (N,), generator=gen) * 2.0 - 1.0
    p = (sign * torch.exp2(torch.rand(N, generator=gen) * 8 - 4)).float()
    grads = [(torch.randn(N, generator=gen) * torch.exp2(torch.rand(N, generator=gen) * 8 - 6)).float() for _ in range(STEPS)]
    return p, grads


def torch_run(cls, dtype, p, grads, lr, wd, state=None, **kw):
    """`cls` (torch.optim.AdamW or Adam) over ONE parameter, a step per gradient under LambdaLR(lr_lambda): -> (parameter, optimizer).
    state: a state_dict to load before the first step (the scheduler then continues from the loaded step count)."""
    q = torch.nn.Parameter(p.detach().to(dtype).clone())
    opt = cls([q], lr=lr, weight_decay=wd, foreach=False, **kw)
    e0 = 0
    if state is not None:
        opt.load_state_dict(state)
        e0 = int(float(next(iter(opt.state_dict()["state"].values()))["step"]))
    for e, g in enumerate(grads):
        for group in opt.param_groups:      # (what LambdaLR writes: initial lr times the factor, as a Python double)
            group["lr"] = lr * lr_lambda(e0 + e)
        q.grad = g.detach().to(dtype).clone()
        opt.step()
    return q.detach(), opt


def references(p, grads, lr, wd):
    """-> (AdamW fp64 result, e32, distance of the coupled fp32 Adam from the AdamW fp64 result)"""
    p64, _ = torch_run(torch.optim.AdamW, torch.float64, p, grads, lr, wd)
    p32, _ = torch_run(torch.optim.AdamW, torch.float32, p, grads, lr, wd)
    c32, _ = torch_run(torch.optim.Adam, torch.float32, p, grads, lr, wd)
    return p64, float((p32.double() - p64).abs().max()), float((c32.double() - p64).abs().max())


def decay_factor(lr, wd, lr_scale=1.0, wd_scale=1.0):
    """dk of sdumc_adamw_step as an fp32 value: the four fp32 factors multiplied in double, pair by pair, the difference rounded once"""
    f = lambda x: float(np.float32(x))      # noqa: E731
    return np.float32(1.0 - (f(lr) * f(lr_scale)) * (f(wd) * f(wd_scale)))
