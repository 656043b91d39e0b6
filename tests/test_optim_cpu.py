"""CPU-only: the drop-in optimizer's binding, ABI mirrors, constructor contract and checkpoint interchange
(sdumc_amd/optim.py, sdumc_adam_multi).  What needs a device is in tests/test_gpu_optim.py."""
import ctypes as C
import os
import subprocess
import tempfile
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_sizes(exprs):
    """The host C compiler's value of each expression with include/sdumc_hip.h in scope."""
    fmt = " ".join(["%zu"] * len(exprs))
    src = ('#include <stdio.h>\n#include "sdumc_hip.h"\nint main(void){printf("%s\\n", %s); return 0;}\n'
           % (fmt, ", ".join("(size_t)(%s)" % e for e in exprs)))
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "t.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "t.c"), "-o", os.path.join(td, "t")])
        return [int(v) for v in subprocess.check_output([os.path.join(td, "t")]).split()]


def test_module_imports_and_entry_point_is_bound():
    import sdumc_amd.optim as optim
    from sdumc_amd import _lib, ops
    assert issubclass(optim.Adam, torch.optim.Optimizer)
    fn = _lib.lib.sdumc_adam_multi
    assert fn.restype is C.c_int and len(fn.argtypes) == 12
    assert "sdumc_adam_multi" in _lib.EXPORTS and callable(ops.adam_multi)
    # bad arguments come back as error codes before anything is launched (no device is touched)
    seg = (_lib.AdamSeg * 1)()
    assert fn(None, 1, 16, 16, 4, 16, 0.9, 0.999, 1e-8, 0.0, 1.0, None) == -1
    assert fn(seg, 0, 16, 16, 4, 16, 0.9, 0.999, 1e-8, 0.0, 1.0, None) == -1          # empty table
    assert fn(seg, 1, 16, 16, 4, 16, 0.9, 0.999, 1e-8, 0.0, 1.0, None) == -1          # null param / grad
    seg[0].param, seg[0].grad, seg[0].state_offset, seg[0].n = 16, 16, 0, 0
    assert fn(seg, 1, 16, 16, 4, 16, 0.9, 0.999, 1e-8, 0.0, 1.0, None) == -1          # n <= 0
    seg[0].state_offset, seg[0].n = 2, 3
    assert fn(seg, 1, 16, 16, 4, 16, 0.9, 0.999, 1e-8, 0.0, 1.0, None) == -1          # state_offset + n > state_len
    seg[0].state_offset, seg[0].n = 0, 4
    assert fn(seg, 1, None, 16, 4, 16, 0.9, 0.999, 1e-8, 0.0, 1.0, None) == -1         # null moments
    assert fn(seg, 1, 16, 16, 4, None, 0.9, 0.999, 1e-8, 0.0, 1.0, None) == -1         # null hyper


def test_struct_sizes_and_table_capacity_match_the_header():
    from sdumc_amd import _lib
    seg, table, cap, chunk = _c_sizes(["sizeof(sdumc_adam_seg)", "sizeof(sdumc_adam_table)", "SDUMC_ADAM_MAX_SEGS",
                                       "SDUMC_ADAM_CHUNK"])
    assert C.sizeof(_lib.AdamSeg) == seg and C.sizeof(_lib.AdamTable) == table
    assert cap == _lib.ADAM_MAX_SEGS and chunk == 1024
    # the table travels by value in the kernel arguments: HIP's 4 KB limit, and this model's 81 tensors in one launch
    assert table <= 4096 and cap >= 81
    assert table + 7 * 8 <= 4096                                   # ... together with the launch's other arguments


def _params(n=3):
    return [torch.nn.Parameter(torch.zeros(4 + i)) for i in range(n)]


def test_constructor_contract():
    from sdumc_amd.optim import Adam
    from sdumc_amd._lib import SdumcError
    for kw in ({"amsgrad": True}, {"maximize": True}, {"capturable": True}, {"differentiable": True}):
        with pytest.raises(SdumcError):
            Adam(_params(), **kw)
    a, b = _params(2)
    with pytest.raises(SdumcError):
        Adam([{"params": [a]}, {"params": [b], "lr": 1e-2}])
    opt = Adam(_params(), lr=1e-4, weight_decay=1e-5, foreach=True, fused=False)      # accepted and ignored
    with pytest.raises(SdumcError):
        opt.add_param_group({"params": _params(1)})
    ref = torch.optim.Adam(_params(), lr=1e-4, weight_decay=1e-5)
    g, rg = opt.param_groups[0], ref.param_groups[0]
    assert set(g) == set(rg)
    assert all(g[k] == rg[k] for k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "capturable",
                                       "differentiable"))
    # positional order of torch.optim.Adam: (params, lr, betas, eps, weight_decay, amsgrad)
    opt = Adam(_params(), 3e-4, (0.8, 0.9), 1e-6, 1e-2, False)
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (3e-4, (0.8, 0.9), 1e-6, 1e-2)
    assert opt.state_dict()["state"] == {}
    # LambdaLR drives it like any torch optimizer
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: 0.5 ** e)
    assert opt.param_groups[0]["lr"] == 3e-4 and sched.get_last_lr() == [3e-4]


def test_step_on_cpu_parameters_raises():
    from sdumc_amd.optim import Adam
    from sdumc_amd._lib import SdumcError
    ps = _params()
    opt = Adam(ps, lr=1e-3)
    assert opt.step() is None                       # no gradients yet: nothing to do, as in torch
    for p in ps:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(SdumcError):
        opt.step()
    assert all(torch.equal(p.detach(), b) for p, b in zip(ps, before)) and not opt.state_dict()["state"]
    half = [torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))]
    half[0].grad = torch.ones_like(half[0])
    with pytest.raises(SdumcError):
        Adam(half).step()


def test_load_state_dict_before_the_first_step_roundtrips_the_fused_steps_state():
    """Resume: checkpoint.adam_state_from_flat(...) -> load_state_dict on an unstepped optimizer -> state_dict()."""
    from sdumc_amd import checkpoint as ck
    from sdumc_amd.model import get_models
    from sdumc_amd.optim import Adam
    from sdumc_amd._lib import SdumcError
    torch.manual_seed(3)
    model = get_models(types.SimpleNamespace(input_dims=(16, 8, 12, 8), model="wengnet_mosei_mult_views_text_missing"))
    net = model.model
    m = torch.arange(net._layout.live, dtype=torch.float32) * 1e-6
    v = torch.arange(net._layout.live, dtype=torch.float32) * 1e-9
    src = ck.adam_state_from_flat(net, m, v, step=7, lr=2e-4)
    opt = Adam(model.parameters(), lr=1e-4, weight_decay=1e-5)
    opt.load_state_dict(src)
    out = opt.state_dict()
    assert out["param_groups"] == src["param_groups"] and opt.param_groups[0]["lr"] == 2e-4
    assert set(out["state"]) == set(src["state"]) and len(out["state"]) == len(net._live_names)
    for i, st in src["state"].items():
        got = out["state"][i]
        assert set(got) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(got["step"]) == 7.0 and got["step"].dtype == st["step"].dtype
        assert torch.equal(got["exp_avg"], st["exp_avg"]) and torch.equal(got["exp_avg_sq"], st["exp_avg_sq"])
    steps = [st["step"] for st in out["state"].values()]
    assert len({t.data_ptr() for t in steps}) == len(steps)       # one tensor per parameter: nothing aliased for a per-parameter counter
    torch.optim.Adam(model.parameters(), lr=1e-4).load_state_dict(out)       # torch accepts it
    m2, v2, step = ck.flat_from_adam_state(net, out, "cpu")
    assert step == 7
    for name in net._layout.live_names():
        off, shape, _ = net._layout.entries[name]
        n = 1
        for s in shape:
            n *= s
        assert torch.equal(m2[off:off + n], m[off:off + n]) and torch.equal(v2[off:off + n], v[off:off + n]), name
    # one shared step count: a state whose parameters disagree on it is refused
    bad = ck.adam_state_from_flat(net, m, v, step=7)
    first = next(iter(bad["state"]))
    bad["state"][first]["step"] = torch.tensor(6.0)
    with pytest.raises(SdumcError):
        Adam(model.parameters()).load_state_dict(bad)
