"""CPU-only: the selectable regression criterion (MSE / L1 / Huber / CCC) as far as it shows without a GPU -- the float64 reference of
the GPU tests (tests/reg_ref.py) against torch's autograd and the fixture, the host-side argument checks, the struct mirror, the
three drop-in classes."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests.reg_ref import reg_ref, sign

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
CRITERIA = ("l1", "huber", "ccc")
# a quarter of the GPU bars of tests/test_gpu_regress.py (values 1e-6, gradients 1e-5): the project's rule for references
VAL_BAR, GRAD_BAR = 0.25e-6, 0.25e-5
CASES = (("", 1.0), ("edge_d025_", 0.25), ("edge_d100_", 1.0), ("const_", 1.0), ("one_", 1.0))


def close(got, want, tol, msg):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = max(1.0, np.abs(want).max())
    np.testing.assert_allclose(got, want.reshape(got.shape), rtol=tol, atol=tol * scale, err_msg=msg)


def _torch_form(name, delta):
    if name == "l1":
        return lambda p, y: torch.nn.L1Loss(reduction="sum")(p.reshape(-1), y.reshape(-1)) / len(p)
    if name == "huber":
        return lambda p, y: torch.nn.HuberLoss(reduction="sum", delta=delta)(p.reshape(-1), y.reshape(-1)) / len(p)

    def ccc(p, y):
        p, y = p.reshape(-1), y.reshape(-1)
        mp, my = p.mean(), y.mean()
        return 1 - 2 * ((p - mp) * (y - my)).mean() / (((p - mp) ** 2).mean() + ((y - my) ** 2).mean() + (mp - my) ** 2)
    return ccc


def test_fixture_is_plain_data_and_its_edge_rows_are_what_the_generator_says():
    path = os.path.join(GOLDEN, "reg_losses.npz")
    assert os.path.getsize(path) < 16 << 10
    g = np.load(path, allow_pickle=False)
    assert all(g[k].dtype != object for k in g.files)
    assert g["pred"].shape == (16, 1) and g["target"].shape == (16,) and g["pred"].dtype == np.float32
    assert np.abs(g["target"]).max() <= 3
    for tag, delta in (("d025", 0.25), ("d100", 1.0)):
        d = g[f"edge_{tag}_pred"].reshape(-1) - g[f"edge_{tag}_target"]
        dl = np.float32(delta)
        up, dn = np.nextafter(dl, np.float32(np.inf)), np.nextafter(dl, np.float32(0))
        assert d.dtype == np.float32 and d.tolist() == [0, 0, dl, -dl, up, -up, dn, -dn, 2.5, -2.5]
    assert np.unique(g["const_pred"]).size == 1 and g["one_pred"].shape == (1, 1)
    assert float(g["one_ccc"]) == 1.0 and not g["one_ccc_dpred"].any() and float(g["const_ccc"]) == 1.0
    for name in CRITERIA:
        assert g[f"{name}_gap"].shape == (2,) and g[f"{name}_gap"].max() < 1e-7      # the criteria's own fp32-vs-fp64 gaps


@pytest.mark.parametrize("name", CRITERIA)
def test_reference_forms_against_the_fixture_and_autograd(name):
    g = np.load(os.path.join(GOLDEN, "reg_losses.npz"), allow_pickle=False)
    for pre, delta in CASES:
        pred, target = torch.from_numpy(g[pre + "pred"]), torch.from_numpy(g[pre + "target"])
        v, dp = reg_ref(name, pred, target, denom=len(pred), delta=delta)
        close(v, g[pre + name], VAL_BAR, f"{pre}{name} value")
        for i in range(dp.numel()):      # element by element: one scale for the tensor would let a large element hide the others
            close(dp[i], g[f"{pre}{name}_dpred"].reshape(-1)[i], GRAD_BAR, f"{pre}{name} dpred[{i}]")
    # fresh draws, float64 autograd, a weight and a denom that is not the row count (a data-parallel share)
    gen = torch.Generator().manual_seed(5)
    for rows in (1, 2, 7, 300):
        y = torch.rand(rows, generator=gen, dtype=torch.float64) * 6 - 3
        p = (y + torch.randn(rows, generator=gen, dtype=torch.float64)).requires_grad_()
        for delta in (0.25, 1.0, 3.0):
            denom = rows if name == "ccc" else 2 * rows
            l = _torch_form(name, delta)(p, y) * (1.0 if name == "ccc" else rows / denom)
            p.grad = None
            (0.7 * l).backward()
            v, dp = reg_ref(name, p, y, denom=denom, weight=0.7, delta=delta)
            close(v, l.detach(), VAL_BAR, f"{name} rows {rows} value")
            close(dp, p.grad, GRAD_BAR, f"{name} rows {rows} dpred")
    if name == "huber":
        v, dp = reg_ref("huber", torch.from_numpy(g["pred"]), torch.from_numpy(g["target"]), denom=16, delta=0.25)
        close(v, g["huber025"], VAL_BAR, "huber025 value")
        close(dp, g["huber025_dpred"], GRAD_BAR, "huber025 dpred")


def test_reference_sign_and_nan_rules():
    d = torch.tensor([0.0, -0.0, 2.0, -3.0, float("nan")], dtype=torch.float64)
    s = sign(d)
    assert s[:4].tolist() == [0.0, 0.0, 1.0, -1.0] and math.isnan(float(s[4]))
    for name in CRITERIA:
        v, dp = reg_ref(name, torch.tensor([1.0, float("nan"), 2.0]), torch.tensor([0.5, 0.0, 0.0]))
        assert math.isnan(float(v)) and math.isnan(float(dp[1]))
    v, dp = reg_ref("ccc", torch.full((4,), 0.25), torch.full((4,), 0.25))
    assert math.isnan(float(v)) and bool(torch.isnan(dp).all())      # D == 0: 0/0


def test_regress_args_accepts_and_rejects_on_the_host():
    from sdumc_amd import _lib
    assert _lib.REGRESS == {"mse": 0, "l1": 1, "huber": 2, "ccc": 3}
    assert _lib.regress_args("mse", 1.0) == (0, 1.0) and _lib.regress_args("l1") == (1, 1.0)
    assert _lib.regress_args("huber", 0.25) == (2, 0.25) and _lib.regress_args("huber", 2) == (2, 2.0)
    assert _lib.regress_args("ccc", 1.0) == (3, 1.0)
    for bad in ("nope", "MSE", 1, None, b"l1"):
        with pytest.raises(_lib.SdumcError, match="regress"):
            _lib.regress_args(bad, 1.0)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), True, "1.0", None, torch.tensor(1.0), 1e-60, 1e60):
        with pytest.raises(_lib.SdumcError, match="regress_delta"):
            _lib.regress_args("huber", bad)
    for name in ("mse", "l1", "ccc"):      # a delta beside a criterion that does not read it
        with pytest.raises(_lib.SdumcError, match="regress_delta"):
            _lib.regress_args(name, 0.5)
    assert _lib.REGRESS_ABI is True and "sdumc_reg_fwd_bwd" in _lib.EXPORTS
    assert len(_lib.lib.sdumc_reg_fwd_bwd.argtypes) == 10


def test_step_cfg_mirrors_the_header_and_a_zeroed_struct_is_mse():
    """`regress` in what was padding behind B_global, `regress_delta` in what was the struct's tail padding: no older field moves,
    sizeof stays; the header's codes; a zeroed struct is the MSE step."""
    from sdumc_amd import _lib
    G = _lib.StepCfg
    exprs = ["offsetof(sdumc_step_cfg, regress)", "offsetof(sdumc_step_cfg, regress_delta)", "offsetof(sdumc_step_cfg, B_global)",
             "offsetof(sdumc_step_cfg, ssd_global)", "offsetof(sdumc_step_cfg, distill)", "sizeof(sdumc_step_cfg)",
             "SDUMC_REGRESS_MSE", "SDUMC_REGRESS_L1", "SDUMC_REGRESS_HUBER", "SDUMC_REGRESS_CCC"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sdumc_hip.h"\nint main(void){printf("%s\\n", %s); return 0;}\n'
           % (" ".join(["%zu"] * len(exprs)), ", ".join("(size_t)(%s)" % e for e in exprs)))
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "t.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "t.c"), "-o", os.path.join(td, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(td, "t")]).split()]
    assert got == [G.regress.offset, _lib.REGRESS_DELTA_OFFSET, G.B_global.offset, G.ssd_global.offset, G.distill.offset, C.sizeof(G),
                   0, 1, 2, 3]
    assert G.regress.offset == G.B_global.offset + 4 and G.regress.size == 4 and _lib.REGRESS_DELTA_OFFSET == G.distill.offset + 4
    z = G()
    assert z.regress == 0 == _lib.REGRESS["mse"] and z.regress_delta == 0.0
    z.regress, z.regress_delta, z.distill = 2, 0.25, 1
    raw = bytes(z)
    assert z.regress_delta == 0.25 and z.distill == 1 and z.regress == 2
    assert np.frombuffer(raw, dtype=np.float32)[_lib.REGRESS_DELTA_OFFSET // 4] == 0.25
    assert np.frombuffer(raw, dtype=np.int32)[G.regress.offset // 4] == 2


def test_constructors_refuse_bad_values_before_any_device_work():
    from sdumc_amd import _lib, engine, trainer
    flat = torch.zeros(16)
    dims, T = (64, 32, 48, 32), (21, 5, 13, 4)
    for kw in ({"regress": "nope"}, {"regress": 1}, {"regress": "huber", "regress_delta": 0.0}, {"regress": "l1", "regress_delta": 0.5},
               {"regress": "huber", "regress_delta": float("nan")}):
        with pytest.raises(_lib.SdumcError, match="regress"):
            engine.TrainStep(flat, 4, T, dims, **kw)
        with pytest.raises(_lib.SdumcError, match="regress"):
            engine.FusedTrainer(flat, dims, **kw)
        with pytest.raises(_lib.SdumcError, match="regress"):
            trainer.DataParallelStep(flat, 4, T, dims, **kw)
    with pytest.raises(_lib.SdumcError, match="not built under data parallelism"):
        trainer.DataParallelStep(flat, 4, T, dims, regress="ccc")
    with pytest.raises(_lib.SdumcError, match="not built under data parallelism"):
        trainer.HipBackend(flat, 4, T, dims, engine.DEFAULT_WEIGHTS, 1e-4, (0.9, 0.999), 1e-8, 1e-5, 0, 0, 8, regress="ccc")


def test_the_three_classes_exist_and_refuse_cpu_tensors():
    from sdumc_amd import loss
    from sdumc_amd._lib import SdumcError
    ns = {}
    exec("from sdumc_amd.loss import *", ns)
    for name in ("L1Loss", "HuberLoss", "CCCLoss", "MSELoss"):
        assert isinstance(ns[name](), torch.nn.Module), name
    assert loss.HuberLoss().delta == 1.0 and loss.HuberLoss(delta=0.25).delta == 0.25
    for bad in (0, -1.0, float("inf"), True):
        with pytest.raises(SdumcError, match="regress_delta"):
            loss.HuberLoss(delta=bad)
    a, b = torch.randn(4, 1, requires_grad=True), torch.randn(4)
    for m in (loss.L1Loss(), loss.HuberLoss(), loss.CCCLoss(), loss.MSELoss()):
        with pytest.raises(SdumcError):
            m(a, b)
