"""CPU-only: the selectable distillation criterion (RMSE / cosine / KL) as far as it shows without a GPU -- the six loss
classes the reference driver builds (main_frame_val_text_missing.py:310-315) exist, refuse CPU tensors, the fused step
refuses an unknown criterion before it touches a device, and the reference fixture is plain data."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_loss_module_exposes_the_six_classes_of_the_reference_driver():
    ns = {}
    exec("from sdumc_amd.loss import *", ns)
    for name in ("MSELoss", "RMSELoss", "CosineSimilarityLoss4Seq", "CELoss", "KLLoss", "RnCLoss"):
        assert isinstance(ns[name](), torch.nn.Module), name
    # main :310-315 + the dict of :331, on the CPU (.cuda() of a parameterless module is a no-op the driver calls)
    losses = {'reg_loss': ns["MSELoss"](), 'cls_loss': ns["CELoss"](), 'kl_loss': ns["KLLoss"](), 'rnc_loss': ns["RnCLoss"](),
              'rmse_loss': ns["RMSELoss"](), 'coss_loss': ns["CosineSimilarityLoss4Seq"]()}
    assert len(losses) == 6


def test_new_criteria_refuse_cpu_tensors():
    from sdumc_amd._lib import SdumcError
    from sdumc_amd.loss import CELoss, CosineSimilarityLoss4Seq, KLLoss
    a, b = torch.randn(4, 8, requires_grad=True), torch.randn(4, 8)
    for m in (CosineSimilarityLoss4Seq(), KLLoss()):
        with pytest.raises(SdumcError):
            m(a, b)
    with pytest.raises(SdumcError):
        CELoss()(torch.randn(4, 3), torch.tensor([0, 1, 2, 0]))


def test_unknown_criterion_is_rejected_before_any_device_work():
    from sdumc_amd import _lib, engine, trainer
    flat = torch.zeros(16)
    dims, T = (64, 32, 48, 32), (21, 5, 13, 4)
    for bad in ("nope", "RMSE", 1, None):
        with pytest.raises(_lib.SdumcError, match="distill"):
            engine.TrainStep(flat, 4, T, dims, distill=bad)
        with pytest.raises(_lib.SdumcError, match="distill"):
            engine.FusedTrainer(flat, dims, distill=bad)
        with pytest.raises(_lib.SdumcError, match="distill"):
            trainer.DataParallelStep(flat, 4, T, dims, distill=bad)
    assert _lib.DISTILL == {"rmse": 0, "cosine": 1, "kl": 2}
    assert _lib.StepCfg().distill == 0                      # a zeroed struct = RMSE: existing callers are unchanged
    assert _lib.StepCfg._fields_[-1][0] == "distill"        # appended, nothing before it moved


def test_header_names_the_three_criteria():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sdumc_hip.h")).read()
    for name, code in (("RMSE", 0), ("COSINE", 1), ("KL", 2)):
        assert f"#define SDUMC_DISTILL_{name} {code}" in header


def test_distill_fixture_is_plain_data():
    path = os.path.join(GOLDEN, "distill_losses.npz")
    assert os.path.getsize(path) < 1 << 20
    g = np.load(path, allow_pickle=False)
    assert g["th_a"].shape == (16, 256) and g["ct_a"].shape == (16, 7, 128) and g["z_a"].shape == (16, 128)
    for crit in ("cos", "kl"):
        for tag in ("th", "ct", "z", "edge"):
            a = g[f"{tag}_a"] if tag != "edge" else g[f"{crit}_edge_a"]
            assert g[f"{crit}_{tag}"].shape == () and np.isfinite(g[f"{crit}_{tag}"])
            assert g[f"{crit}_{tag}_da"].shape == a.shape and g[f"{crit}_{tag}_db"].shape == a.shape
            assert all(g[k].dtype != object for k in g.files)
    assert g["ce_logits"].shape == (16, 4) and g["ce_target"].shape == (16,) and g["ce_dlogits"].shape == (16, 4)
    # the edge rows are what the generator says they are
    assert not g["cos_edge_a"][0].any() and not g["cos_edge_b"][1].any()
    assert np.array_equal(g["cos_edge_a"][2], g["cos_edge_b"][2]) and np.array_equal(g["kl_edge_a"][0], g["kl_edge_b"][0])
    assert g["kl_edge_a"][1].max() == 30 and g["kl_edge_a"][1].min() == -30
