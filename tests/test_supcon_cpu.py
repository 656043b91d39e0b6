"""CPU-only: the selectable contrastive criterion (Rank-N-Contrast / SupCon) as far as it shows without a GPU -- the float64
restatement the GPU tests compare with reproduces the fixture recorded from the reference's own SupConLoss
(tests/golden/make_supcon_goldens.py), the C ABI declares the entries, and the Python layers map and reject."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import supcon_ref  # noqa: E402

CASES = ("cls7", "simclr", "one", "mask", "v1", "odd", "t05", "prenorm", "zero", "round")


def case_kwargs(g, name):
    o = g[f"{name}_opts"]
    kw = dict(temperature=float(o[0]), base_temperature=float(o[1]), contrast_mode="all" if o[2] else "one", normalize=bool(o[3]),
              label_mode=int(o[4]))
    for k in ("labels", "mask"):
        if f"{name}_{k}" in g.files:
            kw[k] = torch.from_numpy(g[f"{name}_{k}"])
    return kw


def test_fixture_is_plain_data_and_holds_every_case(golden):
    path = os.path.join(HERE, "golden", "supcon.npz")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "golden", "distill_losses.npz")) // 2
    g = golden("supcon")
    assert all(g[k].dtype != object for k in g.files)
    shapes = {"cls7": (16, 2, 64), "simclr": (16, 2, 64), "one": (16, 2, 64), "mask": (8, 3, 32), "v1": (6, 1, 16), "odd": (13, 2, 5),
              "t05": (16, 2, 64), "prenorm": (16, 2, 64), "zero": (8, 2, 16), "round": (16, 2, 64)}
    for name in CASES:
        f = g[f"{name}_feat"]
        assert f.shape == shapes[name] and f.dtype == np.float32
        assert g[f"{name}_grad"].shape == f.shape and g[f"{name}_grad"].dtype == np.float64
        assert g[f"{name}_value"].shape == () and np.isfinite(g[f"{name}_value"]) and np.isfinite(g[f"{name}_grad"]).all()
        assert g[f"{name}_gap"].shape == (3,) and (g[f"{name}_gap"] > 0).all()
    # the cases are what the generator says they are
    assert "simclr_labels" not in g.files and "simclr_mask" not in g.files
    m = g["mask_mask"]
    assert set(np.unique(m)) == {0.0, 1.0} and not np.array_equal(m, m.T)
    assert g["v1_labels"].tolist() == [0, 1, 1, 2, 3, 3]
    assert g["one_opts"][2] == 0 and g["t05_opts"][0] == 0.5 and g["prenorm_opts"][3] == 0 and g["round_opts"][4] == 1
    np.testing.assert_allclose(np.linalg.norm(g["prenorm_feat"], axis=-1), 1.0, atol=1e-6)
    assert not g["zero_feat"][3, 1].any() and g["zero_feat"][3, 0].any()
    y = g["round_labels"]
    assert (np.abs(y) <= 3).all() and (y != np.rint(y)).any()
    assert g["n1024_gap"].shape == (5,) and (g["n1024_gap"] > 0).all()


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_fixture(golden, name):
    """tests/supcon_ref.py (a loop over anchors, float64) against the reference's own float64 value and gradient: 1e-12 relative
    (the gradient by norm and by its largest entry).  This pins the restatement the GPU tests use for shapes without a fixture."""
    g = golden("supcon")
    v, gr = supcon_ref.value_and_grad(torch.from_numpy(g[f"{name}_feat"]), **case_kwargs(g, name))
    want_v, want_g = float(g[f"{name}_value"]), torch.from_numpy(g[f"{name}_grad"])
    assert abs(float(v) - want_v) <= 1e-12 * abs(want_v)
    assert float((gr - want_g).norm()) <= 1e-12 * float(want_g.norm())
    assert float((gr - want_g).abs().max()) <= 1e-12 * float(want_g.abs().max())


def test_raw_rows_are_nan_in_the_restatement_as_in_the_reference():
    """Why the fused step normalises: on un-normalised 64-wide rows every off-diagonal exp underflows at T = 0.07, even in float64."""
    f = torch.randn(16, 2, 64, generator=torch.Generator().manual_seed(0)) * 4
    assert torch.isnan(supcon_ref.supcon(f, labels=torch.arange(16.) % 7))
    assert torch.isfinite(supcon_ref.supcon(f, labels=torch.arange(16.) % 7, normalize=True))


def test_header_declares_the_entries_and_the_contrast_codes():
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "sdumc_hip.h")).read()
    assert re.search(r"\bsize_t sdumc_supcon_workspace_bytes\(", header) and re.search(r"\bint sdumc_supcon_fwd_bwd\(", header)
    assert "#define SDUMC_CONTRAST_RNC 0" in header and "#define SDUMC_CONTRAST_SUPCON 1" in header
    assert "loss.py:143-240" in header
    from sdumc_amd import _lib
    assert {"sdumc_supcon_workspace_bytes", "sdumc_supcon_fwd_bwd"} <= set(_lib.EXPORTS)
    # the workspace query needs no GPU: coefficients [A, N], norms [N], row values [A], in doubles; 0 beyond the built limits
    ws = _lib.lib.sdumc_supcon_workspace_bytes
    assert ws(16, 2, 1) == 8 * (32 * 32 + 32 + 32) and ws(16, 2, 0) == 8 * (16 * 32 + 32 + 16)
    assert ws(1024, 2, 1) > 0 and ws(1025, 2, 1) == 0 and ws(4, 0, 1) == 0


def test_contrast_code_maps_and_rejects():
    from sdumc_amd import _lib, engine, trainer
    assert _lib.CONTRAST == {"rnc": 0, "supcon": 1}
    assert _lib.contrast_code("rnc") == (0, 0) and _lib.contrast_code("supcon", "round") == (1, 1)
    for bad in ("nope", "RNC", 1, None):
        with pytest.raises(_lib.SdumcError, match="contrast"):
            _lib.contrast_code(bad)
    flat = torch.zeros(16)
    dims, T = (64, 32, 48, 32), (21, 5, 13, 4)
    for kw in ({"contrast": "simclr"}, {"contrast": 1}, {"contrast": "supcon", "contrast_classes": "seven"},
               {"contrast": "supcon", "contrast_temperature": 0.0}, {"contrast": "supcon", "contrast_temperature": "0.07"}):
        with pytest.raises(_lib.SdumcError, match="contrast"):
            engine.TrainStep(flat, 4, T, dims, **kw)
        with pytest.raises(_lib.SdumcError, match="contrast"):
            engine.FusedTrainer(flat, dims, **kw)
    with pytest.raises(_lib.SdumcError, match="contrast"):
        trainer.DataParallelStep(flat, 4, T, dims, contrast="nope")
    with pytest.raises(_lib.SdumcError, match="data parallelism"):      # the rank exchange carries RnC records only
        trainer.DataParallelStep(flat, 4, T, dims, contrast="supcon")


def test_step_cfg_ends_in_the_new_fields_and_a_zeroed_struct_is_rnc():
    """The four fields close the struct together with `distill`, which tests/test_distill_cpu.py pins as the LAST field: they sit
    directly in front of it, behind everything older, and the C header declares them in the same order."""
    import ctypes as C
    from sdumc_amd import _lib
    names = [f[0] for f in _lib.StepCfg._fields_]
    assert names[-6:] == ["rnc_row0", "contrast", "supcon_label_mode", "supcon_temperature", "supcon_base_temperature", "distill"]
    header = open(os.path.join(os.path.dirname(HERE), "include", "sdumc_hip.h")).read()
    body = header[header.index("typedef struct sdumc_step_cfg {"):header.index("} sdumc_step_cfg;")]
    decl = re.findall(r"^  (?:int32_t|float) (\w+)(?:\[\d+\])?;", body, flags=re.M)
    assert decl[-6:] == names[-6:]
    types = dict(_lib.StepCfg._fields_)
    assert types["contrast"] is C.c_int32 and types["supcon_label_mode"] is C.c_int32
    assert types["supcon_temperature"] is C.c_float and types["supcon_base_temperature"] is C.c_float
    z = _lib.StepCfg()
    assert z.contrast == 0 == _lib.CONTRAST["rnc"] and z.supcon_label_mode == 0 and z.supcon_temperature == 0.0
    cfg = _lib.StepCfg()
    _lib.contrast_cfg(cfg, "rnc", None, "eq")
    assert (cfg.contrast, cfg.temperature, cfg.supcon_temperature) == (0, 2.0, 0.0)
    _lib.contrast_cfg(cfg, "supcon", None, "round")
    assert (cfg.contrast, cfg.supcon_label_mode) == (1, 1) and cfg.supcon_temperature == pytest.approx(0.07, rel=1e-7)
    _lib.contrast_cfg(cfg, "supcon", 0.5, "eq")
    assert cfg.supcon_temperature == 0.5 and cfg.supcon_label_mode == 0


def test_class_has_the_references_signature_and_errors():
    from sdumc_amd import loss
    from sdumc_amd._lib import SdumcError
    assert "SupConLoss" in loss.__all__
    ns = {}
    exec("from sdumc_amd.loss import *", ns)
    assert ns["SupConLoss"] is loss.SupConLoss
    ctor = inspect.signature(loss.SupConLoss.__init__).parameters
    assert [(k, p.default) for k, p in ctor.items() if k != "self"] == [
        ("temperature", 0.07), ("contrast_mode", "all"), ("base_temperature", 0.07), ("normalize", False)]
    assert ctor["normalize"].kind is inspect.Parameter.KEYWORD_ONLY
    fwd = inspect.signature(loss.SupConLoss.forward).parameters
    assert [(k, p.default) for k, p in fwd.items() if k != "self"] == [("features", inspect.Parameter.empty), ("labels", None),
                                                                       ("mask", None)]
    m = loss.SupConLoss()
    assert isinstance(m, torch.nn.Module) and (m.temperature, m.contrast_mode, m.base_temperature, m.normalize) == (0.07, "all", 0.07, False)
    f = torch.randn(4, 2, 8)
    with pytest.raises(ValueError, match="at least 3 dimensions"):
        m(torch.randn(4, 8))
    with pytest.raises(ValueError, match="Cannot define both"):
        m(f, labels=torch.zeros(4), mask=torch.eye(4))
    with pytest.raises(ValueError, match="Num of labels"):
        m(f, labels=torch.zeros(5))
    with pytest.raises(ValueError, match="Unknown mode"):
        loss.SupConLoss(contrast_mode="some")(f)
    # no CPU fallback
    for kw in ({}, {"labels": torch.zeros(4)}, {"mask": torch.eye(4)}):
        with pytest.raises(SdumcError):
            m(f.clone().requires_grad_(), **kw)
    with pytest.raises(SdumcError):
        loss.SupConLoss(normalize=True)(torch.randn(4, 2, 2, 4))
