"""CPU-only: per-tensor learning rates, decay and frozen tensors of the fused step (engine.TensorRates; sdumc_adam_step_rates,
sdumc_zero_segments, sdumc_step_cfg.rates) -- the host side: pattern resolution, the table's order, the struct mirrors against the
C compiler's view of the header, what the entries refuse before any HIP call, and the refusals of the paths it is not built for."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (64, 32, 48)


def _layout():
    from sdumc_amd.engine import ParamLayout
    return ParamLayout.get(*DIMS)


def _rates(**kw):
    from sdumc_amd.engine import TensorRates
    return TensorRates(_layout(), **kw)


def test_table_follows_the_live_names():
    lay = _layout()
    r = _rates(freeze=("frame_dim_reshape_*",), lr_scale={"cross_*": 0.5, "fc_out_v.*": 2.0},
               decay_scale={"*.bias": 0.0, "*.attention_context_vector": 0.0})
    names = lay.live_names()
    assert r.names == names and len(names) == 83
    assert len(r.lr_scale) == len(r.decay_scale) == len(r.frozen) == len(names) == r.c.n
    for i, name in enumerate(names):
        frozen = name.startswith("frame_dim_reshape_")
        assert bool(r.frozen[i]) == frozen == bool(r.c.frozen[i]), name
        want_lr = 0.5 if name.startswith("cross_") else 2.0 if name.startswith("fc_out_v.") else 1.0
        want_wd = 0.0 if (name.endswith(".bias") or name.endswith(".attention_context_vector")) and not frozen else 1.0
        assert r.lr_scale[i] == np.float32(want_lr) == r.c.lr_scale[i], name
        assert r.decay_scale[i] == np.float32(want_wd) == r.c.wd_scale[i], name
    # the segments are the layout's own offsets and element counts, ascending and disjoint
    segs = r.segments()
    for (off, n, ls, ws, fr), name in zip(segs, names):
        o, shape, live = lay.entries[name]
        assert live and off == o and n == int(np.prod(shape))
    assert all(a[0] + a[1] <= b[0] for a, b in zip(segs, segs[1:])) and segs[-1][0] + segs[-1][1] <= lay.live


def test_a_later_entry_overrides_an_earlier_one():
    r = _rates(lr_scale={"*": 0.25, "cross_*": 0.5, "cross_fc_att.*": 4.0}, decay_scale={"*.bias": 0.0, "fc_att.bias": 0.3})
    at = dict(zip(r.names, r.lr_scale))
    assert at["fc_att.weight"] == 0.25 and at["cross_audio_mlp.0.weight"] == 0.5 and at["cross_fc_att.bias"] == 4.0
    wd = dict(zip(r.names, r.decay_scale))
    assert wd["fc_att.bias"] == np.float32(0.3) and wd["fc_out_v.bias"] == 0.0 and wd["fc_out_v.weight"] == 1.0
    # ... in the order given, not in the layout's: the same entries the other way round
    r = _rates(lr_scale={"cross_fc_att.*": 4.0, "cross_*": 0.5, "*": 0.25})
    assert set(r.lr_scale.tolist()) == {0.25}


def test_patterns_that_match_nothing_or_only_dead_parameters():
    from sdumc_amd._lib import SdumcError
    lay = _layout()
    for kw in ({"freeze": ("frame_dim_reshap_*",)}, {"lr_scale": {"no_such_layer.*": 0.5}}, {"decay_scale": {"*.biass": 0.0}},
               {"freeze": ("Frame_dim_reshape_0.weight",)}):      # (case matters, as in the checkpoint's names)
        with pytest.raises(SdumcError, match="matches no parameter"):
            _rates(**kw)
    dead = [n for n in lay.order if not lay.entries[n][2]]
    assert "fc_out_e.weight" in dead and "prelu.weight" in dead
    r = _rates(freeze=("fc_out_e.*", "missing_*"), lr_scale={"prelu.weight": 0.0}, decay_scale={"layer_normali.*": 7.0})
    assert not r.frozen.any() and (r.lr_scale == 1).all() and (r.decay_scale == 1).all()
    # all three off: nothing to build
    from sdumc_amd.engine import TensorRates
    assert not TensorRates.wanted(None, None, None) and TensorRates.wanted(None, None, ())


def test_frozen_and_scaled_contradict_each_other():
    """An entry that reaches frozen tensors only asks for what cannot happen: refused.  A wider pattern ('*.bias' beside a frozen
    projection, the usual no-decay split) scales the others; the frozen ones among its matches stay frozen, their scales at 1."""
    from sdumc_amd._lib import SdumcError
    for kw in ({"lr_scale": {"frame_dim_reshape_0.*": 0.5}}, {"decay_scale": {"frame_dim_reshape_2.bias": 0.0}},
               {"lr_scale": {"*": 1.0, "frame_dim_reshape_?.weight": 2.0}}):
        with pytest.raises(SdumcError, match="frozen"):
            _rates(freeze=("frame_dim_reshape_*",), **kw)
    r = _rates(freeze=("frame_dim_reshape_*",), decay_scale={"*.bias": 0.0}, lr_scale={"*": 0.5})
    for name, fr, ls, ws in zip(r.names, r.frozen, r.lr_scale, r.decay_scale):
        assert (ls, ws) == ((1.0, 1.0) if fr else (0.5, 0.0 if name.endswith(".bias") else 1.0)), name


@pytest.mark.parametrize("bad", [-0.5, -0.0 - 1e-30, float("nan"), float("inf"), -float("inf"), 1e39, True, "0.5", None,
                                 torch.tensor(0.5)])
def test_scales_are_finite_python_numbers_not_below_zero(bad):
    from sdumc_amd._lib import SdumcError
    for key in ("lr_scale", "decay_scale"):
        with pytest.raises(SdumcError, match="finite number"):
            _rates(**{key: {"fc_att.*": bad}})
    _rates(lr_scale={"fc_att.*": 0}, decay_scale={"fc_att.*": 0.0})      # zero is torch's lr = 0 group


def test_option_types():
    from sdumc_amd._lib import SdumcError
    for kw in ({"freeze": "frame_dim_reshape_*"}, {"freeze": {"a": 1}}, {"freeze": (3,)}, {"lr_scale": ["cross_*"]},
               {"decay_scale": (("*.bias", 0.0),)}, {"lr_scale": {3: 0.5}}):
        with pytest.raises(SdumcError):
            _rates(**kw)


def test_struct_mirrors_match_the_header():
    from sdumc_amd import _lib
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sdumc_hip.h"\nint main(){printf("' + "%zu " * 15 + '%d\\n", ' \
          'sizeof(sdumc_rate_seg), offsetof(sdumc_rate_seg, offset), offsetof(sdumc_rate_seg, n), offsetof(sdumc_rate_seg, lr_scale), ' \
          'offsetof(sdumc_rate_seg, wd_scale), offsetof(sdumc_rate_seg, frozen), ' \
          'sizeof(sdumc_tensor_rates), offsetof(sdumc_tensor_rates, n), offsetof(sdumc_tensor_rates, lr_scale), ' \
          'offsetof(sdumc_tensor_rates, wd_scale), offsetof(sdumc_tensor_rates, frozen), ' \
          'sizeof(sdumc_step_cfg), offsetof(sdumc_step_cfg, rnc_labels_global), offsetof(sdumc_step_cfg, rates), ' \
          'offsetof(sdumc_step_cfg, rnc_row0), SDUMC_RATES_MAX_SEGS); return 0;}\n'
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "t.c"), "-o", os.path.join(td, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(td, "t")]).split()]
    S, T, G = _lib.RateSeg, _lib.TensorRates, _lib.StepCfg
    assert got == [C.sizeof(S), S.offset.offset, S.n.offset, S.lr_scale.offset, S.wd_scale.offset, S.frozen.offset,
                   C.sizeof(T), T.n.offset, T.lr_scale.offset, T.wd_scale.offset, T.frozen.offset,
                   C.sizeof(G), G.rnc_labels_global.offset, G.rates.offset, G.rnc_row0.offset, _lib.RATES_MAX_SEGS]
    # in the middle: behind the guard fields and the data-parallel pointers, in front of the tail other tests pin
    assert _lib.RATES_MAX_SEGS == 96 and G.guard_scratch.offset < G.rnc_labels_global.offset < G.rates.offset < G.rnc_row0.offset


@pytest.mark.skipif(torch.cuda.is_available(), reason="invented addresses: on a machine with a GPU tests/test_gpu_adam_rates.py checks "
                    "the refusals with live allocations")
def test_argument_errors_come_back_before_any_hip_call():
    from sdumc_amd import _lib, ops
    lib = _lib.lib
    P, G, M, V, HY, N = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 4096
    good = [(0, 7, 1.0, 1.0, False), (8, 100, 0.5, 0.0, True), (108, 3988, 2.0, 1.0, False)]

    def step(p=P, g=G, m=M, v=V, n=N, hy=HY, segs=good, nseg=None, table=True):
        tb = ops.rate_segments(segs) if table else None
        return lib.sdumc_adam_step_rates(p, g, m, v, n, hy, 0.9, 0.999, 1e-8, 1e-5, 1.0, tb, len(segs) if nseg is None else nseg, None)

    def zero(buf=G, n=N, segs=good, nseg=None, table=True):
        tb = ops.rate_segments(segs) if table else None
        return lib.sdumc_zero_segments(buf, n, tb, len(segs) if nseg is None else nseg, None)

    for what, kw in {"param": {"p": None}, "grad": {"g": None}, "exp_avg": {"m": None}, "exp_avg_sq": {"v": None}, "hyper": {"hy": None},
                     "n": {"n": 0}, "n < 0": {"n": -4}, "param alignment": {"p": P + 4}, "grad alignment": {"g": G + 8},
                     "moment alignment": {"m": M + 4}, "second moment alignment": {"v": V + 12}}.items():
        assert step(**kw) == -1, what
    for what, kw in {"buf": {"buf": None}, "buf alignment": {"buf": G + 4}, "n": {"n": 0}}.items():
        assert zero(**kw) == -1, what
    many = [(4 * i, 3, 1.0, 1.0, i % 2 == 0) for i in range(97)]
    tables = {"no table": {"table": False}, "nseg 0": {"nseg": 0}, "nseg < 0": {"nseg": -1}, "nseg 97": {"segs": many},
              "overlapping": {"segs": [(0, 8, 1.0, 1.0, True), (7, 8, 1.0, 1.0, True)]},
              "descending": {"segs": [(64, 8, 1.0, 1.0, True), (0, 8, 1.0, 1.0, True)]},
              "behind the end": {"segs": [(4090, 7, 1.0, 1.0, True)]}, "offset < 0": {"segs": [(-1, 7, 1.0, 1.0, True)]},
              "empty segment": {"segs": [(16, 0, 1.0, 1.0, True)]}, "n < 0 segment": {"segs": [(16, -3, 1.0, 1.0, True)]},
              "longer than the bucket": {"segs": [(0, 1 << 62, 1.0, 1.0, True)]},
              "negative lr_scale": {"segs": [(0, 8, -0.5, 1.0, True)]}, "NaN lr_scale": {"segs": [(0, 8, float("nan"), 1.0, True)]},
              "Inf lr_scale": {"segs": [(0, 8, float("inf"), 1.0, True)]}, "negative wd_scale": {"segs": [(0, 8, 1.0, -1.0, True)]},
              "NaN wd_scale": {"segs": [(0, 8, 1.0, float("nan"), True)]}, "Inf wd_scale": {"segs": [(0, 8, 1.0, float("inf"), True)]}}
    for what, kw in tables.items():
        assert step(**kw) == -1, what
        assert zero(**kw) == -1, what
    # a table without a frozen segment gives sdumc_zero_segments nothing to launch: fine, and still no HIP call
    assert zero(segs=[(0, 7, 1.0, 1.0, False), (9, 100, 0.5, 0.0, False)]) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="invented addresses")
def test_the_step_refuses_a_bad_rates_table_before_the_forward():
    from sdumc_amd import _lib
    from sdumc_amd.engine import make_dims
    lib = _lib.lib
    d = make_dims(4, 2, 21, 13, (5, 4), DIMS, True)
    io, cfg = _lib.NetIO(), _lib.StepCfg()
    io.audio, io.video, io.params, io.workspace, io.rng_state = 0x10000, 0x20000, 0x30000, 0x1000000, 0x60000
    io.text[0], io.text[1] = 0x40000, 0x50000
    io.vals, io.fused, io.rnc, io.text_hidden, io.cross_text = 0x70000, 0x80000, 0x90000, 0xa0000, 0xb0000
    # one byte short: a step whose options are all accepted then ends with SDUMC_ENOMEM, still in front of every HIP call -- so -1 below
    # is the table's refusal and nothing else's
    io.workspace_bytes = lib.sdumc_step_workspace_bytes(C.byref(d)) - 1
    cfg.adam_m, cfg.adam_v, cfg.hyper, cfg.losses, cfg.labels = 0x2000000, 0x3000000, 0xc0000, 0xd0000, 0xe0000
    good = _rates(freeze=("frame_dim_reshape_*",)).c

    def run(spoil):
        r = _lib.TensorRates.from_buffer_copy(good)
        spoil(r)
        cfg.rates = C.pointer(r)
        return lib.sdumc_train_step(C.byref(d), C.byref(io), C.byref(cfg), None)

    def put(field, i, v):
        return lambda r: getattr(r, field).__setitem__(i, v)

    assert lib.sdumc_train_step(C.byref(d), C.byref(io), C.byref(cfg), None) == -3      # (no table)
    assert run(lambda r: None) == -3
    for what, spoil in {"n - 1": lambda r: setattr(r, "n", 82), "n + 1": lambda r: setattr(r, "n", 84), "n 0": lambda r: setattr(r, "n", 0),
                        "n 97": lambda r: setattr(r, "n", 97), "negative lr_scale": put("lr_scale", 5, -1.0),
                        "NaN lr_scale": put("lr_scale", 82, float("nan")), "Inf wd_scale": put("wd_scale", 0, float("inf")),
                        "negative wd_scale": put("wd_scale", 40, -0.25)}.items():
        assert run(spoil) == -1, what


def test_data_parallel_step_refuses_the_options():
    from sdumc_amd._lib import SdumcError
    from sdumc_amd.trainer import DataParallelStep
    flat = torch.zeros(_layout().total)
    for kw in ({"freeze": ("frame_dim_reshape_*",)}, {"lr_scale": {"cross_*": 0.5}}, {"decay_scale": {"*.bias": 0.0}}):
        with pytest.raises(SdumcError, match="not built under data parallelism"):
            DataParallelStep(flat, 4, (21, 5, 13, 4), DIMS + (32,), **kw)


def test_a_step_takes_the_options_or_their_resolved_form_not_both():
    from sdumc_amd._lib import SdumcError
    from sdumc_amd.engine import ParamLayout, TensorRates, TrainStep
    flat = torch.zeros(_layout().total)
    with pytest.raises(SdumcError, match="one or the other"):
        TrainStep(flat, 4, (21, 5, 13, 4), DIMS + (32,), rates=_rates(freeze=("fc_att.*",)), freeze=("fc_att.*",))
    with pytest.raises(SdumcError, match="ParamLayout"):
        TrainStep(flat, 4, (21, 5, 13, 4), DIMS + (32,), rates=TensorRates(ParamLayout.get(64, 64, 64), freeze=("fc_att.*",)))
    with pytest.raises(SdumcError, match="matches no parameter"):      # resolved before any device work
        TrainStep(flat, 4, (21, 5, 13, 4), DIMS + (32,), freeze=("nothing_*",))
