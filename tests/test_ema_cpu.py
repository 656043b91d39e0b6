"""CPU-only: averaged weights (an EMA of the parameters kept by the fused step: TrainStep / FusedTrainer(ema_decay=, ema_warmup=);
sdumc_adam_step_ema, sdumc_ema_multi, sdumc_step_cfg.ema / ema_decay / ema_warmup) as far as they show without a GPU -- the struct
mirror against the C compiler's view of the header, what the constructors and the entries refuse on the host, the fp64 reference of
the GPU tests against torch's own EMA function, and the checkpoint round trip."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ema_ref  # noqa: E402

ROOT = os.path.dirname(HERE)
DIMS = (64, 32, 48)
BAD_DECAYS = [True, False, "0.9", torch.tensor(0.9), float("nan"), -1e-9, 1.0 + 1e-9, float("inf"), -float("inf"), [0.9], np.array(0.9)]


def _layout():
    from sdumc_amd.engine import ParamLayout
    return ParamLayout.get(*DIMS)


def test_step_cfg_mirrors_the_header():
    """1. offsetof / sizeof from a compiled program; the three fields directly behind `rates` and in front of `rnc_row0`; a zeroed
    struct has them off; the switch and the exports"""
    from sdumc_amd import _lib
    fields = ("rates", "ema", "ema_decay", "ema_warmup", "rnc_row0", "contrast", "distill", "losses", "clip_norm", "B_global",
              "rnc_labels_global")
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sdumc_hip.h"\nint main(){printf("' + "%zu " * (len(fields) + 5) + '\\n", ' \
          + ", ".join(f"offsetof(sdumc_step_cfg, {f})" for f in fields) + ", sizeof(sdumc_step_cfg), sizeof(sdumc_ema_seg), " \
          "offsetof(sdumc_ema_seg, ema), offsetof(sdumc_ema_seg, param), offsetof(sdumc_ema_seg, n)); return 0;}\n"
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "t.c"), "-o", os.path.join(td, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(td, "t")]).split()]
    G, S = _lib.StepCfg, _lib.EmaSeg
    assert got == [getattr(G, f).offset for f in fields] + [C.sizeof(G), C.sizeof(S), S.ema.offset, S.param.offset, S.n.offset]
    names = [f[0] for f in G._fields_]
    i = names.index("rates")
    assert names[i:i + 5] == ["rates", "ema", "ema_decay", "ema_warmup", "rnc_row0"]
    assert names[-6:] == ["rnc_row0", "contrast", "supcon_label_mode", "supcon_temperature", "supcon_base_temperature", "distill"]
    assert names[names.index("losses") + 1] == "clip_norm" and names[i - 1] == "rnc_labels_global"
    z = G()
    assert not z.ema and z.ema_decay == 0.0 and z.ema_warmup == 0
    assert _lib.EMA_ABI is True
    assert "sdumc_adam_step_ema" in _lib.EXPORTS and "sdumc_ema_multi" in _lib.EXPORTS
    # ... and the header declares them
    header = open(os.path.join(ROOT, "include", "sdumc_hip.h")).read()
    assert "int sdumc_adam_step_ema(" in header and "int sdumc_ema_multi(" in header


@pytest.mark.parametrize("bad", BAD_DECAYS, ids=[repr(b)[:24] for b in BAD_DECAYS])
def test_constructors_refuse_a_bad_decay_on_the_host(bad):
    """2. bools, strings, tensors, NaN and values outside [0, 1]: refused before the parameter tensor is looked at (a CPU tensor, and
    None, get as far as this refusal and no further)"""
    from sdumc_amd._lib import SdumcError
    from sdumc_amd.engine import FusedTrainer, TrainStep
    flat = torch.zeros(_layout().total)
    for params in (flat, None):
        with pytest.raises(SdumcError, match="ema_decay"):
            TrainStep(params, 4, (21, 5, 13, 4), DIMS + (32,), ema_decay=bad)
        with pytest.raises(SdumcError, match="ema_decay"):
            FusedTrainer(params, DIMS + (32,), ema_decay=bad)


def test_constructors_take_the_options_and_refuse_warmup_alone():
    from sdumc_amd import _lib
    from sdumc_amd._lib import SdumcError
    from sdumc_amd.engine import FusedTrainer, TrainStep
    import inspect
    for cls in (TrainStep, FusedTrainer):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["ema_decay"].default is None and sig["ema_warmup"].default is False
    for cls, args in ((TrainStep, (4, (21, 5, 13, 4), DIMS + (32,))), (FusedTrainer, (DIMS + (32,),))):
        with pytest.raises(SdumcError, match="ema_warmup=True needs ema_decay"):
            cls(None, *args, ema_warmup=True)
        for w in (1, "yes", None):
            with pytest.raises(SdumcError, match="ema_warmup must be True or False"):
                cls(None, *args, ema_decay=0.9, ema_warmup=w)
    # the accepted values: both ends of the range, ints, and what reaches the struct
    assert _lib.ema_args(None, False) == (False, 0.0, 0)
    assert _lib.ema_args(0, False) == (True, 0.0, 0) and _lib.ema_args(1, True) == (True, 1.0, 1)
    assert _lib.ema_args(0.999, True) == (True, 0.999, 1)


def test_paths_that_are_not_built_refuse():
    """capture() of a step with an EMA, DataParallelStep(ema_decay=), weights='ema' on a trainer without one"""
    from sdumc_amd._lib import SdumcError
    from sdumc_amd.engine import FusedTrainer, TrainStep
    from sdumc_amd.trainer import DataParallelStep
    flat = torch.zeros(_layout().total)
    for kw in ({"ema_decay": 0.999}, {"ema_decay": 0.0}, {"ema_warmup": True}, {"ema_decay": 0.9, "ema_warmup": True}):
        with pytest.raises(SdumcError, match="ema_decay / ema_warmup are not built under data parallelism"):
            DataParallelStep(flat, 4, (21, 5, 13, 4), DIMS + (32,), **kw)
    # no device is needed to ask: objects with the attributes the methods look at first
    ts = TrainStep.__new__(TrainStep)
    ts.guard, ts.rates, ts.ema_params = None, None, flat
    with pytest.raises(SdumcError, match="capture: a step with ema_decay"):
        ts.capture()
    tr = FusedTrainer.__new__(FusedTrainer)
    tr.params = flat
    tr.state = type("S", (), {"ema_params": None})()
    for call in (tr.eval_epoch, tr.saliency_epoch):
        with pytest.raises(SdumcError, match="weights='ema' on a trainer without averaged weights"):
            call(None, None, weights="ema")
        with pytest.raises(SdumcError, match="weights must be 'params' or 'ema'"):
            call(None, None, weights="average")
    from sdumc_amd.engine import _RunState
    tr.state = _RunState.__new__(_RunState)      # (a run without an average)
    for call in (lambda: tr.load_ema(flat), tr.reset_ema):
        with pytest.raises(SdumcError, match="keeps no averaged weights"):
            call()
    tr.state.ema_params = torch.zeros(8)
    for bad in (torch.zeros(7), torch.zeros(8, dtype=torch.float64), [0.0] * 8):
        with pytest.raises(SdumcError, match="load_ema: expected a flat fp32 tensor of 8 elements"):
            tr.load_ema(bad)


@pytest.mark.skipif(torch.cuda.is_available(), reason="invented addresses: on a machine with a GPU tests/test_gpu_adam_ema.py and "
                    "tests/test_gpu_ema_multi.py check the refusals with live allocations")
def test_argument_errors_come_back_before_any_hip_call():
    """3. sdumc_adam_step_ema and sdumc_ema_multi on invented addresses"""
    from sdumc_amd import _lib, ops
    lib = _lib.lib
    P, G, M, V, HY, A, N = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 4096
    good = [(0, 7, 1.0, 1.0, False), (8, 100, 0.5, 0.0, True), (108, 3988, 2.0, 1.0, False)]

    def step(p=P, g=G, m=M, v=V, n=N, hy=HY, segs=None, nseg=None, a=A, decay=0.999, warm=0):
        tb = ops.rate_segments(segs) if segs is not None else None
        return lib.sdumc_adam_step_ema(p, g, m, v, n, hy, 0.9, 0.999, 1e-8, 1e-5, 1.0, tb, (len(segs) if segs is not None else 0)
                                       if nseg is None else nseg, a, decay, warm, None)

    cases = {"param": {"p": None}, "grad": {"g": None}, "exp_avg": {"m": None}, "exp_avg_sq": {"v": None}, "hyper": {"hy": None},
             "n": {"n": 0}, "n < 0": {"n": -4}, "param alignment": {"p": P + 4}, "grad alignment": {"g": G + 8},
             "moment alignment": {"m": M + 4}, "second moment alignment": {"v": V + 12},
             "ema NULL": {"a": None}, "ema alignment": {"a": A + 4}, "ema is param": {"a": P}, "ema overlaps param": {"a": P + 16},
             "ema overlaps param from below": {"a": P - 4 * N + 16},
             "decay < 0": {"decay": -0.5}, "decay > 1": {"decay": 1.5}, "decay NaN": {"decay": float("nan")},
             "decay Inf": {"decay": float("inf")},
             "a table without a count": {"segs": good, "nseg": 0}, "a count without a table": {"nseg": 3},
             "overlapping": {"segs": [(0, 8, 1.0, 1.0, True), (7, 8, 1.0, 1.0, True)]},
             "behind the end": {"segs": [(4090, 7, 1.0, 1.0, True)]}, "NaN lr_scale": {"segs": [(0, 8, float("nan"), 1.0, True)]},
             "97 segments": {"segs": [(4 * i, 3, 1.0, 1.0, False) for i in range(97)]}}
    for what, kw in cases.items():
        assert step(**kw) == -1, what
        if "segs" not in kw and "nseg" not in kw:      # ... and the same refusal in the rates form
            assert step(segs=good, **kw) == -1, what + " (with a table)"

    def multi(segs, nseg=None, w=0.25):
        tb = (_lib.EmaSeg * max(1, len(segs)))()
        for s, (a, p, n) in zip(tb, segs):
            s.ema, s.param, s.n = a, p, n
        return lib.sdumc_ema_multi(tb if segs else None, len(segs) if nseg is None else nseg, w, None)

    ok = [(A, P, 100), (A + 404, P + 404, 7)]
    for what, (segs, kw) in {"no table": ([], {}), "nseg 0": (ok, {"nseg": 0}), "nseg < 0": (ok, {"nseg": -2}),
                             "ema NULL": ([(None, P, 8)], {}), "param NULL": ([(A, None, 8)], {}), "n 0": ([(A, P, 0)], {}),
                             "n < 0": (ok + [(A + 4096, P + 4096, -1)], {}), "ema not a float address": ([(A + 2, P, 8)], {}),
                             "param not a float address": ([(A, P + 1, 8)], {}), "w < 0": (ok, {"w": -0.25}), "w > 1": (ok, {"w": 1.25}),
                             "w NaN": (ok, {"w": float("nan")})}.items():
        assert multi(segs, **kw) == -1, what


@pytest.mark.skipif(torch.cuda.is_available(), reason="invented addresses")
def test_the_step_refuses_bad_ema_fields_before_the_forward():
    """sdumc_train_step checks the new fields with the others: a workspace one byte short gives SDUMC_ENOMEM only once every option
    has been accepted, still in front of every HIP call"""
    from sdumc_amd import _lib
    from sdumc_amd.engine import make_dims
    lib = _lib.lib
    d = make_dims(4, 2, 21, 13, (5, 4), DIMS, True)
    io, cfg = _lib.NetIO(), _lib.StepCfg()
    io.audio, io.video, io.params, io.workspace, io.rng_state = 0x10000, 0x20000, 0x4000000, 0x1000000, 0x60000
    io.text[0], io.text[1] = 0x40000, 0x50000
    io.vals, io.fused, io.rnc, io.text_hidden, io.cross_text = 0x70000, 0x80000, 0x90000, 0xa0000, 0xb0000
    io.workspace_bytes = lib.sdumc_step_workspace_bytes(C.byref(d)) - 1
    cfg.adam_m, cfg.adam_v, cfg.hyper, cfg.losses, cfg.labels = 0x2000000, 0x3000000, 0xc0000, 0xd0000, 0xe0000

    def run(ema, decay, warm):
        cfg.ema, cfg.ema_decay, cfg.ema_warmup = ema, decay, warm
        return lib.sdumc_train_step(C.byref(d), C.byref(io), C.byref(cfg), None)

    E = 0x5000000
    assert run(None, 0.0, 0) == -3 and run(E, 0.999, 0) == -3 and run(E, 0.0, 1) == -3 and run(E, 1.0, 0) == -3
    for what, args in {"decay without ema": (None, 0.5, 0), "warm-up without ema": (None, 0.0, 1), "misaligned": (E + 4, 0.5, 0),
                       "the parameters themselves": (0x4000000, 0.5, 0), "inside the parameters": (0x4000000 + 64, 0.5, 0),
                       "decay < 0": (E, -0.1, 0), "decay > 1": (E, 1.1, 0), "decay NaN": (E, float("nan"), 0)}.items():
        assert run(*args) == -1, what


def test_reference_against_torch_and_the_warmup_schedule():
    """4. tests/ema_ref.py against torch.optim.swa_utils.get_ema_multi_avg_fn on CPU tensors: within a quarter of the bound; the
    warm-up schedule's w for t = 1 .. 20 is the closed form, as exact fp32 values"""
    from torch.optim.swa_utils import get_ema_multi_avg_fn
    g = torch.Generator().manual_seed(3)
    a = torch.exp2(torch.rand(100000, generator=g) * 24 - 12) * (torch.randint(0, 2, (100000,), generator=g) * 2 - 1)
    p = torch.exp2(torch.rand(100000, generator=g) * 24 - 12) * (torch.randint(0, 2, (100000,), generator=g) * 2 - 1)
    p[:30000] = a[:30000] * (1 + torch.randn(30000, generator=g) * 1e-3)       # a parameter close to its average, as in training
    for decay in (0.999, 0.9, 0.5, 0.3, 0.75, 0.0, 1.0):
        w = ema_ref.weight(decay, fp32_decay=False)
        assert w == float(np.float32(1.0 - decay))
        got = a.clone()
        get_ema_multi_avg_fn(decay)([got], [p], 1)
        r = ema_ref.worst(got, a, p, w)
        print(f"decay {decay}: torch's own EMA against the fp64 rule: {r:.4f} of the bound")
        assert r <= 0.25, (decay, r)
        if w in ema_ref.EXACT_WEIGHTS:
            assert torch.equal(got.view(torch.int32), ema_ref.lerp32(a, p, w).view(torch.int32))
        ema_ref.check(got, a, p, w, f"decay {decay}")
    assert torch.equal(ema_ref.lerp32(a, p, 1.0).view(torch.int32), p.view(torch.int32))       # decay 0: the parameters' bits
    assert torch.equal(ema_ref.lerp32(a, a, 0.001).view(torch.int32), a.view(torch.int32))     # a parameter that does not move
    # the warm-up: w_t = fp32(1 - min(d, (1 + t) / (10 + t)))
    for d in (0.999, 0.9, 0.5):
        for t in range(1, 21):
            want = np.float32(1.0 - min(float(np.float32(d)), (1.0 + t) / (10.0 + t)))
            got = ema_ref.weight(d, t, warmup=True)
            assert np.float32(got) == want and got == float(want), (d, t)
    assert ema_ref.weight(0.999, 8, warmup=True) == 0.5 and ema_ref.weight(0.999, 1, warmup=True) == float(np.float32(9.0 / 11.0))
    assert ema_ref.weight(0.9, 1000, warmup=True) == ema_ref.weight(0.9) == float(np.float32(1.0 - float(np.float32(0.9))))
    # the schedule rises to the decay and stays: (1 + t) / (10 + t) reaches 0.9 at t = 80
    assert ema_ref.weight(0.9, 79, warmup=True) > ema_ref.weight(0.9) == ema_ref.weight(0.9, 80, warmup=True)


def test_checkpoint_round_trip(tmp_path):
    """5. ema= is written under the checkpoint's own names; load_ema gives the flat tensor back bit for bit; a file without the key
    gives None and the four old return values are what they were"""
    from sdumc_amd import checkpoint
    from sdumc_amd._lib import SdumcError

    class Net(torch.nn.Module):      # the bare network as the checkpoint code sees it: a layout, a flat buffer, named parameters
        def __init__(self):
            super().__init__()
            self._layout = _layout()
            self._flat = torch.zeros(self._layout.total)
            self.w = torch.nn.Parameter(torch.arange(6.0).reshape(2, 3))

    net, lay = Net(), _layout()
    g = torch.Generator().manual_seed(9)
    flat = torch.zeros(lay.total)
    for v in lay.views(flat).values():      # (alignment padding between tensors is +0.0 in every parameter buffer, this one too)
        v.copy_(torch.randn(v.shape, generator=g))
    flat[3] = -0.0
    plain, with_ema, from_dict = (str(tmp_path / n) for n in ("plain.pt", "ema.pt", "dict.pt"))
    checkpoint.save_checkpoint(plain, net, {"state": {}, "param_groups": []}, 7)
    checkpoint.save_checkpoint(with_ema, net, {"state": {}, "param_groups": []}, 7, ema=flat)
    checkpoint.save_checkpoint(from_dict, net, {"state": {}, "param_groups": []}, 7, ema={k: v.clone() for k, v in lay.views(flat).items()})
    a, b = torch.load(plain, weights_only=True), torch.load(with_ema, weights_only=True)
    assert set(a) == {"epoch", "state_dict", "optimizer"} and set(b) == set(a) | {"ema_state_dict"}
    assert list(b["ema_state_dict"]) == ["model." + k for k in lay.order]
    assert list(b["state_dict"]) == ["model.w"] and list(b["state_dict"]) == list(a["state_dict"])
    for k, v in lay.views(flat).items():
        assert torch.equal(b["ema_state_dict"]["model." + k], v) and b["ema_state_dict"]["model." + k].shape == v.shape
    for path in (with_ema, from_dict):
        back = checkpoint.load_ema(path, net)
        assert back.dtype == torch.float32 and back.shape == flat.shape and back.device.type == "cpu"
        assert torch.equal(back.view(torch.int32), flat.view(torch.int32))
    assert checkpoint.load_ema(plain, net) is None
    for path in (plain, with_ema):
        fresh = Net()
        with torch.no_grad():
            fresh.w.zero_()
        epoch, opt, missing, unexpected = checkpoint.load_checkpoint(path, fresh)
        assert (epoch, opt, list(missing), list(unexpected)) == (7, {"state": {}, "param_groups": []}, [], [])
        assert torch.equal(fresh.w, net.w)
    for bad in (flat[:-1], flat.double(), [flat], {"w": flat}):
        with pytest.raises(SdumcError, match="ema must"):
            checkpoint.save_checkpoint(str(tmp_path / "bad.pt"), net, {}, 0, ema=bad)
