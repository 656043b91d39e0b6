"""CPU-only: the host side of the saliency maps (sdumc_amd/saliency.py; sdumc_frame_saliency, csrc/frame_saliency.hip): the entry is
exported and bound, the ctypes mirror of its descriptor has the header's size and offsets, every SDUMC_EINVAL case returns before any
HIP call (the pointers here are never dereferenced), frame_scores is the written-out fp64 formula, and SaliencyResult's bookkeeping
(empty / fits / reset / of) works on CPU tensors and hand-built tables."""
import ctypes as C
import os
import subprocess
import tempfile
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = ("audio", "text", "video", "feat4")
LENS = {"audio": [3, 1, 4], "text": [2, 2, 1], "video": [1, 5, 2], "feat4": [2, 1, 1]}      # three utterances
ROWS = {"audio": 8, "text": 5, "video": 8, "feat4": 4}


def _store():
    start = {m: torch.tensor([0] + list(torch.tensor(l).cumsum(0)[:-1]), dtype=torch.int64) for m, l in LENS.items()}
    length = {m: torch.tensor(l, dtype=torch.int32) for m, l in LENS.items()}
    return types.SimpleNamespace(names=["u0", "u1", "u2"], start=start, length=length, MODS=MODS)


def test_the_entry_is_exported_and_bound():
    from sdumc_amd import _lib
    assert "sdumc_frame_saliency" in _lib.EXPORTS and hasattr(_lib.lib, "sdumc_frame_saliency")
    header = open(os.path.join(ROOT, "include", "sdumc_hip.h")).read()
    assert "int sdumc_frame_saliency(const sdumc_saliency_desc* descs, int32_t n, const int64_t* idx, void* stream);" in header
    assert f"#define SDUMC_SALIENCY_MAX_DESCS {_lib.SALIENCY_MAX_DESCS}" in header


def test_descriptor_mirror_matches_the_header():
    from sdumc_amd import _lib
    fields = [name for name, _ in _lib.SaliencyDesc._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sdumc_hip.h"\nint main(){printf("%zu", sizeof(sdumc_saliency_desc));\n' + \
          "".join(f'printf(" %zu", offsetof(sdumc_saliency_desc, {f}));\n' for f in fields) + 'return 0;}\n'
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "t.c"), "-o", os.path.join(td, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(td, "t")]).split()]
    D = _lib.SaliencyDesc
    assert got == [C.sizeof(D)] + [getattr(D, f).offset for f in fields]


def _descs(n=3, d=(64, 32, 48, 6)):
    from sdumc_amd import _lib
    arr = (_lib.SaliencyDesc * 4)()
    for k in range(4):
        p = arr[k]
        p.grad, p.feat = 0x100000 + 0x10000 * k, 0x200000 + 0x10000 * k
        p.start, p.length, p.n_utt = 0x300000 + 0x100 * k, 0x400000 + 0x100 * k, 9
        p.dst, p.dst_rows = 0x500000 + 0x1000 * k, 50
        p.B, p.T, p.d = 4, 5 + k, d[k]
    return arr


@pytest.mark.skipif(torch.cuda.is_available(), reason="invented addresses: on a machine with a GPU tests/test_gpu_saliency.py checks "
                    "the same cases with live allocations")
def test_argument_errors_come_back_before_any_hip_call():
    """Host-only machines: every SDUMC_EINVAL case returns before any HIP call, so the invented addresses are never dereferenced.
    Where a GPU is present the test does not run (a case that slipped through would launch on those addresses); its GPU twin passes
    live allocations and a poisoned destination."""
    from sdumc_amd import _lib
    fn = _lib.lib.sdumc_frame_saliency
    IDX = 0x600000
    assert fn(None, 3, IDX, None) == -1
    assert fn(_descs(), 3, None, None) == -1
    for n in (0, -1, 5):
        assert fn(_descs(), n, IDX, None) == -1, n
    cases = {"grad": lambda p: setattr(p, "grad", None), "feat": lambda p: setattr(p, "feat", None),
             "start": lambda p: setattr(p, "start", None), "length": lambda p: setattr(p, "length", None),
             "dst": lambda p: setattr(p, "dst", None),
             "B": lambda p: setattr(p, "B", 0), "T": lambda p: setattr(p, "T", 0), "d": lambda p: setattr(p, "d", 0),
             "n_utt": lambda p: setattr(p, "n_utt", 0), "dst_rows": lambda p: setattr(p, "dst_rows", 0),
             "another B": lambda p: setattr(p, "B", 5),
             "row_map without store_rows": lambda p: setattr(p, "row_map", 0x700000),
             "misaligned grad": lambda p: setattr(p, "grad", p.grad + 4),
             "misaligned dst": lambda p: setattr(p, "dst", p.dst + 8),
             "misaligned feat, d % 4 == 0": lambda p: setattr(p, "feat", p.feat + 4)}
    for what, spoil in cases.items():
        for k in (1, 2):      # (not the first descriptor alone: every descriptor is checked)
            arr = _descs()
            spoil(arr[k])
            assert fn(arr, 3, IDX, None) == -1, (what, k)
    arr = _descs()      # the fourth descriptor is checked only when n says so; its d = 6 takes a feat at any 4-byte address
    arr[3].dst = None
    assert fn(arr, 4, IDX, None) == -1
    arr = _descs()
    arr[0].B = arr[1].B = arr[2].B = 1 << 20      # more than 2^31 - 1 padded rows in all
    arr[0].T = arr[1].T = arr[2].T = 1 << 10
    assert fn(arr, 3, IDX, None) == -1


def test_frame_scores_is_the_written_out_formula():
    from sdumc_amd.saliency import frame_scores, COLUMNS
    assert COLUMNS == ("grad_x_input", "grad_norm")
    g = torch.Generator().manual_seed(3)
    grad, feat = torch.randn(3, 5, 7, generator=g), torch.randn(3, 5, 7, generator=g)
    got = frame_scores(grad, feat)
    assert got.shape == (3, 5, 2) and got.dtype == torch.float64
    for b in range(3):
        for t in range(5):
            dot = sum(float(grad[b, t, c]) * float(feat[b, t, c]) for c in range(7))
            sq = sum(float(grad[b, t, c]) ** 2 for c in range(7))
            assert abs(float(got[b, t, 0]) - dot) <= 1e-14 * (1 + abs(dot)) and abs(float(got[b, t, 1]) - sq ** 0.5) <= 1e-14 * (1 + sq ** 0.5)
    lens = torch.tensor([5, 2, 0])
    cut = frame_scores(grad, feat, lens)
    pad = torch.arange(5)[None, :] >= lens[:, None]
    assert int(pad.sum()) == 8 and bool((cut[pad] == 0).all()) and torch.equal(cut[~pad], got[~pad])
    assert torch.equal(frame_scores(grad[0], feat[0], 3)[:3], got[0, :3]) and bool((frame_scores(grad[0], feat[0], 3)[3:] == 0).all())
    big = torch.tensor([[3e30, 4e30]])      # fp32 inputs whose squares overflow fp32: the sums are formed in fp64
    assert float(frame_scores(big, big)[0, 1]) == pytest.approx(5e30, rel=1e-6)


def test_result_empty_fits_and_reset():
    from sdumc_amd import saliency as S
    store = _store()
    assert S.frame_rows(store) == ROWS
    res = S.SaliencyResult.empty(3, "cpu", ROWS)
    assert res.COLUMNS == S.COLUMNS and tuple(res.maps) == ("full", "missing")
    assert tuple(res.maps["full"]) == ("audio", "text", "video") and tuple(res.maps["missing"]) == ("audio", "feat4", "video")
    for s, d in res.maps.items():
        for m, t in d.items():
            assert t.shape == (ROWS[m], 2) and t.dtype == torch.float32
    assert res.preds.shape == (2, 3) and res.seen.shape == (3,) and res.seen.dtype == torch.uint8
    assert res.fits(3, "cpu", ROWS) and res.fits(3, "cpu", [8, 5, 8, 4]) and res.fits(3, "cpu", ROWS, ("missing", "full"))
    assert not res.fits(4, "cpu", ROWS) and not res.fits(3, "cpu", dict(ROWS, feat4=5)) and not res.fits(3, "cpu", ROWS, ("full",))
    one = S.SaliencyResult.empty(3, "cpu", ROWS, streams=("missing",))
    assert "full" not in one.maps and tuple(one.maps) == ("missing",) and one.fits(3, "cpu", ROWS, ("missing",))
    assert not one.fits(3, "cpu", ROWS) and tuple(S.SaliencyResult.empty(3, "cpu", ROWS, streams="full").maps) == ("full",)
    for bad in (("full", "both"), (), "text"):
        with pytest.raises(S._lib.SdumcError):
            S.SaliencyResult.empty(3, "cpu", ROWS, streams=bad)
    for d in res.maps.values():
        for t in d.values():
            t.zero_()
    res.preds.zero_()
    res.seen.fill_(1)
    assert res.reset() is res and int(res.seen.sum()) == 0 and bool(torch.isnan(res.preds).all())
    assert all(bool(torch.isnan(t).all()) for d in res.maps.values() for t in d.values())


def test_of_slices_by_the_stores_tables_and_refuses_what_it_cannot_serve():
    from sdumc_amd import saliency as S
    store = _store()
    res = S.SaliencyResult.empty(3, "cpu", ROWS).reset()
    for si, (s, d) in enumerate(res.maps.items()):      # element = 1000 * stream + 100 * modality slot + 10 * row + column
        for mi, (m, t) in enumerate(d.items()):
            t.copy_(1000.0 * si + 100.0 * mi + 10.0 * torch.arange(t.shape[0])[:, None] + torch.arange(2.0)[None, :])
    res.seen[0], res.seen[2] = 1, 1
    for key, i in ((0, 0), ("u0", 0), (2, 2), ("u2", 2)):
        got = res.of(store, key)
        assert tuple(got) == ("full", "missing")
        for si, s in enumerate(got):
            for mi, m in enumerate(got[s]):
                a, n = sum(LENS[m][:i]), LENS[m][i]
                assert got[s][m].shape == (n, 2) and torch.equal(got[s][m], res.maps[s][m][a:a + n])
                assert float(got[s][m][0, 0]) == 1000.0 * si + 100.0 * mi + 10.0 * a
                assert got[s][m].data_ptr() == res.maps[s][m][a:a + n].data_ptr()      # a view, not a copy
    for bad in (1, "u1", 3, -1, "nobody"):      # not visited, out of range, unknown name
        with pytest.raises(S._lib.SdumcError):
            res.of(store, bad)
    one = S.SaliencyResult.empty(3, "cpu", ROWS, streams=("missing",)).reset()
    one.seen[1] = 1
    assert tuple(one.of(store, "u1")) == ("missing",) and one.of(store, 1)["missing"]["video"].shape == (5, 2)


def test_package_exports_resolve():
    import sdumc_amd
    from sdumc_amd import saliency
    assert sdumc_amd.saliency_epoch is saliency.saliency_epoch and sdumc_amd.SaliencyResult is saliency.SaliencyResult
    assert {"saliency_epoch", "SaliencyResult"} <= set(sdumc_amd.__all__)
    from sdumc_amd.engine import FusedTrainer
    assert callable(FusedTrainer.saliency_epoch)


def test_module_text_passes_the_product_path_word_check():
    assert "oracle" not in open(os.path.join(ROOT, "sdumc_amd", "saliency.py")).read()      # (tests/test_abi.py's check, on this module)
