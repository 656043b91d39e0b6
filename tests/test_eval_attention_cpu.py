"""CPU-only: the attention-map bookkeeping of evaluate.EvalResult (empty / reset / fits with the attention setting, attention_of's
slicing by the store's start / length tables, the unvisited-utterance error) on CPU tensors and hand-built tables, and the host side of
sdumc_net_export_attention: the ctypes mirror's size and the SDUMC_EINVAL cases, which return before any HIP call (the pointers here
are never dereferenced)."""
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


def _store():
    start = {m: torch.tensor([0] + list(torch.tensor(l).cumsum(0)[:-1]), dtype=torch.int64) for m, l in LENS.items()}
    length = {m: torch.tensor(l, dtype=torch.int32) for m, l in LENS.items()}
    return types.SimpleNamespace(names=["u0", "u1", "u2"], start=start, length=length, MODS=MODS)


def test_empty_reset_and_fits_with_the_attention_setting():
    from sdumc_amd import evaluate as E
    store = _store()
    rows = E.attention_rows(store)
    assert rows == {"audio": 8, "text": 5, "video": 8, "feat4": 4}
    plain = E.EvalResult.empty(3, "cpu", embeddings=True)
    assert plain.attention is None and plain.fits(3, "cpu", True) and not plain.fits(3, "cpu", True, True, rows)
    res = E.EvalResult.empty(3, "cpu", attention=True, rows=rows)
    assert res.embeddings is None and set(res.attention) == {"full", "missing"}
    assert set(res.attention["full"]) == {"audio", "text", "video"} and set(res.attention["missing"]) == {"audio", "feat4", "video"}
    for s, mods in E.ATTENTION:
        for m in mods:
            assert res.attention[s][m].shape == (rows[m], 8) and res.attention[s][m].dtype == torch.float32
    assert res.fits(3, "cpu", False, True, rows) and res.fits(3, "cpu", False, True, [8, 5, 8, 4])
    assert not res.fits(3, "cpu", False) and not res.fits(3, "cpu", True, True, rows) and not res.fits(4, "cpu", False, True, rows)
    assert not res.fits(3, "cpu", False, True, dict(rows, feat4=5))      # another store's frame counts
    with pytest.raises(E._lib.SdumcError):
        E.EvalResult.empty(3, "cpu", attention=True)                     # no row counts
    for d in res.attention.values():
        for t in d.values():
            t.zero_()
    res.preds.zero_()
    res.seen.fill_(1)
    assert res.reset() is res and int(res.seen.sum()) == 0 and bool(torch.isnan(res.preds).all())
    assert all(bool(torch.isnan(t).all()) for d in res.attention.values() for t in d.values())
    both = E.EvalResult.empty(3, "cpu", embeddings=True, attention=True, rows=rows).reset()
    assert both.fits(3, "cpu", True, True, rows) and bool(torch.isnan(both.embeddings["fused"]).all())


def test_attention_of_slices_by_the_stores_tables_by_index_and_by_name():
    from sdumc_amd import evaluate as E
    store = _store()
    res = E.EvalResult.empty(3, "cpu", attention=True, rows=E.attention_rows(store)).reset()
    for si, (s, mods) in enumerate(E.ATTENTION):      # element = 1000 * stream + 100 * modality slot + 10 * row + column
        for mi, m in enumerate(mods):
            t = res.attention[s][m]
            t.copy_(1000.0 * si + 100.0 * mi + 10.0 * torch.arange(t.shape[0])[:, None] + torch.arange(8.0)[None, :])
    res.seen[0], res.seen[2] = 1, 1
    for key, i in ((0, 0), ("u0", 0), (2, 2), ("u2", 2)):
        got = res.attention_of(store, key)
        assert set(got) == {"full", "missing"}
        for si, (s, mods) in enumerate(E.ATTENTION):
            assert tuple(got[s]) == mods
            for mi, m in enumerate(mods):
                a, n = sum(LENS[m][:i]), LENS[m][i]
                assert got[s][m].shape == (n, 8)
                assert torch.equal(got[s][m], res.attention[s][m][a:a + n])
                assert float(got[s][m][0, 0]) == 1000.0 * si + 100.0 * mi + 10.0 * a
                assert got[s][m].data_ptr() == res.attention[s][m][a:a + n].data_ptr()      # a view, not a copy
    assert res.attention_of(store, 2)["missing"]["feat4"].shape == (1, 8) and res.attention_of(store, 0)["full"]["audio"].shape == (3, 8)


def test_attention_of_refuses_what_it_cannot_serve():
    from sdumc_amd import evaluate as E
    store = _store()
    res = E.EvalResult.empty(3, "cpu", attention=True, rows=E.attention_rows(store)).reset()
    res.seen[1] = 1
    res.attention_of(store, "u1")
    for bad in (0, "u2", 3, -1, "nobody"):      # not visited, out of range, unknown name
        with pytest.raises(E._lib.SdumcError):
            res.attention_of(store, bad)
    plain = E.EvalResult.empty(3, "cpu").reset()
    plain.seen.fill_(1)
    with pytest.raises(E._lib.SdumcError):
        plain.attention_of(store, 0)


def test_attn_export_struct_matches_the_header():
    from sdumc_amd import _lib
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sdumc_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n", ' \
          'sizeof(sdumc_attn_export), offsetof(sdumc_attn_export, n_utt), offsetof(sdumc_attn_export, dst), ' \
          'offsetof(sdumc_attn_export, dst_rows)); return 0;}\n'
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "t.c"), "-o", os.path.join(td, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(td, "t")]).split()]
    A = _lib.AttnExport
    assert got == [C.sizeof(A), A.n_utt.offset, A.dst.offset, A.dst_rows.offset]


@pytest.mark.skipif(torch.cuda.is_available(), reason="invented addresses: on a machine with a GPU tests/test_gpu_eval_attention.py "
                    "checks the same cases with live allocations")
def test_export_argument_errors_come_back_before_any_hip_call():
    """Host-only machines: every SDUMC_EINVAL / SDUMC_ENOMEM case returns before any HIP call, so the invented addresses below are never
    dereferenced.  Where a GPU is present the test does not run (a case that slipped through would launch on those addresses); its GPU
    twin, test 6 of tests/test_gpu_eval_attention.py, passes live allocations and a poisoned destination."""
    from sdumc_amd import _lib
    from sdumc_amd.engine import make_dims
    fn = _lib.lib.sdumc_net_export_attention

    def args(streams=2):
        d = make_dims(4, streams, 21, 13, (5, 4), (64, 32, 48), False, 0)
        io = _lib.NetIO()
        io.workspace, io.workspace_bytes = 0x10000, _lib.lib.sdumc_net_workspace_bytes(C.byref(d))
        e = _lib.AttnExport()
        e.idx, e.n_utt = 0x20000, 9
        for k in range(4 if streams == 2 else 3):
            e.start[k], e.length[k] = 0x30000 + 0x100 * k, 0x40000 + 0x100 * k
        for s in range(streams):
            for m in range(3):
                e.dst[s][m], e.dst_rows[s][m] = 0x50000 + 0x1000 * (3 * s + m), 50
        return d, io, e

    def call(d, io, e):
        return fn(C.byref(d) if d is not None else None, C.byref(io) if io is not None else None,
                  C.byref(e) if e is not None else None, None)

    d, io, e = args()
    assert io.workspace_bytes > 0
    assert call(None, io, e) == call(d, None, e) == call(d, io, None) == -1
    cases = {"idx": lambda d, io, e: setattr(e, "idx", None),
             "workspace": lambda d, io, e: setattr(io, "workspace", None),
             "n_utt": lambda d, io, e: setattr(e, "n_utt", 0),
             "start table": lambda d, io, e: e.start.__setitem__(3, None),
             "length table": lambda d, io, e: e.length.__setitem__(0, None),
             "destination": lambda d, io, e: e.dst[1].__setitem__(1, None),
             "alignment": lambda d, io, e: e.dst[0].__setitem__(2, 0x52008),
             "dst_rows": lambda d, io, e: e.dst_rows[1].__setitem__(0, 0),
             "refused dims": lambda d, io, e: setattr(d, "B", 0),
             "refused dims (no feat4 length)": lambda d, io, e: d.Tt.__setitem__(1, 0)}
    for what, spoil in cases.items():
        d, io, e = args()
        spoil(d, io, e)
        assert call(d, io, e) == -1, what
    d, io, e = args(streams=1)
    e.dst[1][2] = 0x60000
    assert call(d, io, e) == -1, "streams == 1 with a stream-1 destination"
    d, io, e = args()
    io.workspace_bytes -= 4
    assert call(d, io, e) == -3, "workspace too small"
