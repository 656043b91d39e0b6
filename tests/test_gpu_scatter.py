"""sdumc_scatter_rows_multi (csrc/elementwise.hip): dst_k[idx[r % B], :] = src_k[r, :] for up to SDUMC_SCATTER_MAX_SEGS tensors in one
launch -- what puts an eval-mode forward's stream-major outputs at their utterances' rows of the store-ordered results
(main_frame_val_text_missing.py:156-163 appends them to host lists; sdumc_amd/evaluate.py).  A copy: every comparison is torch.equal
against torch.index_copy_."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

B, N = 5, 11
WIDTHS = (1, 3, 64, 896)      # one float per lane (1, 3: not a multiple of 4) and 16-byte lanes (64, 896 = the widest output, 7 x 128)
FILL = -77.0
EINVAL = -1


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import _lib, ops
    return _lib, ops


def _idx():
    """[2 B] int64 on the device: the batch's B distinct rows, then B OTHER rows -- a kernel that read idx[r] instead of idx[r % B] for
    the second half of a 2 B-row source would write rows that must keep their fill"""
    p = torch.randperm(N, generator=torch.Generator().manual_seed(3))
    return p[:2 * B].contiguous().cuda()


def _sources(rows_of):
    g = torch.Generator(device="cuda").manual_seed(7)
    out = []
    for w in WIDTHS:
        s = torch.randn(B, w, device="cuda", generator=g)
        out.append(torch.cat([s, s]).contiguous() if rows_of(w) == 2 * B else s)      # (both halves name the same rows: equal data)
    return out


def test_scatter_equals_index_copy_for_every_width_and_row_count(env):
    _lib, ops = env
    idx2 = _idx()
    idx = idx2[:B]
    for rows_of in (lambda w: B, lambda w: 2 * B if w in (3, 896) else B):      # all B rows; B and 2 B rows in the same launch
        srcs = _sources(rows_of)
        dsts = [torch.full((N, w), FILL, device="cuda") for w in WIDTHS]
        mark = torch.zeros(N, dtype=torch.uint8, device="cuda")
        ops.scatter_rows_multi(srcs, dsts, idx, mark=mark)
        torch.cuda.synchronize()
        for s, d, w in zip(srcs, dsts, WIDTHS):
            want = torch.full((N, w), FILL, device="cuda").index_copy_(0, idx, s[:B])
            assert torch.equal(d, want), f"width {w}, rows {s.shape[0]}"      # (rows not named keep their fill)
        want_mark = torch.zeros(N, dtype=torch.uint8, device="cuda").index_fill_(0, idx, 1)
        assert torch.equal(mark, want_mark)
    # ten segments (the evaluation epoch's count) in one launch, three-dimensional rows, no mark; a second launch gives the same bits
    srcs = [torch.randn(B, 7, 128, device="cuda") for _ in range(_lib.SCATTER_MAX_SEGS)]
    dsts = [torch.full((N, 7, 128), FILL, device="cuda") for _ in srcs]
    for _ in range(2):
        ops.scatter_rows_multi(srcs, dsts, idx)
    torch.cuda.synchronize()
    for s, d in zip(srcs, dsts):
        assert torch.equal(d, torch.full((N, 7, 128), FILL, device="cuda").index_copy_(0, idx, s))


def test_misaligned_destination_takes_the_scalar_path_and_is_exact(env):
    """a destination view that starts one float into its buffer (64 columns: the 16-byte path but for the address) and a source view of
    the same kind: exact, and the floats around the view are untouched"""
    _lib, ops = env
    idx = _idx()[:B]
    w = 64
    buf = torch.full((N * w + 8,), FILL, device="cuda")
    dst = buf[1:1 + N * w].view(N, w)
    sbuf = torch.randn(B * w + 8, device="cuda")
    src_mis = sbuf[1:1 + B * w].view(B, w)
    assert dst.data_ptr() % 16 == 4 and src_mis.data_ptr() % 16 == 4 and dst.is_contiguous()
    src = torch.randn(B, w, device="cuda")
    aligned = torch.full((N, w), FILL, device="cuda")
    ops.scatter_rows_multi([src, src_mis], [dst, aligned], idx)
    torch.cuda.synchronize()
    assert torch.equal(dst, torch.full((N, w), FILL, device="cuda").index_copy_(0, idx, src))
    assert torch.equal(aligned, torch.full((N, w), FILL, device="cuda").index_copy_(0, idx, src_mis))
    assert float(buf[0]) == FILL and bool((buf[1 + N * w:] == FILL).all())


def test_argument_contract_returns_before_any_launch(env):
    """every SDUMC_EINVAL case of include/sdumc_hip.h: the code comes back and a VALID first segment of the same call has not been
    written (the check runs over all segments before the one launch)"""
    _lib, ops = env
    lib = _lib.lib
    idx = _idx()[:B]
    src = torch.randn(2 * B, 64, device="cuda")
    dst = torch.full((N, 64), FILL, device="cuda")
    mark = torch.zeros(N, dtype=torch.uint8, device="cuda")

    def seg(**kw):
        s = dict(src=src.data_ptr(), dst=dst.data_ptr(), rows=B, cols=64, dst_rows=N)
        s.update(kw)
        return s

    def call(segs, n=None, idx_p=idx.data_ptr(), b=B):
        arr = (_lib.ScatterSeg * max(1, len(segs)))()
        for a, s in zip(arr, segs):
            a.src, a.dst, a.rows, a.cols, a.dst_rows = s["src"], s["dst"], s["rows"], s["cols"], s["dst_rows"]
        return lib.sdumc_scatter_rows_multi(arr, len(segs) if n is None else n, idx_p, b, mark.data_ptr(), None)

    good = seg()
    cases = {
        "n = 0": lambda: call([good], n=0),
        "n > max": lambda: call([good] * (_lib.SCATTER_MAX_SEGS + 1)),
        "segs NULL": lambda: lib.sdumc_scatter_rows_multi(None, 1, idx.data_ptr(), B, None, None),
        "idx NULL": lambda: call([good], idx_p=None),
        "B = 0": lambda: call([good], b=0),
        "B < 0": lambda: call([good], b=-B),
        "src NULL": lambda: call([good, seg(src=None)]),
        "dst NULL": lambda: call([good, seg(dst=None)]),
        "rows = 0": lambda: call([good, seg(rows=0)]),
        "cols = 0": lambda: call([good, seg(cols=0)]),
        "rows % B": lambda: call([good, seg(rows=B + 1)]),
        "dst_rows = 0": lambda: call([good, seg(dst_rows=0)]),
    }
    for name, fn in cases.items():
        assert fn() == EINVAL, name
    torch.cuda.synchronize()
    assert bool((dst == FILL).all()) and int(mark.sum()) == 0, "a refused call launched"
    with pytest.raises(_lib.SdumcError):
        ops.scatter_rows_multi([src], [torch.empty(N, 32, device="cuda")], idx)      # widths differ
    with pytest.raises(_lib.SdumcError):
        ops.scatter_rows_multi([src], [dst], idx.int())
    # the same table, valid: it runs (rows = 2 B against B indices)
    assert call([seg(rows=2 * B)]) == 0
    torch.cuda.synchronize()
    assert int(mark.sum()) == B
