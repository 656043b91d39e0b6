"""rnc_row_body of loss.hip requests all the loads of its head before the first wait and reads the operands of its two masked LDS
sums unconditionally, sixteen bytes at a time.  That reorders memory traffic only: every sum keeps its order, so every output bit is
what it was.  Held here two ways, stand-alone (sdumc_rnc_fwd_bwd) and inside the fused two-launch losses of the training step
(sdumc_losses_fused_):

  * against float64 with the bars of tests/loss_bars.py (through tests/test_gpu_loss_kernels.check_full, element by element), and
  * against tests/golden/loss_stage_bits.npz: SHA-256 digests of the outputs' bytes, recorded once on an MI355X from the library as
    it was BEFORE the heads were reordered (tests/golden/make_loss_stage_bits.py; the runs are the functions of this file).

Shapes (n, dim): (2, 1) and (255, 3) the scalar distance loop, most threads idle | none idle but one, and n no multiple of 4: the
masked sums one float at a time; (3, 100) 25 quads: the head's sixteen and a tail of nine; (5, 36) nine quads: fewer than the head
requests; (96, 64) the last wave without a first row; (128, 64) the training step's own shape; (256, 64) every thread with a row.
(128, 64) once more from a pointer 4 bytes off 16-byte alignment: the scalar distance loop at the model's width.  The fused form
takes even n only (n = 2 B): 2, 96, 128, 256 (n = 2: LDS arrays off 16-byte boundaries, the masked sums' scalar form)."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

from tests.loss_bars import rnc_case
from tests.test_gpu_elementwise import L, Out, dev  # noqa: F401  (L: the library fixture)
from tests.test_gpu_loss_kernels import D, H, NQ, LossBuffers, RncRun, _bind_fused, check_full

pytestmark = pytest.mark.gpu

KIND, T, WEIGHT = "straddle", 2.0, 0.8
SHAPES = [(2, 1), (3, 100), (5, 36), (96, 64), (128, 64), (255, 3), (256, 64)]
ALONE = [(n, dim, False) for n, dim in SHAPES] + [(128, 64, True)]
FUSED = [(n, dim, False) for n, dim in SHAPES if n % 2 == 0] + [(128, 64, True)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_stage_bits.npz")


def key(form, n, dim, offset):
    return f"{form}_n{n}_d{dim}" + ("_off4" if offset else "")


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.numpy()).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def alone_outputs(r):
    return [r.dist, r.G, r.rowloss, r.loss, r.df]


def run_alone(L, n, dim, offset):
    f, y = rnc_case(n, dim, KIND, T)
    return RncRun(L, f, y, T, weight=WEIGHT, offset=offset)


def run_fused(L, n, dim, offset):
    """One call of sdumc_losses_fused_ with the RnC inputs of rnc_case(n, dim) (labels: its first half, repeated by the kernel) and
    seeded distillation inputs.  Returns (buffers, outputs to digest)."""
    fused, _ = _bind_fused(L)
    B = n // 2
    f, y = rnc_case(n, dim, KIND, T)
    g = torch.Generator().manual_seed(7000 + n)
    vals = torch.randn(n, generator=g)
    th, ct, z = torch.randn(n, D, generator=g), torch.randn(n, NQ, H, generator=g), torch.randn(n, H, generator=g)
    if offset:
        buf = torch.zeros(n * dim + 1, device="cuda")
        buf[1:] = f.reshape(-1).cuda()
        fptr = buf.data_ptr() + 4
        assert fptr % 16 == 4
    else:
        buf = dev(f)
        fptr = buf.data_ptr()
        assert fptr % 16 == 0
    vd, ld, thd, ctd, zd = (dev(x) for x in (vals, y[:B], th, ct, z))
    w6 = (C.c_float * 6)(0.5, 0.5, 0.1, 0.7, 0.13, WEIGHT)
    hyper = Out(4, fill=torch.tensor([1e-4, 0.0, 0.0, 0.0]))
    a = LossBuffers(L, B, dim)
    assert fused(B, vd.data_ptr(), ld.data_ptr(), thd.data_ptr(), ctd.data_ptr(), zd.data_ptr(), fptr, dim, T, w6, a.d_vals.ptr(),
                 a.d_th.ptr(), a.d_ct.ptr(), a.d_z.ptr(), a.d_rnc.ptr(), a.losses.ptr(), a.dws.ptr(), a.rws.ptr(), hyper.ptr(), 0.9, 0.999,
                 0, None) == 0
    nn = n * n
    ws = a.rws.get()
    a.dist, a.G, a.rowloss = ws[:nn].reshape(n, n), ws[4 * nn:5 * nn].reshape(n, n), ws[5 * nn + n:]
    a.df, a.loss = a.d_rnc.get(n, dim), a.losses.get()[6:7]
    outs = [a.dist, a.G, a.rowloss, a.losses.get()[1:7], a.df, a.d_vals.get(), a.d_th.get(), a.d_ct.get(), a.d_z.get(), hyper.get()]
    return a, outs


@pytest.fixture(scope="module")
def bits(golden):
    return golden("loss_stage_bits")


@pytest.mark.parametrize("n,dim,offset", ALONE)
def test_rnc_alone_bits(L, bits, n, dim, offset):
    """sdumc_rnc_fwd_bwd: dist, rowloss, G, loss and df inside their float64 bars, and their bytes those of the recorded library."""
    r, _ = check_full(L, n, dim, KIND, T, WEIGHT, offset=offset)
    got, want = digest(alone_outputs(r)), bits[key("alone", n, dim, offset)]
    print("LOSSBITS", key("alone", n, dim, offset), got.tobytes().hex()[:16], want.tobytes().hex()[:16])
    assert np.array_equal(got, want), key("alone", n, dim, offset) + ": the outputs' bytes are not the recorded ones"


@pytest.mark.parametrize("n,dim,offset", FUSED)
def test_rnc_fused_bits(L, bits, n, dim, offset):
    """sdumc_losses_fused_: its Rank-N-Contrast outputs are, bit for bit, those of the stand-alone call on the same rows (which this
    test holds to the float64 bars through check_full), and the bytes of everything the two launches write are the recorded ones."""
    r, _ = check_full(L, n, dim, KIND, T, WEIGHT, offset=offset)
    a, outs = run_fused(L, n, dim, offset)
    for name in ("dist", "G", "rowloss", "loss", "df"):
        assert torch.equal(getattr(a, name), getattr(r, name)), f"{key('fused', n, dim, offset)}: {name} differs from the stand-alone call"
    got, want = digest(outs), bits[key("fused", n, dim, offset)]
    print("LOSSBITS", key("fused", n, dim, offset), got.tobytes().hex()[:16], want.tobytes().hex()[:16])
    assert np.array_equal(got, want), key("fused", n, dim, offset) + ": the outputs' bytes are not the recorded ones"
