"""CPU-only half of the input-feature gradients: the oracle against golden gradients recorded from the real reference model
(tests/golden/make_input_grad_goldens.py), and the host side of the new C entry points -- the ctypes mirrors against the header, the
scratch queries, and every SDUMC_EINVAL / SDUMC_ENOMEM case, which returns before any HIP call (the addresses are invented and
never dereferenced)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_input_gradients_match_the_reference(golden):
    """oracle.sdumc_oracle.forward in fp64, eval mode, reproduces the reference's input gradients of vals.sum() + sum of the
    embeddings' sums to 1e-10 (relative to each tensor's largest entry), for both text-slot inputs."""
    from oracle import sdumc_oracle as O
    g = golden("input_grads")
    dims = tuple(int(v) for v in g["dims"])
    P = {k: v.double() for k, v in O.init_params(dims, seed=int(g["pseed"])).items()}
    for s, slot in enumerate(("text", "feat4")):
        leaves = [torch.from_numpy(g[n]).double().requires_grad_() for n in ("audio", slot, "video")]
        vals, emb = O.forward(P, *leaves)
        (vals.sum() + sum(e.sum() for e in emb)).backward()
        np.testing.assert_allclose(vals.detach().numpy(), g[f"vals{s}"], rtol=1e-10, atol=1e-12)
        for n, t in zip(("audio", "text", "video"), leaves):
            want = g[f"d_{n}{s}"]
            assert float(np.abs(want).max()) > 0
            np.testing.assert_allclose(t.grad.numpy(), want, rtol=0, atol=1e-10 * float(np.abs(want).max()), err_msg=f"d_{n}, stream {s}")


def test_oracle_padded_rows_have_zero_gradient_under_key_padding(golden):
    """with `lengths` the padded frames are outside every softmax: their input gradient is exactly 0; without, it is not"""
    from oracle import sdumc_oracle as O
    g = golden("input_grads")
    dims = tuple(int(v) for v in g["dims"])
    P = {k: v.double() for k, v in O.init_params(dims, seed=int(g["pseed"])).items()}
    lens = g["lens"]      # [B][audio, text, video, feat4]
    for lengths in (None, tuple(lens[:, i].tolist() for i in range(3))):
        leaves = [torch.from_numpy(g[n]).double().requires_grad_() for n in ("audio", "text", "video")]
        vals, emb = O.forward(P, *leaves, lengths=lengths)
        (vals.sum() + sum(e.sum() for e in emb)).backward()
        for i, t in enumerate(leaves):
            pad = torch.arange(t.shape[1])[None, :] >= torch.from_numpy(lens[:, i])[:, None]
            assert bool(pad.any()) and bool((t.grad[~pad] != 0).any())
            if lengths is None:
                assert bool((t.grad[pad] != 0).any())      # the reference: padded frames take part in the softmax
            else:
                assert bool((t.grad[pad] == 0).all())


def test_struct_mirrors_match_the_header():
    from sdumc_amd import _lib
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sdumc_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", ' \
          'sizeof(sdumc_frame_dx_t), offsetof(sdumc_frame_dx_t, W_frag), offsetof(sdumc_frame_dx_t, ldc), offsetof(sdumc_frame_dx_t, T), ' \
          'offsetof(sdumc_frame_dx_t, scratch_bytes), sizeof(sdumc_net_grads), offsetof(sdumc_net_grads, d_audio), ' \
          'offsetof(sdumc_net_grads, feat_scratch_bytes)); return 0;}\n'
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "t.c"), "-o", os.path.join(td, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(td, "t")]).split()]
    F, G = _lib.FrameDx, _lib.NetGrads
    assert got == [C.sizeof(F), F.W_frag.offset, F.ldc.offset, F.T.offset, F.scratch_bytes.offset, C.sizeof(G), G.d_audio.offset,
                   G.feat_scratch_bytes.offset]


def test_scratch_queries():
    from sdumc_amd import _lib
    from sdumc_amd.engine import make_dims
    lib = _lib.lib
    assert lib.sdumc_frame_dx_scratch_bytes(256) == 6 * 256 * 256 and lib.sdumc_frame_dx_scratch_bytes(4096) == 6 * 256 * 4096
    for bad in (0, -256, 255, 128, 257, 1000):
        assert lib.sdumc_frame_dx_scratch_bytes(bad) == 0, bad
    fn = lib.sdumc_net_feature_grad_scratch_bytes
    big = make_dims(64, 2, 375, 225, (32, 32), (1024, 4096, 1024), True)
    assert fn(C.byref(big)) >= 6 * 256 * (1024 + 4096 + 1024)
    assert fn(C.byref(make_dims(4, 2, 21, 13, (5, 4), (48, 32, 40), False))) > 0      # generic widths: never 0 for dims the engine takes
    assert fn(C.byref(make_dims(64, 2, 375, 225, (32, 32), (1024, 4096, 1024), True, bf16=True))) == 0      # bf16 storage
    assert fn(C.byref(make_dims(0, 2, 375, 225, (32, 32), (1024, 4096, 1024), True))) == 0
    assert fn(None) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="invented addresses: on a machine with a GPU tests/test_gpu_input_grads.py checks "
                    "the refusals with live allocations")
def test_argument_errors_come_back_before_any_hip_call():
    from sdumc_amd import _lib
    from sdumc_amd.engine import make_dims
    lib = _lib.lib

    def desc():
        q = _lib.FrameDx()
        q.M, q.N, q.A, q.W, q.C, q.ldw, q.ldc = 66, 512, 0x10000, 0x200000, 0x400000, 512, 512
        q.scratch, q.scratch_bytes = 0x800000, lib.sdumc_frame_dx_scratch_bytes(512)
        return q

    assert lib.sdumc_frame_dx(None, None) == -1
    cases = {"A": lambda q: setattr(q, "A", None), "C": lambda q: setattr(q, "C", None), "W and W_frag": lambda q: setattr(q, "W", None),
             "A alignment": lambda q: setattr(q, "A", 0x10004), "W alignment": lambda q: setattr(q, "W", 0x200008),
             "C alignment": lambda q: setattr(q, "C", 0x400004), "W_frag alignment": lambda q: setattr(q, "W_frag", 0x900004),
             "scratch alignment": lambda q: setattr(q, "scratch", 0x800008),
             "M": lambda q: setattr(q, "M", 0), "N < 256": lambda q: setattr(q, "N", 128), "N % 256": lambda q: setattr(q, "N", 384),
             "ldw": lambda q: setattr(q, "ldw", 508), "ldc": lambda q: setattr(q, "ldc", 256),
             "lengths without T": lambda q: setattr(q, "lengths", 0x700000),
             "M % T": lambda q: (setattr(q, "lengths", 0x700000), setattr(q, "T", 7))}
    for what, spoil in cases.items():
        q = desc()
        spoil(q)
        assert lib.sdumc_frame_dx(C.byref(q), None) == -1, what
    for spoil in (lambda q: setattr(q, "scratch", None), lambda q: setattr(q, "scratch_bytes", q.scratch_bytes - 1)):
        q = desc()
        spoil(q)
        assert lib.sdumc_frame_dx(C.byref(q), None) == -3
    # the packer
    ok = (0x10000, 512, 0x800000, 256, 512)
    for i, v in ((0, None), (2, None), (0, 0x10004), (2, 0x800008), (1, 508), (3, 0), (3, 24), (4, 0), (4, 48)):
        a = list(ok)
        a[i] = v
        assert lib.sdumc_p3_split_frag_t(*a, None) == -1, (i, v)
    # the network level: decided before anything is enqueued
    d = make_dims(4, 2, 21, 13, (5, 4), (256, 512, 256), False)
    io = _lib.NetIO()
    io.audio, io.video, io.params, io.workspace = 0x10000, 0x20000, 0x30000, 0x1000000
    io.text[0], io.text[1] = 0x40000, 0x50000
    io.workspace_bytes = lib.sdumc_net_workspace_bytes(C.byref(d))

    def grads():
        g = _lib.NetGrads()
        g.grads, g.d_audio, g.d_video = 0x60000, 0x100000, 0x200000
        g.d_text[0], g.d_text[1] = 0x300000, 0x400000
        g.feat_scratch, g.feat_scratch_bytes = 0x500000, lib.sdumc_net_feature_grad_scratch_bytes(C.byref(d))
        return g

    def rc(d, g):
        return (lib.sdumc_net_backward(C.byref(d), C.byref(io), C.byref(g), None),
                lib.sdumc_net_backward_phase(C.byref(d), C.byref(io), C.byref(g), 1, None))
    g = grads()
    g.d_video = 0x200004
    assert rc(d, g) == (-1, -1)
    g = grads()
    g.feat_scratch_bytes -= 1
    assert rc(d, g) == (-3, -3)
    g = grads()
    g.feat_scratch = None
    assert rc(d, g) == (-3, -3)
    one = make_dims(4, 1, 21, 13, (5,), (256, 512, 256), False)
    assert rc(one, grads()) == (-1, -1)      # streams == 1 with d_text[1]
    half = make_dims(4, 2, 21, 13, (5, 4), (256, 512, 256), False, bf16=True)
    assert half.bf16 == 2 and rc(half, grads()) == (-1, -1)
