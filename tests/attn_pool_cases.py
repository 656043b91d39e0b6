"""The cases of the attention-pooling family (include/sdumc_hip.h: sdumc_attnpool, sdumc_attnpool_bwd, sdumc_umca) and their references;
a plain module, no fixtures.  tests/test_attn_pool_parity_cpu.py (the references alone) and tests/test_gpu_attn_pool.py (every launch
route of csrc/attn_pool.hip) read the same table.

The operation, restated in torch at a given dtype from the header's definition (v = virtual sample, x row of v = v % x_samples), every
sum accumulated left to right in that dtype (_acc: the fp32 form is then the same evaluation on every host):

    xd = x[v % x_samples] * xmask[v]                    masks are 0 or 1 / (1 - p), Philox (oracle/philox.py) or all ones
    K  = the tanh keys, given; the K3 form computes K = tanh(xd W^T + b) itself and returns it
    S  = 0.3 K Q^T, frames t >= max(1, lengths[v]) at -inf;  A = softmax_t S;  O = A^T xd;  out = O * omask
    backward of sum(out * dout):  dO = dout * omask;  dxd = A dO (the pooling path alone);  dA = xd dO^T;
                                  dS = A (dA - sum_t A dA);  dK = 0.3 dS Q;  dz = dK (1 - K^2);  dq = 0.3 dS^T K

A tensor is judged slice by slice, a slice being what one workgroup owns: `pooled`, `out`, `dq` per virtual sample v; `attn`, `dz`,
`dxd` (and K3's `keys`) per (v, 64-frame chunk), cut to the sample's valid frames.  A chunk wholly beyond a sample's length is no
slice: those frames are exact zeros by construction, which the GPU test asserts on the device tensor itself.  The judgement is
tests/grad_parity.py::tensor_errors over the slice names, once for the outputs and once for the gradients, with BAR_OUT / BAR_GRAD of
the slice's own norm; no slice may lie "in between" except in the offset cases, whose fp32 scores near 96 have an ulp of 7.6e-6.
The dz and dq slices of a sample with ONE valid frame are exactly zero (softmax of one frame: dS = 1 * (dA - dA)) and are named.

bf16 frames (sdumc_attnpool.bf16): x and keys are bf16 VALUES, both restatements start from the same ones, and the reference of the
bf16 dz / dxd is the fp64 result rounded to bf16 (round to nearest even, from the fp64 bits directly).  Rounding alone is 1.7e-3 of
a slice's norm, so the device is not held to the unrounded value: it is held to the rounded reference, with 4 x the error the two
rounded restatements have against each other (BF16_E_REF, measured by the CPU test, which asserts it again on every run)."""
import functools

import numpy as np
import torch

BAR_OUT = 2e-5           # of a slice's own norm: attn, pooled, out, keys
BAR_GRAD = 2e-4          # dz, dxd, dq
# bf16 dz / dxd slices, fp32 restatement rounded to bf16 against fp64 restatement rounded to bf16: the worst slice over every bf16 case
# but the offset one (tests/test_attn_pool_parity_cpu.py::test_bf16_rounded_references prints each and asserts worst <= this <= 1.5
# worst; measured 4.4e-5 .. 4.3e-4 over the cases).  A 64 x 256 slice in which k elements of typical size round the other way sits at
# sqrt(k / 16384) * 2^-8 ~ 3e-5 sqrt(k): it moves in steps, hence a quarter above the worst measured.  The offset case (1e-3: its unrounded e_ref is 4e-5) lies in between, as in fp32.
BF16_E_REF = 5.5e-4
CH, D, SCALE, P_DROP = 64, 256, 0.3, 0.5
SEED, CALL, SITE_X, SITE_O = 20250117, 5, 23, 24

# V forms: (B samples of x, streams).  "shared": two streams read the same three samples of x; the others own their frames
FORMS = {"shared": (3, 2), "own6": (6, 1), "own5": (5, 1), "one": (1, 1)}


def case_lengths(T):
    return [T, 1, T // 2, T - 1, min(T, 65), min(T, 64)]


def _case(name, T, lens, form="shared", qscale=0.25, offset=False, seed=0):
    return dict(name=name, T=T, lens=lens, form=form, qscale=qscale, offset=offset, seed=seed)


T_SWEEP = [_case("T%d%s" % (T, "L" if lens else ""), T, lens, seed=10 * T + lens)
           for T in (1, 2, 63, 64, 65, 130, 257) for lens in (False, True)]
V_FORMS = [_case("%s_T%d%s" % (form, T, "L" if lens else ""), T, lens, form=form, seed=7000 + 10 * i + lens)
           for i, form in enumerate(("own6", "own5", "one")) for T, lens in ((65, False), (130, True))]
# peaked: queries randn * 0.75, scores span 14 .. 17 and the chunk maxima of a sample differ by up to 4.5.  At randn * 2 (span 34) and
# down to randn * 1 the fp32 restatement itself leaves the held class on single slices of attn (e_ref 9.2e-6, 4.3e-6 against
# BAR_OUT / 4 = 5e-6); at 0.75 its worst slice is 2.9e-6.
PEAKED = _case("peaked_T130L", 130, True, qscale=0.75, seed=8001)
OFFSET = _case("offset_T130L", 130, True, offset=True, seed=8002)
MULTI_ONLY = _case("T37L", 37, True, seed=8003)          # the third site of the multi-site launches (T 130 / 64 / 37)
CASES = T_SWEEP + V_FORMS + [PEAKED, OFFSET, MULTI_ONLY]
IDS = [c["name"] for c in CASES]
# what every route other than the engine's two and v1-with-Philox runs
BASIC = ["T65", "T130L", "peaked_T130L", "offset_T130L"]
SWEEP = [n for n in IDS if n != "T37L"]
NQS = (1, 7, 8, 2)


def by_name(name):
    return CASES[IDS.index(name)]


def shape(case):
    B, S = FORMS[case["form"]]
    return B, S, B * S


def lengths_of(case):
    """valid frames per virtual sample (python ints, already >= 1), T for every sample of a case without lengths"""
    V = shape(case)[2]
    return [max(1, n) for n in case_lengths(case["T"])[:V]] if case["lens"] else [case["T"]] * V


def philox_masks(case, nq, dim=D, x_mask=True):
    """(xmask [V, T, dim], omask [V, nq, dim]) as float32: stream s of the descriptor's row space draws call CALL + s"""
    from oracle import philox
    B, S, V = shape(case)
    om = np.concatenate([philox.dropout_mask(B, nq, dim, P_DROP, SEED, CALL + s, SITE_O) for s in range(S)])
    if not x_mask:
        return torch.ones(V, case["T"], dim), torch.from_numpy(om)
    xm = np.concatenate([philox.dropout_mask(B, case["T"], dim, P_DROP, SEED, CALL + s, SITE_X) for s in range(S)])
    return torch.from_numpy(xm), torch.from_numpy(om)


@functools.lru_cache(maxsize=None)
def _inputs(name, nq, dim, x_mask, bf16, shared_q, k3):
    case = by_name(name)
    B, S, V = shape(case)
    T = case["T"]
    g = torch.Generator().manual_seed(case["seed"] * 100 + nq * 10 + dim // 256)
    x = torch.randn(B, T, dim, generator=g)
    keys = torch.tanh(torch.randn(V, T, dim, generator=g))
    q = torch.randn(1 if shared_q else V, nq, dim, generator=g) * case["qscale"]
    dout = torch.randn(V, nq, dim, generator=g)
    W, b = torch.randn(dim, dim, generator=g) / 16, torch.randn(dim, generator=g) * 0.1
    if case["offset"]:          # every score carries +96: it cancels in the softmax, and overflows expf where no maximum is subtracted
        keys[..., 0] = 1.0
        q[..., 0] = 96.0 / SCALE
        W[0], b[0] = 0.0, 20.0          # (the K3 form: tanh(20) is exactly 1 in fp32 and in fp64)
    if bf16:
        x, keys = x.bfloat16().float(), keys.bfloat16().float()
    xm, om = philox_masks(case, nq, dim, x_mask)
    I = dict(x=x, keys=keys, q=q, dout=dout, xmask=xm, omask=om, lengths=lengths_of(case), x_samples=B)
    if k3:
        I.update(W=W, b=b)
    return I


def inputs(case, nq, dim=D, x_mask=True, bf16=False, shared_q=False, k3=False):
    """fp32 CPU inputs of a case (never to be written to): x [B, T, dim], keys [V, T, dim] (tanh values; bf16 values when bf16),
    q [V or 1, nq, dim], dout, the two masks, lengths as a list of ints, and W, b for the K3 form"""
    return _inputs(case["name"], nq, dim, x_mask, bf16, shared_q, k3)


def _acc(n, term):
    """sum_{k < n} term(k), accumulated left to right in the terms' dtype.  Every reduction of the restatement is written this way, so
    that ref_lo is ONE fp32 evaluation on every host: a BLAS sums in blocks of the host's vector width, and a blocked sum hides
    exactly what the offset case is about -- beside a partial sum of 320 every product lands on a grid of 2^-15, whatever the order."""
    a = term(0)
    for k in range(1, n):
        a = a + term(k)
    return a


def attnpool(x, keys, q, xmask, omask, lengths, dout, dtype, x_samples=None):
    """the operation and its backward at `dtype`; q [V or 1, nq, dim] (a shared query's dq is the sum over v)"""
    V, T, Dm = keys.shape
    nq = q.shape[1]
    xs = x_samples or x.shape[0]
    xd = x.to(dtype)[torch.arange(V) % xs] * xmask.to(dtype)
    K, Q = keys.to(dtype), q.to(dtype).expand(V, -1, -1)
    s = SCALE * _acc(Dm, lambda c: K[:, :, c, None] * Q[:, None, :, c])                      # [V, T, nq]
    valid = torch.arange(T)[None, :] < torch.tensor(lengths)[:, None].clamp(min=1)
    s = s.masked_fill(~valid[:, :, None], float("-inf"))
    e = torch.exp(s - s.amax(1, keepdim=True))
    A = e / _acc(T, lambda t: e[:, t])[:, None]
    pooled = _acc(T, lambda t: A[:, t, :, None] * xd[:, t, None, :])                          # [V, nq, dim]
    out = pooled * omask.to(dtype)
    dO = dout.to(dtype) * omask.to(dtype)
    dxd = _acc(nq, lambda i: A[:, :, i, None] * dO[:, None, i, :])                            # [V, T, dim]
    dA = _acc(Dm, lambda c: xd[:, :, c, None] * dO[:, None, :, c])
    dS = A * (dA - _acc(T, lambda t: A[:, t] * dA[:, t])[:, None])
    dz = SCALE * _acc(nq, lambda i: dS[:, :, i, None] * Q[:, None, i, :]) * (1 - K * K)
    dq = SCALE * _acc(T, lambda t: dS[:, t, :, None] * K[:, t, None, :])
    if q.shape[0] == 1:
        dq = _acc(V, lambda v: dq[v])[None]
    return dict(attn=A, pooled=pooled, out=out), dict(dz=dz, dxd=dxd, dq=dq)


def k3_keys(x, W, b, xmask, dtype, x_samples=None):
    V = xmask.shape[0]
    xd = x.to(dtype)[torch.arange(V) % (x_samples or x.shape[0])] * xmask.to(dtype)
    return torch.tanh(xd @ W.to(dtype).T + b.to(dtype))


def round_bf16(t):
    """float64 -> the nearest bf16 value (ties to even), as float64; rounds the fp64 bits directly, not through fp32"""
    bits = t.detach().double().contiguous().numpy().view(np.uint64)
    low = np.uint64((1 << 45) - 1)
    r = (bits + np.uint64((1 << 44) - 1) + ((bits >> np.uint64(45)) & np.uint64(1))) & ~low
    return torch.from_numpy(r.view(np.float64).copy()).reshape(t.shape)


@functools.lru_cache(maxsize=None)
def _reference(name, nq, dim, x_mask, bf16, shared_q, k3, dtype):
    I = _inputs(name, nq, dim, x_mask, bf16, shared_q, k3)
    keys = k3_keys(I["x"], I["W"], I["b"], I["xmask"], dtype) if k3 else I["keys"]
    outs, grads = attnpool(I["x"], keys, I["q"], I["xmask"], I["omask"], I["lengths"], I["dout"], dtype)
    if k3:
        outs["keys"] = keys
    if bf16:        # the bf16 stores: the reference is the rounded one
        grads["dz"], grads["dxd"] = round_bf16(grads["dz"]).to(dtype), round_bf16(grads["dxd"]).to(dtype)
    return outs, grads


def reference(case, nq, dtype=torch.float64, dim=D, x_mask=True, bf16=False, shared_q=False, k3=False):
    """(outputs, gradients) of the restatement at `dtype` (float64 = ref_hi, float32 = ref_lo of tests/grad_parity.py), whole tensors;
    computed once per process, shared, never to be written to"""
    return _reference(case["name"], nq, dim, x_mask, bf16, shared_q, k3, dtype)


PER_SAMPLE = ("pooled", "out", "dq")
PER_CHUNK = ("attn", "keys", "dz", "dxd")


def slices(tensors, lengths):
    """name -> slice of every tensor of `tensors`: per v, or per (v, 64-frame chunk) cut to the valid frames.  A dq of one row (shared
    query) is one slice."""
    out = {}
    for k, t in tensors.items():
        if k in PER_SAMPLE:
            if t.shape[0] == 1 and len(lengths) > 1:
                out[k + "[sum]"] = t[0]
                continue
            for v in range(t.shape[0]):
                out["%s[v%d]" % (k, v)] = t[v]
        else:
            assert k in PER_CHUNK, k
            for v, n in enumerate(lengths):
                for c in range((n + CH - 1) // CH):
                    out["%s[v%d,c%d]" % (k, v, c)] = t[v, c * CH:min(n, (c + 1) * CH)]
    return out


def zeros(lengths, shared_q=False):
    """the slices that are exactly zero in fp64: dz and dq of a sample with one valid frame (a shared query's summed dq only when
    every sample has one)"""
    z = []
    for v, n in enumerate(lengths):
        if n == 1:
            z.append("dz[v%d,c0]" % v)
            if not shared_q or len(lengths) == 1:
                z.append("dq[v%d]" % v)
    if shared_q and len(lengths) > 1 and all(n == 1 for n in lengths):
        z.append("dq[sum]")
    return tuple(z)


def padded_frames_are_zero(t, lengths):
    """frames at or beyond a sample's length hold exact zeros (attn, dz, dxd)"""
    return all(int(torch.count_nonzero(t[v, n:])) == 0 for v, n in enumerate(lengths))


def judge(got_outs, got_grads, hi, lo, lengths, what, offset=False, shared_q=False, bf16=False):
    """the device's (or a stand-in's) outputs and gradients against ref_hi, slice by slice (module docstring).  hi / lo: the
    (outputs, gradients) pairs of reference().  bf16: dz and dxd are bf16 stores, held to the rounded reference with 4 BF16_E_REF, in a
    call of their own.  -> [TensorErrors of the outputs, of the gradients (, of the bf16 stores)]"""
    from tests import grad_parity as GP
    z = zeros(lengths, shared_q)
    groups = [(got_outs, hi[0], lo[0], BAR_OUT), (dict(got_grads), hi[1], lo[1], BAR_GRAD)]
    if bf16:
        stores = {k: groups[1][0].pop(k) for k in ("dz", "dxd") if k in got_grads}
        groups.append((stores, hi[1], lo[1], 4 * BF16_E_REF))
    res = []
    for got, h, l, bar in groups:
        names = sorted(got)
        if not names:
            res.append(GP.TensorErrors())
            continue
        g = slices({k: got[k] for k in names}, lengths)
        h, l = slices({k: h[k] for k in names}, lengths), slices({k: l[k] for k in names}, lengths)
        r = GP.tensor_errors(list(h), g, h, l, bar, zeros=z, what="%s %s" % (what, "+".join(names)), nosignal=(),
                             between=list(h) if offset else (), max_between=0, keep_old=False)
        assert offset or not r.between, (what, r.between)
        res.append(r)
    return res
