"""What makes the bars of the attention-pooling GPU parity test legitimate: on the CPU, from the restatement alone.  For every case of
tests/attn_pool_cases.py the fp32 restatement (ref_lo) is held against the fp64 one (ref_hi) by the rule the device is held to
(tests/grad_parity.py over the slices a workgroup owns): every slice is known to a quarter of its bar or better, the exact-zero slices
are the named ones, nothing lies in between -- except in the offset case, whose e_ref is recorded here.  A case whose reference
cannot meet this is changed here, not loosened on the device side."""
import pytest
import torch

from tests import attn_pool_cases as AC
from tests import grad_parity as GP

# (case, nq): every shape at the two nq the engine runs, the basic shapes at the edges of MAXQ = 8
RUNS = [(n, nq) for n in AC.IDS for nq in (7, 1)] + [(n, nq) for n in AC.BASIC for nq in (8, 2)]


def _judge_lo(case, nq, **kw):
    hi, lo = AC.reference(case, nq, **kw), AC.reference(case, nq, torch.float32, **kw)
    L = AC.lengths_of(case)
    res = AC.judge(lo[0], lo[1], hi, lo, L, "%s nq %d, fp32 restatement as the device" % (case["name"], nq), offset=case["offset"],
                   shared_q=kw.get("shared_q", False), bf16=kw.get("bf16", False))
    return hi, lo, L, res


@pytest.mark.parametrize("name,nq", RUNS, ids=["%s-nq%d" % r for r in RUNS])
def test_reference_knows_every_slice(name, nq):
    case = AC.by_name(name)
    hi, lo, L, res = _judge_lo(case, nq, k3=True)
    V, T = AC.shape(case)[2], case["T"]
    for t in list(hi[0].values()) + list(hi[1].values()):
        assert t.dtype == torch.float64
    for k in ("attn", "dz", "dxd"):                       # padded frames: the same exact zeros in both precisions
        both = dict(hi[0], **hi[1])[k], dict(lo[0], **lo[1])[k]
        assert all(AC.padded_frames_are_zero(t, L) for t in both)
    named = set(AC.zeros(L))
    assert named == {"%s[v%d%s]" % (k, v, c) for v, n in enumerate(L) if n == 1 for k, c in (("dz", ",c0"), ("dq", ""))}
    assert set(res[0].zero) == set() and set(res[1].zero) == named
    chunks = sum((n + AC.CH - 1) // AC.CH for n in L)
    assert len(res[0]) == 2 * chunks + 2 * V and len(res[1]) + len(named) == 2 * chunks + V       # attn, keys | pooled, out || dz, dxd | dq
    worst = [max(r.e_ref.values()) for r in res]
    print("attn pool parity %s nq %d: e_ref worst slice, outputs %.3g, gradients %.3g" % (name, nq, *worst))
    if case["offset"]:
        # fp32 scores near 96 carry an ulp of 7.6e-6 * 0.3 into the exponent: the reference knows this case less well, measured
        # 3.5e-5 .. 4.5e-5 per sample.  The device is then held to max(bar, 4 e_ref) on the slices in between.
        assert max(worst) <= 0.1
        assert res[0].between or res[1].between
    else:
        assert not res[0].between and not res[1].between
        assert worst[0] <= AC.BAR_OUT / 4 and worst[1] <= AC.BAR_GRAD / 4


def test_peaked_scores_span_tens():
    """the peaked case is what it says: a weight computed against another chunk's maximum is wrong by e^2 or more"""
    case = AC.PEAKED
    I = AC.inputs(case, 7)
    s = AC.SCALE * torch.einsum("vtd,vqd->vtq", I["keys"].double(), I["q"].double())
    cmax = torch.stack([s[:, :64].amax(1), s[:, 64:128].amax(1)])
    assert float(s.max() - s.min()) > 14 and float((cmax[0] - cmax[1]).abs().max()) > 3


def test_closed_form_backward_is_autograd():
    case = AC.by_name("T130L")
    I = AC.inputs(case, 7)
    x = I["x"].double().requires_grad_()
    q = I["q"].double().requires_grad_()
    z = torch.atanh(I["keys"].double()).requires_grad_()
    V = z.shape[0]
    xd = x[torch.arange(V) % x.shape[0]] * I["xmask"].double()
    xd.retain_grad()
    outs, _ = AC.attnpool(xd, torch.tanh(z), q, torch.ones_like(xd), I["omask"], I["lengths"], I["dout"], torch.float64, x_samples=V)
    (outs["out"] * I["dout"].double()).sum().backward()
    _, grads = AC.reference(case, 7)
    # (the closed-form dxd is the pooling path alone: autograd's gradient of xd with the keys held fixed)
    for k, g in (("dz", z.grad), ("dq", q.grad), ("dxd", xd.grad)):
        assert GP.close_norm(g, grads[k], 1e-9, k) < 1e-9


BF16_RUNS = [(n, nq, m) for n in AC.BASIC for nq in (7, 1) for m in (True, False)]


@pytest.mark.parametrize("name,nq,x_mask", BF16_RUNS, ids=["%s-nq%d-%s" % (n, q, "mask" if m else "nomask") for n, q, m in BF16_RUNS])
def test_bf16_rounded_references(name, nq, x_mask):
    """bf16 frames: both restatements start from the same bf16 values; the rounded fp32 restatement against the rounded fp64 one,
    per slice of dz / dxd.  The worst slice over all cases is what tests/attn_pool_cases.BF16_E_REF records."""
    case = AC.by_name(name)
    hi, lo, L, res = _judge_lo(case, nq, bf16=True, x_mask=x_mask)
    I = AC.inputs(case, nq, bf16=True, x_mask=x_mask)
    assert torch.equal(I["x"], I["x"].bfloat16().float()) and torch.equal(I["keys"], I["keys"].bfloat16().float())
    for k in ("dz", "dxd"):
        assert torch.equal(hi[1][k], hi[1][k].bfloat16().double()) and torch.equal(lo[1][k], lo[1][k].bfloat16().float())
    e = max(res[2].e_ref.values())
    print("attn pool parity bf16 %s nq %d %s: rounded e_ref worst slice %.3g" % (name, nq, "mask" if x_mask else "no mask", e))
    if case["offset"]:
        assert e <= 0.1 and res[2].between
        return
    _BF16_SEEN.append(e)
    assert e <= AC.BF16_E_REF and not res[2].between
    if len(_BF16_SEEN) == sum(not AC.by_name(r[0])["offset"] for r in BF16_RUNS):
        assert AC.BF16_E_REF <= 1.5 * max(_BF16_SEEN), "BF16_E_REF is not the measured one: worst %.3g" % max(_BF16_SEEN)


_BF16_SEEN = []


@pytest.mark.parametrize("tensor,change", [
    ("attn[v3,c2]", lambda t: t * 1.0001),           # the two rows of the ragged last chunk of T = 130 (length 129: one row)
    ("dz[v0,c2]", lambda t: t * 1.001),
    ("dq[v5]", lambda t: t * 1.001),
    ("pooled[v2]", lambda t: t * 1.0001),
], ids=["ragged attn", "ragged dz", "one dq", "one pooled"])
def test_a_wrong_slice_fails_by_name(tensor, change):
    """the rule bites where the whole-tensor bar did not: the fp32 restatement plays the device, one slice wrong"""
    case = AC.by_name("T130L")
    hi, lo = AC.reference(case, 7), AC.reference(case, 7, torch.float32)
    L = AC.lengths_of(case)
    bad = [{k: v.clone() for k, v in lo[0].items()}, {k: v.clone() for k, v in lo[1].items()}]
    k = tensor.split("[")[0]
    v, c = (int(s.strip("vc")) for s in (tensor[len(k) + 1:-1] + ",c0").split(",")[:2])
    t = bad[k in lo[1]][k]
    if k in AC.PER_SAMPLE:
        t[v] = change(t[v])
    else:
        t[v, c * 64:(c + 1) * 64] = change(t[v, c * 64:(c + 1) * 64])
    with pytest.raises(AssertionError, match=tensor.replace("[", r"\[").replace("]", r"\]") + ": own-norm gradient error"):
        AC.judge(bad[0], bad[1], hi, lo, L, "changed " + tensor)
