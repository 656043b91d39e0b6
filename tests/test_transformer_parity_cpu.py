"""What makes the bars of the Transformer-family GPU parity test legitimate: on the CPU, from the oracle alone.  For every case of
tests/transformer_cases.py the fp32 oracle (ref_lo) is held against the fp64 oracle (ref_hi) by the rule the device is held to
(tests/grad_parity.py): every tensor is known to a quarter of its bar or better, the no-signal and exact-zero sets are the named ones,
nothing lies in between.  A case whose reference cannot meet this is changed here, not loosened on the device side."""
import pytest
import torch

from tests import grad_parity as GP
from tests import transformer_cases as TC


def _e_ref(lo, hi):
    return float((lo.double() - hi).norm() / hi.norm())


@pytest.mark.parametrize("case", TC.CASES, ids=TC.IDS)
def test_reference_knows_every_tensor(case):
    outs_hi, hi = TC.reference(case)
    outs_lo, lo = TC.reference(case, torch.float32)
    names = list(hi)
    assert set(names) == set(lo) and all(hi[k].dtype == torch.float64 and lo[k].dtype == torch.float32 for k in names)
    for k in outs_hi:
        e = _e_ref(outs_lo[k], outs_hi[k])
        print("transformer parity %s: %s e_ref %.3g" % (case["name"], k, e))
        assert e <= TC.BAR_OUT / 4, k
    if "weights" in outs_hi:        # masked and dropped entries: the same exact zeros in both precisions
        assert torch.equal(outs_hi["weights"] == 0, outs_lo["weights"] == 0)
        if case["mask"] or (case["train"] and case["p"] > 0):
            assert bool((outs_hi["weights"] == 0).any())
    nosig, zeros = TC.no_signal(case, names), TC.zeros(case)
    res = GP.tensor_errors(names, lo, hi, lo, TC.BAR_GRAD, zeros=zeros, what=case["name"] + ", fp32 oracle as the device",
                           nosignal=nosig, max_between=0)
    for k in sorted(res.e_ref, key=res.e_ref.get)[-3:]:
        print("transformer parity %s: %s e_ref %.3g (|g| = %.3g)" % (case["name"], k, res.e_ref[k], float(hi[k].norm())))
    assert set(res.zero) == set(zeros)
    assert set(res.nosignal) == set(nosig) - set(zeros)
    assert not res.between
    assert set(res) == set(names) - set(nosig) - set(zeros)
    assert max(res.e_ref[k] for k in res) <= TC.BAR_GRAD / 4
    # every part of every fused buffer, and every input, is there by name
    assert sum(k.endswith((".q", ".k", ".v")) for k in names) == 6 * (case["layers"] if case["kind"] == "enc" else 1)
    assert sum(k in ("dq", "dk", "dv", "dx", "dkv", "dxk", "dxv") for k in names) == len(TC.inputs(case)[0])
    if TC.extra_rows(case):
        assert res.e_ref["in_proj_bias.k"] <= TC.BAR_GRAD / 4


def _dkey_alone(case, lo):
    """the kv-alias case's input gradient with the value path's share lost: key and value as two leaves, the key's gradient only"""
    from oracle import transformer_oracle as TO
    P = {k: v.clone() for k, v in TC.params(case).items()}
    X, R = TC.inputs(case)
    kv, v = X["kv"].clone().requires_grad_(), X["kv"].clone().requires_grad_()
    out, _ = TO.multi_head_attention(P, "", X["q"], kv, v, case["H"], TO.DropSeq())
    (out * R).sum().backward()
    assert GP.close_norm(kv.grad + v.grad, lo["dkv"], 1e-5, "dkv") < 1e-5
    return kv.grad


@pytest.mark.parametrize("name,tensor,change", [
    ("self", "in_proj_weight.k", lambda case, lo: lo["in_proj_weight.k"] * 1.01),                      # a part's scale
    ("both_extras", "in_proj_bias.k", lambda case, lo: lo["in_proj_bias.k"] * 1.01),                   # a real tensor with extra source rows
    ("kv_alias", "dkv", _dkey_alone),                                                                  # the aliased dkey + dvalue sum, lost
    ("encoder_cross", "layers.1.self_attn.out_proj.bias", lambda case, lo: lo["layers.1.self_attn.out_proj.bias"] * (1 - case["p_res"])),
], ids=["k part scaled", "k bias with extra rows", "alias sum lost", "dropout unscaled"])
def test_a_wrong_tensor_fails_by_name(name, tensor, change):
    """the rule bites: the fp32 oracle plays the device, with one tensor wrong in a way a backward goes wrong"""
    case = TC.by_name(name)
    _, hi = TC.reference(case)
    _, lo = TC.reference(case, torch.float32)
    bad = dict(lo)
    bad[tensor] = change(case, lo)
    with pytest.raises(AssertionError, match=tensor.replace(".", r"\.") + ": own-norm gradient error"):
        GP.tensor_errors(list(hi), bad, hi, lo, TC.BAR_GRAD, zeros=TC.zeros(case), what="changed " + tensor,
                         nosignal=TC.no_signal(case, list(hi)), max_between=0)
