"""The gradient-parity rule of tests/grad_parity.py bites: on the CPU, from the oracle alone.  The fp32 oracle plays the device; a
zeroed, a 1 % scaled and a negated gradient tensor of the audio / video attention sites must each fail with the tensor named.
(The step-level GPU tests apply the same helper to the engine's gradients.)"""
import numpy as np
import pytest
import torch

from tests import grad_parity as GP

DIMS, B, TN = (24, 16, 20, 16), 4, (70, 9, 33, 6)
BAR = 2e-4
# The former rule (per-element rms below 1e-6 of the largest tensor's: only "as small on the device") at this case skipped 17 of the 83
# tensors.  Of the three changes below it ACCEPTED the zeroed fra2utt_0.input_proj.weight and the scaled
# cross_att_fra2utt_2.input_proj.bias (both under its floor) and rejected only the negated fra2utt_2.attention_context_vector.
CHANGES = (("fra2utt_0.input_proj.weight", lambda t: torch.zeros_like(t), True),
           ("cross_att_fra2utt_2.input_proj.bias", lambda t: t * 1.01, True),
           ("fra2utt_2.attention_context_vector", lambda t: -t, False))


@pytest.fixture(scope="module")
def case():
    from oracle import sdumc_oracle as O
    P = O.init_params(DIMS, seed=14)
    batch = O.synthetic_batch(B, TN, DIMS, seed=4)
    hi = GP.oracle_step_grads(P, batch, 31)
    lo = GP.oracle_step_grads(P, batch, 31, dtype=torch.float32)
    names = [k for k in P if not O.is_dead(k)]
    assert set(names) == set(hi) == set(lo) and len(names) == 83
    return names, hi, lo


def old_rule_accepts(names, got, ref, k, bar):
    """would the former rule (skip below 1e-6 G, then only rms of the error < 1e-5 G) have let tensor k of `got` through"""
    G = max(float(ref[n].norm()) / np.sqrt(ref[n].numel()) for n in names)
    d = float((got[k].double() - ref[k]).norm())
    if k in GP.old_rule_compared(names, ref):
        return d / float(ref[k].norm()) < bar
    return d / np.sqrt(ref[k].numel()) < 1e-5 * G


def test_fp32_oracle_as_device_passes_and_is_classified(case):
    names, hi, lo = case
    res = GP.tensor_errors(names, lo, hi, lo, BAR, what="toy, fp32 oracle as the device")
    assert len(res) == 81 and set(res.nosignal) == set(GP.NO_SIGNAL) and not res.zero and not res.between
    assert len(res.old_compared) == 66                  # what the former rule compared here
    assert max(res.values()) < BAR / 4


@pytest.mark.parametrize("name,change,old_accepted", CHANGES, ids=[c[0] for c in CHANGES])
def test_a_wrong_tensor_fails_by_name(case, name, change, old_accepted):
    names, hi, lo = case
    bad = dict(lo)
    bad[name] = change(lo[name])
    assert old_rule_accepts(names, bad, hi, name, BAR) == old_accepted
    with pytest.raises(AssertionError, match=name.replace(".", r"\.") + ": own-norm gradient error"):
        GP.tensor_errors(names, bad, hi, lo, BAR, what="changed " + name)


def test_caps_and_named_zeros(case):
    """the caps are the helper's own: an unnamed exact zero, a third no-signal tensor and a garbage no-signal tensor all fail"""
    names, hi, lo = case
    k = "fra2utt_1.input_proj.bias"
    hi0, lo0 = dict(hi), dict(lo)
    hi0[k], lo0[k] = torch.zeros_like(hi[k]), torch.zeros_like(lo[k])
    with pytest.raises(AssertionError, match="not named"):
        GP.tensor_errors(names, lo0, hi0, lo0, BAR)
    res = GP.tensor_errors(names, lo0, hi0, lo0, BAR, zeros=(k,))
    assert res.zero == [k] and k not in res
    big = dict(lo0)
    big[k] = torch.full_like(lo[k], 1e-3)               # a named zero must still be small on the device
    with pytest.raises(AssertionError, match="no signal"):
        GP.tensor_errors(names, big, hi0, lo0, BAR, zeros=(k,))
    noisy = dict(lo)
    noisy["cross_fused_query_mlp.0.weight"] = lo["cross_fused_query_mlp.0.weight"] * 1.5      # the two references disagree on a third tensor
    with pytest.raises(AssertionError, match="no-signal tensors beyond"):
        GP.tensor_errors(names, noisy, hi, noisy, BAR)
    between = dict(lo)
    k2 = "cross_attention_mlp.0.weight"                 # (the former rule skipped it: the raise applies)
    between[k2] = lo[k2] * (1 + 1e-3)
    res = GP.tensor_errors(names, between, hi, between, BAR)
    assert res.between == [k2] and 3.9e-3 < res.bars[k2] < 4.1e-3
    many = dict(lo)                                     # (three in between: past the cap unless the caller names all three)
    ks = (k2, "fra2utt_0.input_proj.weight", "cross_att_fra2utt_2.input_proj.bias")
    for k in ks:
        many[k] = lo[k] * (1 + 1e-3)
    with pytest.raises(AssertionError, match="in between, not named"):
        GP.tensor_errors(names, many, hi, many, BAR)
    with pytest.raises(AssertionError, match=r"not named: \[\('cross_att_fra2utt_2"):
        GP.tensor_errors(names, many, hi, many, BAR, between=ks[:2])
    assert GP.tensor_errors(names, many, hi, many, BAR, between=ks).between == sorted(ks, key=names.index)
    k3 = "fra2utt_2.attention_context_vector"           # (the former rule compared it: the flat bar stays)
    flat = dict(lo)
    flat[k3] = lo[k3] * (1 + 1e-3)
    with pytest.raises(AssertionError, match=k3):
        GP.tensor_errors(names, flat, hi, flat, BAR)


def test_close_norm_keeps_the_absolute_bar_for_two_names_only():
    tiny = torch.full((8,), 1e-9)
    assert GP.close_norm(tiny * 3, tiny, 2e-4, "orgin_linear_change.2.bias", "case") == 0.0
    with pytest.raises(AssertionError, match="case: frame_dim_reshape_1.bias"):
        GP.close_norm(tiny * 3, tiny, 2e-4, "frame_dim_reshape_1.bias", "case")
    with pytest.raises(AssertionError):                 # (the name decides, not the wording of the case)
        GP.close_norm(tiny * 3, tiny, 2e-4, "frame_dim_reshape_1.bias", "beside orgin_linear_change.2.bias")
    assert GP.close_norm(torch.zeros(8), torch.zeros(8), 2e-4, "frame_dim_reshape_1.bias") == 0.0
    with pytest.raises(AssertionError):
        GP.close_norm(torch.ones(8), torch.zeros(8), 2e-4, "frame_dim_reshape_1.bias")
