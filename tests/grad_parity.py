"""One rule for "every gradient tensor against its OWN norm", shared by the step-level parity tests; a plain module, no fixtures.

A device gradient `got` is judged against a high-precision reference `ref_hi`.  How well a tensor CAN be known is measured on the
reference side alone, from a second, lower-precision evaluation `ref_lo` of the same graph:

    e_ref[k] = |ref_lo[k] - ref_hi[k]| / |ref_hi[k]|

      fp32 storage    ref_hi = the fp64 oracle, ref_lo = the fp32 oracle
      bf16 storage    both the rounding emulation (oracle/bf16_storage.py), with fp64 and with fp32 parameters

No GPU and no code under test takes part in e_ref.  Classes, with `bar` the caller's own-norm tolerance:

    exact zero    |ref_hi| == 0 (T = 1: the softmax gradient vanishes)   the device tensor must be small: rms < 1e-5 G
    no signal     e_ref > 0.1                                            the same check
    held          e_ref <= bar / 4                                       own-norm error < bar
    in between    bar / 4 < e_ref <= 0.1                                 own-norm error < max(bar, 4 e_ref)

G is the largest per-element rms of a reference tensor.  The factor 4: two fp32 evaluations that differ in summation order and in
tanh / exp sit about 2 e_ref apart, and a further factor 2 covers the device's different order.  The raise applies only to tensors
the former rule (per-element rms below 1e-6 G: skipped) did not compare; a tensor it compared keeps the flat bar whatever its e_ref.

Caps, asserted on every call: no-signal tensors are a subset of NO_SIGNAL (the RnC head's biases: the loss is translation invariant,
their gradient is a sum that cancels to rounding noise); at most MAX_BETWEEN tensors in between, or else only tensors that the
caller names one by one; exact zeros only where the caller names them."""
import numpy as np
import torch

NO_SIGNAL = frozenset(("orgin_linear_change.0.bias", "orgin_linear_change.2.bias"))
MAX_BETWEEN = 2
SMALL = 1e-5             # zero / no-signal tensors: rms of the device tensor's error below SMALL * G
OLD_SKIP = 1e-6          # the former rule: tensors whose per-element rms is below OLD_SKIP * G were not compared


class TensorErrors(dict):
    """name -> own-norm error of every compared tensor (held + in between); the classes and the per-tensor bars as attributes"""
    bars = e_ref = None
    between = nosignal = zero = old_compared = ()
    line = ""


def _rms(t):
    return float(t.double().norm()) / np.sqrt(t.numel())


def old_rule_compared(names, ref):
    """the tensors the former skip rule compared: per-element rms of the reference at least 1e-6 of the largest tensor's"""
    rms = {k: _rms(ref[k]) for k in names}
    G = max(rms.values())
    return [k for k in names if rms[k] >= OLD_SKIP * G]


def tensor_errors(lay, got, ref_hi, ref_lo, bar, zeros=(), what="", between=(), nosignal=NO_SIGNAL, max_between=MAX_BETWEEN,
                  keep_old=True):
    """Own-norm error of every live tensor of `got` against `ref_hi`, each held to its class's bar (module docstring); prints one
    summary line and returns a TensorErrors.  lay: a ParamLayout, or the list of tensor names.  zeros: the tensors the caller
    expects to be exactly zero in the reference.  between: where a case has more than MAX_BETWEEN tensors in between, the caller
    names them all, as it names its zeros, and says why; the class may then hold those and no other.  nosignal / max_between: the two
    caps, for a caller whose graph is not the step's (default: the module's NO_SIGNAL and MAX_BETWEEN).  keep_old=False: a family the
    former skip rule never applied to (tests/attn_pool_cases.py): the class of every tensor follows from its e_ref alone.  bar: one
    own-norm tolerance, or name -> tolerance where every tensor has its own (tests/gemm_cases.py); the classes and every assert are
    the same, each tensor against its own bar."""
    names = list(lay.live_names()) if hasattr(lay, "live_names") else list(lay)
    bar_of = bar if isinstance(bar, dict) else dict.fromkeys(names, bar)
    assert set(names) <= set(ref_hi) and set(names) <= set(ref_lo) and set(names) <= set(got)
    hi = {k: ref_hi[k].detach().cpu().double() for k in names}
    G = max(_rms(hi[k]) for k in names)
    old = set(old_rule_compared(names, hi))
    res = TensorErrors()
    res.bars, res.e_ref, res.between, res.nosignal, res.zero, res.old_compared = {}, {}, [], [], [], [k for k in names if k in old]
    small_errs, fails = {}, []
    for k in names:
        g = got[k].detach().cpu().double().reshape(hi[k].shape)
        d = float((g - hi[k]).norm())
        if not np.isfinite(d):
            fails.append(f"{k}: the device gradient is not finite")
            d = float("inf")
        ref = float(hi[k].norm())
        if ref == 0.0:
            res.zero.append(k)
            small_errs[k] = d / np.sqrt(hi[k].numel())
            continue
        e_ref = float((ref_lo[k].detach().cpu().double().reshape(hi[k].shape) - hi[k]).norm()) / ref
        res.e_ref[k] = e_ref
        if (keep_old and k in old) or e_ref <= bar_of[k] / 4:
            res.bars[k] = bar_of[k]
        elif e_ref <= 0.1:
            res.between.append(k)
            res.bars[k] = max(bar_of[k], 4 * e_ref)
        else:
            res.nosignal.append(k)
            small_errs[k] = d / np.sqrt(hi[k].numel())
            continue
        res[k] = d / ref
    vals = sorted(res.values())
    worst = max(res, key=res.get) if res else ""
    res.line = ("grad parity %s: %d of %d tensors compared, %d in between%s, %d no-signal, %d zero; median %.3g, p90 %.3g, worst %s = %.3g"
                % (what, len(res), len(names), len(res.between),
                   " (" + ", ".join("%s e_ref %.2g" % (k, res.e_ref[k]) for k in res.between) + ")" if res.between else "",
                   len(res.nosignal), len(res.zero), float(np.median(vals)) if vals else 0.0,
                   vals[int(0.9 * len(vals))] if vals else 0.0, worst, res[worst] if res else 0.0))
    print(res.line)
    for k, e in res.items():
        if not e < res.bars[k]:
            fails.append(f"{k}: own-norm gradient error {e:.3e}, bar {res.bars[k]:.3g} (|g| = {float(hi[k].norm()):.3e}, e_ref = {res.e_ref[k]:.2e})")
    for k, e in small_errs.items():
        if not e < SMALL * G:
            fails.append(f"{k}: the reference carries no signal here; device error rms {e:.3e} is not below {SMALL * G:.3e}")
    assert not fails, f"{what}: " + "; ".join(fails)
    assert set(res.nosignal) <= set(nosignal), f"{what}: no-signal tensors beyond the named ones: {sorted(set(res.nosignal) - set(nosignal))}"
    assert len(res.between) <= max_between or set(res.between) <= set(between), \
        f"{what}: {len(res.between)} tensors in between, not named: {[(k, res.e_ref[k]) for k in res.between if k not in set(between)]}"
    assert set(res.zero) <= set(zeros), f"{what}: exactly zero in the reference but not named: {sorted(set(res.zero) - set(zeros))}"
    return res


def close_norm(got, want, tol, name, what=""):
    """|got - want| / |want| < tol.  The only tensors with an absolute bar instead: one that is EXACTLY zero in the reference, and the
    RnC head's biases (NO_SIGNAL) where their reference norm is below 1e-7 -- by name, not by size: any other tensor that small is
    held to its own norm like the rest.  name: the tensor's name, which alone decides the class (anything that is no parameter
    name, an input gradient say, is held to its own norm); what: the case, for the message only.  Returns the error."""
    msg = f"{what}: {name}" if what else name
    got, want = got.detach().cpu().double(), want.detach().cpu().double().reshape(got.shape)
    ref = float(want.norm())
    if ref == 0.0 or (name in NO_SIGNAL and ref < 1e-7):
        assert float(got.norm()) < 1e-6, msg
        return 0.0
    err = float((got - want).norm()) / ref
    if ref < 1e-7:
        print("grad parity %s: |g| = %.3g lay under the former absolute floor of 1e-7; own-norm error %.3g" % (msg, ref, err))
    assert err < tol, f"{msg}: relative error {err:.3e} (norms {float(got.norm()):.3e} vs {ref:.3e})"
    return err


def oracle_step_grads(P, batch, seed, dtype=torch.float64, lengths=None, st=None):
    """gradients of one oracle train step (Philox masks, step 0) with parameters and batch in `dtype`; P is left unchanged"""
    from oracle import sdumc_oracle as O
    Pd = {k: v.to(dtype) for k, v in P.items()}
    return O.train_step(Pd, {}, *[t.to(dtype) for t in batch], mode="philox", seed=seed, step=0, lengths=lengths, st=st)[2]
