"""Drop-in replacement of the optimizer line of the reference's training loop
(main_frame_val_text_missing.py:317, `torch.optim.Adam(model.parameters(), lr=..., weight_decay=...)`; stepped at
:150): the same signature, param_groups, state_dict format and LambdaLR behaviour, with the whole step as ONE
sdumc_adam_multi launch over the per-parameter gradient tensors autograd left in `p.grad`.  clip_grad_norm_ is the line that
often stands in front of it, torch.nn.utils.clip_grad_norm_, as three launches over the same tensors and no host synchronisation.
AdamW, and Adam(..., decoupled_weight_decay=True), are torch.optim.AdamW the same way: ONE sdumc_adamw_multi launch.

The one divergence from torch.optim.Adam: ONE step count is shared by all parameters (torch keeps one per
parameter).  That is the model's own situation -- every live parameter receives a gradient on every step -- and it
is enforced: the parameters that carry a gradient at the first step() (or the ones a loaded state_dict holds state
for) are the set of this optimizer, and a later step() that sees another set raises SdumcError instead of letting
the bias corrections of some parameters drift.  Parameters whose grad is None at that first step are skipped and
never get state, as in torch.

There is no CPU or eager fallback: fp32 CUDA parameters on one device, or SdumcError.
"""
import torch

from . import _lib, ops
from ._lib import SdumcError


def _ceil4(n):
    return (n + 3) & ~3


_clip_cache = {}      # the last gradient set's pointer tuple -> (segment table, scratch)


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ over the .grad tensors of `parameters` (sdumc_grad_guard_multi): the total L2 norm in fp64 and a
    fixed order, coef = min(1, max_norm / (norm + 1e-6)), every gradient scaled in place by one fp32 multiply -- untouched, bit for
    bit, when coef == 1.  Three launches whatever the number of tensors, nothing synchronises.  Returns the total norm BEFORE
    clipping as a 0-dim device tensor (torch's return value).  Non-finite gradients behave as in torch with
    error_if_nonfinite=False: a NaN norm gives a NaN coefficient.  foreach is accepted and ignored.
    Not built, SdumcError: norm_type != 2, error_if_nonfinite=True (it would cost the synchronisation this call exists to avoid),
    more than _lib.TENSOR_NORMS_MAX_SEGS gradient tensors; and there is no fallback for CPU, non-fp32, sparse or non-contiguous
    gradients.  max_norm: a positive finite Python number."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    if isinstance(norm_type, bool) or not isinstance(norm_type, (int, float)) or float(norm_type) != 2.0:
        raise SdumcError(f"sdumc_amd.optim.clip_grad_norm_: norm_type={norm_type!r} is not built (the L2 norm only)")
    if error_if_nonfinite:
        raise SdumcError("sdumc_amd.optim.clip_grad_norm_: error_if_nonfinite=True is not built (it needs a host synchronisation)")
    if max_norm is None:
        raise SdumcError("sdumc_amd.optim.clip_grad_norm_: max_norm must be a positive finite number")
    clip, _ = _lib.guard_args(max_norm, False)
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)      # (torch's answer for no gradients)
    dev = grads[0].device
    for g in grads:
        if not g.is_cuda or g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous():
            raise SdumcError("sdumc_amd.optim.clip_grad_norm_: expected dense contiguous fp32 CUDA gradients (there is no fallback)")
        if g.device != dev:
            raise SdumcError("sdumc_amd.optim.clip_grad_norm_: the gradients are on different devices")
    if len(grads) > _lib.TENSOR_NORMS_MAX_SEGS:
        raise SdumcError(f"sdumc_amd.optim.clip_grad_norm_: more than {_lib.TENSOR_NORMS_MAX_SEGS} gradient tensors is not built")
    key = (dev,) + tuple(g.data_ptr() for g in grads) + tuple(g.numel() for g in grads)
    with torch.cuda.device(dev):
        hit = _clip_cache.get(key)
        if hit is None:
            segs = (_lib.NormSeg * len(grads))()
            for sg, g in zip(segs, grads):
                sg.x, sg.y, sg.count = g.data_ptr(), None, g.numel()
            nb = int(_lib.lib.sdumc_grad_guard_multi_scratch_bytes(segs, len(grads)))
            if nb == 0:
                raise SdumcError("sdumc_grad_guard_multi_scratch_bytes refused the gradient table")
            _clip_cache.clear()
            hit = _clip_cache[key] = (segs, torch.empty(nb, dtype=torch.uint8, device=dev))
        segs, scratch = hit
        guard = torch.empty(4, device=dev)
        _lib.check(_lib.lib.sdumc_grad_guard_multi(segs, len(grads), clip, _lib.ptr(scratch), scratch.numel(), _lib.ptr(guard),
                                                   _lib.current_stream()), "sdumc_grad_guard_multi")
    return guard[0]


_ema_cache = {}       # the last tensor set's pointer tuple -> segment table


@torch.no_grad()
def ema_update_(ema_params, params, decay):
    """ema_params[i] <- torch.lerp(ema_params[i], params[i], 1 - decay) for every pair, as ONE launch per 96 tensors
    (sdumc_ema_multi): what torch.optim.swa_utils.get_ema_multi_avg_fn(decay) does with torch._foreach_lerp_, with the weight
    fp32(1 - decay) rounded once from the double.  Nothing synchronises; the tensors may be views at any element offset of a larger
    one.  decay: a Python number in [0, 1].  There is no fallback: dense contiguous fp32 CUDA tensors of equal sizes on one device, or
    SdumcError."""
    on, d, _ = _lib.ema_args(decay, False)
    if not on:
        raise SdumcError("sdumc_amd.optim.ema_update_: decay must be a number in [0, 1]")
    ema_params, params = list(ema_params), list(params)
    if len(ema_params) != len(params):
        raise SdumcError(f"sdumc_amd.optim.ema_update_: {len(ema_params)} averaged tensors for {len(params)} parameters")
    if not params:
        return
    dev = ema_params[0].device
    for a, p in zip(ema_params, params):
        for t in (a, p):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.is_sparse or t.dtype != torch.float32 or not t.is_contiguous() \
                    or t.device != dev:
                raise SdumcError("sdumc_amd.optim.ema_update_: expected dense contiguous fp32 CUDA tensors on one device (there is "
                                 "no fallback)")
        if a.numel() != p.numel() or a.numel() == 0:
            raise SdumcError(f"sdumc_amd.optim.ema_update_: an averaged tensor of {a.numel()} elements for a parameter of {p.numel()}")
    key = (dev,) + tuple(t.data_ptr() for t in ema_params) + tuple(t.data_ptr() for t in params) + tuple(t.numel() for t in params)
    with torch.cuda.device(dev):
        segs = _ema_cache.get(key)
        if segs is None:
            _ema_cache.clear()
            segs = _ema_cache[key] = ops.ema_segments(ema_params, params)
        ops.ema_multi(ema_params, params, 1.0 - d, segs=segs)


def get_ema_multi_avg_fn(decay=0.999):
    """torch.optim.swa_utils.get_ema_multi_avg_fn with ema_update_ inside:
    AveragedModel(model, multi_avg_fn=sdumc_amd.optim.get_ema_multi_avg_fn(0.999)) makes its whole update one launch."""
    on, d, _ = _lib.ema_args(decay, False)
    if not on:
        raise SdumcError("sdumc_amd.optim.get_ema_multi_avg_fn: decay must be a number in [0, 1]")

    def ema_update(ema_param_list, current_param_list, _num_averaged):
        ema_update_(ema_param_list, current_param_list, d)

    return ema_update


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        for name, on in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable),
                         ("differentiable", differentiable)):
            if on:
                raise SdumcError(f"sdumc_amd.optim.Adam: {name}=True is not built (the reference uses none of them)")
        if isinstance(lr, torch.Tensor):
            raise SdumcError("sdumc_amd.optim.Adam: lr must be a Python number (a tensor lr would cost a sync per step)")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay:
            raise ValueError(f"invalid lr / eps / weight_decay: {lr}, {eps}, {weight_decay}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid betas: {betas}")
        if not isinstance(decoupled_weight_decay, bool):
            raise SdumcError(f"sdumc_amd.optim.Adam: decoupled_weight_decay must be True or False, not {decoupled_weight_decay!r}")
        # the keys torch.optim.Adam writes (and checkpoint.adam_state_from_flat with it); foreach / fused are accepted and ignored
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=decoupled_weight_decay)
        self._m = self._v = self._hyper = None      # flat fp32 moments [state_len], device {lr, t, lr/(1-b1^t), sqrt(1-b2^t)}
        self._live = None                            # the parameters of this optimizer's set, in param_groups order
        self._offsets = None                         # their offsets into the flat moments (multiples of 4: 16-byte aligned)
        self._step_t = torch.tensor(0.0)             # the shared step count (host mirror of hyper[1])
        self._lr_written = None
        self._key = self._segs = None                # pointer tuple -> the ctypes segment table built from it
        super().__init__(params, defaults)

    def add_param_group(self, param_group):
        if len(self.param_groups) >= 1:
            raise SdumcError("sdumc_amd.optim.Adam: one param group only (one lr / weight_decay for the whole model, main :317)")
        super().add_param_group(param_group)

    # ------------------------------------------------------------------ state
    def _name(self, p):
        i = next(i for i, q in enumerate(self.param_groups[0]["params"]) if q is p)
        names = self.param_groups[0].get("param_names")
        return f"parameter {i}" + (f" ({names[i]})" if names else "") + f" of shape {tuple(p.shape)}"

    def _loaded_set(self):
        """Parameters a load_state_dict() before the first step installed state for (torch-format entries in self.state)."""
        return [p for p in self.param_groups[0]["params"] if "exp_avg" in self.state.get(p, ())]

    def _check_set(self, live):
        want = self._live if self._live is not None else (self._loaded_set() or live)
        if len(want) != len(live) or any(a is not b for a, b in zip(want, live)):
            ids = {id(p) for p in live}
            missing = [p for p in want if id(p) not in ids]
            ids = {id(p) for p in want}
            extra = [p for p in live if id(p) not in ids]
            what = (f"{self._name(missing[0])} has no gradient now" if missing else
                    f"{self._name(extra[0])} has a gradient now but had none")
            raise SdumcError("sdumc_amd.optim.Adam keeps one step count for all parameters, so every step must see the "
                             f"same parameters with gradients as the first one (or the loaded state): {what}")

    def _init_state(self, live):
        dev = live[0].device
        offsets, total = [], 0
        for p in live:
            offsets.append(total)
            total = _ceil4(total + p.numel())
        m = torch.zeros(total, device=dev)
        v = torch.zeros(total, device=dev)
        step = None
        for p, off in zip(live, offsets):       # state a load_state_dict() left before the first step
            st = self.state.get(p)
            if st is not None and "exp_avg" in st:
                n = p.numel()
                m[off:off + n].copy_(st["exp_avg"].reshape(-1))
                v[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
                step = self._shared_step(step, st["step"], p)
        self._step_t = torch.tensor(float(step or 0))
        self._m, self._v = m, v
        self._hyper = torch.tensor([0.0, float(self._step_t), 0.0, 0.0], device=dev)
        self._lr_written = None
        self._live, self._offsets = list(live), offsets
        for p, off in zip(live, offsets):
            n = p.numel()
            self.state[p] = {"step": self._step_t, "exp_avg": m[off:off + n].view(p.shape),
                             "exp_avg_sq": v[off:off + n].view(p.shape)}

    def _shared_step(self, step, value, p):
        value = float(value)
        if step is not None and value != step:
            raise SdumcError("sdumc_amd.optim.Adam keeps one step count for all parameters; the loaded state has "
                             f"step {value} for {self._name(p)} and {step} before it")
        return value

    def _validate(self, live, grads):
        dev = live[0].device
        for p, g in zip(live, grads):
            if not p.is_cuda or p.dtype != torch.float32 or p.device != dev:
                raise SdumcError(f"sdumc_amd.optim.Adam updates fp32 CUDA parameters on one device (no CPU fallback): "
                                 f"{self._name(p)} is {p.dtype} on {p.device}")
            if g.is_sparse or g.dtype != torch.float32 or g.device != dev or g.shape != p.shape:
                raise SdumcError(f"sdumc_amd.optim.Adam: the gradient of {self._name(p)} must be a dense fp32 tensor of the "
                                 "parameter's shape on its device")
            if not p.is_contiguous():
                raise SdumcError(f"sdumc_amd.optim.Adam: {self._name(p)} is not contiguous")
        if self._m is not None and self._m.device != dev:
            raise SdumcError(f"sdumc_amd.optim.Adam: the parameters moved to {dev}, the optimizer state lives on {self._m.device}")

    # ------------------------------------------------------------------ step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        live, grads = [], []
        for p in group["params"]:
            g = p.grad
            if g is not None:
                live.append(p)
                grads.append(g if g.is_contiguous() else g.contiguous())
        if not live:
            return loss
        self._check_set(live)
        # the table is rebuilt only when a pointer moved (zero_grad(set_to_none=True) moves the gradients, model.cuda() and the
        # model's _reflatten move the parameters); new pointers = tensors not seen before: checked then
        key = tuple([p.data_ptr() for p in live] + [g.data_ptr() for g in grads])
        if key != self._key:
            self._validate(live, grads)
            if self._m is None:
                self._init_state(live)
            self._segs = ops.adam_segments(live, grads, self._offsets)
            self._key = key
        lr = group["lr"]
        if isinstance(lr, torch.Tensor):
            raise SdumcError("sdumc_amd.optim.Adam: group['lr'] must be a Python number")
        with torch.cuda.device(self._m.device):
            if lr != self._lr_written:           # LambdaLR rewrites group['lr'] once per epoch: a device-side fill, no sync
                self._hyper[0] = lr
                self._lr_written = lr
            beta1, beta2 = group["betas"]
            # the group's flag decides, as in torch: the constructor's, or the one a loaded state_dict brought
            multi = ops.adamw_multi if group.get("decoupled_weight_decay") else ops.adam_multi
            multi(live, grads, self._m, self._v, self._offsets, self._hyper, beta1, beta2, group["eps"],
                  group["weight_decay"], segs=self._segs)
        self._step_t += 1
        return loss

    # ------------------------------------------------------------------ checkpoint interchange
    def state_dict(self):
        """torch.optim.Adam's format.  Every parameter gets a `step` tensor of its own (here they share one): an optimizer
        that loads the dict and counts per parameter must not find them aliased."""
        sd = super().state_dict()
        sd["state"] = {k: ({**st, "step": st["step"].clone()} if isinstance(st, dict) and "step" in st else st)
                       for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """Accepts torch.optim.Adam.state_dict(), this class's own and checkpoint.adam_state_from_flat(...).  Before the
        first step() (resume does that) the state waits in torch's format and moves into the flat buffers at that step."""
        live, offsets = self._live, self._offsets
        super().load_state_dict(state_dict)
        if len(self.param_groups) != 1:
            raise SdumcError("sdumc_amd.optim.Adam: one param group only")
        group = self.param_groups[0]
        for name in ("amsgrad", "maximize", "capturable", "differentiable"):
            if group.get(name):
                raise SdumcError(f"sdumc_amd.optim.Adam: the loaded param group has {name}=True, which is not built")
        loaded = self._loaded_set()
        step = None
        for p in loaded:
            step = self._shared_step(step, self.state[p]["step"], p)
        self._key = self._segs = None
        if live is None:
            self._step_t = torch.tensor(float(step or 0))
            for p in loaded:                       # (an own `step` per entry again, whatever the dict aliased)
                self.state[p]["step"] = self._step_t
            return
        if len(loaded) != len(live) or any(a is not b for a, b in zip(loaded, live)):
            raise SdumcError("sdumc_amd.optim.Adam: the loaded state holds another set of parameters than this optimizer "
                             "has been stepping")
        with torch.no_grad():
            for p, off in zip(live, offsets):
                st, n = self.state[p], p.numel()
                self._m[off:off + n].copy_(st["exp_avg"].reshape(-1))
                self._v[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
            self._step_t = torch.tensor(float(step or 0))
            self._hyper[1] = float(self._step_t)       # device-side fill
            for p, off in zip(live, offsets):
                n = p.numel()
                self.state[p] = {"step": self._step_t, "exp_avg": self._m[off:off + n].view(p.shape),
                                 "exp_avg_sq": self._v[off:off + n].view(p.shape)}


class AdamW(Adam):
    """torch.optim.AdamW's signature and defaults (weight_decay=1e-2): Adam above with decoupled_weight_decay=True, so one group, one
    launch (sdumc_adamw_multi), one step count, the same refusals, and torch's param_groups keys and state_dict format."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, decoupled_weight_decay=True)
