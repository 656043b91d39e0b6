"""ctypes binding of libsdumc_hip.so (include/sdumc_hip.h).

There is NO fallback: if the shared library is missing or a symbol is absent the
import of any product module raises.  PyTorch-ROCm tensors provide device
memory and streams; every pointer crossing this boundary is `tensor.data_ptr()`.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SDUMC_LIB") or os.path.join(_HERE, "csrc", "libsdumc_hip.so")   # override: A/B of builds

MAX_GROUPS = 8
D, H, NQ, RNC_DIM, N_SITES = 256, 128, 7, 64, 35
NT, NN, TN = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2

c_float_p = C.c_void_p  # device pointers travel as integers


class Dropout(C.Structure):
    _fields_ = [("enabled", C.c_uint32), ("site", C.c_uint32), ("threshold", C.c_uint32), ("scale", C.c_float),
                ("rows", C.c_uint32), ("width", C.c_uint32), ("samples", C.c_uint32), ("sample0", C.c_uint32),
                ("call0", C.c_uint32), ("stream0", C.c_uint32), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32),
                ("dev_state", C.c_void_p), ("bits", C.c_void_p)]


class Gemm(C.Structure):
    _fields_ = [("layout", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("groups", C.c_int32),
                ("A", C.c_void_p * MAX_GROUPS), ("B", C.c_void_p * MAX_GROUPS),
                ("C", C.c_void_p * MAX_GROUPS), ("bias", C.c_void_p * MAX_GROUPS),
                ("lda", C.c_int32), ("ldb", C.c_int32), ("ldc", C.c_int32),
                ("a_row_mod", C.c_int32), ("b_row_mod", C.c_int32),
                ("a_drop", Dropout), ("b_drop", Dropout),
                ("act", C.c_int32), ("c_drop", Dropout), ("c_drop_group_stride", C.c_int32),
                ("accumulate", C.c_int32), ("splitk", C.c_int32), ("tile", C.c_int32),
                ("ab_drop_group_stride", C.c_int32), ("ab_drop_bits", C.c_void_p * MAX_GROUPS),
                ("c_mask_y", C.c_void_p * MAX_GROUPS), ("c_mask_scale", C.c_float),
                ("colsum_a", C.c_void_p * MAX_GROUPS),
                ("bf16", C.c_int32),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("batch", C.c_int32),
                ("stride_a", C.c_int64), ("stride_b", C.c_int64), ("stride_c", C.c_int64)]


class GemmBf16(C.Structure):
    _fields_ = [("layout", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("groups", C.c_int32),
                ("A", C.c_void_p * MAX_GROUPS), ("B", C.c_void_p * MAX_GROUPS), ("C", C.c_void_p * MAX_GROUPS),
                ("bias", C.c_void_p * MAX_GROUPS), ("colsum_a", C.c_void_p * MAX_GROUPS),
                ("lda", C.c_int32), ("ldb", C.c_int32), ("ldc", C.c_int32),
                ("a_row_mod", C.c_int32), ("b_row_mod", C.c_int32),
                ("act", C.c_int32), ("accumulate", C.c_int32), ("c_bf16", C.c_int32), ("splitk", C.c_int32),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class GGProblem(C.Structure):
    _fields_ = [("A", C.c_void_p * 2), ("B", C.c_void_p * 2), ("b_bits", C.c_void_p * 2),
                ("K", C.c_int32 * 2), ("b_row_mod", C.c_int32 * 2),
                ("C", C.c_void_p), ("colsum_a", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("lda", C.c_int32), ("ldb", C.c_int32), ("ldc", C.c_int32),
                ("bits_qw", C.c_int32), ("b_scale", C.c_float), ("accumulate", C.c_int32), ("b_map", C.c_void_p * 2)]


class GemmP3(C.Structure):
    _fields_ = [("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("A", C.c_void_p), ("B", C.c_void_p), ("lda", C.c_int64), ("ldb", C.c_int64),
                ("a_row_mod", C.c_int32), ("A2", C.c_void_p), ("a2_row0", C.c_int32),
                ("a_bits", C.c_void_p), ("bits_qw", C.c_int32), ("a_scale", C.c_float),
                ("bias", C.c_void_p), ("act", C.c_int32),
                ("C", C.c_void_p), ("ldc", C.c_int32), ("C_p3", C.c_void_p), ("ldc_p3", C.c_int64),
                ("splitk", C.c_int32), ("tile_m", C.c_int32),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("a_map", C.c_void_p), ("a2_map", C.c_void_p), ("a_map_rows", C.c_int64)]


class GemmB1(C.Structure):
    _fields_ = [("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("A", C.c_void_p), ("B", C.c_void_p), ("lda", C.c_int64), ("ldb", C.c_int64),
                ("a_row_mod", C.c_int32), ("A2", C.c_void_p), ("a2_row0", C.c_int32),
                ("bias", C.c_void_p), ("act", C.c_int32),
                ("C", C.c_void_p), ("ldc", C.c_int32), ("c_bf16", C.c_int32), ("splitk", C.c_int32),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("a_map", C.c_void_p), ("a2_map", C.c_void_p), ("a_map_rows", C.c_int64)]


class RowsProblem(C.Structure):
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("a_bits", C.c_void_p), ("bias", C.c_void_p), ("C", C.c_void_p),
                ("M", C.c_int32), ("lda", C.c_int32), ("ldb", C.c_int32), ("ldc", C.c_int32), ("a_row_mod", C.c_int32),
                ("a_scale", C.c_float), ("accumulate", C.c_int32), ("act", C.c_int32),
                ("pool_w", C.c_void_p), ("pool_g", C.c_void_p), ("pool_nq", C.c_int32), ("pool_T", C.c_int32),
                ("c_bits", C.c_void_p), ("c_scale", C.c_float), ("fold", C.c_int32)]


class AttnPool(C.Structure):
    _fields_ = [("V", C.c_int32), ("T", C.c_int32), ("nq", C.c_int32), ("x_samples", C.c_int32),
                ("x", C.c_void_p), ("keys", C.c_void_p), ("q", C.c_void_p), ("q_stride", C.c_int64),
                ("scale", C.c_float), ("x_drop", Dropout), ("out_drop", Dropout),
                ("attn", C.c_void_p), ("pooled", C.c_void_p), ("out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("dim", C.c_int32),
                ("lengths", C.c_void_p), ("bf16", C.c_int32), ("tickets", C.c_void_p), ("partial_only", C.c_int32)]


class Umca(C.Structure):
    _fields_ = [("a", AttnPool), ("w_in", C.c_void_p), ("b_in", C.c_void_p), ("x_p3", C.c_void_p), ("w_in_p3f", C.c_void_p)]


class AttnPoolBwd(C.Structure):
    _fields_ = [("f", AttnPool), ("dout", C.c_void_p), ("dz", C.c_void_p), ("dxd", C.c_void_p),
                ("dq", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("dq_sum", C.c_void_p),
                ("dout_masked", C.c_void_p)]


class DropSum(C.Structure):
    _fields_ = [("terms", C.c_int32), ("g", C.c_void_p * 8), ("drop", Dropout * 8),
                ("stream_idx", C.c_int32 * 8), ("samples", C.c_int32), ("T", C.c_int32), ("dx", C.c_void_p),
                ("bf16", C.c_int32)]


class NetDims(C.Structure):
    _fields_ = [("B", C.c_int32), ("streams", C.c_int32),
                ("Ta", C.c_int32), ("Tv", C.c_int32), ("Tt", C.c_int32 * 2),
                ("da", C.c_int32), ("dt", C.c_int32), ("dv", C.c_int32),
                ("train", C.c_int32), ("sample0", C.c_int32),
                ("p_frame", C.c_double), ("p_mlp", C.c_double), ("bf16", C.c_int32)]


class NetIO(C.Structure):
    _fields_ = [("audio", C.c_void_p), ("video", C.c_void_p), ("text", C.c_void_p * 2),
                ("params", C.c_void_p), ("rng_state", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                # outputs, each [streams*B, ...]
                ("vals", C.c_void_p), ("fused", C.c_void_p), ("rnc", C.c_void_p),
                ("text_hidden", C.c_void_p), ("cross_text", C.c_void_p),
                ("lengths", C.c_void_p * 4),
                ("audio_p3", C.c_void_p), ("video_p3", C.c_void_p), ("text_p3", C.c_void_p * 2),   # optional bf16-plane copies of the features
                ("row_map", C.c_void_p * 4),      # optional: the features are a resident store's packed tensors, read in place through these maps
                ("store_rows", C.c_int64 * 4),    # ... and those tensors' row counts (0 = unknown)
                ("bits_next", C.c_void_p), ("bits_phase", C.c_int32),   # optional: two sets of keep-bits, the next call's generated in this call's middle
                ("bits_next_bytes", C.c_size_t), ("bits_next_dims", C.c_void_p),   # its capacity (0 = this call's dims) / dims of the NEXT call (NULL = the same)
                ("prefetch", C.c_void_p), ("prefetch_workgroups", C.c_int32),      # optional: the NEXT batch's gather descriptor, issued in this call's middle
                ("ctx", C.c_void_p)]          # optional caller-owned execution context (sdumc_ctx_create); None = device default


class NetGrads(C.Structure):
    _fields_ = [("d_vals", C.c_void_p), ("d_fused", C.c_void_p), ("d_rnc", C.c_void_p),
                ("d_text_hidden", C.c_void_p), ("d_cross_text", C.c_void_p),
                ("grads", C.c_void_p),
                # optional input-feature gradients (all None = today's call): [B, T, d] fp32 outputs + the packed frame weights' scratch
                ("d_audio", C.c_void_p), ("d_video", C.c_void_p), ("d_text", C.c_void_p * 2),
                ("feat_scratch", C.c_void_p), ("feat_scratch_bytes", C.c_size_t)]


class FrameDx(C.Structure):
    _fields_ = [("M", C.c_int32), ("N", C.c_int32), ("A", C.c_void_p), ("W", C.c_void_p), ("W_frag", C.c_void_p), ("C", C.c_void_p),
                ("ldw", C.c_int64), ("ldc", C.c_int64), ("lengths", C.c_void_p), ("T", C.c_int32),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


def _guard_abi():
    """False only for an A/B against an older build (SDUMC_LIB, tools/grad_guard_bench.py) from before sdumc_grad_guard: that library
    reads sdumc_step_cfg WITHOUT the four guard fields, which sit in the struct's middle, so StepCfg leaves them out for it."""
    if not os.environ.get("SDUMC_LIB") or not os.path.exists(LIB_PATH):
        return True
    return hasattr(C.CDLL(LIB_PATH), "sdumc_grad_guard")


GUARD_ABI = _guard_abi()
_GUARD_FIELDS = [("clip_norm", C.c_float), ("skip_nonfinite", C.c_int32), ("guard", C.c_void_p), ("guard_scratch", C.c_void_p)]


RATES_MAX_SEGS = 96


class RateSeg(C.Structure):         # sdumc_rate_seg: elements [offset, offset + n) of the bucket, their scales, frozen or not
    _fields_ = [("offset", C.c_int64), ("n", C.c_int64), ("lr_scale", C.c_float), ("wd_scale", C.c_float), ("frozen", C.c_int32)]


class TensorRates(C.Structure):     # sdumc_tensor_rates: sdumc_step_cfg.rates, indexed by live tensor in sdumc_param_table order
    _fields_ = [("n", C.c_int32), ("lr_scale", C.c_float * RATES_MAX_SEGS), ("wd_scale", C.c_float * RATES_MAX_SEGS),
                ("frozen", C.c_uint8 * RATES_MAX_SEGS)]


def _rates_abi():
    """False only for an A/B against an older build (SDUMC_LIB, tools/rates_bench.py) from before sdumc_adam_step_rates: that library
    reads sdumc_step_cfg WITHOUT the rates pointer, which sits in the struct's middle, so StepCfg leaves it out for it."""
    if not os.environ.get("SDUMC_LIB") or not os.path.exists(LIB_PATH):
        return True
    return hasattr(C.CDLL(LIB_PATH), "sdumc_adam_step_rates")


RATES_ABI = _rates_abi()
_RATES_FIELDS = [("rates", C.POINTER(TensorRates))]


def _ema_abi():
    """False only for an A/B against an older build (SDUMC_LIB, tools/ema_bench.py) from before sdumc_adam_step_ema: that library
    reads sdumc_step_cfg WITHOUT the three EMA fields, which sit behind `rates` in the struct's middle, so StepCfg leaves them out for
    it."""
    if not os.environ.get("SDUMC_LIB") or not os.path.exists(LIB_PATH):
        return True
    return hasattr(C.CDLL(LIB_PATH), "sdumc_adam_step_ema")


EMA_ABI = _ema_abi()
_EMA_FIELDS = [("ema", C.c_void_p), ("ema_decay", C.c_float), ("ema_warmup", C.c_int32)]


def ema_args(ema_decay, ema_warmup):
    """TrainStep / FusedTrainer (ema_decay=, ema_warmup=) -> (on, sdumc_step_cfg.ema_decay, .ema_warmup); (False, 0.0, 0) = the step
    without averaged weights.  ema_decay: None or a Python number in [0, 1] (no bool, no string, no tensor, no NaN); ema_warmup: a
    bool, and only beside ema_decay."""
    if not isinstance(ema_warmup, bool):
        raise SdumcError(f"ema_warmup must be True or False, not {ema_warmup!r}")
    if ema_decay is None:
        if ema_warmup:
            raise SdumcError("ema_warmup=True needs ema_decay")
        return False, 0.0, 0
    if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0.0 <= ema_decay <= 1.0:      # (NaN fails both)
        raise SdumcError(f"ema_decay must be a number in [0, 1] or None, not {ema_decay!r}")
    return True, float(ema_decay), int(ema_warmup)


def _adamw_abi():
    """False only for an A/B against an older build (SDUMC_LIB, tools/adamw_bench.py) from before sdumc_adamw_step: that library reads
    sdumc_step_cfg with four bytes of padding where decoupled_decay sits and would silently ignore the field, so StepCfg leaves it
    out for it (the layout is the same either way) and decoupled_decay=True raises on the host."""
    if not os.environ.get("SDUMC_LIB") or not os.path.exists(LIB_PATH):
        return True
    return hasattr(C.CDLL(LIB_PATH), "sdumc_adamw_step")


ADAMW_ABI = _adamw_abi()
_ADAMW_FIELDS = [("decoupled_decay", C.c_int32)]


def decoupled_arg(decoupled_decay):
    """TrainStep / FusedTrainer (decoupled_decay=) -> sdumc_step_cfg.decoupled_decay; a bool and nothing else."""
    if not isinstance(decoupled_decay, bool):
        raise SdumcError(f"decoupled_decay must be True or False, not {decoupled_decay!r}")
    if decoupled_decay and not ADAMW_ABI:
        raise SdumcError("decoupled_decay: the library named by SDUMC_LIB is from before sdumc_adamw_step")
    return int(decoupled_decay)


class StepCfg(C.Structure):
    _fields_ = [("weights", C.c_float * 6), ("temperature", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float)] + (
                _ADAMW_FIELDS if ADAMW_ABI else []) + [
                ("labels", C.c_void_p), ("adam_m", C.c_void_p), ("adam_v", C.c_void_p), ("hyper", C.c_void_p),
                ("losses", C.c_void_p)] + (_GUARD_FIELDS if GUARD_ABI else []) + [
                ("B_global", C.c_int32), ("regress", C.c_int32), ("ssd_global", C.c_void_p), ("rnc_feats_global", C.c_void_p),
                ("rnc_labels_global", C.c_void_p)] + (_RATES_FIELDS if RATES_ABI else []) + (
                _EMA_FIELDS if EMA_ABI else []) + [("rnc_row0", C.c_int32 * 2),
                ("contrast", C.c_int32), ("supcon_label_mode", C.c_int32), ("supcon_temperature", C.c_float),
                ("supcon_base_temperature", C.c_float), ("distill", C.c_int32)]

    # sdumc_step_cfg.regress_delta: the float in the struct's last four bytes, behind `distill` -- tail padding until now, so sizeof
    # and every offset stay (`regress` likewise fills the padding behind B_global; an older library reads neither).  `distill` stays
    # the mirror's last entry, which tests pin: the field is reached at its offset.
    @property
    def regress_delta(self):
        return C.c_float.from_buffer(self, StepCfg.distill.offset + 4).value

    @regress_delta.setter
    def regress_delta(self, v):
        C.c_float.from_buffer(self, StepCfg.distill.offset + 4).value = v


REGRESS_DELTA_OFFSET = StepCfg.distill.offset + 4
assert REGRESS_DELTA_OFFSET + 4 == C.sizeof(StepCfg)


def _regress_abi():
    """False only for an A/B against an older build (SDUMC_LIB, tools/regress_bench.py) from before sdumc_reg_fwd_bwd: that library
    reads sdumc_step_cfg's two regression fields as padding and would silently run MSE, so regress != 'mse' raises on the host."""
    if not os.environ.get("SDUMC_LIB") or not os.path.exists(LIB_PATH):
        return True
    return hasattr(C.CDLL(LIB_PATH), "sdumc_reg_fwd_bwd")


REGRESS_ABI = _regress_abi()

# sdumc_step_cfg.regress: the criterion of the two regression terms (SDUMC_REGRESS_* of include/sdumc_hip.h)
REGRESS = {"mse": 0, "l1": 1, "huber": 2, "ccc": 3}


def regress_args(regress, regress_delta=1.0):
    """TrainStep / FusedTrainer (regress=, regress_delta=) -> (sdumc_step_cfg.regress, .regress_delta).  regress: one of REGRESS;
    regress_delta: Huber's delta, a positive finite Python number (no bool, no string, no tensor) that is positive and finite as
    fp32 too; it is read by 'huber' alone, so anything but the default 1.0 beside another criterion raises."""
    import math
    if not isinstance(regress, str) or regress not in REGRESS:
        raise SdumcError(f"regress must be one of {sorted(REGRESS)}, not {regress!r}")
    d = regress_delta
    if isinstance(d, bool) or not isinstance(d, (int, float)) or not math.isfinite(d) or d <= 0:
        raise SdumcError(f"regress_delta must be a positive finite number, not {d!r}")
    if C.c_float(d).value in (0.0, float("inf")):      # (what the kernel would see)
        raise SdumcError(f"regress_delta must be a positive finite fp32 value, not {d!r}")
    if regress != "huber" and d != 1.0:
        raise SdumcError(f"regress_delta is read by regress='huber' alone, not by {regress!r}")
    if regress != "mse" and not REGRESS_ABI:
        raise SdumcError("regress: the library named by SDUMC_LIB is from before sdumc_reg_fwd_bwd")
    return REGRESS[regress], float(d)


class Teacher(C.Structure):         # sdumc_teacher: a stored teacher's tables beside a step (teacher.TeacherTargets fills it)
    _fields_ = [("text_hidden", C.c_void_p), ("cross_text", C.c_void_p), ("fused", C.c_void_p), ("idx", C.c_void_p),
                ("n_rows", C.c_int64)]


def _teacher_abi():
    """False only for an A/B against an older build (SDUMC_LIB, tools/teacher_bench.py) from before sdumc_train_step_teacher: a
    teacher then raises on the host (that library has no entry that takes one)."""
    if not os.environ.get("SDUMC_LIB") or not os.path.exists(LIB_PATH):
        return True
    return hasattr(C.CDLL(LIB_PATH), "sdumc_train_step_teacher")


TEACHER_ABI = _teacher_abi()


# sdumc_step_cfg.distill: the criterion of the three distillation pairs (SDUMC_DISTILL_* of include/sdumc_hip.h)
DISTILL = {"rmse": 0, "cosine": 1, "kl": 2}


def distill_code(name):
    if not isinstance(name, str) or name not in DISTILL:
        raise SdumcError(f"distill must be one of {sorted(DISTILL)}, not {name!r}")
    return DISTILL[name]


def guard_args(clip_norm, skip_nonfinite):
    """TrainStep / FusedTrainer (clip_norm=, skip_nonfinite=) -> (sdumc_step_cfg.clip_norm, .skip_nonfinite); (0.0, 0) = both off,
    the step without sdumc_grad_guard.  clip_norm: None or a positive finite Python number (no bool, no string, no tensor);
    skip_nonfinite: a bool."""
    import math
    clip = 0.0
    if clip_norm is not None:
        if isinstance(clip_norm, bool) or not isinstance(clip_norm, (int, float)) or not math.isfinite(clip_norm) or clip_norm <= 0:
            raise SdumcError(f"clip_norm must be a positive finite number or None, not {clip_norm!r}")
        clip = float(clip_norm)
        if C.c_float(clip).value in (0.0, float("inf")):      # (what the kernel would see)
            raise SdumcError(f"clip_norm must be a positive finite fp32 value, not {clip_norm!r}")
    if not isinstance(skip_nonfinite, bool):
        raise SdumcError(f"skip_nonfinite must be True or False, not {skip_nonfinite!r}")
    return clip, int(skip_nonfinite)


# sdumc_step_cfg.contrast: the contrastive criterion over the rnc rows (SDUMC_CONTRAST_*); .supcon_label_mode: which labels count as
# one class for SupCon ('eq': equal labels, 'round': equal rint(label), the seven classes of a MOSEI sentiment score)
CONTRAST = {"rnc": 0, "supcon": 1}
CONTRAST_CLASSES = {"eq": 0, "round": 1}


def contrast_code(name, classes="eq"):
    """-> (SDUMC_CONTRAST_* code, label mode)"""
    if not isinstance(name, str) or name not in CONTRAST:
        raise SdumcError(f"contrast must be one of {sorted(CONTRAST)}, not {name!r}")
    if not isinstance(classes, str) or classes not in CONTRAST_CLASSES:
        raise SdumcError(f"contrast_classes must be one of {sorted(CONTRAST_CLASSES)}, not {classes!r}")
    return CONTRAST[name], CONTRAST_CLASSES[classes]


def contrast_cfg(cfg, contrast, temperature, classes):
    """Fill a StepCfg's contrastive fields: 'rnc' (temperature None = the reference's 2.0) or 'supcon' (None = 0.07)."""
    code, mode = contrast_code(contrast, classes)
    if temperature is not None and not (isinstance(temperature, (int, float)) and temperature > 0):
        raise SdumcError(f"contrast_temperature must be a positive number or None, not {temperature!r}")
    if code == CONTRAST["rnc"]:
        cfg.temperature = 2.0 if temperature is None else float(temperature)
    else:
        cfg.temperature = 2.0
        cfg.supcon_temperature = 0.07 if temperature is None else float(temperature)
        cfg.supcon_base_temperature = 0.07
        cfg.supcon_label_mode = mode
    cfg.contrast = code


GATHER_MAX_SEGS = 8


class GatherSeg(C.Structure):
    _fields_ = [("packed", C.c_void_p), ("start_all", C.c_void_p), ("len_all", C.c_void_p), ("out", C.c_void_p),
                ("len_out", C.c_void_p), ("map_out", C.c_void_p), ("zero_row", C.c_int32), ("Tmax", C.c_int32), ("d4", C.c_int32),
                # the random-missing protocol (data.MissingSpec.thresholds; all zero = none of it)
                ("miss_mod", C.c_int32), ("miss_frame_thr", C.c_uint32), ("miss_utt_thr", C.c_uint32), ("miss_all", C.c_uint32),
                ("unit0", C.c_int64)]


class GatherBatch(C.Structure):
    _fields_ = [("seg", GatherSeg * GATHER_MAX_SEGS), ("nseg", C.c_int32), ("B", C.c_int32), ("idx", C.c_void_p),
                ("labels_all", C.c_void_p), ("labels_out", C.c_void_p), ("total", C.c_int64),
                ("miss_seed_lo", C.c_uint32), ("miss_seed_hi", C.c_uint32), ("miss_draw", C.c_uint32), ("miss_enable", C.c_uint32)]


class PoolFrames(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_start", C.c_void_p), ("src_len", C.c_void_p),
                ("dst_start", C.c_void_p), ("dst_len", C.c_void_p), ("src_rows", C.c_int64), ("dst_rows", C.c_int64),
                ("n_utts", C.c_int32), ("cols", C.c_int32), ("bf16", C.c_int32)]


class Softmax(C.Structure):
    _fields_ = [("batch", C.c_int32), ("heads", C.c_int32), ("tq", C.c_int32), ("tk", C.c_int32),
                ("scale", C.c_float), ("mask", C.c_void_p), ("scores", C.c_void_p), ("probs_drop", C.c_void_p),
                ("weights", C.c_void_p), ("drop", Dropout)]


class DropAdd(C.Structure):
    _fields_ = [("x", C.c_void_p), ("alpha", C.c_float), ("pos_table", C.c_void_p), ("pos_src", C.c_void_p),
                ("residual", C.c_void_p), ("y", C.c_void_p),
                ("samples", C.c_int32), ("rows", C.c_int32), ("width", C.c_int32), ("drop", Dropout)]


class Mha(C.Structure):
    _fields_ = [("tq", C.c_int32), ("tk", C.c_int32), ("batch", C.c_int32), ("embed", C.c_int32), ("heads", C.c_int32),
                ("query", C.c_void_p), ("key", C.c_void_p), ("value", C.c_void_p),
                ("in_proj_weight", C.c_void_p), ("in_proj_bias", C.c_void_p),
                ("out_proj_weight", C.c_void_p), ("out_proj_bias", C.c_void_p),
                ("attn_mask", C.c_void_p), ("attn_drop", Dropout),
                ("out", C.c_void_p), ("weights", C.c_void_p),
                ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p),
                ("probs", C.c_void_p), ("probs_drop", C.c_void_p), ("ctx", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("bf16", C.c_int32),
                ("bias_k", C.c_void_p), ("bias_v", C.c_void_p), ("add_zero_attn", C.c_int32)]


class MhaGrads(C.Structure):
    _fields_ = [("dout", C.c_void_p), ("dquery", C.c_void_p), ("dkey", C.c_void_p), ("dvalue", C.c_void_p),
                ("d_in_proj_weight", C.c_void_p), ("d_in_proj_bias", C.c_void_p),
                ("d_out_proj_weight", C.c_void_p), ("d_out_proj_bias", C.c_void_p),
                ("d_bias_k", C.c_void_p), ("d_bias_v", C.c_void_p)]


class ProfEntry(C.Structure):
    _fields_ = [("name", C.c_char_p), ("launches", C.c_int64), ("total_ms", C.c_double), ("total_flops", C.c_double)]


class CopySeg(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("ld_src", C.c_int32), ("ld_dst", C.c_int32),
                ("rows", C.c_int32), ("cols", C.c_int32)]


SCATTER_MAX_SEGS = 10


class ScatterSeg(C.Structure):      # sdumc_scatter_seg: dst[idx[r % B], 0:cols] = src[r, 0:cols]
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32), ("dst_rows", C.c_int64)]


LOG_COLS = 12      # sdumc_epoch_rec.log_row: losses[0..7], grad_norm, non-finite gradient elements, B, learning rate


class EpochRec(C.Structure):        # sdumc_epoch_rec: a completed train step's outputs -> store order, its log row, its gradient norm
    _fields_ = [("seg", ScatterSeg * SCATTER_MAX_SEGS), ("nseg", C.c_int32), ("B", C.c_int32), ("idx", C.c_void_p),
                ("mark", C.c_void_p), ("losses", C.c_void_p), ("hyper", C.c_void_p), ("log_row", C.c_void_p),
                ("grads", C.c_void_p), ("n_grads", C.c_int64), ("scratch", C.c_void_p)]


TENSOR_NORMS_MAX_SEGS = 96


class NormSeg(C.Structure):         # sdumc_norm_seg: one tensor of sdumc_tensor_norms (y: the optional rolling snapshot)
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("count", C.c_int64)]


class AttnExport(C.Structure):      # sdumc_attn_export: a completed eval-mode forward's attention weights -> store-ordered [rows, 8] tensors
    _fields_ = [("idx", C.c_void_p), ("start", C.c_void_p * 4), ("length", C.c_void_p * 4), ("n_utt", C.c_int64),
                ("dst", (C.c_void_p * 3) * 2), ("dst_rows", (C.c_int64 * 3) * 2)]


SALIENCY_MAX_DESCS = 4
SALIENCY_COLS = 2


class SaliencyDesc(C.Structure):    # sdumc_saliency_desc: one modality's feature gradient x features -> a store-ordered [rows, 2] tensor
    _fields_ = [("grad", C.c_void_p), ("feat", C.c_void_p), ("row_map", C.c_void_p), ("store_rows", C.c_int64),
                ("start", C.c_void_p), ("length", C.c_void_p), ("n_utt", C.c_int64), ("dst", C.c_void_p), ("dst_rows", C.c_int64),
                ("B", C.c_int32), ("T", C.c_int32), ("d", C.c_int32)]


ADAM_MAX_SEGS = 96


class AdamSeg(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("state_offset", C.c_int64), ("n", C.c_int64)]


class EmaSeg(C.Structure):         # sdumc_ema_seg: ema[0 .. n) <- lerp(ema, param, weight)
    _fields_ = [("ema", C.c_void_p), ("param", C.c_void_p), ("n", C.c_int64)]


class AdamTable(C.Structure):      # one launch's kernel argument (filled by sdumc_adam_multi; mirrored for the size checks)
    _fields_ = [("seg", AdamSeg * ADAM_MAX_SEGS), ("block_end", C.c_uint32 * ADAM_MAX_SEGS), ("nseg", C.c_int32),
                ("reserved", C.c_int32)]


_SIGS = {
    "sdumc_copy2d_multi": (C.c_int, [C.POINTER(CopySeg), C.c_int32, C.c_void_p]),
    "sdumc_scatter_rows_multi": (C.c_int, [C.POINTER(ScatterSeg), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "sdumc_epoch_record_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "sdumc_epoch_record": (C.c_int, [C.POINTER(EpochRec), C.c_void_p]),
    "sdumc_tensor_norms_scratch_bytes": (C.c_size_t, [C.POINTER(NormSeg), C.c_int32]),
    "sdumc_tensor_norms": (C.c_int, [C.POINTER(NormSeg), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    "sdumc_grad_guard_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "sdumc_grad_guard": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdumc_grad_guard_multi_scratch_bytes": (C.c_size_t, [C.POINTER(NormSeg), C.c_int32]),
    "sdumc_grad_guard_multi": (C.c_int, [C.POINTER(NormSeg), C.c_int32, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "sdumc_profile_enable": (C.c_int, [C.c_int]),
    "sdumc_profile_report": (C.c_int, [C.POINTER(ProfEntry), C.c_int]),
    "sdumc_gemm_workspace_bytes": (C.c_size_t, [C.POINTER(Gemm)]),
    "sdumc_gemm_f32": (C.c_int, [C.POINTER(Gemm), C.c_void_p]),
    "sdumc_gemm_group_workspace_bytes": (C.c_size_t, [C.POINTER(GGProblem), C.c_int32]),
    "sdumc_gemm_group_tn": (C.c_int, [C.POINTER(GGProblem), C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sdumc_gemm_group_bf16_workspace_bytes": (C.c_size_t, [C.POINTER(GGProblem), C.c_int32]),
    "sdumc_gemm_group_tn_bf16": (C.c_int, [C.POINTER(GGProblem), C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sdumc_set_split_": (None, [C.c_int]),
    "sdumc_get_split_": (C.c_int, []),
    "sdumc_gemm_p3_workspace_bytes": (C.c_size_t, [C.POINTER(GemmP3)]),
    "sdumc_gemm_p3_nt": (C.c_int, [C.POINTER(GemmP3), C.c_void_p]),
    "sdumc_p3_split": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]),
    "sdumc_p3_split_frag": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "sdumc_p3_split_frag_t": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "sdumc_frame_dx_scratch_bytes": (C.c_size_t, [C.c_int32]),
    "sdumc_frame_dx": (C.c_int, [C.POINTER(FrameDx), C.c_void_p]),
    "sdumc_p3_join": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]),
    "sdumc_gemm_b1_workspace_bytes": (C.c_size_t, [C.POINTER(GemmB1)]),
    "sdumc_gemm_b1_nt": (C.c_int, [C.POINTER(GemmB1), C.c_void_p]),
    "sdumc_b1_frag_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32), C.c_int, C.c_void_p]),
    "sdumc_gemm_rows256": (C.c_int, [C.POINTER(RowsProblem), C.c_int32, C.c_void_p]),
    "sdumc_gemm_rows256_bf16": (C.c_int, [C.POINTER(RowsProblem), C.c_int32, C.c_void_p]),
    "sdumc_attnpool_fwd_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "sdumc_attnpool_fwd": (C.c_int, [C.POINTER(AttnPool), C.c_void_p]),
    "sdumc_attnpool_fwd_workspace_bytes_dim": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "sdumc_attnpool_bwd_workspace_bytes_dim": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "sdumc_attnpool_bwd_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "sdumc_attnpool_bwd": (C.c_int, [C.POINTER(AttnPoolBwd), C.c_void_p]),
    "sdumc_attnpool_fwd_multi": (C.c_int, [C.POINTER(AttnPool), C.c_int32, C.c_void_p]),
    "sdumc_umca_fwd": (C.c_int, [C.POINTER(Umca), C.c_void_p]),
    "sdumc_attnpool_bwd_multi": (C.c_int, [C.POINTER(AttnPoolBwd), C.c_int32, C.c_void_p]),
    "sdumc_relu_drop_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int64, C.c_void_p]),
    "sdumc_colsum_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "sdumc_colsum": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "sdumc_add_n": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "sdumc_dropsum_bwd": (C.c_int, [C.POINTER(DropSum), C.c_void_p]),
    "sdumc_fusion_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "sdumc_fusion_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "sdumc_hweight_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "sdumc_hweight_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p]),
    "sdumc_zpool_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "sdumc_zpool_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "sdumc_mse_fwd_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdumc_reg_fwd_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_float, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "sdumc_ssd_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "sdumc_ssd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdumc_rmse_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_float, C.c_void_p,
                                 C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "sdumc_cosine_fwd_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdumc_kl_fwd_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdumc_ce_fwd_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdumc_supcon_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "sdumc_supcon_fwd_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_double, C.c_double, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "sdumc_rnc_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "sdumc_rnc_fwd_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32,
                                    C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdumc_rnc_fwd_bwd_rep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32,
                                        C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdumc_distill_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "sdumc_distill_fwd_bwd": (C.c_int, [C.c_int32, C.c_float] + [C.c_void_p] * 14),
    "sdumc_distill_teacher_fwd_bwd": (C.c_int, [C.c_int32, C.c_float] + [C.c_void_p] * 13 + [C.c_int32, C.POINTER(Teacher), C.c_void_p]),
    "sdumc_rnc_dfeat_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdumc_rnc_mask": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "sdumc_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                  C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "sdumc_adam_step_rates": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(RateSeg), C.c_int32,
                                        C.c_void_p]),
    "sdumc_zero_segments": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(RateSeg), C.c_int32, C.c_void_p]),
    "sdumc_adam_step_ema": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(RateSeg), C.c_int32,
                                      C.c_void_p, C.c_float, C.c_int32, C.c_void_p]),
    "sdumc_ema_multi": (C.c_int, [C.POINTER(EmaSeg), C.c_int32, C.c_float, C.c_void_p]),
    "sdumc_adamw_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                   C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(RateSeg), C.c_int32,
                                   C.c_void_p, C.c_float, C.c_int32, C.c_void_p]),
    "sdumc_adamw_multi": (C.c_int, [C.POINTER(AdamSeg), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "sdumc_adam_multi": (C.c_int, [C.POINTER(AdamSeg), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                   C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "sdumc_copy2d": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "sdumc_axpy2d": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "sdumc_gather_pad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "sdumc_mask_apply_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_float, C.c_void_p]),
    "sdumc_gemm_bf16_workspace_bytes": (C.c_size_t, [C.POINTER(GemmBf16)]),
    "sdumc_gemm_bf16_run": (C.c_int, [C.POINTER(GemmBf16), C.c_void_p]),
    "sdumc_ctx_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "sdumc_ctx_destroy": (C.c_int, [C.c_void_p]),
    "sdumc_ctx_set_option": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "sdumc_gather_pad_idx": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "sdumc_gather_batch": (C.c_int, [C.POINTER(GatherBatch), C.c_int32, C.c_void_p]),
    "sdumc_pool_frames": (C.c_int, [C.POINTER(PoolFrames), C.c_int32, C.c_void_p]),
    "sdumc_fill": (C.c_int, [C.c_void_p, C.c_float, C.c_int64, C.c_void_p]),
    "sdumc_rng_advance": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "sdumc_dropout_bits": (C.c_int, [C.POINTER(Dropout), C.c_int32, C.c_void_p, C.c_void_p]),
    "sdumc_dropout_bits_multi": (C.c_int, [C.POINTER(Dropout), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.c_void_p]),
    "sdumc_dropout_bits_apply_bf16": (C.c_int, [C.POINTER(Dropout), C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.c_void_p, C.c_int64,
                                               C.POINTER(C.c_void_p), C.c_void_p]),
    "sdumc_dropout_mask": (C.c_int, [C.POINTER(Dropout), C.c_int32, C.c_void_p, C.c_void_p]),
    "sdumc_version": (C.c_char_p, []),
    # generic MHA / Transformer-encoder pieces (transformer.hip)
    "sdumc_layernorm_fwd": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int32, C.c_float, C.c_void_p]),
    "sdumc_layernorm_bwd_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "sdumc_layernorm_bwd": (C.c_int, [C.c_void_p] * 9 + [C.c_int64, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sdumc_softmax_fwd": (C.c_int, [C.POINTER(Softmax), C.c_void_p]),
    "sdumc_softmax_bwd": (C.c_int, [C.POINTER(Softmax), C.c_void_p, C.c_void_p]),
    "sdumc_drop_add": (C.c_int, [C.POINTER(DropAdd), C.c_void_p]),
    "sdumc_mha_workspace_bytes": (C.c_size_t, [C.POINTER(Mha), C.c_int32]),
    "sdumc_mha_forward": (C.c_int, [C.POINTER(Mha), C.c_void_p]),
    "sdumc_mha_backward": (C.c_int, [C.POINTER(Mha), C.POINTER(MhaGrads), C.c_void_p]),
    # network level (engine.hip)
    "sdumc_param_count": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "sdumc_param_live_count": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "sdumc_param_table": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]),
    "sdumc_set_concurrency": (C.c_int, [C.c_int]),
    "sdumc_set_background_lane": (C.c_int, [C.c_int]),
    "sdumc_set_chain_cluster": (C.c_int, [C.c_int]),
    "sdumc_chain_cluster_error_": (C.c_int, []),
    "sdumc_chain_cluster_reset_error": (C.c_int, []),
    "sdumc_chain_cluster_test_hold_": (C.c_int, [C.c_int]),
    "sdumc_chain_cluster_debug_read_": (C.c_int, [C.c_void_p, C.c_int]),
    "sdumc_chain_cluster_error_flag": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sdumc_chain_cluster_error_merge": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sdumc_debug_marks": (C.c_int, [C.c_int]),
    "sdumc_debug_marks_read": (C.c_int, [C.POINTER(C.c_float), C.c_int]),
    "sdumc_attnpool_set_v2_": (C.c_int, [C.c_int]),
    "sdumc_debug_plan_table": (C.c_int32, [C.POINTER(NetDims), C.c_char_p, C.c_size_t]),
    "sdumc_debug_backward_schedule": (C.c_int32, [C.POINTER(NetDims), C.POINTER(NetIO), C.c_int32, C.c_uint32, C.c_void_p,
                                                  C.c_char_p, C.c_size_t]),
    "sdumc_net_workspace_bytes": (C.c_size_t, [C.POINTER(NetDims)]),
    "sdumc_net_bits_next_bytes": (C.c_size_t, [C.POINTER(NetDims)]),
    "sdumc_net_forward": (C.c_int, [C.POINTER(NetDims), C.POINTER(NetIO), C.c_void_p]),
    "sdumc_net_export_attention": (C.c_int, [C.POINTER(NetDims), C.POINTER(NetIO), C.POINTER(AttnExport), C.c_void_p]),
    "sdumc_net_backward": (C.c_int, [C.POINTER(NetDims), C.POINTER(NetIO), C.POINTER(NetGrads), C.c_void_p]),
    "sdumc_net_backward_phase": (C.c_int, [C.POINTER(NetDims), C.POINTER(NetIO), C.POINTER(NetGrads), C.c_int32, C.c_void_p]),
    "sdumc_param_early_count": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "sdumc_frame_saliency": (C.c_int, [C.POINTER(SaliencyDesc), C.c_int32, C.c_void_p, C.c_void_p]),
    "sdumc_net_feature_grad_scratch_bytes": (C.c_size_t, [C.POINTER(NetDims)]),
    "sdumc_step_workspace_bytes": (C.c_size_t, [C.POINTER(NetDims)]),
    "sdumc_train_step": (C.c_int, [C.POINTER(NetDims), C.POINTER(NetIO), C.POINTER(StepCfg), C.c_void_p]),
    "sdumc_train_step_teacher": (C.c_int, [C.POINTER(NetDims), C.POINTER(NetIO), C.POINTER(StepCfg), C.POINTER(Teacher), C.c_void_p]),
    "sdumc_loss_workspace_bytes": (C.c_size_t, [C.POINTER(NetDims), C.c_int32]),
    "sdumc_loss_ssd": (C.c_int, [C.POINTER(NetDims), C.POINTER(NetIO), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sdumc_loss_backward": (C.c_int, [C.POINTER(NetDims), C.POINTER(NetIO), C.POINTER(StepCfg), C.POINTER(NetGrads),
                                      C.c_void_p, C.c_size_t, C.c_void_p]),
    "sdumc_loss_backward_teacher": (C.c_int, [C.POINTER(NetDims), C.POINTER(NetIO), C.POINTER(StepCfg), C.POINTER(NetGrads),
                                              C.POINTER(Teacher), C.c_void_p, C.c_size_t, C.c_void_p]),
    "sdumc_dp_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "sdumc_dp_record_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "sdumc_dp_record": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdumc_dp_unpack": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "sdumc_step_grads_offset": (C.c_size_t, [C.POINTER(NetDims)]),
}

EXPORTS = tuple(_SIGS)


class SdumcError(RuntimeError):
    pass


_ERR = {-1: "SDUMC_EINVAL (bad argument)", -2: "SDUMC_ELAUNCH (HIP launch/runtime error)",
        -3: "SDUMC_ENOMEM (workspace too small)"}


def _load():
    if not os.path.exists(LIB_PATH):
        raise SdumcError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C sdumc_amd/csrc`. sdumc_amd has no CPU or PyTorch fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        if os.environ.get("SDUMC_LIB") and not hasattr(lib, name):
            continue             # A/B against an older build: it may lack newer entry points
        fn = getattr(lib, name)  # AttributeError (loud) if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(rc, what=""):
    if rc != 0:
        raise SdumcError(f"{what} failed: {_ERR.get(rc, rc)}")


def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def drop_threshold(p):
    return int(float(p) * 4294967296.0)


def make_dropout(enabled, site, p, rows, width, samples, sample0=0, call0=0, seed=0, dev_state=None):
    import numpy as np
    d = Dropout()
    d.enabled = 1 if enabled else 0
    d.site = site
    d.threshold = drop_threshold(p)
    d.scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    d.rows, d.width, d.samples, d.sample0, d.call0 = rows, width, samples, sample0, call0
    d.seed_lo, d.seed_hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    d.dev_state = ptr(dev_state)
    return d
