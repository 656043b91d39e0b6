"""The ragged-shape cases of the generic Transformer family and their references; a plain module, no fixtures.
tests/test_transformer_parity_cpu.py (the references alone) and tests/test_gpu_transformer.py (the HIP modules) read the same table.

Every case is seeded and built on the CPU: xavier weights, non-zero biases, LayerNorm weights 1 + 0.3 randn.  `reference(case, dtype)`
evaluates oracle/transformer_oracle.py with parameters and inputs in `dtype` (float64 = ref_hi, float32 = ref_lo of tests/grad_parity.py)
once per process and returns outputs and gradients under the names the GPU test uses:

    in_proj_weight / in_proj_bias   three tensors in one buffer: judged per part, `<name>.q`, `<name>.k`, `<name>.v`
    every other parameter           whole, under its state_dict name
    input gradients                 dq, dk, dv | dx | dq, dkv | dx, dxk, dxv   (aliased inputs share one summed gradient)

The shapes are the smallest that cross each edge of csrc/transformer.hip and of the strided-batched GEMMs: a 64-row tile in either
length, head dimensions that are no multiple of 4, and the softmax row dispatch (16-byte units up to 512 / 2048 keys, then any
length; scalar units up to 512 keys, then any length; a source length that is no multiple of 4 takes the scalar units)."""
import functools
import math

import torch

BAR_GRAD = 2e-4          # of the tensor's own norm: gradients (README: the bar of the same fp32 product kernels)
BAR_OUT = 2e-5           # outputs and head-averaged attention weights

# alias: "qkv" = three distinct inputs, "self" = one tensor three times, "kv" = key is value
MHA = dict(kind="mha", mask=False, p=0.0, bias_kv=False, zero_attn=False, train=True)
ENC = dict(kind="enc", E=96, H=4, layers=2, B=3, tq=70, p_attn=0.1, p_relu=0.2, p_res=0.15, p_embed=0.1)
CASES = [
    # odd dh; both lengths cross a 64 tile; tk = 131 -> scalar softmax rows
    dict(MHA, name="cross", E=120, H=8, tq=70, tk=131, B=3, alias="qkv", mask=True, p=0.25, seed=101),
    # fused qkv projection; dquery / dkey / dvalue summed into one buffer
    dict(MHA, name="self", E=96, H=4, tq=65, tk=65, B=2, alias="self", mask=True, p=0.1, seed=102),
    # dkey + dvalue aliasing; B = 1; [ts, B, E] buffers of 3870 floats: the second of a pair starts off a 16-byte boundary
    dict(MHA, name="kv_alias", E=30, H=2, tq=33, tk=129, B=1, alias="kv", train=False, seed=103),
    # ts = 63 + 1 + 1 = 65; d_bias_k, d_bias_v; in_proj_bias.k is a real tensor here
    dict(MHA, name="both_extras", E=64, H=4, tq=33, tk=63, B=3, alias="qkv", mask=True, p=0.25, bias_kv=True, zero_attn=True, seed=104),
    # ts = 512: the upper edge of the short vector softmax
    dict(MHA, name="bias_kv", E=32, H=4, tq=5, tk=511, B=2, alias="kv", p=0.2, bias_kv=True, seed=105),
    # ts = 513: falls to the long scalar path
    dict(MHA, name="zero_attn", E=32, H=4, tq=7, tk=512, B=1, alias="kv", p=0.2, zero_attn=True, seed=106),
    # ts = 2049: the any-length path, head mean kept in the output row
    dict(MHA, name="long", E=32, H=2, tq=3, tk=2049, B=1, alias="kv", p=0.1, seed=107),
    # one key: the softmax is the constant 1 and its gradient exactly zero
    dict(MHA, name="T1", E=32, H=4, tq=1, tk=1, B=3, alias="self", train=False, seed=108),
    # all four dropouts, mask, positions; two tokens per input have first channel exactly 0 (the padding row of the table)
    dict(ENC, name="encoder_self", tk=None, seed=109),
    dict(ENC, name="encoder_cross", tk=131, seed=110),
]
IDS = [c["name"] for c in CASES]


def by_name(name):
    return CASES[IDS.index(name)]


def _xavier(g, *shape):
    bound = math.sqrt(6.0 / (shape[0] + shape[1]))
    return (2 * torch.rand(*shape, generator=g) - 1) * bound


def _mha_params(g, E, pre="", bias_kv=False):
    P = {pre + "in_proj_weight": _xavier(g, 3 * E, E), pre + "in_proj_bias": 0.1 * torch.randn(3 * E, generator=g),
         pre + "out_proj.weight": _xavier(g, E, E), pre + "out_proj.bias": 0.1 * torch.randn(E, generator=g)}
    if bias_kv:
        P[pre + "bias_k"] = torch.randn(1, 1, E, generator=g) / math.sqrt(E)
        P[pre + "bias_v"] = torch.randn(1, 1, E, generator=g) / math.sqrt(E)
    return P


def _ln_params(g, E, pre):
    return {pre + "weight": 1 + 0.3 * torch.randn(E, generator=g), pre + "bias": 0.1 * torch.randn(E, generator=g)}


def params(case):
    """fp32 CPU parameters under the modules' state_dict names"""
    g = torch.Generator().manual_seed(case["seed"])
    E = case["E"]
    if case["kind"] == "mha":
        return _mha_params(g, E, bias_kv=case["bias_kv"])
    P = {}
    for i in range(case["layers"]):
        pre = f"layers.{i}."
        P.update(_mha_params(g, E, pre + "self_attn."))
        P.update({pre + "fc1.weight": _xavier(g, 4 * E, E), pre + "fc1.bias": 0.1 * torch.randn(4 * E, generator=g),
                  pre + "fc2.weight": _xavier(g, E, 4 * E), pre + "fc2.bias": 0.1 * torch.randn(E, generator=g)})
        for j in range(2):
            P.update(_ln_params(g, E, f"{pre}layer_norms.{j}."))
    P.update(_ln_params(g, E, "layer_norm."))
    return P


def inputs(case):
    """(fp32 CPU inputs by the name of their gradient without the d, cotangent R of the output)"""
    g = torch.Generator().manual_seed(case["seed"] + 1000)
    E, B, tq = case["E"], case["B"], case["tq"]
    tk = case["tk"] or tq
    if case["kind"] == "mha":
        shapes = {"qkv": dict(q=tq, k=tk, v=tk), "self": dict(x=tq), "kv": dict(q=tq, kv=tk)}[case["alias"]]
    else:
        shapes = dict(x=tq) if case["tk"] is None else dict(x=tq, xk=tk, xv=tk)
    X = {n: torch.randn(T, B, E, generator=g) for n, T in shapes.items()}
    if case["kind"] == "enc":
        for n, t in X.items():          # padding tokens: positions come from the first channel
            t[3, 0, 0] = 0.0
            t[t.shape[0] - 1, B - 1, 0] = 0.0
    return X, torch.randn(tq, B, E, generator=g)


def qkv(case, X):
    """the module's (query, key, value) from the inputs of a "mha" case; aliased inputs are ONE tensor"""
    return {"qkv": lambda: (X["q"], X["k"], X["v"]), "self": lambda: (X["x"],) * 3, "kv": lambda: (X["q"], X["kv"], X["kv"])}[case["alias"]]()


def split_parts(T):
    """name -> tensor with every in_proj_weight / in_proj_bias replaced by its q, k and v parts"""
    out = {}
    for k, t in T.items():
        if k.endswith("in_proj_weight") or k.endswith("in_proj_bias"):
            E = t.shape[0] // 3
            for i, part in enumerate("qkv"):
                out[f"{k}.{part}"] = t[i * E:(i + 1) * E]
        else:
            out[k] = t
    return out


def extra_rows(case):
    return case["kind"] == "mha" and (case["bias_kv"] or case["zero_attn"])


def no_signal(case, names):
    """Without extra source rows the softmax is invariant to the k part of in_proj_bias (it shifts every score of a row by the same
    q . b_k): its gradient is a sum that cancels to rounding noise.  With add_bias_kv / add_zero_attn it is an ordinary tensor."""
    return frozenset() if extra_rows(case) else frozenset(k for k in names if k.endswith("in_proj_bias.k"))


def zeros(case):
    """One key: dS = P (dP - sum P dP) = 1 * (dP - dP) is exactly zero, and with it everything upstream of the scores.
    (in_proj_bias.k is in the no-signal set as well; here it is exactly zero.)"""
    return ("in_proj_weight.q", "in_proj_weight.k", "in_proj_bias.q", "in_proj_bias.k") if case["name"] == "T1" else ()


SEED, CALL = 20240611, 7          # the dropout stream of every case: te.manual_seed(SEED, CALL) / TO.DropSeq(train, SEED, CALL)


@functools.lru_cache(maxsize=None)
def _reference(name, dtype):
    from oracle import transformer_oracle as TO
    case = by_name(name)
    P = {k: v.to(dtype).requires_grad_() for k, v in params(case).items()}
    X, R = inputs(case)
    X = {k: v.to(dtype).requires_grad_() for k, v in X.items()}
    tq, tk = case["tq"], case["tk"] or case["tq"]
    if case["kind"] == "mha":
        drop = TO.DropSeq(case["train"] and case["p"] > 0, SEED, CALL)
        mask = TO.future_mask(tq, tk, dtype) if case["mask"] else None
        out, w = TO.multi_head_attention(P, "", *qkv(case, X), case["H"], drop, case["p"], mask, add_zero_attn=case["zero_attn"])
        outs = {"out": out.detach(), "weights": w.detach()}
    else:
        out = TO.encoder(P, X["x"], case["H"], case["layers"], TO.DropSeq(True, SEED, CALL), case["p_attn"], case["p_relu"], case["p_res"],
                         case["p_embed"], use_mask=True, use_pos=True, x_in_k=X.get("xk"), x_in_v=X.get("xv"))
        outs = {"out": out.detach()}
    (out * R.to(dtype)).sum().backward()
    grads = split_parts({k: v.grad for k, v in P.items()})
    grads.update({"d" + k: v.grad for k, v in X.items()})
    return outs, grads


def reference(case, dtype=torch.float64):
    """(outputs, gradients) of the oracle with parameters and inputs in `dtype`; computed once, shared, never to be written to"""
    return _reference(case["name"], dtype)
