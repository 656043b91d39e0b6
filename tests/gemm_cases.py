"""The cases of the GEMM family (include/sdumc_hip.h: sdumc_gemm_f32, sdumc_gemm_bf16_run, sdumc_gemm_group_tn(_bf16),
sdumc_gemm_p3_nt, sdumc_gemm_b1_nt, sdumc_gemm_rows256(_bf16), sdumc_frame_dx) and their references; a plain module, no fixtures.
tests/test_gemm_parity_cpu.py (the references alone, and the stand-ins that show the bar has teeth) and tests/test_gpu_gemm_parity.py
(every launch route) read the same table, RUNS.

The operation, restated in torch at a given dtype from the header's definitions.  Every form of the family is one product of two
EFFECTIVE matrices Ae [M, K] and Be [N, K] (operands()), which hold what the kernel multiplies after everything the header lets a
call do to an operand -- all of it exact in fp32, so both restatements start from the same values:

    NT  Ae = A[rows]            Be = B                 rows = m % a_row_mod, or a_map[m]; rows >= a2_row0 come from the second tensor
    NN  Ae = A[rows]            Be = B^T
    TN  Ae = A^T                Be = B[rows]^T         rows = k % b_row_mod, or b_map[k]; two K segments = the columns side by side
    keep-bits on A (or on B, TN): the masked operand times keep times scale (scale 2 = 1 / (1 - 0.5): exact)
    bf16 operands (sdumc_gemm.bf16, the bf16-storage entry points): both matrices rounded to bf16 first

    C = sum_k Ae[m, k] Be[n, k]                                        accumulated left to right in the dtype (_acc)
        + sum_i pool_w[m, i] pool_g[m / pool_T, i, n]                  rows256: the pooling term, as further terms of the same sum
    C = sum_{s < fold} keep_s[r] C[s R + r] * c_scale                  rows256 fold: R = M / fold rows leave
    C = act(C + bias);  C += C0 (accumulate);  C *= [Y > 0] * c_mask_scale (c_mask_y)
    colsum_a[m] = sum_k Ae[m, k] (+ its own C0)
    frame_dx: rows b T + t with t >= lengths[b] are exact +0.0

ref_hi is the float64 evaluation, ref_lo the float32 one: K chained roundings, the pessimistic order, and ONE evaluation on every host
(a BLAS sums in blocks of the host's vector width).

Inputs: randn operands, B divided by sqrt(K).  The non-contracted index of each operand is multiplied by an exact power of two drawn
from 2^-12 .. 2^12 (ra over m, rb over n), so output (m, n) carries the known factor ra[m] rb[n]; got, ref_hi and ref_lo are divided by
it before they are judged -- exactly -- and every row and column weighs the same, while a leak between rows of different scale is
magnified by up to 2^24.  Cases with a bias scale the columns only, cases with an activation are unscaled.

Slices: an output is cut into the tiles ONE workgroup (or one stream-K output tile) owns on its route, cut to the valid extent; the
tile is the run's `tile`, read off the launchers (frame_dx: 64 rows x 256 columns, the block a workgroup walks; finer than what it
owns).  colsum_a is one slice per problem.  The judgement is tests/grad_parity.py::tensor_errors over the slice names.

Bars, none taken from the device (rule_of):
    "f32"      fp32 storage, no activation; bf16 storage with fp32 output (the operands are the same bf16 values on both sides, only
               the summation differs): per slice min(BAR_OUT, max(4 e_ref[slice], 2^-22)) -- e_ref = ref_lo against ref_hi on that
               slice, 4 = grad_parity's factor, 2^-22 = four roundings of the stored fp32 result
    "act"      tanh or ReLU: BAR_OUT
    "bf16out"  bf16 output: against round_bf16(ref_hi), with 4 BF16_E_REF (the error the two ROUNDED restatements have against each
               other, measured and asserted again by the CPU test)"""
import functools
import zlib

import numpy as np
import torch

from tests.attn_pool_cases import round_bf16

BAR_OUT = 2e-5            # the project's bar for outputs, of a slice's own norm
FLOOR = 2.0 ** -22
# bf16 outputs, fp32 restatement rounded to bf16 against fp64 restatement rounded to bf16: the worst slice over every bf16-output run
# (tests/test_gemm_parity_cpu.py::test_bf16_rounded_references prints each and asserts worst <= this <= 1.5 worst).  A slice in which
# k of n elements round the other way sits near 2^-8 sqrt(k / n): with restatements 1e-7 apart about one element in 3e4 does, so a
# slice holds one such element or none and the figure moves in steps; measured 0 .. 2.2e-5 over the runs, hence a quarter above the worst.
BF16_E_REF = 2.7e-5
NT, NN, TN = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2


def _acc(n, term):
    """sum_{k < n} term(k), accumulated left to right in the terms' dtype (tests/attn_pool_cases.py::_acc)"""
    a = term(0)
    for k in range(1, n):
        a = a + term(k)
    return a


# ---- the table -------------------------------------------------------------------------------------------------------------------
def P(M, N, K, K1=0, **kw):
    """one problem: shape and what the call does to its operands (module docstring).  Keys: layout bias act acc amod bmod bmod1 colsum
    keep ('A' / 'B') a2 (a2_row0) amap bmap masky bf16 (operands are bf16 values) bf16out pool (T, nq) fold cbits lens (T, lengths)"""
    return dict(dict(M=M, N=N, K=K, K1=K1, layout=NT, bias=False, act=ACT_NONE, acc=False, amod=0, bmod=0, bmod1=0, colsum=False,
                     keep=None, a2=0, amap=False, bmap=False, masky=False, bf16=False, bf16out=False, pool=None, fold=0, cbits=False,
                     lens=None), **kw)


RUNS = []


def run(entry, variant, name, own, probs, launches=1, **opts):
    """entry: the C entry point's short name; variant: the name sdumc_profile_report gives the launch; own: the tile (rows, columns)
    one workgroup owns; probs: one P or a list (groups / batch entries / the problems of a grouped launch); opts: the launcher's own
    arguments (tile=, splitk=, split=, tile_m=, ...); cut = whether the launcher's plan cuts K over workgroups, which the device test
    reads off the workspace query (True: bytes > 0; False: 0)"""
    probs = probs if isinstance(probs, list) else [probs]
    r = dict(entry=entry, variant=variant, name=name, tile=own, probs=probs, launches=launches, opts=opts, id="%s-%s" % (variant, name))
    assert r["id"] not in [x["id"] for x in RUNS], r["id"]
    RUNS.append(r)
    return r


LAY = {NT: "nt", NN: "nn", TN: "tn"}
GENERIC = {1: (128, 128), 2: (64, 64), 4: (128, 64)}
# sdumc_gemm_f32, the register-staged kernels: any M, N, K.  tile = 4 is reported under the 64x64 name (the profile knows two names
# per layout); the launcher's dispatch (gemm_f32.hip: `tile == 4 ? launch<128, 64>`) names it.
for _lay in (NT, NN, TN):
    for _t, (_bm, _bn) in GENERIC.items():
        _v = "gemm_%s_%s" % (LAY[_lay], "128x128" if _t == 1 else "64x64")
        run("f32", _v, "t%d_plus1" % _t, (_bm, _bn), P(_bm + 1, 2 * _bn - 1, 77, layout=_lay), tile=_t, splitk=1)
        run("f32", _v, "t%d_split3" % _t, (_bm, _bn), P(2 * _bm - 1, _bn + 1, 130, layout=_lay, acc=True, colsum=_lay == TN), tile=_t, splitk=3, cut=True)
    run("f32", "gemm_%s_64x64" % LAY[_lay], "autosplit_K2080", (64, 64), P(64, 65, 2080, layout=_lay, colsum=_lay == TN), tile=2, splitk=0, cut=True)
    run("f32", "gemm_%s_64x64" % LAY[_lay], "auto_nosplit_K40", (64, 64), P(65, 64, 40, layout=_lay), tile=2, splitk=0, cut=False)
    run("f32", "gemm_%s_128x128" % LAY[_lay], "full_K16", (128, 128), P(128, 128, 16, layout=_lay), tile=1, splitk=1)
    run("f32", "gemm_%s_64x64" % LAY[_lay], "min_1x1x1", (64, 64), P(1, 1, 1, layout=_lay), tile=2, splitk=1)
    # the small-problem kernel: 32 x 32 tiles, the four waves split K; c_mask_y selects it
    run("f32", "gemm_small_%s" % LAY[_lay], "plus1", (32, 32), P(33, 63, 77, layout=_lay), tile=3, splitk=1)
    run("f32", "gemm_small_%s" % LAY[_lay], "masky_acc", (32, 32), P(63, 33, 130, layout=_lay, masky=True, acc=True), tile=0, splitk=1)
    run("f32", "gemm_small_%s" % LAY[_lay], "full_K8", (32, 32), P(32, 32, 8, layout=_lay, colsum=_lay == TN), tile=3, splitk=1)
    # bf16 operands (sdumc_gemm.bf16): K, lda, ldb multiples of 4; NN: N too; TN: M and N
    for _t in (1, 2):
        _bm, _bn = GENERIC[_t]
        run("f32", "gemm_bf16_%s_%s" % (LAY[_lay], "128x128" if _t == 1 else "64x64"), "t%d" % _t, (_bm, _bn),
            P(_bm + (4 if _lay == TN else 1), _bn + 60, 76, layout=_lay, bf16=True), tile=_t, splitk=1, bf16=True)
run("f32", "gemm_nt_64x64", "bias_tanh", (64, 64), P(65, 127, 40, bias=True, act=ACT_TANH), tile=2, splitk=1)
run("f32", "gemm_nt_64x64", "bias_rowmod", (64, 64), P(130, 65, 77, bias=True, amod=65), tile=2, splitk=1)
run("f32", "gemm_nn_64x64", "bias_relu", (64, 64), P(127, 65, 77, layout=NN, bias=True, act=ACT_RELU), tile=2, splitk=1)
run("f32", "gemm_tn_64x64", "browmod_colsum", (64, 64), P(65, 127, 130, layout=TN, bmod=50, colsum=True), tile=2, splitk=2)
run("f32", "gemm_nt_64x64", "two_groups", (64, 64), [P(65, 64, 40), P(65, 64, 40)], tile=2, splitk=1)
# strided-batched mode: three products of one shape behind each other in memory (the QK^T / PV products of the transformer)
run("f32", "gemm_nt_64x64", "batch3", (64, 64), [P(65, 63, 40) for _ in range(3)], tile=2, splitk=1, batch=3)
run("f32", "gemm_nn_64x64", "batch3", (64, 64), [P(63, 65, 77, layout=NN) for _ in range(3)], tile=2, splitk=1, batch=3)

# gemm_wide.hip, NT: N a multiple of the tile's width, K of 16, M >= 4.  Both settings of split bit 1.
WIDE = {11: (64, 256), 12: (128, 256), 13: (128, 128), 14: (64, 128)}
for _t, (_bm, _bn) in WIDE.items():
    for _split, _v in ((1, "gemm_wide_nt_bf16x3"), (0, "gemm_wide_nt")):
        run("f32", _v, "t%d_plus1" % _t, (_bm, _bn), P(_bm + 1, _bn, 48), tile=_t, splitk=1, split=_split)
        run("f32", _v, "t%d_bias_rowmod" % _t, (_bm, _bn), P(2 * _bm - 2, 2 * _bn, 272, bias=True, amod=_bm - 1), tile=_t, splitk=1, split=_split)
    run("f32", "gemm_wide_nt_bf16x3", "t%d_min4" % _t, (_bm, _bn), P(4, _bn, 16), tile=_t, splitk=1, split=1)
# tile = 15 .. 18 named persistent NT kernels that no longer exist: sdumc_gemm_wide_ declines them and the call must run, and report, the
# generic 64 x 64 kernel -- the silent change of route the recorded launch is there to see
run("f32", "gemm_nt_64x64", "tile15_is_the_generic_kernel", (64, 64), P(65, 256, 48), tile=15, splitk=1)
# a_drop / b_drop with keep-bits attached (ab_drop_bits: byte [row * width / 4 + q], rows = m for A, k for B): the masked loaders
for _split, _v in ((1, "gemm_wide_nt_bf16x3"), (0, "gemm_wide_nt")):
    run("f32", _v, "t13_bits_rowmod", (128, 128), P(2 * 129, 128, 48, keep="A", amod=129), tile=13, splitk=1, split=_split)
    run("f32", _v, "t14_bits_bias_tanh", (64, 128), P(65, 256, 272, keep="A", bias=True, act=ACT_TANH), tile=14, splitk=1, split=_split)
run("f32", "gemm_wide_tn", "t13_bits_split2", (128, 128), P(128, 128, 144, layout=TN, keep="B", colsum=True), tile=13, splitk=2, cut=True)
run("f32", "gemm_nt_64x64", "bits_rowmod", (64, 64), P(130, 65, 76, keep="A", amod=65), tile=2, splitk=1)
run("f32", "gemm_nn_64x64", "bits", (64, 64), P(65, 68, 76, layout=NN, keep="A"), tile=2, splitk=1)
run("f32", "gemm_tn_64x64", "bits_colsum", (64, 64), P(65, 68, 130, layout=TN, keep="B", colsum=True), tile=2, splitk=2, cut=True)
run("f32", "gemm_wide_nt_bf16x3", "auto14_M8192", (64, 128), P(8192, 128, 512), tile=0, splitk=1, split=1)
run("f32", "gemm_wide_nt_bf16x3", "auto13_M32768", (128, 128), P(32768, 128, 128), tile=0, splitk=1, split=1)
# TN: M a multiple of the tile's height too; K ragged; split-K over workgroups (auto: K / 16 / 8 pieces at most)
for _t in (11, 13, 14):
    _bm, _bn = WIDE[_t]
    run("f32", "gemm_wide_tn", "t%d_K77" % _t, (_bm, _bn), P(_bm, _bn, 77, layout=TN), tile=_t, splitk=1, cut=False)
    run("f32", "gemm_wide_tn", "t%d_autosplit_K2064" % _t, (_bm, _bn), P(2 * _bm, _bn, 2064, layout=TN, colsum=True, bmod=1040), tile=_t, splitk=0, cut=True)
    run("f32", "gemm_wide_tn", "t%d_split2_acc" % _t, (_bm, _bn), P(_bm, 2 * _bn, 130, layout=TN, colsum=True, acc=True), tile=_t, splitk=2, cut=True)

# sdumc_gemm_bf16_run: bf16 storage.  NT 64 x 128 tiles below 16384 rows, 128 x 128 from there; TN 128 x 128.  K % 64 (NT), extents % 8.
run("bf16", "gemm_bf16s_nt", "plus1", (64, 128), P(65, 248, 64, bf16=True))
run("bf16", "gemm_bf16s_nt", "bf16c_bias_tanh", (64, 128), P(127, 136, 192, bf16=True, bf16out=True, bias=True, act=ACT_TANH))
run("bf16", "gemm_bf16s_nt", "bf16c", (64, 128), P(65, 256, 128, bf16=True, bf16out=True))
run("bf16", "gemm_bf16s_nt", "acc", (64, 128), P(64, 128, 128, bf16=True, acc=True))
run("bf16", "gemm_bf16s_nt", "bf16c_acc", (64, 128), P(66, 128, 64, bf16=True, bf16out=True, acc=True))
run("bf16", "gemm_bf16s_nt", "rowmod", (64, 128), P(130, 128, 64, bf16=True, amod=65))
run("bf16", "gemm_bf16s_nt", "split2", (64, 128), P(65, 128, 256, bf16=True, bias=True), splitk=2, cut=True)
run("bf16", "gemm_bf16s_nt", "autosplit_K4096", (64, 128), P(65, 128, 4096, bf16=True), splitk=0, cut=True)
run("bf16", "gemm_bf16s_nt", "auto128_M16384", (128, 128), P(16385, 128, 64, bf16=True))
run("bf16", "gemm_bf16s_tn", "plus8_K77", (128, 128), P(136, 248, 77, layout=TN, bf16=True), splitk=1, cut=False)
run("bf16", "gemm_bf16s_tn", "autosplit_K2056", (128, 128), P(256, 128, 2056, layout=TN, bf16=True, colsum=True, bmod=1032), splitk=0, cut=True)
run("bf16", "gemm_bf16s_tn", "split3_acc", (128, 128), P(128, 136, 200, layout=TN, bf16=True, colsum=True, acc=True), splitk=3, cut=True)

# sdumc_gemm_group_tn: stream-K over 256 x 128 output tiles (fp32 MFMAs, bf16 storage) or 256 x 256 (split bit 0).  M, N % 4 (8: bf16);
# b_row_mod >= 16 (64).  `cut`: ONE tile with 131 k-tiles (bf16: 33) and nothing else on the line -- every workgroup holds a piece of it;
# `whole`: 8 rows, 521 / 1041 / 1041 tiles of K = 16 (split / fp32 MFMA / bf16) -- a workgroup's range is 11 / 17 / 25 line units long
# on 256 CUs and a tile takes 5 / 4 / 6, so every range holds whole tiles (and the tiles at its two ends are cut)
for _v, _bn, _split, _hf in (("gemm_group_tn_bf16x3", 256, 1, False), ("gemm_group_tn", 128, 0, False), ("gemm_group_tn_bf16", 128, 1, True)):
    _kw = dict(layout=TN, bf16=_hf)
    _o = dict(split=_split)
    run("group", _v, "cut_K2090", (256, _bn), P(256, _bn, 2090, colsum=True, **_kw), **_o)
    run("group", _v, "whole_K16", (256, _bn), P(8, 256 * 520 + 8, 16, **_kw), **_o)
    run("group", _v, "plus4_acc", (256, _bn), P(256 + 8, _bn + 8, 77, acc=True, colsum=True, **_kw), **_o)
    run("group", _v, "two_segments_rowmod", (256, _bn), P(64, 136, 300, K1=77, bmod=100, **_kw), **_o)
    if not _hf:
        run("group", _v, "two_segments_keepbits", (256, _bn), P(72, 128, 130, K1=40, keep="B", bmod1=24, colsum=True, **_kw), **_o)
    if _split:
        run("group", _v, "bmap", (256, _bn), P(64, 264, 130, K1=48, bmap=True, **_kw), **_o)
    run("group", _v, "mixed_list", (256, _bn), [P(8, 8, 1, **_kw), P(264, _bn + 8, 600, acc=True, **_kw), P(16, 520, 40, K1=16, colsum=True, **_kw),
                                               P(256, _bn, 16, **_kw)], **_o)

# sdumc_gemm_p3_nt: N % 256, K % 64; tile_m rows x 256 columns (0: 64 rows on 256 threads)
for _tm in (0, 64, 96, 128):
    _bm = _tm or 64
    run("p3", "gemm_p3_nt_bf16x3", "tm%d_plus1" % _tm, (_bm, 256), P(_bm + 1, 256, 64), tile_m=_tm, splitk=1, want_p3=True, cut=False)
    run("p3", "gemm_p3_nt_bf16x3", "tm%d_split4_bias" % _tm, (_bm, 256), P(3 * _bm - 1, 512, 2048, bias=True), tile_m=_tm, splitk=4, want_p3=True, cut=True)
    run("p3", "gemm_p3_nt_masked_bf16x3", "tm%d_bits_rowmod_tanh" % _tm, (_bm, 256), P(2 * _bm + 2, 256, 128, keep="A", amod=_bm + 1, bias=True, act=ACT_TANH), tile_m=_tm)
    run("p3", "gemm_p3_nt_masked_bf16x3", "tm%d_bits" % _tm, (_bm, 256), P(_bm + 63, 256, 192, keep="A"), tile_m=_tm)
for _tm in (0, 128):
    run("p3", "gemm_p3_nt_bf16x3", "tm%d_a2" % _tm, (_tm or 64, 256), P(128 + 65, 256, 128, a2=128, bias=True), tile_m=_tm)
run("p3", "gemm_p3_nt_bf16x3", "autosplit_K4096", (64, 256), P(65, 256, 4096), tile_m=0, splitk=0, cut=True)
for _rows in (0, 1):
    run("p3", "gemm_p3_nt_bf16x3", "map%s" % ("_rows" if _rows else ""), (64, 256), P(129, 256, 128, amap=True, bias=True), map_rows=_rows, want_p3=True)
    run("p3", "gemm_p3_nt_bf16x3", "map_a2%s" % ("_rows" if _rows else ""), (64, 256), P(64 + 63, 256, 64, amap=True, a2=64), map_rows=_rows)

# sdumc_gemm_b1_nt: bf16 storage, N % 256, K % 128, 64 x 256 tiles
run("b1", "gemm_b1_nt_bf16", "plus1_f32c", (64, 256), P(65, 256, 128, bf16=True), splitk=1, cut=False)
run("b1", "gemm_b1_nt_bf16", "bf16c_bias_tanh", (64, 256), P(127, 512, 256, bf16=True, bf16out=True, bias=True, act=ACT_TANH), splitk=1)
run("b1", "gemm_b1_nt_bf16", "bf16c", (64, 256), P(66, 256, 128, bf16=True, bf16out=True), splitk=1)
run("b1", "gemm_b1_nt_bf16", "split4_bias", (64, 256), P(191, 256, 2048, bf16=True, bias=True), splitk=4, cut=True)
run("b1", "gemm_b1_nt_bf16", "autosplit_K4096", (64, 256), P(65, 256, 4096, bf16=True), splitk=0, cut=True)
run("b1", "gemm_b1_nt_bf16", "rowmod", (64, 256), P(130, 256, 128, bf16=True, amod=65, bias=True), splitk=1)
run("b1", "gemm_b1_nt_bf16", "a2", (64, 256), P(128 + 65, 256, 128, bf16=True, a2=128), splitk=1)
for _rows in (0, 1):
    run("b1", "gemm_b1_nt_bf16", "map_a2%s" % ("_rows" if _rows else ""), (64, 256), P(64 + 63, 256, 128, bf16=True, amap=True, a2=64, bias=True), splitk=1, map_rows=_rows)

# sdumc_gemm_rows256: K = N = 256, 64-row tiles; the pooling term and the fold need split bit 3
for _v, _split, _hf in (("gemm_rows256_bf16x3", 1, False), ("gemm_rows256", 0, False), ("gemm_rows256_bf16", 1, True)):
    _kw = dict(layout=NT if _hf else NN, bf16=_hf, bf16out=_hf)      # (bf16: B is [256 n][256 k], C = A B^T)
    _o = dict(split=_split)
    run("rows", _v, "plus1", (64, 256), P(65, 256, 256, **_kw), **_o)
    run("rows", _v, "acc_two_problems", (64, 256), [P(127, 256, 256, acc=True, **_kw), P(64, 256, 256, acc=True, **_kw)], **_o)
    if not _hf:
        run("rows", _v, "bits_rowmod_bias_tanh", (64, 256), P(130, 256, 256, keep="A", amod=65, bias=True, act=ACT_TANH, **_kw), **_o)
        run("rows", _v, "bits", (64, 256), P(66, 256, 256, keep="A", **_kw), **_o)
    else:
        run("rows", _v, "rowmod_bias_tanh", (64, 256), P(130, 256, 256, amod=65, bias=True, act=ACT_TANH, **_kw), **_o)
    if _split:
        if not _hf:
            run("rows", _v, "pool_T65_nq7", (64, 256), P(195, 256, 256, pool=(65, 7), **_kw), **_o)
            run("rows", _v, "pool_T32_nq1", (64, 256), P(160, 256, 256, pool=(32, 1), **_kw), **_o)
        run("rows", _v, "fold1_bits", (64, 256), P(195, 256, 256, pool=(65, 7), fold=1, cbits=True, **_kw), **_o)
        run("rows", _v, "fold2_bits_acc", (64, 256), P(2 * 130, 256, 256, pool=(65, 1), fold=2, cbits=True, acc=True, **_kw), **_o)
        run("rows", _v, "fold2_nobits", (64, 256), P(2 * 96, 256, 256, pool=(32, 7), fold=2, **_kw), **_o)
        run("rows", _v, "fold1_acc_nobits", (64, 256), P(130, 256, 256, pool=(65, 7), fold=1, acc=True, **_kw), **_o)

# sdumc_frame_dx: C = dz [M, 256] . W [256, N], N % 256.  The split route has no profile hook: the launcher's dispatch names it
# (frame_dx.hip: bit 1 on -> frame_dx_kernel, nothing recorded; off -> the NN form of sdumc_gemm_f32, which IS recorded)
for _v, _split, _tile in (("frame_dx_bf16x3", 1, (64, 256)), ("gemm_small_nn", 0, (32, 32))):
    for _packed in (0, 1):
        if _packed and not _split:
            continue
        _n = "packed" if _packed else "unpacked"
        run("dx", _v, "dx_%s_plus1" % _n, _tile, P(65, 256, 256, layout=NN), split=_split, packed=_packed, launches=_split ^ 1)
        run("dx", _v, "dx_%s_lengths" % _n, _tile, P(195, 512, 256, layout=NN, lens=(65, (65, 0, 20))), split=_split, packed=_packed, launches=_split ^ 1)

IDS = [r["id"] for r in RUNS]
# what no run holds, and why (profiles/gemm_parity_by_route.txt names them too)
LEFT_OUT = {
    "wide 15-18 (persistent NT)": "no such kernels: removed in round 3 (gemm_wide.hip); sdumc_gemm_wide_ declines cfg 5..8 and the call "
                                  "runs gemm_nt_64x64 (held: tile15_is_the_generic_kernel)",
    "dropout descriptors WITHOUT keep-bits (Philox recomputed in the loader), epilogue dropout": "the masks themselves are held bit for bit by the dropout "
                                                                    "tests; every masked loader is held here with keep-bits attached",
}


def by_id(i):
    return RUNS[IDS.index(i)]


def rule_of(p):
    return "bf16out" if p["bf16out"] else "act" if p["act"] else "f32"


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def pack_bits(keep):
    """bool [rows, cols] -> uint8 [rows, cols / 4]: bit e of byte q = keep column 4 q + e (as sdumc_dropout_bits writes them)"""
    r, c = keep.shape
    return (keep.reshape(r, c // 4, 4).to(torch.int32) * torch.tensor([1, 2, 4, 8], dtype=torch.int32)).sum(-1).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def _operands(rid, i):
    r = by_id(rid)
    p = r["probs"][i]
    g = torch.Generator().manual_seed(zlib.crc32(("%s/%d" % (rid, i)).encode()))
    rn = lambda *s: torch.randn(*s, generator=g)
    M, N, lay = p["M"], p["N"], p["layout"]
    Ks = [k for k in (p["K"], p["K1"]) if k]
    Kt = sum(Ks)
    scaled = p["act"] == ACT_NONE
    pw2 = lambda n: torch.exp2(torch.randint(-12, 13, (n,), generator=g).float())
    R = M // p["fold"] if p["fold"] else M
    ra = pw2(M) if scaled and not p["bias"] else torch.ones(M)
    rb = pw2(N) if scaled else torch.ones(N)
    if p["amod"]:
        ra = ra[torch.arange(M) % p["amod"]]
    if p["fold"]:
        ra = ra[torch.arange(M) % R]
    I = dict(ra=ra, rb=rb, Ks=Ks)
    # A: what the call's A tensor(s) hold.  NT / NN: [rows, K] per source row; TN: [K_s, M] per segment
    if lay == TN:
        I["A"] = [rn(k, M) * ra for k in Ks]
        Ae = torch.cat(I["A"]).t()
        I["B"], parts = [], []
        for s, k in enumerate(Ks):
            mod = p["bmod1" if s else "bmod"]
            Bs = rn(mod or k, N) / Kt ** 0.5 * rb
            I["B"].append(Bs)
            parts.append(Bs[torch.arange(k) % mod] if mod else Bs)
        Bv = torch.cat(parts)                            # [K, N] virtual rows
        if p["bmap"]:                                     # every fifth k-row is a padded frame: it names the store's all-zero row
            Bv[::5] = 0.0
        Be = Bv.t()
    else:
        rows = p["amod"] or M
        A = rn(rows, Kt) * ra[:rows, None]
        if p["amap"]:
            A[::5] = 0.0
        I["A"] = [A]
        Ae = A[torch.arange(M) % p["amod"]] if p["amod"] else A
        B = rn(N, Kt) / Kt ** 0.5 * rb[:, None]
        I["B"] = [B if lay == NT else B.t().contiguous()]
        Be = B
    if p["bf16"]:
        I["A"], I["B"] = [t.bfloat16().float() for t in I["A"]], [t.bfloat16().float() for t in I["B"]]
        Ae, Be = Ae.bfloat16().float(), Be.bfloat16().float()
    if p["bmap"]:
        I["B"] = list(torch.split(Be.t().contiguous(), Ks))      # the VIRTUAL rows: the device test scatters them into the store
    if p["keep"]:
        keep = torch.rand(*((M, Kt) if p["keep"] == "A" else (Kt, N)), generator=g) >= 0.5
        I["keep"], I["scale"] = keep, 2.0
        if p["keep"] == "A":
            Ae = Ae * keep * 2.0
        else:
            Be = Be * keep.t() * 2.0
    I["Ae"], I["Be"] = Ae.contiguous(), Be.contiguous()
    if p["bias"]:
        I["bias"] = rn(N) * rb
    if p["acc"]:
        I["C0"] = rn(R, N) * ra[:R, None] * rb
        if p["bf16out"]:
            I["C0"] = I["C0"].bfloat16().float()
        if p["colsum"]:
            I["cs0"] = rn(M) * ra
    if p["masky"]:
        I["Y"], I["mask_scale"] = rn(M, N), 2.0
    if p["pool"]:
        T, nq = p["pool"]
        I["pool_w"] = torch.softmax(rn(M // T, T, nq), dim=1).reshape(M, nq) * ra[:, None]
        I["pool_g"] = rn(M // T, nq, N) * (torch.rand(M // T, nq, N, generator=g) > 0.3) * rb
    if p["cbits"]:
        I["ckeep"], I["c_scale"] = torch.rand(M, N, generator=g) >= 0.5, 2.0
    if p["amap"] or p["bmap"]:
        # the packed store: 7 rows more than the batch names, the all-zero row among them; -> store row of every virtual row, per tensor
        maps = []
        bounds = [0, p["a2"], M] if p["a2"] else ([0, M] if p["amap"] else [0] + list(np.cumsum(Ks)))
        V = Ae if p["amap"] else Be.t()
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            n = hi - lo
            perm = torch.randperm(n + 7, generator=g)
            zero_row = int(perm[n])
            m = perm[:n].clone()
            m[(V[lo:hi] == 0).all(1)] = zero_row
            maps.append((m.to(torch.int32), n + 7, zero_row))
        I["maps"] = maps
    return I


def operands(r, i=0):
    """fp32 CPU inputs of problem i of a run (never to be written to): the tensors the call is given (A, B: lists, one per segment /
    as stored), the effective matrices Ae [M, K] and Be [N, K] the restatement multiplies, the factors ra [M] and rb [N], and whatever
    else the problem's form reads"""
    return _operands(r["id"], i)


def out_rows(p):
    return p["M"] // p["fold"] if p["fold"] else p["M"]


def zero_rows(p):
    """frame_dx with lengths: bool [M], the rows written as exact +0.0"""
    z = torch.zeros(p["M"], dtype=torch.bool)
    if p["lens"]:
        T, L = p["lens"]
        for b, n in enumerate(L):
            z[b * T + n:(b + 1) * T] = True
    return z


def epilogue(p, I, C, dtype, cs=None):
    """everything behind the K sum (module docstring); C [M, N] at dtype -> name -> tensor"""
    t = lambda x: x.to(dtype)
    M, N = p["M"], p["N"]
    if p["pool"]:
        T, nq = p["pool"]
        pw, pg = t(I["pool_w"]), t(I["pool_g"])
        v = torch.arange(M) // T
        for i in range(nq):
            C = C + pw[:, i, None] * pg[v, i, :]
    if p["fold"]:
        if p["cbits"]:
            C = C * t(I["ckeep"]) * I["c_scale"]
        C = C.view(p["fold"], M // p["fold"], N)
        C = _acc(p["fold"], lambda s: C[s])
    if p["bias"]:
        C = C + t(I["bias"])
    if p["act"] == ACT_TANH:
        C = torch.tanh(C)
    elif p["act"] == ACT_RELU:
        C = torch.relu(C)
    if p["acc"]:
        C = C + t(I["C0"])
    if p["masky"]:
        C = C * t(I["Y"] > 0) * I["mask_scale"]
    if p["lens"]:
        C = C.masked_fill(zero_rows(p)[:, None], 0.0)
    if p["bf16out"]:
        C = round_bf16(C) if dtype == torch.float64 else C.bfloat16().float()
    out = {"C": C}
    if p["colsum"]:
        out["colsum"] = cs + t(I["cs0"]) if p["acc"] else cs
    return out


@functools.lru_cache(maxsize=None)
def _reference(rid, i, dtype):
    r = by_id(rid)
    p, I = r["probs"][i], _operands(rid, i)
    Ae, Be = I["Ae"].to(dtype), I["Be"].to(dtype)
    K = Ae.shape[1]
    C = _acc(K, lambda k: Ae[:, k, None] * Be[None, :, k])
    cs = _acc(K, lambda k: Ae[:, k]) if p["colsum"] else None
    return epilogue(p, I, C, dtype, cs)


def reference(r, i=0, dtype=torch.float64):
    """name -> tensor ("C", "colsum") of problem i at `dtype` (float64 = ref_hi, float32 = ref_lo); computed once per process, shared,
    never to be written to.  A bf16 output is the ROUNDED one in both."""
    return _reference(r["id"], i, dtype)


# ---- slices and the judgement ------------------------------------------------------------------------------------------------------
def slices(r, i, outs):
    """name -> slice of problem i's outputs, divided by the known factor ra[m] rb[n]: one per tile of the route, cut to the valid
    extent; colsum as one slice"""
    p, I = r["probs"][i], operands(r, i)
    bm, bn = r["tile"]
    Rm = out_rows(p)
    ra, rb = I["ra"][:Rm].double(), I["rb"].double()
    pre = "p%d." % i if len(r["probs"]) > 1 else ""
    out = {}
    for k, t in outs.items():
        t = t.detach().cpu().double()
        if k == "colsum":
            out[pre + k] = t.reshape(-1) / I["ra"].double()
            continue
        t = t.reshape(Rm, p["N"]) / (ra[:, None] * rb[None, :])
        for a in range((Rm + bm - 1) // bm):
            for b in range((p["N"] + bn - 1) // bn):
                out["%s%s[%d,%d]" % (pre, k, a, b)] = t[a * bm:(a + 1) * bm, b * bn:(b + 1) * bn]
    return out


def zero_slices(r, i):
    """the slices that are exactly zero in fp64: frame_dx tiles whose rows all lie beyond their sample's length"""
    p = r["probs"][i]
    if not p["lens"]:
        return ()
    z, (bm, bn) = zero_rows(p), r["tile"]
    return tuple("C[%d,%d]" % (a, b) for a in range((p["M"] + bm - 1) // bm) if bool(z[a * bm:(a + 1) * bm].all())
                 for b in range((p["N"] + bn - 1) // bn))


def bars_of(rule, hi, lo):
    """the bar of every slice, from the two references alone (module docstring)"""
    if rule == "act":
        return {k: BAR_OUT for k in hi}
    if rule == "bf16out":
        return {k: 4 * BF16_E_REF for k in hi}
    bars = {}
    for k in hi:
        n = float(hi[k].norm())
        e = float((lo[k].double() - hi[k]).norm()) / n if n else 0.0
        bars[k] = min(BAR_OUT, max(4 * e, FLOOR))
    return bars


def judge(r, got, what=None):
    """the device's (or a stand-in's) outputs of every problem of a run -- got: list of name -> tensor -- against ref_hi, slice by
    slice.  -> (TensorErrors, the run's line)"""
    from tests import grad_parity as GP
    G, H, L, bars, zeros = {}, {}, {}, {}, []
    for i, p in enumerate(r["probs"]):
        hi, lo = reference(r, i), reference(r, i, torch.float32)
        assert set(got[i]) == set(hi), (set(got[i]), set(hi))
        g, h, l = slices(r, i, got[i]), slices(r, i, hi), slices(r, i, lo)
        G.update(g), H.update(h), L.update(l)
        bars.update(bars_of(rule_of(p), h, l))
        zeros += list(zero_slices(r, i))
    res = GP.tensor_errors(list(H), G, H, L, bars, zeros=tuple(zeros), what=what or r["id"], nosignal=(), max_between=0, keep_old=False)
    assert not res.between, (r["id"], res.between)
    k = max(res, key=res.get)
    line = "gemm route %s | %s | worst %s = %.3g (e_ref %.2g, bar %.3g)" % (r["variant"], r["name"], k, res[k], res.e_ref[k], res.bars[k])
    print(line)
    return res, line


# ---- stand-ins for the device (tests/test_gemm_parity_cpu.py) ---------------------------------------------------------------------
SIX = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))


def split3(x):
    """fp32 -> its three bf16 parts (round to nearest, exact residuals), as fp32 tensors"""
    p0 = x.bfloat16().float()
    r1 = x - p0
    p1 = r1.bfloat16().float()
    return p0, p1, (r1 - p1).bfloat16().float()


def standin(r, i=0, parts=SIX, skip_block=None, swap_row=None):
    """the split arithmetic modelled on the host: per k-block of 16 the part products (each exact) are added onto an fp32 accumulator.
    parts: the part pairs summed (SIX = the kernels' six; without (2, 0) = the fault the old bar accepted).  skip_block = (tile row,
    tile column, k-block): that block is left out of that tile.  swap_row = (tile row, tile column): the last row of that tile holds
    its neighbour row's values.  -> name -> tensor, like reference()"""
    p, I = r["probs"][i], operands(r, i)
    Ae, Be = I["Ae"], I["Be"]
    M, K = Ae.shape
    a3, b3 = split3(Ae), split3(Be)
    bm, bn = r["tile"]
    acc = torch.zeros(M, Be.shape[0])
    for k0 in range(0, K, 16):
        for (x, y) in parts:
            c = a3[x][:, k0:k0 + 16].double() @ b3[y][:, k0:k0 + 16].double().t()
            if skip_block is not None and skip_block[2] == k0 // 16:
                ta, tb = skip_block[:2]
                c[ta * bm:(ta + 1) * bm, tb * bn:(tb + 1) * bn] = 0.0
            acc = (acc.double() + c).float()
    if swap_row is not None:
        ta, tb = swap_row
        last = int(torch.nonzero(~zero_rows(p)[:(ta + 1) * bm])[-1])      # the tile's last valid row
        acc[last, tb * bn:(tb + 1) * bn] = acc[last - 1, tb * bn:(tb + 1) * bn]
    cs = _acc(K, lambda k: Ae[:, k]) if p["colsum"] else None
    return epilogue(p, I, acc, torch.float32, cs)
