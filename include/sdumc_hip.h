/* sdumc_hip.h — C ABI of libsdumc_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the ONE hot path of WarmCongee/SDUMC: the
 * WengnetMOSEIMultViewsTextMissing forward/backward, its losses and the Adam
 * step.  The reference has no native code; what its Python calls
 * on this path are torch eager ops.  Each entry point below names the reference
 * code it replaces (file:line relative to the reference repo).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless stated otherwise;
 *     tensors are dense row-major with the strides given;
 *   - every function enqueues work on `stream` (a hipStream_t passed as void*)
 *     and returns immediately: no allocation, no synchronisation, no host
 *     copies -> every call is hipGraph-capturable;
 *   - `stream` must belong to the CURRENT device (hipSetDevice) of the calling thread, like any HIP launch; the
 *     network-level calls keep their internal streams per device (or per caller context, sdumc_net_io.ctx), so calls
 *     on different devices or with different contexts share no state and may run from different host threads;
 *   - return value: 0 = ok, <0 = SDUMC_E* (never throws across the ABI);
 *   - scratch memory is caller-owned; *_workspace_bytes() says how much.
 */
#ifndef SDUMC_HIP_H
#define SDUMC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDUMC_OK 0
#define SDUMC_EINVAL (-1)   /* bad argument (shape, alignment, null pointer) */
#define SDUMC_ELAUNCH (-2)  /* hipLaunch / HIP runtime error */
#define SDUMC_ENOMEM (-3)   /* workspace too small */

#define SDUMC_MAX_GROUPS 8
#define SDUMC_D 256         /* general_dim            (model :191) */
#define SDUMC_H 128         /* layers_list[-1]        (model :187) */
#define SDUMC_NQ 7          /* multi-view queries     (model :332) */
#define SDUMC_RNC_DIM 64    /* orgin_linear_change out (model :246-250) */
#define SDUMC_N_SITES 35    /* nn.Dropout call sites of one forward */

/* ------------------------------------------------------------------------
 * Dropout descriptor.  Replaces nn.Dropout / aten::bernoulli_ (model :54,:77,
 * :270).  Masks are a pure function of (seed, call, site, sample, row, col):
 * Philox4x32-10, ctr = (row*(width/4)+col/4, sample0+sample, site, call+stream),
 * key = seed; element dropped when word[col%4] < threshold; kept elements are
 * multiplied by `scale`.  The row space of the tensor the descriptor is attached
 * to is [streams][samples][rows][width].
 * ---------------------------------------------------------------------- */
typedef struct sdumc_dropout {
  uint32_t enabled;    /* 0 = identity (eval mode) */
  uint32_t site;       /* 0..SDUMC_N_SITES-1 */
  uint32_t threshold;  /* floor(p * 2^32) */
  float scale;         /* 1/(1-p) */
  uint32_t rows;       /* rows per sample (T, NQ or 1) */
  uint32_t width;      /* row width; a multiple of 4 wherever the mask is fused into a GEMM */
  uint32_t samples;    /* samples per stream (local batch B) */
  uint32_t sample0;    /* global index of local sample 0 (data-parallel shard offset) */
  uint32_t call0;      /* Philox call index of stream 0 (ignored when dev_state != NULL) */
  uint32_t stream0;    /* added to the stream index (a tensor that holds only stream 1 passes 1) */
  uint32_t seed_lo, seed_hi;
  const uint32_t* dev_state; /* optional device {seed_lo, seed_hi, call0}: lets a captured
                                hipGraph draw fresh masks on every replay */
  const uint8_t* bits;       /* optional keep-bits precomputed by sdumc_dropout_bits for exactly this row space:
                                byte [row * width/4 + q], bit e = keep column 4q+e.  Kernels that stage the same
                                tile several times (4 n-tiles of a GEMM, forward + backward) then read one byte
                                instead of re-running Philox (~90 VALU ops per 4 elements) */
} sdumc_dropout;

/* ------------------------------------------------------------------------
 * fp32 MFMA GEMM (v_mfma_f32_32x32x2_f32), grouped, with the fusions this path
 * needs.  Replaces F.linear / torch.bmm / their autograd (aten::addmm, mm).
 *   layout SDUMC_NT: C[M,N] = A[M,K] . B[N,K]^T   (forward Linear: x.W^T)
 *   layout SDUMC_NN: C[M,N] = A[M,K] . B[K,N]     (dX = dY.W)
 *   layout SDUMC_TN: C[M,N] = A[K,M]^T . B[K,N]   (dW = dY^T.X)
 * ---------------------------------------------------------------------- */
enum { SDUMC_NT = 0, SDUMC_NN = 1, SDUMC_TN = 2 };
enum { SDUMC_ACT_NONE = 0, SDUMC_ACT_RELU = 1, SDUMC_ACT_TANH = 2 };

typedef struct sdumc_gemm {
  int32_t layout, M, N, K;
  int32_t groups;                        /* 1..SDUMC_MAX_GROUPS independent problems of one shape */
  const float* A[SDUMC_MAX_GROUPS];
  const float* B[SDUMC_MAX_GROUPS];
  float* C[SDUMC_MAX_GROUPS];
  const float* bias[SDUMC_MAX_GROUPS];   /* [N] or NULL */
  int32_t lda, ldb, ldc;
  int32_t a_row_mod;   /* >0: A's source row = row % a_row_mod (NT/NN rows = m; TN rows = k).
                          Lets the two streams share one x_audio / x_video in HBM. */
  int32_t b_row_mod;   /* TN only: B's source row = k % b_row_mod */
  sdumc_dropout a_drop; /* NT/NN: fused dropout on A as it is staged (rows = m, cols = k) */
  sdumc_dropout b_drop; /* TN: fused dropout on B as it is staged (rows = k, cols = n) */
  int32_t act;          /* epilogue activation */
  sdumc_dropout c_drop; /* epilogue dropout on C (rows = m, cols = n) */
  int32_t c_drop_group_stride; /* group g uses site c_drop.site + g * stride (grouped MLPs) */
  int32_t accumulate;   /* C += result (requires act none, no c_drop, no bias) */
  int32_t splitk;       /* 0: auto (tile + split chosen to fill 256 CUs); 1: no split; >1: K split over workgroups.
                           Split results go through fp32 slabs in `workspace` and an ordered, deterministic reduce */
  int32_t tile;         /* 0 auto, 1 = 128x128, 2 = 64x64, 4 = 128x64, 3 = small-problem kernel (32x32 tile, the four waves split K;
                           for the launch-bound utterance-level layers; no operand-side fusions) */
  int32_t ab_drop_group_stride; /* group g draws a_drop / b_drop from site + g * stride ... */
  const uint8_t* ab_drop_bits[SDUMC_MAX_GROUPS]; /* ... or from these per-group keep-bits (NULL: a_drop.bits / b_drop.bits) */
  const float* c_mask_y[SDUMC_MAX_GROUPS]; /* optional epilogue (selects the small-problem kernel): C = C * [Y > 0] * c_mask_scale,
                           Y laid out like C, applied after `accumulate`.  Folds the backward of the NEXT
                           Linear->ReLU->Dropout (dz = dy * [y > 0] / (1-p), model :264-273) into the dX GEMM */
  float c_mask_scale;
  float* colsum_a[SDUMC_MAX_GROUPS]; /* TN only, optional: out[m] (+)= sum_k A[k,m] fused into the staging of A
                           (the bias gradient when A = dz); `accumulate` applies to it too */
  int32_t bf16;         /* 1: operands rounded to bf16 while staged (row-contiguous ones transposed by their LDS stores),
                           v_mfma_f32_32x32x16_bf16, fp32 accumulate and fp32 epilogue / column sums (the "bf16 compute" mode,
                           BASELINE configs[2]; 64x64 and 128x128 tiles, channel extents multiples of 4); 0: exact fp32 (default) */
  float* workspace;
  size_t workspace_bytes;
  int32_t batch;        /* >1: strided-batched mode -- every group is `batch` products of one shape, entry z reads
                           A + z*stride_a, B + z*stride_b and writes C + z*stride_c (the per-(sample, head) QK^T / PV
                           products of sdumc_mha_*, multihead_attention.py:103,123: with [T, B, H*d_h] activations the
                           head slice of (b, h) starts at (b*H + h)*d_h, so one stride walks samples and heads).
                           Plain products only: no operand/epilogue dropout, bias, column sums or split-K */
  int64_t stride_a, stride_b, stride_c;   /* floats */
} sdumc_gemm;

size_t sdumc_gemm_workspace_bytes(const sdumc_gemm* g);
int sdumc_gemm_f32(const sdumc_gemm* g, void* stream);

/* ------------------------------------------------------------------------
 * GEMM on bf16 STORAGE (BASELINE configs[2], configs[4]): A and B are bf16 in HBM, products accumulate in fp32 on
 * v_mfma_f32_32x32x16_bf16, C is fp32 or bf16.  The frame-level products of the step in bf16 mode
 * (sdumc_net_dims.bf16 = 2): frame_dim_reshape (model :282-284), input_proj of FRA2UTT_new / Cross_Attention
 * (model :60, :82) and their autograd (main :149).
 *   SDUMC_NT: C[M,N] = A[M,K] . B[N,K]^T (+ bias, tanh / ReLU; accumulate: C += ...);  K a multiple of 64
 *   SDUMC_TN: C[M,N] = A[K,M]^T . B[K,N]  (fp32 C; split-K through fp32 slabs, ordered reduce; colsum_a = column sums of A)
 * Leading dimensions and the contiguous extents are multiples of 8 elements (16-byte rows), pointers 16-byte aligned.
 * No dropout descriptor: in bf16 mode the masked frames xd = drop(x) are materialised once (sdumc_mask_apply_bf16).
 * ---------------------------------------------------------------------- */
typedef struct sdumc_gemm_bf16 {
  int32_t layout, M, N, K, groups;
  const void* A[SDUMC_MAX_GROUPS];      /* bf16 */
  const void* B[SDUMC_MAX_GROUPS];      /* bf16 */
  void* C[SDUMC_MAX_GROUPS];            /* fp32, or bf16 when c_bf16 */
  const float* bias[SDUMC_MAX_GROUPS];  /* [N] fp32 or NULL */
  float* colsum_a[SDUMC_MAX_GROUPS];    /* TN only, optional: out[m] (+)= sum_k A[k, m] */
  int32_t lda, ldb, ldc;
  int32_t a_row_mod;                    /* NT: A's source row = m % a_row_mod (both streams share x in eval mode) */
  int32_t b_row_mod;                    /* TN: B's source row = k % b_row_mod */
  int32_t act, accumulate, c_bf16;
  int32_t splitk;                       /* TN: 0 auto, >= 1 explicit */
  float* workspace;
  size_t workspace_bytes;
} sdumc_gemm_bf16;
size_t sdumc_gemm_bf16_workspace_bytes(const sdumc_gemm_bf16* g);
int sdumc_gemm_bf16_run(const sdumc_gemm_bf16* g, void* stream);

/* ------------------------------------------------------------------------
 * Grouped weight-gradient GEMM: every dW = dz^T . x of a backward phase in ONE persistent launch (+ one ordered reduce).
 * Replaces the autograd products of the Linear layers (aten::mm of grad_output^T with the saved input, plus the bias
 * gradient's sum over rows) of model :282-284 (frame_dim_reshape), :60 / :82 (input_proj of FRA2UTT_new / Cross_Attention)
 * and :293-368 (utterance-level MLPs) when main :149 calls loss.backward().
 *   problem i:  C_i[M,N] (+)= sum over K-segments s of  A_is[K_s, M]^T . mask_is(B_is[K_s, N]),   colsum_i[m] (+)= sum_k A[k, m]
 * Both operands are row-contiguous in the contraction index (dz [rows, out], x [rows, in]).  The launch is a stream-K
 * decomposition: the k-tiles of all output tiles of all problems form one line that the resident workgroups (one per CU)
 * cut into equal contiguous ranges, so every CU multiplies for the same time whatever the shapes; a tile that ends up in
 * several ranges goes through fp32 partial slabs in `workspace` and the reduce launch sums them in ascending k order
 * (bit-identical from run to run).  Constraints: M, N, lda, ldb multiples of 4; pointers 16-byte aligned; every operand
 * below 4 GiB; M <= 256 * 255.
 * ---------------------------------------------------------------------- */
#define SDUMC_GG_MAX_PROBLEMS 40   /* per launch pair; longer lists are cut into several */
typedef struct sdumc_gg_problem {
  const float* A[2];        /* [K_s, M] with lda: the gradient w.r.t. the layer's pre-activation (segment 1 unused when K[1] == 0) */
  const float* B[2];        /* [K_s, N] with ldb: the layer's saved input */
  const uint8_t* b_bits[2]; /* optional keep-bits of a dropout fused on B (byte [row * bits_qw + col/4], bit col%4; rows = k) */
  int32_t K[2];             /* rows per segment: two segments = the two streams' text frames, which live in separate tensors */
  int32_t b_row_mod[2];     /* >0: B's source row = k % b_row_mod (the streams share x_audio / x_video) */
  float* C;                 /* [M, N] with ldc */
  float* colsum_a;          /* [M] or NULL: the bias gradient */
  int32_t M, N, lda, ldb, ldc;
  int32_t bits_qw;          /* bytes per row of b_bits */
  float b_scale;            /* 1 / (1 - p) of the fused dropout */
  int32_t accumulate;       /* C += ..., colsum_a += ... */
  /* Optional row maps (fp32 operands with the products on the bf16 matrix pipe, i.e. the default arithmetic; else SDUMC_EINVAL):
   * B[s] is then the packed tensor of a RESIDENT feature store, of any size, and k-row r of segment s is ITS row b_map[s][r] (int32,
   * device) -- the frame projections' weight gradient reads the batch in place.  No b_row_mod with it.  The bf16 form
   * (sdumc_gemm_group_tn_bf16) takes maps too; it fetches entries four at a time: b_map[s] must be readable up to 4 * ceil(K[s] / 4)
   * entries. */
  const int32_t* b_map[2];
} sdumc_gg_problem;
size_t sdumc_gemm_group_workspace_bytes(const sdumc_gg_problem* probs, int32_t n);
int sdumc_gemm_group_tn(const sdumc_gg_problem* probs, int32_t n, void* workspace, size_t workspace_bytes, void* stream);
/* The same on bf16 STORAGE (sdumc_net_dims.bf16 = 2; BASELINE configs[2] / [4]): A and B point to bf16 tensors (lda / ldb in
 * elements; M, N, lda, ldb multiples of 8; b_row_mod 0 or >= 64; no fused dropout -- b_bits must be NULL, the engine materialises
 * the masked frames), products accumulate in fp32 on v_mfma_f32_32x32x16_bf16, C / colsum_a / the slabs are fp32. */
size_t sdumc_gemm_group_bf16_workspace_bytes(const sdumc_gg_problem* probs, int32_t n);
int sdumc_gemm_group_tn_bf16(const sdumc_gg_problem* probs, int32_t n, void* workspace, size_t workspace_bytes, void* stream);
/* fp32 products on the bf16 matrix pipe.  v_mfma_f32_32x32x2_f32 runs at 1/16 of the bf16 MFMA rate; an fp32 value is the exact
 * sum of three bf16 values, so the fp32 GEMM kernels below split both operands in registers (round to nearest, exact residuals)
 * and accumulate the six largest of the nine bf16 x bf16 products -- each exact in fp32 -- with six v_mfma_f32_32x32x16_bf16 per
 * 32 x 32 x 16 block instead of eight fp32 MFMAs.  The three dropped products are below 2^-23 |a b| together, the size of ONE fp32
 * rounding: measured against fp64 the results are as close as the fp32-MFMA kernels' (tools/gg_split_check.py,
 * tools/wide_split_check.py; tests/test_gpu_split.py).  Inputs, outputs and accumulators stay fp32.
 * Measurement / test hook, process-wide: bit 0 the grouped weight-gradient launch (sdumc_gemm_group_tn), bit 1 the wide-tile NT
 * launches of the GEMM entry point (frame / key projections), bit 2 the key projection inside sdumc_umca_fwd, bit 3
 * sdumc_gemm_rows256.
 * Default all (environment SDUMC_SPLIT); 0 = every product on the fp32 MFMAs.
 *
 * CONTRACT AT THE EDGES of the split kernels (tests/test_split_arithmetic.py restates it on the CPU, tests/test_gpu_split.py holds
 * each kernel family to it; x = any operand element, fp32 MFMA = what sdumc_set_split_(0) returns):
 *   - finite x with |x| < 0x1.FEp127 (3.3895e38): as documented above.  -0 behaves as +0 in a product sum (as in fp32).
 *   - NaN operand -> NaN in every output element its row / column feeds (same as the fp32 MFMAs).
 *   - +-Inf operand -> NaN there (the fp32 MFMAs keep +-Inf unless 0 * Inf or Inf - Inf occurs): the first part is Inf, the residual
 *     Inf - Inf is NaN.  A step that meets an infinity is lost either way (NaN loss; Adam then spreads it).
 *   - finite |x| >= 0x1.FEp127 (within half a bf16 ulp of FLT_MAX: 3.3895e38 .. 3.4028e38) rounds to Inf in its first part and is
 *     treated like Inf: NaN.  The fp32 MFMAs overflow for such values as soon as |x * b| >= 2^128.
 *   - tiny values: bf16 has fp32's exponent range but its subnormals stop at 2^-133, and the matrix pipe may flush subnormal
 *     inputs.  |x| >= 2^-102: every non-zero part is a normal bf16 -- exact as above.  Below: a part under 2^-126 may be lost, the
 *     absolute error of such an x is < 2^-125 (of a product: < 2^-125 |b|) -- nothing on this path (features ~N(0,1), weights
 *     ~1e-2, gradients >= 1e-20) comes near it.
 * No clamping is done: the kernels do not spend VALU work on values a training step cannot survive anyway.
 *
 * The switch is an option of the execution context -- sdumc_ctx_set_option(ctx, SDUMC_OPT_SPLIT, mask): the network-level calls made
 * with that context then take it (two contexts can hold different arithmetic, nothing process-wide changes).
 * sdumc_set_split_ sets the PROCESS DEFAULT used by contexts without the option and by the stand-alone kernel entry points (deprecated
 * as a control for network-level calls; kept for kernel-level tests and benches); sdumc_get_split_ returns the mask in force for the
 * calling thread (the default, or the context's inside a network-level call). */
void sdumc_set_split_(int mask);
int sdumc_get_split_(void);

/* ------------------------------------------------------------------------
 * fp32 GEMM on operands split ONCE PER TENSOR into three bf16 planes (csrc/gemm_p3.hip).  Replaces F.linear of
 * frame_dim_reshape_{0,1,2} (model :193-195, :282-284) and of input_proj in FRA2UTT_new / Cross_Attention (model :60, :82) in
 * the fp32 step: same arithmetic as the split kernels above (six bf16 x bf16 part products per fp32 product, fp32 accumulation,
 * same edge contract), but the split is paid where a tensor is PRODUCED -- sdumc_p3_split for the features (once per batch; they
 * do not change across epochs) and the weights (once per step), the epilogue of this GEMM for the projected frames -- instead of
 * per workgroup per k-tile.
 * P3 layout of a row-major X[rows][K], K % 8 == 0: row r = 6 K bytes at r * ld_bytes; chunk c (48 bytes) holds k = 8 c .. 8 c + 7
 * as [plane 0: 8 bf16][plane 1][plane 2]; p0 = bf16(x) (round to nearest even), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1);
 * x == (p0 + p1) + p2 exactly for finite |x| < 0x1.FEp127 (edges: see sdumc_set_split_).  1.5x the bytes of the fp32 tensor.
 * The weight operand of the NT product is stored FRAGMENT-MAJOR (sdumc_p3_split_frag): [N / 32][K / 16][3 planes][64 lanes][16 bytes],
 * lane (li = lane & 31, lh = lane >> 5) of block (rb, kt) holds W[32 rb + li][16 kt + 8 lh .. + 7] -- a wavefront's MFMA operand of a
 * k-tile is three contiguous KiB, loaded straight into registers (the weight never passes through LDS: only the wave that owns the
 * 32 output columns multiplies them).
 *   NT:  C[M, N] = act((A . keep)[M, K] . B[N, K]^T * a_scale + bias),  N % 256 == 0, K % 64 == 0
 * ---------------------------------------------------------------------- */
typedef struct sdumc_gemm_p3 {
  int32_t M, N, K;
  const void* A;            /* P3 [M or a_row_mod rows][K], row stride lda BYTES (>= 6 K, multiple of 16; operand below 4 GiB) */
  const void* B;            /* fragment-major P3 of the weight [N][K] (sdumc_p3_split_frag) */
  int64_t lda, ldb;         /* ldb: bytes between two 32-row blocks of B (>= K / 16 * 3072) */
  int32_t a_row_mod;        /* >0: A's source row = m % a_row_mod (the two streams share x_audio / x_video) */
  const void* A2;           /* optional second A tensor: rows [a2_row0, M) are its rows 0 .. (the two streams' text features live in */
  int32_t a2_row0;          /* separate tensors, their projections in adjacent rows of one C); a multiple of 64; no a_row_mod */
  const uint8_t* a_bits;    /* optional keep-bits of a dropout fused on A: byte [m * bits_qw + k/4], bit k%4 (rows = VIRTUAL rows m) */
  int32_t bits_qw;          /* bytes per row of a_bits (>= K/4, multiple of 4) */
  float a_scale;            /* 1 / (1 - p); read only with a_bits */
  const float* bias;        /* [N] or NULL */
  int32_t act;              /* SDUMC_ACT_* */
  float* C;                 /* fp32 [M][N], row stride ldc floats; may be NULL when C_p3 is given */
  int32_t ldc;
  void* C_p3;               /* optional: the same values as a P3 tensor, row stride ldc_p3 bytes (>= 6 N) */
  int64_t ldc_p3;
  int32_t splitk;           /* 0 auto, 1 none, > 1: K split over workgroups (fp32 slabs in workspace + an ordered reduce) */
  int32_t tile_m;           /* 0 = 64-row tiles on 256-thread workgroups, two per CU (the form the step uses: it shares a CU with other lanes'
                               kernels); 64 / 96 / 128 = that many rows per 512-thread workgroup (one per CU: fastest alone on shapes that fill
                               the chip in one round) */
  float* workspace;         /* >= sdumc_gemm_p3_workspace_bytes */
  size_t workspace_bytes;
  /* Optional row maps: A (and A2) are then the packed P3 tensors of a RESIDENT feature store, of any size, and virtual row m reads
   * A's row a_map[m] (m < a2_row0 or no A2) / A2's row a2_map[m - a2_row0]: the batch is read in place (a padded frame's entry names
   * an all-zero row the store keeps).  Rows are fetched by 64-bit address (global_load_lds), so the 4 GiB operand limit does not
   * apply.  Without a_bits / a_row_mod / tile_m; a2_map if and only if A2.  a_map_rows (optional): rows of the packed tensor(s) (the
   * larger of the two): when a_map_rows * lda stays below 4 GiB the kernel keeps its descriptor addressing (faster than 64-bit
   * addresses); 0 = unknown. */
  const int32_t* a_map;
  const int32_t* a2_map;
  int64_t a_map_rows;
} sdumc_gemm_p3;
size_t sdumc_gemm_p3_workspace_bytes(const sdumc_gemm_p3* g);
int sdumc_gemm_p3_nt(const sdumc_gemm_p3* g, void* stream);
/* fp32 [rows][cols] (row stride ld floats, cols % 8 == 0, 16-byte aligned) <-> P3 (row stride ld_bytes); join(split(x)) == x bit for
 * bit for every finite non-zero x below 0x1.FEp127 in magnitude; -0 comes back as +0 */
int sdumc_p3_split(const float* src, int64_t ld, void* dst, int64_t ld_bytes, int64_t rows, int32_t cols, void* stream);
/* fp32 weight [rows][cols] (rows % 32 == 0, cols % 16 == 0) -> fragment-major P3, 6 rows cols bytes, blocks of 32 rows contiguous */
int sdumc_p3_split_frag(const float* src, int64_t ld, void* dst, int32_t rows, int32_t cols, void* stream);
int sdumc_p3_join(const void* src, int64_t ld_bytes, float* dst, int64_t ld, int64_t rows, int32_t cols, void* stream);

/* ------------------------------------------------------------------------
 * The input-feature gradient of a frame projection (csrc/frame_dx.hip): the backward of F.linear of frame_dim_reshape_{0,1,2}
 * (model :193-195, :282-284) with respect to its INPUT,
 *   C[M, N] = A[M, 256] . W[256, N]     A = dz (gradient w.r.t. the projected frames), W = frame_dim_reshape_m.weight as stored,
 * fp32 in, fp32 out.  Arithmetic: the wide-tile family's (sdumc_set_split_ bit 1, the frame / key projections -- this is their
 * backward): six bf16 x bf16 part products per fp32 product on v_mfma_f32_32x32x16_bf16, fp32 accumulation, the edge contract stated
 * at sdumc_set_split_; with bit 1 off the product takes the fp32-MFMA route (the NN form of the generic GEMM; it reads W, which must
 * then be given).  A-stationary: a workgroup splits a 64-row tile of dz once, keeps its planes in LDS and walks the columns; the
 * weight is read k-major per output column, i.e. as the fragment-major P3 layout of W^T [N][256], which sdumc_p3_split_frag_t writes.
 * C is OVERWRITTEN.  No atomics: a repeated launch gives the same bits.  Nothing is allocated.
 * Row zeroing (optional): with `lengths` (device int32 [M / T]) rows b T + t with t >= lengths[b] are written as exact +0.0f
 * whatever A holds there (they are not multiplied).
 * SDUMC_EINVAL before any launch: null or not 16-byte aligned A / C / W / W_frag / scratch (W and W_frag both NULL), M < 1, N < 256
 * or N % 256, ldw < N, ldc < N (or not multiples of 4), lengths without T >= 1 and M % T == 0.  SDUMC_ENOMEM: W_frag NULL and scratch
 * NULL or below the query. */
typedef struct sdumc_frame_dx {
  int32_t M, N;             /* rows (any >= 1), output columns (a multiple of 256) */
  const float* A;           /* [M][256], row stride 256 */
  const float* W;           /* [256][N], row stride ldw floats; may be NULL when W_frag is given and bit 1 of the split mask is on */
  const void* W_frag;       /* sdumc_p3_split_frag_t of W, or NULL: the call packs W into `scratch` first */
  float* C;                 /* [M][N], row stride ldc floats (64-bit row addressing) */
  int64_t ldw, ldc;
  const int32_t* lengths;   /* optional, device int32 [M / T] */
  int32_t T;
  void* scratch;            /* >= sdumc_frame_dx_scratch_bytes(N), read only when W_frag is NULL */
  size_t scratch_bytes;
} sdumc_frame_dx_t;
size_t sdumc_frame_dx_scratch_bytes(int32_t N);      /* bytes of the packed weight: 6 * 256 * N; 0 for an N the kernel refuses */
int sdumc_frame_dx(const sdumc_frame_dx_t* p, void* stream);
/* fp32 src [K][N] (row stride ld floats; K % 16 == 0, N % 32 == 0, 16-byte aligned) -> the fragment-major P3 layout of its TRANSPOSE
 * [N][K], exactly what sdumc_p3_split_frag would write for src^T: 6 K N bytes into caller-owned memory */
int sdumc_p3_split_frag_t(const float* src, int64_t ld, void* dst, int32_t K, int32_t N, void* stream);

/* ------------------------------------------------------------------------
 * The same NT product for the bf16-STORAGE step (sdumc_net_dims.bf16 = 2; csrc/gemm_b1.hip): A and the weight are bf16, fp32
 * accumulation, C bf16 or fp32.  The weight is stored fragment-major -- [N / 32][K / 16][64 lanes][16 bytes], lane (li, lh) of block
 * (rb, kt) holds W[32 rb + li][16 kt + 8 lh .. + 7] (sdumc_b1_frag_multi writes it from the fp32 parameters, round to nearest even)
 * -- and goes straight into registers; only A passes through LDS.
 *   C[M, N] = act(A[M, K] . B[N, K]^T + bias),  N % 256 == 0, K % 128 == 0
 * ---------------------------------------------------------------------- */
typedef struct sdumc_gemm_b1 {
  int32_t M, N, K;
  const void* A;            /* bf16 [M or a_row_mod rows][K], row stride lda ELEMENTS (>= K, multiple of 8; operand below 4 GiB) */
  const void* B;            /* fragment-major bf16 of the weight [N][K] */
  int64_t lda, ldb;         /* ldb: BYTES between two 32-row blocks of B (>= K / 16 * 1024) */
  int32_t a_row_mod;        /* >0: A's source row = m % a_row_mod */
  const void* A2;           /* optional second A tensor holding rows [a2_row0, M) (a2_row0 % 64 == 0; no a_row_mod) */
  int32_t a2_row0;
  const float* bias;        /* [N] fp32 or NULL */
  int32_t act;              /* SDUMC_ACT_* */
  void* C;                  /* [M][N], row stride ldc elements (multiple of 8) */
  int32_t ldc;
  int32_t c_bf16;           /* 1: C is bf16 (round to nearest even), 0: fp32 */
  int32_t splitk;           /* 0 auto, 1 none, > 1: K split over workgroups (fp32 slabs in workspace + an ordered reduce) */
  float* workspace;         /* >= sdumc_gemm_b1_workspace_bytes */
  size_t workspace_bytes;
  /* Optional row maps, as in sdumc_gemm_p3: A (and A2) are the packed bf16 tensors of a resident feature store and virtual row m reads
   * row a_map[m] (a2_map[m - a2_row0]); a_map_rows = rows of the packed tensor(s), 0 = unknown (64-bit addressing). */
  const int32_t* a_map;
  const int32_t* a2_map;
  int64_t a_map_rows;
} sdumc_gemm_b1;
size_t sdumc_gemm_b1_workspace_bytes(const sdumc_gemm_b1* g);
int sdumc_gemm_b1_nt(const sdumc_gemm_b1* g, void* stream);
/* n <= 12 fp32 weights [rows_i][cols_i] at P + src_off[i] floats (contiguous rows; rows % 32 == 0, cols % 16 == 0) -> fragment-major
 * bf16 at dst + dst_off[i] bytes (2 rows cols bytes each), one launch */
int sdumc_b1_frag_multi(const float* P, void* dst, const int64_t* src_off, const int64_t* dst_off, const int32_t* rows,
                        const int32_t* cols, int n, void* stream);

/* ------------------------------------------------------------------------
 * The tall 256 x 256 products of the frame-level part in one persistent launch (gemm_rows.hip):
 *   C[M x 256] = act((A . keep) B * a_scale + bias) (+ C),   K = N = 256
 * - the key projections  keys = tanh(drop(x) W^T + b)  of FRA2UTT_new / Cross_Attention (model :60, :82; main :144 in train
 *   mode): A = the projected frames, a_bits = the keep-bits of the fused input dropout, B = W^T (a [in][out] copy);
 * - their input gradients dxd += dz W (autograd, main :149): A = dz, B = the weight as stored ([out][in]), accumulate = 1.
 * A is [M][256] row-major with row stride lda (floats, 16-byte aligned rows); row r reads source row r % a_row_mod when
 * a_row_mod > 0 (the two streams share the audio / video frames).  B is [256 k][256 n] with row stride ldb.  a_bits (NULL = no
 * dropout) holds one byte per 4 columns and row of A's VIRTUAL rows ([M][64], low nibble, as sdumc_dropout_bits writes it).
 * Every problem of one call takes the same kernel variant: all masked, all accumulating, or neither (else SDUMC_EINVAL).
 * ------------------------------------------------------------------------ */
#define SDUMC_ROWS_MAX_PROBLEMS 8
typedef struct sdumc_rows_problem {
  const float* A;
  const float* B;
  const uint8_t* a_bits;
  const float* bias;        /* [256] or NULL */
  float* C;                 /* [M][256], row stride ldc */
  int32_t M, lda, ldb, ldc;
  int32_t a_row_mod;
  float a_scale;            /* 1 / (1 - p); read only with a_bits */
  int32_t accumulate;
  int32_t act;              /* SDUMC_ACT_NONE or SDUMC_ACT_TANH */
  /* optional rank-nq term of the attention pooling's own input gradient, folded into the product as one more k-tile:
   *   C[r] = A[r] B + sum_i pool_w[r][i] * pool_g[r / pool_T][i][:]
   * pool_w = the attention weights [M][pool_nq] of the site, pool_g = dout * out-dropout mask [M / pool_T][pool_nq][256]
   * (sdumc_attnpool_bwd.dout_masked).  dxd = dz W + (pooling part) then leaves this kernel in ONE pass: the pooling backward
   * does not write dxd and this launch does not read it back.  Needs pool_nq <= 8 (<= 7 with fold), pool_T >= 63 or pool_T == 32 (a
   * 64-row tile spans at most two samples), no a_bits, no bias / act / a_row_mod, M % pool_T == 0; accumulate only together with fold. */
  const float* pool_w;
  const float* pool_g;
  int32_t pool_nq, pool_T;
  /* optional, with the pooling term (fp32: split arithmetic only; sdumc_gemm_rows256_bf16 takes it too -- pool_w / pool_g stay fp32,
   * every problem of a launch the same fold): the mask-sum of the frame-level input dropouts folded in as well --
   *   C[r] (+)= sum_{s < fold} keep_s[r] . (A[s R + r] B + pooling term of row s R + r) * c_scale,   R = M / fold rows of C
   * i.e. dx of a modality = the sum over the streams that share its frames (fold = 2; 1 for separate frames) of the masked dxd of one
   * attention site, written ONCE: dxd never exists in memory.  c_bits = the keep-bits of the site's input dropout over the M virtual
   * rows ([M][64], as a_bits; NULL = keep everything, c_scale unused); accumulate = 1 adds onto C (the second site of the modality).
   * fold = 0: off.  R % pool_T == 0. */
  const uint8_t* c_bits;
  float c_scale;
  int32_t fold;
} sdumc_rows_problem;
int sdumc_gemm_rows256(const sdumc_rows_problem* probs, int32_t n, void* stream);
/* The same on bf16 STORAGE (sdumc_net_dims.bf16 = 2): A ([M][256]), B and C are bf16 tensors (lda / ldb / ldc in elements, lda
 * and ldb multiples of 8, A and B 16-byte aligned); B is [256 n][256 k] -- the rows of B are the OUTPUT columns, C = A B^T: the
 * bf16 weight copy as stored for the key projections, its transposed copy for dxd += dz W; bias fp32; a_bits must be NULL (the
 * engine materialises the masked frames); products accumulate in fp32 on v_mfma_f32_32x32x16_bf16. */
int sdumc_gemm_rows256_bf16(const sdumc_rows_problem* probs, int32_t n, void* stream);

/* ------------------------------------------------------------------------
 * Attention pooling over the time axis = the body shared by
 *   FRA2UTT_new.forward     (model :56-68; nq = 1, query = attention_context_vector, q_stride 0)
 *   Cross_Attention.forward (model :79-95; nq = 7, query = query_proj(multi_query))
 * after the key projection K = tanh(drop(x).W^T + b) has been produced by
 * sdumc_gemm_f32 (NT, a_drop, act tanh).
 *   S[v,t,i] = K[v,t,:].Q[v,i,:] ; A = softmax_t(0.3 S) ; O[v,i,:] = sum_t A[v,t,i] drop(x)[v,t,:]
 *   out = drop_out(O)
 * v = virtual sample = stream*B + b; x row of v is (v % x_samples).
 * ---------------------------------------------------------------------- */
typedef struct sdumc_attnpool {
  int32_t V;           /* virtual samples (streams * B) */
  int32_t T;           /* frames */
  int32_t nq;          /* 1..8 */
  int32_t x_samples;   /* x holds this many samples; x row of v = v % x_samples */
  const float* x;      /* [x_samples, T, 256] */
  const float* keys;   /* [V, T, 256] tanh keys */
  const float* q;      /* [V or 1, nq, 256] projected queries */
  int64_t q_stride;    /* floats between the queries of consecutive v (0 = shared) */
  float scale;         /* 0.3 */
  sdumc_dropout x_drop;   /* the input dropout (same descriptor the key GEMM used) */
  sdumc_dropout out_drop; /* the output dropout, rows = nq */
  float* attn;         /* [V, T, nq]  softmax weights (returned by the reference, saved for backward) */
  float* pooled;       /* [V, nq, 256] O before the output dropout (saved for backward) */
  float* out;          /* [V, nq, 256] */
  float* workspace;    /* >= sdumc_attnpool_fwd_workspace_bytes(V, T, nq): per-chunk softmax partials */
  size_t workspace_bytes;
  int32_t dim;         /* channels per row: 0 or 256 (the model's general_dim, model :191), or 512 / 768 / 1024 for the
                          blocks used on their own (FRA2UTT_new / Cross_Attention default to input_dim = 1024,
                          model :47,:71).  Every "256" in the shapes above and below then reads `dim`; the dropout
                          descriptors carry width = dim; workspaces are sized by the *_dim queries */
  const int32_t* lengths; /* EXTENSION (default NULL = the reference's behaviour, where zero-padded frames take
                          part in the softmax, read_data.py:139-151 / model :63,:90): device int32 [V], valid frames per
                          virtual sample; frames t >= max(1, lengths[v]) get weight exactly 0 (key-padding mask) and
                          therefore zero gradient in sdumc_attnpool_bwd, which needs no mask of its own; a sample with ONE valid
                          frame gets exactly zero dz and dq there, as a sample run on its own with T = 1 does */
  int32_t bf16;        /* 1: x and keys (and, in sdumc_attnpool_bwd, dz and dxd) are bf16 tensors of the same shapes (the engine's
                          bf16-storage mode, BASELINE configs[2] / [4]); scores, softmax, pooling, attn, pooled, out, dq stay
                          fp32.  dim must be 256; a fused x_drop needs precomputed keep-bits.  0 (default): fp32 */
  uint32_t* tickets;   /* NULL, or 2 * V device counters that are ZERO when the call starts (and again when it ends): the
                          per-sample second passes then run inside the first kernels -- the last 64-frame chunk of a sample to
                          finish combines that sample's softmax partials (forward, counters [0, V)) / sums its dq slabs
                          (backward, counters [V, 2V)) -- instead of in a second launch.  Same arithmetic in the same order.
                          (The engine leaves this NULL: at the MOSEI shapes the second launch measured cheaper, see engine.hip.) */
  int32_t partial_only; /* forward: 1 = stop after the per-chunk pass: `workspace` then holds the flash-style partials -- unnormalised
                          pooled rows [V][nchunk][nq][dim], then {chunk max, chunk sum} [V][nchunk][2][8] -- and `attn` the unnormalised
                          weights; out / pooled are NOT written.  The caller finishes the softmax itself (the engine's clustered
                          utterance-level stages do: csrc/chain_cluster.hip).  Requires tickets == NULL.
                          sdumc_attnpool_bwd_multi with f.partial_only = 1: the per-chunk dq slabs [V][nchunk][nq][256] stay in
                          `workspace` and dq is NOT written (the caller sums the chunks). */
} sdumc_attnpool;

size_t sdumc_attnpool_fwd_workspace_bytes(int32_t V, int32_t T, int32_t nq);
size_t sdumc_attnpool_fwd_workspace_bytes_dim(int32_t V, int32_t T, int32_t nq, int32_t dim);
size_t sdumc_attnpool_bwd_workspace_bytes_dim(int32_t V, int32_t T, int32_t nq, int32_t dim);
int sdumc_attnpool_fwd(const sdumc_attnpool* p, void* stream);

/* backward of the above. Produces
 *   dz    [V,T,256]  gradient w.r.t. the pre-tanh key projection (feeds the dW / dX GEMMs)
 *   dxd   [V,T,256]  gradient w.r.t. drop(x) through the pooling ("V") path; the key-projection
 *                    path is ADDED to it by the caller's NN GEMM (accumulate=1)
 *   dq    [V,nq,256] gradient w.r.t. the projected queries (nq=1 shared query: per-v partials,
 *                    reduce over v with sdumc_colsum)
 */
typedef struct sdumc_attnpool_bwd {
  sdumc_attnpool f;      /* the forward descriptor (x, keys, q, attn, pooled, dropouts) */
  const float* dout;     /* [V, nq, 256] gradient w.r.t. out */
  float* dz;
  float* dxd;
  float* dq;
  float* workspace;      /* >= sdumc_attnpool_bwd_workspace_bytes(V, T, nq): per-chunk dq slabs */
  size_t workspace_bytes;
  float* dq_sum;         /* optional [nq, dim]: SHARED query (f.q_stride == 0, FRA2UTT_new's context vector, model :50-52): the
                            sum over v of the per-sample gradients, written by ONE launch that reduces the per-chunk slabs of
                            every sample in a fixed order; dq is then NOT written.  NULL = per-sample dq as above.  Single-site
                            sdumc_attnpool_bwd only (the _multi form requires NULL). */
  float* dout_masked;    /* optional [V, nq, 256]: dout * out-dropout mask as the kernel uses it -- for a consumer that adds the pooling
                            part of dxd itself (sdumc_rows_problem.pool_g); dxd may then be NULL and is not written */
} sdumc_attnpool_bwd_t;

size_t sdumc_attnpool_bwd_workspace_bytes(int32_t V, int32_t T, int32_t nq);
int sdumc_attnpool_bwd(const sdumc_attnpool_bwd_t* p, void* stream);
/* K3, the fused UMCA forward (Cross_Attention model :79-95, FRA2UTT_new :56-68 = the nq = 1 case): key
 * projection + scores + softmax partials + pooling of one 64-frame chunk in ONE kernel -- K = tanh(drop(x) W_in^T + b) is
 * computed on the matrix cores into an LDS tile and consumed there; it goes to HBM only if a.keys != NULL (training keeps the
 * keys for sdumc_attnpool_bwd; inference passes NULL and the [V, T, 256] tensor never exists).  Takes the place of
 * the NT key-projection GEMM (fused input dropout, bias, tanh) followed by sdumc_attnpool_fwd on the same descriptor; same results.
 * fp32, 256 channels, input mask as keep-bits (x_drop.bits) or none, a.tickets NULL. */
typedef struct sdumc_umca {
  sdumc_attnpool a;      /* as for sdumc_attnpool_fwd; a.keys = OUTPUT [V, T, 256] or NULL */
  const float* w_in;     /* input_proj.weight [256, 256] as stored (model :60 / :82) */
  const float* b_in;     /* input_proj.bias [256] */
  /* optional, both or neither: the projection's operands split once per tensor (sdumc_gemm_p3): the frames a.x as a P3 tensor
   * ([x_samples * T][256], rows of 1536 bytes) and w_in fragment-major (sdumc_p3_split_frag).  a.x (fp32) is still read by the
   * pooling part.  Needs the split arithmetic on (sdumc_set_split_ bit 2), else SDUMC_EINVAL. */
  const void* x_p3;
  const void* w_in_p3f;
} sdumc_umca;
int sdumc_umca_fwd(const sdumc_umca* p, void* stream);

/* Up to four pooling sites in ONE launch pair (forward: partial + combine; backward: rows + dq reduce) -- what the step uses for
 * its three Cross_Attention blocks, which are independent and too short to be worth a stream fork.  Every site: 256-channel
 * rows, keep-bits attached or no input mask, the same `bf16` flag, its OWN workspace.  Results are bit-identical to n single
 * calls.  Replaces the three Cross_Attention.forward calls of models/wengnet_mosei_multviews_text_missing.py:334-336. */
int sdumc_attnpool_fwd_multi(const sdumc_attnpool* sites, int32_t n, void* stream);
int sdumc_attnpool_bwd_multi(const sdumc_attnpool_bwd_t* sites, int32_t n, void* stream);
/* Measurement / test hook: 0 routes the 256-channel, keep-bits, two-pass-combine cases back to the round-3 pooling kernels
 * (the round-4 "v2" kernels -- every global load issued up front, XCD-aware stream pairing -- are the default; results are
 * bit-identical: tests/test_gpu_ops.py).  Process-wide. */
int sdumc_attnpool_set_v2_(int on);

/* ------------------------------------------------------------------------
 * Small fused element-wise / reduction kernels of the utterance-level network.
 * ---------------------------------------------------------------------- */

/* dz = dy * [y > 0] * scale  (backward of Linear->ReLU->Dropout given the saved
 * post-dropout output y, model :264-273);  in place allowed.  n elements. */
int sdumc_relu_drop_bwd(const float* dy, const float* y, float scale, float* dz, int64_t n, void* stream);

/* out[j] (+)= sum_r a[r, j], a is [rows, cols] with leading dimension lda (bias gradients).
 * Deterministic two-stage reduction; workspace >= sdumc_colsum_workspace_bytes. */
size_t sdumc_colsum_workspace_bytes(int64_t rows, int32_t cols);
int sdumc_colsum(const float* a, int64_t rows, int32_t cols, int32_t lda, float* out, int32_t accumulate,
                 float* workspace, void* stream);

/* y[i] = sum_k x_k[i] (k <= 8 inputs), or out = a + b*c style helpers */
int sdumc_add_n(const float* const* xs, int32_t k, float* y, int64_t n, void* stream);

/* dx[b,t,:] = sum over `k` (site,stream) terms of g_k[v,t,:] * mask_k   (model backward of the
 * four dropout applications that read one projected feature tensor x) */
typedef struct sdumc_dropsum {
  int32_t terms;                 /* <= 8 */
  const float* g[8];             /* each [samples, T, 256] (already offset to the stream) */
  sdumc_dropout drop[8];         /* per-term dropout; stream offset given through call0/dev_state + stream_idx */
  int32_t stream_idx[8];
  int32_t samples, T;
  float* dx;                     /* [samples, T, 256] */
  int32_t bf16;                  /* 1: g[k] and dx are bf16 tensors (the engine's bf16-storage mode); 0: fp32 */
} sdumc_dropsum;
int sdumc_dropsum_bwd(const sdumc_dropsum* p, void* stream);

/* bf16-storage mode: out[row, :] = bf16(x[row % x_rows, :] * keep * scale) -- the masked frames drop(x) of one attention site
 * (nn.Dropout inside FRA2UTT_new / Cross_Attention, model :59, :81) materialised once, from keep-bits produced by
 * sdumc_dropout_bits (byte [row * width/4 + q], bit e = keep column 4q + e).  x, out: bf16 [.., width], width % 8 == 0. */
int sdumc_mask_apply_bf16(const void* x, const uint8_t* bits, void* out, int64_t rows, int64_t x_rows, int32_t width, float scale,
                          void* stream);

/* Modality fusion (model :301-332 algebra).  u [V,3,256], alpha [V,3]
 *   qin [7][V,256] = (f, f_at, f_tv, f_av, u_a, u_t, u_v)                         */
int sdumc_fusion_fwd(const float* u, const float* alpha, float* qin, int32_t V, void* stream);
/* dqin [7][V,256] -> du [V,3,256] (overwritten), dalpha [V,3] (ACCUMULATED: the second-level
 * fusion's contribution is already there, it runs earlier in the backward order) */
int sdumc_fusion_bwd(const float* u, const float* alpha, const float* dqin, float* du, float* dalpha,
                     int32_t V, void* stream);

/* Second-level fusion (model :346-358).  c [3][V,7,128] (modality-major), alpha [V,3] -> h [V,7,128] */
int sdumc_hweight_fwd(const float* c, const float* alpha, float* h, int32_t V, void* stream);
/* dh [V,7,128] -> dc [3][V,7,128] = alpha_m dh (+ dct [V,7,128] on m = 1, the external gradient of
 * cross_hiddens[:,1]; may be NULL), dalpha [V,3] (overwritten) */
int sdumc_hweight_bwd(const float* c, const float* alpha, const float* dh, const float* dct, float* dc,
                      float* dalpha, int32_t V, float relu_scale, void* stream);
/* relu_scale > 0: dc is additionally multiplied by [c > 0] * relu_scale (c is the post-ReLU/dropout output of
 * cross_*_mlp, so this is the gradient w.r.t. its pre-activation); 0: plain */
/* z[v,:] = sum_i beta[v,i] h[v,i,:]  (model :356-358) */
int sdumc_zpool_fwd(const float* h, const float* beta, float* z, int32_t V, void* stream);
/* dz [V,128] -> dh [V,7,128] (overwritten), dbeta [V,7] (overwritten) */
int sdumc_zpool_bwd(const float* h, const float* beta, const float* dz, float* dh, float* dbeta,
                    int32_t V, void* stream);

/* ------------------------------------------------------------------------
 * Losses (toolkit/utils/loss.py) — value and gradient in one call.
 * ---------------------------------------------------------------------- */

/* MSELoss (loss.py:19-33): loss = sum((pred-target)^2)/denom; dpred = w*2*(pred-target)/denom.
 * denom = len(pred) of the GLOBAL batch (= rows on one GPU).  loss_out (device scalar) is WRITTEN
 * with the unweighted local sum / denom. */
int sdumc_mse_fwd_bwd(const float* pred, const float* target, int32_t rows, float denom, float weight,
                      float* loss_out, float* dpred, void* stream);

/* The regression criteria beside MSELoss, value and gradient in one launch of one workgroup (fixed summation order, bitwise
 * reproducible).  d_i = pred_i - target_i in fp32, inv = fp32(1 / denom), denom as for sdumc_mse_fwd_bwd:
 *   SDUMC_REGRESS_MSE    sdumc_mse_fwd_bwd's launch, bit for bit
 *   SDUMC_REGRESS_L1     torch.nn.L1Loss under MSELoss's reduction: sum |d_i| / denom; dpred_i = (weight * sign(d_i)) * inv,
 *                        sign(0) = 0, a NaN d_i gives NaN
 *   SDUMC_REGRESS_HUBER  torch.nn.HuberLoss(delta) likewise: h_i = 0.5 d_i^2 where |d_i| <= delta, delta (|d_i| - 0.5 delta)
 *                        elsewhere; dpred_i = (weight * g_i) * inv, g_i = d_i or delta * sign(d_i)
 *   SDUMC_REGRESS_CCC    1 - concordance correlation coefficient = 1 - 2 s_py / (s_pp + s_yy + (m_p - m_y)^2), population
 *                        moments over the `rows` elements (denom is not read), accumulated in double in two passes; dpred_i =
 *                        weight * fp32(dLoss/dpred_i in double).  pred and target one shared constant: 0/0 = NaN, value and
 *                        gradient; rows = 1: value 1, gradient +0.
 * loss_out (device scalar) is WRITTEN with the unweighted value (L1 / Huber: the local sum / denom); dpred ([rows], overwritten)
 * may be NULL.  SDUMC_EINVAL before a launch: a NULL pred / target / loss_out, rows < 1, denom <= 0, an unknown code, delta not
 * positive and finite under HUBER (delta is read by HUBER alone). */
#define SDUMC_REGRESS_MSE 0
#define SDUMC_REGRESS_L1 1
#define SDUMC_REGRESS_HUBER 2
#define SDUMC_REGRESS_CCC 3
int sdumc_reg_fwd_bwd(const float* pred, const float* target, int32_t rows, float denom, float weight, int32_t regress,
                      float delta, float* loss_out, float* dpred, void* stream);

/* Sum of squared differences, for RMSELoss (loss.py:37-51) = sqrt(ssd / numel).
 * Splitting ssd from the sqrt lets data-parallel ranks all-reduce ssd first. */
int sdumc_ssd(const float* a, const float* b, int64_t n, float* ssd_out, float* workspace, void* stream);
size_t sdumc_ssd_workspace_bytes(int64_t n);
/* da (+)= w*(a-b)/(rmse*numel_global), db (+)= -that ; rmse = sqrt(*ssd_global/numel_global)
 * loss_out written with rmse.  da / db may be NULL (detached side, main :148). */
int sdumc_rmse_bwd(const float* a, const float* b, int64_t n_local, const float* ssd_global, double numel_global,
                   float weight, float* loss_out, float* da, int32_t da_accumulate, float* db,
                   int32_t db_accumulate, void* stream);

/* RnCLoss (loss.py:271-315). feats [n,dim] = cat(r_stream0, r_stream1), labels [n] (already
 * repeated).  Computes the loss over ALL n rows and the gradient for rows
 * [row0, row0+rows_local) only (data-parallel: every rank holds the gathered feats).
 * loss_out written with the unweighted loss; dfeats [rows_local, dim] overwritten with
 * weight * dLoss/dfeats. */
size_t sdumc_rnc_workspace_bytes(int32_t n);
int sdumc_rnc_fwd_bwd(const float* feats, const float* labels, int32_t n, int32_t dim, float temperature,
                      float weight, int32_t row0, int32_t rows_local, float* loss_out, float* dfeats,
                      float* workspace, void* stream);
/* the same with the labels given once ([n/2]) and read as labels[j % (n/2)] (loss.py:283 labels.repeat(2, 1)) */
int sdumc_rnc_fwd_bwd_rep(const float* feats, const float* labels_half, int32_t n, int32_t dim, float temperature,
                          float weight, int32_t row0, int32_t rows_local, float* loss_out, float* dfeats,
                          float* workspace, void* stream);
/* SupConLoss (loss.py:143-240; forward :153-240): supervised contrastive loss over class labels, SimCLR without them.
 * feats [N, dim], N = bsz * n_views rows VIEW-MAJOR (row v * bsz + b = view v of sample b: the reference's
 * cat(unbind(features, 1)) of :191).  Anchors: all N rows (contrast_all = 1, contrast_mode 'all') or the first bsz
 * (0, 'one').  Logits = dot / temperature minus the row maximum over every column; the self column is left out of the
 * denominator and of the positives; an anchor with fewer than 1e-6 positives divides by 1; the value is
 * -(temperature / base_temperature) * the mean over the anchors.
 * Positives: labels == NULL and mask == NULL: same sample (:180-181); labels [bsz] floats: label_mode 0 = equal labels
 * (torch.eq, :186), 1 = equal rintf(label) (the seven classes of a MOSEI sentiment score); mask [bsz, bsz] floats: the
 * weight of sample j among the positives of sample i (may be asymmetric; tiled as :210).  Both given: SDUMC_EINVAL.
 * normalize = 1: every row is first divided by max(|row|, 1e-12) (F.normalize(x, dim=-1)); dfeats is still the gradient
 * w.r.t. the rows AS GIVEN (the projection is applied here, no normalised copy is written).  On un-normalised 64-wide
 * rows with temperature 0.07 the reference itself returns NaN (every off-diagonal exp underflows: 0 * log 0), and so
 * does this entry.
 * loss_out (device scalar) is WRITTEN with the unweighted value; dfeats [N, dim] (may be NULL) is overwritten with
 * weight * dLoss/dfeats.  fp32 in and out, fp64 between; two launches, fixed summation order, no atomics.
 * Built limits: 2 <= N <= 2048, 1 <= dim <= 1024 (any dim, any N in the range); beyond them, and for n_views < 1,
 * temperature <= 0, base_temperature <= 0, a mode outside 0/1 or a NULL / not 8-byte aligned workspace:
 * SDUMC_EINVAL before anything is launched.  workspace >= sdumc_supcon_workspace_bytes(bsz, n_views, contrast_all). */
size_t sdumc_supcon_workspace_bytes(int32_t bsz, int32_t n_views, int32_t contrast_all);
int sdumc_supcon_fwd_bwd(const float* feats, const float* labels, const float* mask, int32_t bsz, int32_t n_views,
                         int32_t dim, int32_t contrast_all, int32_t label_mode, int32_t normalize, double temperature,
                         double base_temperature, float weight, float* loss_out, float* dfeats, void* workspace,
                         void* stream);
/* The five batch-local terms of main :137-148 in two launches: MSELoss(vals_s, labels) for both streams and the
 * three RMSELoss pairs (text_hidden, cross_text, fused; stream 1 vs stream 0, teacher side detached for the
 * first two).  All tensors are the [2B, ...] stream-major network outputs; weights5 = (full_mse, missing_mse,
 * text_feat, text_query_feat, features); denom = B_global; ssd_global = all-reduced sums or NULL (computed
 * here).  Writes losses[1..5] (unweighted) and the four gradient buffers (every element, incl. the zeros). */
size_t sdumc_distill_workspace_bytes(int32_t B);
int sdumc_distill_fwd_bwd(int32_t B, float denom, const float* vals, const float* labels, const float* th,
                          const float* ct, const float* z, const float* weights5, const float* ssd_global,
                          float* d_vals, float* d_th, float* d_ct, float* d_z, float* losses, float* workspace,
                          void* stream);
/* Distillation targets from a STORED teacher instead of stream 0 (main :148 compares the text-missing stream with the full stream of
 * the same step; a trained full-modality checkpoint, or the averaged weights once per epoch, are the other two teachers).  Up to three
 * device fp32 tables in store order; for a pair whose table is given
 *   - the target of sample b is table row idx[b] (idx NULL: row b, the tables are then [B, ...] in batch order); cosine / KL row
 *     (b, q) of cross_text reads teacher row idx[b] * 7 + q;
 *   - the student is stream 1, the first argument, as before;
 *   - the target is a constant: rows [0, B) of that pair's gradient buffer are written +0.0 -- for `fused` too, whose stream 0
 *     self-distillation does NOT detach;
 *   - the value goes to losses[3 + p] as before.
 * A pair whose table is NULL is computed as without a teacher.  Arithmetic, chunking, partials and their order are the self-
 * distillation's: tables that hold bit copies of stream 0's rows give the same bits.  An index outside [0, n_rows) is never turned
 * into an address: the kernels take a NaN target row for it (NaN value; NaN gradient rows of that sample, of the whole pair for RMSE).
 * SDUMC_EINVAL before anything is enqueued: n_rows < 1 with a table given, idx NULL with n_rows != B, a table or idx that is not
 * 4-byte (idx: 8-byte) aligned, a teacher beside ssd_global or a B_global different from B (the data-parallel exchange carries no
 * teacher), B * 896 beyond int32. */
typedef struct sdumc_teacher {
  const float* text_hidden;   /* [n_rows, 256]    or NULL: that pair as the step always had it */
  const float* cross_text;    /* [n_rows, 7, 128] or NULL */
  const float* fused;         /* [n_rows, 128]    or NULL */
  const int64_t* idx;         /* device [B] rows of the tables, or NULL: row b */
  int64_t n_rows;
} sdumc_teacher;
/* sdumc_distill_fwd_bwd with the criterion of the three pairs (SDUMC_DISTILL_*) and a teacher.  teacher NULL, or all three of its
 * tables NULL: the same launches as without one. */
int sdumc_distill_teacher_fwd_bwd(int32_t B, float denom, const float* vals, const float* labels, const float* th,
                                  const float* ct, const float* z, const float* weights5, const float* ssd_global,
                                  float* d_vals, float* d_th, float* d_ct, float* d_z, float* losses, float* workspace,
                                  int32_t distill, const sdumc_teacher* teacher, void* stream);
/* Row-wise criteria for the drop-in loss modules: value and gradient in ONE launch, one wavefront per row, fixed
 * summation order (rows in index order per wavefront, wavefronts in index order: bitwise reproducible).
 * a, b: [rows, groups, width] contiguous (groups = 1 for 2-D inputs), width <= 1024; denom = size(0) of the GLOBAL
 * batch; loss_out (device scalar) is WRITTEN with the unweighted value; da / db ([rows, groups, width], overwritten
 * with weight * dLoss/da, weight * dLoss/db) may be NULL.  Identical inputs give value 0 and gradient 0.
 *
 * CosineSimilarityLoss4Seq (loss.py:100-119): sum over the groups of the mean over rows of 1 - cos(a_row, b_row)
 *   = sum over all rows*groups / denom.  cos as torch.cosine_similarity: every norm is clamped from below to
 *   eps = 1e-8 on its own, a clamped norm passes no gradient (all-zero rows: cos = 0, gradient = other / (eps * norm)). */
int sdumc_cosine_fwd_bwd(const float* a, const float* b, int32_t rows, int32_t groups, int32_t width, float denom,
                         float weight, float* loss_out, float* da, float* db, void* stream);
/* KLLoss (loss.py:74-97): (KL(softmax b || softmax a) + KL(softmax a || softmax b)) / 2, softmax over the last axis,
 * reduction 'batchmean' = sum over everything / denom.  Log-softmax with the row maximum subtracted, fp32. */
int sdumc_kl_fwd_bwd(const float* a, const float* b, int32_t rows, int32_t groups, int32_t width, float denom,
                     float weight, float* loss_out, float* da, float* db, void* stream);
/* CELoss (loss.py:6-16): log_softmax(a, 1) + NLLLoss(reduction='sum') / denom.  a [rows, width] logits, b [rows] the
 * class indices held as floats (truncated like target.long(); an index outside [0, width) makes the value NaN).
 * groups must be 1 and db NULL (else SDUMC_EINVAL): the targets take no gradient. */
int sdumc_ce_fwd_bwd(const float* a, const float* b, int32_t rows, int32_t groups, int32_t width, float denom,
                     float weight, float* loss_out, float* da, float* db, void* stream);
/* gradient rows [row0, row0+rows) from the workspace a previous sdumc_rnc_fwd_bwd call filled
 * (a data-parallel rank owns two row ranges of the gathered matrix: its stream-0 and stream-1 rows) */
int sdumc_rnc_dfeat_rows(const float* feats, int32_t n, int32_t dim, float temperature, float weight, int32_t row0,
                         int32_t rows, float* dfeats, float* workspace, void* stream);
/* the boolean neg_mask of loss.py:303 for anchor i, exported for the bit-exactness test:
 * mask [n, n-1, n-1] uint8, diagonal removed as loss.py:294-296 does */
int sdumc_rnc_mask(const float* labels, int32_t n, uint8_t* mask, void* stream);

/* ------------------------------------------------------------------------
 * Optimiser: torch.optim.Adam(lr, betas, eps, weight_decay) with coupled L2
 * (main :317) over one flat parameter bucket.  hyper (device, 4 floats) =
 * {lr (host-written), step count t (incremented by the call), lr/(1-beta1^t), sqrt(1-beta2^t)}:
 * kept on the device so that a captured graph replays with the right step count.
 * grad_scale multiplies the gradient first (1/world_size after a sum all-reduce).
 * ---------------------------------------------------------------------- */
int sdumc_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                    float* hyper, float beta1, float beta2, float eps, float weight_decay,
                    float grad_scale, void* stream);

/* The same update over PER-PARAMETER tensors in one launch: what torch.optim.Adam(model.parameters(), ...).step() of
 * main :317 does when the gradients are the separate tensors autograd left in p.grad (sdumc_amd/optim.py).
 * Segment i updates param[0 .. n) from grad[0 .. n) with the moments exp_avg / exp_avg_sq [state_offset .. state_offset + n)
 * of two flat buffers of state_len floats.  param and grad need only their natural 4-byte alignment (views at any element
 * offset of a larger tensor): a segment whose four addresses are all 16-byte aligned moves 16 bytes per lane, any other one
 * float per lane; same arithmetic, bit for bit, either way and as the single-bucket entry above.  Segments must not overlap.
 * hyper advances ONCE per call, as above.  The segments travel to the device BY VALUE in the kernel arguments (no copy, no
 * synchronisation, no allocation): SDUMC_ADAM_MAX_SEGS per launch, a longer list takes further launches of the same kernel.
 * SDUMC_EINVAL (before anything is launched): null pointers, nseg <= 0, a segment with n <= 0 or state_offset < 0 or
 * state_offset + n > state_len. */
#define SDUMC_ADAM_MAX_SEGS 96     /* sizeof(sdumc_adam_table) + the other arguments stay below HIP's 4 KB of kernel arguments */
#define SDUMC_ADAM_CHUNK 1024      /* elements per 256-thread workgroup */
typedef struct sdumc_adam_seg {
  float* param;
  const float* grad;
  int64_t state_offset;    /* floats into exp_avg / exp_avg_sq */
  int64_t n;               /* elements */
} sdumc_adam_seg;
/* one launch's kernel argument: its segments and the running count of workgroups behind each of them (workgroup b works on
 * the segment s with block_end[s - 1] <= b < block_end[s], chunk b - block_end[s - 1]); filled by the call */
typedef struct sdumc_adam_table {
  sdumc_adam_seg seg[SDUMC_ADAM_MAX_SEGS];
  uint32_t block_end[SDUMC_ADAM_MAX_SEGS];
  int32_t nseg;
  int32_t reserved;
} sdumc_adam_table;
int sdumc_adam_multi(const sdumc_adam_seg* segs, int32_t nseg, float* exp_avg, float* exp_avg_sq, int64_t state_len,
                     float* hyper, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                     void* stream);

/* Per-tensor learning rates, decay and frozen tensors over the ONE flat bucket: torch.optim.Adam with one parameter group per tensor
 * and one shared step count.  A segment names elements [offset, offset + n) of param / grad / exp_avg / exp_avg_sq; its elements
 * are updated with step size hyper[2] * lr_scale and coupled L2 weight_decay * wd_scale (two fp32 products; everything else is the
 * expression of sdumc_adam_step, so a table of ones gives that call's bits).  lr_scale == 0 is torch's lr = 0 group: the parameter
 * stays, the moments advance.  frozen != 0 is requires_grad = False: parameter and both moments are neither read nor written, the
 * gradient is not read (the scales of a frozen segment are checked like any and then not used).  Elements of the bucket that
 * belong to no segment (alignment padding) get the update of sdumc_adam_step.  Segments need only their natural 4-byte alignment:
 * any offset, any length >= 1. */
#define SDUMC_RATES_MAX_SEGS 96    /* the table travels in the kernel arguments, like sdumc_adam_table */
typedef struct sdumc_rate_seg {
  int64_t offset, n;       /* elements [offset, offset + n) of the bucket */
  float lr_scale, wd_scale;
  int32_t frozen;
} sdumc_rate_seg;
/* sdumc_adam_step with the table (HOST memory, read during the call): hyper advances once, then ONE launch over the bucket.
 * SDUMC_EINVAL before anything is launched: what sdumc_adam_step refuses (null pointers, n <= 0, a buffer that is not 16-byte
 * aligned), segs NULL, nseg outside 1 .. SDUMC_RATES_MAX_SEGS, a segment with n < 1 or outside [0, n), segments that are not
 * ascending or that overlap, a scale that is negative, NaN or Inf. */
int sdumc_adam_step_rates(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* hyper, float beta1,
                          float beta2, float eps, float weight_decay, float grad_scale, const sdumc_rate_seg* segs, int32_t nseg,
                          void* stream);
/* Writes +0.0f over the segments of buf[0 .. n) with frozen != 0 and nothing else (one launch; none when no segment is frozen):
 * what a frozen tensor's gradient reads as to everyone behind the backward.  buf 16-byte aligned; the table as above, refused
 * alike. */
int sdumc_zero_segments(float* buf, int64_t n, const sdumc_rate_seg* segs, int32_t nseg, void* stream);

/* Averaged weights: an exponential moving average (EMA) of the parameters, kept by the launch that updates them.
 * sdumc_adam_step (segs NULL and nseg 0) or sdumc_adam_step_rates (a table) plus the average `ema` [n]: param, both moments and hyper
 * get those calls' bits, and per element, with a = the average and p = the parameter AFTER this step's update (taken from its
 * register, not re-read), torch.lerp(a, p, w)'s own rule in fp32:
 *     w <  0.5:  a' = a + w * (p - a)              w >= 0.5:  a' = p - (p - a) * (1 - w)
 * (the product fused into the sum; with w = 0.25, 0.5 or 1 it is exact and a' is torch.lerp's, bit for bit).
 * w = (float)(1 - d_eff), computed on the device in double and rounded once; d_eff = ema_decay, or with ema_warmup != 0
 * min(ema_decay, (1 + t) / (10 + t)) with t = hyper[1] after this step's increment (the timm / torch-ema warm-up).  ema_decay == 0:
 * the average holds the parameters' bits.  There is no bias correction: start the average as a copy of the parameters.
 * The average follows the parameter on every path: 16-byte groups where the parameter moves in them, the scalar tail (n % 4), the
 * per-element path at segment boundaries.  Wherever the parameter is not written the average is neither read nor written: a step
 * that is held (the clustered kernels' error word is set), frozen segments.  An lr_scale == 0 segment is updated by the rule.  No
 * atomics, one fixed order: the same bits on every run.
 * SDUMC_EINVAL before anything is launched and before the step count advances: what those two calls refuse (segs NULL with
 * nseg != 0 and the reverse included), ema NULL, not 16-byte aligned or overlapping param[0 .. n), ema_decay outside [0, 1] or NaN. */
int sdumc_adam_step_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* hyper, float beta1,
                        float beta2, float eps, float weight_decay, float grad_scale, const sdumc_rate_seg* segs, int32_t nseg,
                        float* ema, float ema_decay, int32_t ema_warmup, void* stream);
/* The same rule over PER-PARAMETER tensors, for the loop that keeps its module (torch.optim.swa_utils.AveragedModel's multi_avg_fn;
 * sdumc_amd/optim.py): segment i is ema[0 .. n) <- lerp(ema, param, weight) with the weight given (1 - decay).  The table travels in
 * the kernel arguments as sdumc_adam_multi's does: SDUMC_ADAM_MAX_SEGS segments per launch, a longer list takes further launches,
 * chunks of SDUMC_ADAM_CHUNK elements per workgroup; a segment whose two addresses are 16-byte aligned moves 16 bytes per lane, any
 * other one float per lane, the same bits either way.  Segments must not overlap.  Nothing synchronises.
 * SDUMC_EINVAL before anything is launched: segs NULL, nseg <= 0, a NULL or misaligned (4 bytes) pointer, n <= 0, weight outside
 * [0, 1] or NaN. */
typedef struct sdumc_ema_seg {
  float* ema;
  const float* param;
  int64_t n;               /* elements */
} sdumc_ema_seg;
int sdumc_ema_multi(const sdumc_ema_seg* segs, int32_t nseg, float weight, void* stream);

/* Decoupled weight decay: torch.optim.AdamW, or torch.optim.Adam(..., decoupled_weight_decay=True).  The decoupled form of
 * sdumc_adam_step (segs NULL and nseg 0, ema NULL), sdumc_adam_step_rates (a table) or sdumc_adam_step_ema (an average, with or
 * without a table): the same launches over the same bytes, and per element, under the launch's hold,
 *     dk = (float)(1 - (lr * lr_scale) * (weight_decay * wd_scale))      on the device, in double, rounded once
 *     p  = p * dk                                                        ONE fp32 multiply, rounded on its own
 *     then the update of sdumc_adam_step on (p, g, m, v) with weight_decay = 0.
 * lr = hyper[0] as the launch reads it, so whoever rewrites hyper[0] is followed without another word; lr_scale = wd_scale = 1 without
 * a table and for elements of no segment; the four fp32 factors are multiplied in double, each pair exactly, the pairs' product
 * rounded once.  dk is uniform over the launch, or over a segment.  The product p * dk is not contracted into the subtraction behind
 * it: the result is, bit for bit, p.mul_(dk) followed by the coupled call with weight_decay = 0 -- and with weight_decay == 0 that
 * call itself.  lr_scale == 0: dk == 1, the parameter stays and the moments advance.  A frozen segment is neither read nor written.
 * grad_scale multiplies the gradient only.  The average is lerped towards the parameter after decay and update, from its register.
 * SDUMC_EINVAL before anything is launched and before the step count advances: whatever the coupled call of the same form refuses;
 * ema NULL with ema_decay or ema_warmup other than zero. */
int sdumc_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* hyper, float beta1,
                     float beta2, float eps, float weight_decay, float grad_scale, const sdumc_rate_seg* segs, int32_t nseg,
                     float* ema, float ema_decay, int32_t ema_warmup, void* stream);
/* sdumc_adam_multi with that rule (lr_scale = wd_scale = 1): the same segments, launches and refusals, the decoupled
 * instantiation of the same kernel, the bits of sdumc_adamw_step over the concatenation. */
int sdumc_adamw_multi(const sdumc_adam_seg* segs, int32_t nseg, float* exp_avg, float* exp_avg_sq, int64_t state_len,
                      float* hyper, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                      void* stream);

/* Batch assembly from a device-resident packed feature store = the collater's padding
 * (toolkit/utils/read_data.py:139-151, :223-248; toolkit/data/feat_data.py:232-253) on the GPU:
 * out[b, t, :] = packed[start[b] + t, :] for t < len[b], zero beyond, out is [B, Tmax, d].
 * packed [sum T, d] fp32, start int64 [B], len int32 [B] (device), d % 4 == 0. */
int sdumc_gather_pad(const float* packed, const int64_t* start, const int32_t* len, int32_t B, int32_t Tmax, int32_t d,
                     float* out, void* stream);
/* The same from store-wide tables: start_all int64 [N], len_all int32 [N] (device, one entry per stored utterance) and a
 * device index vector idx int64 [B] naming the batch's utterances -- an epoch then assembles its batches without copying
 * per-batch tables to the device.  len_out (optional, int32 [B]): min(len, Tmax) of the batch = the `lengths` the
 * key-padding extension takes (maxT - pad_len of feat_data.py:244-253). */
int sdumc_gather_pad_idx(const float* packed, const int64_t* start_all, const int32_t* len_all, const int64_t* idx, int32_t B,
                         int32_t Tmax, int32_t d, float* out, int32_t* len_out, void* stream);

/* A WHOLE batch in one launch (the collater above for every modality at once, toolkit/data/feat_data.py:232-253): up to
 * SDUMC_GATHER_MAX_SEGS packed tensors -- the four modalities' features and, when the store holds them, their P3 planes
 * (sdumc_p3_split of the packed tensor, made once per dataset: the planes of a zero row are zero bytes, so gathering plane rows
 * equals splitting the gathered batch bit for bit) -- into the step's input buffers, the labels (labels_out[b] =
 * labels_all[idx[b]], both or neither) and the valid frame counts (seg.len_out, optional).  A segment's rows are `d4` 16-byte
 * units wide (fp32 rows: d / 4; bf16 rows: d / 8; P3 rows: 3 d / 8), whatever they hold.  A segment with map_out writes the batch's
 * ROW MAP instead of (or beside) the padded copy: 4 bytes per frame instead of its 10 d.  max_workgroups > 0 caps the grid (the
 * kernel strides): a capped launch on a side stream fills the NEXT step's buffers beside the running step without queueing in
 * front of its kernels (sdumc_amd/engine.py, FusedTrainer); 0 = one pass.  seg.unit0 and total are filled by the call.
 *
 * THE RANDOM-MISSING PROTOCOL (miss_enable != 0; all-zero miss_* fields = none of it: a memset descriptor is unchanged).  Frame t
 * of a segment whose miss_mod is m (0..3 = audio, text, video, feat4), of utterance e = idx[b] (its index IN THE STORE), is ABSENT
 *   iff  word(t) < miss_frame_thr  or  (miss_all & 1)  or  word(0xFFFFFFFF) < miss_utt_thr  or  (miss_all & 2),   where
 *   word(c0) = philox4x32_10(counter = (c0, (uint32) e, 0x4D530000 + m, miss_draw), key = (miss_seed_lo, miss_seed_hi))[0]
 * (thresholds = floor(rate * 2^32), the dropout sites' "dropped when word < threshold"; a rate of 1 does not fit 32 bits and is the
 * miss_all flag; counter word 2 is disjoint from every dropout site under the same seed).  An absent frame is assembled exactly as
 * a padded one -- map_out entry = zero_row, row of the padded copy = zero bytes -- but STAYS A FRAME: len_out is unchanged, the
 * row takes part in the softmaxes like any zero feature row (the reference's audio_feat * mask, main_frame_val_text_missing.py:123-129,
 * without a rescale).  The decision depends on (seed, draw, m, e, t) alone: not on the batch, the position in it, B, Tmax, map or
 * copy, nor on the segment -- a modality's rows segment and its planes segment carry the same miss_mod and so lose the same frames.
 * miss_enable with a miss_mod outside 0..3 (or unknown miss_all bits) in any segment: SDUMC_EINVAL, nothing is launched. */
#define SDUMC_GATHER_MAX_SEGS 8
#define SDUMC_MISSING_SITE 0x4D530000u      /* + miss_mod: Philox counter word 2 of the protocol */
#define SDUMC_MISSING_UTT 0xFFFFFFFFu       /* counter word 0 of the utterance-level (whole modality) draw */
typedef struct sdumc_gather_seg {
  const void* packed;        /* [sum T, 16 d4 bytes] */
  const int64_t* start_all;  /* [N] first row of utterance e */
  const int32_t* len_all;    /* [N] its frames */
  void* out;                 /* [B, Tmax, 16 d4 bytes]; NULL (with d4 = 0 and map_out given): no padded copy, the map only */
  int32_t* len_out;          /* optional [B] */
  int32_t* map_out;          /* optional int32 [B * Tmax]: store row of batch row (b, t) = start_all[e] + t, or zero_row for padding
                                (sdumc_net_io.row_map: the step then reads the batch in place) */
  int32_t zero_row;          /* index of an all-zero row of the packed tensor (the store appends one) */
  int32_t Tmax, d4;
  int32_t miss_mod;          /* the random-missing protocol (above): the segment's modality index 0..3 */
  uint32_t miss_frame_thr;   /* floor(frame rate * 2^32), clamped to 2^32 - 1 */
  uint32_t miss_utt_thr;     /* floor(modality rate * 2^32), likewise: the whole utterance loses this modality */
  uint32_t miss_all;         /* bit 0: frame rate >= 1, bit 1: modality rate >= 1 (every frame absent, exactly) */
  int64_t unit0;            /* (filled by the call: first output row of the segment in the launch's row space) */
} sdumc_gather_seg;
typedef struct sdumc_gather_desc {
  sdumc_gather_seg seg[SDUMC_GATHER_MAX_SEGS];
  int32_t nseg, B;
  const int64_t* idx;        /* device [B] */
  const float* labels_all;   /* [N] or NULL */
  float* labels_out;         /* [B] or NULL */
  int64_t total;             /* (filled by the call: output rows of all segments) */
  uint32_t miss_seed_lo, miss_seed_hi;   /* the protocol's Philox key: seed & 0xffffffff, seed >> 32 */
  uint32_t miss_draw;        /* counter word 3: the epoch number in training, a fixed number in evaluation */
  uint32_t miss_enable;      /* 0: no frame is absent, whatever the other miss_* fields hold */
} sdumc_gather_desc;
int sdumc_gather_batch(const sdumc_gather_desc* g, int32_t max_workgroups, void* stream);

/* Temporal pre-compression of a packed feature tensor on the device = func_mapping_feature (toolkit/utils/read_data.py:120-137)
 * for every utterance of one modality at once: what feature_scale_compress, align_to_text and align_to_utt (:178-200) do per
 * sample on the host in the dataset constructors (toolkit/data/feat_data.py:117-126, :398-407; the driver's --feat_scale and
 * --feat_type, main_frame_val_text_missing.py:225-226).  Utterance e: source rows [src_start[e], + L), L = src_len[e]; destination
 * rows [dst_start[e], + n), n = dst_len[e] >= 1:
 *   L <= n: dst[j] = src[j] for j < L, zero for L <= j < n (the zero rows are frames from then on);
 *   L >  n: q, r = divmod(L, n); pool = q, pad = 0 if r == 0, else pool = q + 1, pad = n - r (padding on the LEFT);
 *           dst[j] = (sum over t in [0, pool) of src[j pool + t - pad]) / pool, a frame index below 0 contributing +0.
 * Arithmetic: the sum in fp64 in frame order, ONE fp64 division by pool (never by the count of real frames), one rounding to fp32
 * -- the reference promotes to float64 through its np.zeros padding and torch.FloatTensor rounds the result.  bf16 rows: the fp64
 * quotient rounded to fp32, then to bf16 (the two roundings of fp32 -> .to(bfloat16)).
 * The kernel ALSO writes destination row [dst_rows] as zeros: the store's trailing all-zero row (row maps name it).  dst therefore
 * holds dst_rows + 1 rows, dst_rows = sum of dst_len.  dst_start must ascend (the owner of a row is found by binary search); a row
 * no utterance owns, or whose source frames do not lie in [0, src_rows), is written as zeros -- nothing is read out of bounds.
 * One wave per destination row, one 16-byte chunk per lane, every element offset in 64 bits; plain loads and stores only.
 * max_workgroups > 0 caps the grid (the kernel strides), 0 = the default cap of 2048 workgroups.
 * SDUMC_EINVAL, before anything is launched: desc or one of its six pointers NULL, src / dst not 16-byte aligned, a table not
 * aligned to its element, cols < 1 or cols % 4 != 0 (cols % 8 != 0 for bf16), n_utts / src_rows / dst_rows < 1, bf16 not 0 or 1. */
typedef struct sdumc_pool_desc {
  const void* src;           /* [src_rows (+ anything), cols] fp32, or bf16 when bf16 = 1 */
  void* dst;                 /* [dst_rows + 1, cols], same element type */
  const int64_t* src_start;  /* device [n_utts] */
  const int32_t* src_len;    /* device [n_utts] */
  const int64_t* dst_start;  /* device [n_utts], ascending */
  const int32_t* dst_len;    /* device [n_utts], every entry >= 1 */
  int64_t src_rows, dst_rows;
  int32_t n_utts, cols;
  int32_t bf16;              /* 0: fp32 rows, 1: bf16 rows */
} sdumc_pool_desc;
int sdumc_pool_frames(const sdumc_pool_desc* p, int32_t max_workgroups, void* stream);

/* ------------------------------------------------------------------------
 * Generic fairseq-style multi-head attention and the pieces of the pre-LN Transformer encoder
 * (toolkit/models/modules/transformers_encoder/, all three files).
 * Activations are Time x Batch x Channel ([T, B, E] row-major) as in the reference (multihead_attention.py:51).
 * Dropout descriptors on [T, B, E] tensors use samples = T, rows = B, width = E; on the attention
 * probabilities [B*H, Tq, Tk] samples = B*H, rows = Tq, width = Tk (a width that is not a multiple of 4
 * uses ceil(width/4) Philox calls per row).
 * ---------------------------------------------------------------------- */

/* nn.LayerNorm(E) (transformer.py:201-203): y = (x - mean) * rstd * gamma + beta over the last axis,
 * biased variance, rstd = 1/sqrt(var + eps).  mean / rstd [rows] are saved for the backward. */
int sdumc_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                        int64_t rows, int32_t width, float eps, void* stream);
/* dx = LayerNorm backward (+ dx_add when not NULL: the residual branch's gradient meeting at x; dx_add may alias dx);
 * dgamma, dbeta [width] overwritten (deterministic two-stage column reduction through `workspace`). */
size_t sdumc_layernorm_bwd_workspace_bytes(int64_t rows, int32_t width);
int sdumc_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                        float* dx, float* dgamma, float* dbeta, const float* dx_add, int64_t rows, int32_t width,
                        float* workspace, size_t workspace_bytes, void* stream);

/* Softmax over the key axis of the attention scores, with the additive mask, the attention dropout and the
 * head-averaged weights the reference returns (multihead_attention.py:104-117, :128-130). */
typedef struct sdumc_softmax {
  int32_t batch, heads, tq, tk;
  float scale;            /* d_h^-0.5: the reference scales q (:84); here it multiplies S = q.k^T */
  const float* mask;      /* optional additive [tq, tk] (attn_mask.unsqueeze(0), :108); may hold -inf */
  float* scores;          /* in: S [batch*heads, tq, tk]; out: P = softmax(scale*S + mask) (saved for backward) */
  float* probs_drop;      /* drop.enabled: P * keep/(1-p), what multiplies V (:117); else unused (may be NULL) */
  float* weights;         /* optional [batch, tq, tk]: mean over heads of what multiplies V (:128-130) */
  sdumc_dropout drop;     /* F.dropout(attn_weights, p=attn_dropout) (:117) */
} sdumc_softmax;
int sdumc_softmax_fwd(const sdumc_softmax* s, void* stream);
/* dscores [batch*heads, tq, tk]: in dL/d(what multiplies V), out (in place) dL/dS.  Reads s->scores (= P). */
int sdumc_softmax_bwd(const sdumc_softmax* s, float* dscores, void* stream);

/* y = drop(alpha * x + pos) + residual over a [samples, rows, width] tensor:
 *   the "dropout -> add residual" of TransformerEncoderLayer.forward (transformer.py:161-162, :168-172; alpha = 1),
 *   the embedding stage of TransformerEncoder.forward (:68-71; alpha = sqrt(E), pos_table = sinusoidal table,
 *   position of token (t, b) = t + 1 if x[t, b, 0] != 0 else 0 -- position_embedding.py:8-26 with padding_idx 0),
 *   and the backward of both (x = dy, residual NULL). */
typedef struct sdumc_dropadd {
  const float* x;
  float alpha;
  const float* pos_table;  /* optional [samples + 1, width], row 0 = padding row */
  const float* pos_src;    /* tensor whose first channel decides padding (the un-scaled input); NULL with pos_table NULL */
  const float* residual;   /* optional */
  float* y;
  int32_t samples, rows, width;
  sdumc_dropout drop;
} sdumc_dropadd;
int sdumc_drop_add(const sdumc_dropadd* d, void* stream);

/* MultiheadAttention.forward (multihead_attention.py:48-131) and its backward.
 * query [tq, B, E], key / value [tk, B, E].  Pointer equality of query / key / value selects the fused
 * projection paths the reference selects with data_ptr() tests (:61-62); the results do not depend on it.
 * add_bias_kv / add_zero_attn (:28-38, default off, never enabled by transformer.py) are not implemented. */
typedef struct sdumc_mha {
  int32_t tq, tk, batch, embed, heads;
  const float* query;
  const float* key;
  const float* value;
  const float* in_proj_weight;   /* [3E, E] rows = (q | k | v) (:24, :133-154) */
  const float* in_proj_bias;     /* [3E] or NULL */
  const float* out_proj_weight;  /* [E, E] (:30) */
  const float* out_proj_bias;    /* [E] or NULL */
  const float* attn_mask;        /* optional additive [tq, tk] */
  sdumc_dropout attn_drop;       /* enabled = training and attn_dropout > 0 */
  float* out;                    /* [tq, B, E] */
  float* weights;                /* [B, tq, tk] head-averaged attention weights, or NULL */
  /* caller-owned intermediates, saved for the backward */
  float* q;                      /* [tq, B, E] projected queries (unscaled) */
  float* k;                      /* [tk, B, E] */
  float* v;                      /* [tk, B, E] */
  float* probs;                  /* [B*H, tq, tk] softmax output */
  float* probs_drop;             /* [B*H, tq, tk] when attn_drop.enabled, else NULL */
  float* ctx;                    /* [tq, B, E] attention output before out_proj */
  float* workspace;              /* >= sdumc_mha_workspace_bytes */
  size_t workspace_bytes;
  int32_t bf16;                  /* 1: every product (projections, q.k^T, P.v and their backward) rounds its operands to bf16,
                                    fp32 accumulate (needs embed and head_dim multiples of 4; otherwise the call stays fp32);
                                    softmax, dropout, bias and the stored tensors are fp32 either way.  0: exact fp32 */
  /* add_bias_kv / add_zero_attn (multihead_attention.py:28-38, :86-104).  With ts = tk + (bias_k != NULL) + add_zero_attn the
   * source length becomes ts: k, v are [ts, B, E], probs / probs_drop [B*H, tq, ts], weights [B, tq, ts], attn_drop.width = ts;
   * attn_mask stays [tq, tk] (the extra columns are unmasked, as the reference's zero-padded mask).  Defaults: NULL, NULL, 0. */
  const float* bias_k;           /* [E] or NULL; both or neither */
  const float* bias_v;
  int32_t add_zero_attn;
} sdumc_mha;

typedef struct sdumc_mha_grads {
  const float* dout;             /* [tq, B, E] */
  float* dquery;                 /* [tq, B, E] overwritten.  Where the forward inputs aliased, pass the same */
  float* dkey;                   /* [tk, B, E] aliasing here: the contributions are then summed into one buffer */
  float* dvalue;                 /* [tk, B, E] */
  float* d_in_proj_weight;       /* [3E, E] overwritten */
  float* d_in_proj_bias;         /* [3E] or NULL */
  float* d_out_proj_weight;      /* [E, E] */
  float* d_out_proj_bias;        /* [E] or NULL */
  float* d_bias_k;               /* [E], required when bias_k is given */
  float* d_bias_v;
} sdumc_mha_grads;

size_t sdumc_mha_workspace_bytes(const sdumc_mha* m, int32_t backward);
int sdumc_mha_forward(const sdumc_mha* m, void* stream);
int sdumc_mha_backward(const sdumc_mha* m, const sdumc_mha_grads* g, void* stream);

/* misc */
/* n (<= 8) strided copies in one launch */
typedef struct sdumc_copy_seg {
  const float* src; float* dst;
  int32_t ld_src, ld_dst, rows, cols;
} sdumc_copy_seg;
int sdumc_copy2d_multi(const sdumc_copy_seg* segs, int32_t n, void* stream);
/* Indexed row scatter of up to SDUMC_SCATTER_MAX_SEGS tensors in ONE launch:
 *   dst_k[idx[r % B], 0:cols_k] = src_k[r, 0:cols_k]   for r < rows_k          (rows_k a multiple of B; both tensors contiguous)
 * What an evaluation epoch over a resident feature store does after every eval-mode forward: the reference's validation / test
 * passes append each batch's predictions and embeddings to host lists (main_frame_val_text_missing.py:156-163,
 * main_frame_val_text_missing_inference.py:166-175); here the forward's five stream-major outputs ([2B, w]: rows [0, B) the full
 * stream, rows [B, 2B) the text-missing one) go to per-stream result tensors [N, w] at the rows the batch's utterances have in the
 * store (idx = the batch's index vector, device int64 [B], as sdumc_gather_desc.idx), so the results are in store order whatever
 * order the sampler visits them in, and nothing is copied to the host per batch.
 * mark (optional, uint8 [segs[0].dst_rows]): mark[idx[b]] = 1 for b < B -- the visited set.
 * A segment moves 16 bytes per lane when cols % 4 == 0 and both base addresses are 16-byte aligned, one float per lane otherwise
 * (cols = 1, odd widths, a view that starts mid-buffer).  Plain stores, no atomics: with distinct indices every destination element
 * is written once, so a repeated launch gives the same bits.  Rows are addressed with 64 bits.  The indices must be distinct and in
 * [0, dst_rows) -- the caller checks (DeviceFeatureStore.plan_epoch does, on the host); a row whose index is not in that range is
 * skipped, never written out of bounds.
 * SDUMC_EINVAL, before anything is launched: n < 1 or > SDUMC_SCATTER_MAX_SEGS, segs / idx NULL, B < 1, a segment with src or dst
 * NULL or not 4-byte aligned, rows < 1, cols < 1, rows % B != 0, dst_rows < 1 or dst_rows * cols beyond 2^61 elements. */
#define SDUMC_SCATTER_MAX_SEGS 10
typedef struct sdumc_scatter_seg {
  const float* src;   /* [rows, cols] */
  float* dst;         /* [dst_rows, cols] */
  int32_t rows, cols;
  int64_t dst_rows;
} sdumc_scatter_seg;
int sdumc_scatter_rows_multi(const sdumc_scatter_seg* segs, int32_t n, const int64_t* idx, int32_t B, uint8_t* mark,
                             void* stream);
/* The record a TRAINING epoch keeps of each step: one call, stream-ordered behind a completed sdumc_train_step, no host
 * synchronisation.  The reference's training pass is the same function as its evaluation pass: it appends every batch's train-mode
 * predictions of both streams (main_frame_val_text_missing.py:156-158), returns them with their MSE (:160-178) and the driver prints
 * train_val_mse_full / train_val_mse_missing once per epoch (:348); the inference variant keeps the four embeddings too
 * (main_frame_val_text_missing_inference.py:166-175).  When the step returns, its losses, its stream-major outputs
 * (sdumc_net_io.vals / fused / rnc / text_hidden / cross_text) and its raw gradients (the bucket at sdumc_step_grads_offset: Adam adds
 * the coupled L2 term inside its own kernel, so the bucket is without it) are on the device; this call files them away.  It reads the
 * step's memory and writes only log_row, the segments' destinations, mark and scratch: a run is bit for bit the same with or without it.
 * Three parts, each optional by its fields:
 *   scatter   nseg (0 .. SDUMC_SCATTER_MAX_SEGS) segments, idx, B, mark: exactly sdumc_scatter_rows_multi (the same device code and
 *             the same segment rules); nseg = 0: none.
 *   log row   log_row[0..7] = losses[0..7] as they stand, [8] = grad_norm, [9] = the number of non-finite gradient elements,
 *             [10] = B, [11] = hyper[0], the learning rate the step used.
 *   gradients grads != NULL: grad_norm = the L2 norm over all n_grads floats, accumulated in fp64 (a sum of fp32 squares cannot
 *             overflow there) and rounded ONCE to fp32 -- so a norm beyond the fp32 range comes out as +Inf (4099 elements of 3e38:
 *             1.9e40 in fp64, +Inf in the row); NaN and +-Inf elements propagate as in torch.linalg.vector_norm.  [9] counts the
 *             elements that are NaN or +-Inf, exactly while n_grads < 2^24.  Fixed order: every workgroup owns a contiguous slice and
 *             folds it in a fixed lane order to one fp64 partial in scratch; a second launch of one workgroup adds the partials in
 *             index order and writes the row: the same input gives the same bits on every call.  16-byte loads from the first
 *             aligned address on, whatever the base.  grads == NULL: [8] = NaN, [9] = 0, no reduce workgroups, one launch.
 *             (A one-launch form -- a ticket in scratch, the last workgroup to arrive adds the partials -- was built and measured:
 *             it tied with this one in the epoch, and the form without communication between workgroups was kept.)
 * scratch: caller-owned, sdumc_epoch_record_scratch_bytes of n_grads bytes (0 for n_grads < 1), 16-byte aligned; every call writes what
 * it reads of it, so it needs no initial value and is ready again after every call; one call at a time per scratch.  No atomics.
 * SDUMC_EINVAL, before anything is launched: r / log_row / losses / hyper NULL or not 4-byte aligned, nseg < 0 or >
 * SDUMC_SCATTER_MAX_SEGS, nseg > 0 with idx NULL or B < 1 or a segment sdumc_scatter_rows_multi would refuse, grads != NULL with
 * n_grads < 1, scratch NULL, grads not 4-byte or scratch not 16-byte aligned. */
typedef struct sdumc_epoch_rec {
  sdumc_scatter_seg seg[SDUMC_SCATTER_MAX_SEGS];
  int32_t nseg, B;
  const int64_t* idx;    /* device int64 [B]: the batch's rows in the store */
  uint8_t* mark;         /* optional, uint8 [seg[0].dst_rows] */
  const float* losses;   /* device float[8]: sdumc_step_cfg.losses */
  const float* hyper;    /* device float[4]: sdumc_step_cfg.hyper */
  float* log_row;        /* device float[12] */
  const float* grads;    /* optional: the step's gradient bucket */
  int64_t n_grads;
  void* scratch;
} sdumc_epoch_rec;
size_t sdumc_epoch_record_scratch_bytes(int64_t n_grads);
int sdumc_epoch_record(const sdumc_epoch_rec* r, void* stream);
/* The same reduce BY TENSOR: the L2 norm and the non-finite count of each of n (1 .. SDUMC_TENSOR_NORMS_MAX_SEGS) segments of fp32
 * device memory in two launches, stream-ordered, no host synchronisation.  What a training epoch keeps per step beside the one norm
 * of the whole bucket -- the gradient bucket cut at the parameter table's offsets, and the flat parameters against a snapshot of
 * their values before the step -- and what a loop over per-parameter .grad tensors asks for.  segs is a HOST table, read by the call.
 * Per segment t:
 *   norm[t]       fp32 of sqrt(sum_i x[i]^2)
 *   nonfinite[t]  the number of x[i] that are NaN or +-Inf (saturating at 2^31 - 1)
 *   y != NULL:    diff_norm[t] = fp32 of sqrt(sum_i (x[i] - y[i])^2), and then y[i] = x[i], in the same pass over the data: the
 *                 rolling snapshot (after the call y equals x bit for bit, so a second call gives 0).  x and y must not overlap.
 *   y == NULL (or count == 0): diff_norm[t] is left as it is; diff_norm may be NULL when no segment has a y.
 * count == 0 gives norm 0, nonfinite 0.  Differences, squares and sums are fp64 (a sum of fp32 squares cannot overflow there), rounded
 * ONCE to fp32 -- a norm beyond the fp32 range comes out as +Inf; NaN and +-Inf elements propagate as in torch.linalg.vector_norm.
 * Fixed order: the call cuts every segment into chunks by its count alone (8192 floats, at most 1024 chunks per segment, longer
 * chunks beyond that; a chunk never spans two segments), one workgroup folds a chunk in a fixed lane order into fp64 partials in
 * scratch, and the second launch adds each segment's partials in index order: the same input gives the same bits on every call,
 * wherever the segments lie.  No atomics.  Nothing but 4-byte alignment is assumed of x and y: 16-byte loads from a chunk's first
 * aligned element on (with a y, where x and y sit alike within 16 bytes; else that segment goes one float per lane), single
 * elements in front and behind.  norm / nonfinite / diff_norm name n consecutive elements, e.g. one row of a [steps, n] tensor.
 * scratch: caller-owned device memory of at least the scratch query's bytes for the same table (it depends on n and the counts
 * only; 0 = a table the entry refuses), 16-byte aligned; every call writes what it reads of it; one call at a time per scratch.
 * SDUMC_EINVAL, before anything is launched: segs NULL or not 8-byte aligned, n < 1 or > SDUMC_TENSOR_NORMS_MAX_SEGS, a negative
 * count, x NULL with count > 0, x or y not 4-byte aligned, norm / nonfinite NULL, diff_norm NULL while a segment has a y, an output
 * not 4-byte aligned, scratch NULL or not 16-byte aligned, scratch_bytes short. */
#define SDUMC_TENSOR_NORMS_MAX_SEGS 96
typedef struct sdumc_norm_seg {
  const float* x;
  float* y;              /* optional: the snapshot */
  int64_t count;         /* floats */
} sdumc_norm_seg;
size_t sdumc_tensor_norms_scratch_bytes(const sdumc_norm_seg* segs, int32_t n);
int sdumc_tensor_norms(const sdumc_norm_seg* segs, int32_t n, float* norm, int32_t* nonfinite, float* diff_norm, void* scratch,
                       size_t scratch_bytes, void* stream);
/* Global-norm gradient clipping and the non-finite step guard on the device: three launches, stream-ordered, no host
 * synchronisation, no atomics.  Over the n floats of `grads` (the fused step's bucket, sdumc_step_grads_offset):
 *   guard[0]  the L2 norm BEFORE clipping: fp64 sum of squares, fixed order, rounded once to fp32 (the reduce of sdumc_tensor_norms:
 *             chunks cut by the count alone, partials added in index order by a one-workgroup launch -- the same input gives the
 *             same bits on every call; a norm beyond the fp32 range reads +Inf here while the coefficient is taken from the fp64 value)
 *   guard[1]  coef = min(1, max_norm / (norm + 1e-6)), evaluated in double from the fp64 norm and rounded once to fp32 -- the
 *             expression of torch.nn.utils.clip_grad_norm_, 1e-6 included; max_norm <= 0: no clipping, coef = 1.  A NaN norm gives
 *             a NaN coefficient, as torch's clamp does.
 *   guard[2]  the number of elements that are NaN or +-Inf (exact below 2^24)
 *   guard[3]  skipped: 1 when skip_nonfinite == 1 and guard[2] > 0, else 0
 * and then grads[i] = grads[i] * coef in place, ONE fp32 multiply per element -- unless coef == 1 or the step is skipped: every
 * workgroup of the third launch reads guard first and then leaves without reading or writing the gradients, so an unclipped bucket
 * keeps its bits (-0.0 and subnormals included).  Scaling in place, not inside Adam: Adam's expression stays what it was, and a
 * clipped step is bit for bit "multiply the bucket by guard[1], then sdumc_adam_step".
 * hyper (optional): sdumc_step_cfg.hyper.  A skipped step sets hyper[1] -= 1, the step count as before the step -- the fused step
 * advances it in its loss stage, before a gradient exists.  hyper[2..3] are derived from hyper[1] and are NOT restored: the next
 * step's advance rewrites both before anyone reads them (the skipped step's own Adam launch applies nothing).
 * Nothing but 4-byte alignment is assumed of grads: 16-byte accesses from a chunk's first aligned element on, single elements in
 * front and behind.  scratch: caller-owned, sdumc_grad_guard_scratch_bytes(n) bytes (0 for n < 1), 16-byte aligned; every call
 * writes what it reads of it; one call at a time per scratch.
 * SDUMC_EINVAL, before anything is launched: grads / scratch / guard NULL, n < 1, max_norm NaN, skip_nonfinite other than 0 / 1,
 * grads, hyper or guard not 4-byte aligned, scratch not 16-byte aligned.
 * sdumc_grad_guard_multi: the same over the per-parameter gradient tensors of a loop that keeps p.grad, found through
 * sdumc_tensor_norms' segment table (HOST memory, read by the call; 1 .. SDUMC_TENSOR_NORMS_MAX_SEGS segments, y must be NULL; the
 * segments are SCALED in place although x is declared const): ONE norm over all segments, every segment scaled by the one
 * coefficient.  No hyper and no skip: guard[3] = 0.  Scratch by sdumc_grad_guard_multi_scratch_bytes of the same table (0 = a table
 * the entry refuses).  SDUMC_EINVAL: a table sdumc_tensor_norms would refuse, a segment with a y, scratch / guard NULL or misaligned
 * as above, max_norm NaN; SDUMC_ENOMEM: scratch_bytes short.  Both before anything is launched. */
size_t sdumc_grad_guard_scratch_bytes(int64_t n);
int sdumc_grad_guard(float* grads, int64_t n, float max_norm, int32_t skip_nonfinite, float* hyper, void* scratch, float* guard,
                     void* stream);
size_t sdumc_grad_guard_multi_scratch_bytes(const sdumc_norm_seg* segs, int32_t nseg);
int sdumc_grad_guard_multi(const sdumc_norm_seg* segs, int32_t nseg, float max_norm, void* scratch, size_t scratch_bytes,
                           float* guard, void* stream);
/* dst[r, 0:cols] = src[r, 0:cols] for r < rows, with leading dimensions */
/* dst[r, 0:cols] += src[r, 0:cols] */
int sdumc_axpy2d(const float* src, int32_t ld_src, float* dst, int32_t ld_dst, int32_t rows, int32_t cols, void* stream);
int sdumc_copy2d(const float* src, int32_t ld_src, float* dst, int32_t ld_dst, int32_t rows, int32_t cols, void* stream);
int sdumc_fill(float* p, float v, int64_t n, void* stream);
/* device rng/step state helpers: state = {seed_lo, seed_hi, call0}; adds `inc` to call0 */
int sdumc_rng_advance(uint32_t* dev_state, uint32_t inc, void* stream);
/* keep-bits of a [streams*samples, rows, width] row space, one byte per 4 columns (see sdumc_dropout.bits) */
int sdumc_dropout_bits(const sdumc_dropout* d, int32_t streams, uint8_t* bits, void* stream);
/* the same for nsite (<= 4) sites d->site + s * site_stride that share the row space, in one launch
 * (width must be a multiple of 16: four quads are packed per 32-bit store; bits[s] 4-byte aligned) */
int sdumc_dropout_bits_multi(const sdumc_dropout* d, int32_t streams, int32_t nsite, int32_t site_stride,
                             uint8_t* const* bits, void* stream);
/* bf16-storage mode: the keep-bits of the TWO sites d->site and d->site + site_stride (they read the same frames: fra2utt_m and
 * cross_att_fra2utt_m, model :59, :81) and the masked frames xd[s][row, :] = bf16(x[row % x_rows, :] * keep_s * d->scale) of
 * both, in one pass over x -- what sdumc_dropout_bits_multi followed by two sdumc_mask_apply_bf16 produce, bit for bit.
 * x, xd[s]: bf16 [.., width], 16-byte aligned; width % 16 == 0; d->enabled must be set. */
int sdumc_dropout_bits_apply_bf16(const sdumc_dropout* d, int32_t streams, int32_t site_stride, uint8_t* const* bits,
                                  const void* x, int64_t x_rows, void* const* xd, void* stream);
/* writes the dropout mask values (0 or scale) of a [streams*samples, rows, width] tensor: test hook */
int sdumc_dropout_mask(const sdumc_dropout* d, int32_t streams, float* mask, void* stream);
const char* sdumc_version(void);

/* Optional per-launch timing of the GEMM kernels with HIP events recorded on the launch stream
 * (bench.py's roofline leg; not for use under graph capture).  enable(1) clears and starts,
 * report() synchronises the recorded events and aggregates per kernel variant. */
typedef struct sdumc_prof_entry {
  const char* name;      /* e.g. "gemm_nt_128x128" */
  int64_t launches;
  double total_ms;
  double total_flops;    /* algorithmic: 2*M*N*K*groups per launch */
} sdumc_prof_entry;
int sdumc_profile_enable(int on);
int sdumc_profile_report(sdumc_prof_entry* out, int max_entries);

/* ========================================================================
 * Network level: WengnetMOSEIMultViewsTextMissing (model :186-370) as one call.
 *
 * Parameters live in ONE flat fp32 buffer: the live parameters (those that receive a
 * gradient) first, the dead ones after; every tensor starts on a
 * 16-byte boundary.  sdumc_param_table() prints "name offset rows cols live\n" lines with the
 * reference's state_dict names, so the Python nn.Module exposes nn.Parameters that are views of
 * the flat buffer and the published checkpoint loads by name.
 * ==================================================================== */
int64_t sdumc_param_count(int32_t da, int32_t dt, int32_t dv);      /* floats in the flat buffer */
int64_t sdumc_param_live_count(int32_t da, int32_t dt, int32_t dv); /* floats in the live prefix (gradient bucket) */
int32_t sdumc_param_table(int32_t da, int32_t dt, int32_t dv, char* buf, size_t buflen); /* bytes written or <0 */

typedef struct sdumc_net_dims {
  int32_t B;        /* local batch */
  int32_t streams;  /* 1 = one reference forward call; 2 = both streams of main :119,:131 batched */
  int32_t Ta, Tv;   /* frames of audio / video (padded to the batch max by the collater) */
  int32_t Tt[2];    /* frames of the text-slot input of stream 0 (text) and stream 1 (feat4) */
  int32_t da, dt, dv;   /* feature widths = args.input_dims[0:3] (model :193-195) */
  int32_t train;    /* 1: dropout on (model.train()), 0: identity (model.eval()) */
  int32_t sample0;  /* global index of local sample 0 (data-parallel shard offset) */
  double p_frame;   /* 0.5: nn.Dropout inside FRA2UTT_new / Cross_Attention (model :54,:77) */
  double p_mlp;     /* 0.3: constructor default dropout (model :187) */
  int32_t bf16;     /* 0 (default): exact fp32 everywhere.
                       1: fp32 storage; the frame-level projections (frame_dim_reshape_*, model :282-284, and the input_proj
                       keys of FRA2UTT_new / Cross_Attention, model :60,:82), forward and backward, round their operands to bf16
                       on the way to v_mfma_f32_32x32x16_bf16 (fp32 accumulation).
                       2: bf16 STORAGE (BASELINE configs[2], configs[4]): the input features (sdumc_net_io.audio / video /
                       text are then bf16 tensors), the projected frames, the masked frames, the tanh keys and the frame-level
                       gradients live in HBM as bf16; products accumulate in fp32, bias / tanh / softmax / pooling / the
                       utterance-level network / losses / Adam (fp32 master weights) stay fp32.  Needs da, dt, dv % 64 == 0. */
} sdumc_net_dims;

typedef struct sdumc_net_io {
  const float* audio;    /* [B, Ta, da] */
  const float* video;    /* [B, Tv, dv] */
  const float* text[2];  /* [B, Tt[s], dt]: stream 0 = text, stream 1 = feat4 (streams==1: text[0]) */
  float* params;         /* flat parameter buffer */
  const uint32_t* rng_state; /* device {seed_lo, seed_hi, call0}; stream s draws call0 + s */
  void* workspace;       /* >= sdumc_net_workspace_bytes(dims); holds the activations saved for backward,
                            so it must stay untouched between forward and backward */
  size_t workspace_bytes;
  /* outputs, V = streams*B rows, stream-major (model :370) */
  float* vals;           /* [V, 1]      vals_out */
  float* fused;          /* [V, 128]    cross_fused_feat */
  float* rnc;            /* [V, 64]     feat4rnc */
  float* text_hidden;    /* [V, 256]    text_hidden (after cross_text_query_mlp, model :329) */
  float* cross_text;     /* [V, 7, 128] cross_hiddens[:,1] */
  /* EXTENSION, default all NULL = reference behaviour: device int32 [B] valid frame counts of audio, text, video, feat4
   * (maxT - pad_len of toolkit/data/feat_data.py:232-253's `pads`); when given, the six attention poolings mask the
   * padded frames (sdumc_attnpool.lengths).  All four (three when streams == 1) or none. */
  const int32_t* lengths[4];
  /* Optional, fp32 storage only: the same features as P3 tensors (sdumc_p3_split: three bf16 planes, 6 bytes per element, rows of
   * 6 d bytes, 16-byte aligned) -- all of them (audio_p3, video_p3, text_p3[0 .. streams - 1]) or none.  When given, the frame
   * projections (model :282-284) and the Cross_Attention key projections (model :82) read planes that were split ONCE -- the
   * features when the batch was installed (they do not change across epochs), the projected frames by the projection's own epilogue --
   * instead of splitting fp32 operands per workgroup per k-tile (csrc/gemm_p3.hip).  The fp32 tensors above are still read by the
   * weight gradients.  Same arithmetic, same results to the last fp32 rounding or two (another summation order). */
  const void* audio_p3;
  const void* video_p3;
  const void* text_p3[2];
  /* Optional, fp32 storage with planes: the batch is read IN PLACE from a resident feature store.  audio / video / text[s] (and the
   * *_p3 pointers) are then the store's PACKED tensors [rows + 1][d] -- every utterance's frames one after the other, of any total size
   * (tens of GB: 64-bit addressing), the last row all zero -- and row_map[i] (i = audio, text, video, feat4 as in `lengths`; device
   * int32 [B * T_i]) names, for batch row b * T_i + t, the store row it is: start of utterance b + t for a valid frame, the zero row for
   * padding (sdumc_gather_batch writes such maps: sdumc_gather_seg.map_out).  No padded copy of the batch exists anywhere: the frame
   * projections fetch their A rows through the map (sdumc_gemm_p3.a_map), the frame projections' weight gradients their B rows
   * (sdumc_gg_problem.b_map); nothing else reads the features.  All four (three when streams == 1) or none; fp32 storage: needs the
   * *_p3 planes and the default split arithmetic; bf16 storage (audio / video / text[s] = the store's packed bf16 tensors): feature
   * widths multiples of 128; else SDUMC_EINVAL.  The backward additionally needs every modality's frame_dim_reshape weight gradient
   * in the grouped launch (grouped weight gradients on; fp32 storage: its split arithmetic on -- sdumc_set_split_ bit 0 --
   * and widths multiples of 4; the packed tensors 16-byte aligned):
   * sdumc_net_backward, sdumc_net_backward_phase (EITHER phase) and sdumc_train_step decide their schedule first and return
   * SDUMC_EINVAL before anything of the call is enqueued -- no fill, no fork, for sdumc_train_step no forward and no loss stage;
   * sdumc_net_forward does not read the fp32 tensors and accepts such a batch.  What the forward needs is a frame projection that
   * reads through a map -- the plane GEMM (fp32 storage: planes given, SDUMC_P3 not 0, the wide-tile family's split arithmetic on:
   * sdumc_set_split_ bit 1) or the fragment-major bf16 GEMM (bf16 storage: widths multiples of 128, SDUMC_P3 not 0); without one
   * sdumc_net_forward and sdumc_train_step, which decide the forward's schedule first as well, return SDUMC_EINVAL before anything
   * of the call is enqueued -- no lengths expansion, no fork, no event.
   * The bf16 weight-gradient kernel reads map entries four at a time: each map must be
   * readable up to a multiple of four entries.  store_rows[i] (optional): rows of packed tensor i -- tensors (and planes) below
   * 4 GiB keep the kernels' descriptor addressing, which is faster than 64-bit addresses; 0 = unknown. */
  const int32_t* row_map[4];
  int64_t store_rows[4];
  /* Optional, train mode in fp32 storage: sdumc_net_bits_next_bytes(dims) bytes the caller keeps ACROSS calls of the same dims (its
   * own allocation, not part of `workspace`; zero it once) -- TWO sets of keep-bits for the frame-level input dropouts, each with a
   * {seed, call} tag.  A call reads set (bits_phase & 1); in its latency-bound middle, where the chip idles, it fills the OTHER set
   * for the next call (Philox call index + 2: what sdumc_train_step advances by) and tags it.  The caller flips bits_phase from call
   * to call (forward and backward of one step take the same value); the next call's head launch then finds its set tagged with its
   * own {seed, call} and has nothing to generate -- at the head the Philox launches compete with the frame projections.
   * Bit-identical masks either way: a set whose tag names another seed, call or batch shape (first call, a reset counter, a different
   * advance, a phase that was not flipped, a ragged epoch's next shape that was not announced) is regenerated at the head of the call
   * that reads it, and re-tagged for that call.
   * Shapes that change from call to call (toolkit/utils/read_data.py:223-248 pads every batch to its own maximum): the buffer is
   * sized for the LARGEST dims of the run (bits_next_bytes = sdumc_net_bits_next_bytes of those; 0 = exactly this call's, the set
   * stride then follows the call's own dims), and bits_next_dims names the dims of the NEXT call (same widths, streams, train and
   * bf16 fields; B, sample0 and the frame counts may differ; NULL = the same as this call): the middle of this call lays the other
   * set out for them.
   * Ordering: sdumc_net_forward returns with the fill of the other set ordered before `stream` (a caller may then advance the
   * counter, or free / re-zero the buffer, behind `stream`); inside sdumc_train_step that join is left to the backward. */
  void* bits_next;
  int32_t bits_phase;
  size_t bits_next_bytes;
  const struct sdumc_net_dims* bits_next_dims;
  /* Optional: the assembly of the NEXT batch (sdumc_gather_batch's descriptor: its row maps, or its padded copy; the output buffers
   * must not be ones this call reads), issued by the call itself on its background lane at the start of its utterance-level middle --
   * from there to the backward's frame-level tail the chip's HBM is mostly idle (the step is latency- and matrix-bound there), so the
   * batch is put together beside the step instead of in front of the next one.  sdumc_train_step (and a sdumc_net_forward on its own)
   * returns with the gather ordered before `stream`.  prefetch_workgroups caps its grid (0 = 512: two small workgroups per CU leave
   * every CU room for the step's own kernels).  The descriptor is read during the call only. */
  const sdumc_gather_desc* prefetch;
  int32_t prefetch_workgroups;
  /* Optional caller-owned execution context (sdumc_ctx_create): the internal side streams and the event ring the call forks
   * its branches on.  NULL = the default context of the current device (one per device, created on first use).  Two host
   * threads that run steps concurrently -- on distinct streams of one device, or on two devices -- give each its own
   * context; a context is used by one thread at a time and only on the device it was created on (else SDUMC_EINVAL). */
  void* ctx;
} sdumc_net_io;

/* Execution contexts (see sdumc_net_io.ctx).  Create / destroy outside stream capture; destroy only when no work issued
 * through the context is pending.  Stream lifetime: the clustered utterance-level launches of a device order themselves behind
 * the previous such launch with an event recorded on THAT launch's stream -- a caller that destroys the stream it ran its last
 * step on must have synchronised it first (torch's pooled streams are never destroyed; the library's own lanes are handled by
 * sdumc_ctx_destroy). */
size_t sdumc_net_bits_next_bytes(const sdumc_net_dims* d);   /* 0 = the dims do not use it (eval, bf16 storage) */
int sdumc_ctx_create(void** ctx);
int sdumc_ctx_destroy(void* ctx);
/* Schedule options of ONE execution context (ctx NULL = the current device's default context): nothing process-wide changes, so
 * two callers -- or two tests -- with their own contexts cannot disturb each other.  value < 0 returns the option to the
 * process-wide default (the sdumc_set_* calls below, kept for callers without a context).
 *   SDUMC_OPT_CONCURRENCY      0 = every launch on the caller's stream (per-kernel profiling), 1 = the internal lanes
 *   SDUMC_OPT_BACKGROUND_LANE  0 / 2 / 3 as sdumc_set_background_lane
 *   SDUMC_OPT_CHAIN_CLUSTER    0 = csrc/chain.hip's kernels, 1 = the clustered ones wherever the shape fits
 *   SDUMC_OPT_SPLIT            0..15: which fp32 GEMM kernel families multiply on the bf16 matrix pipe (bits as sdumc_set_split_) */
enum { SDUMC_OPT_CONCURRENCY = 0, SDUMC_OPT_BACKGROUND_LANE = 1, SDUMC_OPT_CHAIN_CLUSTER = 2, SDUMC_OPT_SPLIT = 3 };
int sdumc_ctx_set_option(void* ctx, int32_t option, int32_t value);

/* The network-level calls issue independent branches (the three per-modality chains; the dW GEMMs) on up to
 * two internal side streams forked from / joined to `stream` with events: the call stays stream-ordered
 * with respect to `stream`.  sdumc_set_concurrency(0) keeps everything on `stream` (per-kernel profiling:
 * overlapping kernels share the GPU, so their individual durations stop being meaningful). */
int sdumc_set_concurrency(int on);
/* The Cross_Attention-site key projections (forward, dW, dX: ~0.4 ms of MFMA-bound GEMMs per step at C2) are not on
 * the critical path of the launch-bound utterance-level chain (model :293-332 forward, its mirror backward).  1 = issue
 * them on a fourth internal stream beside that chain instead of grouped with the FRA2UTT-site ones, 2 = the forward
 * ones only (+1.0 % per step over mode 0 on MI355X: the HBM-bound FRA2UTT pooling then overlaps the MFMA-bound
 * Cross_Attention key GEMM), 3 (the default) = 2 plus the audio modality's backward ones (+0.6 % over 2: the longest
 * frame-level chain gets shorter), 4 = audio and video (+0.4 %); mode 1 loses 1.6 % against mode 2. */
int sdumc_set_background_lane(int on);
/* Debug timeline: with marks on, sdumc_train_step records an event on the caller's stream at fixed points (0 start, 1/2 around
 * the first utterance-level launch, 3/4 the second, 5 after the losses, 6 after the first backward utterance-level launch, 7/8
 * around the second, 9 before Adam, 10 end); _read returns their times in ms since mark 0 (-1 = not recorded) once the caller
 * has synchronised.  Process-wide and single-threaded: a measurement aid (tools/step_marks.py), not part of the data path. */
/* The utterance-level stages run as clustered kernels (four workgroups split every layer's columns and exchange their slices
 * through HBM + a flag, csrc/chain_cluster.hip) whenever all their workgroups fit the device at once (2 x streams x B <= 128
 * on MI355X) and the stream is not being captured; 0 keeps the one-workgroup-per-sample-pair kernels of csrc/chain.hip.
 * Failure contract: the members of a cluster wait for each other with a bounded spin.  A spin that runs into its cap (another
 * process holding the GPU's CUs, a hung member) sets a sticky per-device error word and lets the kernel finish with wrong data;
 * from then on every Adam launch of this library on that device (sdumc_train_step, sdumc_adam_step) applies NOTHING -- parameters
 * and moments keep their values -- and the fused step's total loss reads NaN.  sdumc_chain_cluster_error_() synchronises the
 * device and returns the word (0 = fine); sdumc_chain_cluster_reset_error() clears it (and the clusters' counters) once the
 * caller has dealt with the failed step, e.g. by repeating it with sdumc_set_chain_cluster(0).
 * sdumc_chain_cluster_test_hold_(1) is a test hook: workgroup 0 of every following clustered launch withholds its arrivals, which
 * drives exactly that failure path on purpose (tests/test_gpu_net.py). */
int sdumc_set_chain_cluster(int on);
int sdumc_chain_cluster_error_(void);
int sdumc_chain_cluster_reset_error(void);
int sdumc_chain_cluster_test_hold_(int on);
/* Data-parallel runs (one process per GPU): the error word is per device, so the ranks exchange it with the gradients.
 * _flag writes 1.0f (word set) or 0.0f into `flag` -- a float the caller appends to its gradient bucket -- stream-ordered and
 * without a host synchronisation; after the SUM all-reduce of the bucket, _merge sets the local word when the reduced flag is
 * non-zero, so that every rank's Adam applies nothing and every rank raises (sdumc_amd/trainer.py). */
/* Diagnosis (SDUMC_CL_MODE bit 4): records of cached weight loads that differed from agent-scope loads of the same address in the
 * stage-A forward kernel: out[0] = count, out[8 + 12 i ..] = {workgroup, thread, ring slot, address low word, 4 cached words, 4
 * coherent words}; synchronises the device and clears the records.  Not part of the data path. */
int sdumc_chain_cluster_debug_read_(uint32_t* out, int n);
int sdumc_chain_cluster_error_flag(float* flag, void* stream);
int sdumc_chain_cluster_error_merge(const float* flag, void* stream);
int sdumc_debug_marks(int on);
int sdumc_debug_marks_read(float* ms, int n);
/* Debug: the workspace plan of sdumc_net_forward as text lines "name offset length" (floats, relative to
 * sdumc_net_io.workspace); returns the text length, or minus the buffer size needed.  For probes that compare intermediate
 * tensors of two runs (tools/fwd_determinism_probe.py); not part of the data path. */
int32_t sdumc_debug_plan_table(const sdumc_net_dims* d, char* buf, size_t buflen);
/* Debug: the schedule the backward pass of a call with these dims and io (its context's options, its feature pointers) would take,
 * as text lines "name value": rc, chain, cluster, fra_fold, utterance, frame, dw_grouped, pool_grouped, early_one_launch,
 * flush1_after_pool, flush2_after_query, flush3_after_utt, then per modality (suffix _a / _t / _v) early, early_lane, ca_dw_grouped,
 * fra_dw_grouped, ca_dw_late, dw_on_lane3, dx_sum, frame_dw_grouped, frame_dw_skip, k1.  phases: 3 = sdumc_net_backward and
 * sdumc_train_step, 1 / 2 = sdumc_net_backward_phase 0 / 1; frozen_frame_dw: bit m = frame_dim_reshape_m frozen (the fused step).
 * Returns the text length, minus the buffer size needed, or 0 for arguments the call itself would refuse.  Launches nothing and
 * records no event; for tests that hold every route to the reference (tests/test_gpu_backward_routes.py). */
int32_t sdumc_debug_backward_schedule(const sdumc_net_dims* d, const sdumc_net_io* io, int32_t phases, uint32_t frozen_frame_dw,
                                      void* stream, char* buf, size_t buflen);
size_t sdumc_net_workspace_bytes(const sdumc_net_dims* d);
int sdumc_net_forward(const sdumc_net_dims* d, const sdumc_net_io* io, void* stream);

/* The attention maps of a completed EVAL-mode sdumc_net_forward, per frame and in STORE order (csrc/attn_export.hip).  The
 * reference returns the softmax-over-time weights of its six poolings per stream from both modules (vector_attention, model :68,
 * :95), collects them in forward (attention_masks, model :291) and carries the loop that plots them per utterance in its inference
 * script (main_frame_val_text_missing_inference.py:92, :125, :176-181).  The engine computes and normalises them in its workspace on
 * every route (pair / multi partial + combine; K3; the clustered stages' fold; fp32 and bf16 storage: the weights are fp32 in
 * both), so this entry only COPIES: it rebuilds the workspace plan from `d` (as sdumc_debug_plan_table), finds the weights inside
 * io->workspace and writes, for stream s, modality m, batch sample b and frame t < length[idx[b]], row start[idx[b]] + t of
 * dst[s][m]:
 *   column 0      the FRA2UTT_new weight of that frame
 *   columns 1..7  the seven Cross_Attention weights, in multi_query order (fused, at, tv, av, audio, text, video; model :332)
 * Frames t >= length (the collater's padding) are not exported; rows of utterances not in the batch are not touched; an idx outside
 * [0, n_utt) is skipped, never written.  ONE launch, plain 16-byte stores, 64-bit row addressing, no atomics: a repeated launch
 * gives the same bits.  No host synchronisation.
 * Ordering: stream-ordered behind the forward on `stream`; the workspace holds these weights only until the next forward into it,
 * so the call goes between forward i and forward i + 1 -- where sdumc_scatter_rows_multi goes.  Train-mode weights are computed under
 * dropout and are not what the reference plots: export after eval-mode forwards.
 * Semantics: without sdumc_net_io.lengths (the reference's behaviour) the softmax runs over the batch's PADDED length and the padded
 * frames take part, so an utterance's exported weights depend on the batch it was evaluated in and sum to at most 1 over its valid
 * frames -- what the reference's vector_attention[:, :len] would show.  With lengths (key padding) they sum to 1 and do not depend
 * on the batch.
 * SDUMC_EINVAL, before anything is launched: d / io / e / e->idx / io->workspace NULL; n_utt < 1; dims the engine refuses
 * (sdumc_net_workspace_bytes == 0); for a (stream, modality) the dims contain: a NULL start / length table or destination, a
 * destination not 16-byte aligned, dst_rows < 1; streams == 1 with a non-NULL dst[1][*].  SDUMC_ENOMEM: io->workspace_bytes below
 * sdumc_net_workspace_bytes(d). */
typedef struct sdumc_attn_export {
  const int64_t* idx;          /* device int64 [B]: the batch's index vector (as sdumc_gather_desc.idx) */
  const int64_t* start[4];     /* store-wide tables, device: first packed row of every utterance; audio, text, video, feat4 */
  const int32_t* length[4];    /* store-wide tables, device: frames of every utterance */
  int64_t n_utt;               /* utterances in the store (an idx outside [0, n_utt) is skipped, never written) */
  float* dst[2][3];            /* [stream][audio, text-slot, video]: [dst_rows, 8] fp32; stream 1's text slot is feat4 */
  int64_t dst_rows[2][3];      /* packed rows of that modality in the store (without the trailing zero row) */
} sdumc_attn_export;
int sdumc_net_export_attention(const sdumc_net_dims* d, const sdumc_net_io* io, const sdumc_attn_export* e, void* stream);

typedef struct sdumc_net_grads {
  const float* d_vals;        /* gradients w.r.t. the five outputs, same shapes; NULL = zero */
  const float* d_fused;
  const float* d_rnc;
  const float* d_text_hidden;
  const float* d_cross_text;
  float* grads;               /* [live count] flat gradient bucket; every live tensor is OVERWRITTEN
                                 (alignment padding is left untouched: allocate it zeroed) */
  /* Optional (all NULL / 0 = the call above: same launches, same bits): the gradients with respect to the INPUT FEATURES, i.e. the
   * backward of frame_dim_reshape_{0,1,2} (model :193-195, :282-284) through its input -- what autograd gives the reference for
   * model([audio, text, video, flag]) when a feature tensor requires grad: d_feat_m [B T_m, d_m] = dz_m [B T_m, 256] . W_m [256, d_m].
   * Each pointer independently; fp32, 16-byte aligned, OVERWRITTEN.  streams == 2: d_audio / d_video hold the SUM over both streams
   * (one tensor feeds both calls).  Without sdumc_net_io.lengths every row is computed (padded frames take part in the reference's
   * softmax and have a gradient there too); with lengths the rows t >= length are exact zeros (length 0: every row of the sample,
   * although the poolings treat such a sample as one frame long).  Row-mapped batches: the outputs are
   * padded [B, T, d] tensors all the same.  Widths that are multiples of 256 take sdumc_frame_dx, other widths the generic NN GEMM.
   * Written by sdumc_net_backward and by phase 1 of sdumc_net_backward_phase (phase 0 ignores the fields), each product on its
   * modality's lane once that modality's dz is final; sdumc_train_step and sdumc_loss_backward ignore the fields.
   * Before anything is enqueued (no fill, no fork; gradient bucket and outputs untouched): SDUMC_EINVAL for bf16 storage
   * (sdumc_net_dims.bf16 == 2) with any pointer set, for streams == 1 with d_text[1], for a misaligned output; SDUMC_ENOMEM for
   * feat_scratch NULL or below sdumc_net_feature_grad_scratch_bytes. */
  float* d_audio;             /* [B, Ta, da] */
  float* d_video;             /* [B, Tv, dv] */
  float* d_text[2];           /* [B, Tt[s], dt]: stream 0 = text, stream 1 = feat4 */
  void* feat_scratch;         /* the packed transposed frame weights (caller-owned: the workspace plan does not change) */
  size_t feat_scratch_bytes;
} sdumc_net_grads;
/* bytes of sdumc_net_grads.feat_scratch for `d` (never 0 for dims the engine takes); 0: dims the engine refuses, or bf16 storage */
size_t sdumc_net_feature_grad_scratch_bytes(const sdumc_net_dims* d);

/* loss.backward() through the network (main :149).  Needs the workspace of the matching forward. */
int sdumc_net_backward(const sdumc_net_dims* d, const sdumc_net_io* io, const sdumc_net_grads* g, void* stream);
/* The same in two calls, for a data-parallel step that overlaps its gradient all-reduce with the backward:
 * phase 0 = the utterance-level layers; when it returns (stream-ordered) grads[0, sdumc_param_early_count) are final.
 * phase 1 = the frame-level layers (input_proj of both attention sites, frame_dim_reshape: 0.9 of the 1.4 ms of
 * backward GEMM time at C2), which finish grads[early, live). */
int sdumc_net_backward_phase(const sdumc_net_dims* d, const sdumc_net_io* io, const sdumc_net_grads* g, int32_t phase,
                             void* stream);
int64_t sdumc_param_early_count(int32_t da, int32_t dt, int32_t dv);

/* Per-frame saliency of a completed feature-gradient backward, in STORE order (csrc/frame_saliency.hip): what a gradient-based
 * attribution of model.eval() (model :282-284 through :364) reduces sdumc_net_grads.d_audio / d_text / d_video to.  For a
 * descriptor's sample b < B and frame t < length[idx[b]] (and t < T), with g = grad[b, t, :] and x = that frame's feature row, row
 * start[idx[b]] + t of dst receives
 *   column 0   sum_c g[c] x[c]        (gradient x input, signed)
 *   column 1   sqrt(sum_c g[c]^2)     (gradient norm)
 * x is feat[b, t, :] of a padded [B, T, d] tensor, or -- with row_map, the int32 [B T] map the forward read the batch through
 * (sdumc_net_io.row_map) -- row row_map[b T + t] of the store's packed [store_rows, d] tensor; a map entry outside [0, store_rows)
 * is a zero row and is never read.  Frames t >= length are not written; rows of utterances not in the batch are not touched; an idx
 * outside [0, n_utt) or a destination row outside [0, dst_rows) is skipped, never written.
 * ONE launch for up to SDUMC_SALIENCY_MAX_DESCS descriptors (normally the three modalities of one stream) that share the batch's
 * index vector idx (device int64 [B]; every descriptor has the same B).
 * Arithmetic: the products of the fp32 values are formed in fp64 (exact there); every lane of the row's wave adds its strided
 * chunks (16 bytes when d % 4 == 0, one float otherwise) in index order into two fp64 accumulators; the 64 lanes combine in a fixed
 * butterfly; one fp64 square root for column 1; one rounding to fp32 per column; one 8-byte store per row.  No atomics, no state
 * between launches: a repeated launch gives the same bits, and the order of a row's sum depends on d alone -- the same grad and feat
 * rows give the same bits whatever batch, B, T or batch position they came in.  NaN / Inf in a row propagate to that row's two
 * values, and only to those.  One 64-lane wave per padded frame row on a capped grid, 64-bit element offsets, plain vector loads
 * and stores, no LDS.  Stream-ordered behind the backward that wrote grad; no host synchronisation.
 * SDUMC_EINVAL, before anything is launched: descs or idx NULL; n outside 1 .. SDUMC_SALIENCY_MAX_DESCS; a descriptor with grad,
 * feat, start, length or dst NULL, with B, T, d, n_utt or dst_rows < 1, with a B other than the first descriptor's, with a row_map
 * and store_rows < 1, with grad or dst not 16-byte aligned, or with feat not 16-byte aligned while d % 4 == 0; more than 2^31 - 1
 * padded rows in all. */
#define SDUMC_SALIENCY_MAX_DESCS 4
typedef struct sdumc_saliency_desc {
  const float* grad;         /* [B, T, d] fp32: the d_feat tensor the backward wrote; 16-byte aligned */
  const float* feat;         /* the features the forward read: padded [B, T, d], or with row_map the packed [store_rows, d] rows */
  const int32_t* row_map;    /* device int32 [B T], or NULL */
  int64_t store_rows;        /* rows of the packed tensor (read with row_map only) */
  const int64_t* start;      /* store-wide table, device [n_utt]: first packed row of every utterance of this modality */
  const int32_t* length;     /* store-wide table, device [n_utt]: frames of every utterance */
  int64_t n_utt;
  float* dst;                /* [dst_rows, 2] fp32, 16-byte aligned */
  int64_t dst_rows;          /* packed rows of that modality in the store (without the trailing zero row) */
  int32_t B, T, d;
} sdumc_saliency_desc;
int sdumc_frame_saliency(const sdumc_saliency_desc* descs, int32_t n, const int64_t* idx, void* stream);

/* sdumc_step_cfg.rates: the fused step's per-tensor learning-rate scale, decay scale and frozen flag, indexed by LIVE tensor in
 * sdumc_param_table order (entry i = the i-th line with live == 1).  The step turns it into sdumc_adam_step_rates' segment table
 * with the layout's own offsets. */
typedef struct sdumc_tensor_rates {
  int32_t n;                                /* the live tensor count of the step's dims */
  float lr_scale[SDUMC_RATES_MAX_SEGS];     /* finite, >= 0 */
  float wd_scale[SDUMC_RATES_MAX_SEGS];     /* finite, >= 0 */
  uint8_t frozen[SDUMC_RATES_MAX_SEGS];     /* != 0: torch's requires_grad = False */
} sdumc_tensor_rates;

/* Two-stream self-distillation step (main :119-150). */
typedef struct sdumc_step_cfg {
  float weights[6];      /* full_mse, missing_mse, text_feat, text_query_feat, features, rnc (main :234-239) */
  float temperature;     /* RnCLoss temperature = 2 (loss.py:272) */
  float beta1, beta2, eps, weight_decay;   /* Adam (main :317) */
  /* 0 (a zeroed struct) = the step as it always was, coupled L2, launch for launch; 1 = decoupled weight decay (sdumc_adamw_step,
   * which has the rule): the decoupled form of whichever last launch the step would have made -- Adam's, the rates launch, either
   * with the averaged weights -- with that launch's holds and scalar tail.  Anything else: SDUMC_EINVAL before the forward is
   * enqueued.  (In the four bytes that were padding between weight_decay and labels: no other field moves, sizeof stays.) */
  int32_t decoupled_decay;
  const float* labels;   /* [B] sentiment values of the local samples */
  float* adam_m;         /* [live count] */
  float* adam_v;         /* [live count] */
  float* hyper;          /* device float[4], see sdumc_adam_step */
  float* losses;         /* device float[8]: total, mse_full, mse_missing, rmse_text, rmse_query, rmse_fused, rnc, 0.
                            MSE entries are the LOCAL sum / B_global (sum over ranks = global value). */
  /* Gradient-norm clipping and the non-finite guard (sdumc_grad_guard, which see); all zero/NULL = the step without them, launch
   * for launch.  guard != NULL: between the backward and Adam, on the caller's stream, sdumc_grad_guard(bucket, live count,
   * clip_norm, skip_nonfinite, hyper, guard_scratch, guard) runs, and Adam applies nothing when it skipped the step (guard[3]):
   * parameters, moments and the step count hyper[1] stay as they were, while the dropout call counter advances by 2 and losses[0..6]
   * are written as for any step (losses[7] and a NaN total stay the cluster-failure signal alone).  SDUMC_EINVAL before the forward is
   * enqueued: clip_norm / skip_nonfinite / guard_scratch set while guard is NULL, and whatever sdumc_grad_guard refuses.
   * (The four sit here, in the middle: tests pin `distill` and the contrastive fields as the struct's tail.) */
  float clip_norm;       /* max_norm; <= 0: no clipping (the norm, the count and the guard are still computed) */
  int32_t skip_nonfinite;   /* 1: a bucket with a NaN or +-Inf element skips the step */
  float* guard;          /* device float[4]: L2 norm before clipping, clip coefficient, non-finite count, skipped (0 / 1) */
  void* guard_scratch;   /* sdumc_grad_guard_scratch_bytes(live count) bytes, 16-byte aligned */
  /* data-parallel exactness; all zero/NULL on one GPU */
  int32_t B_global;      /* 0 -> B */
  /* The criterion of the two regression terms (losses[1], losses[2], weights[0], weights[1]; main :137-138): SDUMC_REGRESS_MSE (0 =
   * a zeroed struct) the step as it always was, launch for launch and bit for bit; _L1, _HUBER (with regress_delta, the struct's
   * last four bytes) and _CCC as sdumc_reg_fwd_bwd has them, computed by the workgroups of the loss stage that held the MSE terms:
   * no further launch.  L1 / Huber entries are the LOCAL sum / B_global like the MSE entries.  SDUMC_EINVAL before a launch: a code
   * outside 0..3, a regress_delta that is not positive and finite under _HUBER (it is read by _HUBER alone), _CCC with B_global
   * set and different from B (its moments would need an exchange that is not built).
   * (In the four bytes that were padding between B_global and ssd_global, as regress_delta is in the four behind `distill`: no
   * other field moves and sizeof stays, which tests pin together with `distill` as the last declaration.) */
  int32_t regress;
  const float* ssd_global;       /* device float[3]: all-reduced sums of squared differences (text, query, fused) */
  const float* rnc_feats_global;  /* [2*B_global, 64] = cat(r_stream0 of all ranks, r_stream1 of all ranks) */
  const float* rnc_labels_global; /* [2*B_global] */
  /* Per-tensor learning rates, decay and frozen tensors (sdumc_adam_step_rates, which see); NULL = the step without them, launch
   * for launch.  A HOST pointer, read during the call.  Tensor i is updated with hyper[2] * lr_scale[i] and weight_decay *
   * wd_scale[i] by ONE launch in Adam's place, which carries Adam's holds (cluster failure, a skipped step) and its scalar tail.  A
   * frozen tensor keeps parameter and moments bit for bit, and its segment of the gradient bucket is +0.0f to everyone behind the
   * backward (sdumc_zero_segments, in front of sdumc_grad_guard): the guard's norm and whoever reads the bucket after the step.
   * frame_dim_reshape_m with weight AND bias frozen: modality m's frame dW is not computed at all; every other frozen tensor's
   * gradient is computed and then zeroed.  SDUMC_EINVAL before the forward is enqueued: n other than the live tensor count of the
   * dims, a scale that is negative, NaN or Inf.  (In the middle like the guard fields, which tests pin between `losses` and
   * `B_global`: behind the data-parallel pointers.) */
  const sdumc_tensor_rates* rates;
  /* Averaged weights (sdumc_adam_step_ema, which has the rule); ema NULL = the step without them, launch for launch, and ema_decay /
   * ema_warmup must then be zero.  ema: device float[live count], 16-byte aligned, not the parameters.  The EMA form of the step's
   * last launch (Adam's, or the rates launch with `rates`) runs in its place: no further launch, nothing on the host per step.  It
   * takes that launch's hold -- a step the guard skipped or the clustered kernels poisoned leaves the average bit for bit alone --
   * and with ema_warmup the weight follows the step count the guard left.  A frozen tensor's average is neither read nor written.
   * SDUMC_EINVAL before the forward is enqueued: a misaligned or aliasing ema, ema_decay outside [0, 1] or NaN, options without
   * ema.  (Directly behind `rates`, in front of the tail other tests pin.) */
  float* ema;
  float ema_decay;
  int32_t ema_warmup;
  int32_t rnc_row0[2];  /* rows of this rank's stream-0 / stream-1 features in the gathered matrix */
  /* The contrastive criterion over the [2B, 64] rnc rows (losses[6], weights[5]): SDUMC_CONTRAST_RNC (0 = a zeroed
   * struct) RnCLoss with `temperature`; SDUMC_CONTRAST_SUPCON SupConLoss (loss.py:143-240) with the two streams as the
   * two views of a sample, contrast_mode 'all', positives from `labels` (supcon_label_mode 0: equal labels, 1: equal
   * rintf(label)), supcon_temperature (> 0) and supcon_base_temperature (0 means 0.07).  The rows are L2-normalised
   * inside the kernel (the driver's Proj, main :61-69): on the raw rows the reference's SupConLoss is NaN, so there is
   * no un-normalised option here.  Anything else, or SUPCON together with rnc_feats_global (the data-parallel exchange
   * carries RnC records only): SDUMC_EINVAL before a launch.
   * (These four sit in front of `distill`, which stays the struct's last field; all zero = today's step.) */
  int32_t contrast;
  int32_t supcon_label_mode;
  float supcon_temperature;
  float supcon_base_temperature;
  /* The criterion of the three distillation pairs text_hidden, cross_text, fused (main :148 and its commented-out tail):
   * SDUMC_DISTILL_RMSE (0 = a zeroed struct) RMSELoss, _COSINE CosineSimilarityLoss4Seq, _KL KLLoss; anything else:
   * SDUMC_EINVAL before a launch.  losses[3..5] hold the chosen criterion's values.  Cosine and KL are sums over rows
   * divided by B_global: like the MSE entries, a data-parallel rank writes its LOCAL sum / B_global and ssd_global is
   * not read.
   * regress_delta: Huber's delta of `regress` (which see), in what was the struct's tail padding. */
  int32_t distill; float regress_delta;
} sdumc_step_cfg;
#define SDUMC_DISTILL_RMSE 0
#define SDUMC_DISTILL_COSINE 1
#define SDUMC_DISTILL_KL 2
#define SDUMC_CONTRAST_RNC 0
#define SDUMC_CONTRAST_SUPCON 1

size_t sdumc_loss_workspace_bytes(const sdumc_net_dims* d, int32_t B_global);
/* local sums of squared differences of the three RMSE pairs -> ssd_out float[3] (for the all-reduce) */
int sdumc_loss_ssd(const sdumc_net_dims* d, const sdumc_net_io* io, float* ssd_out, void* scratch,
                   size_t scratch_bytes, void* stream);
/* The data-parallel exactness exchange as ONE record per rank,
 *   record = [ rnc features of this rank, stream-major (2*B x rd) | labels (B) | sums of squares (3) ],  n = 2*B*rd + B + 3 floats,
 * so that one all-gather of W records replaces the three exchanges.  sdumc_dp_unpack turns the gathered [W, n] matrix into
 * what sdumc_step_cfg takes: feats [2*W*B, rd] = (stream-0 rows of rank 0..W-1, then stream-1 rows of rank 0..W-1),
 * labels2 [2*W*B] = the W*B labels twice, ssd[3] = the per-rank sums added in rank order (same bits on every rank).
 * The reference has no data-parallel path: the truth these reproduce is the single-process step on the
 * whole batch (main_frame_val_text_missing.py:119-150). */
int sdumc_dp_pack(const float* rnc, const float* labels, const float* ssd, int32_t B, int32_t rd, float* record,
                  void* stream);
/* sdumc_loss_ssd + sdumc_dp_pack in one launch: the three sums of squares (text_hidden, cross_text, fused: rows [B, 2B)
 * minus rows [0, B) of each [2B, .] output) are reduced in a fixed order by the last block to finish.  `workspace`
 * (>= sdumc_dp_record_workspace_bytes(B), 4-byte aligned) must be ZERO before the first call; every call leaves it
 * ready for the next. */
size_t sdumc_dp_record_workspace_bytes(int32_t B);
int sdumc_dp_record(int32_t B, int32_t rd, const float* text_hidden, const float* cross_text, const float* fused,
                    const float* rnc, const float* labels, float* record, void* workspace, void* stream);
int sdumc_dp_unpack(const float* records, int32_t W, int32_t B, int32_t rd, float* feats, float* labels2, float* ssd,
                    void* stream);
/* loss values + gradients w.r.t. the five network outputs (written to the d_* buffers of `g`,
 * which here are OUTPUTS and must all be non-NULL) */
int sdumc_loss_backward(const sdumc_net_dims* d, const sdumc_net_io* io, const sdumc_step_cfg* cfg,
                        const sdumc_net_grads* g, void* scratch, size_t scratch_bytes, void* stream);
/* ... with the distillation targets of a stored teacher (sdumc_teacher; NULL, or no table: sdumc_loss_backward launch for launch) */
int sdumc_loss_backward_teacher(const sdumc_net_dims* d, const sdumc_net_io* io, const sdumc_step_cfg* cfg,
                                const sdumc_net_grads* g, const sdumc_teacher* teacher, void* scratch, size_t scratch_bytes,
                                void* stream);

/* forward (both streams) + losses + backward + Adam on one GPU.  workspace >= sdumc_step_workspace_bytes. */
size_t sdumc_step_workspace_bytes(const sdumc_net_dims* d);
int sdumc_train_step(const sdumc_net_dims* d, const sdumc_net_io* io, const sdumc_step_cfg* cfg, void* stream);
/* The same step with the distillation targets of a stored teacher: no further launch, the loss stage's kernels read the tables
 * through teacher->idx.  sdumc_step_cfg is full, so the teacher travels beside it.  teacher NULL, or no table: sdumc_train_step. */
int sdumc_train_step_teacher(const sdumc_net_dims* d, const sdumc_net_io* io, const sdumc_step_cfg* cfg,
                             const sdumc_teacher* teacher, void* stream);
/* byte offset of the flat gradient bucket inside the sdumc_train_step workspace (tests, DP all-reduce) */
size_t sdumc_step_grads_offset(const sdumc_net_dims* d);

#ifdef __cplusplus
}
#endif
#endif /* SDUMC_HIP_H */
