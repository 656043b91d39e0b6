// frame_dx.hip -- the input-feature gradient of the frame projections frame_dim_reshape_{0,1,2} (model :193-195, :282-284), gfx950:
//   C[M, N] = A[M, 256] . W[256, N]      A = dz, the gradient w.r.t. the projected frames; W = the projection's weight as stored
// the backward of the wide-tile frame projections, in the same arithmetic: an fp32 value is the exact sum of three bf16 values, the six
// largest of the nine part products go through v_mfma_f32_32x32x16_bf16 with fp32 accumulation (gemm_group.hip has the arithmetic and
// its error bound, sdumc_hip.h the contract at the edges).
//
// Form: A-STATIONARY.  K is 256, all of it: a 64-row tile of dz is read once as fp32, split into its three bf16 planes by the
// workgroup itself and kept in LDS for the whole launch (64 rows x 256 k x 3 planes x 2 bytes = 96 KB, laid out as the k-tiles of
// p3_loop.h's ring: rows of 96 bytes per 16 k, the two 48-byte k-halves swapped by bit 3 of the row).  dz is produced a few launches
// earlier and read by nobody else in this form, so a split pass of its own (sdumc_p3_split: 1.5 KB written and read again per row)
// would only add traffic; the split costs a workgroup 8 split8 per thread.  The weight is needed k-major per OUTPUT column -- W
// transposed -- and is packed once per call into the fragment-major P3 layout of W^T [N][256] (sdumc_p3_split_frag_t): a wave's MFMA
// operand of a k-tile is three contiguous KiB that go straight to registers, three k-tiles ahead, and never touch LDS (only the wave
// that owns the 32 output columns multiplies them).  A workgroup of 8 waves walks `cpw` consecutive 256-column blocks with its tile of
// dz; wave w owns columns [32 w, 32 w + 32) of each.  The output (the 224 MB of a C2 backward) leaves the accumulators directly:
// a half-wave writes 32 consecutive floats of one row, a full 128-byte line.
// No atomics, no split of K, one fixed summation order: a repeated launch gives the same bits.
#include <algorithm>
#include <cstring>

#include "p3_loop.h"

namespace sdumc_fdx {
using namespace sdumc_p3;

constexpr int K = 256, NKT = K / BK, BM = 64, NTHR = 512;
[[maybe_unused]] constexpr int TM = BM / 32;
constexpr int KT_BYTES = BM * ROWB;                      // one k-tile of the row tile: 6 KB
constexpr int A_LDS = NKT * KT_BYTES;                    // 96 KB
constexpr int LDS_BYTES = A_LDS + BM * 4;                // + one keep flag per row
[[maybe_unused]] constexpr int BLK_BYTES = NKT * FRAG_KT;                 // a 32-column block of the packed weight: 48 KB

struct Args {
  const float* A;
  const char* Wf;
  float* C;
  int64_t ldc;
  const int32_t* lengths;
  int32_t M, T, ncb, cpw;      // ncb = N / 256 column blocks, cpw of them per workgroup
};

__global__ __launch_bounds__(NTHR, 1) void frame_dx_kernel(const Args a) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int m0 = blockIdx.x * BM;
  const int cb0 = blockIdx.y * a.cpw, cb1 = min(cb0 + a.cpw, a.ncb);
  int32_t* keep = reinterpret_cast<int32_t*>(lds + A_LDS);

  // ---- this wave's weight fragments of the first three k-tiles are requested before anything else ----
  auto bblock = [&](int cb) { return a.Wf + (size_t)(cb * 8 + wave) * (size_t)BLK_BYTES + lane * 16; };
  const char* bcur = bblock(cb0);
  u32x4 pb[NBS][3];
#pragma unroll
  for (int t = 0; t < DB; ++t)
#pragma unroll
    for (int p = 0; p < 3; ++p) pb[t][p] = *reinterpret_cast<const u32x4*>(bcur + t * FRAG_KT + p * 1024);

  // ---- the row tile of dz: fp32 -> three bf16 planes, once, into LDS (rows past M repeat row M - 1; they are never stored) ----
  for (int u = tid; u < BM * (K / 8); u += NTHR) {
    const int row = u >> 5, c = u & 31;      // a thread: 8 consecutive k of a row; 32 threads read a row's KiB
    const float* s = a.A + (size_t)min(m0 + row, a.M - 1) * K + 8 * c;
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(s), a1 = *reinterpret_cast<const f32x4*>(s + 4);
    const float v[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    u32x4 pl[3];
    split8(v, pl);
    char* d = lds + (c >> 1) * KT_BYTES + row * ROWB + (((c & 1) ^ ((row >> 3) & 1)) * 48);
    *reinterpret_cast<u32x4*>(d) = pl[0];
    *reinterpret_cast<u32x4*>(d + 16) = pl[1];
    *reinterpret_cast<u32x4*>(d + 32) = pl[2];
  }
  if (tid < BM) {      // rows at or past their sample's length are written as +0.0f, whatever dz holds there
    const int row = m0 + tid;
    int k = row < a.M ? 1 : 0;
    if (k && a.lengths) {
      const int b = row / a.T, t = row - b * a.T;
      k = t < a.lengths[b] ? 1 : 0;
    }
    keep[tid] = k;
  }
  __syncthreads();

  const int lane_off = li * ROWB + ((lh ^ ((li >> 3) & 1)) * 48);
  auto op = [](const u32x4& v) { return __builtin_bit_cast(bf16x8, v); };
  for (int cb = cb0; cb < cb1; ++cb) {
    const char* bnext = bblock(min(cb + 1, cb1 - 1));      // (the last block requests three k-tiles of itself again: in bounds, unused)
    // two accumulators per output tile: the leading products a0 b0 (exact in fp32) in one, the five correction terms -- 2^-8 of them
    // and below -- in the other, added once at the end.  The rounding of an accumulation is half an ulp of the ACCUMULATOR: with all
    // 96 MFMAs of K = 256 on one accumulator the error is the random walk of 96 such roundings at the result's magnitude (measured
    // 5.3e-7 of the largest entry against fp64, 2.7x the fp32-MFMA route's); this way 16 of them are, the other 80 are 2^-8 smaller
    f32x16 acc[TM], lo[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) { acc[i][e] = 0.f; lo[i][e] = 0.f; }
    // four k-tiles per trip (the four register sets of B); the trips are not unrolled, so that the weight fragments in flight stay
    // the three k-tiles asked for and the compiler does not hoist a whole column block's 192 registers of loads
#pragma unroll 1
    for (int kq = 0; kq < NKT; kq += NBS) {
#pragma unroll
      for (int j = 0; j < NBS; ++j) {
        const int kt = kq + j;
        const char* src = kt + DB < NKT ? bcur + (kt + DB) * FRAG_KT : bnext + (kt + DB - NKT) * FRAG_KT;
#pragma unroll
        for (int p = 0; p < 3; ++p) pb[(j + DB) % NBS][p] = *reinterpret_cast<const u32x4*>(src + p * 1024);
        u32x4 pa[TM][3];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int p = 0; p < 3; ++p) pa[i][p] = *reinterpret_cast<const u32x4*>(lds + kt * KT_BYTES + i * 32 * ROWB + lane_off + p * 16);
        // smallest terms first, as in p3_loop.h (prims.h: BF16X3_TA / _TB): the first five into `lo`, (a0 b0) into `acc`
#pragma unroll
        for (int t = 0; t < 5; ++t)
#pragma unroll
          for (int i = 0; i < TM; ++i)
            lo[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(op(pa[i][BF16X3_TA[t]]), op(pb[j][BF16X3_TB[t]]), lo[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TM; ++i)
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(op(pa[i][BF16X3_TA[5]]), op(pb[j][BF16X3_TB[5]]), acc[i], 0, 0, 0);
      }
    }
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    const int col = cb * BN + wave * 32 + li;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = 32 * i + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (m0 + r < a.M) a.C[(size_t)(m0 + r) * (size_t)a.ldc + col] = keep[r] ? acc[i][e] + lo[i][e] : 0.f;
      }
    bcur = bnext;
  }
#endif
}

// W [K][N] (row stride ld) -> the fragment-major P3 layout of W^T [N][K]: block (rb, kt), lane (li, lh) holds W[16 kt + 8 lh .. + 7][32 rb + li].
// One thread per (8 k, column): the 32 lanes of a half-wave read 32 consecutive columns of a row of W.
__global__ __launch_bounds__(256) void p3_split_frag_t_kernel(const float* __restrict__ src, int64_t ld, char* __restrict__ dst, int rows_k, int cols_n) {
  const int kc = rows_k >> 3;
  const int64_t total = (int64_t)kc * cols_n;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const int c = (int)(u / cols_n), n = (int)(u - (int64_t)c * cols_n);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = src[(int64_t)(8 * c + j) * ld + n];
    u32x4 pl[3];
    split8(v, pl);
    const int rb = n >> 5, li = n & 31, kt = c >> 1, lh = c & 1;
    char* d = dst + ((int64_t)rb * (rows_k >> 4) + kt) * FRAG_KT + (lh * 32 + li) * 16;
    *reinterpret_cast<u32x4*>(d) = pl[0];
    *reinterpret_cast<u32x4*>(d + 1024) = pl[1];
    *reinterpret_cast<u32x4*>(d + 2048) = pl[2];
  }
}

// rows b T + t with t >= lengths[b] of C [M][N] := +0.0f (behind the fp32-MFMA route and the engine's generic widths); N % 4 == 0 takes
// 16-byte stores
__global__ __launch_bounds__(256) void zero_rows_kernel(float* __restrict__ C, int64_t ldc, int M, int N, const int32_t* __restrict__ lengths, int T) {
  const int row = blockIdx.x;
  if (row >= M) return;
  const int b = row / T, t = row - b * T;
  if (t < lengths[b]) return;
  float* d = C + (size_t)row * (size_t)ldc;
  if (((N | ldc) & 3) == 0 && (reinterpret_cast<uintptr_t>(C) & 15) == 0) {
    for (int c = threadIdx.x * 4; c < N; c += 1024) *reinterpret_cast<f32x4*>(d + c) = f32x4{0.f, 0.f, 0.f, 0.f};
  } else {
    for (int c = threadIdx.x; c < N; c += 256) d[c] = 0.f;
  }
}

// column blocks per workgroup: fewest rounds of 256 workgroups, each round costing its prologue (the tile of dz: read, split, barrier
// -- about a quarter of one column block's MFMA time) plus its column blocks
inline int blocks_per_workgroup(int M, int ncb) {
  const long tiles_m = (M + BM - 1) / BM;
  int best = 1;
  double best_cost = 1e30;
  for (int cpw = 1; cpw <= ncb; ++cpw) {
    const long groups = (ncb + cpw - 1) / cpw;
    if (groups > 65535) continue;
    const long rounds = (tiles_m * groups + 255) / 256;
    const double cost = (double)rounds * (0.25 + cpw);
    if (cost < best_cost - 1e-9) { best_cost = cost; best = cpw; }
  }
  return best;
}

bool prepare() {
  static sdumc_dev_once attr_set;
  return sdumc_once_per_device(attr_set, [] { return sdumc_set_dyn_lds(&frame_dx_kernel, LDS_BYTES); }) == SDUMC_OK;
}

}  // namespace sdumc_fdx

extern "C" size_t sdumc_frame_dx_scratch_bytes(int32_t N) {
  if (N < 256 || (N % 256)) return 0;
  return (size_t)6 * sdumc_fdx::K * (size_t)N;
}

extern "C" int sdumc_frame_dx_prepare_(void) { return sdumc_fdx::prepare() ? SDUMC_OK : SDUMC_ELAUNCH; }

extern "C" int sdumc_p3_split_frag_t(const float* src, int64_t ld, void* dst, int32_t K, int32_t N, void* stream) {
  if (!src || !dst || K <= 0 || N <= 0 || (K & 15) || (N & 31) || ld < N) return SDUMC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) return SDUMC_EINVAL;
  const int64_t units = (int64_t)(K >> 3) * N;
  const unsigned blocks = (unsigned)std::min<int64_t>((units + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(sdumc_fdx::p3_split_frag_t_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), src, ld, static_cast<char*>(dst), (int)K, (int)N);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_zero_padded_rows_(float* C, int64_t ldc, int32_t M, int32_t N, const int32_t* lengths, int32_t T, void* stream) {
  if (!C || !lengths || M < 1 || N < 1 || ldc < N || T < 1 || (M % T)) return SDUMC_EINVAL;
  hipLaunchKernelGGL(sdumc_fdx::zero_rows_kernel, dim3((unsigned)M), dim3(256), 0, as_stream(stream), C, ldc, (int)M, (int)N, lengths, (int)T);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_frame_dx(const sdumc_frame_dx_t* p, void* stream) {
  using namespace sdumc_fdx;
  if (!p) return SDUMC_EINVAL;
  if (!p->A || !p->C || (!p->W && !p->W_frag)) return SDUMC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(p->A) | reinterpret_cast<uintptr_t>(p->W) | reinterpret_cast<uintptr_t>(p->W_frag) | reinterpret_cast<uintptr_t>(p->C) |
       reinterpret_cast<uintptr_t>(p->scratch)) & 15)
    return SDUMC_EINVAL;
  if (p->M < 1 || p->N < 256 || (p->N % 256) || p->ldc < p->N || (p->ldc & 3)) return SDUMC_EINVAL;
  if (p->W && (p->ldw < p->N || (p->ldw & 3))) return SDUMC_EINVAL;
  if (p->lengths && ((reinterpret_cast<uintptr_t>(p->lengths) & 3) || p->T < 1 || (p->M % p->T))) return SDUMC_EINVAL;
  const bool split = sdumc_split_on_(SDUMC_SPLIT_WIDE) != 0;
  if (!split && (!p->W || p->ldw > 0x7FFFFFFF || p->ldc > 0x7FFFFFFF)) return SDUMC_EINVAL;      // (the fp32-MFMA route reads W as stored)
  if (split && !p->W_frag && (!p->scratch || p->scratch_bytes < sdumc_frame_dx_scratch_bytes(p->N))) return SDUMC_ENOMEM;
  if (!split) {
    sdumc_gemm g;
    memset(&g, 0, sizeof(g));
    g.layout = SDUMC_NN;
    g.M = p->M; g.N = p->N; g.K = K;
    g.groups = 1;
    g.A[0] = p->A; g.lda = K;
    g.B[0] = p->W; g.ldb = (int32_t)p->ldw;
    g.C[0] = p->C; g.ldc = (int32_t)p->ldc;
    g.splitk = 1;
    const int rc = sdumc_gemm_f32(&g, stream);
    if (rc != SDUMC_OK) return rc;
    return p->lengths ? sdumc_zero_padded_rows_(p->C, p->ldc, p->M, p->N, p->lengths, p->T, stream) : SDUMC_OK;
  }
  if (!prepare()) return SDUMC_ELAUNCH;
  const void* wf = p->W_frag;
  if (!wf) {
    const int rc = sdumc_p3_split_frag_t(p->W, p->ldw, p->scratch, K, p->N, stream);
    if (rc != SDUMC_OK) return rc;
    wf = p->scratch;
  }
  Args a;
  a.A = p->A;
  a.Wf = static_cast<const char*>(wf);
  a.C = p->C;
  a.ldc = p->ldc;
  a.lengths = p->lengths;
  a.M = p->M;
  a.T = p->lengths ? p->T : 1;
  a.ncb = p->N / BN;
  a.cpw = blocks_per_workgroup(p->M, a.ncb);
  const dim3 grid((unsigned)((p->M + BM - 1) / BM), (unsigned)((a.ncb + a.cpw - 1) / a.cpw));
  hipLaunchKernelGGL(frame_dx_kernel, grid, dim3(NTHR), LDS_BYTES, as_stream(stream), a);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

SDUMC_PRELOAD_HOOK(frame_dx)      // (common.h)
