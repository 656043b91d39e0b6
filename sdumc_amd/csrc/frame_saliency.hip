// frame_saliency.hip — sdumc_frame_saliency: the per-frame reduction of an input-feature gradient (sdumc_net_grads.d_audio / d_text /
// d_video of an eval-mode backward seeded with d_vals) against the features the forward read, into store-ordered [rows, 2] tensors:
// column 0 = sum_c g[c] x[c] (gradient x input), column 1 = sqrt(sum_c g[c]^2) (gradient norm).  include/sdumc_hip.h has the contract.
// HBM-bound: two streams of B T d floats in, 8 bytes per frame out.  Plain vector loads and stores; no atomics, no LDS.
#include <string.h>

#include "common.h"

namespace {

constexpr int MAXD = SDUMC_SALIENCY_MAX_DESCS;

struct SaliencyArgs {
  sdumc_saliency_desc p[MAXD];
  int64_t row_end[MAXD];      // running sum of B * T over the descriptors
  const int64_t* idx;
  int32_t n;
};

__device__ __forceinline__ void acc4(double& dot, double& sq, const f32x4& g, const f32x4& x) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {      // (the products are exact in fp64: an fma rounds once, like the product and the add would)
    const double gd = (double)g[k];
    dot = fma(gd, (double)x[k], dot);
    sq = fma(gd, gd, sq);
  }
}

// One wave per padded frame ROW at a time: its descriptor, sample, utterance and destination row are resolved once per row with
// wave-uniform reads (idx, the two store tables, the row map), then the lanes stride the row -- one 16-byte chunk of both operands per
// lane and step when VEC (d % 4 == 0: every row starts 16-byte aligned), one float otherwise.  The loads of up to four chunks of both
// operands are issued before they are consumed.  Each lane adds its chunks in index order into two fp64 accumulators; the 64 lanes
// combine in a fixed butterfly (xor 32, 16, 8, 4, 2, 1), so the order of a row's sum depends on d alone.  Waves stride the rows on a
// capped grid; rows t >= length, an idx outside the store and a destination row outside dst are skipped before anything is loaded.
template <bool VEC>
__device__ __forceinline__ void row_sums(const float* __restrict__ g, const float* __restrict__ x, int d, int lane, double& dot, double& sq) {
  dot = 0.0;
  sq = 0.0;
  if (VEC) {
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int chunks = d >> 2;
    int c = lane;
    for (; c + 192 < chunks; c += 256) {
      const f32x4 g0 = g4[c], g1 = g4[c + 64], g2 = g4[c + 128], g3 = g4[c + 192];
      const f32x4 x0 = x ? x4[c] : zero, x1 = x ? x4[c + 64] : zero, x2 = x ? x4[c + 128] : zero, x3 = x ? x4[c + 192] : zero;
      acc4(dot, sq, g0, x0);
      acc4(dot, sq, g1, x1);
      acc4(dot, sq, g2, x2);
      acc4(dot, sq, g3, x3);
    }
    for (; c + 64 < chunks; c += 128) {
      const f32x4 g0 = g4[c], g1 = g4[c + 64];
      const f32x4 x0 = x ? x4[c] : zero, x1 = x ? x4[c + 64] : zero;
      acc4(dot, sq, g0, x0);
      acc4(dot, sq, g1, x1);
    }
    for (; c < chunks; c += 64) acc4(dot, sq, g4[c], x ? x4[c] : zero);
  } else {
    int c = lane;
    for (; c + 64 < d; c += 128) {
      const float g0 = g[c], g1 = g[c + 64];
      const float x0 = x ? x[c] : 0.f, x1 = x ? x[c + 64] : 0.f;
      dot = fma((double)g0, (double)x0, dot);
      sq = fma((double)g0, (double)g0, sq);
      dot = fma((double)g1, (double)x1, dot);
      sq = fma((double)g1, (double)g1, sq);
    }
    for (; c < d; c += 64) {
      const float g0 = g[c], x0 = x ? x[c] : 0.f;
      dot = fma((double)g0, (double)x0, dot);
      sq = fma((double)g0, (double)g0, sq);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {      // (a + b == b + a bit for bit: every lane ends with the same two sums)
    dot += __shfl_xor(dot, o, 64);
    sq += __shfl_xor(sq, o, 64);
  }
}

__global__ __launch_bounds__(256) void frame_saliency_kernel(const SaliencyArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const int64_t total = a.row_end[a.n - 1];
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < total; row += nwaves) {
    int k = 0;
    while (k < a.n - 1 && row >= a.row_end[k]) ++k;
    const sdumc_saliency_desc& p = a.p[k];
    const int64_t local = row - (k ? a.row_end[k - 1] : 0);      // = b * T + t (below 2^31: checked by the entry)
    const int b = (int)((uint32_t)local / (uint32_t)p.T), t = (int)((uint32_t)local - (uint32_t)b * (uint32_t)p.T);
    const int64_t e = a.idx[b];
    if ((uint64_t)e >= (uint64_t)p.n_utt) continue;
    if (t >= p.length[e]) continue;
    const int64_t out = p.start[e] + t;
    if ((uint64_t)out >= (uint64_t)p.dst_rows) continue;
    const float* g = p.grad + local * p.d;
    const float* x = p.feat + local * p.d;
    if (p.row_map) {      // (an entry outside the packed tensor: a zero row, never read)
      const int64_t r = p.row_map[local];
      x = (uint64_t)r < (uint64_t)p.store_rows ? p.feat + r * p.d : nullptr;
    }
    double dot, sq;
    if ((p.d & 3) == 0) row_sums<true>(g, x, p.d, lane, dot, sq);
    else row_sums<false>(g, x, p.d, lane, dot, sq);
    if (lane == 0) {
      const float2 v = {(float)dot, (float)sqrt(sq)};
      *reinterpret_cast<float2*>(p.dst + out * 2) = v;
    }
  }
}

}  // namespace

extern "C" int sdumc_frame_saliency(const sdumc_saliency_desc* descs, int32_t n, const int64_t* idx, void* stream) {
  if (!descs || !idx || n < 1 || n > MAXD) return SDUMC_EINVAL;
  SaliencyArgs a;
  memset(&a, 0, sizeof(a));
  int64_t rows = 0;
  for (int k = 0; k < n; ++k) {
    const sdumc_saliency_desc& p = descs[k];
    if (!p.grad || !p.feat || !p.start || !p.length || !p.dst) return SDUMC_EINVAL;
    if (p.B < 1 || p.T < 1 || p.d < 1 || p.n_utt < 1 || p.dst_rows < 1) return SDUMC_EINVAL;
    if (p.B != descs[0].B) return SDUMC_EINVAL;      // (one idx vector names the samples of every descriptor)
    if (p.row_map && p.store_rows < 1) return SDUMC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(p.grad) | reinterpret_cast<uintptr_t>(p.dst)) & 15) return SDUMC_EINVAL;
    if (p.d % 4 == 0 && (reinterpret_cast<uintptr_t>(p.feat) & 15)) return SDUMC_EINVAL;
    a.p[k] = p;
    rows += (int64_t)p.B * p.T;
    a.row_end[k] = rows;
  }
  if (rows > 0x7FFFFFFF) return SDUMC_EINVAL;
  a.idx = idx;
  a.n = n;
  int64_t blocks = (rows + 3) / 4;      // one wave per padded frame row
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(frame_saliency_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

SDUMC_PRELOAD_HOOK(frame_saliency)      // (common.h)
