// tensor_norms.hip — sdumc_tensor_norms: the L2 norm and the non-finite count of every tensor of a segment table {x, y, count} in two
// launches, and with a rolling snapshot y the norm of x - y too, y taking x's values in the same pass (include/sdumc_hip.h has the
// contract).  What a training epoch keeps per step and tensor (FusedTrainer.train_epoch(by_tensor=...)): the gradient bucket cut at
// ParamLayout's offsets, and the flat parameters against their values before the step.
// HBM-bound: x is read once (15 MB for a C2 bucket), y is read once and written once.  The sums are reproducible the way
// epoch_record.hip's are: the host cuts every segment into chunks by its COUNT alone (never across two segments, never by an
// address), a workgroup folds one chunk -- every thread its elements in a fixed order into fp64 accumulators, the 256 threads by a
// fixed LDS tree -- into one partial in the caller's scratch, and the second launch (one workgroup per segment) adds the segment's
// partials in INDEX order, takes the root and rounds once to fp32.  Plain loads and stores, no atomics: the launch boundary orders
// the partials.  The table travels in the kernel arguments, every lookup is a scalar load with a wave-uniform index.
// 16 bytes per lane from a chunk's first 16-byte aligned element on (x and y must then sit alike within 16 bytes), the <= 3 elements
// in front of it and the <= 3 behind the last whole quad one per lane; a segment whose y sits otherwise goes one float per lane.
#include <string.h>

#include "common.h"

namespace {

constexpr int NT = 256;                         // threads per workgroup
constexpr int UNROLL = 8;                       // quads (or single floats) a thread has in flight per operand
constexpr int64_t CHUNK = (int64_t)NT * UNROLL * 4;      // floats of a chunk while a segment has fewer than MAX_CHUNKS of them
constexpr int64_t MAX_CHUNKS = 1024;            // chunks per segment: beyond CHUNK * MAX_CHUNKS floats the chunks grow instead
constexpr int MAXS = SDUMC_TENSOR_NORMS_MAX_SEGS;

struct NormArgs {
  sdumc_norm_seg seg[MAXS];
  uint32_t chunk_end[MAXS];        // running sum of the segments' chunk counts
  int32_t n, any_y;
  double* part_sum;                // [chunks] sums of x^2
  double* part_diff;               // [chunks] sums of (x - y)^2
  uint32_t* part_bad;              // [chunks] counts of non-finite x
  float* norm;
  int32_t* nonfinite;
  float* diff_norm;
};
static_assert(sizeof(NormArgs) + 64 <= 4096, "the table travels in the kernel arguments (4 KB)");

// a segment's chunks: a function of its count alone
inline int64_t chunks_of(int64_t count) { return std::min<int64_t>(MAX_CHUNKS, std::max<int64_t>(1, (count + CHUNK - 1) / CHUNK)); }
__host__ __device__ inline int64_t chunk_floats(int64_t count, int64_t nch) { return ((count + nch - 1) / nch + 3) & ~(int64_t)3; }

template <bool Y>
__device__ __forceinline__ void take(float x, float y, double& acc, double& dacc, uint32_t& bad) {
  sumsq_count_nonfinite(x, acc, bad);
  if (Y) {
    const double d = (double)x - (double)y;      // (exact in fp64)
    dacc = fma(d, d, dacc);
  }
}

// elements [lo, hi) of one segment; VEC: x + lo and y + lo sit alike within 16 bytes
template <bool VEC, bool Y>
__device__ __forceinline__ void fold_chunk(const float* __restrict__ x, float* __restrict__ y, int64_t lo, int64_t hi, int t, double& acc,
                                           double& dacc, uint32_t& bad) {
  if (VEC) {
    const int64_t alo = min(hi, lo + (int64_t)((4 - ((reinterpret_cast<uintptr_t>(x + lo) >> 2) & 3)) & 3));
    const int64_t nq = (hi - alo) >> 2, ahi = alo + 4 * nq;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x + alo);
    f32x4* y4 = reinterpret_cast<f32x4*>(y + alo);
    for (int64_t i = t; i < nq; i += (int64_t)NT * UNROLL) {
      f32x4 v[UNROLL], w[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t k = i + (int64_t)u * NT;
        v[u] = w[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (k < nq) {
          v[u] = x4[k];
          if (Y) w[u] = y4[k];
        }
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
#pragma unroll
        for (int j = 0; j < 4; ++j) take<Y>(v[u][j], w[u][j], acc, dacc, bad);      // (a quad past nq adds exact zeros)
        if (Y && i + (int64_t)u * NT < nq) y4[i + (int64_t)u * NT] = v[u];
      }
    }
    // the elements in front of the first whole quad and behind the last one: at most 3 each, one per lane
    int64_t e = -1;
    if (t < alo - lo) e = lo + t;
    else if (t >= 4 && t - 4 < hi - ahi) e = ahi + (t - 4);
    if (e >= 0) {
      const float xv = x[e];
      take<Y>(xv, Y ? y[e] : 0.f, acc, dacc, bad);
      if (Y) y[e] = xv;
    }
  } else {
    for (int64_t i = lo + t; i < hi; i += (int64_t)NT * UNROLL) {
      float v[UNROLL], w[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t k = i + (int64_t)u * NT;
        v[u] = w[u] = 0.f;
        if (k < hi) {
          v[u] = x[k];
          if (Y) w[u] = y[k];
        }
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        take<Y>(v[u], w[u], acc, dacc, bad);
        if (Y && i + (int64_t)u * NT < hi) y[i + (int64_t)u * NT] = v[u];
      }
    }
  }
}

__global__ __launch_bounds__(NT) void tensor_norms_kernel(const NormArgs a) {
  __shared__ double s_sum[NT];
  __shared__ double s_diff[NT];
  __shared__ uint32_t s_bad[NT];
  const int t = threadIdx.x;
  const uint32_t bid = blockIdx.x;
  int s = 0;
  for (int hi = a.n - 1; s < hi;) {      // the first segment whose chunk_end is beyond this workgroup
    const int mid = (s + hi) >> 1;
    if (bid >= a.chunk_end[mid]) s = mid + 1;
    else hi = mid;
  }
  const uint32_t c0 = s ? a.chunk_end[s - 1] : 0u;
  const int64_t count = a.seg[s].count;
  const float* x = a.seg[s].x;
  float* y = a.seg[s].y;
  const int64_t fpc = chunk_floats(count, (int64_t)(a.chunk_end[s] - c0));
  const int64_t lo = min(count, (int64_t)(bid - c0) * fpc), hi = min(count, lo + fpc);
  double acc = 0.0, dacc = 0.0;
  uint32_t bad = 0;
  if (!y) fold_chunk<true, false>(x, nullptr, lo, hi, t, acc, dacc, bad);
  else if (((reinterpret_cast<uintptr_t>(x) ^ reinterpret_cast<uintptr_t>(y)) & 15) == 0) fold_chunk<true, true>(x, y, lo, hi, t, acc, dacc, bad);
  else fold_chunk<false, true>(x, y, lo, hi, t, acc, dacc, bad);
  s_sum[t] = acc;
  s_diff[t] = dacc;
  s_bad[t] = bad;
  __syncthreads();
#pragma unroll
  for (int k = NT / 2; k > 0; k >>= 1) {
    if (t < k) {
      s_sum[t] += s_sum[t + k];
      s_diff[t] += s_diff[t + k];
      s_bad[t] += s_bad[t + k];
    }
    __syncthreads();
  }
  if (t == 0) {
    a.part_sum[bid] = s_sum[0];
    a.part_diff[bid] = s_diff[0];
    a.part_bad[bid] = s_bad[0];
  }
}

// workgroup s: segment s's partials in index order (staged through LDS NT at a time, added by one thread), one rounding to fp32
__global__ __launch_bounds__(NT) void tensor_norms_final_kernel(const NormArgs a) {
  __shared__ double s_sum[NT];
  __shared__ double s_diff[NT];
  __shared__ uint32_t s_bad[NT];
  const int t = threadIdx.x, s = blockIdx.x;
  const uint32_t c0 = s ? a.chunk_end[s - 1] : 0u, c1 = a.chunk_end[s];
  double sum = 0.0, dsum = 0.0;
  uint64_t cnt = 0;
  for (uint32_t base = c0; base < c1; base += NT) {
    if (base + t < c1) {
      s_sum[t] = a.part_sum[base + t];
      s_diff[t] = a.part_diff[base + t];
      s_bad[t] = a.part_bad[base + t];
    }
    __syncthreads();
    if (t == 0) {
      const int m = (int)min((uint32_t)NT, c1 - base);
      for (int k = 0; k < m; ++k) {
        sum += s_sum[k];
        dsum += s_diff[k];
        cnt += s_bad[k];
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    a.norm[s] = (float)sqrt(sum);
    a.nonfinite[s] = (int32_t)min(cnt, (uint64_t)0x7fffffff);
    if (a.seg[s].y) a.diff_norm[s] = (float)sqrt(dsum);
  }
}

// the table as the kernels take it; < 0: a table the entry refuses, else the number of chunks
int64_t fill_table(NormArgs& a, const sdumc_norm_seg* segs, int32_t n) {
  if (!segs || (reinterpret_cast<uintptr_t>(segs) & 7) || n < 1 || n > MAXS) return -1;
  memset(&a, 0, sizeof(a));
  uint32_t chunks = 0;
  for (int32_t i = 0; i < MAXS; ++i) {
    if (i < n) {
      const sdumc_norm_seg& s = segs[i];
      if (s.count < 0 || (!s.x && s.count > 0)) return -1;
      if ((reinterpret_cast<uintptr_t>(s.x) | reinterpret_cast<uintptr_t>(s.y)) & 3) return -1;
      a.seg[i] = s;
      if (s.count == 0) a.seg[i].y = nullptr;      // (nothing to compare or to copy: diff_norm[i] stays as it is)
      if (a.seg[i].y) a.any_y = 1;
      chunks += (uint32_t)chunks_of(s.count);
    }
    a.chunk_end[i] = chunks;
  }
  a.n = n;
  return chunks;
}

inline size_t scratch_bytes_of(int64_t chunks) { return ((size_t)chunks * 20 + 15) & ~(size_t)15; }

}  // namespace

extern "C" size_t sdumc_tensor_norms_scratch_bytes(const sdumc_norm_seg* segs, int32_t n) {
  NormArgs a;
  const int64_t chunks = fill_table(a, segs, n);
  return chunks < 0 ? 0 : scratch_bytes_of(chunks);
}

extern "C" int sdumc_tensor_norms(const sdumc_norm_seg* segs, int32_t n, float* norm, int32_t* nonfinite, float* diff_norm,
                                  void* scratch, size_t scratch_bytes, void* stream) {
  NormArgs a;
  const int64_t chunks = fill_table(a, segs, n);
  if (chunks < 0 || !norm || !nonfinite || !scratch) return SDUMC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(norm) | reinterpret_cast<uintptr_t>(nonfinite) | reinterpret_cast<uintptr_t>(diff_norm)) & 3) return SDUMC_EINVAL;
  if (a.any_y && !diff_norm) return SDUMC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(scratch) & 15) || scratch_bytes < scratch_bytes_of(chunks)) return SDUMC_EINVAL;
  a.part_sum = reinterpret_cast<double*>(scratch);
  a.part_diff = a.part_sum + chunks;
  a.part_bad = reinterpret_cast<uint32_t*>(a.part_diff + chunks);
  a.norm = norm;
  a.nonfinite = nonfinite;
  a.diff_norm = diff_norm;
  hipLaunchKernelGGL(tensor_norms_kernel, dim3((unsigned)chunks), dim3(NT), 0, as_stream(stream), a);
  SDUMC_CHECK_LAUNCH();
  hipLaunchKernelGGL(tensor_norms_final_kernel, dim3((unsigned)n), dim3(NT), 0, as_stream(stream), a);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

SDUMC_PRELOAD_HOOK(tensor_norms)      // (common.h)
