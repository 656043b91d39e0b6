// grad_guard.hip — sdumc_grad_guard / sdumc_grad_guard_multi: global-norm gradient clipping and the non-finite step guard, on the
// device, in three launches and without a host synchronisation (include/sdumc_hip.h has the contract).
//   1. reduce    every workgroup folds one chunk of the gradients into an fp64 sum of squares and a count of NaN / +-Inf elements
//   2. finalize  one workgroup adds the partials in INDEX order and writes guard = {norm, coef, count, skipped}; a skipped step takes
//                the Adam step count back (hyper[1] -= 1: the fused step advanced it in its loss launch, before a gradient existed)
//   3. scale     g = g * coef in place, ONE fp32 multiply per element; every workgroup reads guard first and leaves without touching
//                the gradients when coef == 1 or the step is skipped
// The reduce is the one of tensor_norms.hip (no snapshot): the host cuts every segment into chunks by its COUNT alone, a thread walks
// its elements in a fixed order, the 256 threads fold by a fixed LDS tree, the partials are added in index order -- the same input
// gives the same bits on every call, wherever it lies.  Plain loads and stores, no atomics, no communication between workgroups: the
// launch boundaries order partials and guard.  The device code is repeated here instead of shared through a header so that
// tensor_norms.hip and epoch_record.hip compile to what they compiled to before.
// 16 bytes per lane from a chunk's first 16-byte aligned element on, the <= 3 elements in front of it and the <= 3 behind the last
// whole quad one per lane: nothing but 4-byte alignment is assumed.  The scale launch walks the same chunks.
// Adam is untouched by the clip: it reads the scaled bucket with the expression it always had (adam.hip), so a clipped step is bit
// for bit "multiply the bucket by guard[1], then today's Adam".
#include <math.h>
#include <string.h>

#include "common.h"

namespace {

constexpr int NT = 256;                         // threads per workgroup
constexpr int UNROLL = 8;                       // quads a thread has in flight
constexpr int64_t CHUNK = (int64_t)NT * UNROLL * 4;      // floats of a chunk while a segment has fewer than MAX_CHUNKS of them
constexpr int64_t MAX_CHUNKS = 1024;            // chunks per segment: beyond CHUNK * MAX_CHUNKS floats the chunks grow instead
constexpr int MAXS = SDUMC_TENSOR_NORMS_MAX_SEGS;

struct GuardArgs {
  float* x[MAXS];
  int64_t count[MAXS];
  uint32_t chunk_end[MAXS];        // running sum of the segments' chunk counts
  int32_t n, skip_nonfinite;
  uint32_t chunks;
  float max_norm;
  double* part_sum;                // [chunks] sums of squares
  uint32_t* part_bad;              // [chunks] counts of non-finite elements
  float* hyper;                    // optional: the fused step's Adam state
  float* guard;                    // float[4]
};
static_assert(sizeof(GuardArgs) + 64 <= 4096, "the table travels in the kernel arguments (4 KB)");

// a segment's chunks: a function of its count alone
inline int64_t chunks_of(int64_t count) { return std::min<int64_t>(MAX_CHUNKS, std::max<int64_t>(1, (count + CHUNK - 1) / CHUNK)); }
__host__ __device__ inline int64_t chunk_floats(int64_t count, int64_t nch) { return ((count + nch - 1) / nch + 3) & ~(int64_t)3; }

// workgroup bid's chunk: its segment's base and the elements [lo, hi) of it
__device__ __forceinline__ float* chunk_of(const GuardArgs& a, uint32_t bid, int64_t& lo, int64_t& hi) {
  int s = 0;
  for (int top = a.n - 1; s < top;) {      // the first segment whose chunk_end is beyond this workgroup
    const int mid = (s + top) >> 1;
    if (bid >= a.chunk_end[mid]) s = mid + 1;
    else top = mid;
  }
  const uint32_t c0 = s ? a.chunk_end[s - 1] : 0u;
  const int64_t count = a.count[s];
  const int64_t fpc = chunk_floats(count, (int64_t)(a.chunk_end[s] - c0));
  lo = min(count, (int64_t)(bid - c0) * fpc);
  hi = min(count, lo + fpc);
  return a.x[s];
}

// [lo, alo) in front of the first whole quad, nq quads from alo on, [ahi, hi) behind the last one
__device__ __forceinline__ void split_chunk(const float* x, int64_t lo, int64_t hi, int64_t& alo, int64_t& nq, int64_t& ahi) {
  alo = min(hi, lo + (int64_t)((4 - ((reinterpret_cast<uintptr_t>(x + lo) >> 2) & 3)) & 3));
  nq = (hi - alo) >> 2;
  ahi = alo + 4 * nq;
}

__global__ __launch_bounds__(NT) void grad_guard_reduce_kernel(const GuardArgs a) {
  __shared__ double s_sum[NT];
  __shared__ uint32_t s_bad[NT];
  const int t = threadIdx.x;
  const uint32_t bid = blockIdx.x;
  int64_t lo, hi, alo, nq, ahi;
  const float* x = chunk_of(a, bid, lo, hi);
  split_chunk(x, lo, hi, alo, nq, ahi);
  double acc = 0.0;
  uint32_t bad = 0;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x + alo);
  for (int64_t i = t; i < nq; i += (int64_t)NT * UNROLL) {
    f32x4 v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t k = i + (int64_t)u * NT;
      v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (k < nq) v[u] = x4[k];
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) sumsq_count_nonfinite(v[u][j], acc, bad);      // (a quad past nq adds exact zeros)
  }
  // the elements in front of the first whole quad and behind the last one: at most 3 each, one per lane
  int64_t e = -1;
  if (t < alo - lo) e = lo + t;
  else if (t >= 4 && t - 4 < hi - ahi) e = ahi + (t - 4);
  if (e >= 0) sumsq_count_nonfinite(x[e], acc, bad);
  s_sum[t] = acc;
  s_bad[t] = bad;
  __syncthreads();
#pragma unroll
  for (int k = NT / 2; k > 0; k >>= 1) {
    if (t < k) {
      s_sum[t] += s_sum[t + k];
      s_bad[t] += s_bad[t + k];
    }
    __syncthreads();
  }
  if (t == 0) {
    a.part_sum[bid] = s_sum[0];
    a.part_bad[bid] = s_bad[0];
  }
}

// ONE workgroup: all partials in index order (staged through LDS NT at a time, added by one thread), then the four guard values
__global__ __launch_bounds__(NT) void grad_guard_final_kernel(const GuardArgs a) {
  __shared__ double s_sum[NT];
  __shared__ uint32_t s_bad[NT];
  const int t = threadIdx.x;
  double sum = 0.0;
  uint64_t cnt = 0;
  for (uint32_t base = 0; base < a.chunks; base += NT) {
    if (base + t < a.chunks) {
      s_sum[t] = a.part_sum[base + t];
      s_bad[t] = a.part_bad[base + t];
    }
    __syncthreads();
    if (t == 0) {
      const int m = (int)min((uint32_t)NT, a.chunks - base);
      for (int k = 0; k < m; ++k) {
        sum += s_sum[k];
        cnt += s_bad[k];
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    const double norm = sqrt(sum);
    // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1), in double, rounded once; a NaN norm gives a NaN
    // coefficient as it does there.  max_norm <= 0: no clipping
    double coef = 1.0;
    if (a.max_norm > 0.f) {
      const double c = (double)a.max_norm / (norm + 1e-6);
      coef = c < 1.0 ? c : (c != c ? c : 1.0);
    }
    const bool skipped = a.skip_nonfinite != 0 && cnt > 0;
    a.guard[0] = (float)norm;
    a.guard[1] = (float)coef;
    a.guard[2] = (float)cnt;      // (exact below 2^24)
    a.guard[3] = skipped ? 1.f : 0.f;
    // the step count as before the step; hyper[2..3] derive from it and are rewritten by the next step's advance before any reader
    if (skipped && a.hyper) a.hyper[1] -= 1.f;
  }
}

__global__ __launch_bounds__(NT) void grad_guard_scale_kernel(const GuardArgs a) {
  const float coef = a.guard[1];
  if (coef == 1.f || a.guard[3] != 0.f) return;      // (wave-uniform: nothing of the gradients is read or written)
  const int t = threadIdx.x;
  int64_t lo, hi, alo, nq, ahi;
  float* x = chunk_of(a, blockIdx.x, lo, hi);
  split_chunk(x, lo, hi, alo, nq, ahi);
  f32x4* x4 = reinterpret_cast<f32x4*>(x + alo);
  for (int64_t i = t; i < nq; i += (int64_t)NT * UNROLL) {
    f32x4 v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t k = i + (int64_t)u * NT;
      if (k < nq) v[u] = x4[k];
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t k = i + (int64_t)u * NT;
      if (k < nq) {
        f32x4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = v[u][j] * coef;
        x4[k] = w;
      }
    }
  }
  int64_t e = -1;
  if (t < alo - lo) e = lo + t;
  else if (t >= 4 && t - 4 < hi - ahi) e = ahi + (t - 4);
  if (e >= 0) x[e] = x[e] * coef;
}

inline size_t scratch_bytes_of(int64_t chunks) { return ((size_t)chunks * 12 + 15) & ~(size_t)15; }

// the table as the kernels take it; < 0: a table the entries refuse, else the number of chunks
int64_t fill_table(GuardArgs& a, const sdumc_norm_seg* segs, int32_t n) {
  if (!segs || (reinterpret_cast<uintptr_t>(segs) & 7) || n < 1 || n > MAXS) return -1;
  memset(&a, 0, sizeof(a));
  uint32_t chunks = 0;
  for (int32_t i = 0; i < MAXS; ++i) {
    if (i < n) {
      const sdumc_norm_seg& s = segs[i];
      if (s.count < 0 || (!s.x && s.count > 0) || s.y) return -1;
      if (reinterpret_cast<uintptr_t>(s.x) & 3) return -1;
      a.x[i] = const_cast<float*>(s.x);
      a.count[i] = s.count;
      chunks += (uint32_t)chunks_of(s.count);
    }
    a.chunk_end[i] = chunks;
  }
  a.n = n;
  a.chunks = chunks;
  return chunks;
}

int launch(GuardArgs& a, void* scratch, void* stream) {
  a.part_sum = reinterpret_cast<double*>(scratch);
  a.part_bad = reinterpret_cast<uint32_t*>(a.part_sum + a.chunks);
  hipLaunchKernelGGL(grad_guard_reduce_kernel, dim3(a.chunks), dim3(NT), 0, as_stream(stream), a);
  SDUMC_CHECK_LAUNCH();
  hipLaunchKernelGGL(grad_guard_final_kernel, dim3(1), dim3(NT), 0, as_stream(stream), a);
  SDUMC_CHECK_LAUNCH();
  hipLaunchKernelGGL(grad_guard_scale_kernel, dim3(a.chunks), dim3(NT), 0, as_stream(stream), a);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

}  // namespace

extern "C" size_t sdumc_grad_guard_scratch_bytes(int64_t n) {
  if (n < 1) return 0;
  return scratch_bytes_of(chunks_of(n));
}

// what sdumc_grad_guard refuses, without a launch (sdumc_train_step asks before its forward is enqueued)
extern "C" int sdumc_grad_guard_check_(const float* grads, int64_t n, float max_norm, int32_t skip_nonfinite, const float* hyper,
                                       const void* scratch, const float* guard) {
  if (!grads || n < 1 || !scratch || !guard) return SDUMC_EINVAL;
  if (max_norm != max_norm || (skip_nonfinite != 0 && skip_nonfinite != 1)) return SDUMC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(hyper) | reinterpret_cast<uintptr_t>(guard)) & 3) return SDUMC_EINVAL;
  if (reinterpret_cast<uintptr_t>(scratch) & 15) return SDUMC_EINVAL;
  return SDUMC_OK;
}

extern "C" int sdumc_grad_guard(float* grads, int64_t n, float max_norm, int32_t skip_nonfinite, float* hyper, void* scratch,
                                float* guard, void* stream) {
  const int rc = sdumc_grad_guard_check_(grads, n, max_norm, skip_nonfinite, hyper, scratch, guard);
  if (rc) return rc;
  const sdumc_norm_seg seg{grads, nullptr, n};
  GuardArgs a;
  if (fill_table(a, &seg, 1) < 0) return SDUMC_EINVAL;
  a.max_norm = max_norm;
  a.skip_nonfinite = skip_nonfinite;
  a.hyper = hyper;
  a.guard = guard;
  return launch(a, scratch, stream);
}

extern "C" size_t sdumc_grad_guard_multi_scratch_bytes(const sdumc_norm_seg* segs, int32_t nseg) {
  GuardArgs a;
  const int64_t chunks = fill_table(a, segs, nseg);
  return chunks < 0 ? 0 : scratch_bytes_of(chunks);
}

extern "C" int sdumc_grad_guard_multi(const sdumc_norm_seg* segs, int32_t nseg, float max_norm, void* scratch, size_t scratch_bytes,
                                      float* guard, void* stream) {
  GuardArgs a;
  const int64_t chunks = fill_table(a, segs, nseg);
  if (chunks < 0 || !scratch || !guard || max_norm != max_norm) return SDUMC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(guard) & 3) || (reinterpret_cast<uintptr_t>(scratch) & 15)) return SDUMC_EINVAL;
  if (scratch_bytes < scratch_bytes_of(chunks)) return SDUMC_ENOMEM;
  a.max_norm = max_norm;
  a.guard = guard;
  return launch(a, scratch, stream);
}

SDUMC_PRELOAD_HOOK(grad_guard)      // (common.h)
