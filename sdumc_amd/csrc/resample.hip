// resample.hip — temporal pre-compression of a device-resident packed feature tensor (sdumc_pool_frames): the reference's
// func_mapping_feature (toolkit/utils/read_data.py:120-137) for every utterance of a modality in one HBM-bound pass, beside
// sdumc_p3_split and sdumc_gather_batch.  Plain vector loads and stores; no atomics, no LDS.
#include "common.h"

namespace {

// One wave per destination ROW at a time (its owner -- utterance, pool, padding -- is resolved once per row with wave-uniform
// reads of the four tables), one 16-byte chunk per lane, lanes striding the row by 64 chunks; waves stride over the rows on a
// capped grid.  Row [dst_rows] is the tensor's trailing all-zero row.  E = elements per chunk (4 fp32 or 8 bf16), each summed in
// fp64 in frame order; the loads of four frames are issued before they are added (utt mode pools hundreds of frames per row).
template <bool BF16>
__global__ __launch_bounds__(256) void pool_frames_kernel(const sdumc_pool_desc p) {
  constexpr int E = BF16 ? 8 : 4;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t chunks = p.cols / E;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const uint4* const src = static_cast<const uint4*>(p.src);
  uint4* const dst = static_cast<uint4*>(p.dst);
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row <= p.dst_rows; row += nwaves) {
    int64_t f0 = 0, f1 = 0;      // source ROWS [f0, f1) of this destination row's pool (empty: a zero row)
    int pool = 1;
    bool padded = true;          // the pool holds a frame index outside the utterance: +0 joins the sum
    if (row < p.dst_rows) {
      int a = 0, b = p.n_utts;   // the last utterance whose first destination row is <= row
      while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (p.dst_start[m] <= row) a = m; else b = m;
      }
      const int64_t j = row - p.dst_start[a];
      const int64_t L = p.src_len[a], n = p.dst_len[a];
      if (j >= 0 && j < n && L > 0) {
        int64_t pad = 0;
        if (L > n) {
          const int64_t q = L / n, r = L - q * n;
          pool = (int)(r ? q + 1 : q);
          pad = r ? n - r : 0;
        }
        const int64_t t0 = j * pool - pad, t1 = t0 + pool;      // frames of the utterance, before clipping to [0, L)
        padded = t0 < 0 || t1 > L;
        const int64_t c0 = t0 < 0 ? 0 : t0, c1 = t1 > L ? L : t1, s = p.src_start[a];
        if (c1 > c0 && s >= 0 && s + c1 <= p.src_rows) f0 = s + c0, f1 = s + c1;
        else padded = true;
      }
    }
    const double den = (double)pool;
    for (int64_t c = lane; c < chunks; c += 64) {
      double acc[E];
#pragma unroll
      for (int k = 0; k < E; ++k) acc[k] = -0.0;      // the additive identity: -0.0 + x == x for every x, -0.0 included
      const uint4* s = src + f0 * chunks + c;
      int64_t left = f1 - f0;
      auto add = [&](const uint4& v) {
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (BF16) {
            acc[2 * k] += (double)__uint_as_float(w[k] << 16);
            acc[2 * k + 1] += (double)__uint_as_float(w[k] & 0xffff0000u);
          } else {
            acc[k] += (double)__uint_as_float(w[k]);
          }
        }
      };
      for (; left >= 4; left -= 4, s += 4 * chunks) {
        const uint4 v0 = s[0], v1 = s[chunks], v2 = s[2 * chunks], v3 = s[3 * chunks];
        add(v0); add(v1); add(v2); add(v3);
      }
      for (; left > 0; --left, s += chunks) add(*s);
      unsigned o[4];
      float f[E];
#pragma unroll
      for (int k = 0; k < E; ++k) {
        if (padded) acc[k] += 0.0;
        f[k] = (float)(acc[k] / den);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (BF16) {
          typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
          const bf16x2 h = {(__bf16)f[2 * k], (__bf16)f[2 * k + 1]};
          o[k] = *reinterpret_cast<const unsigned*>(&h);
        } else {
          o[k] = __float_as_uint(f[k]);
        }
      }
      dst[row * chunks + c] = uint4{o[0], o[1], o[2], o[3]};
    }
  }
}

}  // namespace

extern "C" int sdumc_pool_frames(const sdumc_pool_desc* p, int32_t max_workgroups, void* stream) {
  if (!p || !p->src || !p->dst || !p->src_start || !p->src_len || !p->dst_start || !p->dst_len) return SDUMC_EINVAL;
  if (p->bf16 != 0 && p->bf16 != 1) return SDUMC_EINVAL;
  if (p->cols < 1 || p->cols % (p->bf16 ? 8 : 4)) return SDUMC_EINVAL;
  if (p->n_utts < 1 || p->src_rows < 1 || p->dst_rows < 1 || max_workgroups < 0) return SDUMC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(p->src) | reinterpret_cast<uintptr_t>(p->dst)) & 15) return SDUMC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(p->src_start) | reinterpret_cast<uintptr_t>(p->dst_start)) & 7) return SDUMC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(p->src_len) | reinterpret_cast<uintptr_t>(p->dst_len)) & 3) return SDUMC_EINVAL;
  int64_t blocks = (p->dst_rows + 1 + 3) / 4;      // one wave per row (+ the zero row)
  const int64_t cap = max_workgroups > 0 ? max_workgroups : 2048;
  if (blocks > cap) blocks = cap;
  if (p->bf16)
    hipLaunchKernelGGL(pool_frames_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), *p);
  else
    hipLaunchKernelGGL(pool_frames_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), *p);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

SDUMC_PRELOAD_HOOK(resample)      // (common.h)
