// loss.hip — the loss reductions of the self-distillation step, value + gradient.
//   MSELoss   toolkit/utils/loss.py:19-33   sum((p-t)^2)/len(p)
//   RMSELoss  toolkit/utils/loss.py:37-51   sqrt(mean((a-b)^2))   (split: ssd, then sqrt -> DP-exact)
//   RnCLoss   toolkit/utils/loss.py:271-315 Rank-N-Contrast; the boolean neg_mask (loss.py:303) is
//             evaluated with the same fp32 operations as the reference, so membership is bit-exact.
//   CosineSimilarityLoss4Seq  toolkit/utils/loss.py:100-119   sum over groups of mean over rows of 1 - cos
//   KLLoss    toolkit/utils/loss.py:74-97   (KL(softmax b || softmax a) + KL(softmax a || softmax b)) / 2, batchmean
//   CELoss    toolkit/utils/loss.py:6-16    log_softmax + NLL, summed, / len
// All sums run in a fixed order (no float atomics): results are bitwise reproducible.
#include "common.h"

namespace {

__device__ __forceinline__ float block_sum_256(float v, float* red /*[4]*/) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void mse_kernel(const float* pred, const float* target, int rows, float denom,
                                                  float weight, float* loss_out, float* dpred) {
  __shared__ float red[4];
  float acc = 0.f;
  const float inv = 1.f / denom;
  for (int i = threadIdx.x; i < rows; i += 256) {
    const float d = pred[i] - target[i];
    acc += d * d;
    if (dpred) dpred[i] = weight * 2.f * d * inv;
  }
  const float s = block_sum_256(acc, red);
  if (threadIdx.x == 0) *loss_out = s * inv;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double block_sum_256_d(double v, double* red /*[4]*/) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// ---- the regression criterion of main :137-138 beside MSELoss (SDUMC_REGRESS_*): one helper per criterion, the element's term
// and its gradient before the weight and 1 / denom.  d = pred - target in fp32.  The gradient expressions hold no addition (no
// contraction can change them): a fp32 host expression reproduces them bit for bit.
__device__ __forceinline__ float reg_sign(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : (d == d ? 0.f : d)); }   // sign(0) = 0, NaN stays NaN
// torch.nn.L1Loss: |d|, sign(d)
__device__ __forceinline__ void l1_elem(float d, float& h, float& g) {
  h = fabsf(d);
  g = reg_sign(d);
}
// torch.nn.HuberLoss(delta): 0.5 d^2, d inside |d| <= delta; delta (|d| - 0.5 delta), delta sign(d) outside (a NaN d compares false:
// the outer forms, which keep it)
__device__ __forceinline__ void huber_elem(float d, float delta, float& h, float& g) {
  const float ad = fabsf(d);
  if (ad <= delta) {
    h = 0.5f * d * d;
    g = d;
  } else {
    h = delta * (ad - 0.5f * delta);
    g = delta * reg_sign(d);
  }
}
// Concordance correlation coefficient, 1 - 2 s_py / (s_pp + s_yy + (m_p - m_y)^2) with population moments over the n elements: a
// whole-stream quantity, so the ONE workgroup that owns the stream makes two passes with double accumulators (the means, then the
// centred sums: thread-strided partials, wave reduce, the four wave sums in index order) and a third for the gradient, each
// element's in double, rounded to fp32 once and then multiplied by the weight.  No special cases: D == 0 is 0/0 = NaN; n = 1 gives
// value 1 and gradient +0 (0.0 - x negates like -x except that it turns -0 into +0).
__device__ __forceinline__ void ccc_stream(const float* p, const float* y, int n, float w, float* loss_out, float* dp) {
  __shared__ double red[4];
  double sp = 0.0, sy = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    sp += (double)p[i];
    sy += (double)y[i];
  }
  sp = block_sum_256_d(sp, red);
  sy = block_sum_256_d(sy, red);
  const double nn = (double)n, mp = sp / nn, my = sy / nn;
  double spp = 0.0, syy = 0.0, spy = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double a = (double)p[i] - mp, b = (double)y[i] - my;
    spp += a * a;
    syy += b * b;
    spy += a * b;
  }
  spp = block_sum_256_d(spp, red) / nn;
  syy = block_sum_256_d(syy, red) / nn;
  spy = block_sum_256_d(spy, red) / nn;
  const double dm = mp - my;
  const double D = spp + syy + dm * dm, N = 2.0 * spy;
  if (threadIdx.x == 0) *loss_out = (float)(1.0 - N / D);
  if (!dp) return;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double dN = 2.0 * ((double)y[i] - my) / nn;
    const double dD = 2.0 * ((double)p[i] - mp) / nn + 2.0 * dm / nn;
    const double g = 0.0 - (dN * D - N * dD) / (D * D);
    dp[i] = w * (float)g;
  }
}
// One stream of `rows` elements under criterion reg != MSE, by one workgroup of 256: value -> *loss_out, weight * gradient -> dpred
// (may be null).  L1 / Huber sum in fp32 in the order and with the helper of the MSE form; their value is the LOCAL sum / denom.
__device__ __forceinline__ void reg_stream(int reg, float delta, const float* pred, const float* target, int rows, float denom,
                                           float weight, float* loss_out, float* dpred, float* red /*[4]*/) {
  if (reg == SDUMC_REGRESS_CCC) {
    ccc_stream(pred, target, rows, weight, loss_out, dpred);
    return;
  }
  const float inv = 1.f / denom;
  float acc = 0.f;
  for (int i = threadIdx.x; i < rows; i += 256) {
    const float d = pred[i] - target[i];
    float h, g;
    if (reg == SDUMC_REGRESS_L1) l1_elem(d, h, g);
    else huber_elem(d, delta, h, g);
    acc += h;
    if (dpred) dpred[i] = (weight * g) * inv;
  }
  const float s = block_sum_256(acc, red);
  if (threadIdx.x == 0) *loss_out = s * inv;
}
__global__ __launch_bounds__(256) void reg_kernel(int reg, float delta, const float* pred, const float* target, int rows, float denom,
                                                  float weight, float* loss_out, float* dpred) {
  __shared__ float red[4];
  reg_stream(reg, delta, pred, target, rows, denom, weight, loss_out, dpred, red);
}

constexpr int SSD_CHUNK = 8192;
__global__ __launch_bounds__(256) void ssd_stage1(const float* a, const float* b, int64_t n, float* part) {
  __shared__ float red[4];
  const int64_t i0 = (int64_t)blockIdx.x * SSD_CHUNK, i1 = min(n, i0 + SSD_CHUNK);
  float acc = 0.f;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const float d = a[i] - b[i];
    acc += d * d;
  }
  const float s = block_sum_256(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void ssd_stage2(const float* part, int nchunk, float* out) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nchunk; i += 256) acc += part[i];
  const float s = block_sum_256(acc, red);
  if (threadIdx.x == 0) *out = s;
}

__global__ void rmse_bwd_kernel(const float* a, const float* b, int64_t n, const float* ssd, float inv_numel,
                                float weight, float* loss_out, float* da, int da_acc, float* db, int db_acc) {
  const float rmse = sqrtf(*ssd * inv_numel);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && loss_out) *loss_out = rmse;
  if (i >= n) return;
  // d sqrt(mean)/da = (a-b) / (numel * rmse)   (0/0 -> NaN exactly like torch's sqrt backward)
  const float g = weight * (a[i] - b[i]) * inv_numel / rmse;
  if (da) da[i] = da_acc ? da[i] + g : g;
  if (db) db[i] = db_acc ? db[i] - g : -g;
}

// ---------------------------------------------------------------------------------------------
// Rank-N-Contrast.  Workspace layout (floats): dist[n*n] e[n*n] ldiff[n*n] invD[n*n] G[n*n]
// rowmax[n] rowloss[n]
// ---------------------------------------------------------------------------------------------
struct RncWs {
  float *dist, *e, *ldiff, *invD, *G, *rowmax, *rowloss;
};
__host__ __device__ inline RncWs rnc_ws(float* w, int n) {
  RncWs r;
  const size_t nn = (size_t)n * n;
  r.dist = w;
  r.e = w + nn;
  r.ldiff = w + 2 * nn;
  r.invD = w + 3 * nn;
  r.G = w + 4 * nn;
  r.rowmax = w + 5 * nn;
  r.rowloss = r.rowmax + n;
  return r;
}

__device__ __forceinline__ void rnc_loss_body(int n, RncWs w, float* loss_out) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) acc += w.rowloss[i];
  const float s = block_sum_256(acc, red);
  if (threadIdx.x == 0) *loss_out = -s / ((float)n * (float)(n - 1));
}
__global__ __launch_bounds__(256) void rnc_loss_kernel(int n, RncWs w, float* loss_out) { rnc_loss_body(n, w, loss_out); }

// Measurement builds only (-DSDUMC_LOSS_DBG=1, off in the shipped library): thread 0 of workgroup 0 stamps the phases of rnc_row_body
// (slots 0-5: entry | anchor row in LDS | distances | exp | row loss | G) and of rnc_dfeat_body (8-11: entry | coef in LDS | sums |
// df written) with the 100 MHz wall clock; sdumc_loss_stamps_ copies the sixteen slots out (tools/loss_stamps.py).
#ifndef SDUMC_LOSS_DBG
#define SDUMC_LOSS_DBG 0
#endif
#if SDUMC_LOSS_DBG
__device__ unsigned long long g_loss_stamps[16];
#define LTR_INIT(wg) const bool ltr_on = (wg) == 0 && threadIdx.x == 0
#define LTR(k) do { if (ltr_on) g_loss_stamps[k] = wall_clock64(); } while (0)
#else
#define LTR_INIT(wg)
#define LTR(k)
#endif

constexpr int RNC_HEADQ = 16;   // row quads requested in rnc_row_body's head: 64 channels, the model's RnC width

// sum over q = 0 .. n-1, ascending, of (q != i && pred) ? b[q] : 0 with pred = a[q] >= x (A_GE) or x >= a[q]; a and b in LDS, every
// lane reading the same address.  Both arrays are read unconditionally, sixteen bytes at a time where they are aligned, and the term is
// a select: with b[q] inside the condition each step was two dependent LDS round trips (a[q], the compare, then b[q] under its mask)
// and the two loops of rnc_row_body were 16 of loss_stage1_kernel's 20 us at n = 128.  An excluded term adds 0.f, as it always did.
template <bool A_GE>
__device__ __forceinline__ float rnc_masked_sum(const float* a, const float* b, const float x, const int n, const int i, const bool al4) {
  float sum = 0.f;
  int q = 0;
  if (al4) {
#pragma unroll 4
    for (; q + 4 <= n; q += 4) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(a + q), bv = *reinterpret_cast<const f32x4*>(b + q);
#pragma unroll
      for (int c = 0; c < 4; ++c) sum += (q + c != i && (A_GE ? av[c] >= x : x >= av[c])) ? bv[c] : 0.f;
    }
  }
#pragma unroll 8
  for (; q < n; ++q) {
    const float av = a[q], bv = b[q];
    sum += (q != i && (A_GE ? av >= x : x >= av)) ? bv : 0.f;
  }
  return sum;
}

// One workgroup per anchor i, everything that depends on row i only: distances, label differences, exp,
// the masked denominators D_ik, the row's loss and G_i* = dLoss/dlogit_i*.  labels: y[j] = labels[j % label_mod]
// when label_mod > 0 (the reference's labels.repeat(2, 1), loss.py:283, without materialising it).
__device__ __forceinline__ void rnc_row_body(const float* f, const float* labels, int label_mod, int n, int dim, float inv_t,
                                             RncWs w, int want_grad, const int i, float* sm /* fi[dim] | ld[n] | ee[n] | dd[n] | thr[n] | iD[n] */) {
  __shared__ float red[4];
  float* fi = sm;
  float* ld = fi + ((dim + 3) & ~3);
  float* ee = ld + n;
  float* dd = ee + n;
  float* thr = dd + n;
  float* iD = thr + n;
  const int tid = threadIdx.x;
  const bool vec = (dim & 3) == 0 && (reinterpret_cast<uintptr_t>(f) & 15) == 0;
  const int nq = dim >> 2;   // 16-byte quads of a row (vector form only)
  const bool hfull = vec && nq >= RNC_HEADQ;
  // Head: every load whose address is known at the first instruction goes out before the first wait -- the anchor's channel, both
  // labels and the first RNC_HEADQ quads of this thread's first row (the whole row at the model's width) -- and is consumed below in
  // the order it went out.  One cold round trip instead of five (fi | labels[i] | quads 0-7 | quads 8-15 | labels[j]).
  LTR_INIT(i);
  LTR(0);
  float fi0 = 0.f, yj0 = 0.f;
  f32x4 q[RNC_HEADQ];
  if (tid < dim) fi0 = f[(size_t)i * dim + tid];
  const float yi = labels[label_mod > 0 ? i % label_mod : i];
  if (tid < n) {
    yj0 = labels[label_mod > 0 ? tid % label_mod : tid];
    const f32x4* fj = reinterpret_cast<const f32x4*>(f + (size_t)tid * dim);
    if (hfull) {          // no branch between the requests
#pragma unroll
      for (int u = 0; u < RNC_HEADQ; ++u) q[u] = fj[u];
    } else if (vec) {     // only the quads that exist (a slot without one is never read)
#pragma unroll
      for (int u = 0; u < RNC_HEADQ; ++u)
        if (u < nq) q[u] = fj[u];
    }
  }
  if (tid < dim) fi[tid] = fi0;
  for (int c = tid + 256; c < dim; c += 256) fi[c] = f[(size_t)i * dim + c];
  __syncthreads();
  LTR(1);
  float mx = -INFINITY;
  // quads [c0, nq) of row j, 16-byte loads, 8 in flight (a scalar loop is one dependent L2 round trip per channel).  Same summation
  // order as the scalar loop: s over the channels ascending.  The fused multiply-add is written out: left to contraction, a chain that
  // starts from a literal 0 may become fma(d0, d0, d1 * d1) -- the other order, other bits.
  auto quads_from = [&](const int j, int c0, float s) -> float {
    const f32x4* fj = reinterpret_cast<const f32x4*>(f + (size_t)j * dim);
    for (; c0 < nq; c0 += 8) {
      f32x4 r[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) r[u] = c0 + u < nq ? fj[c0 + u] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (c0 + u < nq) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float d = fi[4 * (c0 + u) + e] - r[u][e];
            s = __fmaf_rn(d, d, s);
          }
        }
    }
    return s;
  };
  auto scalar_row = [&](const int j) -> float {
    float s = 0.f;
    for (int c = 0; c < dim; ++c) {
      const float d = fi[c] - f[(size_t)j * dim + c];
      s = __fmaf_rn(d, d, s);
    }
    return s;
  };
  auto put = [&](const int j, const float s, const float yj) {
    const float dist = sqrtf(s);
    dd[j] = dist;
    w.dist[(size_t)i * n + j] = dist;
    const float l = fabsf(yi - yj);
    ld[j] = l;
    thr[j] = __fsub_rn(l, 0.0001f);
    mx = fmaxf(mx, -dist * inv_t);
  };
  if (tid < n) {   // the row whose loads are already on their way
    float s = 0.f;
    if (hfull) {
#pragma unroll
      for (int u = 0; u < RNC_HEADQ; ++u) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = fi[4 * u + e] - q[u][e];
          s = __fmaf_rn(d, d, s);
        }
      }
      s = quads_from(tid, RNC_HEADQ, s);
    } else if (vec) {
#pragma unroll
      for (int u = 0; u < RNC_HEADQ; ++u)
        if (u < nq) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float d = fi[4 * u + e] - q[u][e];
            s = __fmaf_rn(d, d, s);
          }
        }
      s = quads_from(tid, RNC_HEADQ, s);
    } else {
      s = scalar_row(tid);
    }
    put(tid, s, yj0);
  }
  for (int j = tid + 256; j < n; j += 256)
    put(j, vec ? quads_from(j, 0, 0.f) : scalar_row(j), labels[label_mod > 0 ? j % label_mod : j]);
  LTR(2);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  for (int j = threadIdx.x; j < n; j += 256) ee[j] = expf(-dd[j] * inv_t - mx);
  __syncthreads();
  LTR(3);
  const bool al4 = (n & 3) == 0 && (reinterpret_cast<uintptr_t>(ld) & 15) == 0;   // ld, ee, thr, iD: all on 16-byte boundaries then
  float acc = 0.f;
  for (int k = threadIdx.x; k < n; k += 256) {
    if (k == i) {
      iD[k] = 0.f;
      continue;
    }
    const float t = thr[k];
    const float dsum = rnc_masked_sum<true>(ld, ee, t, n, i, al4);    // j ascending: (j != i && ld[j] >= t) ? ee[j] : 0
    iD[k] = 1.f / dsum;
    acc += (-dd[k] * inv_t - mx) - logf(dsum);
  }
  const float s = block_sum_256(acc, red);
  if (threadIdx.x == 0) w.rowloss[i] = s;
  LTR(4);
  if (!want_grad) return;
  __syncthreads();
  const float c = 1.f / ((float)n * (float)(n - 1));
  for (int j = threadIdx.x; j < n; j += 256) {
    float g = 0.f;
    if (j != i) {
      const float lj = ld[j];
      const float sum = rnc_masked_sum<false>(thr, iD, lj, n, i, al4);   // k ascending: (k != i && lj >= thr[k]) ? iD[k] : 0
      g = -c * (1.f - ee[j] * sum);
    }
    w.G[(size_t)i * n + j] = g;
  }
  LTR(5);
}
__global__ __launch_bounds__(256) void rnc_row_kernel(const float* f, const float* labels, int label_mod, int n,
                                                      int dim, float inv_t, RncWs w, int want_grad) {
  extern __shared__ float sm[];
  rnc_row_body(f, labels, label_mod, n, dim, inv_t, w, want_grad, blockIdx.x, sm);
}

// ---- O(n^2 log n) formulation (n <= 2048) ---------------------------------------------------------------------
// For anchor i the reference's neg_mask row for k, {j : |y_i - y_j| >= |y_i - y_k| - 1e-4} (loss.py:303), is the
// complement of a window around i in the order of the labels: with the labels sorted ONCE (rnc_sort_kernel) it is a
// prefix [0, L) plus a suffix [U, n) of the sorted order, and the gradient's {k : |y_i - y_k| - 1e-4 <= |y_i - y_j|}
// is a window [A, B] around i.  Prefix / suffix sums of exp(logit) and window sums of 1/D then replace the two
// O(n^2) loops per anchor of rnc_row_kernel; L, U, A, B come from binary searches that evaluate the SAME fp32
// predicate as the reference on the probed elements (fabsf(y_i - y_j) >= fsub(|y_i - y_k|, 1e-4f): monotone on either
// side of i), so set membership stays bit-exact.  All partial sums are sums of non-negative terms taken outward from
// the ends / from i (no prefix differences -> no cancellation), in a fixed order.
// At n = 128 (one GPU, B = 64) this is on par with the direct loops; at n = 1024 (B_global = 512 under data
// parallelism, where EVERY rank evaluates the full loss) it is 0.67 ms -> tens of microseconds per step.
// sorted order of the labels by counting: rank[j] = #{k : y_k < y_j or (y_k == y_j and k < j)} (ties by index: a
// total, deterministic order), perm = rank^-1.  n threads x n comparisons from LDS: a few microseconds at n = 1024.
__global__ __launch_bounds__(256) void rnc_sort_kernel(const float* labels, int label_mod, int n, int* perm, int* rank) {
  extern __shared__ float ysm[];   // [n]
  for (int t = threadIdx.x; t < n; t += 256) ysm[t] = labels[label_mod > 0 ? t % label_mod : t];
  __syncthreads();
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const float yj = ysm[j];
  int r = 0;
#pragma unroll 8
  for (int k = 0; k < n; ++k) {
    const float yk = ysm[k];
    r += (yk < yj || (yk == yj && k < j)) ? 1 : 0;
  }
  rank[j] = r;
  perm[r] = j;
}

// inclusive scan of a[0..n) in LDS with 256 threads (reverse: suffix sums), fixed order; tmp: >= 4 floats
__device__ __forceinline__ void block_scan(float* a, int n, bool reverse, float* tmp) {
  const int per = (n + 255) / 256;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lo = t * per, hi = min(n, lo + per);
  float s = 0.f;
  for (int p = lo; p < hi; ++p) s += a[reverse ? n - 1 - p : p];
  // exclusive scan of the 256 per-thread partials: shuffles inside a wave, then the four wave totals
  float incl = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  __syncthreads();                 // tmp may still be read by a previous scan
  if (lane == 63) tmp[wave] = incl;
  __syncthreads();
  float run = incl - s;
  for (int w2 = 0; w2 < wave; ++w2) run += tmp[w2];
  for (int p = lo; p < hi; ++p) {
    const int q = reverse ? n - 1 - p : p;
    run += a[q];
    a[q] = run;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void rnc_row_sorted_kernel(const float* f, const float* labels, int label_mod, int n, int dim,
                                                             float inv_t, RncWs w, const int* perm, const int* rank,
                                                             int want_grad) {
  extern __shared__ float sm[];   // fi[dim4] | ys[n] | dd[n] | ee[n] | pre[n] | suf[n] | iD[n] | oL[n] | oR[n] | tmp[8]
  __shared__ float red[4];
  const int dim4 = (dim + 3) & ~3;
  float* fi = sm;
  float* ys = fi + dim4;
  float* dd = ys + n;
  float* ee = dd + n;
  float* pre = ee + n;
  float* suf = pre + n;
  float* iD = suf + n;
  float* oL = iD + n;
  float* oR = oL + n;
  float* tmp = oR + n;
  const int i = blockIdx.x, tid = threadIdx.x;
  const int pos_i = rank[i];
  for (int c = tid; c < dim; c += 256) fi[c] = f[(size_t)i * dim + c];
  for (int r = tid; r < n; r += 256) {
    const int j = perm[r];
    ys[r] = labels[label_mod > 0 ? j % label_mod : j];
  }
  __syncthreads();
  const float yi = ys[pos_i];
  const bool vec = (dim & 3) == 0 && (reinterpret_cast<uintptr_t>(f) & 15) == 0;
  float mx = -INFINITY;
  for (int r = tid; r < n; r += 256) {
    const int j = perm[r];
    float s = 0.f;
    if (vec) {
      const f32x4* fj = reinterpret_cast<const f32x4*>(f + (size_t)j * dim);
      for (int c0 = 0; c0 < dim / 4; c0 += 8) {
        f32x4 rr[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) rr[u] = c0 + u < dim / 4 ? fj[c0 + u] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (c0 + u < dim / 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float d = fi[4 * (c0 + u) + e] - rr[u][e];
              s += d * d;
            }
          }
      }
    } else {
      for (int c = 0; c < dim; ++c) {
        const float d = fi[c] - f[(size_t)j * dim + c];
        s += d * d;
      }
    }
    const float dist = sqrtf(s);
    dd[r] = dist;
    w.dist[(size_t)i * n + j] = dist;
    mx = fmaxf(mx, -dist * inv_t);
  }
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  for (int r = tid; r < n; r += 256) {
    const float e = r == pos_i ? 0.f : expf(-dd[r] * inv_t - mx);   // the anchor itself is excluded (diagonal removal, loss.py:294-296)
    ee[r] = e;
    pre[r] = e;
    suf[r] = e;
  }
  __syncthreads();
  block_scan(pre, n, false, tmp);   // pre[r] = sum_{p <= r} ee[p]
  block_scan(suf, n, true, tmp);    // suf[r] = sum_{p >= r} ee[p]
  float acc = 0.f;
  for (int r = tid; r < n; r += 256) {
    float inv = 0.f;
    if (r != pos_i) {
      const float t = __fsub_rn(fabsf(yi - ys[r]), 0.0001f);
      // L = number of p in [0, pos_i] with fabsf(yi - ys[p]) >= t (true ... true false ... false)
      int lo = 0, hi = pos_i + 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (fabsf(yi - ys[mid]) >= t) lo = mid + 1; else hi = mid;
      }
      const int L = lo;
      // U = first p in [pos_i, n) with fabsf(yi - ys[p]) >= t (false ... false true ... true)
      lo = pos_i;
      hi = n;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (fabsf(yi - ys[mid]) >= t) hi = mid; else lo = mid + 1;
      }
      const int U = lo;
      const float dsum = (L > 0 ? pre[L - 1] : 0.f) + (U < n ? suf[U] : 0.f);
      inv = 1.f / dsum;
      acc += (-dd[r] * inv_t - mx) - logf(dsum);
    }
    iD[r] = inv;
  }
  const float sl = block_sum_256(acc, red);
  if (tid == 0) w.rowloss[i] = sl;
  if (!want_grad) return;
  __syncthreads();
  for (int r = tid; r < n; r += 256) {
    oL[r] = r <= pos_i ? iD[r] : 0.f;
    oR[r] = r >= pos_i ? iD[r] : 0.f;
  }
  __syncthreads();
  block_scan(oL, n, true, tmp);     // oL[p] = sum_{q = p .. pos_i} iD[q]   (p <= pos_i)
  block_scan(oR, n, false, tmp);    // oR[p] = sum_{q = pos_i .. p} iD[q]   (p >= pos_i)
  const float c = 1.f / ((float)n * (float)(n - 1));
  for (int r = tid; r < n; r += 256) {
    const int j = perm[r];
    float g = 0.f;
    if (r != pos_i) {
      const float lj = fabsf(yi - ys[r]);
      // A = first p in [0, pos_i] with thr(p) <= lj  (thr non-increasing towards pos_i: false ... false true ... true)
      int lo = 0, hi = pos_i;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lj >= __fsub_rn(fabsf(yi - ys[mid]), 0.0001f)) hi = mid; else lo = mid + 1;
      }
      const int A = lo;
      // B = last p in [pos_i, n) with thr(p) <= lj  (true ... true false ... false)
      lo = pos_i;
      hi = n - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (lj >= __fsub_rn(fabsf(yi - ys[mid]), 0.0001f)) lo = mid; else hi = mid - 1;
      }
      const int B = lo;
      g = -c * (1.f - ee[r] * (oL[A] + oR[B]));   // iD[pos_i] = 0: counting it on both sides is harmless
    }
    w.G[(size_t)i * n + j] = g;
  }
}

// df_i = -(1/t) sum_j (G_ij + G_ji) (f_i - f_j) / dist_ij ; one workgroup per local row
__device__ __forceinline__ void rnc_dfeat_body(const float* f, int n, int dim, float inv_t, float weight, int row0, RncWs w, float* df,
                                               const int bx, float* sm /* coef[n], then red[4][64] */) {
  float* coef = sm;
  float* red = sm + n;
  const int i = row0 + bx;
  LTR_INIT(bx);
  LTR(8);
  for (int j = threadIdx.x; j < n; j += 256) {
    const float d = w.dist[(size_t)i * n + j];
    coef[j] = (j != i && d > 0.f) ? (w.G[(size_t)i * n + j] + w.G[(size_t)j * n + i]) / d : 0.f;
  }
  __syncthreads();
  LTR(9);
  const int part = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int c0 = 0; c0 < dim; c0 += 64) {
    const int c = c0 + lane;
    float acc = 0.f;
    if (c < dim) {
      const float fic = f[(size_t)i * dim + c];
      int j = part;
      for (; j + 28 < n; j += 32) {   // 8 rows of loads in flight (same summation order as the plain loop)
        float fj[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) fj[u] = f[(size_t)(j + 4 * u) * dim + c];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += coef[j + 4 * u] * (fic - fj[u]);
      }
      for (; j < n; j += 4) acc += coef[j] * (fic - f[(size_t)j * dim + c]);
    }
    LTR(10);
    red[part * 64 + lane] = acc;
    __syncthreads();
    if (part == 0 && c < dim)
      df[(size_t)bx * dim + c] = -weight * inv_t * (red[lane] + red[64 + lane] + red[128 + lane] + red[192 + lane]);
    __syncthreads();
  }
  LTR(11);
}
__global__ __launch_bounds__(256) void rnc_dfeat_kernel(const float* f, int n, int dim, float inv_t, float weight,
                                                        int row0, RncWs w, float* df) {
  extern __shared__ float sm[];
  rnc_dfeat_body(f, n, dim, inv_t, weight, row0, w, df, blockIdx.x, sm);
}

__global__ void rnc_mask_kernel(const float* y, int n, uint8_t* mask) {
  const int64_t total = (int64_t)n * (n - 1) * (n - 1);
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int i = (int)(e / ((int64_t)(n - 1) * (n - 1)));
  const int64_t r = e - (int64_t)i * (n - 1) * (n - 1);
  int k = (int)(r / (n - 1)), j = (int)(r - (int64_t)k * (n - 1));
  k += (k >= i);
  j += (j >= i);
  const float dij = fabsf(y[i] - y[j]), dik = fabsf(y[i] - y[k]);
  mask[e] = dij >= __fsub_rn(dik, 0.0001f) ? 1 : 0;
}


// ---- row-wise criteria: one wavefront per row of W <= 1024 elements, the row held in registers (16 per lane) ----------
// Every row's value and gradient depend on that row alone and the loss is a plain sum of row values / denom, so -- unlike
// RMSE, the square root of a GLOBAL mean -- the gradient needs no first pass and shards of a batch add up exactly.
constexpr int ROW_MAXW = 1024;
constexpr int ROW_K = ROW_MAXW / 64;
constexpr int CRIT_COSINE = SDUMC_DISTILL_COSINE, CRIT_KL = SDUMC_DISTILL_KL, CRIT_CE = 3;

// 1 - cos(x, y) as torch.cosine_similarity (ATen Distance.cpp): x / max(|x|, eps) . y / max(|y|, eps), eps = 1e-8, each norm
// clamped on its own; clamp_min passes the gradient where norm >= eps only, so a clamped norm is a constant.
// gx / gy (may be null): scale * d(1 - cos)/dx, /dy.  Returns the row's value in every lane.
template <bool GRAD>
__device__ __forceinline__ float cosine_row(const float* xr, const float* yr, int W, int lane, float scale, float* gx, float* gy) {
  float x[ROW_K], y[ROW_K];
#pragma unroll
  for (int k = 0; k < ROW_K; ++k) {
    const int c = lane + 64 * k;
    x[k] = c < W ? xr[c] : 0.f;
    y[k] = c < W ? yr[c] : 0.f;
  }
  float sx = 0.f, sy = 0.f;
#pragma unroll
  for (int k = 0; k < ROW_K; ++k) {
    sx += x[k] * x[k];
    sy += y[k] * y[k];
  }
  const float nx = sqrtf(wave_sum(sx)), ny = sqrtf(wave_sum(sy));
  const float eps = 1e-8f;
  const float cx = fmaxf(nx, eps), cy = fmaxf(ny, eps);
  float dot = 0.f;
#pragma unroll
  for (int k = 0; k < ROW_K; ++k) {
    x[k] = x[k] / cx;
    y[k] = y[k] / cy;
    dot += x[k] * y[k];
  }
  const float cs = wave_sum(dot);
  if (GRAD) {
    const float kx = nx >= eps ? cs : 0.f, ky = ny >= eps ? cs : 0.f;
#pragma unroll
    for (int k = 0; k < ROW_K; ++k) {
      const int c = lane + 64 * k;
      if (c < W) {
        if (gx) gx[c] = -scale * (y[k] - kx * x[k]) / cx;
        if (gy) gy[c] = -scale * (x[k] - ky * y[k]) / cy;
      }
    }
  }
  return 1.f - cs;
}

// stable softmax / log-softmax of one row held in registers: e[k] <- softmax, l[k] <- log-softmax (row maximum subtracted)
__device__ __forceinline__ void softmax_row(const float (&v)[ROW_K], int W, int lane, float (&e)[ROW_K], float (&l)[ROW_K]) {
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < ROW_K; ++k)
    if (lane + 64 * k < W) mx = fmaxf(mx, v[k]);
  mx = wave_max(mx);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < ROW_K; ++k) {
    e[k] = lane + 64 * k < W ? expf(v[k] - mx) : 0.f;
    s += e[k];
  }
  s = wave_sum(s);
  const float ls = logf(s);
#pragma unroll
  for (int k = 0; k < ROW_K; ++k) {
    e[k] = e[k] / s;
    l[k] = lane + 64 * k < W ? (v[k] - mx) - ls : 0.f;
  }
}

// S = sum_i (Q_i - P_i)(log Q_i - log P_i) = KL(Q || P) + KL(P || Q), P = softmax(x), Q = softmax(y); the loss is S / 2 per row.
// With d = log Q - log P:  dS/dx_j = P_j (E_P[d] - d_j) + P_j - Q_j,   dS/dy_j = Q_j (d_j - E_Q[d]) + Q_j - P_j.
// scale already holds the 1/2.  Equal rows: d = 0 and P = Q exactly -> value 0, gradient 0.
template <bool GRAD>
__device__ __forceinline__ float kl_row(const float* xr, const float* yr, int W, int lane, float scale, float* gx, float* gy) {
  float x[ROW_K], y[ROW_K], P[ROW_K], Q[ROW_K], d[ROW_K];
#pragma unroll
  for (int k = 0; k < ROW_K; ++k) {
    const int c = lane + 64 * k;
    x[k] = c < W ? xr[c] : 0.f;
    y[k] = c < W ? yr[c] : 0.f;
  }
  softmax_row(x, W, lane, P, x);   // x <- log P
  softmax_row(y, W, lane, Q, y);   // y <- log Q
  float S = 0.f, ep = 0.f, eq = 0.f;
#pragma unroll
  for (int k = 0; k < ROW_K; ++k) {
    d[k] = y[k] - x[k];            // (0 beyond the row)
    S += (Q[k] - P[k]) * d[k];
    ep += P[k] * d[k];
    eq += Q[k] * d[k];
  }
  S = wave_sum(S);
  if (GRAD) {
    ep = wave_sum(ep);
    eq = wave_sum(eq);
#pragma unroll
    for (int k = 0; k < ROW_K; ++k) {
      const int c = lane + 64 * k;
      if (c < W) {
        if (gx) gx[c] = scale * (P[k] * (ep - d[k]) + (P[k] - Q[k]));
        if (gy) gy[c] = scale * (Q[k] * (d[k] - eq) + (Q[k] - P[k]));
      }
    }
  }
  return S;
}

// -log_softmax(x)[t]; gx = scale * (softmax(x) - onehot(t)).  t outside [0, W): NaN (torch raises there; a kernel cannot).
__device__ __forceinline__ float ce_row(const float* xr, float target, int W, int lane, float scale, float* gx) {
  float x[ROW_K], P[ROW_K];
#pragma unroll
  for (int k = 0; k < ROW_K; ++k) x[k] = lane + 64 * k < W ? xr[lane + 64 * k] : 0.f;
  softmax_row(x, W, lane, P, x);
  const int t = (int)target;       // target.long(): truncation
  float pick = 0.f;
#pragma unroll
  for (int k = 0; k < ROW_K; ++k) {
    const int c = lane + 64 * k;
    if (c == t && c < W) pick = x[k];
    if (gx && c < W) gx[c] = scale * (P[k] - (c == t ? 1.f : 0.f));
  }
  pick = wave_sum(pick);
  return (t >= 0 && t < W) ? -pick : NAN;
}

template <bool GRAD>
__device__ __forceinline__ float crit_row(int crit, const float* xr, const float* yr, int W, int lane, float scale, float* gx,
                                          float* gy) {
  return crit == CRIT_COSINE ? cosine_row<GRAD>(xr, yr, W, lane, scale, gx, gy) : kl_row<GRAD>(xr, yr, W, lane, scale, gx, gy);
}

// The modules' standalone call: ONE workgroup of 16 wavefronts, wavefront w takes rows w, w + 16, ... in order, then the 16
// partial sums are added in index order.  (No workspace in the call's signature, and the module loop is not the fast path:
// the fused step runs the same row bodies across many workgroups, below.)
__global__ __launch_bounds__(1024) void row_crit_kernel(int crit, const float* a, const float* b, int R, int W, float gscale,
                                                        float vscale, float* loss_out, float* da, float* db) {
  __shared__ float red[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float acc = 0.f;
  for (int r = wave; r < R; r += 16) {
    const size_t o = (size_t)r * W;
    if (crit == CRIT_CE)
      acc += ce_row(a + o, b[r], W, lane, gscale, da ? da + o : nullptr);
    else
      acc += crit_row<true>(crit, a + o, b + o, W, lane, gscale, da ? da + o : nullptr, db ? db + o : nullptr);
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < 16; ++w) s += red[w];
    *loss_out = s * vscale;
  }
}

// ---- the five "small" distillation terms of main :137-148 in two launches -------------------------------
// pass 1: per-block partial sums of squared differences of the three RMSE pairs (+ both MSE terms, block 0)
// pass 2: every block re-reduces the (few) partials in a fixed order, then writes the gradients of its chunk
struct DistillArgs {
  int B;            // local samples per stream
  float denom;      // B_global
  const float *vals, *labels, *th, *ct, *z;   // network outputs [2B, ...]
  float w[5];       // full_mse, missing_mse, text_feat, text_query_feat, features
  const float* ssd_global;                      // [3] or nullptr
  float *d_vals, *d_th, *d_ct, *d_z;
  float* losses;    // [8]: writes 1..5
  float* part;      // [3][nblk]
  int nblk[3];
  int crit;         // SDUMC_DISTILL_*: uniform per launch
  int reg;          // SDUMC_REGRESS_*: the criterion of the two regression terms, uniform per launch
  float reg_delta;  // Huber's delta (read by SDUMC_REGRESS_HUBER alone)
  // a stored teacher (sdumc_teacher): tt[p] != nullptr -> the target of pair p's sample b is row tidx[b] (tidx nullptr: row b) of
  // that table instead of row b of stream 0, and stream 0 gets no gradient from the pair
  const float* tt[3];     // text_hidden [tn_rows, 256] | cross_text [tn_rows, 7, 128] | fused [tn_rows, 128]
  const int64_t* tidx;    // [B] or nullptr
  int64_t tn_rows;
};
constexpr int DCH = 4096;   // elements per block
static_assert(DCH % SDUMC_D == 0 && DCH % SDUMC_H == 0 && SDUMC_D <= ROW_MAXW && SDUMC_H <= ROW_MAXW,
              "a block's chunk is a whole number of rows of every distillation pair");
// The teacher's rows of one block's chunk.  A chunk of DCH elements touches at most 32 samples of a pair (`fused`: 32 rows of 128;
// text_hidden 16; cross_text, whose 896-element samples straddle chunk edges, at most 6): their indices are read ONCE, in front of the loops, one per thread, into LDS as element offsets into the
// table -- the loops then wait for no global read of an index.  An index outside [0, tn_rows) is never turned into an address: its
// slot holds -1, teacher_row gives nullptr and the caller takes NaN for the row.
constexpr int T_SLOTS = 40;
struct TeacherChunk {
  int b0;               // first sample of the chunk
  long long* off;       // LDS [T_SLOTS]
};
__device__ __forceinline__ TeacherChunk teacher_chunk(const DistillArgs& a, const int p, const int bx, const int64_t n, long long* off) {
  const int per = p == 0 ? SDUMC_D : (p == 1 ? SDUMC_NQ * SDUMC_H : SDUMC_H);
  const int64_t e0 = (int64_t)bx * DCH, e1 = min(n, e0 + DCH);      // (e0 < e1 <= B * per: every sample below is one of the batch)
  const int b0 = (int)(e0 / per), nb = (int)((e1 - 1) / per) - b0 + 1;
  if ((int)threadIdx.x < nb && (int)threadIdx.x < T_SLOTS) {
    const int b = b0 + threadIdx.x;
    const int64_t r = a.tidx ? a.tidx[b] : (int64_t)b;
    off[threadIdx.x] = (r >= 0 && r < a.tn_rows) ? r * per : -1;
  }
  __syncthreads();
  return TeacherChunk{b0, off};
}
// (b is the same in every lane of a wavefront wherever this is called: a pair's samples are whole multiples of 64 elements)
__device__ __forceinline__ const float* teacher_row(const DistillArgs& a, const int p, const TeacherChunk& c, const int b) {
  const long long o = c.off[b - c.b0];
  return o >= 0 ? a.tt[p] + o : nullptr;
}
__device__ __forceinline__ void distill_pair(const DistillArgs& a, int p, const float*& s1, const float*& s0, float*& g,
                                             int64_t& n) {
  const int64_t per = p == 0 ? SDUMC_D : (p == 1 ? SDUMC_NQ * SDUMC_H : SDUMC_H);
  n = (int64_t)a.B * per;
  const float* base = p == 0 ? a.th : (p == 1 ? a.ct : a.z);
  s0 = base;
  s1 = base + n;
  g = p == 0 ? a.d_th : (p == 1 ? a.d_ct : a.d_z);
}
// cosine / KL: the rows of a pair are its last axis (text_hidden [B,256], cross_text [B*7,128], fused [B,128]); a block's chunk
// of DCH elements is 16 or 32 whole rows.  Pass 1: wavefront w adds the values of rows w, w + 4, ... of the chunk, the four sums
// are added in order -> one partial per block, in the slots the sums of squares take.
__device__ __forceinline__ void distill_rows_partials(const DistillArgs& a, const int bx, const int p, float* red, long long* toff) {
  const float *s1, *s0;
  float* g;
  int64_t n;
  distill_pair(a, p, s1, s0, g, n);
  const int W = p == 0 ? SDUMC_D : SDUMC_H;
  const int rpb = DCH / W, rows = (int)(n / W);
  const int r1 = min(rows, (bx + 1) * rpb);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float acc = 0.f;
  if (a.tt[p]) {      // the same rows against the teacher's: row r of the pair is row r % rps of sample r / rps
    const int rps = p == 1 ? SDUMC_NQ : 1;
    const TeacherChunk tc = teacher_chunk(a, p, bx, n, toff);
    for (int r = bx * rpb + wave; r < r1; r += 4) {
      const int b = __builtin_amdgcn_readfirstlane(r / rps);
      const float* t = teacher_row(a, p, tc, b);
      // (no row to read: the value a NaN target row gives, without running the row body on an address that does not exist)
      acc += t ? crit_row<false>(a.crit, s1 + (size_t)r * W, t + (r - b * rps) * W, W, lane, 0.f, nullptr, nullptr) : NAN;
    }
  } else {
    for (int r = bx * rpb + wave; r < r1; r += 4)
      acc += crit_row<false>(a.crit, s1 + (size_t)r * W, s0 + (size_t)r * W, W, lane, 0.f, nullptr, nullptr);
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) a.part[p * a.nblk[1] + bx] = red[0] + red[1] + red[2] + red[3];
}
// Pass 2: block 0 of a pair adds the partials in index order (the value); every block writes the gradients of its rows, which
// need nothing from other rows.  Stream 1 is the first argument (main :148: loss(x_1, x_0.detach())).
__device__ __forceinline__ void distill_rows_apply(const DistillArgs& a, const int bx, const int p, float* red, long long* toff) {
  const float *s1, *s0;
  float* g;
  int64_t n;
  distill_pair(a, p, s1, s0, g, n);
  const float half = a.crit == CRIT_KL ? 0.5f : 1.f;
  if (bx == 0) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < a.nblk[p]; i += 256) acc += a.part[p * a.nblk[1] + i];
    const float s = block_sum_256(acc, red);
    if (threadIdx.x == 0) a.losses[3 + p] = s * half / a.denom;
  }
  const int W = p == 0 ? SDUMC_D : SDUMC_H;
  const int rpb = DCH / W, rows = (int)(n / W);
  const int r1 = min(rows, (bx + 1) * rpb);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float scale = a.w[2 + p] * half / a.denom;
  if (a.tt[p]) {      // a stored teacher is a constant: stream 0's rows of this pair's gradient are +0.0, for `fused` too
    const int rps = p == 1 ? SDUMC_NQ : 1;
    const TeacherChunk tc = teacher_chunk(a, p, bx, n, toff);
    for (int r = bx * rpb + wave; r < r1; r += 4) {
      const size_t o = (size_t)r * W;
      const int b = __builtin_amdgcn_readfirstlane(r / rps);
      const float* t = teacher_row(a, p, tc, b);
      if (t)
        crit_row<true>(a.crit, s1 + o, t + (r - b * rps) * W, W, lane, scale, g + n + o, nullptr);
      for (int c = lane; c < W; c += 64) {
        if (!t) g[n + o + c] = NAN;      // the student's gradient against a NaN target row
        g[o + c] = 0.f;
      }
    }
    return;
  }
  for (int r = bx * rpb + wave; r < r1; r += 4) {
    const size_t o = (size_t)r * W;
    crit_row<true>(a.crit, s1 + o, s0 + o, W, lane, scale, g + n + o, p == 2 ? g + o : nullptr);
    if (p != 2)      // stream 0 detached for text_feat / text_query_feat: its gradient buffer is written with zeros
      for (int c = lane; c < W; c += 64) g[o + c] = 0.f;
  }
}
// RMSE against a stored teacher: element i of the pair is column i % per of sample i / per; the 256 threads walk the chunk as they
// do without one (coalesced inside a row), the target comes from the teacher's row of that sample.
__device__ __forceinline__ float teacher_elem(const DistillArgs& a, const int p, const int per, const TeacherChunk& tc, const int64_t i) {
  // (shifts and one division by a constant, in 32 bits: the host refuses a teacher where B * 896 leaves int32)
  const unsigned u = (unsigned)i;
  const int b = __builtin_amdgcn_readfirstlane((int)(p == 0 ? u / (unsigned)SDUMC_D : (p == 1 ? u / (unsigned)(SDUMC_NQ * SDUMC_H) : u / (unsigned)SDUMC_H)));
  const float* t = teacher_row(a, p, tc, b);
  return t ? t[i - (int64_t)b * per] : NAN;
}
__device__ __forceinline__ void distill_partials_body(const DistillArgs a, const int bx, const int p) {
  __shared__ float red[4];
  __shared__ long long toff[T_SLOTS];      // (a stored teacher's row offsets of this block's chunk: teacher_chunk)
  if (bx >= a.nblk[p]) return;
  if (a.crit != SDUMC_DISTILL_RMSE) {
    distill_rows_partials(a, bx, p, red, toff);
    return;
  }
  const float *s1, *s0;
  float* g;
  int64_t n;
  distill_pair(a, p, s1, s0, g, n);
  const int64_t i0 = (int64_t)bx * DCH, i1 = min(n, i0 + DCH);
  float acc = 0.f;
  if (a.tt[p]) {
    const int per = p == 0 ? SDUMC_D : (p == 1 ? SDUMC_NQ * SDUMC_H : SDUMC_H);
    const TeacherChunk tc = teacher_chunk(a, p, bx, n, toff);
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
      const float d = s1[i] - teacher_elem(a, p, per, tc, i);
      acc += d * d;
    }
  } else {
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
      const float d = s1[i] - s0[i];
      acc += d * d;
    }
  }
  const float s = block_sum_256(acc, red);
  if (threadIdx.x == 0) a.part[p * a.nblk[1] + bx] = s;
}
__global__ __launch_bounds__(256) void distill_partials_kernel(const DistillArgs a) { distill_partials_body(a, blockIdx.x, blockIdx.y); }
__device__ __forceinline__ void distill_apply_body(const DistillArgs a, const int bx, const int p) {
  __shared__ float red[4];
  __shared__ long long toff[T_SLOTS];
  if (p == 3) {   // MSELoss on both streams (loss.py:19-33): value + gradient
    if (bx > 1) return;
    const int sidx = bx;
    if (a.reg != SDUMC_REGRESS_MSE) {   // L1 / Huber / CCC instead (sdumc_step_cfg.regress): the same workgroup, no further launch
      reg_stream(a.reg, a.reg_delta, a.vals + sidx * a.B, a.labels, a.B, a.denom, a.w[sidx], a.losses + 1 + sidx,
                 a.d_vals + sidx * a.B, red);
      return;
    }
    const float inv = 1.f / a.denom;
    float acc = 0.f;
    for (int i = threadIdx.x; i < a.B; i += 256) {
      const float d = a.vals[sidx * a.B + i] - a.labels[i];
      acc += d * d;
      a.d_vals[sidx * a.B + i] = a.w[sidx] * 2.f * d * inv;
    }
    const float s = block_sum_256(acc, red);
    if (threadIdx.x == 0) a.losses[1 + sidx] = s * inv;
    return;
  }
  if (bx >= a.nblk[p]) return;
  if (a.crit != SDUMC_DISTILL_RMSE) {
    distill_rows_apply(a, bx, p, red, toff);
    return;
  }
  const float *s1, *s0;
  float* g;
  int64_t n;
  distill_pair(a, p, s1, s0, g, n);
  float ssd;
  if (a.ssd_global) {
    ssd = a.ssd_global[p];
  } else {   // ordered re-reduction of the partials (identical in every block)
    float acc = 0.f;
    for (int i = threadIdx.x; i < a.nblk[p]; i += 256) acc += a.part[p * a.nblk[1] + i];
    ssd = block_sum_256(acc, red);
  }
  const float per = p == 0 ? SDUMC_D : (p == 1 ? SDUMC_NQ * SDUMC_H : SDUMC_H);
  const float inv_numel = 1.f / (a.denom * per);
  const float rmse = sqrtf(ssd * inv_numel);
  if (bx == 0 && threadIdx.x == 0) a.losses[3 + p] = rmse;
  const float k = a.w[2 + p] * inv_numel / rmse;   // 0/0 -> NaN exactly like torch's sqrt backward
  const int64_t i0 = (int64_t)bx * DCH, i1 = min(n, i0 + DCH);
  if (a.tt[p]) {
    const TeacherChunk tc = teacher_chunk(a, p, bx, n, toff);
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
      g[n + i] = k * (s1[i] - teacher_elem(a, p, (int)per, tc, i));      // stream 1 (student)
      g[i] = 0.f;                                                   // stream 0: no part in the pair
    }
    return;
  }
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const float gr = k * (s1[i] - s0[i]);
    g[n + i] = gr;                        // stream 1 (student)
    g[i] = p == 2 ? -gr : 0.f;           // stream 0: detached for text_feat / text_query_feat (main :148), not for features
  }
}
__global__ __launch_bounds__(256) void distill_apply_kernel(const DistillArgs a) { distill_apply_body(a, blockIdx.x, blockIdx.y); }

// ---- the six loss launches of a single-GPU step as TWO (+ the one-thread total): the distillation terms and Rank-N-Contrast
// are independent, so their first passes share a launch (workgroups [0, n): one RnC anchor each; the rest: partial sums of
// squares) and so do their second passes (RnC feature gradients | distillation values + gradients | the RnC mean).  No
// atomics, no change in any summation order: same bits as the separate launches.
struct RncArgs {
  const float* f;
  const float* labels;
  int label_mod, n, dim;
  float inv_t, weight;
  RncWs w;
  float* loss_out;
  float* df;
};
__global__ __launch_bounds__(256) void loss_stage1_kernel(const DistillArgs a, const RncArgs r, const int mx) {
  extern __shared__ float sm[];
  const int bid = blockIdx.x;
  if (bid < r.n) {
    rnc_row_body(r.f, r.labels, r.label_mod, r.n, r.dim, r.inv_t, r.w, 1, bid, sm);
  } else {
    const int q = bid - r.n;
    distill_partials_body(a, q % mx, q / mx);
  }
}
__global__ __launch_bounds__(256) void loss_stage2_kernel(const DistillArgs a, const RncArgs r, const int amx, float* hyper,
                                                          const double beta1, const double beta2) {
  extern __shared__ float sm[];
  const int bid = blockIdx.x;
  if (bid < r.n) {
    rnc_dfeat_body(r.f, r.n, r.dim, r.inv_t, r.weight, 0, r.w, r.df, bid, sm);
  } else if (bid < r.n + 4 * amx) {
    const int q = bid - r.n;
    distill_apply_body(a, q % amx, q / amx);
  } else {
    rnc_loss_body(r.n, r.w, r.loss_out);
    if (hyper && threadIdx.x == 0) {   // Adam bias correction of this step (adam.hip's adam_hyper_kernel, same double arithmetic)
      const double t = (double)hyper[1] + 1.0;
      hyper[1] = (float)t;
      hyper[2] = (float)((double)hyper[0] / (1.0 - pow(beta1, t)));
      hyper[3] = (float)sqrt(1.0 - pow(beta2, t));
    }
  }
}
}  // namespace

namespace {
// The whole data-parallel exchange record of one rank in ONE launch: blockIdx.y = 0..2 -> partial sums of squares of the
// three RMSE pairs (DCH elements per block), blockIdx.y = 3 -> copies of the RnC features and the labels.  The last
// block to finish (device-scope counter) adds the partials of each pair in index order -- the same bits whatever the
// scheduling -- writes the three sums behind the labels and re-arms the counter.
struct DpRecordArgs {
  int B, rd;
  const float *th, *ct, *z, *rnc, *labels;
  float* rec;        // [2*B*rd | B | 3]
  float* part;       // [3][nblk_max]
  unsigned* counter; // zero before the first launch; left zero by every launch
  int nblk[3], nblk_max, ncopy;
};
__global__ __launch_bounds__(256) void dp_record_kernel(const DpRecordArgs a) {
  __shared__ float red[4];
  __shared__ bool last;
  const int p = blockIdx.y;
  const int nf = 2 * a.B * a.rd;
  if (p == 3) {
    if ((int)blockIdx.x < a.ncopy) {
      const int i0 = blockIdx.x * DCH, i1 = min(nf + a.B, i0 + DCH);
      for (int i = i0 + threadIdx.x; i < i1; i += 256) a.rec[i] = i < nf ? a.rnc[i] : a.labels[i - nf];
    }
  } else if ((int)blockIdx.x < a.nblk[p]) {
    const int64_t per = p == 0 ? SDUMC_D : (p == 1 ? SDUMC_NQ * SDUMC_H : SDUMC_H);
    const int64_t n = (int64_t)a.B * per;
    const float* s0 = p == 0 ? a.th : (p == 1 ? a.ct : a.z);
    const float* s1 = s0 + n;
    const int64_t i0 = (int64_t)blockIdx.x * DCH, i1 = min(n, i0 + DCH);
    float acc = 0.f;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
      const float d = s1[i] - s0[i];
      acc += d * d;
    }
    const float sum = block_sum_256(acc, red);
    if (threadIdx.x == 0) a.part[p * a.nblk_max + blockIdx.x] = sum;
  }
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) last = atomicAdd(a.counter, 1u) == gridDim.x * gridDim.y - 1;
  __syncthreads();
  if (!last) return;
  __threadfence();
  for (int q = 0; q < 3; ++q) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < a.nblk[q]; i += 256) acc += __builtin_nontemporal_load(a.part + q * a.nblk_max + i);
    const float sum = block_sum_256(acc, red);
    if (threadIdx.x == 0) a.rec[nf + a.B + q] = sum;
    __syncthreads();
  }
  if (threadIdx.x == 0) *a.counter = 0u;
}
}  // namespace

extern "C" size_t sdumc_dp_record_workspace_bytes(int32_t B) {
  const int64_t nb = ((int64_t)B * SDUMC_NQ * SDUMC_H + DCH - 1) / DCH;
  return (size_t)(3 * nb + 16) * sizeof(float);
}

extern "C" int sdumc_dp_record(int32_t B, int32_t rd, const float* text_hidden, const float* cross_text, const float* fused,
                               const float* rnc, const float* labels, float* record, void* workspace, void* stream) {
  if (B <= 0 || rd <= 0 || !text_hidden || !cross_text || !fused || !rnc || !labels || !record || !workspace)
    return SDUMC_EINVAL;
  DpRecordArgs a;
  a.B = B; a.rd = rd;
  a.th = text_hidden; a.ct = cross_text; a.z = fused; a.rnc = rnc; a.labels = labels;
  a.rec = record;
  const int64_t per[3] = {SDUMC_D, SDUMC_NQ * SDUMC_H, SDUMC_H};
  int mx = 1;
  for (int p = 0; p < 3; ++p) {
    a.nblk[p] = (int)(((int64_t)B * per[p] + DCH - 1) / DCH);
    mx = a.nblk[p] > mx ? a.nblk[p] : mx;
  }
  a.nblk_max = a.nblk[1];
  a.ncopy = (2 * B * rd + B + DCH - 1) / DCH;
  mx = a.ncopy > mx ? a.ncopy : mx;
  a.counter = reinterpret_cast<unsigned*>(workspace);
  a.part = static_cast<float*>(workspace) + 16;
  hipLaunchKernelGGL(dp_record_kernel, dim3(mx, 4), dim3(256), 0, as_stream(stream), a);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_mse_fwd_bwd(const float* pred, const float* target, int32_t rows, float denom, float weight,
                                 float* loss_out, float* dpred, void* stream) {
  if (!pred || !target || !loss_out || rows <= 0 || denom <= 0.f) return SDUMC_EINVAL;
  hipLaunchKernelGGL(mse_kernel, dim3(1), dim3(256), 0, as_stream(stream), pred, target, rows, denom, weight, loss_out, dpred);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_reg_fwd_bwd(const float* pred, const float* target, int32_t rows, float denom, float weight, int32_t regress,
                                 float delta, float* loss_out, float* dpred, void* stream) {
  if (!pred || !target || !loss_out || rows < 1 || !(denom > 0.f) || !sdumc_regress_valid(regress, delta)) return SDUMC_EINVAL;
  if (regress == SDUMC_REGRESS_MSE)
    hipLaunchKernelGGL(mse_kernel, dim3(1), dim3(256), 0, as_stream(stream), pred, target, rows, denom, weight, loss_out, dpred);
  else
    hipLaunchKernelGGL(reg_kernel, dim3(1), dim3(256), 0, as_stream(stream), regress, delta, pred, target, rows, denom, weight,
                       loss_out, dpred);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" size_t sdumc_ssd_workspace_bytes(int64_t n) { return (size_t)((n + SSD_CHUNK - 1) / SSD_CHUNK) * sizeof(float); }

extern "C" int sdumc_ssd(const float* a, const float* b, int64_t n, float* ssd_out, float* workspace, void* stream) {
  if (!a || !b || !ssd_out || !workspace || n <= 0) return SDUMC_EINVAL;
  const int nchunk = (int)((n + SSD_CHUNK - 1) / SSD_CHUNK);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ssd_stage1, dim3(nchunk), dim3(256), 0, st, a, b, n, workspace);
  SDUMC_CHECK_LAUNCH();
  hipLaunchKernelGGL(ssd_stage2, dim3(1), dim3(256), 0, st, workspace, nchunk, ssd_out);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_rmse_bwd(const float* a, const float* b, int64_t n_local, const float* ssd_global,
                              double numel_global, float weight, float* loss_out, float* da, int32_t da_accumulate,
                              float* db, int32_t db_accumulate, void* stream) {
  if (!a || !b || !ssd_global || n_local <= 0 || numel_global <= 0) return SDUMC_EINVAL;
  hipLaunchKernelGGL(rmse_bwd_kernel, dim3((unsigned)((n_local + 255) / 256)), dim3(256), 0, as_stream(stream), a, b,
                     n_local, ssd_global, (float)(1.0 / numel_global), weight, loss_out, da, da_accumulate, db,
                     db_accumulate);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" size_t sdumc_rnc_workspace_bytes(int32_t n) { return ((size_t)5 * n * n + 2 * (size_t)n) * sizeof(float); }

static int rnc_impl(const float* feats, const float* labels, int label_mod, int32_t n, int32_t dim, float temperature,
                    float weight, int32_t row0, int32_t rows_local, float* loss_out, float* dfeats, float* workspace,
                    void* stream) {
  if (!feats || !labels || !loss_out || !workspace || n < 2 || dim <= 0 || temperature <= 0.f) return SDUMC_EINVAL;
  if (row0 < 0 || rows_local < 0 || row0 + rows_local > n) return SDUMC_EINVAL;
  hipStream_t st = as_stream(stream);
  const RncWs w = rnc_ws(workspace, n);
  const float inv_t = 1.f / temperature;
  const int want_grad = dfeats && rows_local > 0;
  if (n > 256 && n <= 2048) {
    // sorted formulation; perm / rank live in the (otherwise unused) `e` region of the workspace
    int* perm = reinterpret_cast<int*>(w.e);
    int* rank = perm + n;
    hipLaunchKernelGGL(rnc_sort_kernel, dim3((n + 255) / 256), dim3(256), (size_t)n * sizeof(float), st, labels, label_mod, n,
                       perm, rank);
    SDUMC_CHECK_LAUNCH();
    const size_t lds = ((((size_t)dim + 3) & ~(size_t)3) + 8 * (size_t)n + 8) * sizeof(float);
    if (lds > 160 * 1024) return SDUMC_EINVAL;
    if (lds > 48 * 1024 &&
        !sdumc_set_dyn_lds(rnc_row_sorted_kernel, lds))      // (the size follows n and dim: set per call, not once per device)
      return SDUMC_ELAUNCH;
    hipLaunchKernelGGL(rnc_row_sorted_kernel, dim3(n), dim3(256), lds, st, feats, labels, label_mod, n, dim, inv_t, w, perm,
                       rank, want_grad);
    SDUMC_CHECK_LAUNCH();
  } else {
    const size_t lds = (((size_t)dim + 3) & ~(size_t)3) * sizeof(float) + 5 * (size_t)n * sizeof(float);
    if (lds > 64 * 1024) return SDUMC_EINVAL;
    hipLaunchKernelGGL(rnc_row_kernel, dim3(n), dim3(256), lds, st, feats, labels, label_mod, n, dim, inv_t, w, want_grad);
    SDUMC_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(rnc_loss_kernel, dim3(1), dim3(256), 0, st, n, w, loss_out);
  SDUMC_CHECK_LAUNCH();
  if (want_grad) {
    hipLaunchKernelGGL(rnc_dfeat_kernel, dim3(rows_local), dim3(256), (n + 256) * sizeof(float), st, feats, n, dim,
                       inv_t, weight, row0, w, dfeats);
    SDUMC_CHECK_LAUNCH();
  }
  return SDUMC_OK;
}

extern "C" int sdumc_rnc_fwd_bwd(const float* feats, const float* labels, int32_t n, int32_t dim, float temperature,
                                 float weight, int32_t row0, int32_t rows_local, float* loss_out, float* dfeats,
                                 float* workspace, void* stream) {
  return rnc_impl(feats, labels, 0, n, dim, temperature, weight, row0, rows_local, loss_out, dfeats, workspace, stream);
}

// labels given once ([n/2]) and read as labels[j % (n/2)]: the reference's labels.repeat(2, 1) (loss.py:283)
extern "C" int sdumc_rnc_fwd_bwd_rep(const float* feats, const float* labels_half, int32_t n, int32_t dim,
                                     float temperature, float weight, int32_t row0, int32_t rows_local, float* loss_out,
                                     float* dfeats, float* workspace, void* stream) {
  if (n & 1) return SDUMC_EINVAL;
  return rnc_impl(feats, labels_half, n / 2, n, dim, temperature, weight, row0, rows_local, loss_out, dfeats, workspace,
                  stream);
}

extern "C" size_t sdumc_distill_workspace_bytes(int32_t B) {
  const int64_t nb = ((int64_t)B * SDUMC_NQ * SDUMC_H + DCH - 1) / DCH;
  return (size_t)(3 * nb + 64) * sizeof(float);
}

// MSE x2 + the chosen criterion x3 of main :137-148 (value + gradients w.r.t. the network outputs) in two launches.
// distill != RMSE: ssd_global is not read (the value is a sum over local rows / denom) and pass 1 always runs.
// regress: the criterion of the two regression terms (SDUMC_REGRESS_*; the p == 3 workgroups of the second launch).
namespace {
// the teacher's part of the kernels' argument (checked by the caller: sdumc_teacher_check)
void distill_teacher(DistillArgs& a, const sdumc_teacher* t) {
  a.tt[0] = t ? t->text_hidden : nullptr;
  a.tt[1] = t ? t->cross_text : nullptr;
  a.tt[2] = t ? t->fused : nullptr;
  a.tidx = t ? t->idx : nullptr;
  a.tn_rows = t ? t->n_rows : 0;
}
}  // namespace
extern "C" int sdumc_distill_crit_teacher_(int32_t B, float denom, const float* vals, const float* labels, const float* th,
                                           const float* ct, const float* z, const float* weights5, const float* ssd_global,
                                           float* d_vals, float* d_th, float* d_ct, float* d_z, float* losses, float* workspace,
                                           int32_t distill, int32_t regress, float regress_delta, const sdumc_teacher* teacher,
                                           void* stream) {
  const int have_teacher = sdumc_teacher_check(teacher, B, ssd_global != nullptr || denom != (float)B);
  if (have_teacher < 0) return SDUMC_EINVAL;
  if (B <= 0 || denom <= 0.f || !vals || !labels || !th || !ct || !z || !weights5 || !d_vals || !d_th || !d_ct || !d_z ||
      !losses || !workspace || distill < SDUMC_DISTILL_RMSE || distill > SDUMC_DISTILL_KL ||
      !sdumc_regress_valid(regress, regress_delta))
    return SDUMC_EINVAL;
  if (distill != SDUMC_DISTILL_RMSE) ssd_global = nullptr;
  DistillArgs a;
  a.crit = distill;
  a.reg = regress;
  a.reg_delta = regress_delta;
  a.B = B;
  a.denom = denom;
  a.vals = vals; a.labels = labels; a.th = th; a.ct = ct; a.z = z;
  for (int i = 0; i < 5; ++i) a.w[i] = weights5[i];
  a.ssd_global = ssd_global;
  a.d_vals = d_vals; a.d_th = d_th; a.d_ct = d_ct; a.d_z = d_z;
  a.losses = losses;
  a.part = workspace;
  distill_teacher(a, have_teacher ? teacher : nullptr);
  const int64_t per[3] = {SDUMC_D, SDUMC_NQ * SDUMC_H, SDUMC_H};
  int mx = 1;
  for (int p = 0; p < 3; ++p) {
    a.nblk[p] = (int)(((int64_t)B * per[p] + DCH - 1) / DCH);
    mx = a.nblk[p] > mx ? a.nblk[p] : mx;
  }
  hipStream_t st = as_stream(stream);
  if (!ssd_global) {
    hipLaunchKernelGGL(distill_partials_kernel, dim3(mx, 3), dim3(256), 0, st, a);
    SDUMC_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(distill_apply_kernel, dim3(mx > 2 ? mx : 2, 4), dim3(256), 0, st, a);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_distill_crit_reg_(int32_t B, float denom, const float* vals, const float* labels, const float* th,
                                       const float* ct, const float* z, const float* weights5, const float* ssd_global,
                                       float* d_vals, float* d_th, float* d_ct, float* d_z, float* losses, float* workspace,
                                       int32_t distill, int32_t regress, float regress_delta, void* stream) {
  return sdumc_distill_crit_teacher_(B, denom, vals, labels, th, ct, z, weights5, ssd_global, d_vals, d_th, d_ct, d_z, losses,
                                     workspace, distill, regress, regress_delta, nullptr, stream);
}

extern "C" int sdumc_distill_teacher_fwd_bwd(int32_t B, float denom, const float* vals, const float* labels, const float* th,
                                             const float* ct, const float* z, const float* weights5, const float* ssd_global,
                                             float* d_vals, float* d_th, float* d_ct, float* d_z, float* losses, float* workspace,
                                             int32_t distill, const sdumc_teacher* teacher, void* stream) {
  return sdumc_distill_crit_teacher_(B, denom, vals, labels, th, ct, z, weights5, ssd_global, d_vals, d_th, d_ct, d_z, losses,
                                     workspace, distill, SDUMC_REGRESS_MSE, 0.f, teacher, stream);
}

extern "C" int sdumc_distill_crit_(int32_t B, float denom, const float* vals, const float* labels, const float* th,
                                   const float* ct, const float* z, const float* weights5, const float* ssd_global,
                                   float* d_vals, float* d_th, float* d_ct, float* d_z, float* losses, float* workspace,
                                   int32_t distill, void* stream) {
  return sdumc_distill_crit_reg_(B, denom, vals, labels, th, ct, z, weights5, ssd_global, d_vals, d_th, d_ct, d_z, losses,
                                 workspace, distill, SDUMC_REGRESS_MSE, 0.f, stream);
}

extern "C" int sdumc_distill_fwd_bwd(int32_t B, float denom, const float* vals, const float* labels, const float* th,
                                     const float* ct, const float* z, const float* weights5, const float* ssd_global,
                                     float* d_vals, float* d_th, float* d_ct, float* d_z, float* losses,
                                     float* workspace, void* stream) {
  return sdumc_distill_crit_(B, denom, vals, labels, th, ct, z, weights5, ssd_global, d_vals, d_th, d_ct, d_z, losses,
                             workspace, SDUMC_DISTILL_RMSE, stream);
}

static int row_crit_launch(int crit, const float* a, const float* b, int32_t rows, int32_t groups, int32_t width, float denom,
                           float weight, float* loss_out, float* da, float* db, void* stream) {
  if (!a || !b || !loss_out || rows <= 0 || groups <= 0 || width <= 0 || width > ROW_MAXW || !(denom > 0.f)) return SDUMC_EINVAL;
  if ((int64_t)rows * groups > INT32_MAX / ROW_MAXW) return SDUMC_EINVAL;
  if (crit == CRIT_CE && (groups != 1 || db)) return SDUMC_EINVAL;
  const float half = crit == CRIT_KL ? 0.5f : 1.f;
  hipLaunchKernelGGL(row_crit_kernel, dim3(1), dim3(1024), 0, as_stream(stream), crit, a, b, rows * groups, width,
                     weight * half / denom, half / denom, loss_out, da, db);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}
extern "C" int sdumc_cosine_fwd_bwd(const float* a, const float* b, int32_t rows, int32_t groups, int32_t width, float denom,
                                    float weight, float* loss_out, float* da, float* db, void* stream) {
  return row_crit_launch(CRIT_COSINE, a, b, rows, groups, width, denom, weight, loss_out, da, db, stream);
}
extern "C" int sdumc_kl_fwd_bwd(const float* a, const float* b, int32_t rows, int32_t groups, int32_t width, float denom,
                                float weight, float* loss_out, float* da, float* db, void* stream) {
  return row_crit_launch(CRIT_KL, a, b, rows, groups, width, denom, weight, loss_out, da, db, stream);
}
extern "C" int sdumc_ce_fwd_bwd(const float* a, const float* b, int32_t rows, int32_t groups, int32_t width, float denom,
                                float weight, float* loss_out, float* da, float* db, void* stream) {
  return row_crit_launch(CRIT_CE, a, b, rows, groups, width, denom, weight, loss_out, da, db, stream);
}

// MSE x2 + the distillation criterion x3 + RnC over cat(stream 0, stream 1) with the labels repeated (main :134-148): values and every gradient
// w.r.t. the network outputs in two launches.  Returns 1 when the shape is not one it takes (n = 2B > 256: the sorted RnC form).
// regress: the criterion of the two regression terms (SDUMC_REGRESS_*; the p == 3 workgroups of the second launch).
extern "C" int sdumc_losses_fused_teacher_(int32_t B, const float* vals, const float* labels, const float* th, const float* ct,
                                           const float* z, const float* rnc_feats, int32_t rd, float temperature,
                                           const float* weights6, float* d_vals, float* d_th, float* d_ct, float* d_z,
                                           float* d_rnc, float* losses, float* distill_ws, float* rnc_workspace, float* hyper,
                                           double beta1, double beta2, int32_t distill, int32_t regress, float regress_delta,
                                           const sdumc_teacher* teacher, void* stream) {
  const int n = 2 * B;
  const int have_teacher = sdumc_teacher_check(teacher, B, false);
  if (have_teacher < 0) return SDUMC_EINVAL;
  if (distill < SDUMC_DISTILL_RMSE || distill > SDUMC_DISTILL_KL || !sdumc_regress_valid(regress, regress_delta)) return SDUMC_EINVAL;
  if (B <= 0 || n > 256 || rd <= 0 || temperature <= 0.f) return 1;
  const size_t lds1 = (((size_t)rd + 3) & ~(size_t)3) * sizeof(float) + 5 * (size_t)n * sizeof(float);
  const size_t lds2 = ((size_t)n + 256) * sizeof(float);
  if (lds1 > 64 * 1024) return 1;
  DistillArgs a;
  a.B = B;
  a.denom = (float)B;
  a.vals = vals; a.labels = labels; a.th = th; a.ct = ct; a.z = z;
  for (int i = 0; i < 5; ++i) a.w[i] = weights6[i];
  a.ssd_global = nullptr;
  a.crit = distill;
  a.reg = regress;
  a.reg_delta = regress_delta;
  a.d_vals = d_vals; a.d_th = d_th; a.d_ct = d_ct; a.d_z = d_z;
  a.losses = losses;
  a.part = distill_ws;
  distill_teacher(a, have_teacher ? teacher : nullptr);
  const int64_t per[3] = {SDUMC_D, SDUMC_NQ * SDUMC_H, SDUMC_H};
  int mx = 1;
  for (int p = 0; p < 3; ++p) {
    a.nblk[p] = (int)(((int64_t)B * per[p] + DCH - 1) / DCH);
    mx = a.nblk[p] > mx ? a.nblk[p] : mx;
  }
  const int amx = mx > 2 ? mx : 2;
  RncArgs r;
  r.f = rnc_feats; r.labels = labels; r.label_mod = B; r.n = n; r.dim = rd;
  r.inv_t = 1.f / temperature; r.weight = weights6[5];
  r.w = rnc_ws(rnc_workspace, n);
  r.loss_out = losses + 6;
  r.df = d_rnc;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(loss_stage1_kernel, dim3(n + 3 * mx), dim3(256), lds1, st, a, r, mx);
  SDUMC_CHECK_LAUNCH();
  hipLaunchKernelGGL(loss_stage2_kernel, dim3(n + 4 * amx + 1), dim3(256), lds2, st, a, r, amx, hyper, beta1, beta2);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_losses_fused_reg_(int32_t B, const float* vals, const float* labels, const float* th, const float* ct,
                                       const float* z, const float* rnc_feats, int32_t rd, float temperature,
                                       const float* weights6, float* d_vals, float* d_th, float* d_ct, float* d_z, float* d_rnc,
                                       float* losses, float* distill_ws, float* rnc_workspace, float* hyper, double beta1,
                                       double beta2, int32_t distill, int32_t regress, float regress_delta, void* stream) {
  return sdumc_losses_fused_teacher_(B, vals, labels, th, ct, z, rnc_feats, rd, temperature, weights6, d_vals, d_th, d_ct, d_z, d_rnc,
                                     losses, distill_ws, rnc_workspace, hyper, beta1, beta2, distill, regress, regress_delta, nullptr,
                                     stream);
}

extern "C" int sdumc_losses_fused_(int32_t B, const float* vals, const float* labels, const float* th, const float* ct,
                                   const float* z, const float* rnc_feats, int32_t rd, float temperature, const float* weights6,
                                   float* d_vals, float* d_th, float* d_ct, float* d_z, float* d_rnc, float* losses,
                                   float* distill_ws, float* rnc_workspace, float* hyper, double beta1, double beta2,
                                   int32_t distill, void* stream) {
  return sdumc_losses_fused_reg_(B, vals, labels, th, ct, z, rnc_feats, rd, temperature, weights6, d_vals, d_th, d_ct, d_z, d_rnc,
                                 losses, distill_ws, rnc_workspace, hyper, beta1, beta2, distill, SDUMC_REGRESS_MSE, 0.f, stream);
}

#if SDUMC_LOSS_DBG
// measurement builds only: the sixteen stamp slots of the last launches (call after synchronising the stream)
extern "C" int sdumc_loss_stamps_(unsigned long long* out16) {
  if (!out16) return SDUMC_EINVAL;
  return hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_loss_stamps), 16 * sizeof(unsigned long long)) == hipSuccess ? SDUMC_OK : SDUMC_ELAUNCH;
}
#endif

extern "C" int sdumc_rnc_dfeat_rows(const float* feats, int32_t n, int32_t dim, float temperature, float weight,
                                    int32_t row0, int32_t rows, float* dfeats, float* workspace, void* stream) {
  if (!feats || !dfeats || !workspace || n < 2 || dim <= 0 || row0 < 0 || rows <= 0 || row0 + rows > n) return SDUMC_EINVAL;
  const RncWs w = rnc_ws(workspace, n);
  hipLaunchKernelGGL(rnc_dfeat_kernel, dim3(rows), dim3(256), (n + 256) * sizeof(float), as_stream(stream), feats, n,
                     dim, 1.f / temperature, weight, row0, w, dfeats);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_rnc_mask(const float* labels, int32_t n, uint8_t* mask, void* stream) {
  if (!labels || !mask || n < 2) return SDUMC_EINVAL;
  const int64_t total = (int64_t)n * (n - 1) * (n - 1);
  hipLaunchKernelGGL(rnc_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), labels, n, mask);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

// ---------------------------------------------------------------------------------------------
// SupConLoss (loss.py:143-240).  N = bsz * n_views contrast rows, view-major; A anchors = the first N ('all') or bsz ('one') rows.
// With T = 0.07 the logits span ~ +-14 and fp32 logits alone cost ~1e-6 of the gradient, which is the whole budget (the
// reference's own fp32-vs-fp64 gap): inputs and outputs are fp32, everything between them is fp64 -- N^2 * D fp64 multiply-adds,
// microseconds at the step's N = 128.  Workspace (doubles): G[A*N] = dLoss/dlogit | nrm[N] row norms | rowval[A].
//   pass 1, workgroup i: i < A: logits of anchor i against every row (one wavefront per contrast row, lanes over channels,
//           butterfly sum), row maximum, denominator without the self column, positives -> rowval[i], G[i][*]; every i: nrm[i].
//   pass 2, workgroup r < N: dL/dxhat_r = (1/T) sum_j (G[r][j] + G[j][r]) xhat_j, then the projection of F.normalize; workgroup N:
//           the mean of rowval.  Every sum has one fixed order; nothing is accumulated across workgroups.
// ---------------------------------------------------------------------------------------------
namespace {
constexpr int SUPCON_MAX_N = 2048, SUPCON_MAX_D = 1024;
constexpr double SUPCON_NORM_EPS = 1e-12;   // F.normalize's eps

// (wave_sum_d / block_sum_256_d: beside block_sum_256, at the head of the file)
__device__ __forceinline__ double block_max_256_d(double v, double* red /*[4]*/) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

struct SupconArgs {
  const float* f;        // [N, D]
  const float* labels;   // [bsz] or null
  const float* mask;     // [bsz, bsz] or null
  int bsz, N, A, D, label_mode, normalize;
  double inv_t, scale;   // 1 / T, T / base_T
  float weight;
  double *G, *nrm, *rowval;
  float* loss_out;
  float* df;             // [N, D] or null
};
// the weight of contrast row j among the positives of anchor i, self column included (the caller masks it): loss.py:180-188, :210
__device__ __forceinline__ double supcon_pos(const SupconArgs& a, int i, int j) {
  const int bi = i % a.bsz, bj = j % a.bsz;
  if (a.mask) return (double)a.mask[(size_t)bi * a.bsz + bj];
  if (!a.labels) return bi == bj ? 1.0 : 0.0;
  const float yi = a.labels[bi], yj = a.labels[bj];
  return (a.label_mode == 1 ? rintf(yi) == rintf(yj) : yi == yj) ? 1.0 : 0.0;
}
__device__ __forceinline__ double supcon_inv_norm(const SupconArgs& a, double nrm) {
  return a.normalize ? 1.0 / fmax(nrm, SUPCON_NORM_EPS) : 1.0;
}

__global__ __launch_bounds__(256) void supcon_row_kernel(const SupconArgs a) {
  extern __shared__ double smd[];   // xi[D] | lg[N]
  __shared__ double red[4];
  double* xi = smd;
  double* lg = smd + a.D;
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, D = a.D;
  const float* fi = a.f + (size_t)i * D;
  double q = 0.0;
  for (int c = lane; c < D; c += 64) {
    const double v = (double)fi[c];
    q += v * v;
  }
  const double nrm_i = sqrt(wave_sum_d(q));   // (the same bits in every wavefront)
  if (tid == 0) a.nrm[i] = nrm_i;
  if (i >= a.A) return;                       // contrast_mode 'one': the later views are no anchors
  const double inv_i = supcon_inv_norm(a, nrm_i);
  for (int c = tid; c < D; c += 256) xi[c] = (double)fi[c] * inv_i;
  __syncthreads();
  for (int j = wave; j < N; j += 4) {
    const float* fj = a.f + (size_t)j * D;
    double s = 0.0, qj = 0.0;
    for (int c = lane; c < D; c += 64) {
      const double v = (double)fj[c];
      s += xi[c] * v;
      qj += v * v;
    }
    s = wave_sum_d(s);
    qj = wave_sum_d(qj);
    if (lane == 0) lg[j] = s * supcon_inv_norm(a, sqrt(qj)) * a.inv_t;
  }
  __syncthreads();
  double mx = -INFINITY;
  for (int j = tid; j < N; j += 256) mx = fmax(mx, lg[j]);   // over every column, the anchor's own included (loss.py:206)
  mx = block_max_256_d(mx, red);
  double den = 0.0;
  for (int j = tid; j < N; j += 256) den += j == i ? 0.0 : exp(lg[j] - mx);
  den = block_sum_256_d(den, red);
  const double logden = log(den);
  // positives: m * log_prob over every column with the self column's weight forced to 0 (0 * log_prob, as loss.py:218,:235 has it)
  double cnt = 0.0, sp = 0.0;
  for (int j = tid; j < N; j += 256) {
    const double m = j == i ? 0.0 : supcon_pos(a, i, j);
    cnt += m;
    sp += m * ((lg[j] - mx) - logden);
  }
  cnt = block_sum_256_d(cnt, red);
  sp = block_sum_256_d(sp, red);
  const double pairs = cnt < 1e-6 ? 1.0 : cnt;   // an anchor without positives divides by 1 (loss.py:232-234)
  if (tid == 0) a.rowval[i] = sp / pairs;
  if (!a.df) return;
  // d loss / d logit_ij = -(T / base_T) / (A * pairs) * (m_ij - cnt * p_ij),  p_ij = exp(logit_ij - mx) / den off the diagonal
  const double k = -a.scale / ((double)a.A * pairs);
  for (int j = tid; j < N; j += 256) {
    double g = 0.0;
    if (j != i) g = k * (supcon_pos(a, i, j) - cnt * (exp(lg[j] - mx) / den));
    a.G[(size_t)i * N + j] = g;
  }
}

__global__ __launch_bounds__(256) void supcon_dfeat_kernel(const SupconArgs a) {
  extern __shared__ double smd[];   // coef[N] | g[D] | part[4][64]
  __shared__ double red[4];
  const int N = a.N, D = a.D, A = a.A;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (r == N) {   // the value: -(T / base_T) * mean over anchors
    double acc = 0.0;
    for (int i = tid; i < A; i += 256) acc += a.rowval[i];
    const double s = block_sum_256_d(acc, red);
    if (tid == 0) *a.loss_out = (float)(-a.scale * s / (double)A);
    return;
  }
  if (!a.df) return;
  double* coef = smd;
  double* g = coef + N;
  double* part = g + D;
  for (int j = tid; j < N; j += 256) {
    double cj = 0.0;
    if (r < A) cj += a.G[(size_t)r * N + j];   // r as the anchor
    if (j < A) cj += a.G[(size_t)j * N + r];   // r as a contrast row of anchor j
    coef[j] = cj * supcon_inv_norm(a, a.nrm[j]);
  }
  __syncthreads();
  for (int c0 = 0; c0 < D; c0 += 64) {
    const int c = c0 + lane;
    double acc = 0.0;
    if (c < D)
      for (int j = wave; j < N; j += 4) acc += coef[j] * (double)a.f[(size_t)j * D + c];
    part[wave * 64 + lane] = acc;
    __syncthreads();
    if (wave == 0 && c < D) g[c] = part[lane] + part[64 + lane] + part[128 + lane] + part[192 + lane];
    __syncthreads();
  }
  // through xhat = x / max(|x|, eps): (g - xhat (xhat . g)) / |x| where the norm is not clamped, g / eps where it is
  // (clamp_min passes the gradient where norm >= eps only)
  const float* fr = a.f + (size_t)r * D;
  const double nrm = a.nrm[r], inv = supcon_inv_norm(a, nrm);
  double dot = 0.0;
  if (a.normalize && nrm >= SUPCON_NORM_EPS) {
    double acc = 0.0;
    for (int c = tid; c < D; c += 256) acc += (double)fr[c] * inv * g[c];
    dot = block_sum_256_d(acc, red);
  }
  const double w = (double)a.weight * a.inv_t;
  for (int c = tid; c < D; c += 256) a.df[(size_t)r * D + c] = (float)(w * inv * (g[c] - (double)fr[c] * inv * dot));
}
}  // namespace

static int supcon_anchors(int32_t bsz, int32_t n_views, int32_t contrast_all) { return contrast_all ? bsz * n_views : bsz; }

extern "C" size_t sdumc_supcon_workspace_bytes(int32_t bsz, int32_t n_views, int32_t contrast_all) {
  if (bsz < 1 || n_views < 1 || (int64_t)bsz * n_views > SUPCON_MAX_N) return 0;
  const size_t N = (size_t)bsz * n_views, A = (size_t)supcon_anchors(bsz, n_views, contrast_all);
  return (A * N + N + A) * sizeof(double);
}

extern "C" int sdumc_supcon_fwd_bwd(const float* feats, const float* labels, const float* mask, int32_t bsz, int32_t n_views,
                                    int32_t dim, int32_t contrast_all, int32_t label_mode, int32_t normalize, double temperature,
                                    double base_temperature, float weight, float* loss_out, float* dfeats, void* workspace,
                                    void* stream) {
  if (!feats || !loss_out || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 7)) return SDUMC_EINVAL;
  if (labels && mask) return SDUMC_EINVAL;
  if (bsz < 1 || n_views < 1 || dim < 1 || dim > SUPCON_MAX_D) return SDUMC_EINVAL;
  if ((int64_t)bsz * n_views < 2 || (int64_t)bsz * n_views > SUPCON_MAX_N) return SDUMC_EINVAL;
  if (!(temperature > 0.0) || !(base_temperature > 0.0)) return SDUMC_EINVAL;
  if (label_mode < 0 || label_mode > 1 || contrast_all < 0 || contrast_all > 1 || normalize < 0 || normalize > 1) return SDUMC_EINVAL;
  SupconArgs a;
  a.f = feats; a.labels = labels; a.mask = mask;
  a.bsz = bsz; a.N = bsz * n_views; a.A = supcon_anchors(bsz, n_views, contrast_all); a.D = dim;
  a.label_mode = label_mode; a.normalize = normalize;
  a.inv_t = 1.0 / temperature; a.scale = temperature / base_temperature;
  a.weight = weight;
  a.G = static_cast<double*>(workspace);
  a.nrm = a.G + (size_t)a.A * a.N;
  a.rowval = a.nrm + a.N;
  a.loss_out = loss_out; a.df = dfeats;
  hipStream_t st = as_stream(stream);
  // LDS: at most (1024 + 2048) and (2048 + 1024 + 256) doubles = 24 / 26 KiB: under the 64 KiB a kernel gets without an attribute
  hipLaunchKernelGGL(supcon_row_kernel, dim3(a.N), dim3(256), (size_t)(a.D + a.N) * sizeof(double), st, a);
  SDUMC_CHECK_LAUNCH();
  hipLaunchKernelGGL(supcon_dfeat_kernel, dim3(a.N + 1), dim3(256), (size_t)(a.N + a.D + 256) * sizeof(double), st, a);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

SDUMC_PRELOAD_HOOK(loss)      // (common.h)
