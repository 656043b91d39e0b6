// adam.hip — torch.optim.Adam(lr, betas=(.9,.999), eps=1e-8, weight_decay=l2) with coupled L2
// (main_frame_val_text_missing.py:317) as ONE launch over the flat live-parameter bucket.
// Dead parameters (never receive a gradient) live outside the bucket and are
// never touched, exactly like torch.optim.Adam skips grad-None parameters.
// sdumc_adam_multi is the same update for the loop that keeps `optimizer = optim.Adam(model.parameters(), ...)` of
// main_frame_val_text_missing.py:317 as a line of its own (sdumc_amd/optim.py): ONE launch over the per-parameter gradient
// tensors autograd left in p.grad, found through a segment table that travels in the kernel arguments.
// sdumc_adam_step_ema is either flat-bucket launch with the averaged weights (an EMA of the parameters) riding along: one more stream,
// loaded and stored where the parameter is; sdumc_ema_multi is that rule alone over per-parameter tensors, for the loop above.
// sdumc_adamw_step / sdumc_adamw_multi are torch.optim.AdamW's rule, decoupled weight decay, as a further form of each of these launches
// (adam_decay_mul below has the rule).
// The forms of a launch (table or none, average or none, coupled or decoupled) are instantiations of ONE body per kernel shape.  What
// they promise is bits: each form gives the others' where their rules agree (a table of ones is no table, ...), and the bits of every
// form are pinned by tests/golden/adam_bits.npz, recorded from the kernels as they were before the bodies were shared.  (Through three
// added options each older form was also kept instruction for instruction; that promise cost a copy of the text per option and bought
// nothing a user sees, so it was dropped for the recorded bits.)
//
// hyper (device, 4 floats): [0] lr (host-written, LambdaLR value)   [1] step count t (kernel-incremented)
//                           [2] lr / (1 - beta1^t)                  [3] sqrt(1 - beta2^t)
// The bias corrections are derived on the device (in double, like torch's Python-side doubles) so a
// captured hipGraph replays with the right step count.
#include "common.h"
#include <string.h>

namespace {

__global__ void adam_hyper_kernel(float* hyper, double beta1, double beta2) {
  const double t = (double)hyper[1] + 1.0;
  hyper[1] = (float)t;
  hyper[2] = (float)((double)hyper[0] / (1.0 - pow(beta1, t)));
  hyper[3] = (float)sqrt(1.0 - pow(beta2, t));
}

// The update of ONE element, shared by the flat-bucket kernel and the per-parameter one (same expression = same bits):
// coupled L2, exp_avg.lerp_(grad, 1-beta1), exp_avg_sq.mul_(b2).addcmul_(g,g,1-b2), denom = sqrt(v)/bc2_sqrt + eps
__device__ __forceinline__ void adam_update(float& p, const float g, float& m, float& v, const float step_size,
                                            const float bc2_sqrt, const float beta1, const float beta2, const float eps,
                                            const float wd, const float gscale) {
  // (the two sums of two products name the product that is fused: which one the compiler contracts is otherwise its choice per
  //  kernel -- a wd held in a vector register made it the other one -- and the kernels of this file promise each other's bits.
  //  The fused one is the one adam_kernel and adam_multi_kernel got from `g * gscale + wd * p` when that was the compiler's choice.)
  const float ge = __builtin_fmaf(gscale, g, wd * p);
  m = m + (ge - m) * (1.f - beta1);
  v = __builtin_fmaf(v, beta2, (1.f - beta2) * ge * ge);
  p = p - step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
}

// Decoupled weight decay (sdumc_adamw_step, sdumc_adamw_multi; torch.optim.AdamW): p <- p * dk in front of adam_update with no L2 term,
//     dk = fp32(1 - (lr * lr_scale) * (weight_decay * wd_scale)),
// the four fp32 factors multiplied in double -- each pair's product is exact there, so one rounding for the product, one for the
// difference's conversion -- with lr = hyper[0] as the launch reads it and both scales 1 without a table.  Derived on the device, uniform
// over the launch (over a segment with a table): nothing on the host changes per step, and set_lr is followed.
__device__ __forceinline__ float adam_decay_factor(const float lr, const float lr_scale, const float wd, const float wd_scale) {
  return (float)(1.0 - ((double)lr * (double)lr_scale) * ((double)wd * (double)wd_scale));
}
// ... and the product itself, ONE fp32 multiply rounded on its own: it must not be contracted into adam_update's last subtraction (the
// kernels of this file promise each other's bits, and torch's p.mul_(1 - lr * wd) rounds here)
__device__ __forceinline__ float adam_decay_mul(const float p, const float dk) {
#pragma clang fp contract(off)
  return p * dk;
}
// What one element's update is made of: uniform over a launch, or with a table over a segment.  ew: the average's weight (read by the
// EMA forms only), dk: the decay factor (by the decoupled forms only).
struct adam_consts {
  float step_size, bc2_sqrt, beta1, beta2, eps, wd, gscale, ew, dk;
};
// adam_update (DEC false: wd is the coupled L2 factor, dk is not read) or its decoupled form (DEC true: dk, and wd is not read)
template <bool DEC>
__device__ __forceinline__ void adam_update_d(float& p, const float g, float& m, float& v, const adam_consts& c) {
  if constexpr (DEC) {
    p = adam_decay_mul(p, c.dk);
    adam_update(p, g, m, v, c.step_size, c.bc2_sqrt, c.beta1, c.beta2, c.eps, 0.f, c.gscale);
  } else {
    adam_update(p, g, m, v, c.step_size, c.bc2_sqrt, c.beta1, c.beta2, c.eps, c.wd, c.gscale);
  }
}

// The averaged weights (sdumc_adam_step_ema, sdumc_ema_multi): torch.lerp(a, p, w)'s own rule in fp32, with the product that is fused
// named (as in adam_update: the kernels of this file promise each other's bits).  With w = 0.25, 0.5 or 1 the product is exact and
// the result is torch.lerp's bit for bit; w = 1 gives p's bits.
__device__ __forceinline__ float ema_lerp(const float a, const float p, const float w) {
  const float d = p - a;
  return w < 0.5f ? __builtin_fmaf(w, d, a) : __builtin_fmaf(-d, 1.f - w, p);
}
// w = fp32(1 - d_eff) in double, rounded once; warm-up: d_eff = min(decay, (1 + t) / (10 + t)) with t = the step count as this
// launch sees it (hyper[1] after the step's increment).  Uniform over the launch: nothing on the host changes per step.
__device__ __forceinline__ float ema_weight(const float* hyper, const float decay, const int warmup) {
  double d = (double)decay;
  if (warmup) {
    const double t = (double)hyper[1];
    const double dw = (1.0 + t) / (10.0 + t);
    d = dw < d ? dw : d;
  }
  return (float)(1.0 - d);
}

// ONE element through memory: every scalar path of this file (the scalar tails, the per-element path at segment boundaries, the ragged
// ends and unaligned tensors of the per-parameter kernel).  EMA: the average is read where the parameter is, and the lerp is fed the
// parameter value just computed, from its register.
template <bool EMA, bool DEC>
__device__ __forceinline__ void adam_update1(float* p, const float* g, float* m, float* v, float* a, const int64_t t,
                                             const adam_consts& c) {
  if constexpr (EMA) {
    float pe = p[t], me = m[t], ve = v[t];
    const float ae = a[t];
    adam_update_d<DEC>(pe, g[t], me, ve, c);
    p[t] = pe; m[t] = me; v[t] = ve;
    a[t] = ema_lerp(ae, pe, c.ew);
  } else {
    adam_update_d<DEC>(p[t], g[t], m[t], v[t], c);
  }
}
// 16 bytes of ONE tensor (or of padding) at element e0: every vector path of this file.  EMA: a fifth stream `a`, loaded and stored in
// 16-byte groups exactly where p is.
template <bool EMA, bool DEC>
__device__ __forceinline__ void adam_update4(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, float* __restrict__ a, const int64_t e0, const adam_consts& c) {
  f32x4 pp = *reinterpret_cast<f32x4*>(p + e0);
  const f32x4 gg = *reinterpret_cast<const f32x4*>(g + e0);
  f32x4 mm = *reinterpret_cast<f32x4*>(m + e0);
  f32x4 vv = *reinterpret_cast<f32x4*>(v + e0);
  f32x4 aa;
  if constexpr (EMA) aa = *reinterpret_cast<f32x4*>(a + e0);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float pe = pp[e], me = mm[e], ve = vv[e];
    adam_update_d<DEC>(pe, gg[e], me, ve, c);
    pp[e] = pe; mm[e] = me; vv[e] = ve;
    if constexpr (EMA) aa[e] = ema_lerp(aa[e], pe, c.ew);
  }
  *reinterpret_cast<f32x4*>(p + e0) = pp;
  *reinterpret_cast<f32x4*>(m + e0) = mm;
  *reinterpret_cast<f32x4*>(v + e0) = vv;
  if constexpr (EMA) *reinterpret_cast<f32x4*>(a + e0) = aa;
}

// The average of a flat-bucket launch, behind the arguments every form takes: the buffer (nullptr: none), the decay, the warm-up flag.
struct ema_opts { float* a; float decay; int warmup; };
// A launch's constants from its arguments: the bias corrections of hyper, the average's weight (EMA), the decay factor of an element of
// no segment (DEC).
template <bool EMA, bool DEC>
__device__ __forceinline__ adam_consts launch_consts(const float* hyper, float beta1, float beta2, float eps, float wd, float gscale,
                                                     const ema_opts& ea) {
  adam_consts c{hyper[2], hyper[3], beta1, beta2, eps, wd, gscale, 0.f, 0.f};
  if constexpr (EMA) c.ew = ema_weight(hyper, ea.decay, ea.warmup);
  if constexpr (DEC) c.dk = adam_decay_factor(hyper[0], 1.f, wd, 1.f);
  return c;
}
// What thread 0 of a flat-bucket launch does beside its elements: the dropout call counter (every reader of this step is ordered
// before this launch) and the step's weighted total (main :149), for the caller's read-back: the six terms were final long ago
__device__ __forceinline__ void step_tail(uint32_t* rng, const uint32_t rng_inc, const sdumc_total_loss& tl, const bool poisoned) {
  if (rng) rng[2] += rng_inc;
  if (tl.losses) {
    float* L = tl.losses;
    L[0] = tl.w[0] * L[1] + tl.w[1] * L[2] + tl.w[2] * L[3] + tl.w[3] * L[4] + tl.w[4] * L[5] + tl.w[5] * L[6];
    L[7] = 0.f;
    // fail loudly: a clustered utterance-level kernel whose spin ran into its cap finished with wrong data
    if (poisoned) { L[0] = __int_as_float(0x7fc00000); L[7] = 1.f; }
  }
}

// Thread i owns the 16-byte group [4 i, 4 i + 4) of the bucket; thread 0 also has step_tail and the up to three elements behind the
// last group.  EMA: the average travels with the parameter; DEC: decoupled weight decay, one factor for the whole launch.
template <bool EMA, bool DEC>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n4,
                                                   int64_t n, const float* hyper, float beta1, float beta2, float eps,
                                                   float wd, float gscale, uint32_t* rng, uint32_t rng_inc,
                                                   const sdumc_total_loss tl, const ema_opts ea) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // A clustered utterance-level kernel whose spin ran into its cap finished with wrong data: the gradients of this step are
  // garbage, so NOTHING is applied -- parameters and moments stay as they were (every thread reads the word; it is sticky
  // until sdumc_chain_cluster_reset_error)
  const bool poisoned = tl.chain_err != nullptr && *tl.chain_err != 0;
  // ... and a step sdumc_grad_guard skipped (non-finite gradients, guard[3]) applies nothing either; its dropout counter and its
  // total below are those of a finite step
  const bool hold = poisoned || (tl.guard != nullptr && tl.guard[3] != 0.f);
  const adam_consts c = launch_consts<EMA, DEC>(hyper, beta1, beta2, eps, wd, gscale, ea);
  float* __restrict__ a = ea.a;
  if (i < n4 && !hold) adam_update4<EMA, DEC>(p, g, m, v, a, 4 * i, c);
  if (i == 0) {
    step_tail(rng, rng_inc, tl, poisoned);
    for (int64_t t = n4 * 4; t < n && !hold; ++t) adam_update1<EMA, DEC>(p, g, m, v, a, t, c);
  }
}

// Workgroup b's place in a table of running workgroup counts (adam_multi_kernel, ema_multi_kernel, zero_segments_kernel): the first
// segment with block_end > b, and which of that segment's chunks b is.  The table is a kernel argument, every lookup is a scalar load
// with a wave-uniform index.  (Two steps, so that a kernel asks for its segment's record between them: the record's load and the
// load of block_end[seg - 1] are then in flight together.)
__device__ __forceinline__ int chunk_segment(const uint32_t* block_end, const int nseg, const uint32_t b) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (block_end[mid] > b) hi = mid; else lo = mid + 1;
  }
  return lo;
}
__device__ __forceinline__ uint32_t chunk_index(const uint32_t* block_end, const int seg, const uint32_t b) {
  return b - (seg > 0 ? block_end[seg - 1] : 0u);
}

// The same update over per-parameter tensors (sdumc_adam_multi; DEC: sdumc_adamw_multi, one factor for the whole launch): workgroup b
// finds its (segment, chunk of SDUMC_ADAM_CHUNK elements) with chunk_segment and chunk_index.  A chunk starts a multiple of 4 KiB behind its segment's
// base, so the segment's alignment is the chunk's: 16 bytes per lane where param, grad and both moments are 16-byte aligned, one float
// per lane (stride 256, coalesced) elsewhere.
template <bool DEC>
__global__ __launch_bounds__(256) void adam_multi_kernel(const sdumc_adam_table tb, float* __restrict__ m_all,
                                                         float* __restrict__ v_all, const float* hyper, float beta1,
                                                         float beta2, float eps, float wd, float gscale,
                                                         const int32_t* chain_err) {
  if (chain_err != nullptr && *chain_err != 0) return;     // garbage gradients (see adam_kernel): NOTHING is applied
  const adam_consts c = launch_consts<false, DEC>(hyper, beta1, beta2, eps, wd, gscale, ema_opts{nullptr, 0.f, 0});
  const int seg = chunk_segment(tb.block_end, tb.nseg, blockIdx.x);
  const sdumc_adam_seg sg = tb.seg[seg];
  const int64_t base = (int64_t)chunk_index(tb.block_end, seg, blockIdx.x) * SDUMC_ADAM_CHUNK;
  const int64_t left = sg.n - base;
  const int cnt = left < SDUMC_ADAM_CHUNK ? (int)left : SDUMC_ADAM_CHUNK;
  float* __restrict__ p = sg.param + base;
  const float* __restrict__ g = sg.grad + base;
  float* __restrict__ m = m_all + sg.state_offset + base;
  float* __restrict__ v = v_all + sg.state_offset + base;
  const int tid = threadIdx.x;
  const bool aligned = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                         reinterpret_cast<uintptr_t>(v)) & 15) == 0;
  if (aligned) {
    const int e0 = 4 * tid;
    if (e0 + 4 <= cnt) {
      adam_update4<false, DEC>(p, g, m, v, nullptr, e0, c);
    } else {
      for (int e = e0; e < cnt; ++e) adam_update1<false, DEC>(p, g, m, v, nullptr, e, c);
    }
  } else {
    for (int e = tid; e < cnt; e += 256) adam_update1<false, DEC>(p, g, m, v, nullptr, e, c);
  }
}

// Per-tensor learning rates, decay and frozen tensors (sdumc_adam_step_rates): adam_kernel's launch over the flat bucket, with each
// element's tensor found through a segment table that travels in the kernel arguments.  The table is a kernel argument, so a lookup
// with a wave-uniform index is a scalar load.
struct rates_table {
  sdumc_rate_seg seg[SDUMC_RATES_MAX_SEGS];
  int32_t nseg;
};
__device__ __forceinline__ int64_t seg_end(const rates_table& tb, int s) { return tb.seg[s].offset + tb.seg[s].n; }
// the first segment that ends behind element e (nseg: none does): e lies in it, or in the padding in front of it
__device__ __forceinline__ int first_seg_behind(const rates_table& tb, int64_t e) {
  int lo = 0, hi = tb.nseg;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (seg_end(tb, mid) > e) hi = mid; else lo = mid + 1;
  }
  return lo;
}
// A segment's constants from the launch's: its two scales applied to step size and coupled L2 factor.  Decoupled (DEC, lr0 =
// hyper[0]): its factor is adam_decay_factor of its two scales, derived where a path needs it; the coupled forms read neither.  An
// element of no segment (alignment padding) has scales 1: the default update, and the factor of sdumc_adamw_step without a table.
template <bool DEC>
__device__ __forceinline__ adam_consts seg_consts(const adam_consts& c, const float lr0, const float lr_scale, const float wd_scale) {
  adam_consts o = c;
  o.step_size = c.step_size * lr_scale;
  o.wd = c.wd * wd_scale;
  if constexpr (DEC) o.dk = adam_decay_factor(lr0, lr_scale, c.wd, wd_scale);
  return o;
}// ONE element, on the per-element path.  s: the first segment that ends behind some element at or in front of t; moved on to t's.
// An element of a frozen segment is neither read nor written -- nor is its average.
template <bool EMA, bool DEC>
__device__ __forceinline__ void adam_rates_one(const rates_table& tb, int& s, const int64_t t, float* __restrict__ p,
                                               const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                               float* __restrict__ a, const adam_consts& c, const float lr0) {
  while (s < tb.nseg && seg_end(tb, s) <= t) ++s;
  float lr_scale = 1.f, wd_scale = 1.f;
  if (s < tb.nseg && tb.seg[s].offset <= t) {
    if (tb.seg[s].frozen) return;
    lr_scale = tb.seg[s].lr_scale;
    wd_scale = tb.seg[s].wd_scale;
  }
  adam_update1<EMA, DEC>(p, g, m, v, a, t, seg_consts<DEC>(c, lr0, lr_scale, wd_scale));
}

// Thread i owns the 16-byte group [4 i, 4 i + 4) of the bucket, as in adam_kernel.  A wave whose 256 elements lie inside one segment
// (all but a handful: the tensors are thousands of elements long) finds it with a scalar binary search and takes its scales from
// scalar registers; a frozen segment's waves leave without touching memory.  In a wave that meets a boundary every lane walks on from
// the wave's segment to its own: a group inside one segment (or inside padding) still moves 16 bytes, a group that straddles a boundary
// -- segments start at any residue mod 4 -- goes element by element.  Holds and scalar tail are adam_kernel's; EMA and DEC as there,
// on every one of these paths.
template <bool EMA, bool DEC>
__global__ __launch_bounds__(256) void adam_rates_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, int64_t n4, int64_t n,
                                                         const float* hyper, float beta1, float beta2, float eps, float wd,
                                                         float gscale, uint32_t* rng, uint32_t rng_inc, const sdumc_total_loss tl,
                                                         const rates_table tb, const ema_opts ea) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool poisoned = tl.chain_err != nullptr && *tl.chain_err != 0;                   // (see adam_kernel)
  const bool hold = poisoned || (tl.guard != nullptr && tl.guard[3] != 0.f);
  const adam_consts c = launch_consts<EMA, false>(hyper, beta1, beta2, eps, wd, gscale, ea);      // (dk: seg_consts', per path)
  float* __restrict__ a = ea.a;
  float lr0 = 0.f;
  if constexpr (DEC) lr0 = hyper[0];
  // the wave's first element and the first segment that ends behind it: scalar registers, scalar loads
  const int64_t w0 = 4 * ((int64_t)blockIdx.x * blockDim.x + __builtin_amdgcn_readfirstlane((int)threadIdx.x));
  const int s0 = first_seg_behind(tb, w0);
  if (i < n4 && !hold) {
    const int64_t e0 = 4 * i;
    if (s0 < tb.nseg && tb.seg[s0].offset <= w0 && w0 + 256 <= seg_end(tb, s0)) {        // (wave-uniform)
      if (!tb.seg[s0].frozen)
        adam_update4<EMA, DEC>(p, g, m, v, a, e0, seg_consts<DEC>(c, lr0, tb.seg[s0].lr_scale, tb.seg[s0].wd_scale));
    } else {
      int s = s0;
      while (s < tb.nseg && seg_end(tb, s) <= e0) ++s;
      const bool padding = s == tb.nseg || tb.seg[s].offset >= e0 + 4;                   // the group meets no segment
      if (padding) {
        adam_update4<EMA, DEC>(p, g, m, v, a, e0, seg_consts<DEC>(c, lr0, 1.f, 1.f));
      } else if (tb.seg[s].offset <= e0 && e0 + 4 <= seg_end(tb, s)) {                   // ... lies inside one
        if (!tb.seg[s].frozen)
          adam_update4<EMA, DEC>(p, g, m, v, a, e0, seg_consts<DEC>(c, lr0, tb.seg[s].lr_scale, tb.seg[s].wd_scale));
      } else {                                                                           // ... straddles a boundary
        for (int e = 0; e < 4; ++e) adam_rates_one<EMA, DEC>(tb, s, e0 + e, p, g, m, v, a, c, lr0);
      }
    }
  }
  if (i == 0) {
    step_tail(rng, rng_inc, tl, poisoned);
    if (!hold && n4 * 4 < n) {
      int s = first_seg_behind(tb, n4 * 4);
      for (int64_t t = n4 * 4; t < n; ++t) adam_rates_one<EMA, DEC>(tb, s, t, p, g, m, v, a, c, lr0);
    }
  }
}

// The averaged weights of the loop that keeps the module (sdumc_ema_multi): ema_lerp over per-parameter tensors, found like
// adam_multi_kernel's -- workgroup b's (segment, chunk of SDUMC_ADAM_CHUNK elements) with chunk_segment and chunk_index, 16 bytes per lane where both
// addresses are 16-byte aligned, one float per lane elsewhere; the same bits either way.
struct ema_table {
  sdumc_ema_seg seg[SDUMC_ADAM_MAX_SEGS];
  uint32_t block_end[SDUMC_ADAM_MAX_SEGS];
  int32_t nseg;
};
__global__ __launch_bounds__(256) void ema_multi_kernel(const ema_table tb, const float w) {
  const int seg = chunk_segment(tb.block_end, tb.nseg, blockIdx.x);
  const sdumc_ema_seg sg = tb.seg[seg];
  const int64_t base = (int64_t)chunk_index(tb.block_end, seg, blockIdx.x) * SDUMC_ADAM_CHUNK;
  const int64_t left = sg.n - base;
  const int cnt = left < SDUMC_ADAM_CHUNK ? (int)left : SDUMC_ADAM_CHUNK;
  float* __restrict__ a = sg.ema + base;
  const float* __restrict__ p = sg.param + base;
  const int tid = threadIdx.x;
  const bool aligned = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(p)) & 15) == 0;
  if (aligned) {
    const int e0 = 4 * tid;
    if (e0 + 4 <= cnt) {
      f32x4 aa = *reinterpret_cast<f32x4*>(a + e0);
      const f32x4 pp = *reinterpret_cast<const f32x4*>(p + e0);
#pragma unroll
      for (int e = 0; e < 4; ++e) aa[e] = ema_lerp(aa[e], pp[e], w);
      *reinterpret_cast<f32x4*>(a + e0) = aa;
    } else {
      for (int e = e0; e < cnt; ++e) a[e] = ema_lerp(a[e], p[e], w);
    }
  } else {
    for (int e = tid; e < cnt; e += 256) a[e] = ema_lerp(a[e], p[e], w);
  }
}

// +0.0f over the frozen segments of a bucket (sdumc_zero_segments).  The launch's table holds the frozen segments only; workgroup b
// finds its (segment, chunk) with chunk_segment and chunk_index.  A segment's whole 16-byte groups are split into chunks of ZERO_CHUNK elements, 16 bytes
// per store; its first workgroup also writes the up to three elements in front of the first whole group and behind the last, one float
// per lane.
constexpr int ZERO_CHUNK = 4096;
struct zero_table {
  int64_t offset[SDUMC_RATES_MAX_SEGS], n[SDUMC_RATES_MAX_SEGS];
  uint32_t block_end[SDUMC_RATES_MAX_SEGS];
  int32_t nseg;
};
__host__ __device__ inline int64_t zero_groups_begin(int64_t first) { return (first + 3) & ~(int64_t)3; }
__global__ __launch_bounds__(256) void zero_segments_kernel(float* __restrict__ buf, const zero_table tb) {
  const int seg = chunk_segment(tb.block_end, tb.nseg, blockIdx.x);
  const int64_t k = chunk_index(tb.block_end, seg, blockIdx.x);
  const int64_t first = tb.offset[seg], last = first + tb.n[seg];
  const int64_t a = zero_groups_begin(first), z = last & ~(int64_t)3;      // the whole groups: [a, z), none when a >= z
  const int tid = threadIdx.x;
  const int64_t c1 = a + (k + 1) * ZERO_CHUNK < z ? a + (k + 1) * ZERO_CHUNK : z;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int64_t e = a + k * ZERO_CHUNK + 4 * tid; e < c1; e += 4 * 256) *reinterpret_cast<f32x4*>(buf + e) = zero;
  if (k == 0) {
    const int64_t head_end = a < last ? a : last;           // [first, head_end): in front of the first whole group
    if (first + tid < head_end) buf[first + tid] = 0.f;
    const int64_t tail = z > head_end ? z : head_end;       // [tail, last): behind the last one
    if (tail + tid < last) buf[tail + tid] = 0.f;
  }
}

// what every entry asks of a table: 1 .. SDUMC_RATES_MAX_SEGS segments, ascending, disjoint, inside [0, n), scales finite and >= 0
int rates_table_check(const sdumc_rate_seg* segs, int32_t nseg, int64_t n) {
  if (!segs || nseg < 1 || nseg > SDUMC_RATES_MAX_SEGS || n <= 0) return SDUMC_EINVAL;
  int64_t end = 0;
  for (int32_t i = 0; i < nseg; ++i) {
    const sdumc_rate_seg& s = segs[i];
    if (s.n < 1 || s.n > n || s.offset < end || s.offset > n - s.n) return SDUMC_EINVAL;
    if (!(s.lr_scale >= 0.f) || !(s.wd_scale >= 0.f) || s.lr_scale > 3.402823466e38f || s.wd_scale > 3.402823466e38f)
      return SDUMC_EINVAL;
    end = s.offset + s.n;
  }
  return SDUMC_OK;
}

bool misaligned16(const void* a, const void* b, const void* c, const void* d) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
           reinterpret_cast<uintptr_t>(d)) & 15) != 0;
}

// the flat-bucket kernel of this form, with the table or without
template <bool EMA, bool DEC>
void launch_flat(const sdumc_adam_launch& L, const sdumc_total_loss& tl, const rates_table* tb, void* stream) {
  const int64_t n4 = L.n / 4;
  const int64_t threads = n4 > 0 ? n4 : 1;
  const dim3 grid((unsigned)((threads + 255) / 256));
  const ema_opts ea{L.ema, L.ema_decay, L.ema_warmup != 0 ? 1 : 0};
  if (tb)
    hipLaunchKernelGGL((adam_rates_kernel<EMA, DEC>), grid, dim3(256), 0, as_stream(stream), L.param, L.grad, L.exp_avg, L.exp_avg_sq,
                       n4, L.n, L.hyper, L.beta1, L.beta2, L.eps, L.weight_decay, L.grad_scale, L.rng_state, L.rng_inc, tl, *tb, ea);
  else
    hipLaunchKernelGGL((adam_kernel<EMA, DEC>), grid, dim3(256), 0, as_stream(stream), L.param, L.grad, L.exp_avg, L.exp_avg_sq, n4,
                       L.n, L.hyper, L.beta1, L.beta2, L.eps, L.weight_decay, L.grad_scale, L.rng_state, L.rng_inc, tl, ea);
}

}  // namespace

extern "C" int sdumc_adam_hyper_(float* hyper, float beta1, float beta2, void* stream) {
  if (!hyper) return SDUMC_EINVAL;
  hipLaunchKernelGGL(adam_hyper_kernel, dim3(1), dim3(1), 0, as_stream(stream), hyper, (double)beta1, (double)beta2);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_adam_check_(const sdumc_adam_launch* L) {
  if (!L || !L->param || !L->grad || !L->exp_avg || !L->exp_avg_sq || !L->hyper || L->n <= 0) return SDUMC_EINVAL;
  if (misaligned16(L->param, L->grad, L->exp_avg, L->exp_avg_sq)) return SDUMC_EINVAL;
  if (L->segs != nullptr || L->nseg != 0) {      // (a table without a count, and the reverse, are refused by the table's check)
    const int rc = rates_table_check(L->segs, L->nseg, L->n);
    if (rc) return rc;
  }
  if (L->ema) {      // a 16-byte aligned buffer of n floats that is not the parameters', a decay in [0, 1]
    if (reinterpret_cast<uintptr_t>(L->ema) & 15) return SDUMC_EINVAL;
    if (!(L->ema_decay >= 0.f && L->ema_decay <= 1.f)) return SDUMC_EINVAL;      // (NaN fails both)
    const uintptr_t a = reinterpret_cast<uintptr_t>(L->ema), p = reinterpret_cast<uintptr_t>(L->param), bytes = (uintptr_t)L->n * 4u;
    if (a < p + bytes && p < a + bytes) return SDUMC_EINVAL;                     // the two ranges overlap
  } else if (L->ema_decay != 0.f || L->ema_warmup != 0) {      // options of an average without one (a NaN decay compares unequal too)
    return SDUMC_EINVAL;
  }
  if (L->decoupled != 0 && L->decoupled != 1) return SDUMC_EINVAL;
  return SDUMC_OK;
}

extern "C" int sdumc_adam_apply_(const sdumc_adam_launch* L, void* stream) {
  static_assert(sizeof(rates_table) + sizeof(sdumc_total_loss) + 152 <= 4096, "the table travels in the kernel arguments (4 KB)");
  const int rc = sdumc_adam_check_(L);
  if (rc) return rc;
  sdumc_total_loss tl{};      // (no loss record, no weights, no guard)
  if (L->total) tl = *L->total;
  // (callers without a loss record -- the data-parallel step, the public entries -- are guarded by the device's error word too)
  if (!tl.chain_err) tl.chain_err = sdumc_chain_cluster_err_ptr_();
  rates_table tb;
  if (L->nseg != 0) {
    memset(&tb, 0, sizeof(tb));
    tb.nseg = L->nseg;
    for (int32_t i = 0; i < L->nseg; ++i) tb.seg[i] = L->segs[i];
  }
  const rates_table* table = L->nseg != 0 ? &tb : nullptr;
  if (L->ema && L->decoupled) launch_flat<true, true>(*L, tl, table, stream);
  else if (L->ema) launch_flat<true, false>(*L, tl, table, stream);
  else if (L->decoupled) launch_flat<false, true>(*L, tl, table, stream);
  else launch_flat<false, false>(*L, tl, table, stream);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

namespace {
// A public flat-bucket entry, behind its own precondition: every refusal before the step count advances, then the bias corrections,
// then the launch.  The entries' records name no dropout counter and no loss record (the three fields in front of `segs`).
int adam_step_entry(const sdumc_adam_launch& L, float* hyper, void* stream) {
  int rc = sdumc_adam_check_(&L);
  if (rc) return rc;
  rc = sdumc_adam_hyper_(hyper, L.beta1, L.beta2, stream);
  if (rc) return rc;
  return sdumc_adam_apply_(&L, stream);
}
}  // namespace

extern "C" int sdumc_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                               float* hyper, float beta1, float beta2, float eps, float weight_decay,
                               float grad_scale, void* stream) {
  return adam_step_entry({param, grad, exp_avg, exp_avg_sq, n, hyper, beta1, beta2, eps, weight_decay, grad_scale, nullptr, 0u, nullptr,
                          nullptr, 0, nullptr, 0.f, 0, 0}, hyper, stream);
}

extern "C" int sdumc_adam_step_rates(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* hyper,
                                     float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                     const sdumc_rate_seg* segs, int32_t nseg, void* stream) {
  if (!segs || nseg < 1) return SDUMC_EINVAL;      // (this entry's own: a table)
  return adam_step_entry({param, grad, exp_avg, exp_avg_sq, n, hyper, beta1, beta2, eps, weight_decay, grad_scale, nullptr, 0u, nullptr,
                          segs, nseg, nullptr, 0.f, 0, 0}, hyper, stream);
}

extern "C" int sdumc_adam_step_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* hyper,
                                   float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                   const sdumc_rate_seg* segs, int32_t nseg, float* ema, float ema_decay, int32_t ema_warmup,
                                   void* stream) {
  if (!ema) return SDUMC_EINVAL;      // (this entry's own: an average)
  return adam_step_entry({param, grad, exp_avg, exp_avg_sq, n, hyper, beta1, beta2, eps, weight_decay, grad_scale, nullptr, 0u, nullptr,
                          segs, nseg, ema, ema_decay, ema_warmup, 0}, hyper, stream);
}

extern "C" int sdumc_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* hyper,
                                float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                const sdumc_rate_seg* segs, int32_t nseg, float* ema, float ema_decay, int32_t ema_warmup,
                                void* stream) {
  return adam_step_entry({param, grad, exp_avg, exp_avg_sq, n, hyper, beta1, beta2, eps, weight_decay, grad_scale, nullptr, 0u, nullptr,
                          segs, nseg, ema, ema_decay, ema_warmup, 1}, hyper, stream);
}

namespace {
// The per-parameter launches (sdumc_adam_multi, sdumc_adamw_multi, sdumc_ema_multi) walk their segment list in groups of
// SDUMC_ADAM_MAX_SEGS, one launch each.  multi_grids_ok: no group's chunks of SDUMC_ADAM_CHUNK elements exceed one launch's grid (asked
// before anything is enqueued; every n > 0).  multi_table: the table of the group that starts at segs[s0] -> its workgroups.
template <class Seg>
bool multi_grids_ok(const Seg* segs, int32_t nseg) {
  uint64_t blocks = 0;
  for (int32_t i = 0; i < nseg; ++i) {
    if (i % SDUMC_ADAM_MAX_SEGS == 0) blocks = 0;
    blocks += (uint64_t)((segs[i].n + SDUMC_ADAM_CHUNK - 1) / SDUMC_ADAM_CHUNK);
    if (blocks > 0x7fffffffull) return false;
  }
  return true;
}
template <class Table, class Seg>
uint32_t multi_table(Table& tb, const Seg* segs, int32_t nseg, int32_t s0) {
  memset(&tb, 0, sizeof(tb));      // (segments behind the last one: null pointers, no elements)
  tb.nseg = nseg - s0 < SDUMC_ADAM_MAX_SEGS ? nseg - s0 : SDUMC_ADAM_MAX_SEGS;
  uint32_t blocks = 0;
  for (int32_t i = 0; i < SDUMC_ADAM_MAX_SEGS; ++i) {
    if (i < tb.nseg) {
      tb.seg[i] = segs[s0 + i];
      blocks += (uint32_t)((tb.seg[i].n + SDUMC_ADAM_CHUNK - 1) / SDUMC_ADAM_CHUNK);
    }
    tb.block_end[i] = blocks;
  }
  return blocks;
}

// sdumc_adam_multi (DEC false) and sdumc_adamw_multi (true): the same refusals, tables and grids, the kernel of either rule
template <bool DEC>
int adam_multi_launch(const sdumc_adam_seg* segs, int32_t nseg, float* exp_avg, float* exp_avg_sq, int64_t state_len, float* hyper,
                      float beta1, float beta2, float eps, float weight_decay, float grad_scale, void* stream) {
  static_assert(sizeof(sdumc_adam_table) + 64 <= 4096, "the table travels in the kernel arguments (4 KB)");
  if (!segs || nseg <= 0 || !exp_avg || !exp_avg_sq || !hyper || state_len <= 0) return SDUMC_EINVAL;
  for (int32_t i = 0; i < nseg; ++i) {
    const sdumc_adam_seg& s = segs[i];
    if (!s.param || !s.grad || s.n <= 0 || s.state_offset < 0 || s.state_offset > state_len || s.n > state_len - s.state_offset)
      return SDUMC_EINVAL;
  }
  if (!multi_grids_ok(segs, nseg)) return SDUMC_EINVAL;
  int rc = sdumc_adam_hyper_(hyper, beta1, beta2, stream);
  if (rc) return rc;
  const int32_t* chain_err = sdumc_chain_cluster_err_ptr_();
  for (int32_t s0 = 0; s0 < nseg; s0 += SDUMC_ADAM_MAX_SEGS) {
    sdumc_adam_table tb;
    const uint32_t blocks = multi_table(tb, segs, nseg, s0);
    hipLaunchKernelGGL(adam_multi_kernel<DEC>, dim3(blocks), dim3(256), 0, as_stream(stream), tb, exp_avg, exp_avg_sq, hyper, beta1,
                       beta2, eps, weight_decay, grad_scale, chain_err);
    SDUMC_CHECK_LAUNCH();
  }
  return SDUMC_OK;
}
}  // namespace

extern "C" int sdumc_adam_multi(const sdumc_adam_seg* segs, int32_t nseg, float* exp_avg, float* exp_avg_sq, int64_t state_len,
                                float* hyper, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                void* stream) {
  return adam_multi_launch<false>(segs, nseg, exp_avg, exp_avg_sq, state_len, hyper, beta1, beta2, eps, weight_decay, grad_scale,
                                  stream);
}

extern "C" int sdumc_adamw_multi(const sdumc_adam_seg* segs, int32_t nseg, float* exp_avg, float* exp_avg_sq, int64_t state_len,
                                 float* hyper, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                 void* stream) {
  return adam_multi_launch<true>(segs, nseg, exp_avg, exp_avg_sq, state_len, hyper, beta1, beta2, eps, weight_decay, grad_scale,
                                 stream);
}

extern "C" int sdumc_ema_multi(const sdumc_ema_seg* segs, int32_t nseg, float weight, void* stream) {
  static_assert(sizeof(ema_table) + 64 <= 4096, "the table travels in the kernel arguments (4 KB)");
  if (!segs || nseg <= 0 || !(weight >= 0.f && weight <= 1.f)) return SDUMC_EINVAL;
  for (int32_t i = 0; i < nseg; ++i) {
    const sdumc_ema_seg& s = segs[i];
    if (!s.ema || !s.param || s.n <= 0 || (reinterpret_cast<uintptr_t>(s.ema) & 3) || (reinterpret_cast<uintptr_t>(s.param) & 3))
      return SDUMC_EINVAL;
  }
  if (!multi_grids_ok(segs, nseg)) return SDUMC_EINVAL;
  for (int32_t s0 = 0; s0 < nseg; s0 += SDUMC_ADAM_MAX_SEGS) {
    ema_table tb;
    const uint32_t blocks = multi_table(tb, segs, nseg, s0);
    hipLaunchKernelGGL(ema_multi_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), tb, weight);
    SDUMC_CHECK_LAUNCH();
  }
  return SDUMC_OK;
}

extern "C" int sdumc_zero_segments(float* buf, int64_t n, const sdumc_rate_seg* segs, int32_t nseg, void* stream) {
  static_assert(sizeof(zero_table) + 64 <= 4096, "the table travels in the kernel arguments (4 KB)");
  if (!buf || (reinterpret_cast<uintptr_t>(buf) & 15)) return SDUMC_EINVAL;
  const int rc = rates_table_check(segs, nseg, n);
  if (rc) return rc;
  zero_table tb;
  memset(&tb, 0, sizeof(tb));
  uint64_t blocks = 0;
  for (int32_t i = 0; i < nseg; ++i) {
    if (!segs[i].frozen) continue;
    const int64_t a = zero_groups_begin(segs[i].offset), z = (segs[i].offset + segs[i].n) & ~(int64_t)3;
    const int64_t chunks = z > a ? (z - a + ZERO_CHUNK - 1) / ZERO_CHUNK : 0;
    blocks += (uint64_t)(chunks > 0 ? chunks : 1);
    if (blocks > 0x7fffffffull) return SDUMC_EINVAL;      // (one launch's grid)
    tb.offset[tb.nseg] = segs[i].offset;
    tb.n[tb.nseg] = segs[i].n;
    tb.block_end[tb.nseg++] = (uint32_t)blocks;
  }
  if (tb.nseg == 0) return SDUMC_OK;
  for (int32_t i = tb.nseg; i < SDUMC_RATES_MAX_SEGS; ++i) tb.block_end[i] = (uint32_t)blocks;
  hipLaunchKernelGGL(zero_segments_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), buf, tb);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

SDUMC_PRELOAD_HOOK(adam)      // (common.h)
