// elementwise.hip — the small fused element-wise / reduction kernels of the utterance-level
// network (model :293-368) and of its backward.  All HBM/L2-streaming: 16-B accesses where the
// layout allows, wave64 shuffles for the per-sample dot products.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "scatter_rows.h"

namespace {

constexpr int D = SDUMC_D;
constexpr int H = SDUMC_H;
constexpr int NQ = SDUMC_NQ;

__global__ void relu_drop_bwd_kernel(const float* dy, const float* y, float scale, float* dz, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dz[i] = y[i] > 0.f ? dy[i] * scale : 0.f;
}
__global__ void relu_drop_bwd_add_kernel(const float* dy, const float* y, float scale, float* dz, int64_t n,
                                         const float* add, int row_len, int col0, int width) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float g = dy[i];
  const int64_t row = i / row_len;
  const int col = (int)(i - row * row_len) - col0;
  if (col >= 0 && col < width) g += add[row * width + col];
  dz[i] = y[i] > 0.f ? g * scale : 0.f;
}

// ---- column sums -------------------------------------------------------------------------
constexpr int CS_ROWS = 512;  // rows per first-stage chunk
__global__ __launch_bounds__(256) void colsum_stage1(const float* a, int64_t rows, int cols, int lda, float* part) {
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.y * CS_ROWS;
  const int64_t r1 = min(rows, r0 + CS_ROWS);
  float acc = 0.f;
  if (c < cols)
    for (int64_t r = r0 + rl; r < r1; r += 4) acc += a[r * lda + c];
  red[rl][threadIdx.x & 63] = acc;
  __syncthreads();
  if (rl == 0 && c < cols) part[(size_t)blockIdx.y * cols + c] = red[0][c & 63] + red[1][c & 63] + red[2][c & 63] + red[3][c & 63];
}
__global__ void colsum_stage2(const float* part, int nchunk, int cols, float* out, int accumulate) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  float acc = accumulate ? out[c] : 0.f;
  for (int k = 0; k < nchunk; ++k) acc += part[(size_t)k * cols + c];
  out[c] = acc;
}

struct AddN {
  const float* x[8];
};
__global__ void add_n_kernel(AddN a, int k, float* y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = a.x[0][i];
  for (int j = 1; j < k; ++j) s += a.x[j][i];
  y[i] = s;
}

__global__ void copy2d_kernel(const float* src, int ld_src, float* dst, int ld_dst, int rows, int cols) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)rows * cols) return;
  const int r = (int)(i / cols), c = (int)(i - (int64_t)r * cols);
  dst[(size_t)r * ld_dst + c] = src[(size_t)r * ld_src + c];
}

__global__ void axpy2d_kernel(const float* src, int ld_src, float* dst, int ld_dst, int rows, int cols) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)rows * cols) return;
  const int r = (int)(i / cols), c = (int)(i - (int64_t)r * cols);
  dst[(size_t)r * ld_dst + c] += src[(size_t)r * ld_src + c];
}

struct CopySegs {
  sdumc_copy_seg s[8];
};
__global__ void copy2d_multi_kernel(const CopySegs cs) {
  const sdumc_copy_seg& sg = cs.s[blockIdx.y];
  const int64_t n = (int64_t)sg.rows * sg.cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / sg.cols), c = (int)(i - (int64_t)r * sg.cols);
    sg.dst[(size_t)r * sg.ld_dst + c] = sg.src[(size_t)r * sg.ld_src + c];
  }
}

// dst_k[idx[r % B], :] = src_k[r, :]: one launch puts the outputs of an eval-mode forward (stream-major [2B, w]) at the rows the
// batch's utterances have in the store (sdumc_scatter_rows_multi).  blockIdx.y = segment; the body (and the argument rules of the
// entry) live in scatter_rows.h, shared with the training epoch's record launch (epoch_record.hip).
__global__ __launch_bounds__(256) void scatter_rows_multi_kernel(const ScatterSegs ss) {
  scatter_rows_segment(ss, blockIdx.y, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// out[b, t, :] = packed[start[b] + t, :] for t < len[b], 0 beyond: the collater's right-zero-padding
// (toolkit/utils/read_data.py:139-151, :223-248) done on the device from a packed feature store.
// one thread per 16 bytes; d must be a multiple of 4
__global__ void gather_pad_kernel(const float* packed, const int64_t* start, const int32_t* len, int B, int Tmax, int d4,
                                  float* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)B * Tmax * d4;
  if (i >= total) return;
  const int c = (int)(i % d4);
  const int64_t r = i / d4;
  const int t = (int)(r % Tmax), b = (int)(r / Tmax);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (t < len[b]) v = ld4(packed + ((size_t)(start[b] + t) * d4 + c) * 4);
  st4(out + 4 * i, v);
}

// the same with store-wide start / len tables and a device index vector: sample b of the batch = store entry idx[b]
// (no per-batch host -> device copies of the tables); len_out (optional) receives the valid frame counts of the batch
__global__ void gather_pad_idx_kernel(const float* packed, const int64_t* start_all, const int32_t* len_all, const int64_t* idx,
                                      int B, int Tmax, int d4, float* out, int32_t* len_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)B * Tmax * d4;
  if (i >= total) return;
  const int c = (int)(i % d4);
  const int64_t r = i / d4;
  const int t = (int)(r % Tmax), b = (int)(r / Tmax);
  const int64_t e = idx[b];
  const int n = len_all[e];
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (t < n) v = ld4(packed + ((size_t)(start_all[e] + t) * d4 + c) * 4);
  st4(out + 4 * i, v);
  if (len_out && t == 0 && c == 0) len_out[b] = n < Tmax ? n : Tmax;
}

// One launch assembles a WHOLE batch: up to SDUMC_GATHER_MAX_SEGS packed tensors (the four modalities' features, and their bf16
// planes when the store holds them) gathered / right-zero-padded into the step's input buffers, plus the labels and the valid frame
// counts.  One wave per output ROW at a time (the row's source -- utterance, frame, or "padding" -- is resolved once per row, in
// 32-bit arithmetic; the lanes then stream its 16-byte units, four loads in flight each), waves striding over the rows of all
// segments, and a CAPPED number of workgroups: the launch is meant to run on a side stream BESIDE a step (engine.FusedTrainer
// prefetches the next batch), where an uncapped grid would queue tens of thousands of workgroups in front of the step's own kernels.
// MISS: the random-missing protocol is enabled (g.miss_enable); a descriptor without it launches the instantiation that has no trace of it.
template <bool MISS>
__global__ __launch_bounds__(256) void gather_batch_kernel(const sdumc_gather_desc g) {
  const int i0 = blockIdx.x * 256 + threadIdx.x;
  if (i0 < g.B) {
    const int64_t e = g.idx[i0];
    if (g.labels_out) g.labels_out[i0] = g.labels_all[e];
    for (int s = 0; s < g.nseg; ++s)
      if (g.seg[s].len_out) {
        const int n = g.seg[s].len_all[e];
        g.seg[s].len_out[i0] = n < g.seg[s].Tmax ? n : g.seg[s].Tmax;
      }
  }
  const int lane = threadIdx.x & 63;
  const uint32_t nwaves = gridDim.x * 4u, total = (uint32_t)g.total;
  for (uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6); row < total; row += nwaves) {
    int s = 0;
    while (s + 1 < g.nseg && (uint32_t)g.seg[s + 1].unit0 <= row) ++s;
    const sdumc_gather_seg& sg = g.seg[s];
    const uint32_t r = row - (uint32_t)sg.unit0;
    const uint32_t b = r / (uint32_t)sg.Tmax, t = r - b * (uint32_t)sg.Tmax;
    const int64_t e = g.idx[b];
    bool valid = (int)t < sg.len_all[e];
    // the random-missing protocol (include/sdumc_hip.h): an absent frame is assembled as a padded one.  Decided once per row from
    // (seed, draw, modality, utterance, frame) alone -- wave-uniform, at most two Philox calls, none for a level whose rate is 0
    if (MISS && valid) {
      bool absent = sg.miss_all != 0u;
      const uint32_t c2 = SDUMC_MISSING_SITE + (uint32_t)sg.miss_mod;
      if (!absent && sg.miss_frame_thr)
        absent = philox4x32_10(t, (uint32_t)e, c2, g.miss_draw, g.miss_seed_lo, g.miss_seed_hi).w[0] < sg.miss_frame_thr;
      if (!absent && sg.miss_utt_thr)
        absent = philox4x32_10(SDUMC_MISSING_UTT, (uint32_t)e, c2, g.miss_draw, g.miss_seed_lo, g.miss_seed_hi).w[0] < sg.miss_utt_thr;
      valid = !absent;
    }
    const int d4 = sg.d4;
    if (sg.map_out && lane == 0) sg.map_out[r] = valid ? (int32_t)(sg.start_all[e] + t) : sg.zero_row;
    if (!sg.out) continue;      // (the map only: the step reads the batch in place)
    const float* src = static_cast<const float*>(sg.packed) + (size_t)(valid ? sg.start_all[e] + t : 0) * d4 * 4;
    float* dst = static_cast<float*>(sg.out) + (size_t)r * d4 * 4;
    for (int c = lane; c < d4; c += 256) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (valid && c + 64 * u < d4) v[u] = ld4(src + 4 * (c + 64 * u));
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (c + 64 * u < d4) st4(dst + 4 * (c + 64 * u), v[u]);
    }
  }
}

// ---- bf16-storage mode helpers ---------------------------------------------------------------------------------------
// xd[row, :] = bf16( x[row % x_rows, :] * keep * scale ): the masked frames of one (site, stream set), materialised once so
// that every consumer (key projection, pooling, their backward) reads plain bf16 rows.  One thread per 8 channels.
__global__ void mask_apply_bf16_kernel(const unsigned short* __restrict__ x, const uint8_t* __restrict__ bits, unsigned short* __restrict__ out,
                                       int64_t rows, int64_t x_rows, int width8, float scale) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * width8) return;
  const int64_t row = i / width8;
  const int c8 = (int)(i - row * width8);
  const uint4 u = *reinterpret_cast<const uint4*>(x + ((row % x_rows) * width8 + c8) * 8);
  const unsigned m = *reinterpret_cast<const unsigned short*>(bits + (row * width8 + c8) * 2);   // 2 bytes = 8 keep-bits
  const unsigned w[4] = {u.x, u.y, u.z, u.w};
  unsigned o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // byte (k >> 1) of m covers channels 4 (k >> 1) .. +3; word k holds channels 2k (low half) and 2k + 1 (high half)
    const unsigned b0 = (m >> (8 * (k >> 1) + 2 * (k & 1))) & 1u, b1 = (m >> (8 * (k >> 1) + 2 * (k & 1) + 1)) & 1u;
    const float lo = b0 ? __uint_as_float(w[k] << 16) * scale : 0.f, hi = b1 ? __uint_as_float(w[k] & 0xffff0000u) * scale : 0.f;
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 h = {(__bf16)lo, (__bf16)hi};
    o[k] = *reinterpret_cast<const unsigned*>(&h);
  }
  *reinterpret_cast<uint4*>(out + i * 8) = uint4{o[0], o[1], o[2], o[3]};
}

// fp32 parameters -> bf16 copies: as stored ([out][in], dst) and, optionally, transposed ([in][out], dst_t), same element
// offsets as in the flat parameter buffer; up to 16 matrices per launch
struct CvtList {
  int n;
  struct { int64_t off; int32_t out, in, want_t; } e[16];
};
__global__ __launch_bounds__(256) void weights_to_bf16_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst,
                                                              unsigned short* __restrict__ dst_t, const CvtList cl) {
  __shared__ float t[32][33];
  const auto& e = cl.e[blockIdx.z];
  const int o0 = blockIdx.y * 32, i0 = blockIdx.x * 32;
  if (o0 >= e.out || i0 >= e.in) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8)
    if (o0 + k < e.out && i0 + tx < e.in) {
      const float v = src[e.off + (int64_t)(o0 + k) * e.in + i0 + tx];
      t[k][tx] = v;
      __bf16 h = (__bf16)v;
      dst[e.off + (int64_t)(o0 + k) * e.in + i0 + tx] = *reinterpret_cast<unsigned short*>(&h);
    }
  if (!e.want_t) return;
  __syncthreads();
  for (int k = ty; k < 32; k += 8)
    if (i0 + k < e.in && o0 + tx < e.out) {
      __bf16 h = (__bf16)t[tx][k];
      dst_t[e.off + (int64_t)(i0 + k) * e.out + o0 + tx] = *reinterpret_cast<unsigned short*>(&h);
    }
}

// dropsum on bf16 gradients: dx = sum_k g_k * mask_k, bf16 in and out (one thread per 4 channels, keep-bits or Philox as the
// fp32 kernel)
__global__ void dropsum_bwd_bf16_kernel(const sdumc_dropsum p, int64_t nquads) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nquads) return;
  const uint32_t row = (uint32_t)(i / (D / 4)), cq = (uint32_t)(i - (int64_t)row * (D / 4));
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < p.terms; ++k) {
    const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(p.g[k]) + 4 * i);
    f32x4 g = {__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
    const DropRT d = drop_resolve(p.drop[k]);
    if (d.enabled) g *= drop_mask4(d, (uint32_t)p.stream_idx[k] * (uint32_t)(p.samples * p.T) + row, cq);
    acc += g;
  }
  typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
  const bf16x4 h = {(__bf16)acc[0], (__bf16)acc[1], (__bf16)acc[2], (__bf16)acc[3]};
  *reinterpret_cast<bf16x4*>(reinterpret_cast<unsigned short*>(p.dx) + 4 * i) = h;
}

__global__ void fill_kernel(float* p, float v, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

__global__ void rng_advance_kernel(uint32_t* st, uint32_t inc) { st[2] += inc; }

__global__ void dropout_mask_kernel(const sdumc_dropout d, int64_t nquads, float* mask) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nquads) return;
  const DropRT r = drop_resolve(d);
  const uint32_t vrow = (uint32_t)(i / r.qwidth), cq = (uint32_t)(i - (int64_t)vrow * r.qwidth);
  f32x4 m = {1.f, 1.f, 1.f, 1.f};
  if (r.enabled) m = drop_mask4(r, vrow, cq);
  st4(mask + 4 * i, m);
}

// keep-bits for `nsite` dropout sites that share one row space (site, site + stride, ...): one thread packs
// four consecutive column quads into one 32-bit store (the byte-per-thread form was store-bound: 53 us for
// the audio tensor; this one is bound by the ~90 VALU ops of Philox per quad)
struct BitsOut {
  uint8_t* p[4];
};
// `call_add`: the keep-bits of the call that many Philox calls AHEAD (the next step's, generated in this step's idle middle).
// `tag`: the {seed, call, magic} the buffers were last filled for: when it names the call this launch is for, there is nothing to do
// (the launch is a tag read per thread); any other tag: generated as ever.
// The tag also names the SHAPE the set was laid out for (sdumc_bits_shape: batch, shard offset, frames per modality): the keep-bit of
// (sample, frame, channel) does not depend on the batch's padded lengths, but its position in the buffer does, so a set filled for
// another shape is a foreign set (a ragged epoch changes shape from step to step).
__device__ __forceinline__ bool bits_tag_matches(const uint32_t* __restrict__ tag, const DropRT& r, const sdumc_bits_shape& sh) {
  if (!(tag[0] == r.k0 && tag[1] == r.k1 && tag[2] == r.call0 && tag[3] == 0x5D0Cb175u)) return false;
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if (tag[4 + i] != sh.w[i]) return false;
  return true;
}
__global__ void dropout_bits_kernel(const sdumc_dropout d, int64_t nwords, int nsite, int site_stride, BitsOut out,
                                    const uint32_t* __restrict__ tag, int call_add, const sdumc_bits_shape shape) {
  DropRT r0 = drop_resolve(d);
  r0.bits = nullptr;   // always from Philox
  r0.call0 += (uint32_t)call_add;
  if (tag != nullptr && bits_tag_matches(tag, r0, shape)) return;
  const uint32_t wpr = r0.qwidth >> 2;                     // 32-bit words per row
  // (grid-stride: with a tag the launch is capped at 1024 workgroups -- as fast when it generates, a third of the workgroups to
  //  retire when it has nothing to do)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += (int64_t)gridDim.x * blockDim.x) {
    DropRT r = r0;
    const uint32_t vrow = (uint32_t)(i / wpr), w = (uint32_t)(i - (int64_t)vrow * wpr);
    for (int s = 0; s < nsite; ++s) {
      uint32_t word = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 m = drop_mask4(r, vrow, 4 * w + q);
        word |= (uint32_t)((m[0] != 0.f) | ((m[1] != 0.f) << 1) | ((m[2] != 0.f) << 2) | ((m[3] != 0.f) << 3)) << (8 * q);
      }
      reinterpret_cast<uint32_t*>(out.p[s])[i] = word;
      r.site += (uint32_t)site_stride;
    }
  }
}

// the tag of pre-generated keep-bits: {seed_lo, seed_hi, call, magic, shape[6]}; call_add < 0: invalidate (written before the buffers
// are refilled)
__global__ void bits_tag_kernel(const sdumc_dropout d, uint32_t* tag, int call_add, const sdumc_bits_shape shape) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const DropRT r = drop_resolve(d);
  tag[0] = r.k0;
  tag[1] = r.k1;
  tag[2] = r.call0 + (uint32_t)(call_add < 0 ? 0 : call_add);
#pragma unroll
  for (int i = 0; i < 6; ++i) tag[4 + i] = shape.w[i];
  tag[3] = call_add < 0 ? 0u : 0x5D0Cb175u;
}

// bf16-storage mode: the keep-bits of TWO sites that share a row space (fra2utt_m and cross_att_fra2utt_m read the same frames)
// AND the masked frames xd_s = bf16(x * keep_s * scale) of both, in one pass over x: a thread owns 16 channels of one virtual
// row = one 32-bit word of keep-bits per site (dropout_bits_kernel's arithmetic) and 32 bytes of x (mask_apply_bf16_kernel's).
struct XdOut {
  unsigned short* p[2];
};
__global__ void dropout_bits_apply_bf16_kernel(const sdumc_dropout d, int64_t nwords, int site_stride, BitsOut out,
                                               const unsigned short* __restrict__ x, int64_t x_rows, XdOut xd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nwords) return;
  DropRT r = drop_resolve(d);
  r.bits = nullptr;   // always from Philox
  const uint32_t wpr = r.qwidth >> 2;                      // 32-bit words (16 channels) per row
  const uint32_t vrow = (uint32_t)(i / wpr), w = (uint32_t)(i - (int64_t)vrow * wpr);
  const uint4* xp = reinterpret_cast<const uint4*>(x + (((int64_t)vrow % x_rows) * wpr + w) * 16);
  const uint4 xin[2] = {xp[0], xp[1]};
  const float scale = r.scale;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    uint32_t word = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 m = drop_mask4(r, vrow, 4 * w + q);
      word |= (uint32_t)((m[0] != 0.f) | ((m[1] != 0.f) << 1) | ((m[2] != 0.f) << 2) | ((m[3] != 0.f) << 3)) << (8 * q);
    }
    reinterpret_cast<uint32_t*>(out.p[s])[i] = word;
    uint4 o[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {      // 8 channels = bytes 2h, 2h + 1 of the word
      const unsigned m = (word >> (16 * h)) & 0xffffu;
      const unsigned wv[4] = {xin[h].x, xin[h].y, xin[h].z, xin[h].w};
      unsigned ov[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned b0 = (m >> (8 * (k >> 1) + 2 * (k & 1))) & 1u, b1 = (m >> (8 * (k >> 1) + 2 * (k & 1) + 1)) & 1u;
        const float lo = b0 ? __uint_as_float(wv[k] << 16) * scale : 0.f, hi = b1 ? __uint_as_float(wv[k] & 0xffff0000u) * scale : 0.f;
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        const bf16x2 hh = {(__bf16)lo, (__bf16)hi};
        ov[k] = *reinterpret_cast<const unsigned*>(&hh);
      }
      o[h] = uint4{ov[0], ov[1], ov[2], ov[3]};
    }
    uint4* op = reinterpret_cast<uint4*>(xd.p[s] + i * 16);
    op[0] = o[0];
    op[1] = o[1];
    r.site += (uint32_t)site_stride;
  }
}

// dx[b,t,:] = sum_k g_k[b,t,:] * mask_k  : one thread per 4 channels
__global__ void dropsum_bwd_kernel(const sdumc_dropsum p, int64_t nquads) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nquads) return;
  const uint32_t row = (uint32_t)(i / (D / 4)), cq = (uint32_t)(i - (int64_t)row * (D / 4));  // row = b*T + t
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < p.terms; ++k) {
    f32x4 g = ld4(p.g[k] + 4 * i);
    const DropRT d = drop_resolve(p.drop[k]);
    if (d.enabled) g *= drop_mask4(d, (uint32_t)p.stream_idx[k] * (uint32_t)(p.samples * p.T) + row, cq);
    acc += g;
  }
  st4(p.dx + 4 * i, acc);
}

// ---- modality fusion (model :301-332): one wave per virtual sample ---------------------------
__global__ __launch_bounds__(256) void fusion_fwd_kernel(const float* u, const float* alpha, float* qin, int V) {
  const int v = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (v >= V) return;
  const f32x4 ua = ld4(u + ((size_t)v * 3 + 0) * D + 4 * lane);
  const f32x4 ut = ld4(u + ((size_t)v * 3 + 1) * D + 4 * lane);
  const f32x4 uv = ld4(u + ((size_t)v * 3 + 2) * D + 4 * lane);
  const float aa = alpha[v * 3 + 0], at = alpha[v * 3 + 1], av = alpha[v * 3 + 2];
  const size_t o = (size_t)v * D + 4 * lane, gs = (size_t)V * D;
  st4(qin + 0 * gs + o, ua * aa + ut * at + uv * av);
  st4(qin + 1 * gs + o, ua * aa + ut * at);
  st4(qin + 2 * gs + o, ut * at + uv * av);
  st4(qin + 3 * gs + o, ua * aa + uv * av);
  st4(qin + 4 * gs + o, ua);
  st4(qin + 5 * gs + o, ut);
  st4(qin + 6 * gs + o, uv);
}

__global__ __launch_bounds__(256) void fusion_bwd_kernel(const float* u, const float* alpha, const float* dqin,
                                                         float* du, float* dalpha, int V) {
  const int v = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (v >= V) return;
  const size_t o = (size_t)v * D + 4 * lane, gs = (size_t)V * D;
  const f32x4 df = ld4(dqin + o), dfat = ld4(dqin + gs + o), dftv = ld4(dqin + 2 * gs + o),
              dfav = ld4(dqin + 3 * gs + o);
  const f32x4 ga = df + dfat + dfav, gt = df + dfat + dftv, gv = df + dftv + dfav;
  const f32x4 ua = ld4(u + ((size_t)v * 3 + 0) * D + 4 * lane);
  const f32x4 ut = ld4(u + ((size_t)v * 3 + 1) * D + 4 * lane);
  const f32x4 uv = ld4(u + ((size_t)v * 3 + 2) * D + 4 * lane);
  const float aa = alpha[v * 3 + 0], at = alpha[v * 3 + 1], av = alpha[v * 3 + 2];
  st4(du + ((size_t)v * 3 + 0) * D + 4 * lane, ga * aa + ld4(dqin + 4 * gs + o));
  st4(du + ((size_t)v * 3 + 1) * D + 4 * lane, gt * at + ld4(dqin + 5 * gs + o));
  st4(du + ((size_t)v * 3 + 2) * D + 4 * lane, gv * av + ld4(dqin + 6 * gs + o));
  const float da = wave_sum(dot4(ga, ua)), dt = wave_sum(dot4(gt, ut)), dv = wave_sum(dot4(gv, uv));
  if (lane == 0) {
    dalpha[v * 3 + 0] += da;
    dalpha[v * 3 + 1] += dt;
    dalpha[v * 3 + 2] += dv;
  }
}

// ---- second-level fusion (model :346-349): h = sum_m alpha_m c_m, one wave per (v, i) -----------
__global__ __launch_bounds__(256) void hweight_fwd_kernel(const float* c, const float* alpha, float* h, int V) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // index over V*7*128/4
  const int64_t total = (int64_t)V * NQ * H / 4;
  if (e >= total) return;
  const int v = (int)(e / (NQ * H / 4));
  const int64_t r = e - (int64_t)v * (NQ * H / 4);
  const size_t gs = (size_t)V * NQ * H;  // c is [3][V,7,128]
  const float* cb = c + (size_t)v * NQ * H + 4 * r;
  st4(h + 4 * e, ld4(cb) * alpha[v * 3] + ld4(cb + gs) * alpha[v * 3 + 1] + ld4(cb + 2 * gs) * alpha[v * 3 + 2]);
}

// one 256-thread workgroup per v: dc_m = alpha_m dh (+ dct on m = 1), dalpha_m = <dh, c_m>
__global__ __launch_bounds__(256) void hweight_bwd_kernel(const float* c, const float* alpha, const float* dh,
                                                          const float* dct, float* dc, float* dalpha, int V,
                                                          float relu_scale) {
  __shared__ float red[3][4];
  const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float acc[3] = {0.f, 0.f, 0.f};
  const float a0 = alpha[v * 3], a1 = alpha[v * 3 + 1], a2 = alpha[v * 3 + 2];
  for (int e = tid; e < NQ * H / 4; e += 256) {
    const f32x4 g = ld4(dh + (size_t)v * NQ * H + 4 * e);
    const size_t gs = (size_t)V * NQ * H;  // c, dc are [3][V,7,128]
    const size_t cb = (size_t)v * NQ * H + 4 * e;
    const f32x4 c0 = ld4(c + cb), c1 = ld4(c + cb + gs), c2 = ld4(c + cb + 2 * gs);
    acc[0] += dot4(g, c0);
    acc[1] += dot4(g, c1);
    acc[2] += dot4(g, c2);
    f32x4 g0 = g * a0, g1 = g * a1, g2 = g * a2;
    if (dct) g1 += ld4(dct + (size_t)v * NQ * H + 4 * e);
    if (relu_scale > 0.f) {   // gradient w.r.t. the pre-activation of cross_*_mlp.3 (ReLU + dropout backward)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        g0[j] = c0[j] > 0.f ? g0[j] * relu_scale : 0.f;
        g1[j] = c1[j] > 0.f ? g1[j] * relu_scale : 0.f;
        g2[j] = c2[j] > 0.f ? g2[j] * relu_scale : 0.f;
      }
    }
    st4(dc + cb, g0);
    st4(dc + cb + gs, g1);
    st4(dc + cb + 2 * gs, g2);
  }
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const float s = wave_sum(acc[m]);
    if (lane == 0) red[m][wave] = s;
  }
  __syncthreads();
  if (tid < 3) dalpha[v * 3 + tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
}

// z[v,:] = sum_i beta_i h_i : thread per (v, 4 channels)
__global__ void zpool_fwd_kernel(const float* h, const float* beta, float* z, int V) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= V * (H / 4)) return;
  const int v = e / (H / 4), cq = e - v * (H / 4);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NQ; ++i) acc += ld4(h + ((size_t)v * NQ + i) * H + 4 * cq) * beta[v * NQ + i];
  st4(z + (size_t)v * H + 4 * cq, acc);
}

// one wave per v (lanes 0..31 hold 4 channels each): dh_i = beta_i dz ; dbeta_i = <dz, h_i>
__global__ __launch_bounds__(256) void zpool_bwd_kernel(const float* h, const float* beta, const float* dz,
                                                        const float* dz_add, float* dh, float* dbeta, int V) {
  const int v = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (v >= V) return;
  const bool on = lane < H / 4;
  f32x4 g = {0.f, 0.f, 0.f, 0.f};
  if (on) g = ld4(dz + (size_t)v * H + 4 * lane);
  if (on && dz_add) g += ld4(dz_add + (size_t)v * H + 4 * lane);
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    float d = 0.f;
    if (on) {
      d = dot4(g, ld4(h + ((size_t)v * NQ + i) * H + 4 * lane));
      st4(dh + ((size_t)v * NQ + i) * H + 4 * lane, g * beta[v * NQ + i]);
    }
    d = wave_sum(d);
    if (lane == 0) dbeta[v * NQ + i] = d;
  }
}

inline unsigned nblk(int64_t n, int b = 256) { return (unsigned)((n + b - 1) / b); }

}  // namespace

extern "C" int sdumc_relu_drop_bwd(const float* dy, const float* y, float scale, float* dz, int64_t n, void* stream) {
  if (!dy || !y || !dz || n < 0) return SDUMC_EINVAL;
  if (n == 0) return SDUMC_OK;
  hipLaunchKernelGGL(relu_drop_bwd_kernel, dim3(nblk(n)), dim3(256), 0, as_stream(stream), dy, y, scale, dz, n);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" size_t sdumc_colsum_workspace_bytes(int64_t rows, int32_t cols) {
  const int64_t nchunk = (rows + CS_ROWS - 1) / CS_ROWS;
  return (size_t)nchunk * cols * sizeof(float);
}

extern "C" int sdumc_colsum(const float* a, int64_t rows, int32_t cols, int32_t lda, float* out, int32_t accumulate,
                            float* workspace, void* stream) {
  if (!a || !out || !workspace || rows <= 0 || cols <= 0 || lda < cols) return SDUMC_EINVAL;
  const int nchunk = (int)((rows + CS_ROWS - 1) / CS_ROWS);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(colsum_stage1, dim3((cols + 63) / 64, nchunk), dim3(256), 0, st, a, rows, cols, lda, workspace);
  SDUMC_CHECK_LAUNCH();
  hipLaunchKernelGGL(colsum_stage2, dim3(nblk(cols)), dim3(256), 0, st, workspace, nchunk, cols, out, accumulate);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_add_n(const float* const* xs, int32_t k, float* y, int64_t n, void* stream) {
  if (!xs || k < 1 || k > 8 || !y || n < 0) return SDUMC_EINVAL;
  AddN a;
  for (int i = 0; i < 8; ++i) {
    a.x[i] = i < k ? xs[i] : nullptr;
    if (i < k && !xs[i]) return SDUMC_EINVAL;
  }
  if (n == 0) return SDUMC_OK;
  hipLaunchKernelGGL(add_n_kernel, dim3(nblk(n)), dim3(256), 0, as_stream(stream), a, k, y, n);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_copy2d(const float* src, int32_t ld_src, float* dst, int32_t ld_dst, int32_t rows, int32_t cols,
                            void* stream) {
  if (!src || !dst || rows <= 0 || cols <= 0 || ld_src < cols || ld_dst < cols) return SDUMC_EINVAL;
  hipLaunchKernelGGL(copy2d_kernel, dim3(nblk((int64_t)rows * cols)), dim3(256), 0, as_stream(stream), src, ld_src, dst,
                     ld_dst, rows, cols);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_copy2d_multi(const sdumc_copy_seg* segs, int32_t n, void* stream) {
  if (!segs || n < 1 || n > 8) return SDUMC_EINVAL;
  CopySegs cs;
  int64_t mx = 0;
  for (int i = 0; i < n; ++i) {
    if (!segs[i].src || !segs[i].dst || segs[i].rows <= 0 || segs[i].cols <= 0) return SDUMC_EINVAL;
    cs.s[i] = segs[i];
    mx = std::max<int64_t>(mx, (int64_t)segs[i].rows * segs[i].cols);
  }
  hipLaunchKernelGGL(copy2d_multi_kernel, dim3(std::min<unsigned>(nblk(mx), 256u), n), dim3(256), 0, as_stream(stream), cs);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_scatter_rows_multi(const sdumc_scatter_seg* segs, int32_t n, const int64_t* idx, int32_t B, uint8_t* mark,
                                        void* stream) {
  ScatterSegs ss;
  int64_t mx = 0;      // lanes of the widest segment (the mark pass needs B)
  if (scatter_segs_fill(&ss, segs, n, idx, B, mark, &mx) != SDUMC_OK) return SDUMC_EINVAL;
  hipLaunchKernelGGL(scatter_rows_multi_kernel, dim3(std::min<unsigned>(nblk(mx), 256u), n), dim3(256), 0, as_stream(stream), ss);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_gather_pad_idx(const float* packed, const int64_t* start_all, const int32_t* len_all, const int64_t* idx,
                                    int32_t B, int32_t Tmax, int32_t d, float* out, int32_t* len_out, void* stream) {
  if (!packed || !start_all || !len_all || !idx || !out || B <= 0 || Tmax <= 0 || d <= 0 || (d & 3)) return SDUMC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(out)) & 15) return SDUMC_EINVAL;
  const int64_t total = (int64_t)B * Tmax * (d / 4);
  hipLaunchKernelGGL(gather_pad_idx_kernel, dim3(nblk(total)), dim3(256), 0, as_stream(stream), packed, start_all, len_all, idx, B,
                     Tmax, d / 4, out, len_out);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_gather_batch(const sdumc_gather_desc* gp, int32_t max_workgroups, void* stream) {
  if (!gp || gp->nseg < 1 || gp->nseg > SDUMC_GATHER_MAX_SEGS || gp->B <= 0 || !gp->idx) return SDUMC_EINVAL;
  if ((gp->labels_out != nullptr) != (gp->labels_all != nullptr)) return SDUMC_EINVAL;
  sdumc_gather_desc g = *gp;
  int64_t total = 0;      // output rows of all segments
  for (int s = 0; s < g.nseg; ++s) {
    sdumc_gather_seg& sg = g.seg[s];
    if (!sg.start_all || !sg.len_all || sg.Tmax <= 0 || (!sg.out && !sg.map_out)) return SDUMC_EINVAL;
    if (sg.out && (!sg.packed || sg.d4 <= 0)) return SDUMC_EINVAL;
    if (sg.map_out && ((reinterpret_cast<uintptr_t>(sg.map_out) & 3) || sg.zero_row < 0)) return SDUMC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(sg.packed) | reinterpret_cast<uintptr_t>(sg.out)) & 15) return SDUMC_EINVAL;
    if (g.miss_enable && ((uint32_t)sg.miss_mod > 3u || (sg.miss_all & ~3u))) return SDUMC_EINVAL;      // (the random-missing protocol)
    sg.unit0 = total;
    total += (int64_t)g.B * sg.Tmax;
  }
  if (total >= 0x7FFFFFFF) return SDUMC_EINVAL;
  g.total = total;
  int64_t blocks = (total + 3) / 4;      // one wave per row
  if (max_workgroups > 0 && blocks > max_workgroups) blocks = max_workgroups;
  if (blocks < (g.B + 255) / 256) blocks = (g.B + 255) / 256;
  if (g.miss_enable) hipLaunchKernelGGL(gather_batch_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), g);
  else hipLaunchKernelGGL(gather_batch_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), g);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_gather_pad(const float* packed, const int64_t* start, const int32_t* len, int32_t B, int32_t Tmax,
                                int32_t d, float* out, void* stream) {
  if (!packed || !start || !len || !out || B <= 0 || Tmax <= 0 || d <= 0 || (d & 3)) return SDUMC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(out)) & 15) return SDUMC_EINVAL;
  const int64_t total = (int64_t)B * Tmax * (d / 4);
  hipLaunchKernelGGL(gather_pad_kernel, dim3(nblk(total)), dim3(256), 0, as_stream(stream), packed, start, len, B, Tmax,
                     d / 4, out);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_axpy2d(const float* src, int32_t ld_src, float* dst, int32_t ld_dst, int32_t rows, int32_t cols,
                            void* stream) {
  if (!src || !dst || rows <= 0 || cols <= 0 || ld_src < cols || ld_dst < cols) return SDUMC_EINVAL;
  hipLaunchKernelGGL(axpy2d_kernel, dim3(nblk((int64_t)rows * cols)), dim3(256), 0, as_stream(stream), src, ld_src, dst,
                     ld_dst, rows, cols);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_fill(float* p, float v, int64_t n, void* stream) {
  if (!p || n < 0) return SDUMC_EINVAL;
  if (n == 0) return SDUMC_OK;
  hipLaunchKernelGGL(fill_kernel, dim3(nblk(n)), dim3(256), 0, as_stream(stream), p, v, n);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_rng_advance(uint32_t* dev_state, uint32_t inc, void* stream) {
  if (!dev_state) return SDUMC_EINVAL;
  hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(1), 0, as_stream(stream), dev_state, inc);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_dropout_mask(const sdumc_dropout* d, int32_t streams, float* mask, void* stream) {
  if (!d || !mask || streams < 1 || (d->width & 3) || d->width == 0) return SDUMC_EINVAL;
  const int64_t nquads = (int64_t)streams * d->samples * (d->rows ? d->rows : 1) * (d->width / 4);
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(nblk(nquads)), dim3(256), 0, as_stream(stream), *d, nquads, mask);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

// tag: the launch is a no-op when it names this call (see the kernel); call_add: generate for the call that many ahead
extern "C" int sdumc_dropout_bits_multi_ex_(const sdumc_dropout* d, int32_t streams, int32_t nsite, int32_t site_stride,
                                            uint8_t* const* bits, const uint32_t* tag, int32_t call_add, const sdumc_bits_shape* shape,
                                            void* stream) {
  if (!d || !bits || streams < 1 || nsite < 1 || nsite > 4 || (d->width & 15) || d->width == 0) return SDUMC_EINVAL;
  BitsOut out;
  for (int s = 0; s < 4; ++s) {
    out.p[s] = s < nsite ? bits[s] : nullptr;
    if (s < nsite && (!bits[s] || (reinterpret_cast<uintptr_t>(bits[s]) & 3))) return SDUMC_EINVAL;
  }
  const int64_t nwords = (int64_t)streams * d->samples * (d->rows ? d->rows : 1) * (d->width / 16);
  constexpr unsigned cap = 1024;      // (with a tag: 1.2536-1.2572 ms per fp32 C2 step; uncapped 1.255-1.2617; 512 / 256: 1.257-1.2594)
  unsigned grid = (unsigned)nblk(nwords);
  if (tag && grid > cap) grid = cap;
  sdumc_bits_shape sh;
  memset(&sh, 0, sizeof(sh));
  if (shape) sh = *shape;
  hipLaunchKernelGGL(dropout_bits_kernel, dim3(grid), dim3(256), 0, as_stream(stream), *d, nwords, nsite,
                     site_stride, out, tag, call_add, sh);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}
extern "C" int sdumc_dropout_bits_multi(const sdumc_dropout* d, int32_t streams, int32_t nsite, int32_t site_stride,
                                        uint8_t* const* bits, void* stream) {
  return sdumc_dropout_bits_multi_ex_(d, streams, nsite, site_stride, bits, nullptr, 0, nullptr, stream);
}
extern "C" int sdumc_bits_tag_(const sdumc_dropout* d, uint32_t* tag, int32_t call_add, const sdumc_bits_shape* shape, void* stream) {
  if (!d || !tag) return SDUMC_EINVAL;
  sdumc_bits_shape sh;
  memset(&sh, 0, sizeof(sh));
  if (shape) sh = *shape;
  hipLaunchKernelGGL(bits_tag_kernel, dim3(1), dim3(64), 0, as_stream(stream), *d, tag, call_add, sh);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_dropout_bits_apply_bf16(const sdumc_dropout* d, int32_t streams, int32_t site_stride, uint8_t* const* bits,
                                             const void* x, int64_t x_rows, void* const* xd, void* stream) {
  if (!d || !bits || !xd || !x || streams < 1 || x_rows <= 0 || (d->width & 15) || d->width == 0 || !d->enabled) return SDUMC_EINVAL;
  BitsOut out;
  XdOut xo;
  for (int s = 0; s < 4; ++s) out.p[s] = nullptr;
  for (int s = 0; s < 2; ++s) {
    if (!bits[s] || !xd[s] || (reinterpret_cast<uintptr_t>(bits[s]) & 3) || (reinterpret_cast<uintptr_t>(xd[s]) & 15)) return SDUMC_EINVAL;
    out.p[s] = bits[s];
    xo.p[s] = static_cast<unsigned short*>(xd[s]);
  }
  if (reinterpret_cast<uintptr_t>(x) & 15) return SDUMC_EINVAL;
  const int64_t nwords = (int64_t)streams * d->samples * (d->rows ? d->rows : 1) * (d->width / 16);
  hipLaunchKernelGGL(dropout_bits_apply_bf16_kernel, dim3(nblk(nwords)), dim3(256), 0, as_stream(stream), *d, nwords, site_stride, out,
                     static_cast<const unsigned short*>(x), x_rows, xo);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_dropout_bits(const sdumc_dropout* d, int32_t streams, uint8_t* bits, void* stream) {
  uint8_t* one[1] = {bits};
  return sdumc_dropout_bits_multi(d, streams, 1, 0, one, stream);
}

extern "C" int sdumc_mask_apply_bf16(const void* x, const uint8_t* bits, void* out, int64_t rows, int64_t x_rows, int32_t width,
                                     float scale, void* stream) {
  if (!x || !bits || !out || rows <= 0 || x_rows <= 0 || width <= 0 || (width & 7)) return SDUMC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15 || (reinterpret_cast<uintptr_t>(bits) & 1)) return SDUMC_EINVAL;
  const int64_t n = rows * (width / 8);
  hipLaunchKernelGGL(mask_apply_bf16_kernel, dim3(nblk(n)), dim3(256), 0, as_stream(stream), static_cast<const unsigned short*>(x), bits,
                     static_cast<unsigned short*>(out), rows, x_rows, width / 8, scale);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_weights_to_bf16_(const float* src, void* dst, void* dst_t, const int64_t* offs, const int32_t* outs,
                                      const int32_t* ins, const int32_t* want_t, int n, void* stream) {
  if (!src || !dst || n <= 0 || n > 16) return SDUMC_EINVAL;
  CvtList cl;
  cl.n = n;
  int mo = 0, mi = 0;
  for (int i = 0; i < n; ++i) {
    cl.e[i].off = offs[i];
    cl.e[i].out = outs[i];
    cl.e[i].in = ins[i];
    cl.e[i].want_t = want_t[i];
    if (want_t[i] && !dst_t) return SDUMC_EINVAL;
    mo = outs[i] > mo ? outs[i] : mo;
    mi = ins[i] > mi ? ins[i] : mi;
  }
  hipLaunchKernelGGL(weights_to_bf16_kernel, dim3((mi + 31) / 32, (mo + 31) / 32, n), dim3(256), 0, as_stream(stream), src,
                     static_cast<unsigned short*>(dst), static_cast<unsigned short*>(dst_t), cl);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_dropsum_bwd(const sdumc_dropsum* p, void* stream) {
  if (!p || p->terms < 1 || p->terms > 8 || !p->dx || p->samples <= 0 || p->T <= 0) return SDUMC_EINVAL;
  for (int k = 0; k < p->terms; ++k)
    if (!p->g[k]) return SDUMC_EINVAL;
  const int64_t nquads = (int64_t)p->samples * p->T * (D / 4);
  if (p->bf16) {
    hipLaunchKernelGGL(dropsum_bwd_bf16_kernel, dim3(nblk(nquads)), dim3(256), 0, as_stream(stream), *p, nquads);
    SDUMC_CHECK_LAUNCH();
    return SDUMC_OK;
  }
  hipLaunchKernelGGL(dropsum_bwd_kernel, dim3(nblk(nquads)), dim3(256), 0, as_stream(stream), *p, nquads);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_fusion_fwd(const float* u, const float* alpha, float* qin, int32_t V, void* stream) {
  if (!u || !alpha || !qin || V <= 0) return SDUMC_EINVAL;
  hipLaunchKernelGGL(fusion_fwd_kernel, dim3((V + 3) / 4), dim3(256), 0, as_stream(stream), u, alpha, qin, V);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_fusion_bwd(const float* u, const float* alpha, const float* dqin, float* du, float* dalpha,
                                int32_t V, void* stream) {
  if (!u || !alpha || !dqin || !du || !dalpha || V <= 0) return SDUMC_EINVAL;
  hipLaunchKernelGGL(fusion_bwd_kernel, dim3((V + 3) / 4), dim3(256), 0, as_stream(stream), u, alpha, dqin, du, dalpha, V);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_hweight_fwd(const float* c, const float* alpha, float* h, int32_t V, void* stream) {
  if (!c || !alpha || !h || V <= 0) return SDUMC_EINVAL;
  hipLaunchKernelGGL(hweight_fwd_kernel, dim3(nblk((int64_t)V * NQ * H / 4)), dim3(256), 0, as_stream(stream), c, alpha, h, V);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_hweight_bwd(const float* c, const float* alpha, const float* dh, const float* dct, float* dc,
                                 float* dalpha, int32_t V, float relu_scale, void* stream) {
  if (!c || !alpha || !dh || !dc || !dalpha || V <= 0) return SDUMC_EINVAL;
  hipLaunchKernelGGL(hweight_bwd_kernel, dim3(V), dim3(256), 0, as_stream(stream), c, alpha, dh, dct, dc, dalpha, V,
                     relu_scale);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_zpool_fwd(const float* h, const float* beta, float* z, int32_t V, void* stream) {
  if (!h || !beta || !z || V <= 0) return SDUMC_EINVAL;
  hipLaunchKernelGGL(zpool_fwd_kernel, dim3(nblk((int64_t)V * (H / 4))), dim3(256), 0, as_stream(stream), h, beta, z, V);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_zpool_bwd(const float* h, const float* beta, const float* dz, float* dh, float* dbeta, int32_t V,
                               void* stream) {
  if (!h || !beta || !dz || !dh || !dbeta || V <= 0) return SDUMC_EINVAL;
  return sdumc_zpool_bwd_add_(h, beta, dz, nullptr, dh, dbeta, V, stream);
}

extern "C" int sdumc_zpool_bwd_add_(const float* h, const float* beta, const float* dz, const float* dz_add, float* dh,
                                    float* dbeta, int32_t V, void* stream) {
  if (!h || !beta || !dz || !dh || !dbeta || V <= 0) return SDUMC_EINVAL;
  hipLaunchKernelGGL(zpool_bwd_kernel, dim3((V + 3) / 4), dim3(256), 0, as_stream(stream), h, beta, dz, dz_add, dh, dbeta, V);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_relu_drop_bwd_add_(const float* dy, const float* y, float scale, float* dz, int64_t n, const float* add,
                                        int32_t row_len, int32_t col0, int32_t width, void* stream) {
  if (!dy || !y || !dz || n < 0 || row_len <= 0) return SDUMC_EINVAL;
  if (n == 0) return SDUMC_OK;
  if (!add) return sdumc_relu_drop_bwd(dy, y, scale, dz, n, stream);
  hipLaunchKernelGGL(relu_drop_bwd_add_kernel, dim3(nblk(n)), dim3(256), 0, as_stream(stream), dy, y, scale, dz, n, add,
                     row_len, col0, width);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

namespace {
__global__ void dp_pack_kernel(const float* __restrict__ rnc, const float* __restrict__ labels, const float* __restrict__ ssd,
                               int nf, int B, float* __restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nf) rec[i] = rnc[i];
  else if (i < nf + B) rec[i] = labels[i - nf];
  else if (i < nf + B + 3) rec[i] = ssd[i - nf - B];
}
__global__ void dp_unpack_kernel(const float* __restrict__ recs, int W, int B, int rd, float* __restrict__ feats,
                                 float* __restrict__ labels2, float* __restrict__ ssd) {
  const int nf = 2 * B * rd, n = nf + B + 3;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over the [2*W*B, rd] feature matrix
  const int64_t total = (int64_t)W * nf;
  if (i < total) {
    const int col = (int)(i % rd);
    const int64_t row = i / rd;            // s * W * B + r * B + b
    const int s = (int)(row / ((int64_t)W * B));
    const int rb = (int)(row % ((int64_t)W * B));
    const int r = rb / B, b = rb % B;
    feats[i] = recs[(int64_t)r * n + (int64_t)(s * B + b) * rd + col];
    if (col == 0) labels2[row] = recs[(int64_t)r * n + nf + b];
  }
  if (i < 3) {
    float acc = 0.f;
    for (int r = 0; r < W; ++r) acc += recs[(int64_t)r * n + nf + B + (int)i];   // fixed order: identical on every rank
    ssd[i] = acc;
  }
}
}  // namespace

extern "C" int sdumc_dp_pack(const float* rnc, const float* labels, const float* ssd, int32_t B, int32_t rd, float* record,
                             void* stream) {
  if (!rnc || !labels || !ssd || !record || B <= 0 || rd <= 0) return SDUMC_EINVAL;
  const int nf = 2 * B * rd, n = nf + B + 3;
  hipLaunchKernelGGL(dp_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), rnc, labels, ssd, nf, B, record);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" int sdumc_dp_unpack(const float* records, int32_t W, int32_t B, int32_t rd, float* feats, float* labels2,
                               float* ssd, void* stream) {
  if (!records || !feats || !labels2 || !ssd || W <= 0 || B <= 0 || rd <= 0) return SDUMC_EINVAL;
  const int64_t total = (int64_t)W * 2 * B * rd;
  hipLaunchKernelGGL(dp_unpack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), records, W, B,
                     rd, feats, labels2, ssd);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

extern "C" const char* sdumc_version(void) { return "sdumc_hip 0.1 (gfx950)"; }

SDUMC_PRELOAD_HOOK(elementwise)      // (common.h)
