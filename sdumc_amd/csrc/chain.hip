// chain.hip — the utterance-level network of WengnetMOSEIMultViewsTextMissing as FOUR launches instead of ~77.
//
//   stage A forward   model :293-332  audio/text/video_mlp -> attention_mlp -> fc_att -> fusion algebra -> the 7 query MLPs
//                                      -> query_proj of the three Cross_Attention blocks (model :85)
//   stage B forward   model :338-368  cross_{audio,text,video}_mlp -> modality-weighted sum -> cross_attention_mlp ->
//                                      cross_fc_att -> cross_fused_feat -> fc_out_v, orgin_linear_change
//   stage B backward / stage A backward: the dX mirror of both (loss.backward(), main :149); every pre-activation gradient
//   is written to HBM, so the weight gradients stay grouped MFMA GEMMs (dW = dz^T x) on a side lane, off this chain.
//
// Why one launch per stage: every layer here is per-sample (row-independent), M = 2B or 14B rows, 0.03-0.6 GFLOP -- the
// ~77 launches they used to be cost 6-13 us each whatever they computed (0.65 ms of a 2.1 ms step with the chip nearly
// idle).  Here a 512-thread workgroup owns R virtual samples and walks the whole stage with the activations in LDS; the
// only thing streamed is the weights (5.1 MB in stage A, 2.2 MB in stage B, L2-resident across the grid).
//
// The per-layer product is out[r][:] = sum_i in[r][i] * M[i][:] with M row-major [I][O]:
//   forward  M = W^T (the engine keeps transposed copies of the utterance-level weights, refreshed once per forward call)
//   backward M = W as stored ([out][in]): dX = dz W
// so that a lane owns 4 consecutive OUTPUT columns, a wave-load is one fully coalesced KiB of M, the input value is a
// wave-uniform LDS broadcast, and the inner loop is pure FMA (no cross-lane reduction per output).  The 8 waves split the
// I range; their partial rows meet in LDS once per layer, in a fixed order (bitwise reproducible, no atomics).
// fp32 throughout: with M <= 14 rows per workgroup the matrix cores would run at 1/16 .. 1/2 occupancy of their 16/32-row
// tiles, and fp32 MFMA has the VALU's rate anyway (MI355X_MICROARCH.md) -- the bound here is the weight stream per CU.
#include "chain_common.h"


namespace {

// the stages' LDS layouts here: the full-width partial-sum area, one modality at a time
template <int R> using FwdA = FwdALds<R, PART_FLOATS>;
template <int R> using FwdB = FwdBLds<R, PART_FLOATS, 1, 1>;
template <int R> using BwdB = BwdBLds<R, PART_FLOATS, 1>;
template <int R> using BwdA = BwdALds<R, PART_FLOATS, 1>;

// ------------------------------------------------------------------------------------------------------------------
// stage A forward (model :293-332 + :85)
// ------------------------------------------------------------------------------------------------------------------
template <int R, class WT>
__device__ __forceinline__ void chain_fwd_a_body(const sdumc_chain_args a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  using L = FwdA<R>;
  float *part = sm + L::part, *s_hpre = sm + L::hpre, *s_u1 = sm + L::u1, *s_u = sm + L::u, *s_att1 = sm + L::att1, *s_att2 = sm + L::att2,
        *s_qin = sm + L::qin, *s_q = sm + L::q, *s_bias = sm + L::bias;
  const int V = a.V, v0 = blockIdx.x * R;
  const int64_t VD = (int64_t)V * D;
  fwd_a_stage_bias(a, s_bias);

  const DropRT dbase = drop_resolve(a.drop);
  RingOf<D, D, WT> ring;          // every layer of this stage streams through the same ring type (NB = 1, 4 deep)
  rxm_prefetch<D, D, WT>(ring, a.umlp0_w[0], D);
  for (int m = 0; m < 3; ++m) load_rows<R>(s_hpre + m * R * D, a.hpre + m * VD, D, D, v0, V);
  __syncthreads();
  // audio / text / video_mlp (model :293-295)
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    FwdEpi e{s_bias + m * D, s_u1 + m * R * D, D, a.u1 + m * VD + (int64_t)v0 * D, D, true,
             mkdrop_rt(dbase, 6 + 2 * m, 1, D), (uint32_t)v0, 1u};
    auto epi = [&](int r, int col, f32x4 v) { if (v0 + r < V) e(r, col, v); };
    rxm_run<R, D, D, WT>(ring, s_hpre + m * R * D, D, a.umlp0_w[m], D, part, epi,
                     [&] { rxm_prefetch<D, D, WT>(ring, m < 2 ? a.umlp0_w[m + 1] : a.umlp3_w[0], D); });
  }
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    FwdEpi e{s_bias + (3 + m) * D, s_u + m * D, 3 * D, a.u + (int64_t)v0 * 3 * D + m * D, 3 * D, true,
             mkdrop_rt(dbase, 7 + 2 * m, 1, D), (uint32_t)v0, 1u};
    auto epi = [&](int r, int col, f32x4 v) { if (v0 + r < V) e(r, col, v); else st4(s_u + r * 3 * D + m * D + col, f32x4{0.f, 0.f, 0.f, 0.f}); };
    rxm_run<R, D, D, WT>(ring, s_u1 + m * R * D, D, a.umlp3_w[m], D, part, epi, [&] {
      if (m < 2) rxm_prefetch<D, D, WT>(ring, a.umlp3_w[m + 1], D);
      else rxm_prefetch<3 * D, D, WT>(ring, a.att0_w, D);
    });
  }
  // attention_mlp + fc_att (model :301-303)
  {
    FwdEpi e{s_bias + 6 * D, s_att1, D, a.att1 + (int64_t)v0 * D, D, true, mkdrop_rt(dbase, 12, 1, D), (uint32_t)v0, 1u};
    auto epi = [&](int r, int col, f32x4 v) { if (v0 + r < V) e(r, col, v); else st4(s_att1 + r * D + col, f32x4{0.f, 0.f, 0.f, 0.f}); };
    rxm_run<R, 3 * D, D, WT>(ring, s_u, 3 * D, a.att0_w, D, part, epi, [&] { rxm_prefetch<D, D, WT>(ring, a.att3_w, D); });
  }
  {
    FwdEpi e{s_bias + 7 * D, s_att2, D, a.att2 + (int64_t)v0 * D, D, true, mkdrop_rt(dbase, 13, 1, D), (uint32_t)v0, 1u};
    auto epi = [&](int r, int col, f32x4 v) { if (v0 + r < V) e(r, col, v); else st4(s_att2 + r * D + col, f32x4{0.f, 0.f, 0.f, 0.f}); };
    rxm_run<R, D, D, WT>(ring, s_att1, D, a.att3_w, D, part, epi, [&] { rxm_prefetch<D, D, WT>(ring, a.query_w[0], D); });
  }
  fwd_a_alpha<L>(a, sm, v0, V, true);
  fwd_a_fusion<L>(a, sm, v0, V, [](int) { return true; });
  // the 7 query MLPs -> multi_query [V, 7, 256] (model :324-332); text_hidden = query 5 (model :329, :370)
#pragma unroll 1
  for (int i = 0; i < 7; ++i) {
    FwdEpi e{s_bias + (8 + i) * D, s_q + i * D, NQ * D, a.q + (int64_t)v0 * NQ * D + i * D, (int64_t)NQ * D, true,
             mkdrop_rt(dbase, 14 + i, 1, D), (uint32_t)v0, 1u};
    float* th = (i == 5 && a.o_text_hidden) ? a.o_text_hidden + (int64_t)v0 * D : nullptr;
    auto epi = [&](int r, int col, f32x4 v) {
      if (v0 + r < V) {
        e(r, col, v);
        if (th) st4(th + (int64_t)r * D + col, ld4(s_q + r * NQ * D + i * D + col));
      } else {
        st4(s_q + r * NQ * D + i * D + col, f32x4{0.f, 0.f, 0.f, 0.f});
      }
    };
    rxm_run<R, D, D, WT>(ring, s_qin + i * R * D, D, a.query_w[i], D, part, epi,
                     [&] { rxm_prefetch<D, D, WT>(ring, i < 6 ? a.query_w[i + 1] : a.caq_w[0], D); });
  }
  // query_proj of the three Cross_Attention blocks (model :85): rows = (sample, query)
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    FwdEpi e{s_bias + (15 + m) * D, nullptr, 0, a.qp + ((int64_t)m * V + v0) * NQ * D, D, false, DropRT{}, 0u, 0u};
    auto epi = [&](int r, int col, f32x4 v) { if (v0 + r / NQ < V) e(r, col, v); };
    rxm_run<NQ * R, D, D, WT>(ring, s_q, D, a.caq_w[m], D, part, epi, [&] { if (m < 2) rxm_prefetch<D, D, WT>(ring, a.caq_w[m + 1], D); });
  }
}
template <int R, class WT>
__global__ __launch_bounds__(NTHR) void chain_fwd_a_kernel(const sdumc_chain_args a) { chain_fwd_a_body<R, WT>(a); }

// ------------------------------------------------------------------------------------------------------------------
// stage B forward (model :338-368)
// ------------------------------------------------------------------------------------------------------------------
template <int R, class WT>
__device__ __forceinline__ void chain_fwd_b_body(const sdumc_chain_args a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  using L = FwdB<R>;      // x: ca_out_m, one modality at a time
  float *part = sm + L::part, *s_x = sm + L::x, *s_c1 = sm + L::c1, *s_c = sm + L::c, *s_h = sm + L::h, *s_e1 = sm + L::e1, *s_e2 = sm + L::e2,
        *s_bias = sm + L::bias;
  const int V = a.V, v0 = blockIdx.x * R;
  const int64_t VQ = (int64_t)V * NQ;
  fwd_b_stage_bias(a, s_bias);

  const DropRT dbase = drop_resolve(a.drop);
  RingOf<D, D, WT> ring;
  rxm_prefetch<D, D, WT>(ring, a.cmlp0_w[0], D);
  fwd_b_load_alpha<L>(a, sm, v0, V);
  // cross_{audio,text,video}_mlp (model :338-340), rows = (sample, query)
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    __syncthreads();
    load_rows<NQ * R>(s_x, a.ca_out + (int64_t)m * VQ * D, D, D, v0 * NQ, V * NQ);
    __syncthreads();
    {
      FwdEpi e{s_bias + m * D, s_c1, D, a.c1 + ((int64_t)m * VQ + (int64_t)v0 * NQ) * D, D, true,
               mkdrop_rt(dbase, 27 + 2 * m, NQ, D), (uint32_t)(v0 * NQ), 1u};
      auto epi = [&](int r, int col, f32x4 v) { if (v0 * NQ + r < V * NQ) e(r, col, v); else st4(s_c1 + r * D + col, f32x4{0.f, 0.f, 0.f, 0.f}); };
      rxm_run<NQ * R, D, D, WT>(ring, s_x, D, a.cmlp0_w[m], D, part, epi, [&] { rxm_prefetch<D, H, WT>(ring, a.cmlp3_w[m], H); });
    }
    {
      FwdEpi e{s_bias + 3 * D + m * H, s_c + m * NQ * R * H, H, a.c + ((int64_t)m * VQ + (int64_t)v0 * NQ) * H, H, true,
               mkdrop_rt(dbase, 28 + 2 * m, NQ, H), (uint32_t)(v0 * NQ), 1u};
      float* ct = (m == 1 && a.o_cross_text) ? a.o_cross_text + (int64_t)v0 * NQ * H : nullptr;
      auto epi = [&](int r, int col, f32x4 v) {
        if (v0 * NQ + r < V * NQ) {
          e(r, col, v);
          if (ct) st4(ct + (int64_t)r * H + col, ld4(s_c + (m * NQ * R + r) * H + col));
        } else {
          st4(s_c + (m * NQ * R + r) * H + col, f32x4{0.f, 0.f, 0.f, 0.f});
        }
      };
      rxm_run<NQ * R, D, H, WT>(ring, s_c1, D, a.cmlp3_w[m], H, part, epi, [&] {
        if (m < 2) rxm_prefetch<D, D, WT>(ring, a.cmlp0_w[m + 1], D);
        else rxm_prefetch<NQ * H, D, WT>(ring, a.catt0_w, D);
      });
    }
  }
  fwd_b_hsum<L>(a, sm, v0, V, true);
  // cross_attention_mlp + cross_fc_att (model :352-354)
  {
    FwdEpi e{s_bias + 3 * D + 3 * H, s_e1, D, a.e1 + (int64_t)v0 * D, D, true, mkdrop_rt(dbase, 33, 1, D), (uint32_t)v0, 1u};
    auto epi = [&](int r, int col, f32x4 v) { if (v0 + r < V) e(r, col, v); else st4(s_e1 + r * D + col, f32x4{0.f, 0.f, 0.f, 0.f}); };
    rxm_run<R, NQ * H, D, WT>(ring, s_h, NQ * H, a.catt0_w, D, part, epi, [&] { rxm_prefetch<D, H, WT>(ring, a.catt3_w, H); });
  }
  {
    FwdEpi e{s_bias + 4 * D + 3 * H, s_e2, H, a.e2 + (int64_t)v0 * H, H, true, mkdrop_rt(dbase, 34, 1, H), (uint32_t)v0, 1u};
    auto epi = [&](int r, int col, f32x4 v) { if (v0 + r < V) e(r, col, v); else st4(s_e2 + r * H + col, f32x4{0.f, 0.f, 0.f, 0.f}); };
    rxm_run<R, D, H, WT>(ring, s_e1, D, a.catt3_w, H, part, epi, [] {});
  }
  fwd_b_tail<L>(a, sm, v0, V);
}
template <int R, class WT>
__global__ __launch_bounds__(NTHR) void chain_fwd_b_kernel(const sdumc_chain_args a) { chain_fwd_b_body<R, WT>(a); }

// ------------------------------------------------------------------------------------------------------------------
// stage B backward: d(vals, fused, rnc, cross_text) -> d_ca_out [3][V,7,256], d_alpha (second-level part), and every
// pre-activation gradient the dW GEMMs need (d_rnc is the caller's; d_r1, d_z, d_beta, d_e2, d_e1, d_c, d_c1)
// ------------------------------------------------------------------------------------------------------------------
template <int R, class WT>
__device__ __forceinline__ void chain_bwd_b_body(const sdumc_chain_args a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  using L = BwdB<R>;      // dc, c1: one modality at a time
  float *part = sm + L::part, *s_dz = sm + L::dz, *s_dh = sm + L::dh, *s_e1 = sm + L::e1, *s_dc = sm + L::dc, *s_c1 = sm + L::c1;
  const int V = a.V, v0 = blockIdx.x * R;
  const int64_t VQ = (int64_t)V * NQ;
  const float sc = a.relu_scale;

  RingOf<H, D, WT> ring;           // catt3 / cmlp3 / cmlp0 backward: NB = 1, 4 deep
  RingOf<D, NQ * H, WT> ring4;     // catt0 backward: 896 output columns = 4 blocks, 2 deep
  rxm_prefetch<H, D, WT>(ring, a.catt3_w, D);
  bwd_b_load_head<L>(a, sm, v0, V);
  __syncthreads();
  bwd_b_rnc<L>(a, sm, v0, V, true);
  bwd_b_zpool<L>(a, sm, v0, V, true);
  // 11'. cross_fc_att: d_e2 = (d_beta W_cfa) [e2 > 0] s ; cross_attention_mlp.3: d_e1 = (d_e2 W) [e1 > 0] s ; .0: d_h += d_e1 W
  bwd_b_de2<L>(a, sm, v0, V, sc, true);
  {
    BwdEpi e{nullptr, 0, s_e1, D, sc, s_e1, D, a.d_e1 + (int64_t)v0 * D, D};
    auto epi = [&](int r, int col, f32x4 v) { if (v0 + r < V) e(r, col, v); else st4(s_e1 + r * D + col, f32x4{0.f, 0.f, 0.f, 0.f}); };
    rxm_run<R, H, D, WT>(ring, s_dz, H, a.catt3_w, D, part, epi, [&] { rxm_prefetch<D, NQ * H, WT>(ring4, a.catt0_w, NQ * H); });
  }
  {
    BwdEpi e{s_dh, NQ * H, nullptr, 0, 1.f, s_dh, NQ * H, nullptr, 0};
    auto epi = [&](int r, int col, f32x4 v) { e(r, col, v); };
    rxm_run<R, D, NQ * H, WT>(ring4, s_e1, D, a.catt0_w, NQ * H, part, epi, [&] { rxm_prefetch<H, D, WT>(ring, a.cmlp3_w[0], D); });
  }
  // 10'. modality-weighted sum backward, then 9'. cross_*_mlp, one modality at a time
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    bwd_b_dc<L>(a, sm, s_dc, m, v0, V, sc, true);
    load_rows<NQ * R>(s_c1, a.c1 + (int64_t)m * VQ * D, D, D, v0 * NQ, V * NQ);
    __syncthreads();
    {
      BwdEpi e{nullptr, 0, s_c1, D, sc, s_c1, D, a.d_c1 + ((int64_t)m * VQ + (int64_t)v0 * NQ) * D, D};
      auto epi = [&](int r, int col, f32x4 v) { if (v0 * NQ + r < V * NQ) e(r, col, v); else st4(s_c1 + r * D + col, f32x4{0.f, 0.f, 0.f, 0.f}); };
      rxm_run<NQ * R, H, D, WT>(ring, s_dc, H, a.cmlp3_w[m], D, part, epi, [&] { rxm_prefetch<D, D, WT>(ring, a.cmlp0_w[m], D); });
    }
    {
      BwdEpi e{nullptr, 0, nullptr, 0, 1.f, nullptr, 0, a.d_ca_out + ((int64_t)m * VQ + (int64_t)v0 * NQ) * D, D};
      auto epi = [&](int r, int col, f32x4 v) { if (v0 * NQ + r < V * NQ) e(r, col, v); };
      rxm_run<NQ * R, D, D, WT>(ring, s_c1, D, a.cmlp0_w[m], D, part, epi, [&] { if (m < 2) rxm_prefetch<H, D, WT>(ring, a.cmlp3_w[m + 1], D); });
    }
  }
}
template <int R, class WT>
__global__ __launch_bounds__(NTHR) void chain_bwd_b_kernel(const sdumc_chain_args a) { chain_bwd_b_body<R, WT>(a); }

// ------------------------------------------------------------------------------------------------------------------
// stage A backward: d_qp [3][V,7,256] (+ d text_hidden, + d_alpha from stage B) -> d_hpre [3][V,256] and the
// pre-activation gradients d_q, d_qin (as d of the query MLP inputs), d_att2, d_att1, d_u, d_u1
// ------------------------------------------------------------------------------------------------------------------
template <int R, class WT>
__device__ __forceinline__ void chain_bwd_a_body(const sdumc_chain_args a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  using L = BwdA<R>;      // x: d_qp_m, one modality at a time
  float *part = sm + L::part, *s_x = sm + L::x, *s_dq = sm + L::dq, *s_dqin = sm + L::dqin, *s_u = sm + L::u, *s_du = sm + L::du, *s_a2 = sm + L::a2,
        *s_a1 = sm + L::a1, *s_u1 = sm + L::u1;
  const int V = a.V, v0 = blockIdx.x * R;
  const int64_t VD = (int64_t)V * D, VQ = (int64_t)V * NQ;
  const float sc = a.relu_scale;

  RingOf<D, D, WT> ring;
  RingOf<D, 3 * D, WT> ring3;      // att0 backward: 768 output columns = 3 blocks, 2 deep
  rxm_prefetch<D, D, WT>(ring, a.caq_w[0], D);
  load_rows<R>(s_u, a.u, 3 * D, 3 * D, v0, V);
  load_rows<R>(s_a2, a.att2, D, D, v0, V);
  load_rows<R>(s_a1, a.att1, D, D, v0, V);
  for (int m = 0; m < 3; ++m) load_rows<R>(s_u1 + m * R * D, a.u1 + m * VD, D, D, v0, V);
  bwd_a_load_alpha<L>(a, sm, v0, V);
  // 7'. query_proj: d_q = sum_m d_qp_m W_q[m]  (accumulated in LDS over the three modalities)
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    __syncthreads();
    load_rows<NQ * R>(s_x, a.d_qp + (int64_t)m * VQ * D, D, D, v0 * NQ, V * NQ);
    __syncthreads();
    BwdEpi e{m > 0 ? s_dq : nullptr, D, nullptr, 0, 1.f, s_dq, D, nullptr, 0};
    auto epi = [&](int r, int col, f32x4 v) { e(r, col, v); };
    rxm_run<NQ * R, D, D, WT>(ring, s_x, D, a.caq_w[m], D, part, epi,
                          [&] { rxm_prefetch<D, D, WT>(ring, m < 2 ? a.caq_w[m + 1] : a.query_w[0], D); });
  }
  // 6'. mask of q -> d_q (pre-activation); query MLPs
  bwd_a_mask_q<L, D>(a, sm, v0, V, sc, 0, [](f32x4 g, float* lds, float* hbm, bool live) {
    st4(lds, g);
    if (live) st4(hbm, g);
  });
  __syncthreads();
#pragma unroll 1
  for (int i = 0; i < 7; ++i) {
    BwdEpi e{nullptr, 0, nullptr, 0, 1.f, s_dqin + i * R * D, D, a.d_qin + i * VD + (int64_t)v0 * D, D};
    auto epi = [&](int r, int col, f32x4 v) { if (v0 + r < V) e(r, col, v); else st4(s_dqin + (i * R + r) * D + col, f32x4{0.f, 0.f, 0.f, 0.f}); };
    rxm_run<R, D, D, WT>(ring, s_dq + i * D, NQ * D, a.query_w[i], D, part, epi,
                     [&] { rxm_prefetch<D, D, WT>(ring, i < 6 ? a.query_w[i + 1] : a.att3_w, D); });
  }
  bwd_a_fusion<L>(a, sm, v0, V, true);
  // 4'. fc_att: d_att2 ; attention_mlp.3: d_att1 = (d_att2 W) [att1 > 0] s ; .0: d_u = (d_u + d_att1 W) [u > 0] s
  bwd_a_datt2<L>(a, sm, v0, V, sc, true);
  {
    BwdEpi e{nullptr, 0, s_a1, D, sc, s_a1, D, a.d_att1 + (int64_t)v0 * D, D};
    auto epi = [&](int r, int col, f32x4 v) { if (v0 + r < V) e(r, col, v); else st4(s_a1 + r * D + col, f32x4{0.f, 0.f, 0.f, 0.f}); };
    rxm_run<R, D, D, WT>(ring, s_a2, D, a.att3_w, D, part, epi, [&] { rxm_prefetch<D, 3 * D, WT>(ring3, a.att0_w, 3 * D); });
  }
  {
    BwdEpi e{s_du, 3 * D, s_u, 3 * D, sc, s_du, 3 * D, a.d_u + (int64_t)v0 * 3 * D, 3 * D};
    auto epi = [&](int r, int col, f32x4 v) { if (v0 + r < V) e(r, col, v); else st4(s_du + r * 3 * D + col, f32x4{0.f, 0.f, 0.f, 0.f}); };
    rxm_run<R, D, 3 * D, WT>(ring3, s_a1, D, a.att0_w, 3 * D, part, epi, [&] { rxm_prefetch<D, D, WT>(ring, a.umlp3_w[0], D); });
  }
  // 3'. audio / text / video_mlp: d_u1 = (d_u_m W3) [u1 > 0] s ; d_hpre = d_u1 W0
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    {
      BwdEpi e{nullptr, 0, s_u1 + m * R * D, D, sc, s_u1 + m * R * D, D, a.d_u1 + m * VD + (int64_t)v0 * D, D};
      auto epi = [&](int r, int col, f32x4 v) { if (v0 + r < V) e(r, col, v); else st4(s_u1 + (m * R + r) * D + col, f32x4{0.f, 0.f, 0.f, 0.f}); };
      rxm_run<R, D, D, WT>(ring, s_du + m * D, 3 * D, a.umlp3_w[m], D, part, epi, [&] { rxm_prefetch<D, D, WT>(ring, a.umlp0_w[m], D); });
    }
    {
      BwdEpi e{nullptr, 0, nullptr, 0, 1.f, nullptr, 0, a.d_hpre + m * VD + (int64_t)v0 * D, D};
      auto epi = [&](int r, int col, f32x4 v) { if (v0 + r < V) e(r, col, v); };
      rxm_run<R, D, D, WT>(ring, s_u1 + m * R * D, D, a.umlp0_w[m], D, part, epi, [&] { if (m < 2) rxm_prefetch<D, D, WT>(ring, a.umlp3_w[m + 1], D); });
    }
  }
}
template <int R, class WT>
__global__ __launch_bounds__(NTHR) void chain_bwd_a_kernel(const sdumc_chain_args a) { chain_bwd_a_body<R, WT>(a); }

// transposed mirror of the utterance-level weights: dst[i][o] = src[o][i] for up to 40 matrices in one launch
struct TransposeList {
  int n;
  struct { int64_t off; int32_t out, in; } e[40];
};
__global__ __launch_bounds__(256) void transpose_params_kernel(const float* __restrict__ src, float* __restrict__ dst, const TransposeList tl) {
  __shared__ float t[32][33];
  const auto& e = tl.e[blockIdx.z];
  const int o0 = blockIdx.y * 32, i0 = blockIdx.x * 32;
  if (o0 >= e.out || i0 >= e.in) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8)
    if (o0 + k < e.out && i0 + tx < e.in) t[k][tx] = src[e.off + (int64_t)(o0 + k) * e.in + i0 + tx];
  __syncthreads();
  for (int k = ty; k < 32; k += 8)
    if (i0 + k < e.in && o0 + tx < e.out) dst[e.off + (int64_t)(i0 + k) * e.out + o0 + tx] = t[tx][k];
}

}  // namespace

// which: 0 = stage A forward, 1 = stage B forward, 2 = stage B backward, 3 = stage A backward
extern "C" int sdumc_chain_launch_(const sdumc_chain_args* a, int which, void* stream) {
  if (!a || a->V <= 0 || which < 0 || which > 3) return SDUMC_EINVAL;
  constexpr int R = 2;
  typedef unsigned short bf;
  static sdumc_dev_once attr;
  if (sdumc_once_per_device(attr, [] {
        return sdumc_set_dyn_lds(chain_fwd_a_kernel<R, float>, FwdA<R>::bytes) && sdumc_set_dyn_lds(chain_fwd_b_kernel<R, float>, FwdB<R>::bytes) &&
               sdumc_set_dyn_lds(chain_bwd_b_kernel<R, float>, BwdB<R>::bytes) && sdumc_set_dyn_lds(chain_bwd_a_kernel<R, float>, BwdA<R>::bytes) &&
               sdumc_set_dyn_lds(chain_fwd_a_kernel<R, bf>, FwdA<R>::bytes) && sdumc_set_dyn_lds(chain_fwd_b_kernel<R, bf>, FwdB<R>::bytes) &&
               sdumc_set_dyn_lds(chain_bwd_b_kernel<R, bf>, BwdB<R>::bytes) && sdumc_set_dyn_lds(chain_bwd_a_kernel<R, bf>, BwdA<R>::bytes);
      }) != SDUMC_OK)
    return SDUMC_ELAUNCH;
  const dim3 grid((a->V + R - 1) / R), blk(NTHR);
  hipStream_t st = as_stream(stream);
  // (one entry point per stage and weight type: the whole device build carries no packed fp32 operations -- Makefile, NOPACK --,
  //  so the "_np_" twins of round 4 compiled to the same code and are gone)
  if (a->w_bf16) {
    switch (which) {
      case 0: hipLaunchKernelGGL((chain_fwd_a_kernel<R, bf>), grid, blk, FwdA<R>::bytes, st, *a); break;
      case 1: hipLaunchKernelGGL((chain_fwd_b_kernel<R, bf>), grid, blk, FwdB<R>::bytes, st, *a); break;
      case 2: hipLaunchKernelGGL((chain_bwd_b_kernel<R, bf>), grid, blk, BwdB<R>::bytes, st, *a); break;
      default: hipLaunchKernelGGL((chain_bwd_a_kernel<R, bf>), grid, blk, BwdA<R>::bytes, st, *a); break;
    }
  } else {
    switch (which) {
      case 0: hipLaunchKernelGGL((chain_fwd_a_kernel<R, float>), grid, blk, FwdA<R>::bytes, st, *a); break;
      case 1: hipLaunchKernelGGL((chain_fwd_b_kernel<R, float>), grid, blk, FwdB<R>::bytes, st, *a); break;
      case 2: hipLaunchKernelGGL((chain_bwd_b_kernel<R, float>), grid, blk, BwdB<R>::bytes, st, *a); break;
      default: hipLaunchKernelGGL((chain_bwd_a_kernel<R, float>), grid, blk, BwdA<R>::bytes, st, *a); break;
    }
  }
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

// dst[off .. ] = transpose of the n listed [out][in] matrices of src (same offsets): the forward chain's weight layout
extern "C" int sdumc_chain_transpose_(const float* src, float* dst, const int64_t* offs, const int32_t* outs, const int32_t* ins, int n,
                                      void* stream) {
  if (!src || !dst || n <= 0 || n > 40) return SDUMC_EINVAL;
  TransposeList tl;
  tl.n = n;
  int mo = 0, mi = 0;
  for (int i = 0; i < n; ++i) {
    tl.e[i].off = offs[i];
    tl.e[i].out = outs[i];
    tl.e[i].in = ins[i];
    mo = outs[i] > mo ? outs[i] : mo;
    mi = ins[i] > mi ? ins[i] : mi;
  }
  hipLaunchKernelGGL(transpose_params_kernel, dim3((mi + 31) / 32, (mo + 31) / 32, n), dim3(256), 0, as_stream(stream), src, dst, tl);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

SDUMC_PRELOAD_HOOK(chain)      // (common.h)
