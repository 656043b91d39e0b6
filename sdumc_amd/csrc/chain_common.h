// chain_common.h -- what chain.hip (one workgroup per R samples) and chain_cluster.hip (the same stages with every layer's output
// columns split over a cluster of workgroups) share: the rows-x-matrix engine, each stage's LDS layout, and every section of the
// network that lies between the split layers.  See chain.hip for the design notes.
// (These kernels must not issue packed fp32 VALU operations beside bf16 MFMA neighbours: the whole library is built without
//  them -- Makefile, NOPACK.)
#pragma once
#include <type_traits>

#include "common.h"

namespace {

constexpr int D = SDUMC_D, H = SDUMC_H, NQ = SDUMC_NQ, RD = SDUMC_RNC_DIM;
constexpr int NTHR = 512, NWV = 8;
constexpr int PART_FLOATS = NWV * 7 * D;   // partial-sum area: 8 waves x up to 7 rows x 256 columns (or 2 rows x 896)

__device__ __forceinline__ DropRT mkdrop_rt(const DropRT& base, uint32_t site, uint32_t rows, uint32_t width) {
  DropRT d = base;     // resolved once per kernel (seed / call counter come from device memory)
  d.site = site;
  d.rows = rows;
  d.qwidth = width >> 2;
  d.bits = nullptr;
  return d;
}

// ------------------------------------------------------------------------------------------------------------------
// rows x matrix.  in_lds: [ROWS][ld_in] floats in LDS; M: global row-major [I][ldm]; result rows are handed, 4 columns at
// a time, to epi(r, col, f32x4) (every (r, col quad) exactly once, by some thread).  `part` is PART_FLOATS of LDS scratch.
// All 512 threads must call it (barriers inside); it ends with a barrier, so LDS written by epi is visible afterwards.
//
// The weight rows stream through a register ring DEP iterations deep (one iteration = 4 rows of M per lane group, 16-byte
// loads): DEP - 1 iterations stay in flight under the FMAs.  The ring is an argument: rxm_prefetch() issues a layer's first
// DEP - 1 iterations, rxm_run() consumes them -- and calls `hook` between its k-loop and its reduction, where the caller
// prefetches the NEXT layer's first rows, so that their latency (and the L2 miss of a cold weight matrix) passes under this
// layer's reduction, epilogue and barriers instead of at the head of the next one: the chain is a sequence of ~20 dependent
// layers per stage and that head latency was half of its time.
// ------------------------------------------------------------------------------------------------------------------
// WT = float, or unsigned short for bf16 weights (the engine's bf16-storage mode streams bf16 copies of the utterance-level
// weights: half the bytes of the stream this chain is bound by; accumulation stays fp32)
template <int I, int O, class WT>
struct RxmGeom {
  static constexpr int EPL = 16 / (int)sizeof(WT);      // weight elements (output columns) per lane per 16-byte load
  static constexpr int QPL = EPL / 4;                   // f32x4 accumulators per lane per block
  static constexpr int OG = O / EPL;                    // lane-groups of output columns
  static constexpr int OGW = OG >= 64 ? 64 : OG;        // lanes that cover one row of M
  static constexpr int S = 64 / OGW;                    // rows of M covered by one wave-load (1, 2, 4 or 8)
  static constexpr int NB = (OG + 63) / 64;             // column blocks of 64 lanes
  static constexpr int BW = 64 * EPL;                   // columns per block
  static constexpr int UNITS = I / (4 * S);             // 4-row groups of M per lane group
  // 8 waves, or 7 when that makes the per-wave trip count even where 8 leaves it odd (I = 896 at S = 4: 7 x 8 instead of 8 x 7,
  // so that the register ring can run 4 deep)
  static constexpr int WAVES = UNITS >= NWV ? ((UNITS % 8 == 0 && (UNITS / 8) % 2 == 1 && UNITS % 7 == 0 && (UNITS / 7) % 2 == 0) ? 7 : NWV)
                                            : UNITS;
  static constexpr int IW = I / WAVES;                  // rows of M per wave
  static constexpr int ITER = IW / (4 * S);
  // ring depth: 4 for fp32 single-block layers; bf16 lanes carry two accumulator quads per row, so their ring stays 2 deep
  // (deeper spilled at 14 rows)
  static constexpr int DEP = (ITER % 4 == 0 && NB == 1 && EPL == 4) ? 4 : ((ITER % 2 == 0) ? 2 : 1);
  // PF1 (opt-in, chain_cluster.hip): a single-iteration layer prefetches that one iteration too
  static constexpr bool ONE = ITER == 1;
  static_assert(I % (4 * S * WAVES) == 0 && ITER >= 1, "k range must split evenly");
  static_assert(S <= 8 && O % EPL == 0, "at least 8 lane-groups of output columns");
};
template <int NB>
struct WRing {
  uint4 w[4][4][NB];          // raw 16-byte loads (4 fp32 or 8 bf16), expanded when they are multiplied; a layer uses the first
                              // DEP (1, 2 or 4) slots, so that layers of different depth can hand one ring on to each other
};
template <int I, int O, class WT>
using RingOf = WRing<RxmGeom<I, O, WT>::NB>;

template <int I, int O, class WT, int NBv>
__device__ __forceinline__ void rxm_load(uint4 (&dst)[4][NBv], const WT* mp, int j, int ldm, int cg) {
  using G = RxmGeom<I, O, WT>;
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int b = 0; b < G::NB; ++b) {
      if (b * 64 + cg < G::OG) dst[e][b] = *reinterpret_cast<const uint4*>(mp + (size_t)(j * 4 * G::S + e) * ldm + b * G::BW);
      else dst[e][b] = uint4{0u, 0u, 0u, 0u};
    }
}

template <int I, int O, class WT, bool PF1 = false>
__device__ __forceinline__ void rxm_prefetch(RingOf<I, O, WT>& ring, const void* __restrict__ Mv, int ldm) {
  using G = RxmGeom<I, O, WT>;
  if constexpr (PF1 && G::ONE) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave < G::WAVES) {
      const int sq = lane / G::OGW, cg = lane % G::OGW;
      const WT* mp = static_cast<const WT*>(Mv) + (size_t)(wave * G::IW + 4 * sq) * ldm + G::EPL * cg;
      rxm_load<I, O, WT, G::NB>(ring.w[0], mp, 0, ldm, cg);
    }
  } else if constexpr (G::DEP > 1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave < G::WAVES) {
      const int sq = lane / G::OGW, cg = lane % G::OGW;
      const WT* mp = static_cast<const WT*>(Mv) + (size_t)(wave * G::IW + 4 * sq) * ldm + G::EPL * cg;
#pragma unroll
      for (int d = 0; d < G::DEP - 1; ++d) rxm_load<I, O, WT, G::NB>(ring.w[d], mp, d, ldm, cg);
    }
  }
}

template <int ROWS, int I, int O, class WT, bool PF1 = false, class Epi, class Hook>
__device__ __forceinline__ void rxm_run(RingOf<I, O, WT>& ring, const float* in_lds, int ld_in, const void* __restrict__ Mv, int ldm,
                                        float* part, Epi&& epi, Hook&& hook) {
  using G = RxmGeom<I, O, WT>;
  constexpr int OG = G::OG, OGW = G::OGW, S = G::S, NB = G::NB, WAVES = G::WAVES, IW = G::IW, ITER = G::ITER, DEP = G::DEP;
  constexpr int EPL = G::EPL, QPL = G::QPL, BW = G::BW;
  constexpr int RC = ROWS > 7 ? 7 : ROWS;        // rows per reduction round
  static_assert(NWV * RC * O <= PART_FLOATS, "partial-sum area too small");
  static_assert(ROWS % RC == 0, "rows per round");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sq = lane / OGW, cg = lane % OGW;

  f32x4 acc[ROWS][NB][QPL];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int q = 0; q < QPL; ++q) acc[r][b][q] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (wave < WAVES) {
    const int i0 = wave * IW + 4 * sq;
    const WT* mp = static_cast<const WT*>(Mv) + (size_t)i0 * ldm + EPL * cg;
    auto fma = [&](int j, const uint4 (&ws)[4][NB]) {
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const f32x4 x = ld4(in_lds + r * ld_in + i0 + j * 4 * S);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            const uint4 u = ws[e][b];
            if constexpr (QPL == 1) {
              acc[r][b][0] += f32x4{__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w)} * x[e];
            } else {        // 8 bf16: low halves are the even columns
              acc[r][b][0] += f32x4{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                                    __uint_as_float(u.y & 0xffff0000u)} * x[e];
              acc[r][b][1] += f32x4{__uint_as_float(u.z << 16), __uint_as_float(u.z & 0xffff0000u), __uint_as_float(u.w << 16),
                                    __uint_as_float(u.w & 0xffff0000u)} * x[e];
            }
          }
        // (keeps the scheduler from hoisting every row's LDS read of several iterations to the top: with 14 rows that
        // alone is 56 live registers per iteration in flight, and the kernel spilled)
        if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    if constexpr (PF1 && G::ONE) {
      fma(0, ring.w[0]);                       // already loaded by rxm_prefetch<.., true>
    } else if constexpr (DEP == 1) {
#pragma unroll
      for (int j = 0; j < ITER; ++j) {
        rxm_load<I, O, WT, NB>(ring.w[0], mp, j, ldm, cg);
        fma(j, ring.w[0]);
      }
    } else {
#pragma unroll 1
      for (int jb = 0; jb < ITER; jb += DEP) {
#pragma unroll
        for (int d = 0; d < DEP; ++d) {
          const int j = jb + d;
          const int jn = j + DEP - 1 < ITER ? j + DEP - 1 : ITER - 1;     // past the end: a harmless re-load, no branch
          rxm_load<I, O, WT, NB>(ring.w[(d + DEP - 1) % DEP], mp, jn, ldm, cg);
          fma(j, ring.w[d]);
        }
      }
    }
    if constexpr (S >= 2) {
#pragma unroll
      for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int q = 0; q < QPL; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              acc[r][b][q][c] += __shfl_xor(acc[r][b][q][c], 32, 64);
              if constexpr (S >= 4) acc[r][b][q][c] += __shfl_xor(acc[r][b][q][c], 16, 64);
              if constexpr (S == 8) acc[r][b][q][c] += __shfl_xor(acc[r][b][q][c], 8, 64);
            }
    }
  }
  hook();        // the next layer's first weight rows start moving here
#pragma unroll
  for (int r0 = 0; r0 < ROWS; r0 += RC) {
    if (wave < WAVES && sq == 0) {
#pragma unroll
      for (int r = 0; r < RC; ++r)
#pragma unroll
        for (int b = 0; b < NB; ++b)
          if (b * 64 + cg < OG) {
#pragma unroll
            for (int q = 0; q < QPL; ++q) st4(part + (wave * RC + r) * O + b * BW + EPL * cg + 4 * q, acc[r0 + r][b][q]);
          }
    }
    __syncthreads();
    for (int u = tid; u < RC * (O / 4); u += NTHR) {
      const int r = u / (O / 4), cq = u - r * (O / 4);
      f32x4 v = ld4(part + r * O + 4 * cq);
#pragma unroll
      for (int ww = 1; ww < WAVES; ++ww) v += ld4(part + (ww * RC + r) * O + 4 * cq);
      epi(r0 + r, 4 * cq, v);
    }
    __syncthreads();
  }
}

// stand-alone form (fp32 weights): prefetch + run, nothing chained behind it
template <int ROWS, int I, int O, class Epi>
__device__ __forceinline__ void rows_x_matrix(const float* in_lds, int ld_in, const float* __restrict__ M, int ldm, float* part,
                                              Epi&& epi) {
  RingOf<I, O, float> ring;
  rxm_prefetch<I, O, float>(ring, M, ldm);
  rxm_run<ROWS, I, O, float>(ring, in_lds, ld_in, M, ldm, part, epi, [] {});
}

// y = drop(relu(v + bias)): `col` is the layer's global output column, bias_lds the layer's staged bias row
__device__ __forceinline__ f32x4 fwd_val(f32x4 v, const float* bias_lds, int col, bool relu, const DropRT& drop, uint32_t vrow) {
  v += ld4(bias_lds + col);
  if (relu) {
    v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f);
  }
  if (drop.enabled) v *= drop_mask4(drop, vrow, (uint32_t)(col >> 2));
  return v;
}
// [y > 0] * scale: the backward mask of a layer, from its saved post-dropout output y
__device__ __forceinline__ f32x4 mask_val(f32x4 v, f32x4 y, float sc) {
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = y[j] > 0.f ? v[j] * sc : 0.f;
  return v;
}

// y = drop(relu(v + bias)) -> LDS and HBM (forward layer epilogue)
struct FwdEpi {
  const float* bias;
  float* out_lds;  int ld_lds;          // may be nullptr
  float* out_g;    int64_t ld_g;        // row r of this workgroup -> out_g + r * ld_g (already offset to the first row)
  bool relu;
  DropRT drop;                           // drop.enabled == 0: none
  uint32_t vrow0, vrow_stride;           // dropout row of local row r = vrow0 + r * vrow_stride ... see call sites
  __device__ __forceinline__ void operator()(int r, int col, f32x4 v) const {
    v = fwd_val(v, bias, col, relu, drop, vrow0 + (uint32_t)r * vrow_stride);
    if (out_lds) st4(out_lds + r * ld_lds + col, v);
    if (out_g) st4(out_g + (int64_t)r * ld_g + col, v);
  }
};

// dx = v (+ add) masked by the saved post-dropout output y of the layer below: [y > 0] * scale (backward epilogue)
struct BwdEpi {
  const float* add_lds;  int ld_add;     // optional term added before the mask (LDS), may be nullptr
  const float* y_lds;    int ld_y;       // optional mask source (LDS), may be nullptr (= plain)
  float scale;
  float* out_lds;  int ld_lds;
  float* out_g;    int64_t ld_g;
  __device__ __forceinline__ void operator()(int r, int col, f32x4 v) const {
    if (add_lds) v += ld4(add_lds + r * ld_add + col);
    if (y_lds) v = mask_val(v, ld4(y_lds + r * ld_y + col), scale);
    if (out_lds) st4(out_lds + r * ld_lds + col, v);
    if (out_g) st4(out_g + (int64_t)r * ld_g + col, v);
  }
};

// rows [v0, v0 + R) of a global [.., width] tensor -> LDS [R][width] (rows beyond V are zero-filled)
template <int R>
__device__ __forceinline__ void load_rows(float* dst_lds, const float* src, int64_t ld, int width, int v0, int V) {
  const int q = width >> 2;
  for (int u = threadIdx.x; u < R * q; u += NTHR) {
    const int r = u / q, c = u - r * q;
    st4(dst_lds + r * width + 4 * c, v0 + r < V ? ld4(src + (int64_t)(v0 + r) * ld + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f});
  }
}

// load_rows in two halves, for a stage head that wants every request in flight before its first wait: rows_request asks for the
// rows into registers, rows_store puts them into LDS [ROWS][WIDTH] (rows beyond V zero-filled).  The request is branch-free -- a unit
// without a live row re-reads the last live one and is zeroed at the store: behind a branch around a load the compiler has to wait
// for every older load as well, which is the serial chain of round trips the split is there to remove.  v0 < V.
template <int ROWS, int WIDTH>
struct RowsReg {
  static constexpr int Q = WIDTH / 4, N = (ROWS * Q + NTHR - 1) / NTHR;
  f32x4 v[N];
};
template <int ROWS, int WIDTH>
__device__ __forceinline__ void rows_request(RowsReg<ROWS, WIDTH>& g, const float* src, int64_t ld, int v0, int V) {
  constexpr int Q = WIDTH / 4;
#pragma unroll
  for (int k = 0; k < RowsReg<ROWS, WIDTH>::N; ++k) {
    const int u = min((int)threadIdx.x + k * NTHR, ROWS * Q - 1), r = u / Q, c = u - r * Q;
    g.v[k] = ld4(src + (int64_t)min(v0 + r, V - 1) * ld + 4 * c);
  }
}
template <int ROWS, int WIDTH>
__device__ __forceinline__ void rows_store(const RowsReg<ROWS, WIDTH>& g, float* dst_lds, int v0, int V, bool zero = false) {
  constexpr int Q = WIDTH / 4;
#pragma unroll
  for (int k = 0; k < RowsReg<ROWS, WIDTH>::N; ++k) {
    const int u = threadIdx.x + k * NTHR;
    if (u < ROWS * Q) st4(dst_lds + 4 * u, (v0 + u / Q < V && !zero) ? g.v[k] : f32x4{0.f, 0.f, 0.f, 0.f});
  }
}

// ------------------------------------------------------------------------------------------------------------------
// LDS layouts: float offsets into a stage's dynamic LDS.  One definition per stage: the kernel takes its pointers from it and the
// host takes the launch's dynamic-LDS bytes from `bytes`.  PART = the partial-sum area (PART_FLOATS here, PARTC in
// chain_cluster.hip); a plane count is 1 where chain.hip walks one modality at a time and 3 where chain_cluster.hip keeps the
// three modalities side by side.
// ------------------------------------------------------------------------------------------------------------------
template <int R_, int PART>
struct FwdALds {
  static constexpr int R = R_;
  static constexpr int part = 0;
  static constexpr int hpre = part + PART;            // [3][R][256]
  static constexpr int u1 = hpre + 3 * R * D;         // [3][R][256]
  static constexpr int u = u1 + 3 * R * D;            // [R][768]
  static constexpr int att1 = u + 3 * R * D;          // [R][256]
  static constexpr int att2 = att1 + R * D;           // [R][256]
  static constexpr int alpha = att2 + R * D;          // [R][4]
  static constexpr int qin = alpha + R * 4;           // [7][R][256]
  static constexpr int q = qin + 7 * R * D;           // [R][7][256]
  static constexpr int bias = q + 7 * R * D;          // [18][256]: every bias of the stage (an epilogue then waits on no global load)
  static constexpr int total = bias + 18 * D;
  static constexpr size_t bytes = sizeof(float) * total;
};
// NX planes of x (ca_out; chain_cluster.hip's three also take c1 afterwards), NC1 planes of c1 of their own
template <int R_, int PART, int NX, int NC1>
struct FwdBLds {
  static constexpr int R = R_;
  static constexpr int part = 0;
  static constexpr int x = part + PART;               // [NX][7R][256]
  static constexpr int c1 = x + NX * NQ * R * D;      // [NC1][7R][256]
  static constexpr int c = c1 + NC1 * NQ * R * D;     // [3][7R][128]
  static constexpr int h = c + 3 * NQ * R * H;        // [R][896]
  static constexpr int e1 = h + R * NQ * H;           // [R][256]
  static constexpr int e2 = e1 + R * D;               // [R][128]
  static constexpr int z = e2 + R * H;                // [R][128]
  static constexpr int r1 = z + R * H;                // [R][64]
  static constexpr int alpha = r1 + R * RD;           // [R][4]
  static constexpr int beta = alpha + 4 * R;          // [R][8]
  static constexpr int bias = beta + 8 * R;           // cmlp0 [3][256], cmlp3 [3][128], catt0 [256], catt3 [128], rnc0 [64], rnc2 [64]
  static constexpr int total = bias + 4 * D + 4 * H + 2 * RD;
  static constexpr size_t bytes = sizeof(float) * total;
};
// NP planes of d_c and of c1
template <int R_, int PART, int NP>
struct BwdBLds {
  static constexpr int R = R_;
  static constexpr int part = 0;
  static constexpr int g = part + PART;               // [R][64]   d_rnc
  static constexpr int r1 = g + R * RD;               // [R][64]   saved r1, then d_r1
  static constexpr int dz = r1 + R * RD;              // [R][128]  d_z, then d_e2
  static constexpr int h = dz + R * H;                // [R][896]  saved h
  static constexpr int dh = h + R * NQ * H;           // [R][896]
  static constexpr int e2 = dh + R * NQ * H;          // [R][128]  saved e2
  static constexpr int e1 = e2 + R * H;               // [R][256]  saved e1, then d_e1
  static constexpr int dc = e1 + R * D;               // [NP][7R][128] d_c
  static constexpr int c1 = dc + NP * NQ * R * H;     // [NP][7R][256] saved c1, then d_c1
  static constexpr int beta = c1 + NP * NQ * R * D;   // [R][8]
  static constexpr int dbeta = beta + 8 * R;          // [R][8]
  static constexpr int alpha = dbeta + 8 * R;         // [R][4]
  static constexpr int dvals = alpha + 4 * R;         // [R] (+ 3 R unused)
  static constexpr int total = dvals + 4 * R;
  static constexpr size_t bytes = sizeof(float) * total;
};
// NX planes of x (d_qp)
template <int R_, int PART, int NX>
struct BwdALds {
  static constexpr int R = R_;
  static constexpr int part = 0;
  static constexpr int x = part + PART;               // [NX][7R][256]  d_qp
  static constexpr int dq = x + NX * NQ * R * D;      // [R][7][256]
  static constexpr int dqin = dq + NQ * R * D;        // [7][R][256]
  static constexpr int u = dqin + NQ * R * D;         // [R][768]  saved u
  static constexpr int du = u + 3 * R * D;            // [R][768]
  static constexpr int a2 = du + 3 * R * D;           // [R][256]  saved att2, then d_att2
  static constexpr int a1 = a2 + R * D;               // [R][256]  saved att1, then d_att1
  static constexpr int u1 = a1 + R * D;               // [3][R][256] saved u1, then d_u1
  static constexpr int alpha = u1 + 3 * R * D;        // [R][4]
  static constexpr int dalpha = alpha + 4 * R;        // [R][4]
  static constexpr int total = dalpha + 4 * R;
  static constexpr size_t bytes = sizeof(float) * total;
};

// ------------------------------------------------------------------------------------------------------------------
// The sections of the four stages that lie between the split layers, once for both families.  L = the stage's layout, sm = the
// base of its dynamic LDS; rows [v0, v0 + R) of V.  Every workgroup that calls a section computes all of it into LDS; `wr` says
// whether this workgroup also writes the results to HBM (chain.hip: always; chain_cluster.hip: member 0).  All 512 threads call.
// The summation orders are fixed (bitwise reproducible steps): do not reorder a sum here.
// ------------------------------------------------------------------------------------------------------------------

// A pointer of the kernel's argument block as an opaque scalar value.  A select between two pointers that were both loaded from the
// argument block the compiler turns into ONE load through a selected address: with a per-thread condition that is a vector load,
// a dependent round trip in front of the load the pointer is for.  Through arg_value the select stays a select of values.
template <class T>
__device__ __forceinline__ const T* arg_value(const T* p) {
  asm("" : "+s"(p));
  return p;
}
// stage A forward: the 18 bias rows of the stage -> LDS.  Unit u (< FWD_A_BIAS_UNITS) is four floats: fwd_a_bias_src(a, u) -> s_bias + 4 u.
// (a chain of selects, not a table of pointers indexed by u: the table lived in scratch memory -- the 160 bytes of
//  chain_fwd_a_cl_kernel's frame -- and every bias load waited for a scratch load first)
constexpr int FWD_A_BIAS_UNITS = 18 * (D / 4);
__device__ __forceinline__ const float* fwd_a_bias_src(const sdumc_chain_args& a, int u) {
  const float* t[18] = {arg_value(a.umlp0_b[0]), arg_value(a.umlp0_b[1]), arg_value(a.umlp0_b[2]), arg_value(a.umlp3_b[0]),
                        arg_value(a.umlp3_b[1]), arg_value(a.umlp3_b[2]), arg_value(a.att0_b), arg_value(a.att3_b),
                        arg_value(a.query_b[0]), arg_value(a.query_b[1]), arg_value(a.query_b[2]), arg_value(a.query_b[3]),
                        arg_value(a.query_b[4]), arg_value(a.query_b[5]), arg_value(a.query_b[6]), arg_value(a.caq_b[0]),
                        arg_value(a.caq_b[1]), arg_value(a.caq_b[2])};
  const int row = u / (D / 4);
  const float* p = t[0];
#pragma unroll
  for (int k = 1; k < 18; ++k) p = row == k ? t[k] : p;
  return p + 4 * (u % (D / 4));
}
__device__ __forceinline__ void fwd_a_stage_bias(const sdumc_chain_args& a, float* s_bias) {
  for (int u = threadIdx.x; u < FWD_A_BIAS_UNITS; u += NTHR) st4(s_bias + 4 * u, ld4(fwd_a_bias_src(a, u)));
}

// stage A forward, fc_att (model :303): alpha[r][j] = att2[r] . W[j] + b[j]; ends with a barrier
template <class L>
__device__ __forceinline__ void fwd_a_alpha(const sdumc_chain_args& a, float* sm, int v0, int V, bool wr) {
  constexpr int R = L::R;
  const float* s_att2 = sm + L::att2;
  float* s_alpha = sm + L::alpha;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int p = wave; p < 3 * R; p += NWV) {
    const int r = p / 3, j = p - 3 * r;
    const float s = wave_sum(dot4(ld4(s_att2 + r * D + 4 * lane), ld4(a.fc_att_w + j * D + 4 * lane)));
    if (lane == 0) {
      const float al = s + a.fc_att_b[j];
      s_alpha[r * 4 + j] = al;
      if (v0 + r < V && wr) a.alpha[(int64_t)(v0 + r) * 3 + j] = al;
    }
  }
  __syncthreads();
}

// stage A forward, fusion algebra (model :305-320): the 7 query inputs fused, a+t, t+v, a+v, a, t, v.  own(c): this workgroup
// writes column c to HBM (chain_cluster.hip: the owner of the column slice).  Ends with a barrier.
// (own holds its state BY VALUE: with a lambda that captured `member` by reference the compiler contracted the shared products
//  ua * aa, ut * at, uv * av into other fmas and every clustered result changed in its last bits -- tools/chain_digest.py shows it)
template <class L, class Own>
__device__ __forceinline__ void fwd_a_fusion(const sdumc_chain_args& a, float* sm, int v0, int V, Own own) {
  constexpr int R = L::R;
  const float *s_u = sm + L::u, *s_alpha = sm + L::alpha;
  float* s_qin = sm + L::qin;
  const int64_t VD = (int64_t)V * D;
  for (int u = threadIdx.x; u < R * (D / 4); u += NTHR) {
    const int r = u / (D / 4), c = 4 * (u - r * (D / 4));
    const f32x4 ua = ld4(s_u + r * 3 * D + c), ut = ld4(s_u + r * 3 * D + D + c), uv = ld4(s_u + r * 3 * D + 2 * D + c);
    const float aa = s_alpha[r * 4], at = s_alpha[r * 4 + 1], av = s_alpha[r * 4 + 2];
    f32x4 o[7] = {ua * aa + ut * at + uv * av, ua * aa + ut * at, ut * at + uv * av, ua * aa + uv * av, ua, ut, uv};
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      st4(s_qin + (i * R + r) * D + c, o[i]);
      if (v0 + r < V && own(c)) st4(a.qin + i * VD + (int64_t)(v0 + r) * D + c, o[i]);
    }
  }
  __syncthreads();
}

// stage B forward: the bias rows of the stage -> LDS, back to back in the order of FwdBLds::bias.  Unit u (< FWD_B_BIAS_UNITS) is
// four floats: fwd_b_bias_src(a, u) -> s_bias + 4 u.
constexpr int FWD_B_BIAS_UNITS = (4 * D + 4 * H + 2 * RD) / 4;
__device__ __forceinline__ const float* fwd_b_bias_src(const sdumc_chain_args& a, int u) {
  constexpr int U0 = 3 * (D / 4), U1 = U0 + 3 * (H / 4), U2 = U1 + D / 4, U3 = U2 + H / 4, U4 = U3 + RD / 4;
  const int m0 = u / (D / 4), m1 = (u - U0) / (H / 4);
  const float *c0 = arg_value(a.cmlp0_b[0]), *c1 = arg_value(a.cmlp0_b[1]), *c2 = arg_value(a.cmlp0_b[2]), *d0 = arg_value(a.cmlp3_b[0]),
              *d1 = arg_value(a.cmlp3_b[1]), *d2 = arg_value(a.cmlp3_b[2]), *e0 = arg_value(a.catt0_b), *e3 = arg_value(a.catt3_b),
              *r0 = arg_value(a.rnc0_b), *r2 = arg_value(a.rnc2_b);
  const float* p = c0 + 4 * u;
  p = m0 == 1 ? c1 + 4 * (u - D / 4) : p;
  p = m0 == 2 ? c2 + 4 * (u - 2 * (D / 4)) : p;
  p = u >= U0 ? d0 + 4 * (u - U0) : p;
  p = (u >= U0 && m1 == 1) ? d1 + 4 * (u - U0 - H / 4) : p;
  p = (u >= U0 && m1 == 2) ? d2 + 4 * (u - U0 - 2 * (H / 4)) : p;
  p = u >= U1 ? e0 + 4 * (u - U1) : p;
  p = u >= U2 ? e3 + 4 * (u - U2) : p;
  p = u >= U3 ? r0 + 4 * (u - U3) : p;
  p = u >= U4 ? r2 + 4 * (u - U4) : p;
  return p;
}
__device__ __forceinline__ void fwd_b_stage_bias(const sdumc_chain_args& a, float* s_bias) {
  for (int u = threadIdx.x; u < FWD_B_BIAS_UNITS; u += NTHR) st4(s_bias + 4 * u, ld4(fwd_b_bias_src(a, u)));
}

// alpha (or d_alpha) of rows [v0, v0 + R) -> LDS [R][4], in request / store halves as rows_request / rows_store: thread u < 3 R
// holds alpha[r][j], u = 3 r + j
template <int R>
__device__ __forceinline__ float alpha_request(const float* alpha, int v0, int V) {
  static_assert(R * 3 <= NTHR, "one element per thread");
  const int u = min((int)threadIdx.x, R * 3 - 1), r = u / 3, j = u - 3 * r;
  return alpha[(int64_t)min(v0 + r, V - 1) * 3 + j];
}
template <int R>
__device__ __forceinline__ void alpha_store(float al, float* s_alpha, int v0, int V) {
  const int u = threadIdx.x, r = u / 3, j = u - 3 * r;
  if (u < R * 3) s_alpha[r * 4 + j] = v0 + r < V ? al : 0.f;
}
// stage B forward: alpha of rows [v0, v0 + R) -> LDS [R][4]
template <class L>
__device__ __forceinline__ void fwd_b_load_alpha(const sdumc_chain_args& a, float* sm, int v0, int V) {
  alpha_store<L::R>(alpha_request<L::R>(a.alpha, v0, V), sm + L::alpha, v0, V);
}

// stage B forward, modality-weighted sum (model :346-349): h[r][i][:] = sum_m alpha[r][m] c_m[r][i][:]; ends with a barrier
template <class L>
__device__ __forceinline__ void fwd_b_hsum(const sdumc_chain_args& a, float* sm, int v0, int V, bool wr) {
  constexpr int R = L::R;
  const float *s_c = sm + L::c, *s_alpha = sm + L::alpha;
  float* s_h = sm + L::h;
  for (int u = threadIdx.x; u < R * NQ * (H / 4); u += NTHR) {
    const int ri = u / (H / 4), c = 4 * (u - ri * (H / 4)), r = ri / NQ;
    const f32x4 hv = ld4(s_c + ri * H + c) * s_alpha[r * 4] + ld4(s_c + (NQ * R + ri) * H + c) * s_alpha[r * 4 + 1] +
                     ld4(s_c + (2 * NQ * R + ri) * H + c) * s_alpha[r * 4 + 2];
    st4(s_h + ri * H + c, hv);
    if (v0 + r < V && wr) st4(a.h + ((int64_t)v0 * NQ + ri) * H + c, hv);
  }
  __syncthreads();
}

// stage B forward, the tail behind cross_attention_mlp (model :354-368): beta = cross_fc_att(e2), cross_fused_feat, fc_out_v, both
// orgin_linear_change layers.  At most 128 columns wide: one workgroup computes and writes all of it (e2 and h are in LDS).
template <class L>
__device__ __forceinline__ void fwd_b_tail(const sdumc_chain_args& a, float* sm, int v0, int V) {
  constexpr int R = L::R;
  float* part = sm + L::part;
  const float *s_e2 = sm + L::e2, *s_h = sm + L::h, *s_bias = sm + L::bias;
  float *s_z = sm + L::z, *s_r1 = sm + L::r1, *s_beta = sm + L::beta;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int p = wave; p < NQ * R; p += NWV) {          // beta[r][i] = e2[r] . W[i] + b[i]
    const int r = p / NQ, i = p - NQ * r;
    float s = lane < H / 4 ? dot4(ld4(s_e2 + r * H + 4 * lane), ld4(a.cfa_w + i * H + 4 * lane)) : 0.f;
    s = wave_sum(s);
    if (lane == 0) {
      const float bt = s + a.cfa_b[i];
      s_beta[r * 8 + i] = bt;
      if (v0 + r < V) a.beta[(int64_t)(v0 + r) * NQ + i] = bt;
    }
  }
  __syncthreads();
  // cross_fused_feat (model :356-358), fc_out_v (model :364)
  for (int u = tid; u < R * (H / 4); u += NTHR) {
    const int r = u / (H / 4), c = 4 * (u - r * (H / 4));
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NQ; ++i) acc += ld4(s_h + (r * NQ + i) * H + c) * s_beta[r * 8 + i];
    st4(s_z + r * H + c, acc);
    if (v0 + r < V) {
      st4(a.z + (int64_t)(v0 + r) * H + c, acc);
      if (a.o_fused) st4(a.o_fused + (int64_t)(v0 + r) * H + c, acc);
    }
  }
  __syncthreads();
  for (int r = wave; r < R; r += NWV) {
    float s = lane < H / 4 ? dot4(ld4(s_z + r * H + 4 * lane), ld4(a.fcv_w + 4 * lane)) : 0.f;
    s = wave_sum(s);
    if (lane == 0 && v0 + r < V) {
      const float y = s + a.fcv_b[0];
      a.vals[v0 + r] = y;
      if (a.o_vals) a.o_vals[v0 + r] = y;
    }
  }
  // orgin_linear_change (model :246-250, :368): Linear -> ReLU -> Linear
  {
    FwdEpi e{s_bias + 4 * D + 4 * H, s_r1, RD, a.r1 + (int64_t)v0 * RD, RD, true, DropRT{}, 0u, 0u};
    auto epi = [&](int r, int col, f32x4 v) { if (v0 + r < V) e(r, col, v); else st4(s_r1 + r * RD + col, f32x4{0.f, 0.f, 0.f, 0.f}); };
    rows_x_matrix<R, H, RD>(s_z, H, a.rnc0_w, RD, part, epi);
  }
  {
    FwdEpi e{s_bias + 4 * D + 4 * H + RD, nullptr, 0, a.r + (int64_t)v0 * RD, RD, false, DropRT{}, 0u, 0u};
    float* ro = a.o_rnc ? a.o_rnc + (int64_t)v0 * RD : nullptr;
    const float* b2 = s_bias + 4 * D + 4 * H + RD;
    auto epi = [&](int r, int col, f32x4 v) {
      if (v0 + r < V) {
        e(r, col, v);
        if (ro) st4(ro + (int64_t)r * RD + col, v + ld4(b2 + col));
      }
    };
    rows_x_matrix<R, RD, RD>(s_r1, RD, a.rnc2_w, RD, part, epi);
  }
}

// stage B backward, head loads: d_rnc, saved r1 / h / e2 / e1, beta, alpha, d_vals (rows beyond V zero).  No barrier.
// In two halves (rows_request / rows_store): all of it is requested before any of it is waited for.
template <int R>
struct BwdBHead {
  RowsReg<R, RD> g, r1;
  RowsReg<R, NQ * H> h;
  RowsReg<R, H> e2;
  RowsReg<R, D> e1;
  float beta, alpha, dval;      // thread u < 8 R: u = 8 r + i
};
template <class L>
__device__ __forceinline__ void bwd_b_head_request(BwdBHead<L::R>& hd, const sdumc_chain_args& a, int v0, int V) {
  constexpr int R = L::R;
  static_assert(R * 8 <= NTHR, "one element per thread");
  rows_request(hd.g, a.g_rnc ? a.g_rnc : a.r1, RD, v0, V);      // (no d_rnc: any live rows, zeroed at the store)
  rows_request(hd.r1, a.r1, RD, v0, V);
  rows_request(hd.h, a.h, NQ * H, v0, V);
  rows_request(hd.e2, a.e2, H, v0, V);
  rows_request(hd.e1, a.e1, D, v0, V);
  const int u = min((int)threadIdx.x, R * 8 - 1), i = u & 7;
  const int64_t v = min(v0 + (u >> 3), V - 1);
  hd.beta = a.beta[v * NQ + min(i, NQ - 1)];
  hd.alpha = a.alpha[v * 3 + min(i, 2)];
  hd.dval = (a.g_vals ? a.g_vals : a.beta)[v];
}
template <class L>
__device__ __forceinline__ void bwd_b_head_store(const BwdBHead<L::R>& hd, const sdumc_chain_args& a, float* sm, int v0, int V) {
  constexpr int R = L::R;
  float *s_beta = sm + L::beta, *s_alpha = sm + L::alpha, *s_dvals = sm + L::dvals;
  rows_store(hd.g, sm + L::g, v0, V, a.g_rnc == nullptr);
  rows_store(hd.r1, sm + L::r1, v0, V);
  rows_store(hd.h, sm + L::h, v0, V);
  rows_store(hd.e2, sm + L::e2, v0, V);
  rows_store(hd.e1, sm + L::e1, v0, V);
  const int u = threadIdx.x, r = u >> 3, i = u & 7;
  if (u < R * 8) {
    s_beta[u] = (i < NQ && v0 + r < V) ? hd.beta : 0.f;
    if (i < 3) s_alpha[r * 4 + i] = v0 + r < V ? hd.alpha : 0.f;
    if (i == 0) s_dvals[r] = (a.g_vals && v0 + r < V) ? hd.dval : 0.f;
  }
}
template <class L>
__device__ __forceinline__ void bwd_b_load_head(const sdumc_chain_args& a, float* sm, int v0, int V) {
  BwdBHead<L::R> hd;
  bwd_b_head_request<L>(hd, a, v0, V);
  bwd_b_head_store<L>(hd, a, sm, v0, V);
}

// stage B backward, 12'. orgin_linear_change: d_r1 = (d_rnc W2) [r1 > 0] ; d_z = d_r1 W0 + d_vals w_v + d_fused
template <class L>
__device__ __forceinline__ void bwd_b_rnc(const sdumc_chain_args& a, float* sm, int v0, int V, bool wr) {
  constexpr int R = L::R;
  float *part = sm + L::part, *s_r1 = sm + L::r1, *s_dz = sm + L::dz;
  const float *s_g = sm + L::g, *s_dvals = sm + L::dvals;
  {
    BwdEpi e{nullptr, 0, s_r1, RD, 1.0f, s_r1, RD, wr ? a.d_r1 + (int64_t)v0 * RD : nullptr, RD};
    auto epi = [&](int r, int col, f32x4 v) { if (v0 + r < V) e(r, col, v); else st4(s_r1 + r * RD + col, f32x4{0.f, 0.f, 0.f, 0.f}); };
    rows_x_matrix<R, RD, RD>(s_g, RD, a.rnc2_w, RD, part, epi);
  }
  {
    const float* gf = a.g_fused;
    const float* wv = a.fcv_w;
    float* dzg = a.d_z;
    auto epi = [&](int r, int col, f32x4 v) {
      v += ld4(wv + col) * s_dvals[r];
      if (gf && v0 + r < V) v += ld4(gf + (int64_t)(v0 + r) * H + col);
      if (v0 + r >= V) v = f32x4{0.f, 0.f, 0.f, 0.f};
      st4(s_dz + r * H + col, v);
      if (v0 + r < V && wr) st4(dzg + (int64_t)(v0 + r) * H + col, v);
    };
    rows_x_matrix<R, RD, H>(s_r1, RD, a.rnc0_w, H, part, epi);
  }
}

// stage B backward, zpool: d_h[i] = beta_i d_z ; d_beta_i = <d_z, h_i>; ends with a barrier
template <class L>
__device__ __forceinline__ void bwd_b_zpool(const sdumc_chain_args& a, float* sm, int v0, int V, bool wr) {
  constexpr int R = L::R;
  const float *s_dz = sm + L::dz, *s_h = sm + L::h, *s_beta = sm + L::beta;
  float *s_dh = sm + L::dh, *s_dbeta = sm + L::dbeta;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int u = tid; u < R * NQ * (H / 4); u += NTHR) {
    const int ri = u / (H / 4), c = 4 * (u - ri * (H / 4)), r = ri / NQ, i = ri - r * NQ;
    st4(s_dh + ri * H + c, ld4(s_dz + r * H + c) * s_beta[r * 8 + i]);
  }
  for (int p = wave; p < NQ * R; p += NWV) {
    const int r = p / NQ, i = p - NQ * r;
    float s = lane < H / 4 ? dot4(ld4(s_dz + r * H + 4 * lane), ld4(s_h + (r * NQ + i) * H + 4 * lane)) : 0.f;
    s = wave_sum(s);
    if (lane == 0) {
      s_dbeta[r * 8 + i] = s;
      if (v0 + r < V && wr) a.d_beta[(int64_t)(v0 + r) * NQ + i] = s;
    }
  }
  __syncthreads();
}

// stage B backward, 11'. cross_fc_att: d_e2 = (d_beta W_cfa) [e2 > 0] s, into the LDS slot of d_z (dead by now); ends with a barrier
template <class L>
__device__ __forceinline__ void bwd_b_de2(const sdumc_chain_args& a, float* sm, int v0, int V, float sc, bool wr) {
  constexpr int R = L::R;
  const float *s_e2 = sm + L::e2, *s_dbeta = sm + L::dbeta;
  float* s_dz = sm + L::dz;
  for (int u = threadIdx.x; u < R * (H / 4); u += NTHR) {
    const int r = u / (H / 4), c = 4 * (u - r * (H / 4));
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NQ; ++i) g += ld4(a.cfa_w + i * H + c) * s_dbeta[r * 8 + i];
    g = mask_val(g, ld4(s_e2 + r * H + c), sc);
    if (v0 + r < V && wr) st4(a.d_e2 + (int64_t)(v0 + r) * H + c, g);
    st4(s_dz + r * H + c, g);
  }
  __syncthreads();
}

// stage B backward, 10'. modality-weighted sum backward of modality m: d_c_m = (alpha_m d_h (+ d_cross_text on m = 1)) [c_m > 0] s
// -> s_dcm [7R][128]; d_alpha_m = <d_h, c_m> (per-quad partials through `part`, summed per sample in a fixed order).  One barrier
// inside, none at the end.
template <class L>
__device__ __forceinline__ void bwd_b_dc(const sdumc_chain_args& a, float* sm, float* s_dcm, int m, int v0, int V, float sc, bool wr) {
  constexpr int R = L::R;
  float* part = sm + L::part;
  const float *s_dh = sm + L::dh, *s_alpha = sm + L::alpha;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t VQ = (int64_t)V * NQ;
  for (int u = tid; u < R * NQ * (H / 4); u += NTHR) {
    const int ri = u / (H / 4), c = 4 * (u - ri * (H / 4)), r = ri / NQ;
    const bool live = v0 + r < V;
    f32x4 cm = {0.f, 0.f, 0.f, 0.f}, g = ld4(s_dh + ri * H + c);
    if (live) cm = ld4(a.c + ((int64_t)m * VQ + (int64_t)v0 * NQ + ri) * H + c);
    part[u] = dot4(g, cm);
    g = g * s_alpha[r * 4 + m];
    if (m == 1 && a.g_cross_text && live) g += ld4(a.g_cross_text + ((int64_t)v0 * NQ + ri) * H + c);
    g = mask_val(g, cm, sc);
    st4(s_dcm + ri * H + c, g);
    if (live && wr) st4(a.d_c + ((int64_t)m * VQ + (int64_t)v0 * NQ + ri) * H + c, g);
  }
  __syncthreads();
  for (int r = wave; r < R; r += NWV) {
    float s = 0.f;
    for (int k = lane; k < NQ * (H / 4); k += 64) s += part[r * NQ * (H / 4) + k];
    s = wave_sum(s);
    if (lane == 0 && v0 + r < V && wr) a.d_alpha[(int64_t)(v0 + r) * 3 + m] = s;
  }
}

// stage A backward: alpha and stage B's d_alpha of rows [v0, v0 + R) -> LDS [R][4] each
template <class L>
__device__ __forceinline__ void bwd_a_load_alpha(const sdumc_chain_args& a, float* sm, int v0, int V) {
  const float al = alpha_request<L::R>(a.alpha, v0, V), dal = alpha_request<L::R>(a.d_alpha, v0, V);
  alpha_store<L::R>(al, sm + L::alpha, v0, V);
  alpha_store<L::R>(dal, sm + L::dalpha, v0, V);
}

// stage A backward, 6'. + the external gradient of text_hidden (= query 5), ReLU/dropout mask of q -> d_q (pre-activation), for
// columns [c0, c0 + W) of every (sample, query) row.  out(g, lds, hbm, live): where the value goes -- its slot in s_dq and in d_q.
template <class L, int W, class Out>
__device__ __forceinline__ void bwd_a_mask_q(const sdumc_chain_args& a, float* sm, int v0, int V, float sc, int c0, Out out) {
  constexpr int R = L::R;
  float* s_dq = sm + L::dq;
  for (int u = threadIdx.x; u < R * NQ * (W / 4); u += NTHR) {
    const int ri = u / (W / 4), c = c0 + 4 * (u - ri * (W / 4)), r = ri / NQ, i = ri - r * NQ;
    f32x4 g = ld4(s_dq + ri * D + c);
    const bool live = v0 + r < V;
    if (i == 5 && a.g_text_hidden && live) g += ld4(a.g_text_hidden + (int64_t)(v0 + r) * D + c);
    f32x4 y = {0.f, 0.f, 0.f, 0.f};
    if (live) y = ld4(a.q + ((int64_t)(v0 + r) * NQ + i) * D + c);
    g = mask_val(g, y, sc);
    out(g, s_dq + ri * D + c, a.d_q + ((int64_t)(v0 + r) * NQ + i) * D + c, live);
  }
}

// stage A backward, 5'. fusion algebra backward: d_u (fusion part), d_alpha += <g_m, u_m> (partials through `part`, fixed order);
// the final d_alpha is what the fc_att dW GEMM reads.  Ends with a barrier.
template <class L>
__device__ __forceinline__ void bwd_a_fusion(const sdumc_chain_args& a, float* sm, int v0, int V, bool wr) {
  constexpr int R = L::R;
  float *part = sm + L::part, *s_du = sm + L::du, *s_dalpha = sm + L::dalpha;
  const float *s_dqin = sm + L::dqin, *s_u = sm + L::u, *s_alpha = sm + L::alpha;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int u = tid; u < R * (D / 4); u += NTHR) {
    const int r = u / (D / 4), c = 4 * (u - r * (D / 4));
    const f32x4 df = ld4(s_dqin + (0 * R + r) * D + c), dfat = ld4(s_dqin + (1 * R + r) * D + c),
                dftv = ld4(s_dqin + (2 * R + r) * D + c), dfav = ld4(s_dqin + (3 * R + r) * D + c);
    const f32x4 ga = df + dfat + dfav, gt = df + dfat + dftv, gv = df + dftv + dfav;
    const float aa = s_alpha[r * 4], at = s_alpha[r * 4 + 1], av = s_alpha[r * 4 + 2];
    st4(s_du + r * 3 * D + c, ga * aa + ld4(s_dqin + (4 * R + r) * D + c));
    st4(s_du + r * 3 * D + D + c, gt * at + ld4(s_dqin + (5 * R + r) * D + c));
    st4(s_du + r * 3 * D + 2 * D + c, gv * av + ld4(s_dqin + (6 * R + r) * D + c));
    part[(r * 3 + 0) * (D / 4) + (c >> 2)] = dot4(ga, ld4(s_u + r * 3 * D + c));
    part[(r * 3 + 1) * (D / 4) + (c >> 2)] = dot4(gt, ld4(s_u + r * 3 * D + D + c));
    part[(r * 3 + 2) * (D / 4) + (c >> 2)] = dot4(gv, ld4(s_u + r * 3 * D + 2 * D + c));
  }
  __syncthreads();
  for (int p = wave; p < 3 * R; p += NWV) {
    const float s = wave_sum(part[p * (D / 4) + lane]);
    if (lane == 0) {
      const int r = p / 3, j = p - 3 * r;
      const float da = s_dalpha[r * 4 + j] + s;
      s_dalpha[r * 4 + j] = da;
      if (v0 + r < V && wr) a.d_alpha[(int64_t)(v0 + r) * 3 + j] = da;
    }
  }
  __syncthreads();
}

// stage A backward, 4'. fc_att: d_att2 = (d_alpha W_fc) [att2 > 0] s, over the saved att2 in LDS; ends with a barrier
template <class L>
__device__ __forceinline__ void bwd_a_datt2(const sdumc_chain_args& a, float* sm, int v0, int V, float sc, bool wr) {
  constexpr int R = L::R;
  float* s_a2 = sm + L::a2;
  const float* s_dalpha = sm + L::dalpha;
  for (int u = threadIdx.x; u < R * (D / 4); u += NTHR) {
    const int r = u / (D / 4), c = 4 * (u - r * (D / 4));
    f32x4 g = ld4(a.fc_att_w + c) * s_dalpha[r * 4] + ld4(a.fc_att_w + D + c) * s_dalpha[r * 4 + 1] +
              ld4(a.fc_att_w + 2 * D + c) * s_dalpha[r * 4 + 2];
    g = mask_val(g, ld4(s_a2 + r * D + c), sc);
    st4(s_a2 + r * D + c, g);
    if (v0 + r < V && wr) st4(a.d_att2 + (int64_t)(v0 + r) * D + c, g);
  }
  __syncthreads();
}

}  // namespace
