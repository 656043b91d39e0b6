// chain_cluster.hip — the four utterance-level stages of chain.hip with every layer's OUTPUT COLUMNS split over a cluster of
// four workgroups.
//
// Why: in chain.hip one workgroup owns R samples and streams every weight matrix of a stage through one CU; the stage then
// takes (bytes of weights) / (what one CU pulls out of L2, ~100 GB/s measured) whatever R is -- 104 / 69 / 66 / 100 us at C2
// with 64 of the 256 CUs busy, a fifth of the 2.0 ms step and the part of it during which the chip idles.  Here the R samples
// belong to a cluster of CL = 4 workgroups on 4 CUs; member j computes columns [64 j, 64 j + 64) of every 256-wide layer
// (32-column slices of the 128-wide ones, 64-column blocks j, j + 4, .. of the 768- and 896-wide backward products), so each
// CU streams a quarter of the weights and does a quarter of the FMAs.  After a layer (or a group of independent layers) the
// members swap their slices:
//
//   * the slices go to the activation / gradient tensors in HBM that the stage writes anyway (the backward and the dW GEMMs read
//     them), with agent-scope (sc1, write-through) stores;
//   * s_waitcnt vmcnt(0), workgroup barrier, one agent-scope atomic add on the cluster's arrival counter, spin until it reads
//     CL x (exchanges so far), barrier;
//   * every member reloads the full rows into LDS with agent-scope loads.
//
// tools/probes/cluster_sync_probe.hip measured that hand-shake on MI355X: 1.3 us per exchange when the members share an XCD
// (blockIdx = cluster + member * nclusters, equal modulo 8 whenever nclusters % 8 == 0), 1.6 us across XCDs, 0 stale elements
// in 1.3e8 checked reads with and without a bandwidth-heavy kernel on another stream.  17 exchanges per step.
//
// Co-residency: members spin on each other, so all nclusters x CL workgroups must be resident at once: the launch refuses
// shapes with more workgroups than CUs (V <= 128 on MI355X; sdumc_chain_cluster_ok_), and cluster launches of different
// streams of one device are serialised with an event (two half-resident cluster kernels would deadlock each other).  A spin
// that exceeds its cap sets an error word and lets the kernel run to its end (wrong results, no hang).
// fp32 weights only (a 64-column slice of a bf16 row is half a cache line per lane group; the stream is no longer the bound).
#include <atomic>
#include <mutex>

#include "chain_common.h"

namespace {

constexpr int CL = 4;             // workgroups per cluster
constexpr int OC = D / CL;        // column slice of a 256-wide layer
constexpr int HC = H / CL;        // column slice of a 128-wide layer
constexpr int PARTC = NWV * 7 * OC;   // partial-sum area of the split layers (also covers the un-split 2 x 128 tail layers)
constexpr int SPIN_CAP = 400000;
static_assert(PARTC >= NWV * 2 * H, "tail layers");

// the stages' LDS layouts here: the slice-wide partial-sum area, the three modalities side by side
template <int R> using FwdA = FwdALds<R, PARTC>;
template <int R> using FwdB = FwdBLds<R, PARTC, 3, 0>;
template <int R> using BwdB = BwdBLds<R, PARTC, 3>;
template <int R> using BwdA = BwdALds<R, PARTC, 3>;

struct Cl {
  uint32_t* arrive;
  uint32_t* depart;
  int32_t* err;
  uint32_t round;
  bool hold;        // test hook (sdumc_chain_cluster_test_hold_): this workgroup withholds its arrivals, so its cluster runs into the cap
  uint32_t mode;    // sdumc_chain_args.cl_mode
};

// rows [row0, row0 + ROWS) of a global [.., width] tensor (written by the cluster's members in this launch) -> LDS
template <int ROWS>
__device__ __forceinline__ void reload_rows(float* dst_lds, int ld_dst, const float* src, int64_t ld_src, int width, int row0, int nrows) {
  const int q = width >> 2;
  for (int u = threadIdx.x; u < ROWS * q; u += NTHR) {
    const int r = u / q, c = u - r * q;
    st4(dst_lds + r * ld_dst + 4 * c, row0 + r < nrows ? ld4_dev(src + (int64_t)(row0 + r) * ld_src + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f});
  }
}

// every member's stores of the phase are complete and every member has arrived; ends with a workgroup barrier
__device__ __forceinline__ void cl_sync(Cl& cl, int* s_bail) {
  if (cl.mode & 1u) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0 && !*s_bail) {
    if (!cl.hold) {
      if (cl.mode & 1u) __hip_atomic_fetch_add(cl.arrive, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      else __hip_atomic_fetch_add(cl.arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint32_t want = (uint32_t)CL * (cl.round + 1u);
    int spins = 0;
    while (__hip_atomic_load(cl.arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
      if (++spins > SPIN_CAP) {
        *s_bail = 1;
        __hip_atomic_store(cl.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  ++cl.round;
  __syncthreads();
  if (cl.mode & 1u) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}
// after a member's last cl_sync: the last one to leave zeroes the counters for the next launch
__device__ __forceinline__ void cl_exit(Cl& cl) {
  if (threadIdx.x == 0) {
    const uint32_t n = __hip_atomic_fetch_add(cl.depart, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n == (uint32_t)CL - 1u) {
      __hip_atomic_store(cl.arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(cl.depart, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// rows x matrix-slice for the clustered kernels.  Same contract as rxm_run (chain_common.h) for O = 32 or 64 fp32 columns,
// re-cut for what bounds a SLICE: not the weight stream (16-64 KB per layer and member) but the chain of latencies per layer
// (measured 1.5 us for a 2-row layer, 6 us for a 14-row one with rxm_run: half of each wave's weight rows were loaded inside
// the k-loop with their L2 / Infinity-Cache latency exposed, and every row added shuffles and reduction rounds):
//   * the 8 waves form RS = 2 groups; a group owns half of the rows and splits K over its 4 waves, so each wave walks
//     twice as many weight rows (4 iterations at I = 256) and the register ring runs 4 deep: 3 iterations are issued by the
//     previous layer's hook, the 4th under the first FMAs;
//   * 7 (or 1) rows per wave instead of 14 (2): half the shuffles, ONE reduction round instead of two.
// ------------------------------------------------------------------------------------------------------------------
// RSv = 1: the 8 waves split K (2-row layers).  RSv = 2 (14-row layers): two groups of 4 waves, each owns 7 rows and splits K
// 4 ways -- half the shuffles per wave and ONE reduction round, at the price of both groups streaming the slice.
// The ring holds 4 iterations: a layer of <= 4 iterations per wave (every 256-deep one) is loaded WHOLE by the prefetch, which
// the previous layer issues from its hook, so that a k-loop starts on data that has been in flight during the previous
// layer's reduction, epilogue and barriers; longer layers (768 / 896 deep) refill a slot as soon as it has been consumed.
template <int I, int O, int RSv>
struct CGeom {
  static constexpr int OG = O / 4;                 // lane groups across the slice's columns (8 or 16)
  static constexpr int S = 64 / OG;                // rows of M covered by one wave-load (8 or 4)
  static constexpr int MW = NWV / RSv;             // waves that split K
  static constexpr int UNITS = I / (4 * S);
  static constexpr int WAVES = UNITS >= MW ? MW : UNITS;
  static constexpr int IW = I / WAVES;
  static constexpr int ITER = IW / (4 * S);
  static constexpr int PRE = ITER >= 4 ? 4 : ITER;   // iterations issued by the prefetch
  static_assert(O == 32 || O == 64, "slice width");
  static_assert(I % (4 * S * WAVES) == 0 && ITER >= 1, "k range must split evenly");
};
// (every index into the ring is a compile-time constant in the SOURCE -- static_for, not an unrolled loop variable: with loop
//  indices hipcc (ROCm 7.2) kept the 16-register ring in scratch memory as soon as a hook prefetched more than two slots)
struct CRing {
  uint4 w[16];      // [slot][e]
};
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (N > 0) {
    static_for<N - 1>(f);
    f(std::integral_constant<int, N - 1>{});
  }
}

template <int I, int O, int RSv, int SLOT>
__device__ __forceinline__ void cxm_load(CRing& ring, const float* mp, int j, int ldm) {
  using G = CGeom<I, O, RSv>;
  static_for<4>([&](auto ec) {
    constexpr int e = decltype(ec)::value;
    ring.w[SLOT * 4 + e] = *reinterpret_cast<const uint4*>(mp + (size_t)(j * 4 * G::S + e) * ldm);
  });
}

template <int I, int O, int RSv>
__device__ __forceinline__ void cxm_prefetch(CRing& ring, const float* __restrict__ M, int ldm) {
  using G = CGeom<I, O, RSv>;
  const int lane = threadIdx.x & 63, wg = (threadIdx.x >> 6) % G::MW;
  if (wg < G::WAVES) {
    const int sq = lane / G::OG, cg = lane % G::OG;
    const float* mp = M + (size_t)(wg * G::IW + 4 * sq) * ldm + 4 * cg;
    static_for<G::PRE>([&](auto dc) { cxm_load<I, O, RSv, decltype(dc)::value>(ring, mp, decltype(dc)::value, ldm); });
    // every prefetch writes all 16 registers: a hook that picks between two layer shapes (`if (m < 2) PF(..) else PF14(..)`)
    // otherwise ends in stores to DIFFERENT ring slots, SimplifyCFG sinks them into one store through a phi of two addresses,
    // and the ring can no longer leave scratch memory (measured: every layer then took ~8 us instead of ~2)
    static_for<16 - 4 * G::PRE>([&](auto kc) { ring.w[4 * G::PRE + decltype(kc)::value] = uint4{0u, 0u, 0u, 0u}; });
  }
}

// diagnosis (cl_mode bit 4): the weights the prefetch has just loaded through the caches against agent-scope (cache-bypassing)
// loads of the same addresses; a difference is recorded in dbg = {count, -, .. | records of 12 words}
template <int I, int O, int RSv>
__device__ __forceinline__ void cxm_selfcheck(const CRing& ring, const float* M, int ldm, uint32_t* dbg) {
  using G = CGeom<I, O, RSv>;
  const int lane = threadIdx.x & 63, wg = (threadIdx.x >> 6) % G::MW;
  if (wg < G::WAVES && dbg) {
    const int sq = lane / G::OG, cg = lane % G::OG;
    const float* mp = M + (size_t)(wg * G::IW + 4 * sq) * ldm + 4 * cg;
    static_for<G::PRE>([&](auto dc) {
      constexpr int sl = decltype(dc)::value;
      static_for<4>([&](auto ec) {
        constexpr int e = decltype(ec)::value;
        const uint32_t* ad = reinterpret_cast<const uint32_t*>(mp + (size_t)(sl * 4 * G::S + e) * ldm);
        const uint4 c = ring.w[sl * 4 + e];
        uint32_t b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = __hip_atomic_load(ad + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c.x != b[0] || c.y != b[1] || c.z != b[2] || c.w != b[3]) {
          const uint32_t idx = atomicAdd(dbg, 1u);
          if (idx < 20) {
            uint32_t* r = dbg + 8 + 12 * idx;
            r[0] = blockIdx.x; r[1] = threadIdx.x; r[2] = sl * 4 + e;
            r[3] = (uint32_t)(reinterpret_cast<uintptr_t>(ad) & 0xffffffffu);
            r[4] = c.x; r[5] = c.y; r[6] = c.z; r[7] = c.w; r[8] = b[0]; r[9] = b[1]; r[10] = b[2]; r[11] = b[3];
          }
        }
      });
    });
  }
}

// A forward stage's input rows from the softmax partials of the pooling sites in front of it (sdumc_chain_fold): what
// attn_fwd_combine_body (attn_pool.hip) does per sample and query -- fac_c = exp(max_c - max) / sum_c' l_c' exp(max_c' - max); pooled =
// sum_c fac_c part_c (ascending c); out = dropout(pooled); stored weights *= fac -- for this cluster's R samples of the three
// modalities.  Every member computes the rows (it needs them in LDS; the partials are L2-resident: 22 KB per cluster at the
// FRA2UTT sites of C2, 154 KB at the Cross_Attention sites); the (modality, sample) pairs are dealt round-robin to the members
// for the writes to HBM (the stage's input tensor, pooled) and for the in-place normalisation of the stored weights.
// s_rows: [3][R * NQT][256]; s_fac: scratch [3 R][FOLD_MAXCHUNK][8]; out: [3][V][NQT][256].
constexpr int FOLD_MAXCHUNK = 32;
// (round 5: every loop below requests its loads in batches of 8 before it uses the first -- as written first, one dependent
//  L2 / fabric round trip per chunk, these folds were most of their stages: 19 + 17 us of stage A forward's 77 incl. the wait for the
//  slowest member at the first exchange, 29 of stage B forward's 60, 57 of stage A backward's 120 (profiles/r4z_step_marks_fp32.txt);
//  the in-place normalisation of the stored weights is dealt to the members by ELEMENT range, not by (modality, sample) pair: the
//  member that drew audio's 375 frames kept the other three waiting at the first exchange)
// (the fold is cut into a REQUEST half and two later halves, so that a stage head asks for everything whose address it knows at
//  its first instruction -- chunk statistics, the first batch of partial rows, the stored weights, biases, alpha, the first
//  layer's weights -- before it waits for any of it; profiles/README.md, "Stage heads".  Three rules keep the requests in flight
//  together:
//   * a request is branch-free where something older is still awaited behind it: a thread without a live item re-reads a live
//     address and drops the value.  Behind a branch around a load the compiler can no longer count the loads in front of a use
//     and waits for all of them (vmcnt(0));
//   * modality tables (part, stats, nchunk, T) are read through sel3, a pair of selects: indexed by a per-thread m they are vector
//     loads from the kernel's argument block, one more dependent round trip in front of every address;
//   * each arithmetic statement exists once, as in the loops this replaces: the sums run as a two-deep pipeline over (unit, batch of 8 chunks)
//     items whose first item is requested early, not as a peeled first pass.)
template <class T>
__device__ __forceinline__ T sel3v(T t0, T t1, T t2, int m) { return m == 0 ? t0 : (m == 1 ? t1 : t2); }
// (the three VALUES are passed, not a reference to the table: a select between addresses inside the argument block made the compiler
//  keep a copy of the whole block in scratch memory -- 1336 bytes per thread, every pointer then a flat one)
#define sel3(t, m) sel3v((t)[0], (t)[1], (t)[2], m)

// A thread's share of a sum over chunks: output units u = tid, tid + NTHR, .. < NU (four columns of one row), per unit the rows of
// its nc chunks, STRIDE floats apart, in batches of 8.  desc(u, src, nc): chunk 0's address of a unit < NU (a live address also for
// a row beyond V) and its chunk count (0: row beyond V).
struct ChunkItem {
  const float* src;
  int u, c0, nc;      // unit, first chunk of the batch, chunks of the unit; nc < 0: the thread has no such item
};
template <int NU, class Desc>
__device__ __forceinline__ ChunkItem chunk_item(int u, int c0, Desc& desc) {
  ChunkItem it;
  it.u = u;
  it.c0 = c0;
  desc(min(u, NU - 1), it.src, it.nc);
  if (u >= NU) it.nc = -1;
  return it;
}
// (only the chunks that exist are requested: a 16-byte load per lane that is dropped afterwards still takes its turn in the
//  texture path, and at C2 the text and video rows have one or two chunks of the eight.  These loads ARE behind branches: what is
//  waited for with them in flight has to be complete before -- chunk_drain's rows are, its copy at the end of a round waits)
template <int STRIDE>
__device__ __forceinline__ void chunk_request(const ChunkItem& it, f32x4 (&pv)[8]) {
  static_for<8>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    if (it.c0 + j < it.nc) pv[j] = ld4(it.src + (size_t)(it.c0 + j) * STRIDE);
  });
}
// cur's rows have been requested into pa.  acc(sum, row, u, c) adds chunk c (ascending); fin(u, sum) takes a unit's finished sum.
template <int NU, int STRIDE, class Desc, class Acc, class Fin>
__device__ __forceinline__ void chunk_drain(ChunkItem cur, f32x4 (&pa)[8], Desc& desc, Acc&& acc, Fin&& fin) {
  f32x4 sum = {0.f, 0.f, 0.f, 0.f};
  while (cur.nc >= 0) {
    const bool more = cur.c0 + 8 < cur.nc;
    const ChunkItem nx = chunk_item<NU>(more ? cur.u : cur.u + NTHR, more ? cur.c0 + 8 : 0, desc);
    f32x4 pb[8];
    chunk_request<STRIDE>(nx, pb);      // the next item's rows travel under this item's arithmetic
    if (cur.c0 == 0) sum = f32x4{0.f, 0.f, 0.f, 0.f};
    static_for<8>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      if (cur.c0 + j < cur.nc) acc(sum, pa[j], cur.u, cur.c0 + j);
    });
    if (!more) fin(cur.u, sum);
    cur = nx;
    static_for<8>([&](auto jc) { pa[decltype(jc)::value] = pb[decltype(jc)::value]; });
  }
}

template <int R, int NQT>
struct FoldHead {
  static constexpr int NS = 3 * R * NQT;            // (modality, sample, query) rows: one thread each for the statistics
  static constexpr int NU = NS * (D / 4);           // units of the pooled rows
  static_assert(NS <= NTHR, "one statistics row per thread");
  float cm[8], cs[8];     // chunk maxima and sums of this thread's row (nc <= 8)
  ChunkItem it;           // the first item of the partial rows ...
  f32x4 pa[8];            // ... and its rows
};
template <int R, int NQT>
struct FoldDesc {
  const sdumc_chain_fold& f;
  int v0, V;
  __device__ __forceinline__ void operator()(int u, const float*& src, int& nc) const {
    const int row = u / (D / 4), cq = u - row * (D / 4);         // row = (m R + r) NQT + i
    const int mr = row / NQT, i = row - mr * NQT;
    const int m = mr / R, v = v0 + (mr - m * R);
    const int ncm = sel3(f.nchunk, m);
    src = sel3(f.part, m) + ((size_t)min(v, V - 1) * ncm * NQT + i) * D + 4 * cq;
    nc = v < V ? ncm : 0;
  }
};

// the request half: chunk statistics (nc <= 8) and the first batch of partial rows
template <int R, int NQT>
__device__ __forceinline__ void fold_request(FoldHead<R, NQT>& h, const sdumc_chain_fold& f, const int v0, const int V) {
  using FH = FoldHead<R, NQT>;
  const int u = min((int)threadIdx.x, FH::NS - 1);
  const int mr = u / NQT, i = u - mr * NQT;
  const int m = mr / R, v = min(v0 + (mr - m * R), V - 1);
  const int nc = sel3(f.nchunk, m);
  const float* st = sel3(f.stats, m) + (size_t)v * nc * 16 + i;
  static_for<8>([&](auto cc) {
    constexpr int c = decltype(cc)::value;
    const int k = min(c, nc - 1);
    h.cm[c] = st[k * 16];
    h.cs[c] = st[k * 16 + 8];
  });
  FoldDesc<R, NQT> desc{f, v0, V};
  h.it = chunk_item<FH::NU>(threadIdx.x, 0, desc);
  chunk_request<NQT * D>(h.it, h.pa);
}

// the second half: s_fac, the barrier that publishes it, the pooled rows
template <int R, int NQT>
__device__ __forceinline__ void fold_combine(FoldHead<R, NQT>& h, const sdumc_chain_fold& f, float* out, float* s_rows, float* s_fac, const int v0,
                                             const int V, const int member, const DropRT& dbase) {
  using FH = FoldHead<R, NQT>;
  const int tid = threadIdx.x;
  if (tid < FH::NS) {
    const int u = tid;
    const int mr = u / NQT, i = u - mr * NQT;
    const int m = mr / R, v = v0 + (mr - m * R);
    if (v < V) {
      const int nc = sel3(f.nchunk, m);
      if (nc <= 8) {      // the chunk statistics of a row in registers: 16 independent loads, requested by fold_request
        float cm[8], cs[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          cm[c] = c < nc ? h.cm[c] : -INFINITY;
          cs[c] = c < nc ? h.cs[c] : 0.f;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < 8; ++c) mx = fmaxf(mx, cm[c]);
        float l = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (c < nc) l += cs[c] * expf(cm[c] - mx);      // ascending c, as attn_fwd_combine_body
        const float inv = 1.f / l;
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (c < nc) s_fac[(mr * FOLD_MAXCHUNK + c) * 8 + i] = expf(cm[c] - mx) * inv;
      } else {
        const float* st = sel3(f.stats, m) + (size_t)v * nc * 16 + i;
        float mx = -INFINITY;
        for (int c = 0; c < nc; ++c) mx = fmaxf(mx, st[c * 16]);
        float l = 0.f;
        for (int c = 0; c < nc; ++c) l += st[c * 16 + 8] * expf(st[c * 16] - mx);
        const float inv = 1.f / l;
        for (int c = 0; c < nc; ++c) s_fac[(mr * FOLD_MAXCHUNK + c) * 8 + i] = expf(st[c * 16] - mx) * inv;
      }
    }
  }
  __syncthreads();      // (the partial rows requested by fold_request stay in flight across it)
  FoldDesc<R, NQT> desc{f, v0, V};
  chunk_drain<FH::NU, NQT * D>(
      h.it, h.pa, desc,
      [&](f32x4& sum, const f32x4 pv, int u, int c) {
        const int row = u / (D / 4), mr = row / NQT, i = row - mr * NQT;
        sum += pv * s_fac[(mr * FOLD_MAXCHUNK + c) * 8 + i];
      },
      [&](int u, const f32x4 sum) {
        const int row = u / (D / 4), cq = u - row * (D / 4);
        const int mr = row / NQT, i = row - mr * NQT;
        const int m = mr / R, v = v0 + (mr - m * R);
        f32x4 o = sum;      // (zero for a row beyond V)
        if (v < V) {
          if (dbase.enabled) {
            DropRT od = mkdrop_rt(dbase, (uint32_t)sel3(f.site, m), NQT, D);
            od.threshold = f.threshold;
            od.scale = f.scale;
            o *= drop_mask4(od, (uint32_t)(v * NQT + i), (uint32_t)cq);
          }
          if ((mr & (CL - 1)) == member) {
            st4(sel3(f.pooled, m) + ((size_t)v * NQT + i) * D + 4 * cq, sum);
            st4(out + (((size_t)m * V + v) * NQT + i) * D + 4 * cq, o);
          }
        }
        st4(s_rows + (size_t)row * D + 4 * cq, o);
      });
}

// stored weights *= fac, in place: every (modality, sample) row range is cut into CL equal parts, one per member, and a member walks
// its part in rounds of NTHR elements.  Nothing in the launch reads the weights (the pooling backward and the exports do), so the
// first KR rounds of every pair -- all of them up to T = 2048 at the FRA2UTT sites and T = 585 at the Cross_Attention sites -- are
// requested with the head's other loads (fold_norm_request), wait in registers, and are scaled and stored behind the first layer
// group (fold_norm_finish), off the path to the first layer; later rounds are loaded there.  Pair and round of a register are
// compile-time constants: the element's address and factor cost a handful of instructions.
// (The request is not issued behind the input rows, under the layers: the layer loop's waits for its weights are counted for the
//  loop's later rounds, where the weights are the youngest loads, and in its first round they would wait for anything younger too.)
// fold_norm_finish reads s_fac: before its host buffer is reused.
template <int R, int NQT>
struct FoldNorm {
  static constexpr int KR = NQT == 1 ? 1 : 2;
  float wv[3 * R * KR];      // [round][pair]
};
struct NormSlot {
  float* p;       // the element (a live one also for a dead slot)
  int fac;        // its factor's index in s_fac
  bool live;
};
template <int R, int NQT>
__device__ __forceinline__ NormSlot fold_norm_slot(const sdumc_chain_fold& f, int mr, int k, int v0, int V, int member) {
  const int m = mr / R, v = v0 + (mr - m * R);
  const int n = sel3(f.T, m) * NQT, per = (n + CL - 1) / CL;
  const int e0 = member * per, e1 = min(n, e0 + per);
  const int e = e0 + (int)threadIdx.x + k * NTHR, ec = min(e, n - 1);
  const int t = ec / NQT, i = ec - t * NQT;
  NormSlot o;
  o.p = sel3(f.attn, m) + (size_t)min(v, V - 1) * n + ec;
  o.fac = (mr * FOLD_MAXCHUNK + (t >> 6)) * 8 + i;
  o.live = v < V && e < e1;
  return o;
}
template <int R, int NQT>
__device__ __forceinline__ void fold_norm_request(FoldNorm<R, NQT>& g, const sdumc_chain_fold& f, int v0, int V, int member) {
  static_for<3 * R * FoldNorm<R, NQT>::KR>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    g.wv[s] = *fold_norm_slot<R, NQT>(f, s % (3 * R), s / (3 * R), v0, V, member).p;
  });
}
template <int R, int NQT>
__device__ __forceinline__ void fold_norm_finish(const FoldNorm<R, NQT>& g, const sdumc_chain_fold& f, const float* s_fac, int v0, int V, int member) {
#if defined(SDUMC_FOLD_DBG)
  if (SDUMC_FOLD_DBG & 1) return;
#endif
  constexpr int KR = FoldNorm<R, NQT>::KR;
  static_for<3 * R * KR>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    const NormSlot sl = fold_norm_slot<R, NQT>(f, s % (3 * R), s / (3 * R), v0, V, member);
    if (sl.live) *sl.p = g.wv[s] * s_fac[sl.fac];
  });
  const int tmax = max(f.T[0], max(f.T[1], f.T[2]));
  const int kp = ((tmax * NQT + CL - 1) / CL + NTHR - 1) / NTHR;
#pragma unroll 1
  for (int k = KR; k < kp; ++k)
#pragma unroll 1
    for (int mr = 0; mr < 3 * R; ++mr) {
      const NormSlot sl = fold_norm_slot<R, NQT>(f, mr, k, v0, V, member);
      if (sl.live) *sl.p = *sl.p * s_fac[sl.fac];
    }
}

// diagnosis (cl_mode bit 6): the LDS copy of the stage's input rows against global memory (the inputs are final before the launch)
template <int ROWS>
__device__ __forceinline__ void lds_selfcheck(const float* lds_rows, const float* src, int width, int row0, int nrows, uint32_t* dbg, int tag) {
  if (!dbg) return;
  const int q = width >> 2;
  for (int u = threadIdx.x; u < ROWS * q; u += NTHR) {
    const int r = u / q, c = u - r * q;
    if (row0 + r >= nrows) continue;
    const f32x4 l = ld4(lds_rows + r * width + 4 * c);
    const f32x4 g = ld4(src + (int64_t)(row0 + r) * width + 4 * c);
    if (__float_as_uint(l[0]) != __float_as_uint(g[0]) || __float_as_uint(l[1]) != __float_as_uint(g[1]) ||
        __float_as_uint(l[2]) != __float_as_uint(g[2]) || __float_as_uint(l[3]) != __float_as_uint(g[3])) {
      const uint32_t idx = atomicAdd(dbg, 1u);
      if (idx < 20) {
        uint32_t* rec = dbg + 8 + 12 * idx;
        rec[0] = blockIdx.x; rec[1] = threadIdx.x; rec[2] = (uint32_t)tag; rec[3] = (uint32_t)(r * width + 4 * c);
#pragma unroll
        for (int k = 0; k < 4; ++k) { rec[4 + k] = __float_as_uint(l[k]); rec[8 + k] = __float_as_uint(g[k]); }
      }
    }
  }
}

// in_lds: [ROWS][ld_in]; M: this member's column slice of a row-major [I][ldm] matrix; epi(r, col, v) with col in [0, O).
// The matching prefetch is cxm_prefetch<I, O, ROWS >= 14 ? 2 : 1> (macros PF / PF14 below).
template <int ROWS, int I, int O, class Epi, class Hook>
__device__ __forceinline__ void cxm_run(CRing& ring, const float* in_lds, int ld_in, const float* __restrict__ M, int ldm, float* part,
                                        Epi&& epi, Hook&& hook) {
  constexpr int RSv = ROWS >= 14 ? 2 : 1;
  using G = CGeom<I, O, RSv>;
  constexpr int OG = G::OG, S = G::S, MW = G::MW, WAVES = G::WAVES, IW = G::IW, ITER = G::ITER;
  constexpr int RG = ROWS / RSv;                   // rows per wave group
  static_assert(ROWS % RSv == 0 && RG <= 7, "rows per group");
  static_assert(RSv * WAVES * RG * O <= PARTC, "partial-sum area too small");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = wave / MW, wg = wave % MW;
  const int sq = lane / OG, cg = lane % OG;
  f32x4 acc[RG];
#pragma unroll
  for (int r = 0; r < RG; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (wg < WAVES) {
    const int i0 = wg * IW + 4 * sq;
    const float* mp = M + (size_t)i0 * ldm + 4 * cg;
    const float* xin = in_lds + grp * RG * ld_in + i0;
    static_for<ITER>([&](auto jc) {
      constexpr int j = decltype(jc)::value, sl = (j % 4) * 4;
#pragma unroll
      for (int r = 0; r < RG; ++r) {
        const f32x4 x = ld4(xin + r * ld_in + j * 4 * S);
        static_for<4>([&](auto ec) {
          constexpr int e = decltype(ec)::value;
          const uint4 u = ring.w[sl + e];
          acc[r] += f32x4{__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w)} * x[e];
        });
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (j + 4 < ITER) cxm_load<I, O, RSv, j % 4>(ring, mp, j + 4, ldm);
    });
#pragma unroll
    for (int r = 0; r < RG; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc[r][c] += __shfl_xor(acc[r][c], 32, 64);
        acc[r][c] += __shfl_xor(acc[r][c], 16, 64);
        if constexpr (S == 8) acc[r][c] += __shfl_xor(acc[r][c], 8, 64);
      }
  }
  hook();        // the next layer's weight rows start moving here
  if (wg < WAVES && sq == 0) {
#pragma unroll
    for (int r = 0; r < RG; ++r) st4(part + ((grp * WAVES + wg) * RG + r) * O + 4 * cg, acc[r]);
  }
  __syncthreads();
  for (int u = tid; u < ROWS * (O / 4); u += NTHR) {
    const int r = u / (O / 4), cq = u - r * (O / 4);          // r = grp * RG + row within the group
    const int g = r / RG, rr = r - g * RG;
    f32x4 v = ld4(part + ((g * WAVES) * RG + rr) * O + 4 * cq);
#pragma unroll
    for (int ww = 1; ww < WAVES; ++ww) v += ld4(part + ((g * WAVES + ww) * RG + rr) * O + 4 * cq);
    epi(r, 4 * cq, v);
  }
  __syncthreads();
}

// optional phase trace (sdumc_chain_cluster_trace_): workgroup 0 stamps the 100 MHz wall clock at every phase boundary
#define TR(k) do { if (a.cl_trace && blockIdx.x == 0 && threadIdx.x == 0) a.cl_trace[k] = wall_clock64(); } while (0)

#define CL_PROLOGUE()                                                                                          \
  __shared__ int s_bail;                                                                                       \
  const int cluster = blockIdx.x % ncl, member = blockIdx.x / ncl;                                             \
  const int V = a.V, v0 = cluster * R, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;                    \
  const int coff = member * OC;                                                                                \
  Cl cl{a.cl_flags + cluster * 64, a.cl_flags + cluster * 64 + 32, a.cl_err, 0u, a.cl_test_hold == 1 && blockIdx.x == 0, (uint32_t)a.cl_mode};                              \
  if (tid == 0) s_bail = 0;                                                                                    \
  (void)lane; (void)wave

typedef float WT;   // weights stream as fp32
#define PF(I_, O_, ptr, ldm) cxm_prefetch<I_, O_, 1>(ring, ptr, ldm)       /* the next layer has 2 rows */
#define PF14(I_, O_, ptr, ldm) cxm_prefetch<I_, O_, 2>(ring, ptr, ldm)     /* the next layer has 14 rows */

// ------------------------------------------------------------------------------------------------------------------
// stage A forward (model :293-332 + :85); 5 exchanges: u1, u, att1, att2, q
// ------------------------------------------------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ void chain_fwd_a_cl_body(const sdumc_chain_args a, const int ncl) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  using L = FwdA<R>;
  float *part = sm + L::part, *s_hpre = sm + L::hpre, *s_u1 = sm + L::u1, *s_u = sm + L::u, *s_att1 = sm + L::att1, *s_att2 = sm + L::att2,
        *s_qin = sm + L::qin, *s_q = sm + L::q, *s_bias = sm + L::bias;
  CL_PROLOGUE();
  TR(0);
  const int64_t VD = (int64_t)V * D;
  const bool fold = a.fra.part[0] != nullptr;
  // the head: every request whose address is known here goes out before the first wait -- the fold's statistics and first partial
  // rows, the biases, the first layer's weights -- and is consumed in that order
  FoldHead<R, 1> fh;
  FoldNorm<R, 1> fn;
  if (fold) {
    fold_request<R, 1>(fh, a.fra, v0, V);
    fold_norm_request<R, 1>(fn, a.fra, v0, V, member);
  }
  constexpr int NBIAS = (FWD_A_BIAS_UNITS + NTHR - 1) / NTHR;
  f32x4 bias[NBIAS];
  static_for<NBIAS>([&](auto kc) { bias[decltype(kc)::value] = ld4(fwd_a_bias_src(a, min(tid + decltype(kc)::value * NTHR, FWD_A_BIAS_UNITS - 1))); });
  const DropRT dbase = drop_resolve(a.drop);
  CRing ring;
  if (a.cl_mode & 2) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (a.cl_mode & 8)
    for (int i = 0; i < 8; ++i) __builtin_amdgcn_s_sleep(127);
  PF(D, OC, a.umlp0_w[0] + coff, D);
  if (a.cl_mode & 16) cxm_selfcheck<D, OC, 1>(ring, a.umlp0_w[0] + coff, D, a.cl_dbg);
  // the FRA2UTT sites' combine (three launches, 31-39 us each inside the step, on every modality lane's way to this stage) rides here
  if (fold) fold_combine<R, 1>(fh, a.fra, a.hpre, s_hpre, s_qin, v0, V, member, dbase);      // (s_qin: free until the fusion algebra)
  else for (int m = 0; m < 3; ++m) load_rows<R>(s_hpre + m * R * D, a.hpre + m * VD, D, D, v0, V);
  static_for<NBIAS>([&](auto kc) {
    const int u = tid + decltype(kc)::value * NTHR;
    if (u < FWD_A_BIAS_UNITS) st4(s_bias + 4 * u, bias[decltype(kc)::value]);
  });
  __syncthreads();
  TR(11);
  if ((a.cl_mode & 64) && !a.fra.part[0])
    for (int m = 0; m < 3; ++m) lds_selfcheck<R>(s_hpre + m * R * D, a.hpre + m * VD, D, v0, V, a.cl_dbg, 10 + m);
  // audio / text / video_mlp (model :293-295)
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    const DropRT dr = mkdrop_rt(dbase, 6 + 2 * m, 1, D);
    float* dst = a.u1 + m * VD + (int64_t)v0 * D;
    auto epi = [&](int r, int col, f32x4 v) {
      col += coff;
      if (v0 + r < V) st4_dev(dst + (int64_t)r * D + col, fwd_val(v, s_bias + m * D, col, true, dr, (uint32_t)(v0 + r)));
    };
    cxm_run<R, D, OC>(ring, s_hpre + m * R * D, D, a.umlp0_w[m] + coff, D, part, epi,
                                [&] { PF(D, OC, (m < 2 ? a.umlp0_w[m + 1] : a.umlp3_w[0]) + coff, D); });
  }
  if (fold) fold_norm_finish<R, 1>(fn, a.fra, s_qin, v0, V, member);      // the stored weights' normalisation, requested in the head
  TR(1);
  if ((a.cl_mode & 64) && !a.fra.part[0])       // ... and again after the three layers that read it
    for (int m = 0; m < 3; ++m) lds_selfcheck<R>(s_hpre + m * R * D, a.hpre + m * VD, D, v0, V, a.cl_dbg, 20 + m);
  cl_sync(cl, &s_bail);
  TR(2);
  for (int m = 0; m < 3; ++m) reload_rows<R>(s_u1 + m * R * D, D, a.u1 + m * VD, D, D, v0, V);
  __syncthreads();
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    const DropRT dr = mkdrop_rt(dbase, 7 + 2 * m, 1, D);
    float* dst = a.u + (int64_t)v0 * 3 * D + m * D;
    auto epi = [&](int r, int col, f32x4 v) {
      col += coff;
      if (v0 + r < V) st4_dev(dst + (int64_t)r * 3 * D + col, fwd_val(v, s_bias + (3 + m) * D, col, true, dr, (uint32_t)(v0 + r)));
    };
    cxm_run<R, D, OC>(ring, s_u1 + m * R * D, D, a.umlp3_w[m] + coff, D, part, epi, [&] {
      if (m < 2) PF(D, OC, a.umlp3_w[m + 1] + coff, D);
      else PF(3 * D, OC, a.att0_w + coff, D);
    });
  }
  TR(3);
  cl_sync(cl, &s_bail);
  TR(4);
  reload_rows<R>(s_u, 3 * D, a.u, 3 * D, 3 * D, v0, V);
  __syncthreads();
  // attention_mlp + fc_att (model :301-303)
  {
    const DropRT dr = mkdrop_rt(dbase, 12, 1, D);
    float* dst = a.att1 + (int64_t)v0 * D;
    auto epi = [&](int r, int col, f32x4 v) {
      col += coff;
      if (v0 + r < V) st4_dev(dst + (int64_t)r * D + col, fwd_val(v, s_bias + 6 * D, col, true, dr, (uint32_t)(v0 + r)));
    };
    cxm_run<R, 3 * D, OC>(ring, s_u, 3 * D, a.att0_w + coff, D, part, epi, [&] { PF(D, OC, a.att3_w + coff, D); });
  }
  TR(5);
  cl_sync(cl, &s_bail);
  TR(6);
  reload_rows<R>(s_att1, D, a.att1, D, D, v0, V);
  __syncthreads();
  {
    const DropRT dr = mkdrop_rt(dbase, 13, 1, D);
    float* dst = a.att2 + (int64_t)v0 * D;
    auto epi = [&](int r, int col, f32x4 v) {
      col += coff;
      if (v0 + r < V) st4_dev(dst + (int64_t)r * D + col, fwd_val(v, s_bias + 7 * D, col, true, dr, (uint32_t)(v0 + r)));
    };
    cxm_run<R, D, OC>(ring, s_att1, D, a.att3_w + coff, D, part, epi, [&] { PF(D, OC, a.query_w[0] + coff, D); });
  }
  TR(7);
  cl_sync(cl, &s_bail);
  TR(8);
  reload_rows<R>(s_att2, D, a.att2, D, D, v0, V);
  __syncthreads();
  // alpha and the fusion algebra: every member, redundantly (HBM: alpha by member 0, qin by the owner of the column slice)
  fwd_a_alpha<L>(a, sm, v0, V, member == 0);
  fwd_a_fusion<L>(a, sm, v0, V, [member](int c) { return c / OC == member; });
  // the 7 query MLPs -> multi_query [V, 7, 256] (model :324-332); text_hidden = query 5 (model :329, :370)
#pragma unroll 1
  for (int i = 0; i < 7; ++i) {
    const DropRT dr = mkdrop_rt(dbase, 14 + i, 1, D);
    float* dst = a.q + (int64_t)v0 * NQ * D + i * D;
    float* th = (i == 5 && a.o_text_hidden) ? a.o_text_hidden + (int64_t)v0 * D : nullptr;
    auto epi = [&](int r, int col, f32x4 v) {
      col += coff;
      if (v0 + r < V) {
        const f32x4 y = fwd_val(v, s_bias + (8 + i) * D, col, true, dr, (uint32_t)(v0 + r));
        st4_dev(dst + (int64_t)r * NQ * D + col, y);
        if (th) st4(th + (int64_t)r * D + col, y);
      }
    };
    cxm_run<R, D, OC>(ring, s_qin + i * R * D, D, a.query_w[i] + coff, D, part, epi,
                                [&] { if (i < 6) PF(D, OC, a.query_w[i + 1] + coff, D); else PF14(D, OC, a.caq_w[0] + coff, D); });
  }
  TR(9);
  cl_sync(cl, &s_bail);
  TR(10);
  reload_rows<R>(s_q, NQ * D, a.q, NQ * D, NQ * D, v0, V);
  __syncthreads();
  cl_exit(cl);
  // query_proj of the three Cross_Attention blocks (model :85): rows = (sample, query)
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    float* dst = a.qp + ((int64_t)m * V + v0) * NQ * D;
    auto epi = [&](int r, int col, f32x4 v) {
      col += coff;
      if (v0 + r / NQ < V) st4(dst + (int64_t)r * D + col, v + ld4(s_bias + (15 + m) * D + col));
    };
    cxm_run<NQ * R, D, OC>(ring, s_q, D, a.caq_w[m] + coff, D, part, epi, [&] { if (m < 2) PF14(D, OC, a.caq_w[m + 1] + coff, D); });
  }
  TR(31);
}
template <int R>
__global__ __launch_bounds__(NTHR) void chain_fwd_a_cl_kernel(const sdumc_chain_args a, const int ncl) { chain_fwd_a_cl_body<R>(a, ncl); }

// ------------------------------------------------------------------------------------------------------------------
// stage B forward (model :338-368); 4 exchanges: c1, c, e1, e2.  The tail (beta, cross_fused_feat, fc_out_v,
// orgin_linear_change: 2 x <= 128 columns) is member 0's alone.
// ------------------------------------------------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ void chain_fwd_b_cl_body(const sdumc_chain_args a, const int ncl) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  using L = FwdB<R>;      // x: ca_out of the three modalities, then c1
  float *part = sm + L::part, *s_x = sm + L::x, *s_c = sm + L::c, *s_h = sm + L::h, *s_e1 = sm + L::e1, *s_e2 = sm + L::e2, *s_bias = sm + L::bias;
  CL_PROLOGUE();
  TR(0);
  const int64_t VQ = (int64_t)V * NQ;
  const int hoff = member * HC;
  const bool fold = a.ca.part[0] != nullptr;
  // the head, as stage A forward's: one batch of requests, consumed in the order they went out
  FoldHead<R, NQ> fh;
  FoldNorm<R, NQ> fn;
  if (fold) {
    fold_request<R, NQ>(fh, a.ca, v0, V);
    fold_norm_request<R, NQ>(fn, a.ca, v0, V, member);
  }
  static_assert(FWD_B_BIAS_UNITS <= NTHR, "one bias unit per thread");
  const f32x4 bias = ld4(fwd_b_bias_src(a, min(tid, FWD_B_BIAS_UNITS - 1)));
  const float al = alpha_request<R>(a.alpha, v0, V);
  const DropRT dbase = drop_resolve(a.drop);
  CRing ring;
  PF14(D, OC, a.cmlp0_w[0] + coff, D);
  // the Cross_Attention sites' combine (one grouped launch between the pooling and this stage) rides here
  if (fold) fold_combine<R, NQ>(fh, a.ca, a.ca_out, s_x, s_c, v0, V, member, dbase);      // (s_c: first written by cross_*_mlp.3)
  else for (int m = 0; m < 3; ++m) load_rows<NQ * R>(s_x + m * NQ * R * D, a.ca_out + (int64_t)m * VQ * D, D, D, v0 * NQ, V * NQ);
  if (tid < FWD_B_BIAS_UNITS) st4(s_bias + 4 * tid, bias);
  alpha_store<R>(al, sm + L::alpha, v0, V);
  __syncthreads();
  TR(11);
  // cross_{audio,text,video}_mlp (model :338-340), rows = (sample, query)
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    const DropRT dr = mkdrop_rt(dbase, 27 + 2 * m, NQ, D);
    float* dst = a.c1 + ((int64_t)m * VQ + (int64_t)v0 * NQ) * D;
    auto epi = [&](int r, int col, f32x4 v) {
      col += coff;
      if (v0 * NQ + r < V * NQ) st4_dev(dst + (int64_t)r * D + col, fwd_val(v, s_bias + m * D, col, true, dr, (uint32_t)(v0 * NQ + r)));
    };
    cxm_run<NQ * R, D, OC>(ring, s_x + m * NQ * R * D, D, a.cmlp0_w[m] + coff, D, part, epi, [&] {
      if (m < 2) PF14(D, OC, a.cmlp0_w[m + 1] + coff, D);
      else PF14(D, HC, a.cmlp3_w[0] + hoff, H);
    });
  }
  if (fold) fold_norm_finish<R, NQ>(fn, a.ca, s_c, v0, V, member);      // the stored weights' normalisation, requested in the head
  TR(1);
  cl_sync(cl, &s_bail);
  TR(2);
  for (int m = 0; m < 3; ++m) reload_rows<NQ * R>(s_x + m * NQ * R * D, D, a.c1 + (int64_t)m * VQ * D, D, D, v0 * NQ, V * NQ);
  __syncthreads();
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    const DropRT dr = mkdrop_rt(dbase, 28 + 2 * m, NQ, H);
    float* dst = a.c + ((int64_t)m * VQ + (int64_t)v0 * NQ) * H;
    float* ct = (m == 1 && a.o_cross_text) ? a.o_cross_text + (int64_t)v0 * NQ * H : nullptr;
    auto epi = [&](int r, int col, f32x4 v) {
      col += hoff;
      if (v0 * NQ + r < V * NQ) {
        const f32x4 y = fwd_val(v, s_bias + 3 * D + m * H, col, true, dr, (uint32_t)(v0 * NQ + r));
        st4_dev(dst + (int64_t)r * H + col, y);
        if (ct) st4(ct + (int64_t)r * H + col, y);
      }
    };
    cxm_run<NQ * R, D, HC>(ring, s_x + m * NQ * R * D, D, a.cmlp3_w[m] + hoff, H, part, epi, [&] {
      if (m < 2) PF14(D, HC, a.cmlp3_w[m + 1] + hoff, H);
      else PF(NQ * H, OC, a.catt0_w + coff, D);
    });
  }
  TR(3);
  cl_sync(cl, &s_bail);
  TR(4);
  for (int m = 0; m < 3; ++m) reload_rows<NQ * R>(s_c + m * NQ * R * H, H, a.c + (int64_t)m * VQ * H, H, H, v0 * NQ, V * NQ);
  __syncthreads();
  fwd_b_hsum<L>(a, sm, v0, V, member == 0);
  // cross_attention_mlp + cross_fc_att (model :352-354)
  {
    const DropRT dr = mkdrop_rt(dbase, 33, 1, D);
    float* dst = a.e1 + (int64_t)v0 * D;
    auto epi = [&](int r, int col, f32x4 v) {
      col += coff;
      if (v0 + r < V) st4_dev(dst + (int64_t)r * D + col, fwd_val(v, s_bias + 3 * D + 3 * H, col, true, dr, (uint32_t)(v0 + r)));
    };
    cxm_run<R, NQ * H, OC>(ring, s_h, NQ * H, a.catt0_w + coff, D, part, epi, [&] { PF(D, HC, a.catt3_w + hoff, H); });
  }
  TR(5);
  cl_sync(cl, &s_bail);
  TR(6);
  reload_rows<R>(s_e1, D, a.e1, D, D, v0, V);
  __syncthreads();
  {
    const DropRT dr = mkdrop_rt(dbase, 34, 1, H);
    float* dst = a.e2 + (int64_t)v0 * H;
    auto epi = [&](int r, int col, f32x4 v) {
      col += hoff;
      if (v0 + r < V) st4_dev(dst + (int64_t)r * H + col, fwd_val(v, s_bias + 4 * D + 3 * H, col, true, dr, (uint32_t)(v0 + r)));
    };
    cxm_run<R, D, HC>(ring, s_e1, D, a.catt3_w + hoff, H, part, epi, [] {});
  }
  TR(7);
  cl_sync(cl, &s_bail);
  TR(8);
  cl_exit(cl);
  if (member != 0) return;
  TR(30);
  reload_rows<R>(s_e2, H, a.e2, H, H, v0, V);
  __syncthreads();
  fwd_b_tail<L>(a, sm, v0, V);
  TR(31);
}
template <int R>
__global__ __launch_bounds__(NTHR) void chain_fwd_b_cl_kernel(const sdumc_chain_args a, const int ncl) { chain_fwd_b_cl_body<R>(a, ncl); }

// ------------------------------------------------------------------------------------------------------------------
// stage B backward; 3 exchanges: d_e1, d_h, d_c1.  The head (orgin_linear_change, zpool, cross_fc_att backward: <= 128
// columns) is computed by every member, written by member 0.
// ------------------------------------------------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ void chain_bwd_b_cl_body(const sdumc_chain_args a, const int ncl) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  using L = BwdB<R>;      // dc, c1: the three modalities side by side
  float *part = sm + L::part, *s_dz = sm + L::dz, *s_dh = sm + L::dh, *s_e1 = sm + L::e1, *s_dc = sm + L::dc, *s_c1 = sm + L::c1;
  CL_PROLOGUE();
  TR(0);
  const int64_t VQ = (int64_t)V * NQ;
  const float sc = a.relu_scale;
  const bool wr = member == 0;

  // the head: the saved activations of the whole stage as one batch of requests, one wait
  BwdBHead<R> hd;
  RowsReg<NQ * R, D> c1[3];
  bwd_b_head_request<L>(hd, a, v0, V);
  static_for<3>([&](auto mc) { rows_request(c1[decltype(mc)::value], a.c1 + (int64_t)decltype(mc)::value * VQ * D, D, v0 * NQ, V * NQ); });
  CRing ring;
  PF(H, OC, a.catt3_w + coff, D);
  bwd_b_head_store<L>(hd, a, sm, v0, V);
  static_for<3>([&](auto mc) { rows_store(c1[decltype(mc)::value], s_c1 + decltype(mc)::value * NQ * R * D, v0 * NQ, V * NQ); });
  __syncthreads();
  bwd_b_rnc<L>(a, sm, v0, V, wr);
  bwd_b_zpool<L>(a, sm, v0, V, wr);
  bwd_b_de2<L>(a, sm, v0, V, sc, wr);
  // cross_attention_mlp.3: d_e1 = (d_e2 W) [e1 > 0] s
  {
    float* dst = a.d_e1 + (int64_t)v0 * D;
    auto epi = [&](int r, int col, f32x4 v) {
      col += coff;
      if (v0 + r < V) st4_dev(dst + (int64_t)r * D + col, mask_val(v, ld4(s_e1 + r * D + col), sc));
    };
    cxm_run<R, H, OC>(ring, s_dz, H, a.catt3_w + coff, D, part, epi, [&] { PF(D, OC, a.catt0_w + member * OC, NQ * H); });
  }
  TR(1);
  cl_sync(cl, &s_bail);
  TR(2);
  reload_rows<R>(s_e1, D, a.d_e1, D, D, v0, V);
  __syncthreads();
  // .0: d_h += d_e1 W   (896 columns = 14 blocks of 64: member j takes blocks j, j + 4, ..)
#pragma unroll 1
  for (int blk = member; blk < 14; blk += CL) {
    float* dst = a.d_h + (int64_t)v0 * NQ * H;
    const int boff = blk * OC;
    auto epi = [&](int r, int col, f32x4 v) {
      col += boff;
      if (v0 + r < V) st4_dev(dst + (int64_t)r * NQ * H + col, v + ld4(s_dh + r * NQ * H + col));
    };
    cxm_run<R, D, OC>(ring, s_e1, D, a.catt0_w + boff, NQ * H, part, epi, [&] {
      if (blk + CL < 14) PF(D, OC, a.catt0_w + boff + CL * OC, NQ * H);
      else PF14(H, OC, a.cmlp3_w[0] + coff, D);
    });
  }
  TR(3);
  cl_sync(cl, &s_bail);
  TR(4);
  reload_rows<R>(s_dh, NQ * H, a.d_h, NQ * H, NQ * H, v0, V);
  __syncthreads();
  // 10'. modality-weighted sum backward (every member; HBM by member 0)
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    bwd_b_dc<L>(a, sm, s_dc + m * NQ * R * H, m, v0, V, sc, wr);
    __syncthreads();
  }
  // 9'. cross_*_mlp.3: d_c1 = (d_c W3) [c1 > 0] s
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    float* dst = a.d_c1 + ((int64_t)m * VQ + (int64_t)v0 * NQ) * D;
    const float* y = s_c1 + m * NQ * R * D;
    auto epi = [&](int r, int col, f32x4 v) {
      col += coff;
      if (v0 * NQ + r < V * NQ) st4_dev(dst + (int64_t)r * D + col, mask_val(v, ld4(y + r * D + col), sc));
    };
    cxm_run<NQ * R, H, OC>(ring, s_dc + m * NQ * R * H, H, a.cmlp3_w[m] + coff, D, part, epi, [&] {
      if (m < 2) PF14(H, OC, a.cmlp3_w[m + 1] + coff, D);
      else PF14(D, OC, a.cmlp0_w[0] + coff, D);
    });
  }
  TR(5);
  cl_sync(cl, &s_bail);
  TR(6);
  cl_exit(cl);
  for (int m = 0; m < 3; ++m) reload_rows<NQ * R>(s_c1 + m * NQ * R * D, D, a.d_c1 + (int64_t)m * VQ * D, D, D, v0 * NQ, V * NQ);
  __syncthreads();
  //     .0: d_ca_out = d_c1 W0
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    float* dst = a.d_ca_out + ((int64_t)m * VQ + (int64_t)v0 * NQ) * D;
    auto epi = [&](int r, int col, f32x4 v) {
      col += coff;
      if (v0 * NQ + r < V * NQ) st4(dst + (int64_t)r * D + col, v);
    };
    cxm_run<NQ * R, D, OC>(ring, s_c1 + m * NQ * R * D, D, a.cmlp0_w[m] + coff, D, part, epi,
                                     [&] { if (m < 2) PF14(D, OC, a.cmlp0_w[m + 1] + coff, D); });
  }
  TR(31);
}
template <int R>
__global__ __launch_bounds__(NTHR) void chain_bwd_b_cl_kernel(const sdumc_chain_args a, const int ncl) { chain_bwd_b_cl_body<R>(a, ncl); }

// ------------------------------------------------------------------------------------------------------------------
// stage A backward; 6 exchanges: d_q, d_qin, d_att1, d_u, d_u1 (+ none for d_hpre, the stage's output)
// ------------------------------------------------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ void chain_bwd_a_cl_body(const sdumc_chain_args a, const int ncl) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  using L = BwdA<R>;      // x: d_qp of the three modalities
  float *part = sm + L::part, *s_x = sm + L::x, *s_dq = sm + L::dq, *s_dqin = sm + L::dqin, *s_u = sm + L::u, *s_du = sm + L::du, *s_a2 = sm + L::a2,
        *s_a1 = sm + L::a1, *s_u1 = sm + L::u1;
  CL_PROLOGUE();
  TR(0);
  const int64_t VD = (int64_t)V * D, VQ = (int64_t)V * NQ;
  const float sc = a.relu_scale;
  const bool wr = member == 0;

  // the head: the dq slabs' first batch, alpha / d_alpha and the first layer's weights first -- the query_proj products wait for
  // them -- and with them the saved activations, which nothing reads before the second exchange: they stay in registers until the
  // three products are done and go to LDS in front of the first exchange
  const bool slabs = a.dq_part[0] != nullptr;
  auto dq_desc = [&](int u, const float*& src, int& nc) {
    const int row = u / (D / 4), cq = u - row * (D / 4);           // row = (m R + r) NQ + i
    const int mr = row / NQ, i = row - mr * NQ;
    const int m = mr / R, v = v0 + (mr - m * R);
    const int ncm = sel3(a.dq_nchunk, m);
    src = sel3(a.dq_part, m) + ((size_t)min(v, V - 1) * ncm * NQ + i) * D + 4 * cq;
    nc = v < V ? ncm : 0;
  };
  constexpr int NUX = 3 * R * NQ * (D / 4);
  ChunkItem it;
  f32x4 pa[8];
  RowsReg<NQ * R, D> x[3];
  if (slabs) {      // the pooling backward's dq reduce (a launch between it and this stage) rides here
    it = chunk_item<NUX>(tid, 0, dq_desc);
    chunk_request<NQ * D>(it, pa);
  } else {
    static_for<3>([&](auto mc) { rows_request(x[decltype(mc)::value], a.d_qp + (int64_t)decltype(mc)::value * VQ * D, D, v0 * NQ, V * NQ); });
  }
  const float al = alpha_request<R>(a.alpha, v0, V), dal = alpha_request<R>(a.d_alpha, v0, V);
  CRing ring;
  PF14(D, OC, a.caq_w[0] + coff, D);
  RowsReg<R, 3 * D> g_u;
  RowsReg<R, D> g_a2, g_a1, g_u1[3];
  rows_request(g_u, a.u, 3 * D, v0, V);
  rows_request(g_a2, a.att2, D, v0, V);
  rows_request(g_a1, a.att1, D, v0, V);
  static_for<3>([&](auto mc) { rows_request(g_u1[decltype(mc)::value], a.u1 + decltype(mc)::value * VD, D, v0, V); });
  if (slabs) {
    chunk_drain<NUX, NQ * D>(
        it, pa, dq_desc, [](f32x4& sum, const f32x4 pv, int, int) { sum += pv; },      // ascending c, as dq_reduce_multi
        [&](int u, const f32x4 sum) {
          const int row = u / (D / 4), cq = u - row * (D / 4);
          const int mr = row / NQ, i = row - mr * NQ;
          const int m = mr / R, v = v0 + (mr - m * R);
          if (v < V && (mr & (CL - 1)) == member) st4(a.d_qp + (((size_t)m * V + v) * NQ + i) * D + 4 * cq, sum);
          st4(s_x + (size_t)row * D + 4 * cq, sum);
        });
  } else {
    static_for<3>([&](auto mc) { rows_store(x[decltype(mc)::value], s_x + decltype(mc)::value * NQ * R * D, v0 * NQ, V * NQ); });
  }
  alpha_store<R>(al, sm + L::alpha, v0, V);
  alpha_store<R>(dal, sm + L::dalpha, v0, V);
  __syncthreads();
  // 7'. query_proj: d_q = sum_m d_qp_m W_q[m]  (this member's columns, accumulated in LDS over the three modalities)
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    auto epi = [&](int r, int col, f32x4 v) {
      col += coff;
      if (m > 0) v += ld4(s_dq + r * D + col);
      st4(s_dq + r * D + col, v);
    };
    cxm_run<NQ * R, D, OC>(ring, s_x + m * NQ * R * D, D, a.caq_w[m] + coff, D, part, epi,
                                     [&] { if (m < 2) PF14(D, OC, a.caq_w[m + 1] + coff, D); else PF(D, OC, a.query_w[0] + coff, D); });
  }
  // 6'. mask of q -> d_q (pre-activation): this member's columns, exchanged through HBM
  bwd_a_mask_q<L, OC>(a, sm, v0, V, sc, coff, [](f32x4 g, float*, float* hbm, bool live) {
    if (live) st4_dev(hbm, g);
  });
  rows_store(g_u, s_u, v0, V);
  rows_store(g_a2, s_a2, v0, V);
  rows_store(g_a1, s_a1, v0, V);
  static_for<3>([&](auto mc) { rows_store(g_u1[decltype(mc)::value], s_u1 + decltype(mc)::value * R * D, v0, V); });
  TR(1);
  cl_sync(cl, &s_bail);
  TR(2);
  reload_rows<R>(s_dq, NQ * D, a.d_q, NQ * D, NQ * D, v0, V);
  __syncthreads();
#pragma unroll 1
  for (int i = 0; i < 7; ++i) {
    float* dst = a.d_qin + i * VD + (int64_t)v0 * D;
    auto epi = [&](int r, int col, f32x4 v) {
      col += coff;
      if (v0 + r < V) st4_dev(dst + (int64_t)r * D + col, v);
    };
    cxm_run<R, D, OC>(ring, s_dq + i * D, NQ * D, a.query_w[i] + coff, D, part, epi,
                                [&] { PF(D, OC, (i < 6 ? a.query_w[i + 1] : a.att3_w) + coff, D); });
  }
  TR(3);
  cl_sync(cl, &s_bail);
  TR(4);
  for (int i = 0; i < 7; ++i) reload_rows<R>(s_dqin + i * R * D, D, a.d_qin + i * VD, D, D, v0, V);
  __syncthreads();
  // 5'. fusion algebra backward and 4'. fc_att: d_att2 (every member; HBM by member 0)
  bwd_a_fusion<L>(a, sm, v0, V, wr);
  bwd_a_datt2<L>(a, sm, v0, V, sc, wr);
  //     attention_mlp.3: d_att1 = (d_att2 W) [att1 > 0] s
  {
    float* dst = a.d_att1 + (int64_t)v0 * D;
    auto epi = [&](int r, int col, f32x4 v) {
      col += coff;
      if (v0 + r < V) st4_dev(dst + (int64_t)r * D + col, mask_val(v, ld4(s_a1 + r * D + col), sc));
    };
    cxm_run<R, D, OC>(ring, s_a2, D, a.att3_w + coff, D, part, epi, [&] { PF(D, OC, a.att0_w + member * OC, 3 * D); });
  }
  TR(5);
  cl_sync(cl, &s_bail);
  TR(6);
  reload_rows<R>(s_a1, D, a.d_att1, D, D, v0, V);
  __syncthreads();
  //     .0: d_u = (d_u + d_att1 W) [u > 0] s   (768 columns = 12 blocks of 64: member j takes blocks j, j + 4, j + 8)
#pragma unroll 1
  for (int blk = member; blk < 12; blk += CL) {
    float* dst = a.d_u + (int64_t)v0 * 3 * D;
    const int boff = blk * OC;
    auto epi = [&](int r, int col, f32x4 v) {
      col += boff;
      if (v0 + r < V) st4_dev(dst + (int64_t)r * 3 * D + col, mask_val(v + ld4(s_du + r * 3 * D + col), ld4(s_u + r * 3 * D + col), sc));
    };
    cxm_run<R, D, OC>(ring, s_a1, D, a.att0_w + boff, 3 * D, part, epi, [&] {
      if (blk + CL < 12) PF(D, OC, a.att0_w + boff + CL * OC, 3 * D);
      else PF(D, OC, a.umlp3_w[0] + coff, D);
    });
  }
  TR(7);
  cl_sync(cl, &s_bail);
  TR(8);
  reload_rows<R>(s_du, 3 * D, a.d_u, 3 * D, 3 * D, v0, V);
  __syncthreads();
  // 3'. audio / text / video_mlp: d_u1 = (d_u_m W3) [u1 > 0] s ; d_hpre = d_u1 W0
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    float* dst = a.d_u1 + m * VD + (int64_t)v0 * D;
    const float* y = s_u1 + m * R * D;
    auto epi = [&](int r, int col, f32x4 v) {
      col += coff;
      if (v0 + r < V) st4_dev(dst + (int64_t)r * D + col, mask_val(v, ld4(y + r * D + col), sc));
    };
    cxm_run<R, D, OC>(ring, s_du + m * D, 3 * D, a.umlp3_w[m] + coff, D, part, epi,
                                [&] { PF(D, OC, (m < 2 ? a.umlp3_w[m + 1] : a.umlp0_w[0]) + coff, D); });
  }
  TR(9);
  cl_sync(cl, &s_bail);
  TR(10);
  cl_exit(cl);
  for (int m = 0; m < 3; ++m) reload_rows<R>(s_u1 + m * R * D, D, a.d_u1 + m * VD, D, D, v0, V);
  __syncthreads();
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    float* dst = a.d_hpre + m * VD + (int64_t)v0 * D;
    auto epi = [&](int r, int col, f32x4 v) {
      col += coff;
      if (v0 + r < V) st4(dst + (int64_t)r * D + col, v);
    };
    cxm_run<R, D, OC>(ring, s_u1 + m * R * D, D, a.umlp0_w[m] + coff, D, part, epi,
                                [&] { if (m < 2) PF(D, OC, a.umlp0_w[m + 1] + coff, D); });
  }
  TR(31);
}
template <int R>
__global__ __launch_bounds__(NTHR) void chain_bwd_a_cl_kernel(const sdumc_chain_args a, const int ncl) { chain_bwd_a_cl_body<R>(a, ncl); }

#undef PF
#undef PF14
#undef CL_PROLOGUE

// per device: the clusters' counters (zero between launches), the error word, and the event that serialises cluster launches
// of different streams
struct ClusterDev {
  std::mutex mu;
  uint32_t* flags = nullptr;     // [128 clusters][64 words]: arrival counter at +0, departure counter at +32 (own 128-byte lines)
  int32_t* err = nullptr;
  unsigned long long* trace = nullptr;   // 4 x 32 time stamps, written only while tracing is on
  uint32_t* dbg = nullptr;               // 256 words of diagnosis records (cl_mode bit 4)
  bool tracing = false;
  hipEvent_t done = nullptr;
  hipStream_t last = nullptr;
  bool any = false;
  bool multi = false;            // more than one stream has launched clustered kernels on this device: record the event eagerly
  int cus = 0;
  int attr = 0;      // 0 = not tried, 1 = the kernels' dynamic-LDS limits are set on this device and every kernel fits a CU, -1 = failed
  int test_hold = 0;
};
ClusterDev g_cl[16];
constexpr int kMaxClusters = 128;

ClusterDev* cluster_dev() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  ClusterDev& d = g_cl[dev];
  std::lock_guard<std::mutex> lk(d.mu);
  if (!d.flags) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return nullptr;
    uint32_t* f = nullptr;
    if (hipMalloc(&f, (kMaxClusters * 64 + 64 + 256 + 256) * sizeof(uint32_t)) != hipSuccess) return nullptr;
    if (hipMemset(f, 0, (kMaxClusters * 64 + 64 + 256 + 256) * sizeof(uint32_t)) != hipSuccess) return nullptr;
    d.trace = reinterpret_cast<unsigned long long*>(f + kMaxClusters * 64 + 64);
    d.dbg = f + kMaxClusters * 64 + 64 + 256;
    if (hipEventCreateWithFlags(&d.done, hipEventDisableTiming) != hipSuccess) return nullptr;
    d.err = reinterpret_cast<int32_t*>(f + kMaxClusters * 64);
    d.cus = cus;
    d.flags = f;
  }
  return &d;
}

}  // namespace

// 1 = V samples qualify for the cluster kernels on the current device (every workgroup resident at once)
namespace { std::atomic<int> g_cluster_on{-1}; }
// experiment / test knob (also SDUMC_CHAIN_CLUSTER=0|1 at start-up): 0 keeps chain.hip's one-workgroup-per-sample-pair kernels
extern "C" int sdumc_set_chain_cluster(int on) {
  g_cluster_on.store(on ? 1 : 0);
  return SDUMC_OK;
}
namespace {
// per device, under d->mu: raise the kernels' dynamic-LDS limit and check with the occupancy query that a workgroup of each of
// them fits a CU at all (the members of a cluster spin on each other: a grid that cannot be resident must not be launched)
template <int R>
bool cluster_prepare(ClusterDev* d) {
  std::lock_guard<std::mutex> lk(d->mu);
  if (d->attr == 0) {
    d->attr = -1;
    if (!(sdumc_set_dyn_lds(chain_fwd_a_cl_kernel<R>, 158 * 1024) && sdumc_set_dyn_lds(chain_fwd_b_cl_kernel<R>, FwdB<R>::bytes) &&
          sdumc_set_dyn_lds(chain_bwd_b_cl_kernel<R>, BwdB<R>::bytes) && sdumc_set_dyn_lds(chain_bwd_a_cl_kernel<R>, BwdA<R>::bytes)))
      return false;
    int n[4] = {0, 0, 0, 0};
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n[0], chain_fwd_a_cl_kernel<R>, NTHR, FwdA<R>::bytes) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&n[1], chain_fwd_b_cl_kernel<R>, NTHR, FwdB<R>::bytes) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&n[2], chain_bwd_b_cl_kernel<R>, NTHR, BwdB<R>::bytes) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&n[3], chain_bwd_a_cl_kernel<R>, NTHR, BwdA<R>::bytes) != hipSuccess)
      return false;
    if (n[0] < 1 || n[1] < 1 || n[2] < 1 || n[3] < 1) return false;
    d->attr = 1;
  }
  return d->attr == 1;
}
}  // namespace

extern "C" int sdumc_chain_cluster_ok_(int V) {
  if (g_cluster_on.load() < 0) { const char* e = getenv("SDUMC_CHAIN_CLUSTER"); g_cluster_on.store(e ? (atoi(e) ? 1 : 0) : 1); }
  if (!g_cluster_on.load()) return 0;
  return sdumc_chain_cluster_fits_(V);
}
extern "C" int sdumc_chain_cluster_fits_(int V) {
  if (V <= 0) return 0;
  ClusterDev* d = cluster_dev();
  if (!d) return 0;
  const int ncl = (V + 1) / 2;
  if (!(ncl <= kMaxClusters && ncl * CL <= d->cus)) return 0;
  return cluster_prepare<2>(d) ? 1 : 0;
}

// which: 0 = stage A forward, 1 = stage B forward, 2 = stage B backward, 3 = stage A backward; 1 = shape does not qualify
extern "C" int sdumc_chain_cluster_launch_(const sdumc_chain_args* ap, int which, void* stream) {
  if (!ap || ap->V <= 0 || which < 0 || which > 3) return SDUMC_EINVAL;
  if (!sdumc_chain_cluster_fits_(ap->V)) return 1;      // (whether to take the clustered kernels at all is the caller's decision)
  constexpr int R = 2;
  ClusterDev* d = cluster_dev();
  if (!d) return SDUMC_ELAUNCH;
  sdumc_chain_args a = *ap;
  a.cl_test_hold = d->test_hold;
  a.cl_flags = d->flags;
  a.cl_err = d->err;
  a.cl_trace = d->tracing ? d->trace + 32 * which : nullptr;
  a.w_bf16 = 0;
  a.cl_mode = 0;      // (the exchange / diagnosis variants of round 4's hunt for the packed-fp32 hazard: reachable from a debugger only)
  a.cl_dbg = d->dbg;
  const int ncl = (a.V + R - 1) / R;
  const dim3 grid(ncl * CL), blk(NTHR);
  hipStream_t st = as_stream(stream);
  std::lock_guard<std::mutex> lk(d->mu);
  // One cluster kernel at a time per device: a launch on ANOTHER stream than the previous one is ordered behind everything
  // submitted to that stream so far.  The event is recorded here, when it is needed, not after every launch: an event record
  // behind a kernel costs the recording stream ~8 us before its next kernel starts (four of them sat on the step's critical
  // path, between the utterance-level stages and the pooling / loss launches that follow them).
  // Once a SECOND stream has launched clustered kernels on this device (several host threads with their own contexts), every
  // launch records the event on its own -- live -- stream right away, and a launch of another stream only waits on it: the handle
  // of a stream that may have been destroyed in the meantime is touched at that first hand-over only (single-stream callers, the
  // normal case, never record).
  if (d->any && d->last != st) {
    if (!d->multi) {
      d->multi = true;
      if (hipEventRecord(d->done, d->last) != hipSuccess) {
        (void)hipGetLastError();                                 // (the other stream is gone: nothing of it can still be running
        if (hipDeviceSynchronize() != hipSuccess) return SDUMC_ELAUNCH;   //  after this)
      }
    }
    if (hipStreamWaitEvent(st, d->done, 0) != hipSuccess) return SDUMC_ELAUNCH;
  }
  const size_t smem_a = (a.cl_mode & 32) ? (size_t)158 * 1024 : FwdA<R>::bytes;   // (bit 5, diagnosis: the whole CU's LDS -> no LDS-using neighbour on the CU)
  switch (which) {
    case 0: hipLaunchKernelGGL(chain_fwd_a_cl_kernel<R>, grid, blk, smem_a, st, a, ncl); break;
    case 1: hipLaunchKernelGGL(chain_fwd_b_cl_kernel<R>, grid, blk, FwdB<R>::bytes, st, a, ncl); break;
    case 2: hipLaunchKernelGGL(chain_bwd_b_cl_kernel<R>, grid, blk, BwdB<R>::bytes, st, a, ncl); break;
    default: hipLaunchKernelGGL(chain_bwd_a_cl_kernel<R>, grid, blk, BwdA<R>::bytes, st, a, ncl); break;
  }
  SDUMC_CHECK_LAUNCH();
  if (d->multi && hipEventRecord(d->done, st) != hipSuccess) return SDUMC_ELAUNCH;
  d->last = st;
  d->any = true;
  return SDUMC_OK;
}

// A stream that is about to be destroyed (sdumc_ctx_destroy: the context's lanes) must not stay behind as "the stream of the last
// clustered launch": the next launch would record its ordering event on a dead handle.  Waits for the stream's work and forgets it.
// (Caller-owned streams: a caller that destroys the stream of its last step must have synchronised it -- include/sdumc_hip.h.)
// (every device's record is searched: the context may be destroyed while another device is current)
extern "C" int sdumc_chain_cluster_forget_stream_(void* stream) {
  for (int dev = 0; dev < 16; ++dev) {
    ClusterDev& d = g_cl[dev];
    std::lock_guard<std::mutex> lk(d.mu);
    if (d.any && d.last == as_stream(stream)) {
      if (hipStreamSynchronize(d.last) != hipSuccess) return SDUMC_ELAUNCH;
      d.any = false;
      d.last = nullptr;
    }
  }
  return SDUMC_OK;
}

extern "C" const int32_t* sdumc_chain_cluster_err_ptr_() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  return g_cl[dev].err;
}

// clears the error word of the current device (after the caller has dealt with a failed step); synchronises the device
extern "C" int sdumc_chain_cluster_reset_error(void) {
  ClusterDev* d = cluster_dev();
  if (!d) return SDUMC_ELAUNCH;
  if (hipDeviceSynchronize() != hipSuccess) return SDUMC_ELAUNCH;
  // (the counters too: a launch that bailed out may have left arrivals behind)
  if (hipMemset(d->flags, 0, (kMaxClusters * 64 + 64) * sizeof(uint32_t)) != hipSuccess) return SDUMC_ELAUNCH;
  return SDUMC_OK;
}
// Data-parallel runs: the error word is per device, so a rank whose spin hit its cap would all-reduce garbage gradients into
// every rank while only ITS Adam applies nothing.  The ranks therefore exchange the word with the gradient bucket: _flag writes
// 1.0 / 0.0 into a float the caller appends to the bucket (stream-ordered, no host sync), the sum all-reduce carries it, and
// _merge sets the local word when the reduced value is non-zero -- every rank then skips the update and raises together.
namespace {
__global__ void cl_err_flag_kernel(const int32_t* err, float* flag) { flag[0] = (err && *err != 0) ? 1.f : 0.f; }
__global__ void cl_err_merge_kernel(int32_t* err, const float* flag) {
  if (flag[0] != 0.f) *err = 1;      // (NaN included: a poisoned reduction is a failure too)
}
}  // namespace
extern "C" int sdumc_chain_cluster_error_flag(float* flag, void* stream) {
  if (!flag) return SDUMC_EINVAL;
  ClusterDev* d = cluster_dev();
  if (!d) return SDUMC_ELAUNCH;
  hipLaunchKernelGGL(cl_err_flag_kernel, dim3(1), dim3(1), 0, as_stream(stream), d->err, flag);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}
extern "C" int sdumc_chain_cluster_error_merge(const float* flag, void* stream) {
  if (!flag) return SDUMC_EINVAL;
  ClusterDev* d = cluster_dev();
  if (!d) return SDUMC_ELAUNCH;
  hipLaunchKernelGGL(cl_err_merge_kernel, dim3(1), dim3(1), 0, as_stream(stream), d->err, flag);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

// test hook: on != 0 makes workgroup 0 of every following cluster launch withhold its arrivals, so that its cluster runs into
// the spin cap (error word set, kernel finishes with wrong data): the failure path can be driven on purpose
extern "C" int sdumc_chain_cluster_test_hold_(int on) {
  ClusterDev* d = cluster_dev();
  if (!d) return SDUMC_ELAUNCH;
  std::lock_guard<std::mutex> lk(d->mu);
  d->test_hold = on ? 1 : 0;
  return SDUMC_OK;
}

// 0 = no cluster spin ever exceeded its cap on the current device (synchronises the device; tests)
extern "C" int sdumc_chain_cluster_error_() {
  ClusterDev* d = cluster_dev();
  if (!d) return -1;
  int32_t e = 0;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(&e, d->err, sizeof(e), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return e;
}

// diagnosis records of cl_mode bit 4 (synchronises the device); clears them
extern "C" int sdumc_chain_cluster_debug_read_(uint32_t* out, int n) {
  ClusterDev* d = cluster_dev();
  if (!d || !out || n < 1 || n > 256) return SDUMC_EINVAL;
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, d->dbg, n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return SDUMC_ELAUNCH;
  if (hipMemset(d->dbg, 0, 256 * sizeof(uint32_t)) != hipSuccess) return SDUMC_ELAUNCH;
  return SDUMC_OK;
}

// debug: on = 1 makes workgroup 0 of every cluster kernel stamp its phase boundaries; out (4 x 32 doubles, may be null) receives
// the stamps of the last launches in microseconds since each kernel's first stamp (synchronises the device)
extern "C" int sdumc_chain_cluster_trace_(int on, double* out) {
  ClusterDev* d = cluster_dev();
  if (!d) return SDUMC_ELAUNCH;
  if (out) {
    unsigned long long h[128];
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, d->trace, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return SDUMC_ELAUNCH;
    for (int k = 0; k < 4; ++k)
      for (int i = 0; i < 32; ++i) out[k * 32 + i] = h[k * 32 + i] ? (double)(h[k * 32 + i] - h[k * 32]) * 0.01 : -1.0;
    if (hipMemset(d->trace, 0, sizeof(h)) != hipSuccess) return SDUMC_ELAUNCH;
  }
  std::lock_guard<std::mutex> lk(d->mu);
  d->tracing = on != 0;
  return SDUMC_OK;
}

SDUMC_PRELOAD_HOOK(chain_cluster)      // (common.h)
