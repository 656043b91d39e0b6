// gemm_rows.hip — C[M x 256] = act((A . keep) B * scale + bias) (+ C): the tall 256 x 256 products of the frame-level part in
// one persistent, B-stationary launch (gfx950).
//
// What runs here (C2 shapes): the input gradients dxd += dz W of the input_proj layers of FRA2UTT_new / Cross_Attention
// (autograd of model :60, :82; M = 2*B*T up to 48000 rows, B = the weight as stored, K = N = 256).  The same kernel computes the
// key projections keys = tanh(drop(x) W^T + b) (B = a transposed weight copy, input dropout fused on x): a tested entry point
// (tests/test_gpu_gemm_rows.py) the engine does not call -- see engine.hip rows_on() for the measurement.
//
// Why a kernel of its own: these products are tall and thin -- a 64-row tile has only 256 rows of K behind it, so a tiled
// GEMM launch (gemm_wide.hip, gemm_f32.hip) is one short k-loop per workgroup: ring start-up, 8-16 k-tiles, epilogue, exit;
// both operands cross LDS, B (the same 256 KB for every tile) is fetched again by every workgroup, and A is read twice because
// the tile is 128 columns wide.  They ran at 66-85 TF of the 157 TF fp32 matrix peak; this one at 101-113 (tools/rows_bench.py).
//
// Structure:
//   * one 512-thread workgroup per CU works through a contiguous range of 64-row tiles; a tile is 64 x 256 -- ALL columns, so
//     A is read from HBM exactly once;
//   * B never touches LDS: wave w keeps columns [32 w, 32 w + 32) of all 256 rows of K in 128 VGPRs (one MFMA B operand per
//     register) for as long as the workgroup stays on one problem;
//   * A streams through an 8-slot LDS ring (one slot = 64 rows x 32 k = 8 KB, a tile = 8 slots) by LDS-DMA, six stages ahead,
//     and the ring never drains between tiles: the loads of the next tile are in flight while this tile's epilogue runs.
//     The rows are k-contiguous; the 16-byte chunks of a row are XOR-swizzled by the row (applied to the DMA's source address
//     and again at the ds_read_b128 fragment read: conflict-free);
//   * every wave multiplies the same A fragments (64 rows) with its own 32 columns: 2 independent 32x32x2 fp32 MFMA chains, 32
//     MFMAs per stage and wave against 8 ds_read_b128 and one DMA instruction;
//   * the input-dropout keep-bits of a tile (64 rows x 64 bytes) ride ahead of it as two 256-byte pieces per wave
//     (double-buffered) and are applied to the A fragments; the scale 1 / (1 - p) multiplies the tile once, in the epilogue;
//   * `accumulate`: the C tile is prefetched into registers two stages before the epilogue needs it;
//   * round 5 (split and bf16 kernels): the attention pooling's own input gradient as one more k-tile (`pool_w` / `pool_g`) and the
//     mask-sum of the frame-level input dropouts as the epilogue (`c_bits`, `fold`): dx of a modality leaves the launch in one pass
//     (gr_split_kernel<.., POOL, FOLD>, gr_bf16_kernel<ACC, FOLD>; sdumc_hip.h: sdumc_rows_problem).
// The vector-memory queue of a wave holds, in issue order, LDS-DMA loads, the C prefetch and the epilogue's stores; the waits
// are counted (s_waitcnt vmcnt(n) with n = the loads issued after the one waited for -- loads return in order; stores only make
// a wait conservative), so nothing ever drains the queue inside a problem.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "common.h"

namespace sdumc_gr {

constexpr int BM = 64, DK = 256, DN = 256, BK = 32;
constexpr int NS = DK / BK;                      // stages per tile = ring slots
constexpr int NW = 8, NTHR = 64 * NW;
constexpr int PF = 6;                            // stages in flight ahead of the one being multiplied
constexpr int A_STAGE = BM * BK * 4;             // 8 KB: one 1-KB piece per wave
constexpr int RING = NS * A_STAGE;
constexpr int QW = DK / 4;                       // keep-bits: one byte per 4 columns (low nibble), 64 bytes per row
constexpr int BITS_TILE = BM * QW;               // 4 KB: two 256-byte pieces per wave
constexpr int LDS_BYTES = RING + 2 * BITS_TILE;
constexpr int MAXP = SDUMC_ROWS_MAX_PROBLEMS;
#define SDUMC_GR_NULL_OFF 0x80000000u            /* a byte offset outside every descriptor: the load returns zeros */
static_assert(A_STAGE == NW * 1024 && BITS_TILE == NW * 512 && NS == 8, "pieces per wave; the stage list below is written out for 8");

struct Launch {
  sdumc_rows_problem p[MAXP];
  int32_t unit0[MAXP + 1];   // first 64-row tile of problem i in the launch's tile list; unit0[n] = all tiles
  int32_t n, nwg;
};

// ---- the vector-memory bookkeeping of one wave --------------------------------------------------------------------------
// The ledger of a kernel: every issue point t of the 8-point cycle issues one A piece (the stage `pf` ahead), and some carry
// further PIECES -- `ops` vector-memory instructions before or after that A piece.  Each kernel states its pieces once; its stage
// code asks carries() of the same entry whether to issue, and younger() counts from it: the two cannot disagree about where.
// A load added to an issue point = one entry here plus the issuing code, `ops` being the constant that code loops over or asserts.
struct Piece {
  int ops;
  unsigned points;         // bit t: carried at issue point t (0: the variant does not have the piece)
  bool before_a = false;
};
struct Ledger {
  int pf, ahead;           // the A piece of stage s + pf is issued at point s; the wait in stage s is for the A piece of stage s + ahead
  Piece pc[4];
};
constexpr unsigned at(bool on, int t) { return on ? 1u << t : 0u; }
constexpr bool carries(Piece p, int t) { return (p.points >> t) & 1u; }
// the operations issued after the A piece that stage s waits for (issued at point s + ahead - pf): what followed it at its own
// issue point, plus every operation of the issue points between
constexpr int younger(const Ledger& g, int s) {
  const int t0 = ((s + g.ahead - g.pf) % NS + NS) % NS, between = g.pf - g.ahead - 1;
  int n = between;                                     // (their A pieces)
  for (const Piece& p : g.pc) {
    if (carries(p, t0) && !p.before_a) n += p.ops;
    for (int t = 1; t <= between; ++t) n += carries(p, (t0 + t) % NS) ? p.ops : 0;
  }
  return n;
}
constexpr int BITS_OPS = 2, CPRE_OPS = 32;      // the keep-bits of a tile: two pieces; a C tile into registers: one load per accumulator element

// gr_kernel: the two keep-bits pieces of the next tile ahead of the A piece of point 2, the C tile behind that of point 5
enum { G_BITS, G_C };
template <bool MASK, bool ACC>
constexpr Ledger plain = {PF, 1, {{BITS_OPS, at(MASK, 2), true}, {CPRE_OPS, at(ACC, 5)}}};

// (the tables this produces, stage 0..7: plain 4 x 8; masked 4 4 4 6 6 6 6 4; accumulating 36 36 36 4 4 4 36 36)
static_assert(younger(plain<false, false>, 0) == 4 && younger(plain<false, false>, 5) == 4, "plain");
static_assert(younger(plain<true, false>, 2) == 4 && younger(plain<true, false>, 3) == 6 && younger(plain<true, false>, 6) == 6 && younger(plain<true, false>, 7) == 4, "masked");
static_assert(younger(plain<false, true>, 2) == 36 && younger(plain<false, true>, 3) == 4 && younger(plain<false, true>, 5) == 4 && younger(plain<false, true>, 6) == 36, "accumulating");

template <bool MASK, bool ACC>
__global__ __launch_bounds__(NTHR, 2) void gr_kernel(const Launch L) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int n0 = wave * 32;
  const int U = L.unit0[L.n];
  int u = (int)(((uint32_t)blockIdx.x * (uint32_t)U) / (uint32_t)L.nwg);
  const int u_end = (int)((((uint32_t)blockIdx.x + 1u) * (uint32_t)U) / (uint32_t)L.nwg);

  // fragment reads: rows 32 i + li of the slot, 16-byte chunk 2 c + lh (k = 8 c + 4 lh .. + 3 of the stage)
  uint32_t foff[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) foff[c] = (uint32_t)(li * (BK * 4) + (((2 * c + lh) ^ (li & 7)) << 4));
  const uint32_t moff = (uint32_t)(li * QW), msh = 8u * (uint32_t)lh;
  // LDS-DMA: this wave's piece of a stage = rows 8 wave .. + 7; lane -> row 8 wave + lane / 8, LDS chunk lane % 8
  const int dr = 8 * wave + (lane >> 3);
  const uint32_t dq16 = (uint32_t)(((lane & 7) ^ (lane >> 3)) << 4);    // source chunk of that LDS chunk (bytes)
  char* const bits_lds = lds + RING;

  typedef float f32x4_ __attribute__((ext_vector_type(4)));
  f32x16 acc[2];

  while (u < u_end) {
    int p = 0;
    while (p + 1 < L.n && L.unit0[p + 1] <= u) ++p;
    const sdumc_rows_problem& pr = L.p[p];
    const int ub = min(u_end, L.unit0[p + 1]);
    const int tile0 = L.unit0[p];
    const uint32_t lda4 = (uint32_t)pr.lda * 4u, ldc4 = (uint32_t)pr.ldc * 4u;
    const int a_rows = pr.a_row_mod > 0 ? pr.a_row_mod : pr.M;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pr.A), 0, (int)((uint32_t)a_rows * lda4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rbits = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(MASK ? pr.a_bits : (const uint8_t*)pr.A), 0,
                                                                           MASK ? (int)((uint32_t)pr.M * QW) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(pr.C, 0, (int)((uint32_t)pr.M * ldc4), 0x00020000);

    // B: one register per MFMA step j = 16 s + 4 c + e  <->  k = 32 s + 8 c + 4 lh + e (the order the A fragments arrive in)
    float breg[DK / 2];
    {
      const uint32_t ldb4 = (uint32_t)pr.ldb * 4u;
      const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pr.B), 0, (int)((uint32_t)DK * ldb4), 0x00020000);
      const uint32_t bo = (uint32_t)(4 * lh) * ldb4 + (uint32_t)(n0 + li) * 4u;
#pragma unroll
      for (int j = 0; j < DK / 2; ++j)
        breg[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rb, bo, (32 * (j >> 4) + 8 * ((j >> 2) & 3) + (j & 3)) * ldb4, 0));
    }
    const float bias = pr.bias ? pr.bias[n0 + li] : 0.f;
    const float scale = MASK ? pr.a_scale : 1.f;
    const bool do_tanh = pr.act == SDUMC_ACT_TANH;

    // byte offset of this lane's 16 bytes of stage 0 of tile t (rows past M: outside the descriptor, or wrapped by the modulo)
    auto a_off = [&](int t) -> uint32_t {
      int r = (t - tile0) * BM + dr;
      if (pr.a_row_mod > 0) r %= pr.a_row_mod;
      return (uint32_t)r * lda4 + dq16;
    };
    // (the wave's 8 rows of keep-bits are 512 contiguous bytes: two 256-byte pieces)
    auto bits_off = [&](int t) -> uint32_t { return (uint32_t)((t - tile0) * BM + 8 * wave) * QW + 4u * lane; };
    auto issue_a = [&](uint32_t off, int chunk) {    // stage `chunk` of a tile into slot `chunk` (the k offset rides in the scalar
                                                     // offset: an instruction offset would move the LDS address too)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void_t*)(lds + chunk * A_STAGE + wave * 1024), 16, off, chunk * (BK * 4), 0, 0);
    };
    auto issue_bits = [&](uint32_t off, int par) {
      static_assert(BITS_OPS == 2, "the two instructions below");
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rbits, (lds_void_t*)(bits_lds + par * BITS_TILE + wave * 512), 4, off, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rbits, (lds_void_t*)(bits_lds + par * BITS_TILE + wave * 512 + 256), 4, off, 256, 0, 0);
    };
    // half h of a stage = k 16 h .. 16 h + 15 of its 32: chunks c = 2 h, 2 h + 1 of both 32-row blocks -- the two accumulator
    // chains alternate inside every half
    struct Frag {
      f32x4_ a[2][2];
      uint32_t mw[2];
    };
    auto read_frag = [&](int slot, int h, int par, Frag& f) {
      const char* base = lds + slot * A_STAGE;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) f.a[i][cc] = *reinterpret_cast<const f32x4_*>(base + i * (32 * BK * 4) + foff[2 * h + cc]);
      if constexpr (MASK) {   // keep-bits bytes 8 slot + 4 h .. + 3 of the row; byte 2 cc + lh is chunk (2 h + cc, lh): its bit e -> bit 16 cc + e
#pragma unroll
        for (int i = 0; i < 2; ++i)
          f.mw[i] = *reinterpret_cast<const uint32_t*>(bits_lds + par * BITS_TILE + i * (32 * QW) + moff + 8 * slot + 4 * h) >> msh;
      }
    };
    auto mma = [&](Frag& f, int h, int s) {
#pragma unroll
      for (int cc = 0; cc < 2; ++cc)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            float a = f.a[i][cc][e];
            if constexpr (MASK) a = __uint_as_float(__float_as_uint(a) & (uint32_t)__builtin_amdgcn_sbfe((int)f.mw[i], 16 * cc + e, 1u));
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, breg[16 * s + 4 * (2 * h + cc) + e], acc[i], 0, 0, 0);
          }
      if constexpr (MASK) {   // keep every mask next to its MFMA (all 16 computed up front cost 16 more live registers: spills)
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        }
      }
    };

    // ---- prologue: the ring belongs to this problem from here (the previous one drained it) ----
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    int par = 0;
    {
      const uint32_t o = a_off(u);
      if constexpr (MASK) issue_bits(bits_off(u), 0);
#pragma unroll
      for (int s = 0; s < PF; ++s) issue_a(o, s);
    }
    __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
    __builtin_amdgcn_s_barrier();
    Frag fa, fb;
    read_frag(0, 0, par, fa);

    // ---- steady state: 8 stages per tile, one barrier per stage ----
#pragma nounroll
    for (; u < ub; ++u) {
      const uint32_t o_cur = a_off(u);
      const uint32_t o_nxt = u + 1 < ub ? a_off(u + 1) : SDUMC_GR_NULL_OFF;
      const uint32_t b_nxt = u + 1 < ub ? bits_off(u + 1) : SDUMC_GR_NULL_OFF;
      // C/D layout of the 32x32 MFMA: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
      const uint32_t c_off = (uint32_t)((u - tile0) * BM + 4 * lh) * ldc4 + (uint32_t)(n0 + li) * 4u;
      float cpre[ACC ? 32 : 1];
      auto stage = [&](auto sc) {
        constexpr int s = decltype(sc)::value;
        constexpr const Ledger& G = plain<MASK, ACC>;
        read_frag(s, 1, par, fb);
        __builtin_amdgcn_sched_barrier(0);
        mma(fa, 0, s);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(waitcnt_vm(younger(G, s)));
        __builtin_amdgcn_s_barrier();
        // (the outer conditions keep what a variant lacks out of this generic lambda's captures: with `cpre` or `issue_bits` captured
        //  and unused, the register allocation of the whole kernel came out differently)
        if constexpr (MASK) {
          if constexpr (carries(G.pc[G_BITS], s)) issue_bits(b_nxt, par ^ 1);
        }
        issue_a(s + PF < NS ? o_cur : o_nxt, (s + PF) % NS);
        if constexpr (ACC) {
          if constexpr (carries(G.pc[G_C], s)) {
            static_assert(CPRE_OPS == 2 * 16, "one load per accumulator element");
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
              for (int e = 0; e < 16; ++e)
                cpre[i * 16 + e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rc, c_off, (32 * i + (e & 3) + 8 * (e >> 2)) * ldc4, 0));
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        read_frag((s + 1) % NS, 0, s + 1 == NS ? par ^ 1 : par, fa);
        __builtin_amdgcn_sched_barrier(0);
        mma(fb, 1, s);
        __builtin_amdgcn_sched_barrier(0);
      };
      stage(std::integral_constant<int, 0>{});
      stage(std::integral_constant<int, 1>{});
      stage(std::integral_constant<int, 2>{});
      stage(std::integral_constant<int, 3>{});
      stage(std::integral_constant<int, 4>{});
      stage(std::integral_constant<int, 5>{});
      stage(std::integral_constant<int, 6>{});
      stage(std::integral_constant<int, 7>{});
      // ---- epilogue of tile u (the next tile's stages are in flight behind it) ----
      auto epilogue = [&](auto tanh_c) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            float v = acc[i][e];
            if constexpr (MASK) v *= scale;
            v += bias;
            if constexpr (ACC) v += cpre[i * 16 + e];
            if constexpr (decltype(tanh_c)::value) v = fast_tanh(v);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rc, c_off, (32 * i + (e & 3) + 8 * (e >> 2)) * ldc4, 0);
            acc[i][e] = 0.f;
          }
      };
      if (do_tanh) epilogue(std::true_type{});
      else epilogue(std::false_type{});
      __builtin_amdgcn_sched_barrier(0);
      par ^= 1;
    }
    // the last tile's issue points loaded "the next tile" from nowhere (zeros into free slots): let them land before the next
    // problem's prologue reuses the ring
    __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
    __builtin_amdgcn_s_barrier();
  }
#endif
}

// ------------------------------------------------------------------------------------------------------------------------
// The fp32 launch with its products on the bf16 matrix pipe (sdumc_hip.h: sdumc_set_split_; the arithmetic -- every fp32 operand
// the exact sum of three bf16 parts, the six largest of the nine part products accumulated in fp32 -- is described in
// gemm_group.hip).  What changes against gr_kernel:
//   * A is split ONCE per workgroup, not once per wave: after the barrier that publishes raw stage s + 1 every lane converts one
//     16-byte chunk of it (4 k of one row; the keep-bits are applied here) into three bf16 planes in LDS ([64 rows][32 k] bf16
//     per plane and stage, double-buffered, 16-byte chunks XOR-swizzled by row / 4); the MFMA operands of stage s + 1 are then
//     one ds_read_b128 per plane -- the VALU work per wave and stage is 22 operations for A instead of 176;
//   * B stays fp32 in 128 VGPRs (three planes would be 192) and the 16 values of a stage are split beside the MFMAs (88 VALU
//     operations per stage and wave, under the 24 MFMAs = 768 matrix-pipe cycles);
//   * a lane's eight k of one MFMA operand are contiguous (k = 16 h + 8 lh .. + 7 of the stage), so B is loaded in that order;
//   * the raw ring is consumed one stage earlier (the conversion of stage s + 1 runs in stage s), so the LDS-DMA runs PF2 = 7
//     stages ahead instead of 6 and the keep-bits of the next tile are issued at stage 0.
// One barrier per stage, as before: it publishes raw stage s + 2 AND the planes of stage s + 1, and it retires the planes of
// stage s - 1 (overwritten by the conversion in stage s + 1... of the same parity).
// ------------------------------------------------------------------------------------------------------------------------
namespace sp {
constexpr int PF2 = 7;
constexpr int PL_STAGE = 3 * BM * BK * 2;            // three planes of one stage: 12 KB
constexpr int C_TILE = BM * DN * 4;                  // `accumulate`: the C tile waits in LDS (64 KB; MASK and ACC exclude each other,
                                                     // so it starts where the keep-bits would lie) -- 32 registers a wave does not have
constexpr int LDS_BYTES2 = RING + 2 * PL_STAGE + (C_TILE > 2 * BITS_TILE ? C_TILE : 2 * BITS_TILE);
constexpr int C_OPS = BM / NW;                       // LDS-DMA instructions per wave for the C tile: one row each
// POOL (sdumc_rows_problem.pool_w / pool_g): the operands of the tile's extra k-tile -- its 64 rows of attention weights (<= 2 KB)
// and the masked dout rows of the <= 2 samples it spans (2 x 8 x 1 KB) -- ride in by LDS-DMA at issue point 1 of the tile itself
// (three instructions per wave) and are multiplied behind stage 7: the wait of stage 7 is for a piece issued after them.
constexpr int P_OPS = 3;
constexpr int POOL_W = BM * 8 * 4, POOL_G = 2 * 8 * DN * 4;      // LDS bytes (where the keep-bits / the C tile lie in the other variants)
// FOLD (sdumc_rows_problem.fold): `fold` row blocks of A add up, each under its own keep-bits, into ONE C tile -- the mask-sum of the
// frame-level input dropouts (dx = sum over sites and streams of keep . dxd) folded into the launch that produces dxd.  The partial
// tile waits in LDS where the C tile of `accumulate` lies (and is that tile when both are on); the keep-bits of the tile's rows (4 KB)
// ride with the attention weights at issue point 1 (three instructions per wave again), the masked dout rows come straight into
// eight registers at issue point 5 (no LDS left for them: ring 64 + planes 24 + tile 64 + weights 2 + bits 4 + a dummy row 1 = 159 KB).
constexpr int G_OPS = 7;      // (fold: at most 7 queries -- k = 7 of a slot is a zero)
constexpr int LDS_FOLD = RING + 2 * PL_STAGE + C_TILE + POOL_W + BITS_TILE + DN * 4;
static_assert(LDS_FOLD <= 160 * 1024, "LDS of the folding variant");
// the ledger: the keep-bits ahead of the A piece of point 0; the pool operands and the C tile behind that of point 1, the masked dout
// rows behind that of point 5; the wait in stage s is for the A piece of stage s + 2
enum { S_BITS, S_POOL, S_G, S_C };
template <bool MASK, bool ACC, bool POOL = false, bool FOLD = false>
constexpr Ledger split = {PF2, 2, {{BITS_OPS, at(MASK, 0), true}, {P_OPS, at(POOL, 1)}, {G_OPS, at(FOLD, 5)}, {C_OPS, at(ACC, 1)}}};
static_assert(younger(split<false, true, true, true>, 7) == 11 && younger(split<false, true, true, true>, 6) == 22 && younger(split<false, false, true, true>, 2) == 14,
              "fold: 3 + 8 (+ 8) loads behind the piece of issue point 1, 8 behind the piece of issue point 5");
static_assert(younger(split<false, false>, 0) == 4 && younger(split<false, false>, 7) == 4, "plain: four issue points of one piece");
static_assert(younger(split<false, false, true>, 7) == 4 && younger(split<false, false, true>, 6) == 7 && younger(split<false, false, true>, 2) == 7 && younger(split<false, false, true>, 1) == 4,
              "pool: the three loads are behind the piece of issue point 1 (waited for in stage 6) and ahead of every later piece");
static_assert(POOL_W + POOL_G <= (C_TILE > 2 * BITS_TILE ? C_TILE : 2 * BITS_TILE), "the pool operands fit where the C tile would lie");
}  // namespace sp

template <bool MASK, bool ACC, bool POOL = false, bool FOLD = false>
__global__ __launch_bounds__(NTHR, 2) void gr_split_kernel(const Launch L) {
  static_assert(!FOLD || (POOL && !MASK), "the folding variant carries the pooling term");
#if defined(__HIP_DEVICE_COMPILE__)
  using namespace sp;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int n0 = wave * 32;
  const int U = L.unit0[L.n];
  int u = (int)(((uint32_t)blockIdx.x * (uint32_t)U) / (uint32_t)L.nwg);
  const int u_end = (int)((((uint32_t)blockIdx.x + 1u) * (uint32_t)U) / (uint32_t)L.nwg);

  typedef float f32x4_ __attribute__((ext_vector_type(4)));
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

  // conversion: this lane's chunk of a raw stage = row cr, k 4 cg .. 4 cg + 3
  const int cq = (wave << 6) + lane, cr = cq >> 3, cg = cq & 7;
  const uint32_t raw_off = (uint32_t)(cr * (BK * 4) + ((cg ^ (cr & 7)) << 4));
  const uint32_t pl_woff = (uint32_t)(cr * (BK * 2) + ((((cg >> 1) ^ ((cr >> 2) & 3)) << 4) | ((cg & 1) << 3)));
  const uint32_t cbit_off = (uint32_t)(cr * QW + cg);
  // operand reads: rows 32 i + li, plane chunk 2 h + lh
  uint32_t pl_roff[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = 32 * i + li;
      pl_roff[i][h] = (uint32_t)(row * (BK * 2) + (((2 * h + lh) ^ ((row >> 2) & 3)) << 4));
    }
  // LDS-DMA: this wave's piece of a stage = rows 8 wave .. + 7; lane -> row 8 wave + lane / 8, LDS chunk lane % 8
  const int dr = 8 * wave + (lane >> 3);
  const uint32_t dq16 = (uint32_t)(((lane & 7) ^ (lane >> 3)) << 4);
  char* const planes = lds + RING;
  char* const bits_lds = planes + 2 * PL_STAGE;       // MASK: the keep-bits of two tiles; ACC: the C tile
  char* const c_lds = bits_lds;
  // FOLD: [C / partial tile 64 KB][attention weights 2 KB][keep-bits 4 KB][dummy row 1 KB]; POOL alone: [weights 2 KB][dout rows 16 KB]
  char* const pw_lds = FOLD ? c_lds + C_TILE : bits_lds;
  char* const cb_lds = pw_lds + POOL_W;
  // (the dummy row: c_lds + C_TILE + POOL_W + BITS_TILE)

  f32x16 acc[2];

  while (u < u_end) {
    int p = 0;
    while (p + 1 < L.n && L.unit0[p + 1] <= u) ++p;
    const sdumc_rows_problem& pr = L.p[p];
    const int ub = min(u_end, L.unit0[p + 1]);
    const int tile0 = L.unit0[p];
    const uint32_t lda4 = (uint32_t)pr.lda * 4u, ldc4 = (uint32_t)pr.ldc * 4u;
    const int a_rows = pr.a_row_mod > 0 ? pr.a_row_mod : pr.M;
    // FOLD: unit w of the problem = (output tile w / fold, row block w % fold); R = rows of C = rows of one block
    const int fold = FOLD ? pr.fold : 1;
    const int R = FOLD ? pr.M / fold : pr.M;
    const bool cmask = FOLD && pr.c_bits != nullptr;
    const float cscale = cmask ? pr.c_scale : 1.f;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pr.A), 0, (int)((uint32_t)a_rows * lda4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rbits = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(MASK ? pr.a_bits : (cmask ? pr.c_bits : (const uint8_t*)pr.A)), 0,
                                                                           (MASK || cmask) ? (int)((uint32_t)pr.M * QW) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(pr.C, 0, (int)((uint32_t)R * ldc4), 0x00020000);
    auto blk_of = [&](int w) -> int { return fold == 2 ? (w & 1) : 0; };
    auto tile_of = [&](int w) -> int { return fold == 2 ? (w >> 1) : w; };
    auto vrow0 = [&](int w) -> uint32_t { return (uint32_t)(blk_of(w) * R + tile_of(w) * BM); };      // first (virtual) row of unit w
    const int pnq = POOL ? pr.pool_nq : 0, pT = POOL ? pr.pool_T : 1;
    const __amdgpu_buffer_rsrc_t rpw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(POOL ? pr.pool_w : pr.A), 0,
                                                                         POOL ? (int)((uint32_t)pr.M * (uint32_t)pnq * 4u) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rpg = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(POOL ? pr.pool_g : pr.A), 0,
                                                                         POOL ? (int)((uint32_t)(pr.M / pT) * (uint32_t)pnq * (DN * 4u)) : 0, 0x00020000);

    // B: register j = 16 s + 8 h + e  <->  k = 32 s + 16 h + 8 lh + e
    float breg[DK / 2];
    {
      const uint32_t ldb4 = (uint32_t)pr.ldb * 4u;
      const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pr.B), 0, (int)((uint32_t)DK * ldb4), 0x00020000);
      const uint32_t bo = (uint32_t)(8 * lh) * ldb4 + (uint32_t)(n0 + li) * 4u;
#pragma unroll
      for (int j = 0; j < DK / 2; ++j)
        breg[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rb, bo, (32 * (j >> 4) + 16 * ((j >> 3) & 1) + (j & 7)) * ldb4, 0));
    }
    const float bias = pr.bias ? pr.bias[n0 + li] : 0.f;
    const float scale = MASK ? pr.a_scale : 1.f;
    const bool do_tanh = pr.act == SDUMC_ACT_TANH;

    auto a_off = [&](int w) -> uint32_t {      // (w: unit of this problem)
      int r = (int)vrow0(w) + dr;
      if (pr.a_row_mod > 0) r %= pr.a_row_mod;
      return (uint32_t)r * lda4 + dq16;
    };
    auto bits_off = [&](int w) -> uint32_t { return (vrow0(w) + 8u * (uint32_t)wave) * QW + 4u * lane; };
    auto issue_a = [&](uint32_t off, int chunk) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void_t*)(lds + chunk * A_STAGE + wave * 1024), 16, off, chunk * (BK * 4), 0, 0);
    };
    auto issue_bits = [&](uint32_t off, int par) {
      static_assert(BITS_OPS == 2, "the two instructions below");
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rbits, (lds_void_t*)(bits_lds + par * BITS_TILE + wave * 512), 4, off, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rbits, (lds_void_t*)(bits_lds + par * BITS_TILE + wave * 512 + 256), 4, off, 256, 0, 0);
    };
    // POOL: wave w brings 256 bytes of the tile's attention weights (rows r0 .. r0 + 63, pnq floats each: contiguous) and row w of
    // both samples' masked dout ([slot][8][256] in LDS; rows >= pnq and samples past the last one: outside the descriptor, zeros)
    auto issue_pool = [&](int w) {
      static_assert(P_OPS == 3, "the weights, then two keep-bits pieces (FOLD) or the two samples' dout rows");
      const uint32_t r0 = vrow0(w), v0 = r0 / (uint32_t)pT;
      const uint32_t wb = 256u * (uint32_t)wave + 4u * (uint32_t)lane;
      const uint32_t woff = wb < (uint32_t)(BM * pnq * 4) ? r0 * (uint32_t)pnq * 4u + wb : SDUMC_GR_NULL_OFF;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rpw, (lds_void_t*)(pw_lds + wave * 256), 4, woff, 0, 0, 0);
      if constexpr (FOLD) {      // the keep-bits of the unit's 64 rows (all-zero rows past the end; unused without c_bits)
        // (the uniform part of the address in the scalar offset: no lane-dependent offset register lives across the stages)
        const uint32_t bs = cmask ? (r0 + 8u * (uint32_t)wave) * QW : SDUMC_GR_NULL_OFF;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rbits, (lds_void_t*)(cb_lds + wave * 512), 4, 4u * (uint32_t)lane, bs, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rbits, (lds_void_t*)(cb_lds + wave * 512 + 256), 4, 4u * (uint32_t)lane, bs + 256u, 0, 0);      // (an immediate offset would move the LDS address too)
        return;
      }
#pragma unroll
      for (int slot = 0; slot < 2; ++slot) {
        const uint32_t goff = wave < pnq ? ((v0 + slot) * (uint32_t)pnq + (uint32_t)wave) * (DN * 4u) + 16u * (uint32_t)lane : SDUMC_GR_NULL_OFF;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rpg, (lds_void_t*)(bits_lds + POOL_W + (slot * 8 + wave) * (DN * 4)), 16, goff, 0, 0, 0);
      }
    };
    // raw stage `slot` (keep-bits parity `par`) -> planes buffer `pb`
    auto convert = [&](int slot, int par, int pb) {
      f32x4_ v = *reinterpret_cast<const f32x4_*>(lds + slot * A_STAGE + raw_off);
      if constexpr (MASK) {
        const uint32_t b = *reinterpret_cast<const uint8_t*>(bits_lds + par * BITS_TILE + cbit_off + 8 * slot);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __uint_as_float(__float_as_uint(v[e]) & (uint32_t)__builtin_amdgcn_sbfe((int)b, e, 1u));
      }
      uint32_t q[3][2];
      split_bf16x3(v[0], v[1], q[0][0], q[1][0], q[2][0]);
      split_bf16x3(v[2], v[3], q[0][1], q[1][1], q[2][1]);
      char* dst = planes + pb * PL_STAGE + pl_woff;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
        const u32x2 w = {q[pl][0], q[pl][1]};
        *reinterpret_cast<u32x2*>(dst + pl * (BM * BK * 2)) = w;
      }
    };
    // the three parts of the 8 B values of half h of stage s (registers 16 s + 8 h .. + 7)
    struct Parts {
      u32x4 p[3];
    };
    auto bsplit = [&](int s, int h, Parts& o) {
      uint32_t bq[3][4];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        // (the parts of B do not change from tile to tile, and the compiler would hoist all 192 registers of them out of the
        //  tile loop and spill: an empty asm makes the two values opaque here)
        float x = breg[16 * s + 8 * h + 2 * d], y = breg[16 * s + 8 * h + 2 * d + 1];
        asm volatile("" : "+v"(x), "+v"(y));
        split_bf16x3(x, y, bq[0][d], bq[1][d], bq[2][d]);
      }
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) o.p[pl] = u32x4{bq[pl][0], bq[pl][1], bq[pl][2], bq[pl][3]};
    };
    auto read_a = [&](int pb, int i, int h, Parts& o) {
      const char* base = planes + pb * PL_STAGE + pl_roff[i][h];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) o.p[pl] = *reinterpret_cast<const u32x4*>(base + pl * (BM * BK * 2));
    };
    auto mma6 = [&](int i, const Parts& a, const Parts& bb) { mfma_bf16x3(acc[i], a.p, bb.p); };

    // ---- prologue: the ring belongs to this problem from here (the previous one drained it) ----
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    int par = 0;
    int w = (u - tile0) * fold;                    // this workgroup's units of the problem: [w, w_end)
    const int w_end = (ub - tile0) * fold;
    {
      const uint32_t o = a_off(w);
      if constexpr (MASK) issue_bits(bits_off(w), 0);
#pragma unroll
      for (int s = 0; s < PF2; ++s) issue_a(o, s);
    }
    __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
    __builtin_amdgcn_s_barrier();
    convert(0, 0, 0);
    __builtin_amdgcn_s_barrier();
    Parts bh0;
    bsplit(0, 0, bh0);

    // ---- steady state: 8 stages per tile, one barrier per stage ----
#pragma nounroll
    for (; w < w_end; ++w) {
      const uint32_t o_cur = a_off(w);
      const uint32_t o_nxt = w + 1 < w_end ? a_off(w + 1) : SDUMC_GR_NULL_OFF;
      const uint32_t b_nxt = w + 1 < w_end ? bits_off(w + 1) : SDUMC_GR_NULL_OFF;
      const int to = tile_of(w);
      const bool first = blk_of(w) == 0, last = blk_of(w) == fold - 1;      // FOLD: the unit opens / closes its output tile
      const uint32_t c_off = (uint32_t)(to * BM + 4 * lh) * ldc4 + (uint32_t)(n0 + li) * 4u;
      const uint32_t c_row0 = (uint32_t)(to * BM + 8 * wave) * ldc4 + 16u * (uint32_t)lane;
      float gq[8];      // FOLD: this lane's masked dout values G[v0 + lh][j][n0 + li] (issue point 5)
      auto stage = [&](auto sc) {
        constexpr int s = decltype(sc)::value;
        constexpr const Ledger& G = split<MASK, ACC, POOL, FOLD>;
        // raw stage s + 1 (published by the previous barrier) -> the other planes buffer; stage 8 = the next tile's first
        convert((s + 1) % NS, s + 1 == NS ? par ^ 1 : par, (s + 1) & 1);
        // four blocks of six MFMAs: (h, i) = (0, 0), (0, 1), (1, 0), (1, 1).  The A parts of the next block are read and the B
        // parts of the next half are split while a block multiplies; bh0 (the B parts of this stage's first half) was made in
        // the previous stage's last block.
        Parts a0, a1, bh1;
        read_a(s & 1, 0, 0, a0);
        __builtin_amdgcn_sched_barrier(0);
        read_a(s & 1, 1, 0, a1);
        bsplit(s, 1, bh1);
        mma6(0, a0, bh0);
        __builtin_amdgcn_sched_barrier(0);
        read_a(s & 1, 0, 1, a0);
        mma6(1, a1, bh0);
        __builtin_amdgcn_sched_barrier(0);
        read_a(s & 1, 1, 1, a1);
        bsplit((s + 1) % NS, 0, bh0);
        mma6(0, a0, bh1);
        __builtin_amdgcn_sched_barrier(0);
        mma6(1, a1, bh1);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(waitcnt_vm(younger(G, s)));
        __builtin_amdgcn_s_barrier();
        if constexpr (MASK) {      // (the outer conditions keep what a variant lacks out of the lambda's captures)
          if constexpr (carries(G.pc[S_BITS], s)) issue_bits(b_nxt, par ^ 1);
        }
        issue_a(s + PF2 < NS ? o_cur : o_nxt, (s + PF2) % NS);
        if constexpr (POOL) {
          if constexpr (carries(G.pc[S_POOL], s)) issue_pool(w);
        }
        if constexpr (FOLD) {
          if constexpr (carries(G.pc[S_G], s)) {
            const uint32_t v0 = vrow0(w) / (uint32_t)pT;
            const uint32_t gv = (uint32_t)lh * (uint32_t)pnq * (DN * 4u) + (uint32_t)(n0 + li) * 4u;
#pragma unroll
            for (int j = 0; j < G_OPS; ++j)
              gq[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rpg, gv, j < pnq ? (v0 * (uint32_t)pnq + (uint32_t)j) * (DN * 4u) : SDUMC_GR_NULL_OFF, 0));
            gq[7] = 0.f;
          }
        }
        if constexpr (ACC) {
          if constexpr (carries(G.pc[S_C], s)) {   // this wave's rows 8 wave .. + 7 of the C tile (rows past M: outside the descriptor, zeros)
            // (FOLD: only the unit that opens the tile fetches it; the others send their eight loads, from nowhere, to a dummy row --
            //  the queue of every unit holds the same operations)
            const bool real = !FOLD || first;
#pragma unroll
            for (int j = 0; j < C_OPS; ++j)
              __builtin_amdgcn_raw_ptr_buffer_load_lds(rc, (lds_void_t*)(c_lds + (real ? (8 * wave + j) * (DN * 4) : C_TILE + POOL_W + BITS_TILE)), 16,
                                                       real ? c_row0 + (uint32_t)j * ldc4 : SDUMC_GR_NULL_OFF, 0, 0, 0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      };
      stage(std::integral_constant<int, 0>{});
      stage(std::integral_constant<int, 1>{});
      stage(std::integral_constant<int, 2>{});
      stage(std::integral_constant<int, 3>{});
      stage(std::integral_constant<int, 4>{});
      stage(std::integral_constant<int, 5>{});
      stage(std::integral_constant<int, 6>{});
      stage(std::integral_constant<int, 7>{});
      if constexpr (POOL) {      // the extra k-tile: k = 8 slot + j  <->  (sample v0 + slot, query j); a row multiplies its own sample's slot only
        const uint32_t r0 = vrow0(w), v0 = r0 / (uint32_t)pT;
        const int rb = (int)((v0 + 1u) * (uint32_t)pT - r0);                 // first row of the tile that belongs to sample v0 + 1
        const float* wl = reinterpret_cast<const float*>(pw_lds);
        const float* gl = reinterpret_cast<const float*>(bits_lds + POOL_W) + lh * (8 * DN) + n0 + li;
        Parts pb_, pa_;
        {
          float g[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) g[j] = FOLD ? gq[j] : gl[j * DN];
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            uint32_t q0, q1, q2;
            split_bf16x3(g[2 * d], g[2 * d + 1], q0, q1, q2);
            pb_.p[0][d] = q0; pb_.p[1][d] = q1; pb_.p[2][d] = q2;
          }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int row = 32 * i + li;
          const bool mine = (row >= rb ? 1 : 0) == lh;
          float w[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) w[j] = (mine && j < pnq) ? wl[row * pnq + j] : 0.f;
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            uint32_t q0, q1, q2;
            split_bf16x3(w[2 * d], w[2 * d + 1], q0, q1, q2);
            pa_.p[0][d] = q0; pa_.p[1][d] = q1; pa_.p[2][d] = q2;
          }
          mma6(i, pa_, pb_);
        }
      }
      if constexpr (FOLD) {      // keep . (A B + pooling term) * scale, summed over the tile's row blocks in LDS; the closing unit stores
        // (one lane-dependent base per array, the element's row as an immediate offset; the uniform conditions select one of eight
        //  straight-line bodies -- per-element address registers spilled, and a spill reload waits for the whole load queue)
        const uint8_t* cb = reinterpret_cast<const uint8_t*>(cb_lds) + 8 * wave + (li >> 2) + 4 * lh * QW;
        char* cl = c_lds + (4 * lh) * (DN * 4) + (n0 + li) * 4;
        const uint32_t sh = (uint32_t)(li & 3);
        auto body = [&](auto cm, auto ap, auto la) {
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int eb = 0; eb < 16; eb += 8) {      // eight elements at a time: their LDS reads first, in one batch (element by element they serialise)
              uint32_t kb[8];
              float pv[8];
#pragma unroll
              for (int q = 0; q < 8; ++q) {
                const int e = eb + q, rc_ = 32 * i + (e & 3) + 8 * (e >> 2);      // the element's row without the lane's 4 lh
                if constexpr (decltype(cm)::value) kb[q] = cb[rc_ * QW];
                if constexpr (decltype(ap)::value) pv[q] = *reinterpret_cast<const float*>(cl + rc_ * (DN * 4));
              }
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int q = 0; q < 8; ++q) {
                const int e = eb + q, rc_ = 32 * i + (e & 3) + 8 * (e >> 2);
                float v = acc[i][e];
                if constexpr (decltype(cm)::value) v = ((kb[q] >> sh) & 1u) ? v * cscale : 0.f;
                if constexpr (decltype(ap)::value) v += pv[q];
                if constexpr (decltype(la)::value) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rc, c_off, rc_ * ldc4, 0);
                else *reinterpret_cast<float*>(cl + rc_ * (DN * 4)) = v;
                acc[i][e] = 0.f;
              }
              __builtin_amdgcn_sched_barrier(0);
            }
        };
        const bool ap = ACC || !first;
        using T_ = std::true_type;
        using F_ = std::false_type;
        if (cmask) {
          if (ap) { if (last) body(T_{}, T_{}, T_{}); else body(T_{}, T_{}, F_{}); }
          else { if (last) body(T_{}, F_{}, T_{}); else body(T_{}, F_{}, F_{}); }
        } else {
          if (ap) { if (last) body(F_{}, T_{}, T_{}); else body(F_{}, T_{}, F_{}); }
          else { if (last) body(F_{}, F_{}, T_{}); else body(F_{}, F_{}, F_{}); }
        }
      }
      auto epilogue = [&](auto tanh_c) {
        if constexpr (FOLD) return;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            float v = acc[i][e];
            if constexpr (MASK) v *= scale;
            v += bias;
            if constexpr (ACC) v += *reinterpret_cast<const float*>(c_lds + (32 * i + (e & 3) + 8 * (e >> 2) + 4 * lh) * (DN * 4) + (n0 + li) * 4);
            if constexpr (decltype(tanh_c)::value) v = fast_tanh(v);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rc, c_off, (32 * i + (e & 3) + 8 * (e >> 2)) * ldc4, 0);
            acc[i][e] = 0.f;
          }
      };
      if (do_tanh) epilogue(std::true_type{});
      else epilogue(std::false_type{});
      __builtin_amdgcn_sched_barrier(0);
      par ^= 1;
    }
    u = ub;
    __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
    __builtin_amdgcn_s_barrier();
  }
#endif
}

// ------------------------------------------------------------------------------------------------------------------------
// The same launch on bf16 STORAGE (the engine's bf16 mode, BASELINE configs[2] / [4]): A ([M][256], the masked frames xd or dz),
// B ([256 n][256 k]: the weight copy whose rows are the output columns) and C are bf16 tensors, products accumulate in fp32 on
// v_mfma_f32_32x32x16_bf16, bias / tanh in fp32.  A row of a stage is 64 k = 128 bytes, so the ring slots, the swizzle, the
// DMA pieces and the fragment reads are those of the fp32 kernel; a tile is 4 stages, the 8-slot ring holds two, and the
// unrolled body works through a PAIR of tiles.  B is 64 VGPRs per wave.  At bf16 matrix rates a 64-row tile multiplies in
// under a microsecond: the kernel is bound by its streams (A in, C out, C in for the accumulate) -- what the persistent ring
// buys here is 48 KB per CU in flight all the time instead of one short k-loop per workgroup.
// ------------------------------------------------------------------------------------------------------------------------
namespace hf {
#define SDUMC_GR_HNS 4                            /* stages per tile (64 k each) */
// FOLD (1 or 2 = sdumc_rows_problem.fold, one value per launch): the pooling term as one more k-tile (split arithmetic: its operands are
// fp32) and the mask-sum of the input dropouts, as in gr_split_kernel.  A unit's operands -- 64 rows of attention weights (2 KB), the
// masked dout rows of its <= 2 samples (16 KB), its keep-bits (4 KB) -- ride in by LDS-DMA six stages before the unit's last one:
// at issue point 5 for the first unit of the NEXT pair, at issue point 1 for the second unit of this one (five instructions per
// wave; one LDS buffer per unit of the pair).  FOLD = 2: the pair IS one output tile -- its first unit opens the running sum (the C
// prefetch registers; with `accumulate` they start from C), its second closes and stores it: no C prefetch at issue point 5.
constexpr int HP_OPS = 5;
constexpr int HP_W = BM * 8 * 4, HP_G = 2 * 8 * DN * 4, HP_BUF = HP_W + HP_G + BITS_TILE;
// the ledger, over the pair's 8 issue points: the C prefetch of tile 0 behind the A piece of point 1, of tile 1 behind that of point 5;
// the pool operands behind both
enum { H_C, H_POOL };
template <bool ACC, int FOLD = 0>
constexpr Ledger pair = {PF, 1, {{CPRE_OPS, at(ACC, 1) | at(ACC && FOLD != 2, 5)}, {HP_OPS, at(FOLD != 0, 1) | at(FOLD != 0, 5)}}};
static_assert(younger(pair<false, 1>, 0) == 4 + HP_OPS && younger(pair<false, 2>, 2) == 4 + 2 * HP_OPS && younger(pair<true, 2>, 2) == 4 + 2 * HP_OPS + 32, "bf16 fold");
}  // namespace hf

// (stage 0..7 of a pair: plain 4 x 8; accumulating 36 36 68 36 36 36 68 36 -- 68 = both C prefetches were issued behind the A piece)
static_assert(younger(hf::pair<false>, 0) == 4 && younger(hf::pair<true>, 0) == 36 && younger(hf::pair<true>, 1) == 36 && younger(hf::pair<true>, 2) == 68 &&
              younger(hf::pair<true>, 3) == 36 && younger(hf::pair<true>, 6) == 68 && younger(hf::pair<true>, 7) == 36, "bf16 pair: C prefetch at stages 1 and 5");

template <bool ACC, int FOLD = 0>
__global__ __launch_bounds__(NTHR, 2) void gr_bf16_kernel(const Launch L) {
#if defined(__HIP_DEVICE_COMPILE__)
  using namespace hf;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int n0 = wave * 32;
  const int U = L.unit0[L.n];
  int u = (int)(((uint32_t)blockIdx.x * (uint32_t)U) / (uint32_t)L.nwg);
  const int u_end = (int)((((uint32_t)blockIdx.x + 1u) * (uint32_t)U) / (uint32_t)L.nwg);
  uint32_t foff[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) foff[c] = (uint32_t)(li * 128 + (((2 * c + lh) ^ (li & 7)) << 4));
  const int dr = 8 * wave + (lane >> 3);
  const uint32_t dq16 = (uint32_t)(((lane & 7) ^ (lane >> 3)) << 4);
  typedef float f32x4_ __attribute__((ext_vector_type(4)));
  f32x16 acc[2];

  while (u < u_end) {
    int p = 0;
    while (p + 1 < L.n && L.unit0[p + 1] <= u) ++p;
    const sdumc_rows_problem& pr = L.p[p];
    const int ub = min(u_end, L.unit0[p + 1]);
    const int tile0 = L.unit0[p];
    const uint32_t lda2 = (uint32_t)pr.lda * 2u, ldc2 = (uint32_t)pr.ldc * 2u;
    const int a_rows = pr.a_row_mod > 0 ? pr.a_row_mod : pr.M;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pr.A), 0, (int)((uint32_t)a_rows * lda2), 0x00020000);
    // FOLD: unit w of the problem = (output tile w / FOLD, row block w % FOLD); R = rows of C = rows of one block
    const int R = FOLD ? pr.M / (FOLD > 0 ? FOLD : 1) : pr.M;
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(pr.C, 0, (int)((uint32_t)R * ldc2), 0x00020000);
    const bool cmask = FOLD && pr.c_bits != nullptr;
    const float cscale = cmask ? pr.c_scale : 1.f;
    const int pnq = FOLD ? pr.pool_nq : 0, pT = FOLD ? pr.pool_T : 1;
    const __amdgpu_buffer_rsrc_t rbits = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(cmask ? pr.c_bits : (const uint8_t*)pr.A), 0,
                                                                           cmask ? (int)((uint32_t)pr.M * QW) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rpw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(FOLD ? pr.pool_w : pr.A), 0,
                                                                         FOLD ? (int)((uint32_t)pr.M * (uint32_t)pnq * 4u) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rpg = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(FOLD ? pr.pool_g : pr.A), 0,
                                                                         FOLD ? (int)((uint32_t)(pr.M / pT) * (uint32_t)pnq * (DN * 4u)) : 0, 0x00020000);
    // B: the MFMA operand of step j = 4 s + c is k = 64 s + 16 c + 8 lh .. + 7 of row n0 + li: one 16-byte load
    bf16x8 breg[16];
    {
      const uint32_t ldb2 = (uint32_t)pr.ldb * 2u;
      const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pr.B), 0, (int)((uint32_t)DN * ldb2), 0x00020000);
      const uint32_t bo = (uint32_t)(n0 + li) * ldb2 + 16u * (uint32_t)lh;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rb, bo, 32 * j, 0);
        breg[j] = *reinterpret_cast<const bf16x8*>(&v);
      }
    }
    const float bias = pr.bias ? pr.bias[n0 + li] : 0.f;
    const bool do_tanh = pr.act == SDUMC_ACT_TANH;

    // (t: unit of the launch for FOLD = 0 -- a tile -- and unit of this problem for FOLD > 0; t_end: the end of this workgroup's run)
    const int t_end = FOLD ? (ub - tile0) * FOLD : ub;
    auto vrow0 = [&](int t) -> uint32_t {      // first (virtual) row of unit t
      if constexpr (FOLD == 2) return (uint32_t)((t & 1) * R + (t >> 1) * BM);
      else if constexpr (FOLD == 1) return (uint32_t)(t * BM);
      else return (uint32_t)((t - tile0) * BM);
    };
    auto a_off = [&](int t) -> uint32_t {      // tiles at and past the end of this workgroup's run of the problem: nothing
      if (t >= t_end) return SDUMC_GR_NULL_OFF;
      int r = (int)vrow0(t) + dr;
      if (pr.a_row_mod > 0) r %= pr.a_row_mod;
      return (uint32_t)r * lda2 + dq16;
    };
    auto c_off_of = [&](int t) -> uint32_t {
      if (t >= t_end) return SDUMC_GR_NULL_OFF;
      const int row0 = FOLD == 2 ? (t >> 1) * BM : (FOLD == 1 ? t * BM : (t - tile0) * BM);
      return (uint32_t)(row0 + 4 * lh) * ldc2 + (uint32_t)(n0 + li) * 2u;
    };
    // FOLD: the operands of unit t's extra k-tile and its keep-bits -> LDS buffer `buf` (past the run's end: from nowhere, zeros)
    char* const pool_lds = lds + RING;
    auto issue_pool = [&](int t, int buf) {
      static_assert(HP_OPS == 1 + 2 + 2, "the weights, the two samples' dout rows, two keep-bits pieces");
      char* base = pool_lds + buf * HP_BUF;
      const bool live = t < t_end;
      const uint32_t r0 = live ? vrow0(t) : 0u, v0 = r0 / (uint32_t)pT;
      const uint32_t wb = 256u * (uint32_t)wave + 4u * (uint32_t)lane;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rpw, (lds_void_t*)(base + wave * 256), 4,
                                               (live && wb < (uint32_t)(BM * pnq * 4)) ? r0 * (uint32_t)pnq * 4u + wb : SDUMC_GR_NULL_OFF, 0, 0, 0);
#pragma unroll
      for (int slot = 0; slot < 2; ++slot)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rpg, (lds_void_t*)(base + HP_W + (slot * 8 + wave) * (DN * 4)), 16,
                                                 (live && wave < pnq) ? ((v0 + slot) * (uint32_t)pnq + (uint32_t)wave) * (DN * 4u) + 16u * (uint32_t)lane : SDUMC_GR_NULL_OFF,
                                                 0, 0, 0);
      const uint32_t bo = (live && cmask) ? (r0 + 8u * (uint32_t)wave) * QW + 4u * (uint32_t)lane : SDUMC_GR_NULL_OFF;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rbits, (lds_void_t*)(base + HP_W + HP_G + wave * 512), 4, bo, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rbits, (lds_void_t*)(base + HP_W + HP_G + wave * 512 + 256), 4, bo, 256, 0, 0);
    };
    auto issue_a = [&](uint32_t off, int chunk, int slot) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void_t*)(lds + slot * A_STAGE + wave * 1024), 16, off, chunk * 128, 0, 0);
    };
    struct Frag {
      f32x4_ a[2][2];
    };
    auto read_frag = [&](int slot, int h, Frag& f) {
      const char* base = lds + slot * A_STAGE;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) f.a[i][cc] = *reinterpret_cast<const f32x4_*>(base + i * (32 * 128) + foff[2 * h + cc]);
    };
    auto mma = [&](Frag& f, int h, int s4) {
#pragma unroll
      for (int cc = 0; cc < 2; ++cc)
#pragma unroll
        for (int i = 0; i < 2; ++i)
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&f.a[i][cc]), breg[4 * s4 + 2 * h + cc], acc[i], 0, 0, 0);
    };

#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    int w = FOLD ? (u - tile0) * FOLD : u;      // the unit counter of the loop below
    {
      const uint32_t o0 = a_off(w), o1 = a_off(w + 1);
#pragma unroll
      for (int s = 0; s < PF; ++s) issue_a(s < SDUMC_GR_HNS ? o0 : o1, s % SDUMC_GR_HNS, s);
      if constexpr (FOLD) issue_pool(w, 0);
    }
    __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
    __builtin_amdgcn_s_barrier();
    Frag fa, fb;
    read_frag(0, 0, fa);

#pragma nounroll
    for (; w < t_end; w += 2) {
      const uint32_t o[4] = {a_off(w), a_off(w + 1), a_off(w + 2), a_off(w + 3)};
      const uint32_t co[2] = {c_off_of(w), c_off_of(w + 1)};
      float cpre[(ACC || FOLD == 2) ? 32 : 1];
      // FOLD: the extra k-tile of unit w + U (k = 8 slot + j  <->  sample v0 + slot, query j; a row multiplies its own sample's slot only),
      // then keep . (...) * scale into the running sum / out to C
      auto fold_tail = [&](auto uc) {
        constexpr int U = decltype(uc)::value;
        auto split8 = [&](const float (&x)[8], u32x4 (&pp)[3]) {
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            uint32_t p0, p1, p2;
            split_bf16x3(x[2 * d], x[2 * d + 1], p0, p1, p2);
            pp[0][d] = p0; pp[1][d] = p1; pp[2][d] = p2;
          }
        };
        const char* base = pool_lds + U * HP_BUF;
        const uint32_t r0 = vrow0(w + U), v0 = r0 / (uint32_t)pT;
        const int rb = (int)((v0 + 1u) * (uint32_t)pT - r0);                 // first row of the unit that belongs to sample v0 + 1
        const float* wl = reinterpret_cast<const float*>(base);
        const float* gl = reinterpret_cast<const float*>(base + HP_W) + lh * (8 * DN) + n0 + li;
        u32x4 pb_[3], pa_[3];
        {
          float g[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) g[j] = gl[j * DN];
          split8(g, pb_);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int row = 32 * i + li;
          const bool mine = (row >= rb ? 1 : 0) == lh;
          float x[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] = (mine && j < pnq) ? wl[row * pnq + j] : 0.f;
          split8(x, pa_);
          mfma_bf16x3(acc[i], pa_, pb_);
        }
        const uint8_t* cb = reinterpret_cast<const uint8_t*>(base + HP_W + HP_G) + 8 * wave + (li >> 2) + 4 * lh * QW;
        const uint32_t sh = (uint32_t)(li & 3);
        const uint32_t c_off = co[U];
        constexpr bool opens = FOLD == 1 || U == 0, closes = FOLD == 1 || U == 1;
        auto run = [&](auto cm) {
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int eb = 0; eb < 16; eb += 8) {
              uint32_t kb[8];
#pragma unroll
              for (int q = 0; q < 8; ++q) {
                const int e = eb + q;
                if constexpr (decltype(cm)::value) kb[q] = cb[(32 * i + (e & 3) + 8 * (e >> 2)) * QW];
              }
#pragma unroll
              for (int q = 0; q < 8; ++q) {
                const int e = eb + q;
                float v = acc[i][e];
                if constexpr (decltype(cm)::value) v = ((kb[q] >> sh) & 1u) ? v * cscale : 0.f;
                if constexpr (ACC || !opens) v += cpre[i * 16 + e];
                if constexpr (closes) __builtin_amdgcn_raw_buffer_store_b16(f2bf(v), rc, c_off, (32 * i + (e & 3) + 8 * (e >> 2)) * ldc2, 0);
                else cpre[i * 16 + e] = v;
                acc[i][e] = 0.f;
              }
            }
        };
        if (cmask) run(std::true_type{});
        else run(std::false_type{});
      };
      auto epilogue = [&](uint32_t c_off, auto tanh_c) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            float v = acc[i][e] + bias;
            if constexpr (ACC) v += cpre[i * 16 + e];
            if constexpr (decltype(tanh_c)::value) v = fast_tanh(v);
            __builtin_amdgcn_raw_buffer_store_b16(f2bf(v), rc, c_off, (32 * i + (e & 3) + 8 * (e >> 2)) * ldc2, 0);
            acc[i][e] = 0.f;
          }
      };
      auto stage = [&](auto sc) {
        constexpr int s = decltype(sc)::value;        // stage of the pair: tile s / 4, its stage s % 4; ring slot s
        constexpr const Ledger& G = pair<ACC, FOLD>;
        read_frag(s, 1, fb);
        __builtin_amdgcn_sched_barrier(0);
        mma(fa, 0, s % SDUMC_GR_HNS);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(waitcnt_vm(younger(G, s)));
        __builtin_amdgcn_s_barrier();
        issue_a(o[(s + PF) / SDUMC_GR_HNS], (s + PF) % SDUMC_GR_HNS, (s + PF) % NS);
        if constexpr (ACC) {      // (the outer conditions keep what a variant lacks out of the lambda's captures)
          if constexpr (carries(G.pc[H_C], s)) {      // (of the tile this point lies in)
            static_assert(CPRE_OPS == 2 * 16, "one load per accumulator element");
            const uint32_t c_off = co[s / SDUMC_GR_HNS];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
              for (int e = 0; e < 16; ++e)
                cpre[i * 16 + e] = bf2f(__builtin_amdgcn_raw_buffer_load_b16(rc, c_off, (32 * i + (e & 3) + 8 * (e >> 2)) * ldc2, 0));
          }
        }
        if constexpr (FOLD != 0) {      // (behind the C prefetch; issue point 1: this pair's second unit into buffer 1, 5: the next pair's first into buffer 0)
          if constexpr (carries(G.pc[H_POOL], s)) issue_pool(w + 1 + s / SDUMC_GR_HNS, 1 - s / SDUMC_GR_HNS);
        }
        __builtin_amdgcn_sched_barrier(0);
        read_frag((s + 1) % NS, 0, fa);
        __builtin_amdgcn_sched_barrier(0);
        mma(fb, 1, s % SDUMC_GR_HNS);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (s % SDUMC_GR_HNS == SDUMC_GR_HNS - 1) {       // a tile is complete (the next one's stages are in flight behind its epilogue)
          if constexpr (FOLD != 0) {
            fold_tail(std::integral_constant<int, s / SDUMC_GR_HNS>{});
          } else {
            if (do_tanh) epilogue(co[s / SDUMC_GR_HNS], std::true_type{});
            else epilogue(co[s / SDUMC_GR_HNS], std::false_type{});
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      stage(std::integral_constant<int, 0>{});
      stage(std::integral_constant<int, 1>{});
      stage(std::integral_constant<int, 2>{});
      stage(std::integral_constant<int, 3>{});
      stage(std::integral_constant<int, 4>{});
      stage(std::integral_constant<int, 5>{});
      stage(std::integral_constant<int, 6>{});
      stage(std::integral_constant<int, 7>{});
    }
    u = ub;
    __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
    __builtin_amdgcn_s_barrier();
  }
#endif
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// Every instantiation, once: set_lds_attr() walks both tables and a launcher looks its variant up in one, so none is launchable
// without its attribute; a combination without a row is refused.  `fold`: the bf16 kernels are compiled per fold count; the split
// kernel reads the count from each problem, its key is fold > 0.
struct Variant {
  bool split, mask, acc, pool;
  int fold;
  void (*kernel)(const Launch);
  size_t lds;
};
constexpr size_t LDS_HF_FOLD = RING + 2 * hf::HP_BUF;
constexpr Variant F32_VARIANTS[] = {
    {false, false, false, false, 0, &gr_kernel<false, false>, LDS_BYTES},
    {false, true, false, false, 0, &gr_kernel<true, false>, LDS_BYTES},
    {false, false, true, false, 0, &gr_kernel<false, true>, LDS_BYTES},
    {true, false, false, false, 0, &gr_split_kernel<false, false>, sp::LDS_BYTES2},
    {true, true, false, false, 0, &gr_split_kernel<true, false>, sp::LDS_BYTES2},
    {true, false, true, false, 0, &gr_split_kernel<false, true>, sp::LDS_BYTES2},
    {true, false, false, true, 0, &gr_split_kernel<false, false, true>, sp::LDS_BYTES2},      // (the pooling k-tile: split arithmetic only)
    {true, false, false, true, 1, &gr_split_kernel<false, false, true, true>, sp::LDS_FOLD},
    {true, false, true, true, 1, &gr_split_kernel<false, true, true, true>, sp::LDS_FOLD},
};
constexpr Variant BF16_VARIANTS[] = {      // (no fused dropout -- the engine materialises the masked frames -- and no pooling term without the fold)
    {false, false, false, false, 0, &gr_bf16_kernel<false>, RING},
    {false, false, true, false, 0, &gr_bf16_kernel<true>, RING},
    {false, false, false, true, 1, &gr_bf16_kernel<false, 1>, LDS_HF_FOLD},
    {false, false, true, true, 1, &gr_bf16_kernel<true, 1>, LDS_HF_FOLD},
    {false, false, false, true, 2, &gr_bf16_kernel<false, 2>, LDS_HF_FOLD},
    {false, false, true, true, 2, &gr_bf16_kernel<true, 2>, LDS_HF_FOLD},
};
template <size_t N>
const Variant* find(const Variant (&table)[N], bool split, const sdumc_rows_problem& p, int fold) {
  for (const Variant& v : table)
    if (v.split == split && v.mask == (p.a_bits != nullptr) && v.acc == (p.accumulate != 0) && v.pool == (p.pool_w != nullptr) && v.fold == fold) return &v;
  return nullptr;
}

bool set_lds_attr() {   // the dynamic-LDS limit is a per-device function attribute
  static sdumc_dev_once attr_set;
  return sdumc_once_per_device(attr_set, [] {
           for (const Variant& v : F32_VARIANTS)
             if (!sdumc_set_dyn_lds(v.kernel, v.lds)) return false;
           for (const Variant& v : BF16_VARIANTS)
             if (!sdumc_set_dyn_lds(v.kernel, v.lds)) return false;
           return true;
         }) == SDUMC_OK;
}

// What differs between the problems of the two entry points; the rest of valid() is shared.
struct Form {
  int esz;                    // bytes per element of A, B and C
  int lda_mask, ldb_mask;     // fp32: lda a multiple of 4; bf16: lda and ldb multiples of 8 (16-byte rows)
  int b_align, c_align;       // bytes (A: 16 in both)
  int margin;                 // rows past M that are still addressed: two tiles, four for the bf16 kernel's pairs
  bool fold_exact;            // bf16: one fold count per launch; fp32: problems of fold 1 and 2 may share a launch
};
constexpr Form FORM_F32 = {4, 3, 0, 4, 4, 2 * BM, false}, FORM_BF16 = {2, 7, 7, 16, 2, 4 * BM, true};

bool valid(const sdumc_rows_problem& p, const Form& f, const Variant& v) {
  auto off = [](const void* q, uintptr_t align) { return (reinterpret_cast<uintptr_t>(q) & (align - 1)) != 0; };
  if (!p.A || !p.B || !p.C || p.M <= 0 || p.lda < DK || p.ldb < DN || p.ldc < DN || (p.lda & f.lda_mask) || (p.ldb & f.ldb_mask) || p.a_row_mod < 0) return false;
  if (off(p.A, 16) || off(p.B, f.b_align) || off(p.C, f.c_align) || off(p.a_bits, 4)) return false;
  if (p.act != SDUMC_ACT_NONE && p.act != SDUMC_ACT_TANH) return false;
  // 32-bit byte offsets, descriptor ranges below 2 GiB (a tile past the last row is still addressed)
  const size_t rows = (size_t)p.M + f.margin;
  if (rows * p.lda * f.esz >= 0x7FFFFFF0u || rows * p.ldc * f.esz >= 0x7FFFFFF0u) return false;
  // one kernel variant per launch
  if ((p.a_bits != nullptr) != v.mask || (p.accumulate != 0) != v.acc || (p.pool_w != nullptr) != v.pool) return false;
  if ((f.fold_exact ? p.fold : (int)(p.fold > 0)) != v.fold) return false;
  if (v.pool) {      // (fold: at most 7 queries -- k = 7 of a slot is a zero)
    if (!p.pool_g || p.pool_nq < 1 || p.pool_nq > (v.fold ? 7 : 8) || !(p.pool_T >= 63 || p.pool_T == 32) || (p.M % p.pool_T) || p.a_row_mod || p.bias || p.act != SDUMC_ACT_NONE) return false;
    if (off(p.pool_w, 4) || off(p.pool_g, 16)) return false;
  }
  if (v.fold && (p.fold > 2 || (p.M % p.fold) || ((p.M / p.fold) % p.pool_T) || off(p.c_bits, 4))) return false;
  return true;
}

// max_wg > 0: at most that many (persistent) workgroups -- a launch that should leave part of the chip to a neighbour
int launch(const sdumc_rows_problem* probs, int32_t n, int32_t max_wg, void* stream, const Form& f, const Variant* v, int prof_variant) {
  if (!v) return SDUMC_EINVAL;
  Launch L;
  memset(&L, 0, sizeof(L));
  int units = 0;
  double flops = 0.0;
  for (int i = 0; i < n; ++i) {
    const sdumc_rows_problem& p = probs[i];
    if (!valid(p, f, *v)) return SDUMC_EINVAL;
    L.p[i] = p;
    L.unit0[i] = units;
    units += ((v->fold ? p.M / p.fold : p.M) + BM - 1) / BM;      // (fold: a unit of the launch = an OUTPUT tile)
    flops += 2.0 * p.M * (double)DK * DN;
  }
  L.unit0[n] = units;
  L.n = n;
  L.nwg = std::min(sdumc_cu_count(), units);      // (bf16: a workgroup works through pairs of tiles; with fewer tiles than CUs a pair is one tile and nothing)
  if (max_wg > 0) L.nwg = std::min(L.nwg, (int)max_wg);
  if ((long long)units * (L.nwg + 1) >= (1LL << 31)) return SDUMC_EINVAL;
  if (!set_lds_attr()) return SDUMC_ELAUNCH;
  const int tok = sdumc_prof_begin_(prof_variant, flops, stream);
  hipLaunchKernelGGL(v->kernel, dim3(L.nwg), dim3(NTHR), v->lds, as_stream(stream), L);
  sdumc_prof_end_(tok, stream);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

}  // namespace sdumc_gr
using namespace sdumc_gr;

extern "C" int sdumc_gemm_rows_prepare_(void) { return set_lds_attr() ? SDUMC_OK : SDUMC_ELAUNCH; }

extern "C" int sdumc_gemm_rows256(const sdumc_rows_problem* probs, int32_t n, void* stream) {
  return sdumc_gemm_rows256_capped_(probs, n, 0, stream);
}
extern "C" int sdumc_gemm_rows256_capped_(const sdumc_rows_problem* probs, int32_t n, int32_t max_wg, void* stream) {
  if (!probs || n <= 0 || n > MAXP) return SDUMC_EINVAL;
  const bool split = sdumc_split_on_(SDUMC_SPLIT_ROWS);
  return launch(probs, n, max_wg, stream, FORM_F32, find(F32_VARIANTS, split, probs[0], probs[0].fold > 0),
                split ? SDUMC_PV_gemm_rows256_bf16x3 : SDUMC_PV_gemm_rows256);
}

// A ([M][256]), B ([256 n][256 k], row stride ldb: C = A B^T) and C are bf16 tensors (lda / ldb / ldc in elements, lda a multiple
// of 8, A 16-byte aligned); bias fp32; fp32 pool_w / pool_g with the fold
extern "C" int sdumc_gemm_rows256_bf16(const sdumc_rows_problem* probs, int32_t n, void* stream) {
  return sdumc_gemm_rows256_bf16_capped_(probs, n, 0, stream);
}
extern "C" int sdumc_gemm_rows256_bf16_capped_(const sdumc_rows_problem* probs, int32_t n, int32_t max_wg, void* stream) {
  if (!probs || n <= 0 || n > MAXP) return SDUMC_EINVAL;
  return launch(probs, n, max_wg, stream, FORM_BF16, find(BF16_VARIANTS, false, probs[0], probs[0].fold), SDUMC_PV_gemm_rows256_bf16);
}

SDUMC_PRELOAD_HOOK(gemm_rows)      // (common.h)
