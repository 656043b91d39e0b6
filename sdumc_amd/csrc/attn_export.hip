// attn_export.hip — sdumc_net_export_attention: the softmax-over-time weights of a completed eval-mode forward, out of the forward's
// workspace and into store-ordered per-frame tensors (include/sdumc_hip.h has the contract).  The reference returns these weights
// from FRA2UTT_new / Cross_Attention (vector_attention, model :68, :95) and collects them in forward (attention_masks, model :291).
//
// Source: Plan.attn[k][m] (engine.hip), per run [V][T][nq] with v = s * B + b; the text slot is two runs when the two streams'
// padded lengths differ, else one run of 2 B samples -- either way sample (s, b) of modality m starts at row s * B * T[m][0] + b * T[m][s].
// Every route of the forward leaves NORMALISED weights there in eval mode, fp32 in both storage modes: the pair / multi partial pass
// writes exp(score - chunk max) and the combine pass (attn_fwd_combine_body, attn_pool.hip) scales by exp(chunk max - max) / sum; K3
// (sdumc_umca_fwd) ends in that same combine launch; with the clustered stages' fold the partial-only pass leaves the unnormalised
// weights and fold_combine (chain_cluster.hip) scales them in place before the stage's first exchange.  So this kernel copies; it
// does not normalise, and it reads no chunk statistics.
//
// One launch per batch: a flat grid over (stream, modality) pairs x samples x 64-frame chunks, one wavefront per item.  The chunk's
// FRA2UTT weights are 64 contiguous floats (one per lane); its Cross_Attention weights are 64 rows of 7 floats = 1 792 contiguous
// bytes: seven coalesced dword loads per lane into the wavefront's LDS tile, read back with stride 7 dwords (7 is odd: the 32 lanes
// of a ds_read_b32 group hit 32 different banks), so that lane t owns frame t0 + t and writes its 32-byte destination row with two
// 16-byte stores.  Destination rows are addressed with 64 bits.  Plain stores, no atomics: a repeated launch gives the same bits.
#include <string.h>

#include "common.h"

namespace {
constexpr int CH = 64, NQ = SDUMC_NQ, WAVES = 4, MAXPAIR = 6;

struct ExportArgs {
  const float* a0[MAXPAIR];        // FRA2UTT weights of the pair's stream: [B][T] floats
  const float* a1[MAXPAIR];        // Cross_Attention weights: [B][T][7]
  float* dst[MAXPAIR];             // [dst_rows][8]
  int64_t dst_rows[MAXPAIR];
  const int64_t* start[MAXPAIR];   // store-wide tables of the pair's modality
  const int32_t* length[MAXPAIR];
  int32_t T[MAXPAIR], nchunk[MAXPAIR];
  int32_t item_end[MAXPAIR];       // running sum of B * nchunk
  const int64_t* idx;
  int64_t n_utt;
  int32_t B, npair;
};

__global__ __launch_bounds__(64 * WAVES) void attn_export_kernel(const ExportArgs a) {
  __shared__ float tile[WAVES][CH * NQ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int item = blockIdx.x * WAVES + wave;
  int p = 0;
  while (p < a.npair - 1 && item >= a.item_end[p]) ++p;
  int nvalid = 0, t0 = 0;          // frames of this item's chunk to export (0: nothing -- the wavefront still meets the barrier)
  int64_t row0 = 0;
  const float *s0 = nullptr, *s1 = nullptr;
  if (item < a.item_end[a.npair - 1]) {
    const int local = item - (p ? a.item_end[p - 1] : 0);
    const int b = local / a.nchunk[p], chunk = local - b * a.nchunk[p];
    const int64_t e = a.idx[b];
    if ((uint64_t)e < (uint64_t)a.n_utt) {
      const int T = a.T[p];
      const int len = min(a.length[p][e], T);      // (never beyond the padded length the forward ran with)
      t0 = chunk * CH;
      nvalid = max(0, min(CH, len - t0));
      row0 = a.start[p][e] + t0;
      s0 = a.a0[p] + ((int64_t)b * T + t0);
      s1 = a.a1[p] + ((int64_t)b * T + t0) * NQ;
    }
  }
  float w0 = 0.f;
  if (lane < nvalid) w0 = s0[lane];
  float w[NQ];      // (all seven loads in flight before the first LDS store)
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    const int o = j * CH + lane;
    w[j] = o < nvalid * NQ ? s1[o] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < NQ; ++j) tile[wave][j * CH + lane] = w[j];
  // (every wavefront reads back only its OWN tile: wave-local ordering of the LDS stores and loads is all that is needed.  The
  //  workgroup barrier is the portable way to state it; no wavefront returns before it, which is why the out-of-range cases above
  //  fall through with nvalid = 0 instead of returning.)
  __syncthreads();
  if (lane < nvalid) {
    const int64_t row = row0 + lane;
    if ((uint64_t)row < (uint64_t)a.dst_rows[p]) {
      const float* r = &tile[wave][lane * NQ];
      const f32x4 lo = {w0, r[0], r[1], r[2]}, hi = {r[3], r[4], r[5], r[6]};
      float* d = a.dst[p] + row * 8;
      st4(d, lo);
      st4(d + 4, hi);
    }
  }
}
}  // namespace

extern "C" int sdumc_net_export_attention(const sdumc_net_dims* d, const sdumc_net_io* io, const sdumc_attn_export* e, void* stream) {
  if (!d || !io || !e || !e->idx || !io->workspace || e->n_utt < 1) return SDUMC_EINVAL;
  sdumc_attn_layout lay;
  if (sdumc_plan_attn_layout_(d, &lay) != SDUMC_OK) return SDUMC_EINVAL;      // dims the engine refuses
  if (io->workspace_bytes < (size_t)lay.total * sizeof(float)) return SDUMC_ENOMEM;
  if (lay.S == 1 && (e->dst[1][0] || e->dst[1][1] || e->dst[1][2])) return SDUMC_EINVAL;
  const float* W = static_cast<const float*>(io->workspace);
  ExportArgs a;
  memset(&a, 0, sizeof(a));
  int64_t items = 0;
  for (int s = 0; s < lay.S; ++s)
    for (int m = 0; m < 3; ++m) {
      const int slot = m == 0 ? 0 : (m == 2 ? 2 : (s == 0 ? 1 : 3));      // tables: audio, text, video, feat4
      float* dst = e->dst[s][m];
      if (!dst || !e->start[slot] || !e->length[slot] || e->dst_rows[s][m] < 1) return SDUMC_EINVAL;
      if (reinterpret_cast<uintptr_t>(dst) & 15) return SDUMC_EINVAL;
      const int p = a.npair++;
      const int T = lay.T[m][s];
      const int64_t r0 = (int64_t)s * lay.B * lay.T[m][0];      // first virtual row of stream s (one run of 2 B or two runs: the same)
      a.a0[p] = W + lay.attn[0][m] + r0;
      a.a1[p] = W + lay.attn[1][m] + r0 * NQ;
      a.dst[p] = dst;
      a.dst_rows[p] = e->dst_rows[s][m];
      a.start[p] = e->start[slot];
      a.length[p] = e->length[slot];
      a.T[p] = T;
      a.nchunk[p] = (T + CH - 1) / CH;
      items += (int64_t)lay.B * a.nchunk[p];
      if (items > 0x7FFFFFFF - WAVES) return SDUMC_EINVAL;
      a.item_end[p] = (int32_t)items;
    }
  a.idx = e->idx;
  a.n_utt = e->n_utt;
  a.B = lay.B;
  hipLaunchKernelGGL(attn_export_kernel, dim3((unsigned)((items + WAVES - 1) / WAVES)), dim3(64 * WAVES), 0, as_stream(stream), a);
  SDUMC_CHECK_LAUNCH();
  return SDUMC_OK;
}

SDUMC_PRELOAD_HOOK(attn_export)      // (common.h)
