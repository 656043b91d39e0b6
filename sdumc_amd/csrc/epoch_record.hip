// epoch_record.hip — the record a training epoch keeps of every step (sdumc_epoch_record): behind a completed sdumc_train_step one
// launch files the step's train-mode outputs at the rows its utterances have in the store (the scatter of scatter_rows.h, shared
// with sdumc_scatter_rows_multi) and writes the step's 12-float log row; with a gradient bucket given, the same launch folds the
// bucket into per-workgroup partials (sum of squares, count of non-finite elements) and a second, one-workgroup launch adds them and
// writes the row.  Read-only towards the step: nothing of its workspace, losses or hyper is written.
//
// Grid of the first launch (1-D): the first `nred` workgroups reduce, the others scatter (workgroup q of those: segment q / sblk).
// The reduce is reproducible: workgroup b owns the contiguous quads [b qpb, (b + 1) qpb) of the 16-byte aligned body of the bucket
// (the <= 3 floats in front of it and the <= 3 behind it go to workgroup 0's thread 0), every thread walks its quads in a fixed
// order into one fp64 sum of squares and one count, the 256 threads' values are folded by a fixed LDS tree, and the second launch
// adds the workgroups' partials in INDEX order.  Plain loads and stores, no atomics: the launch boundary orders the partials.
// Two launches, not one with a last-arriver ticket: both forms were built and alternated in the epoch (profiles/README.md) and tied
// within the run-to-run spread -- the ticket form's agent-scope publish, ticket and re-read cost its kernel the 6 us the second
// launch costs here -- so the form without inter-workgroup communication stays.
#include "common.h"
#include "scatter_rows.h"

namespace {

constexpr int NT = 256;            // threads per workgroup
constexpr int UNROLL = 16;         // quads a thread has in flight: a C2 bucket (3.9 M floats) is ONE round of loads on 256 workgroups
constexpr int MAX_RED = 256;       // reduce workgroups (one per CU; their partials fit the second launch's one workgroup)
constexpr int MAX_SBLK = 64;       // scatter workgroups per segment
static_assert(MAX_RED <= NT, "the final launch reads one partial per thread");

struct RecordArgs {
  ScatterSegs ss;
  int32_t nseg, sblk, nred, B;
  const float* grads;              // the bucket; body = grads + head
  int64_t n, head, nquad, qpb;     // floats; floats in front of the aligned body; quads of the body; quads per reduce workgroup
  double* part_sum;                // [nred] sums of squares
  uint32_t* part_bad;              // [nred] counts of non-finite elements
  const float *losses, *hyper;
  float* log_row;
};

// columns 0..7 the loss vector as it stands, 8 grad_norm, 9 non-finite gradient elements, 10 B, 11 the learning rate
__device__ __forceinline__ void write_log_row(const RecordArgs& a, float norm, float bad) {
  const int t = threadIdx.x;
  if (t < 8) a.log_row[t] = a.losses[t];
  else if (t == 8) a.log_row[8] = norm;
  else if (t == 9) a.log_row[9] = bad;
  else if (t == 10) a.log_row[10] = (float)a.B;
  else if (t == 11) a.log_row[11] = a.hyper[0];
}

__global__ __launch_bounds__(NT) void epoch_record_kernel(const RecordArgs a) {
  __shared__ double s_sum[NT];
  __shared__ uint32_t s_bad[NT];
  const int bid = blockIdx.x, t = threadIdx.x;
  if (bid >= a.nred) {
    if (a.nseg > 0) {
      const int q = bid - a.nred;
      scatter_rows_segment(a.ss, q / a.sblk, (int64_t)(q % a.sblk) * NT + t, (int64_t)a.sblk * NT);
    }
    if (a.nred == 0 && bid == 0) write_log_row(a, __uint_as_float(0x7fc00000u), 0.f);      // (no bucket: NaN, 0)
    return;
  }
  // ---- this workgroup's slice of the bucket ----
  const float* body = a.grads + a.head;
  const int64_t q0 = (int64_t)bid * a.qpb, q1 = min(q0 + a.qpb, a.nquad);
  double acc = 0.0;
  uint32_t bad = 0;
  for (int64_t i = q0 + t; i < q1; i += (int64_t)NT * UNROLL) {
    f32x4 v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t k = i + (int64_t)u * NT;
      v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (k < q1) v[u] = *reinterpret_cast<const f32x4*>(body + 4 * k);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) sumsq_count_nonfinite(v[u][j], acc, bad);
  }
  if (bid == 0 && t == 0) {
    for (int64_t k = 0; k < a.head; ++k) sumsq_count_nonfinite(a.grads[k], acc, bad);
    for (int64_t k = a.head + 4 * a.nquad; k < a.n; ++k) sumsq_count_nonfinite(a.grads[k], acc, bad);
  }
  s_sum[t] = acc;
  s_bad[t] = bad;
  __syncthreads();
#pragma unroll
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (t < s) {
      s_sum[t] += s_sum[t + s];
      s_bad[t] += s_bad[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    a.part_sum[bid] = s_sum[0];
    a.part_bad[bid] = s_bad[0];
  }
}

// the partials in index order, one rounding to fp32 (a count below 2^24 is exact), the log row
__global__ __launch_bounds__(NT) void epoch_record_final_kernel(const RecordArgs a) {
  __shared__ double s_sum[NT];
  __shared__ uint32_t s_bad[NT];
  const int t = threadIdx.x;
  if (t < a.nred) {
    s_sum[t] = a.part_sum[t];
    s_bad[t] = a.part_bad[t];
  }
  __syncthreads();
  if (t == 0) {
    double sum = 0.0;
    uint32_t cnt = 0;
    for (int k = 0; k < a.nred; ++k) {
      sum += s_sum[k];
      cnt += s_bad[k];
    }
    s_sum[0] = sqrt(sum);
    s_bad[0] = cnt;
  }
  __syncthreads();
  write_log_row(a, (float)s_sum[0], (float)s_bad[0]);
}

// reduce workgroups for a body of `nquad` quads: a thread's UNROLL quads per workgroup at least, MAX_RED workgroups at most
inline int reduce_workgroups(int64_t nquad) {
  const int64_t per = (int64_t)NT * UNROLL;
  return (int)std::min<int64_t>(MAX_RED, std::max<int64_t>(1, (nquad + per - 1) / per));
}

}  // namespace

extern "C" size_t sdumc_epoch_record_scratch_bytes(int64_t n_grads) {
  if (n_grads < 1) return 0;
  return 16 * (size_t)reduce_workgroups(n_grads / 4);      // the workgroups' fp64 sums of squares, then (8 bytes each) their counts
}

extern "C" int sdumc_epoch_record(const sdumc_epoch_rec* r, void* stream) {
  if (!r || !r->log_row || !r->losses || !r->hyper) return SDUMC_EINVAL;
  if (r->nseg < 0 || r->nseg > SDUMC_SCATTER_MAX_SEGS) return SDUMC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(r->log_row) | reinterpret_cast<uintptr_t>(r->losses) | reinterpret_cast<uintptr_t>(r->hyper)) & 3)
    return SDUMC_EINVAL;
  RecordArgs a;
  memset(&a, 0, sizeof(a));
  int64_t lanes = 0;
  if (r->nseg > 0) {
    if (scatter_segs_fill(&a.ss, r->seg, r->nseg, r->idx, r->B, r->mark, &lanes) != SDUMC_OK) return SDUMC_EINVAL;
    a.sblk = (int)std::min<int64_t>(MAX_SBLK, (lanes + NT - 1) / NT);
  }
  a.nseg = r->nseg;
  a.B = r->B;
  if (r->grads) {
    if (r->n_grads < 1 || !r->scratch) return SDUMC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(r->grads) & 3) || (reinterpret_cast<uintptr_t>(r->scratch) & 15)) return SDUMC_EINVAL;
    a.grads = r->grads;
    a.n = r->n_grads;
    a.head = std::min<int64_t>(a.n, (int64_t)((16 - (reinterpret_cast<uintptr_t>(r->grads) & 15)) & 15) / 4);
    a.nquad = (a.n - a.head) / 4;
    a.nred = reduce_workgroups(a.nquad);      // (<= the count sdumc_epoch_record_scratch_bytes(n_grads) sized the scratch for)
    a.qpb = (a.nquad + a.nred - 1) / a.nred;
    a.part_sum = reinterpret_cast<double*>(r->scratch);
    a.part_bad = reinterpret_cast<uint32_t*>(a.part_sum + reduce_workgroups(a.n / 4));
  }
  a.losses = r->losses;
  a.hyper = r->hyper;
  a.log_row = r->log_row;
  const int grid = std::max(1, a.nred + a.nseg * a.sblk);
  hipLaunchKernelGGL(epoch_record_kernel, dim3(grid), dim3(NT), 0, as_stream(stream), a);
  SDUMC_CHECK_LAUNCH();
  if (a.nred > 0) {
    hipLaunchKernelGGL(epoch_record_final_kernel, dim3(1), dim3(NT), 0, as_stream(stream), a);
    SDUMC_CHECK_LAUNCH();
  }
  return SDUMC_OK;
}

SDUMC_PRELOAD_HOOK(epoch_record)      // (common.h)
