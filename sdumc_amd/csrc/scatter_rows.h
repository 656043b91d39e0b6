// scatter_rows.h — the indexed row scatter dst_k[idx[r % B], :] = src_k[r, :] as ONE piece of device code and ONE set of argument
// rules, for the two launches that do it: sdumc_scatter_rows_multi (elementwise.hip: after an eval-mode forward) and
// sdumc_epoch_record (epoch_record.hip: after a train step, beside the step's log row).
#pragma once
#include <algorithm>
#include <cstring>

#include "common.h"

// the segments as the kernels get them (by value in the kernel arguments): vec[k] = segment k moves 16 bytes per lane
struct ScatterSegs {
  sdumc_scatter_seg s[SDUMC_SCATTER_MAX_SEGS];
  uint8_t vec[SDUMC_SCATTER_MAX_SEGS];
  const int64_t* idx;
  uint8_t* mark;
  int32_t B;
};

// Segment `seg` on the `nthr` threads of which this one is `tid`: a lane moves 16 bytes where the segment's width and base addresses
// allow it (vec, decided by scatter_segs_fill), one float otherwise.  64-bit row addressing; an index outside [0, dst_rows) is
// skipped.  The threads of segment 0 also set the visited marks.
__device__ __forceinline__ void scatter_rows_segment(const ScatterSegs& ss, int seg, int64_t tid, int64_t nthr) {
  const sdumc_scatter_seg& sg = ss.s[seg];
  if (seg == 0 && ss.mark)
    for (int64_t b = tid; b < ss.B; b += nthr) {
      const int64_t e = ss.idx[b];
      if ((uint64_t)e < (uint64_t)sg.dst_rows) ss.mark[e] = 1;
    }
  const int lpr = ss.vec[seg] ? sg.cols >> 2 : sg.cols;      // lanes per row
  const int64_t n = (int64_t)sg.rows * lpr;
  for (int64_t i = tid; i < n; i += nthr) {
    const int64_t r = i / lpr;
    const int c = (int)(i - r * lpr);
    const int64_t e = ss.idx[r % ss.B];
    if ((uint64_t)e >= (uint64_t)sg.dst_rows) continue;
    if (ss.vec[seg])
      *reinterpret_cast<f32x4*>(sg.dst + (e * sg.cols + 4 * c)) = *reinterpret_cast<const f32x4*>(sg.src + (r * sg.cols + 4 * c));
    else
      sg.dst[e * sg.cols + c] = sg.src[r * sg.cols + c];
  }
}

// The argument rules of include/sdumc_hip.h (sdumc_scatter_rows_multi) and the kernel-side table.  SDUMC_EINVAL or SDUMC_OK;
// *lanes = the lanes of the widest segment (at least B: the mark pass).  Host only, no HIP call.
static inline int scatter_segs_fill(ScatterSegs* ss, const sdumc_scatter_seg* segs, int32_t n, const int64_t* idx, int32_t B,
                                    uint8_t* mark, int64_t* lanes) {
  if (!segs || n < 1 || n > SDUMC_SCATTER_MAX_SEGS || !idx || B < 1) return SDUMC_EINVAL;
  memset(ss, 0, sizeof(*ss));
  int64_t mx = B;
  for (int i = 0; i < n; ++i) {
    const sdumc_scatter_seg& sg = segs[i];
    if (!sg.src || !sg.dst || sg.rows < 1 || sg.cols < 1 || sg.rows % B != 0) return SDUMC_EINVAL;
    if (sg.dst_rows < 1 || sg.dst_rows > ((int64_t)1 << 61) / sg.cols) return SDUMC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(sg.src) | reinterpret_cast<uintptr_t>(sg.dst)) & 3) return SDUMC_EINVAL;
    ss->s[i] = sg;
    ss->vec[i] = (sg.cols % 4 == 0 && !((reinterpret_cast<uintptr_t>(sg.src) | reinterpret_cast<uintptr_t>(sg.dst)) & 15)) ? 1 : 0;
    mx = std::max<int64_t>(mx, (int64_t)sg.rows * (ss->vec[i] ? sg.cols / 4 : sg.cols));
  }
  ss->idx = idx;
  ss->mark = mark;
  ss->B = B;
  *lanes = mx;
  return SDUMC_OK;
}
