// Depth of coverage (DESIGN §2 [EXT], §4.11): what one base of one record adds.
// One text for the gfx950 kernels (depth.hip) and the host check
// (tools/micro/depth_test.cpp); everything works over caller spans, one base
// at a time, so that a lane can take a base.
//
//   dp_counted    the record filter (ref_id, CIGAR, flags, MAPQ bounds)
//   dp_base_ok    the base quality bounds
//   dp_in_window  the window offset of a counted position, or -1
//   dp_run_first / dp_run_last   the ends of the maximal runs of counted bases
//                 at consecutive positions among 64 neighbours
//   dp_bin / dp_quantile         the histogram bin and the granular quantile
// The CIGAR walks (cigar_span, cigar_site) are cigar_walk.h's.
#pragma once

#include <stdint.h>

#include "cigar_walk.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DP_HD __host__ __device__ __forceinline__
#else
#define DP_HD inline
#endif

namespace fcs {

constexpr int kDpBins = 501, kDpAbove = 15, kDpPieceMax = 65536;
constexpr uint16_t kDpFlagFilter = 0x4 | 0x100 | 0x200 | 0x400;
constexpr int kDpStatusField = 1, kDpStatusRef = 2, kDpStatusOverflow = 4;

DP_HD bool dp_counted(uint16_t flag, int32_t ref_id, int64_t n_ops, uint8_t mapq, int32_t min_mapq, int32_t max_mapq) {
  return ref_id >= 0 && n_ops > 0 && (flag & kDpFlagFilter) == 0 && (int32_t)mapq >= min_mapq && (int32_t)mapq <= max_mapq;
}

DP_HD bool dp_base_ok(int q, int32_t min_baseq, int32_t max_baseq) { return q >= min_baseq && q <= max_baseq; }

// The window offset of position p of a contig of clen bases, or -1 outside the
// window [w0, w0 + wlen) or the contig.
DP_HD int32_t dp_in_window(int64_t p, int64_t w0, int64_t wlen, int64_t clen) {
  return p >= 0 && p < clen && p >= w0 && p < w0 + wlen ? (int32_t)(p - w0) : -1;
}

// Lane `lane` of 64 holds window offset off (>= 0: counted).  counted is the
// ballot of off >= 0, prev / next the neighbours' offsets (lane - 1, lane + 1).
DP_HD bool dp_run_first(int lane, unsigned long long counted, int32_t off, int32_t prev) {
  return off >= 0 && (lane == 0 || !((counted >> (lane - 1)) & 1u) || prev != off - 1);
}
DP_HD bool dp_run_last(int lane, unsigned long long counted, int32_t off, int32_t next) {
  return off >= 0 && (lane == 63 || !((counted >> (lane + 1)) & 1u) || next != off + 1);
}

DP_HD int dp_bin(uint32_t depth) { return depth < (uint32_t)(kDpBins - 1) ? (int)depth : kDpBins - 1; }

// Bin b is the k-th granular quantile (k = 1, 2, 3) of n > 0 loci when the
// counts up to and including it reach k/4 of n and those before it do not.
DP_HD bool dp_is_quantile(uint64_t cum_before, uint64_t cum_with, uint64_t n, int k) {
  return 4 * cum_with >= (uint64_t)k * n && 4 * cum_before < (uint64_t)k * n;
}
DP_HD uint32_t dp_reported(int bin) { return bin < 1 ? 1u : (uint32_t)bin; }

}  // namespace fcs
