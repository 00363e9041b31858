// The rules of minimizer seeding and chaining that the device kernel
// (mm_chain.hip), the host path (host/minimizer.cpp) and the stand-alone
// program (tools/micro/mm_test.cpp) share, each stated once (DESIGN §2 [EXT]
// "minimizer seeding and chaining"): the k-mer hash, the anchor's target key,
// the test and the score of a candidate predecessor, and the order in which
// candidates are compared.  Integers only.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MM_HD __host__ __device__ __forceinline__
#else
#define MM_HD inline
#endif

namespace fcs {

constexpr int kMmLookback = 64;         // predecessors j in [i - 64, i - 1]
constexpr int kMmSpanMax = 64;          // the largest span (k)
constexpr int kMmGapMax = 1 << 20;      // the largest max_gap and bw
constexpr int kMmReadAnchors = 1 << 24; // anchors of one read: f stays below 2^31
constexpr int kMmStatusField = 1, kMmStatusOrder = 2;

// The invertible 64-bit mix, masked to 2k bits (mask = 4^k - 1).
MM_HD uint64_t mm_hash64(uint64_t key, uint64_t mask) {
  key = (~key + (key << 21)) & mask;
  key = key ^ key >> 24;
  key = ((key + (key << 3)) + (key << 8)) & mask;
  key = key ^ key >> 14;
  key = ((key + (key << 2)) + (key << 4)) & mask;
  key = key ^ key >> 28;
  key = (key + (key << 31)) & mask;
  return key;
}

// t = (contig * 2 + rev) << 32 | position of the k-mer's last base on the forward reference.
MM_HD int64_t mm_target(int contig, bool rev, int64_t pos) { return (int64_t)(((uint64_t)contig * 2 + (rev ? 1 : 0)) << 32 | (uint64_t)pos); }
MM_HD int mm_target_contig(int64_t t) { return (int)((uint64_t)t >> 33); }
MM_HD bool mm_target_rev(int64_t t) { return ((uint64_t)t >> 32) & 1; }
MM_HD int64_t mm_target_pos(int64_t t) { return (int64_t)((uint64_t)t & 0xFFFFFFFFu); }

// Anchors are sorted by (t, q): is (ta, qa) allowed before (tb, qb)?
MM_HD bool mm_in_order(int64_t ta, int32_t qa, int64_t tb, int32_t qb) { return ta < tb || (ta == tb && qa <= qb); }

// floor(log2(v)), v > 0
MM_HD int mm_ilog2(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return 31 - __clz((int)v);
#else
  return 31 - __builtin_clz(v);
#endif
}

struct MmParams {
  int32_t max_gap, bw, span;
};

// Anchor j = (tj, qj) with its final f[j] = fj as a predecessor of anchor i =
// (ti, qi): false when j is skipped, else its score in sc.  dr <= 0 is dr == 0
// on sorted anchors; a contig or strand change makes dr larger than any gap.
MM_HD bool mm_candidate(int64_t ti, int32_t qi, int64_t tj, int32_t qj, int32_t fj, const MmParams& P, int32_t& sc) {
  const int64_t dr = (int64_t)((uint64_t)ti - (uint64_t)tj), dq = (int64_t)qi - qj;
  if (dr <= 0 || dr > P.max_gap || dq <= 0 || dq > P.max_gap) return false;
  const int32_t dd = (int32_t)(dr > dq ? dr - dq : dq - dr);
  if (dd > P.bw) return false;
  const int32_t m = (int32_t)(dq < dr ? dq : dr);
  sc = fj + (m < P.span ? m : P.span) - ((dd * P.span) / 100 + (dd ? mm_ilog2((uint32_t)dd) >> 1 : 0));
  return true;
}

// The running best of anchor i (f = span and p = -1 at the start) takes the
// candidate j, applied in ascending j: the largest score wins, among equal
// scores the largest j, and only a score strictly above span is taken.
MM_HD void mm_take(int32_t sc, int32_t j, int32_t span, int32_t& f, int32_t& p) {
  if (sc > span && sc >= f) f = sc, p = j;
}

}  // namespace fcs
