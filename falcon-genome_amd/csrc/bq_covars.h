// Base quality recalibration (DESIGN §2 [EXT], §4.10): what one base of one
// record contributes.  One text for the gfx950 kernels (bqsr.hip) and the host
// check (tools/micro/bqsr_test.cpp); everything works over caller spans, one
// base at a time, so that a lane can take a base.
//
//   bq_clips     the soft-clipped bases before the first and after the last of
//                M / I / = / X, and the bases the CIGAR covers
//   bq_site      where read base i lies: aligned at a reference position,
//                inserted after one, or soft-clipped
//   bq_low_ends  the runs of qualities <= 2 at both ends (N for the context)
//   bq_context   4 * code(prev) + code(cur) in sequencing order, or -1
//   bq_cycle     2 * (|c| - 1) + (c < 0)
//   bq_skipped / bq_error / bq_new_quality   the predicates and the apply formula
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BQ_HD __host__ __device__ __forceinline__
#else
#define BQ_HD inline
#endif

namespace fcs {

constexpr int kBqNq = 94, kBqNctx = 16, kBqNcyc = 1000, kBqMaxCycle = 500;
constexpr int kBqCols = kBqNctx + kBqNcyc;  // one device row per (read group, quality): contexts, then cycles
constexpr uint16_t kBqFlagPaired = 0x1, kBqFlagReverse = 0x10, kBqFlagRead2 = 0x80;
constexpr uint16_t kBqFlagFilter = 0x4 | 0x100 | 0x200 | 0x400;
enum : int { kBqAligned = 0, kBqInserted = 1, kBqClipped = 2 };

BQ_HD int bq_code(uint32_t b) {
  b &= 0xDFu;
  return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : -1;
}

BQ_HD bool bq_counted(uint16_t flag, int32_t rg, uint8_t mapq, bool qual_absent) {
  return rg >= 0 && !qual_absent && (flag & kBqFlagFilter) == 0 && mapq != 0 && mapq != 255;
}
BQ_HD bool bq_applied(int32_t rg, bool qual_absent) { return rg >= 0 && !qual_absent; }
BQ_HD bool bq_second(uint16_t flag) { return (flag & kBqFlagPaired) && (flag & kBqFlagRead2); }

// One pass over the record's n_ops CIGAR words (len << 4 | op).
BQ_HD void bq_clips(const uint32_t* cigar, int64_t n_ops, int64_t& lead, int64_t& trail, int64_t& covered) {
  lead = trail = covered = 0;
  bool seen = false;
  for (int64_t k = 0; k < n_ops; ++k) {
    const uint32_t op = cigar[k] & 15u;
    const int64_t len = (int64_t)(cigar[k] >> 4);
    if (op == 4u) {
      if (seen) trail += len;
      else lead += len;
      covered += len;
    } else if (op == 0u || op == 1u || op == 7u || op == 8u) {
      seen = true;
      trail = 0;
      covered += len;
    }
  }
}

// Read base i (0 <= i < covered): its kind, and in p the reference position
// (aligned) or the aligned position before the insertion (inserted).
BQ_HD int bq_site(const uint32_t* cigar, int64_t n_ops, int32_t pos, int64_t i, int64_t& p) {
  int64_t q = 0, r = pos;
  for (int64_t k = 0; k < n_ops; ++k) {
    const uint32_t op = cigar[k] & 15u;
    const int64_t len = (int64_t)(cigar[k] >> 4);
    if (op == 0u || op == 7u || op == 8u) {
      if (i < q + len) {
        p = r + (i - q);
        return kBqAligned;
      }
      q += len, r += len;
    } else if (op == 1u || op == 4u) {
      if (i < q + len) {
        p = r - 1;
        return op == 1u ? kBqInserted : kBqClipped;
      }
      q += len;
    } else if (op == 2u || op == 3u) {
      r += len;
    }
  }
  p = 0;
  return kBqClipped;  // beyond the CIGAR: the callers refuse or flag such a record first
}

// The runs of qualities <= 2 at the start and at the end of qual[0, k).
BQ_HD void bq_low_ends(const uint8_t* qual, int64_t k, int64_t& nl, int64_t& nr) {
  nl = nr = 0;
  while (nl < k && qual[nl] <= 2) ++nl;
  while (nr < k && qual[k - 1 - nr] <= 2) ++nr;
}

// The context key of base j of seq[0, k) (the kept read, or the whole read in
// apply): the previous base in sequencing order is j - 1, or j + 1 of the
// complement on the reverse strand; a base inside a low-quality end is N.
BQ_HD int bq_context(const uint8_t* seq, int64_t k, int64_t j, int64_t nl, int64_t nr, bool reverse) {
  const int64_t jp = reverse ? j + 1 : j - 1;
  if (j < nl || j >= k - nr || jp < nl || jp >= k - nr || jp < 0 || jp >= k) return -1;
  int cc = bq_code(seq[j]), cp = bq_code(seq[jp]);
  if (cc < 0 || cp < 0) return -1;
  if (reverse) cc = 3 - cc, cp = 3 - cp;
  return 4 * cp + cc;
}

BQ_HD int bq_cycle(int64_t k, int64_t j, bool reverse, bool second) {
  const int64_t cycle = reverse ? k - j : j + 1;
  return (int)(2 * (cycle - 1) + (second ? 1 : 0));
}

// A counted record's base that is no observation (before the known-site test).
BQ_HD bool bq_skipped(int kind, int code, int q) { return kind == kBqClipped || code < 0 || q < 6 || q >= kBqNq; }

// Bit g of the known-sites bitmap.
BQ_HD bool bq_known(const uint64_t* known, int64_t g) { return (known[g >> 6] >> (g & 63)) & 1u; }

BQ_HD bool bq_error(int kind, int code, uint8_t ref_byte) { return kind == kBqAligned && bq_code(ref_byte) != code; }

// clamp(trunc(base + dctx + dcyc + 0.5), 1, 93), the terms added in this order (no contraction).
BQ_HD uint8_t bq_new_quality(double base, double dctx, double dcyc) {
  const double v = ((base + dctx) + dcyc) + 0.5;
  return (uint8_t)(!(v >= 1.0) ? 1 : v > 93.0 ? 93 : (int)v);
}

}  // namespace fcs
