// Duplicate marking (DESIGN §2 [EXT], §4.9): what one record and one pair
// contribute to the grouping.  One text for the gfx950 kernels (markdup.hip),
// the host path (host/markdup.cpp) and the host check
// (tools/micro/markdup_test.cpp); everything works over caller spans.
//
// An examined record r (none of unmapped, secondary, supplementary) has
//   u5     its unclipped 5' position: pos - leading S/H (forward), pos + reflen
//          - 1 + trailing S/H (reverse); signed
//   score  the sum of its quality bytes >= 15, a 32-bit sum
//   end    (lib, ref, u5, strand) packed into one 64-bit word that compares as
//          the tuple does: lib 11 bits | ref_id + 1 21 bits | u5 + 2^30 31 bits
//          | strand 1 bit.  A batch whose values do not fit is refused by the
//          entry point (md_fits_*), so two different tuples never share a word;
//          the all-ones word (lib 2047) is kept free as the sort's sentinel.
// A pair's key is 117 bits, (lib; lesser end; greater end), as two words: hi =
// the lesser end's whole end word, lo = the greater end's without the library.
// Winner words: (score << 32) | ~index, so that a 64-bit max keeps the greatest
// score and, among equals, the smallest index; in a fragment group a paired
// record's word also carries bit 63, so it beats every fragment.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MD_HD __host__ __device__ __forceinline__
#else
#define MD_HD inline
#endif

namespace fcs {

constexpr int kMdLibBits = 11, kMdRefBits = 21, kMdPosBits = 31;
constexpr int32_t kMdMaxLibs = (1 << kMdLibBits) - 1;  // lib in [0, 2047): 2047 is the sentinel's
constexpr int32_t kMdMaxRefs = (1 << kMdRefBits) - 1;  // ref_id + 1 in [0, 2^21)
constexpr int64_t kMdPosBias = (int64_t)1 << (kMdPosBits - 1);  // |u5| < 2^30
constexpr int64_t kMdMaxQual = (int64_t)1 << 22;  // quality bytes per record: score < 2^30, a pair's < 2^31
constexpr int64_t kMdMaxRecords = (int64_t)1 << 30;
constexpr uint64_t kMdSentinel = ~(uint64_t)0;
constexpr uint64_t kMdPairedBit = (uint64_t)1 << 63;
constexpr int kMdEndBits = kMdRefBits + kMdPosBits + 1;  // an end word without its library: 53 bits

constexpr uint16_t kMdFlagPaired = 0x1, kMdFlagUnmapped = 0x4, kMdFlagMateUnmapped = 0x8, kMdFlagReverse = 0x10,
                   kMdFlagSecondary = 0x100, kMdFlagDuplicate = 0x400, kMdFlagSupplementary = 0x800;

MD_HD bool md_examined(uint16_t flag) {
  return (flag & (kMdFlagUnmapped | kMdFlagSecondary | kMdFlagSupplementary)) == 0;
}

// The unclipped 5' position from the record's n_ops CIGAR words (len << 4 | op;
// S = 4, H = 5).  One pass: the clips before the first other operation lead,
// the clips after the last one trail (a CIGAR of clips only has no trailing
// ones), M / D / N / = / X consume the reference.
MD_HD int64_t md_u5(int32_t pos, bool reverse, const uint32_t* cigar, int64_t n_ops) {
  int64_t lead = 0, trail = 0, reflen = 0;
  bool leading = true;
  for (int64_t k = 0; k < n_ops; ++k) {
    const uint32_t c = cigar[k], op = c & 15u;
    const int64_t len = (int64_t)(c >> 4);
    if (op == 4u || op == 5u) {
      if (leading) lead += len;
      else trail += len;
    } else {
      leading = false;
      trail = 0;
      if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) reflen += len;
    }
  }
  return reverse ? (int64_t)pos + reflen - 1 + trail : (int64_t)pos - lead;
}

MD_HD bool md_fits_u5(int64_t u5) { return u5 > -kMdPosBias && u5 < kMdPosBias; }

// The bytes >= 15 of a dword whose bytes lo .. hi - 1 (0 <= lo <= hi <= 4) belong to the record.
MD_HD uint32_t md_score_word(uint32_t w, int lo, int hi) {
  uint32_t s = 0;
  for (int b = 0; b < 4; ++b) {
    const uint32_t q = (w >> (8 * b)) & 0xffu;
    s += (b >= lo && b < hi && q >= 15u) ? q : 0u;
  }
  return s;
}

// The same sum over a byte span (the host's form).
MD_HD uint32_t md_score(const uint8_t* qual, int64_t n) {
  uint32_t s = 0;
  for (int64_t i = 0; i < n; ++i) s += qual[i] >= 15 ? (uint32_t)qual[i] : 0u;
  return s;
}

// (ref, u5, strand) in 53 bits; ref_id in [-1, kMdMaxRefs - 1), md_fits_u5(u5).
MD_HD uint64_t md_end_word(int32_t ref_id, int64_t u5, bool reverse) {
  return ((uint64_t)(uint32_t)(ref_id + 1) << (kMdPosBits + 1)) | ((uint64_t)(u5 + kMdPosBias) << 1) |
         (reverse ? 1u : 0u);
}

// The fragment-group key E = (lib, ref, u5, strand); lib in [0, kMdMaxLibs).
MD_HD uint64_t md_frag_key(int32_t lib, uint64_t end_word) { return ((uint64_t)(uint32_t)lib << kMdEndBits) | end_word; }

// Record a's end sorts before record b's: (ref, u5, strand, index).  Both keys carry the same library.
MD_HD bool md_end_before(uint64_t ka, int32_t ia, uint64_t kb, int32_t ib) { return ka < kb || (ka == kb && ia < ib); }

// The pair key of two fragment keys of one library, lesser end first.
MD_HD void md_pair_key(uint64_t lesser, uint64_t greater, uint64_t& hi, uint64_t& lo) {
  hi = lesser;
  lo = greater & (((uint64_t)1 << kMdEndBits) - 1);
}

MD_HD uint64_t md_winner(uint32_t score, int32_t index) { return ((uint64_t)score << 32) | (uint32_t)~(uint32_t)index; }

}  // namespace fcs
