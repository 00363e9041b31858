// The two walks over a record's CIGAR words (len << 4 | op) that depth
// (dp_runs.h) and ug (ug_pile.h) share, one text for the gfx950 kernels, the
// checks of the entry points before the device and the host programs under
// tools/micro.
//
//   cigar_span   the read bases the CIGAR covers, the reference span, and
//                whether an aligned base lies outside its contig
//   cigar_site   whether read base i is aligned (M / = / X), and where
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CW_HD __host__ __device__ __forceinline__
#else
#define CW_HD inline
#endif

namespace fcs {

// One pass over the record's n_ops CIGAR words: the read bases of S / M / I /
// = / X, the reference bases of M / D / N / = / X, and whether an aligned base
// lies outside [0, clen) when the record starts at pos.
CW_HD void cigar_span(const uint32_t* cigar, int64_t n_ops, int64_t pos, int64_t clen, int64_t& covered, int64_t& ref_len,
                      bool& beyond) {
  covered = ref_len = 0;
  beyond = false;
  for (int64_t k = 0; k < n_ops; ++k) {
    const uint32_t op = cigar[k] & 15u;
    const int64_t len = (int64_t)(cigar[k] >> 4);
    if (op == 0u || op == 1u || op == 4u || op == 7u || op == 8u) covered += len;
    if ((op == 0u || op == 7u || op == 8u) && len > 0 && (pos + ref_len < 0 || pos + ref_len + len > clen)) beyond = true;
    if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) ref_len += len;
  }
}

// The same pass without the bounds test, for dp_runs_kernel, which finds
// "beyond" per base.  A walk of its own: calling the one above and dropping
// `beyond` keeps that kernel's registers but not its machine code.
CW_HD void cigar_span(const uint32_t* cigar, int64_t n_ops, int64_t& covered, int64_t& ref_len) {
  covered = ref_len = 0;
  for (int64_t k = 0; k < n_ops; ++k) {
    const uint32_t op = cigar[k] & 15u;
    const int64_t len = (int64_t)(cigar[k] >> 4);
    if (op == 0u || op == 1u || op == 4u || op == 7u || op == 8u) covered += len;
    if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) ref_len += len;
  }
}

// Read base i (0 <= i < covered): true, with its reference position in p, when it lies in M, = or X.
CW_HD bool cigar_site(const uint32_t* cigar, int64_t n_ops, int64_t pos, int64_t i, int64_t& p) {
  int64_t q = 0, r = pos;
  for (int64_t k = 0; k < n_ops; ++k) {
    const uint32_t op = cigar[k] & 15u;
    const int64_t len = (int64_t)(cigar[k] >> 4);
    if (op == 0u || op == 7u || op == 8u) {
      if (i < q + len) {
        p = r + (i - q);
        return true;
      }
      q += len, r += len;
    } else if (op == 1u || op == 4u) {
      if (i < q + len) break;
      q += len;
    } else if (op == 2u || op == 3u) {
      r += len;
    }
  }
  p = 0;
  return false;
}

}  // namespace fcs
