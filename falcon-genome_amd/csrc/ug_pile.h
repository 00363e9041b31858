// UnifiedGenotyper, SNP model (DESIGN §2 [EXT], §4.12): what one base of one
// record adds to a locus, and what a locus's sums make of it.  One text for the
// gfx950 kernels (ug.hip) and the host check (tools/micro/ug_test.cpp);
// everything works over caller spans, one base at a time, so that a lane can
// take a base.  Every value is an integer.
//
//   ug_counted   the record filter (ref_id, CIGAR, flags, MAPQ 255)
//   ug_qe        the effective quality min(q, MAPQ, 93)
//   ug_code      the letter code of a read or reference byte (A C G T = 0 .. 3, else 4)
//   ug_is_site   the site predicate
//   ug_alt       the alt choice
//   ug_gl        the three genotype sums
// The CIGAR walks (cigar_span, cigar_site) are cigar_walk.h's.
#pragma once

#include <stdint.h>

#include "cigar_walk.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define UG_HD __host__ __device__ __forceinline__
#else
#define UG_HD inline
#endif

namespace fcs {

constexpr uint16_t kUgFlagFilter = 0x4 | 0x100 | 0x200 | 0x400;
constexpr int kUgMaxQ = 93, kUgTableRows = 94;
constexpr int kUgStatusField = 1, kUgStatusRef = 2, kUgStatusOrder = 4, kUgStatusSites = 8;

UG_HD bool ug_counted(uint16_t flag, int32_t ref_id, int64_t n_ops, uint8_t mapq) {
  return ref_id >= 0 && n_ops > 0 && (flag & kUgFlagFilter) == 0 && mapq != 255;
}

UG_HD int ug_qe(int q, int mapq) {
  const int m = mapq < kUgMaxQ ? mapq : kUgMaxQ;
  return q < m ? q : m;
}

UG_HD int ug_code(uint8_t c) {
  c &= 0xDF;  // upper case
  return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
}

// A locus of reference code r (4: not A C G T) is a site when a non-reference letter was counted.
UG_HD bool ug_is_site(int r, const uint32_t* n) {
  if (r > 3) return false;
  for (int x = 0; x < 4; ++x)
    if (x != r && n[x] > 0) return true;
  return false;
}

// The non-reference letter with the largest qsum; ties go to the smaller of A < C < G < T.
UG_HD int ug_alt(int r, const uint32_t* qsum) {
  int a = r == 0 ? 1 : 0;
  for (int x = a + 1; x < 4; ++x)
    if (x != r && qsum[x] > qsum[a]) a = x;
  return a;
}

// gl[0] ref/ref, gl[1] ref/alt, gl[2] alt/alt from the sums of the table's
// columns per letter: A = sum T[qe][0], B = sum T[qe][1], C = sum T[qe][2].
UG_HD void ug_gl(int r, int a, const int64_t* A, const int64_t* B, const int64_t* C, int64_t* gl) {
  gl[0] = A[r], gl[1] = B[r] + B[a], gl[2] = A[a];
  for (int x = 0; x < 4; ++x) {
    if (x != r) gl[0] += C[x];
    if (x != r && x != a) gl[1] += C[x];
    if (x != a) gl[2] += C[x];
  }
}

}  // namespace fcs
