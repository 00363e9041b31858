// The pileup in front of htc's and mutect2's PairHMM: what one
// aligned base of one read adds to its locus, and when a locus is an active
// site.  One text for the gfx950 kernels (pileup.hip) and the host statement
// (host/pileup.cpp); every decision is taken per base, so that a lane can own a
// locus.  Letters are compared as bytes: a lower-case reference letter differs
// from every read letter.
//
//   pu_counted   the base's quality reaches min_bq
//   pu_nonref    the read letter differs from the reference letter, neither is N
//   pu_row       the table row of a quality, min(bq, 93)
//   pu_col       which of a row's three entries goes to which gl slot
//   pu_active    the site predicate over a locus's events and depth
//   pu_letter    the count slot of a read letter (A C G T = 0 .. 3, N = 4, else 5)
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PU_HD __host__ __device__ __forceinline__
#else
#define PU_HD inline
#endif

namespace fcs {

constexpr int kPuMaxQ = 93, kPuTableRows = 94;
constexpr int kPuStatusField = 1, kPuStatusRef = 2, kPuStatusOrder = 4, kPuStatusSites = 8, kPuStatusSnvs = 16,
              kPuStatusLetter = 32;
constexpr int kPuMinSupport = 2;  // reads an SNV needs to be listed, events a site needs

PU_HD bool pu_counted(int bq, int min_bq) { return bq >= min_bq; }

PU_HD bool pu_nonref(char b, char r) { return b != r && r != 'N' && b != 'N'; }

PU_HD int pu_row(int bq) { return bq < kPuMaxQ ? bq : kPuMaxQ; }

// gl[slot] takes t[pu_col(nonref, slot)] of the base's row t: [0] a reference
// base under 0/0, [1] any base under 0/1, [2] a non-reference base under 0/0.
PU_HD int pu_col(bool nonref, int slot) { return slot == 1 ? 1 : (slot == 0) == nonref ? 2 : 0; }

PU_HD bool pu_active(int ev, int depth, double frac) {
  const int dp = depth > 1 ? depth : 1;
  return ev >= kPuMinSupport && ev >= frac * dp;
}

PU_HD int pu_letter(uint8_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : b == 'N' ? 4 : 5; }

}  // namespace fcs
