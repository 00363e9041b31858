// From a read's SMEMs (fmd_smem.h's fmd_collect, in emission order) to what
// chain_read consumes: the SMEMs in bwa's final order and the BWT rows of the
// occurrences it samples.  One text for the gfx950 kernels (fmd_seeds.hip) and
// a plain host loop (tools/micro/fmd_expand_test.cpp).
//
// Order: the stable sort by (qb, qe) mem_collect_intv ends with, written as a
// rank: SMEM i goes to position #{j : key_j < key_i, or key_j == key_i and
// j < i}.  The key packs (qb, qe) into one 64-bit word, and the emission index
// is the SMEM's slot, so the ranks of k SMEMs are a permutation of 0 .. k - 1
// whatever the slots hold.
//
// Rows: bwa's loop over an SMEM's occurrences,
//   step = s > max_occ ? s / max_occ : 1;
//   for (j = 0, kept = 0; j < s && kept < max_occ; j += step, ++kept) row k + j
// keeps exactly min(s, max_occ) rows (step * (max_occ - 1) < s when s >
// max_occ), so the counts are known before any row is written.  SMEM i's rows
// start at the sum of the counts of the SMEMs ranked before it (its in-read
// offset), which the same pass over the keys accumulates.
//
// No dynamically indexed local array and no struct temporary (see
// fmd_smem.h); every loop is bounded by a count its caller has clamped.
#pragma once

#include "fmd_smem.h"

namespace fcs {

// (qb, qe) as one word that compares as the pair does.  qb, qe >= 0.
FMD_HD uint64_t fmd_seed_key(int32_t qb, int32_t qe) { return ((uint64_t)(uint32_t)qb << 32) | (uint32_t)qe; }

// SMEM (ka, ia) sorts before SMEM (kb, ib): the stable order.
FMD_HD bool fmd_seed_before(uint64_t ka, int32_t ia, uint64_t kb, int32_t ib) {
  return ka < kb || (ka == kb && ia < ib);
}

// Rows bwa's sampling loop keeps of an interval of s rows: min(s, max_occ).
FMD_HD int32_t fmd_seed_count(int64_t s, int32_t max_occ) {
  return s <= 0 ? 0 : s < (int64_t)max_occ ? (int32_t)s : max_occ;
}

FMD_HD int64_t fmd_seed_step(int64_t s, int32_t max_occ) { return s > (int64_t)max_occ ? s / max_occ : 1; }

// Where an SMEM goes: its position in the sorted list and the rows before its own.
struct FmdSeedPlace {
  int32_t rank;
  int32_t pad;
  int64_t row0;
};

// Adds what the SMEMs base .. base + n - 1 (keys[j], counts[j] for j < n)
// contribute to the place of SMEM i with key `key`.  Called once over the whole
// list (host) or once per staged tile (device).
FMD_HD void fmd_seed_rank_span(uint64_t key, int32_t i, int32_t base, int32_t n, const uint64_t* keys,
                               const int32_t* counts, int32_t& rank, int64_t& row0) {
  for (int32_t j = 0; j < n; ++j) {
    const bool before = fmd_seed_before(keys[j], base + j, key, i);
    rank += before ? 1 : 0;
    row0 += before ? (int64_t)counts[j] : 0;
  }
}

// The sampled rows of [k, k + s) to dst[at ...], `count` of them
// (fmd_seed_count), none at or beyond cap.  encode: as -1 - row, the form of a
// position that is still to be looked up.
FMD_HD void fmd_seed_rows(int64_t k, int64_t s, int32_t max_occ, int32_t count, bool encode, int64_t* dst, int64_t at,
                          int64_t cap) {
  const int64_t step = fmd_seed_step(s, max_occ);
  for (int32_t kept = 0; kept < count; ++kept) {
    const int64_t w = at + kept, row = k + (int64_t)kept * step;
    if (w >= 0 && w < cap) dst[w] = encode ? -1 - row : row;
  }
}

}  // namespace fcs
