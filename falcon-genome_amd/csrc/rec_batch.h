// What the record-walking features (markdup.hip, bqsr.hip, depth.hip, ug.hip)
// share around their kernels.  A batch is n records over flat arrays: a CIGAR
// word range and a base range per record, by two arrays of n + 1 offsets.
//
// Host side: the offset and scalar checks of the entry points, and the
// layout-and-stage pair (over fcship_internal.h's Arena) of fcsdp_batch, fcsug_batch and
// fcsbq_batch (the same field names).  A staged batch holds only the CIGAR
// words and bases [off[0], off[n]) and keeps the caller's offsets: the device
// view's cigar / bases / qual pointers are shifted down by the first offsets.
//
// Device side: clamp64, rec_fields and block_scan_excl.  The depth and ug
// kernels take a record's two ranges from rec_fields; bq_count_kernel keeps
// them in its own order (bqsr.hip says why), and md_ends_kernel's quality
// range has a length limit of its own, so both use clamp64 alone.
#pragma once

#include <cstring>
#include <string>

#include "cigar_walk.h"
#include "fcship_internal.h"

namespace fcs {

// The n + 1 offsets of the `what` ranges into `total` elements; with max_len
// also that no record's range is longer.
inline int check_offsets(const char* who, const char* what, const int64_t* off, int64_t n, int64_t total, int64_t max_len = -1) {
  if (n > 0 && off[0] < 0) return fail_invalid(who, std::string(what) + " offsets start below zero");
  for (int64_t r = 0; r < n; ++r) {
    if (off[r + 1] < off[r]) return fail_invalid(who, std::string(what) + " offsets out of order at record " + std::to_string(r));
    if (max_len >= 0 && off[r + 1] - off[r] > max_len)
      return fail_invalid(who, "record " + std::to_string(r) + " has " + std::to_string(off[r + 1] - off[r]) + " " + what +
                                   " bytes, more than " + std::to_string(max_len));
  }
  if (n > 0 && off[n] > total)
    return fail_invalid(who, std::string(what) + " offsets end at " + std::to_string(off[n]) + ", beyond the " +
                                 std::to_string(total) + " given");
  return FCS_OK;
}

// The scalar fields of a batch, checked alike by every entry point.
template <class Batch>
int check_batch_scalars(const Batch* b, bool need_bases, const char* who) {
  if (!b) return fail_invalid(who, "null batch");
  if (b->n < 0) return fail_invalid(who, "negative record count " + std::to_string(b->n));
  if (b->n_cigar < 0 || b->n_bases < 0) return fail_invalid(who, "negative CIGAR or base size");
  bool null_array = !b->flag || !b->ref_id || !b->pos || !b->mapq || !b->cigar_off || !b->base_off || !b->qual_absent;
  if constexpr (requires { b->rg; }) null_array |= !b->rg;
  if (b->n > 0 && null_array) return fail_invalid(who, "null array");
  if ((b->n_cigar > 0 && !b->cigar) || (b->n_bases > 0 && (!b->qual || (need_bases && !b->bases))))
    return fail_invalid(who, need_bases ? "null CIGAR, base or quality bytes" : "null CIGAR or quality bytes");
  return FCS_OK;
}

// Both offset arrays of a batch of host arrays: the CIGAR ones first.
template <class Batch>
int check_batch_offsets(const Batch* b, const char* who) {
  const int rc = check_offsets(who, "CIGAR", b->cigar_off, b->n, b->n_cigar);
  return rc ? rc : check_offsets(who, "base", b->base_off, b->n, b->n_bases);
}

// Where a batch's arrays lie in a session's arenas, and the ranges staged.
struct BatchLayout {
  size_t flag, ref_id, pos, mapq, absent, coff, boff, cigar, qual, bases;
  size_t c_lo, nc, b_lo, nb;  // CIGAR words [c_lo, c_lo + nc) and bases [b_lo, b_lo + nb)
  bool with_bases;
};

// Before the session is acquired; b holds checked offsets and n > 0 records.
template <class Batch>
BatchLayout layout_batch(const Batch& b, bool with_bases, Arena& a) {
  const size_t N = (size_t)b.n;
  BatchLayout l{};
  l.c_lo = (size_t)b.cigar_off[0], l.nc = (size_t)b.cigar_off[b.n] - l.c_lo;
  l.b_lo = (size_t)b.base_off[0], l.nb = (size_t)b.base_off[b.n] - l.b_lo;
  l.with_bases = with_bases;
  l.flag = a.add(2 * N), l.ref_id = a.add(4 * N), l.pos = a.add(4 * N), l.mapq = a.add(N), l.absent = a.add(N);
  l.coff = a.add(8 * (N + 1)), l.boff = a.add(8 * (N + 1)), l.cigar = a.add(4 * l.nc), l.qual = a.add(l.nb);
  if (with_bases) l.bases = a.add(l.nb);
  return l;
}

// Copies the batch into the host arena and answers its device view.  Fields
// of Batch that the layout does not know (fcsbq_batch's rg) are the caller's.
template <class Batch>
Batch stage_batch(const Batch& b, const BatchLayout& l, char* host, char* dev) {
  const size_t N = (size_t)b.n;
  std::memcpy(host + l.flag, b.flag, 2 * N);
  std::memcpy(host + l.ref_id, b.ref_id, 4 * N);
  std::memcpy(host + l.pos, b.pos, 4 * N);
  std::memcpy(host + l.mapq, b.mapq, N);
  std::memcpy(host + l.absent, b.qual_absent, N);
  std::memcpy(host + l.coff, b.cigar_off, 8 * (N + 1));
  std::memcpy(host + l.boff, b.base_off, 8 * (N + 1));
  if (l.nc) std::memcpy(host + l.cigar, b.cigar + l.c_lo, 4 * l.nc);
  if (l.nb) std::memcpy(host + l.qual, b.qual + l.b_lo, l.nb);
  if (l.nb && l.with_bases) std::memcpy(host + l.bases, b.bases + l.b_lo, l.nb);
  Batch d = b;
  d.flag = reinterpret_cast<const uint16_t*>(dev + l.flag);
  d.ref_id = reinterpret_cast<const int32_t*>(dev + l.ref_id);
  d.pos = reinterpret_cast<const int32_t*>(dev + l.pos);
  d.mapq = reinterpret_cast<const uint8_t*>(dev + l.mapq);
  d.qual_absent = reinterpret_cast<const uint8_t*>(dev + l.absent);
  d.cigar_off = reinterpret_cast<const int64_t*>(dev + l.coff);
  d.base_off = reinterpret_cast<const int64_t*>(dev + l.boff);
  d.cigar = reinterpret_cast<const uint32_t*>(dev + l.cigar) - l.c_lo;
  d.qual = reinterpret_cast<const uint8_t*>(dev + l.qual) - l.b_lo;
  d.bases = l.with_bases ? reinterpret_cast<const uint8_t*>(dev + l.bases) - l.b_lo : nullptr;
  d.n_cigar = b.cigar_off[b.n];
  d.n_bases = b.base_off[b.n];
  return d;
}

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// The clamped CIGAR and base ranges of record r; false when a field was clamped.
template <class Batch>
__device__ __forceinline__ bool rec_fields(const Batch& b, int64_t r, int64_t& c0, int64_t& c1, int64_t& q0, int64_t& q1) {
  const int64_t k0 = b.cigar_off[r], k1 = b.cigar_off[r + 1], o0 = b.base_off[r], o1 = b.base_off[r + 1];
  c0 = clamp64(k0, 0, b.n_cigar), c1 = clamp64(k1, c0, b.n_cigar);
  q0 = clamp64(o0, 0, b.n_bases), q1 = clamp64(o1, q0, b.n_bases);
  return c0 == k0 && c1 == k1 && q0 == o0 && q1 == o1;
}

// The exclusive scan of one value per lane of a block of kWaves waves
// (wrapping), and the block's total.
template <int kWaves>
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t& total, uint32_t* wave_sums) {
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  uint32_t inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d);
    if (lane >= d) inc += up;
  }
  if (lane == 63) wave_sums[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
  for (int k = 0; k < kWaves; ++k) {
    const uint32_t s = wave_sums[k];
    if (k < wave) before += s;
    total += s;
  }
  __syncthreads();  // wave_sums may be written again
  return before + inc - v;
}

}  // namespace fcs
