// SMEM seeding on the FMD-index, restated for fixed-capacity spans so that one
// text serves the gfx950 kernels (fmd_seed.hip) and a plain host loop
// (tools/micro/fmd_smem_test.cpp): occ4, the one-base extension, bwt_smem1,
// mem_collect_intv's three rounds and the LF walk of a sampled suffix array.
// The definitions are host/fmindex.cpp's (FmdIndex::occ4 / extend / smem1 /
// collect / sa_at; [EXT] bwa bwt.c, bwamem.c), which stay the oracle: every
// SMEM field and every located position must equal theirs.
//
// No std::vector, no recursion, no dynamically indexed local array (a register
// array indexed by a run-time value becomes scratch on the device): the
// interval stacks and the output are caller-provided spans, and the selected
// extension is picked with compares inside unrolled loops.
//
// F, the fetch policy, says how a 64-byte occ line is read:
//   void counts(int64_t blk, uint64_t mask, int64_t o[4]) const
//       o[c] = B[c] + popcount(B[4 + c] & mask) of line blk (B = occ + 8 blk)
//   uint64_t word(int64_t w) const            occ[w]
// FmdHostFetch reads the line in a loop; the device's quad policy has lane c of
// a quad read B[c] and B[4 + c] and exchanges the four counts (fmd_seed.hip).
// All control state is a function of the counts and the query alone, so the
// four lanes of a quad that run this text on the same read stay uniform.
//
// Every loop is bounded by the read length or an explicit cap, whatever the
// index holds: occ4 clamps its position to [0, n], a stack push beyond the
// span's capacity or an output beyond max_out raises `overflow` (the caller
// redoes the read on the host), and the LF walk stops at max_steps or at a row
// outside [0, n).  A corrupt index gives wrong seeds, never a hang or a read
// outside the arrays.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define FMD_HD __host__ __device__ __forceinline__
#define FMD_UNROLL _Pragma("unroll")
#else
#define FMD_HD inline
#define FMD_UNROLL
#endif

namespace fcs {

// FmdIndex's BiInterval: the SA interval [k, k + s) of P, [l, l + s) of
// revcomp(P), and P's query range [qb, qe).
struct FmdIv {
  int64_t k, l, s;
  int32_t qb, qe;
};

struct FmdCollectParams {
  int32_t min_len, split_len, split_width;
  int64_t max_mem_intv;
};

template <class F>
struct FmdIx {
  F f;
  int64_t n;     // rows of the BWT (text length with $)
  const int64_t* C;  // C[c] = symbols < c, c = 0 .. 5: read where used (in memory it may be indexed by a run-time base)
};

struct FmdHostFetch {
  const uint64_t* occ;
  FMD_HD void counts(int64_t blk, uint64_t mask, int64_t o[4]) const {
    const uint64_t* B = occ + 8 * blk;
    for (int c = 0; c < 4; ++c) o[c] = (int64_t)(B[c] + (uint64_t)__builtin_popcountll(B[4 + c] & mask));
  }
  FMD_HD uint64_t word(int64_t w) const { return occ[w]; }
};

// Occurrences of A, C, G, T in BWT[0, i): zero for i <= 0, an empty mask when
// i is a multiple of 64, and the totals block for i == n.
template <class F>
FMD_HD void fmd_occ4(const FmdIx<F>& ix, int64_t i, int64_t o[4]) {
  // without a branch (the device pays registers for every level of divergent
  // control flow): for i <= 0 line 0 is read under an empty mask and the counts dropped
  const bool none = i <= 0;
  if (none) i = 0;
  if (i > ix.n) i = ix.n;  // never taken on a sound index
  ix.f.counts(i >> 6, (1ull << (i & 63)) - 1, o);
FMD_UNROLL
  for (int c = 0; c < 4; ++c) o[c] = none ? 0 : o[c];
}

// Field by field: a struct temporary would be a stack object on the device.
FMD_HD void fmd_swap(FmdIv& a, FmdIv& b) {
  const int64_t k = a.k, l = a.l, s = a.s;
  const int32_t qb = a.qb, qe = a.qe;
  a.k = b.k, a.l = b.l, a.s = b.s, a.qb = b.qb, a.qe = b.qe;
  b.k = k, b.l = l, b.s = s, b.qb = qb, b.qe = qe;
}

FMD_HD void fmd_set_intv(const int64_t* C, int c, FmdIv& iv) {  // c = 1 .. 4
  iv.k = C[c];
  iv.s = C[c + 1] - C[c];
  iv.l = C[5 - c];
}

// bwt_extend, keeping extension c (1 .. 4) of the four: backward (cP), or
// forward (index c is the backward extension of revcomp(P) by c).  o keeps
// its qb / qe.
template <class F>
FMD_HD void fmd_extend(const FmdIx<F>& ix, const FmdIv& ik, bool is_back, int c, FmdIv& o) {
  const int64_t base = is_back ? ik.k : ik.l;
  int64_t tk[4], tl[4];
  fmd_occ4(ix, base, tk);
  fmd_occ4(ix, base + ik.s, tl);
  int64_t acc = is_back ? ik.l : ik.k, same = 0, other = 0, sz = 0;
FMD_UNROLL
  for (int j = 4; j >= 1; --j) {
    const int64_t s = tl[j - 1] - tk[j - 1];
    if (j == c) same = tk[j - 1], other = acc, sz = s;
    acc += s;
  }
  same += ix.C[c];
  o.k = is_back ? same : other;
  o.l = is_back ? other : same;
  o.s = sz;
}

// What a collect call reports besides its SMEMs.
struct FmdCollectState {
  int32_t n_out = 0;       // SMEMs written to out
  int32_t max_depth = 0;   // deepest interval stack seen
  bool overflow = false;   // out or a stack was too small: the SMEMs are not complete
};

// bwt_smem1 at x with the length filter of its callers applied at emission:
// SMEMs of at least min_len bases go to out[st.n_out ...] in start order.  a0
// and a1 hold `cap` intervals each.  Returns the next start position.
template <class F>
FMD_HD int fmd_smem1(const FmdIx<F>& ix, const uint8_t* q, int len, int x, int64_t min_intv, int min_len, FmdIv* a0,
                     FmdIv* a1, int cap, FmdIv* out, int max_out, FmdCollectState& st) {
  if (q[x] > 3) return x + 1;
  if (min_intv < 1) min_intv = 1;
  FmdIv *prev = a0, *curr = a1;
  int np = 0, nc = 0;
  FmdIv ik, o;
  fmd_set_intv(ix.C, q[x] + 1, ik);
  ik.qb = 0;
  ik.qe = x + 1;
  o.k = o.l = o.s = 0;
  o.qb = o.qe = 0;
#define FMD_PUSH(v)                 \
  do {                              \
    if (nc < cap) curr[nc++] = (v); \
    else st.overflow = true;        \
  } while (0)
  int i;
  for (i = x + 1; i < len; ++i) {  // forward search: at most len rounds
    if (ik.s < min_intv) break;
    if (q[i] < 4) {
      const int c = 4 - q[i];
      fmd_extend(ix, ik, false, c, o);
      if (o.s != ik.s) {  // pushed only when the interval size changes
        FMD_PUSH(ik);
        if (o.s < min_intv) break;
      }
      ik.k = o.k, ik.l = o.l, ik.s = o.s;
      ik.qe = i + 1;
    } else {
      FMD_PUSH(ik);
      break;
    }
  }
  if (i == len) FMD_PUSH(ik);  // the match reaches the end of the query
#undef FMD_PUSH
  if (nc > st.max_depth) st.max_depth = nc;
  if (nc == 0 || st.overflow) return x + 1;  // nc == 0: min_intv above the first base's count (the host's front() of an empty list)
  for (int a = 0, b = nc - 1; a < b; ++a, --b) fmd_swap(curr[a], curr[b]);  // longest forward match first
  const int ret = curr[0].qe;
  {
    FmdIv* t = curr;
    curr = prev;
    prev = t;
    np = nc;
  }
  const int out0 = st.n_out;
  bool have_mem = false;
  int last_qb = 0;
  o.s = 0;  // the host's ok[] is zero until its first backward extension
  for (i = x - 1; i >= -1; --i) {  // backward search: x + 1 rounds over at most len intervals
    const int c = i < 0 ? -1 : q[i] < 4 ? q[i] + 1 : -1;
    nc = 0;
    int64_t last_s = 0;
    for (int j = 0; j < np; ++j) {
      const FmdIv p = prev[j];
      if (c >= 0) {
        if (ik.s >= min_intv) fmd_extend(ix, p, true, c, o);  // bwa tests ik, not p
        else o.s = 0;  // only with one interval below min_intv, before any extension
      }
      if (c < 0 || o.s < min_intv) {
        if (nc == 0) {  // no longer match in this round: p is maximal
          if (!have_mem || i + 1 < last_qb) {
            ik = p;
            ik.qb = i + 1;
            have_mem = true;
            last_qb = i + 1;
            if (ik.qe - ik.qb >= min_len) {
              if (st.n_out >= max_out) {
                st.overflow = true;
                return ret;
              }
              out[st.n_out++] = ik;
            }
          }
        }
      } else if (nc == 0 || o.s != last_s) {
        o.qb = 0;
        o.qe = p.qe;
        curr[nc++] = o;  // nc <= j: inside the span
        last_s = o.s;
      }
    }
    if (nc == 0) break;
    FmdIv* t = curr;
    curr = prev;
    prev = t;
    np = nc;
  }
  for (int a = out0, b = st.n_out - 1; a < b; ++a, --b) fmd_swap(out[a], out[b]);  // by start coordinate
  return ret;
}

// mem_collect_intv: rounds 1, 2, 3 in the host's emission order (the caller
// applies the final stable sort by (qb, qe)).  stack holds 2 * cap intervals.
template <class F>
FMD_HD void fmd_collect(const FmdIx<F>& ix, const uint8_t* q, int len, const FmdCollectParams& P, FmdIv* stack, int cap,
                        FmdIv* out, int max_out, FmdCollectState& st) {
  FmdIv *a0 = stack, *a1 = stack + cap;
  int x = 0;
  for (int it = 0; it < len && x < len && !st.overflow; ++it) {
    if (q[x] < 4) x = fmd_smem1(ix, q, len, x, 1, P.min_len, a0, a1, cap, out, max_out, st);
    else ++x;
  }
  const int n0 = st.n_out;
  for (int k = 0; k < n0 && !st.overflow; ++k) {  // re-seeding inside long SMEMs with few hits
    const FmdIv p = out[k];
    if (p.qe - p.qb < P.split_len || p.s > P.split_width) continue;
    fmd_smem1(ix, q, len, (p.qb + p.qe) >> 1, p.s + 1, P.min_len, a0, a1, cap, out, max_out, st);
  }
  if (P.max_mem_intv > 0) {  // bwt_seed_strategy1
    x = 0;
    for (int it = 0; it < len && x < len && !st.overflow; ++it) {
      if (q[x] > 3) {
        ++x;
        continue;
      }
      FmdIv ik, o;
      fmd_set_intv(ix.C, q[x] + 1, ik);
      int next = len;
      for (int i = x + 1; i < len; ++i) {  // at most len rounds per start
        if (q[i] > 3) {
          next = i + 1;
          break;
        }
        fmd_extend(ix, ik, false, 4 - q[i], o);
        if (o.s < P.max_mem_intv && i - x >= P.min_len) {
          if (o.s > 0) {
            if (st.n_out >= max_out) {
              st.overflow = true;
              break;
            }
            o.qb = x;
            o.qe = i + 1;
            out[st.n_out++] = o;
          }
          next = i + 1;
          break;
        }
        ik.k = o.k, ik.l = o.l, ik.s = o.s;
      }
      x = next;
    }
  }
}

// FmdIndex::sa_at: SA[row] by LF steps back to a sampled row (row % sa_intv
// == 0) or to a stored special row (its BWT symbol is $ or a separator;
// special = (row, SA) pairs sorted by row).  Status of the walk:
enum : int {
  kFmdLocated = 0,
  kFmdStepCap = 1,   // max_steps LF steps without reaching a stored row
  kFmdBadRow = 2,    // a row outside [0, n), or a special row missing from the table
};
template <class F>
FMD_HD int fmd_sa_walk(const FmdIx<F>& ix, const uint64_t* sa, int64_t n_sa, int32_t sa_intv, const int64_t* special,
                       int64_t n_special, int64_t row, int32_t max_steps, int64_t& pos, int32_t& steps_out) {
  int32_t steps = 0;
  pos = -1;
  steps_out = 0;
  for (;;) {
    if (row < 0 || row >= ix.n) return kFmdBadRow;
    if (row % sa_intv == 0) {
      if (row / sa_intv >= n_sa) return kFmdBadRow;
      pos = (int64_t)sa[row / sa_intv] + steps;
      steps_out = steps;
      return kFmdLocated;
    }
    const int64_t blk = row >> 6;
    const uint64_t bit = 1ull << (row & 63);
    int c = -1;
    uint64_t wc = 0;
FMD_UNROLL
    for (int k = 0; k < 4; ++k) {
      const uint64_t w = ix.f.word(8 * blk + 4 + k);
      if (w & bit) c = k, wc = w;
    }
    if (c < 0) {  // $ or a separator precedes this suffix: stored
      int64_t lo = 0, hi = n_special;
      while (lo < hi) {  // at most 64 rounds
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (special[2 * mid] < row) lo = mid + 1;
        else hi = mid;
      }
      if (lo >= n_special || special[2 * lo] != row) return kFmdBadRow;
      pos = special[2 * lo + 1] + steps;
      steps_out = steps;
      return kFmdLocated;
    }
    if (steps >= max_steps) return kFmdStepCap;
    row = ix.C[c + 1] + (int64_t)(ix.f.word(8 * blk + c) + (uint64_t)__builtin_popcountll(wc & (bit - 1)));
    ++steps;
  }
}

}  // namespace fcs
