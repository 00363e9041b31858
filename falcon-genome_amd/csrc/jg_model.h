// GenotypeGVCFs, round 20 (DESIGN §2 [EXT], §4.13): the integer rules of joint
// genotyping over one-sample GVCF records.  One text for the gfx950 kernels
// (joint.hip), the host oracle (host/joint.cpp) and tools/micro/jg_test.cpp.
// Every value is an integer; the unit of a log value is 2^-20 of a PL
// (10 log10), larger = more likely.
//
//   jg_lse        the table log-sum of two values
//   jg_cell       one cell z_j[k] of the exact allele-frequency recurrence
//   jg_own        a merged allele's index among a record's own alleles
//   jg_collapse   a record's PLs as c0, c1, c2 of one ALT, minimum subtracted
//   jg_source     a sample's source record at a site
//   jg_genotype   a sample's PLs, GT and GQ over REF and the kept ALTs
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JG_HD __host__ __device__ __forceinline__
#else
#define JG_HD inline
#endif

namespace fcs {

constexpr int kJgUnitBits = 20;                                 // 2^-20 PL
constexpr int kJgAltsMax = 6;                                   // FCSJG_ALTS_MAX
constexpr int kJgPlMax = (1 << 20) - 1;                         // FCSJG_PL_MAX
constexpr int kJgSRows = 1282;                                  // S[i], i = d >> 16, d < 80 PL, and the two rows the last step reads
constexpr int64_t kJgCut = (int64_t)80 << kJgUnitBits;          // beyond it the maximum alone
constexpr int kJgGenotypesMax = (kJgAltsMax + 1) * (kJgAltsMax + 2) / 2;  // 28
constexpr int kJgKindBlock = 0, kJgKindCall = 1;
constexpr int kJgNoCall = 255;
constexpr int kJgStatusField = 1, kJgStatusPl = 2;

JG_HD int64_t jg_lse(int64_t a, int64_t b, const int32_t* S) {
  const int64_t hi = a > b ? a : b, d = hi - (a > b ? b : a);
  if (d >= kJgCut) return hi;
  const int i = (int)(d >> 16);
  const int64_t f = d & 0xFFFF;
  const int64_t s0 = S[i], s1 = S[i + 1];  // S decreases: the product below is not negative
  return hi + s0 - (((s0 - s1) * f) >> 16);
}

// z_j[k] for 0 <= k <= 2j, j >= 1, from row j - 1 at k (z0), k - 1 (z1) and
// k - 2 (z2); a term whose coefficient is zero is absent and its z is not read.
// LG holds at least 4j entries (the middle coefficient is LG[2k] + LG[2j - k]).
JG_HD int64_t jg_cell(int j, int k, int64_t z0, int64_t z1, int64_t z2, int64_t g0, int64_t g1, int64_t g2,
                      const int32_t* LG, const int32_t* S) {
  const int m = 2 * j - k;
  bool have = false;
  int64_t acc = 0;
  if (m >= 2) acc = z0 + g0 + LG[m] + LG[m - 1], have = true;
  if (k >= 1 && m >= 1) {
    const int64_t t = z1 + g1 + LG[2 * k] + LG[m];
    acc = have ? jg_lse(acc, t, S) : t, have = true;
  }
  if (k >= 2) {
    const int64_t t = z2 + g2 + LG[k] + LG[k - 1];
    acc = have ? jg_lse(acc, t, S) : t;
  }
  return acc - ((int64_t)LG[2 * j] + LG[2 * j - 1]);
}

// The own allele of merged allele x (0: REF, 1 .. n_alt): a block's are {REF,
// <NON_REF>}; a call's are {REF, its ALT (merged index alt; 0: cut), <NON_REF>}.
JG_HD int jg_own(int kind, int alt, int x) { return x == 0 ? 0 : kind == kJgKindBlock ? 1 : x == alt ? 1 : 2; }

// PLs are in VCF genotype order: {a, b}, a <= b, at b (b + 1) / 2 + a.
JG_HD int jg_pl_index(int a, int b) { return a <= b ? b * (b + 1) / 2 + a : a * (a + 1) / 2 + b; }

JG_HD int32_t jg_clamp_pl(int32_t v) { return v < 0 ? 0 : v > kJgPlMax ? kJgPlMax : v; }

// A record's six PLs, clamped, in registers: at() is a chain of selects, so
// that an index computed from alleles costs no indexed memory.
struct JgPl {
  int32_t v0, v1, v2, v3, v4, v5;
  bool clamped;
  JG_HD int32_t at(int i) const { return i == 0 ? v0 : i == 1 ? v1 : i == 2 ? v2 : i == 3 ? v3 : i == 4 ? v4 : v5; }
};

// p: the record's six values; a block's last three are not looked at.
JG_HD JgPl jg_load_pl(const int32_t* p, int kind) {
  JgPl r;
  const bool six = kind != kJgKindBlock;
  r.v0 = jg_clamp_pl(p[0]), r.v1 = jg_clamp_pl(p[1]), r.v2 = jg_clamp_pl(p[2]);
  r.v3 = six ? jg_clamp_pl(p[3]) : 0, r.v4 = six ? jg_clamp_pl(p[4]) : 0, r.v5 = six ? jg_clamp_pl(p[5]) : 0;
  r.clamped = r.v0 != p[0] || r.v1 != p[1] || r.v2 != p[2] || (six && (r.v3 != p[3] || r.v4 != p[4] || r.v5 != p[5]));
  return r;
}

// c[0], c[1], c[2]: the smallest merged PL with no, one and two copies of ALT
// i (1 .. n_alt), minus the smallest of the three.
JG_HD void jg_collapse(int kind, int alt, int n_alt, int i, const JgPl& pl, int32_t* c) {
  const int oi = jg_own(kind, alt, i);
  int32_t c0 = INT32_MAX, c1 = INT32_MAX;
  for (int x = 0; x <= n_alt; ++x) {
    if (x == i) continue;
    const int ox = jg_own(kind, alt, x);
    const int32_t one = pl.at(jg_pl_index(ox, oi));
    c1 = one < c1 ? one : c1;
    for (int y = x; y <= n_alt; ++y) {
      if (y == i) continue;
      const int32_t none = pl.at(jg_pl_index(ox, jg_own(kind, alt, y)));
      c0 = none < c0 ? none : c0;
    }
  }
  const int32_t c2 = pl.at(jg_pl_index(oi, oi));
  const int32_t m = c0 < c1 ? (c0 < c2 ? c0 : c2) : (c1 < c2 ? c1 : c2);
  c[0] = c0 - m, c[1] = c1 - m, c[2] = c2 - m;
}

// The source of a sample whose records are [lo, hi) at site p: the last record
// with beg <= p, on equal beg the first; -1 (no call) without one, when p is at
// or beyond its end, or when it is a call that began before p.
JG_HD int64_t jg_source(const int32_t* beg, const int32_t* end, const uint8_t* kind, int64_t lo, int64_t hi, int32_t p) {
  int64_t a = lo, b = hi;
  while (a < b) {  // the first record with beg > p
    const int64_t mid = a + (b - a) / 2;
    if (beg[mid] > p) b = mid;
    else a = mid + 1;
  }
  if (a == lo) return -1;
  const int32_t at = beg[a - 1];
  int64_t c = lo;
  b = a - 1;
  while (c < b) {  // the first record with beg >= at
    const int64_t mid = c + (b - c) / 2;
    if (beg[mid] >= at) b = mid;
    else c = mid + 1;
  }
  if (p >= end[c]) return -1;
  if (kind[c] != kJgKindBlock && at < p) return -1;
  return c;
}

// The kept alleles of a site, four bits each: nibble 0 = REF, then the ALTs of
// the mask in order; K, the number of kept ALTs, through the pointer.
JG_HD uint32_t jg_kept(int mask, int* K) {
  uint32_t a = 0;
  int n = 0;
  for (int i = 1; i <= kJgAltsMax; ++i)
    if (mask >> (i - 1) & 1) a |= (uint32_t)i << (4 * ++n);
  *K = n;
  return a;
}

JG_HD int jg_kept_at(uint32_t a, int x) { return (int)(a >> (4 * x) & 15u); }

// A sample's PLs over the genotypes of REF and the K kept ALTs (jg_kept's a),
// in VCF order, minus their minimum, through out(g, value); gt: the first
// minimum as merged alleles, gq = min(99, the second smallest).  False (gt = no
// call, gq = 0) when all the PLs are equal.
template <class Out>
JG_HD bool jg_genotype(int kind, int alt, const JgPl& pl, uint32_t a, int K, Out&& out, int* gt, int* gq) {
  int32_t lo = INT32_MAX, hi = -1;
  for (int y = 0; y <= K; ++y)
    for (int x = 0; x <= y; ++x) {
      const int32_t v = pl.at(jg_pl_index(jg_own(kind, alt, jg_kept_at(a, x)), jg_own(kind, alt, jg_kept_at(a, y))));
      lo = v < lo ? v : lo, hi = v > hi ? v : hi;
    }
  int32_t second = INT32_MAX;
  bool first = false;
  int g = 0, g0 = kJgNoCall, g1 = kJgNoCall;
  for (int y = 0; y <= K; ++y)
    for (int x = 0; x <= y; ++x, ++g) {
      const int32_t v = pl.at(jg_pl_index(jg_own(kind, alt, jg_kept_at(a, x)), jg_own(kind, alt, jg_kept_at(a, y)))) - lo;
      out(g, v);
      if (v == 0 && !first) first = true, g0 = jg_kept_at(a, x), g1 = jg_kept_at(a, y);
      else second = v < second ? v : second;
    }
  const bool called = lo != hi;
  gt[0] = called ? g0 : kJgNoCall, gt[1] = called ? g1 : kJgNoCall;
  *gq = !called ? 0 : second < 99 ? (int)second : 99;
  return called;
}

}  // namespace fcs
