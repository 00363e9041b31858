// The pileup in front of htc's and mutect2's PairHMM on the device
// (include/fcspu.h).  The per-base rules are csrc/pu_rules.h, one
// text for these kernels and host/pileup.cpp.  All work of a call is queued on
// one stream, without a host round trip.
//
// The pass is a gather: a lane owns a locus and a wave 64 consecutive loci, so
// that a locus's three sums in double are added read after read in the order of
// the batch, as the host adds them, and equal the host's bit for bit.  Depth,
// events, the four letter counts and the three sums are lane registers; the
// pass has no atomic in it but the status word's, and no result depends on
// scheduling.  The sums are additions only and the library is built with
// -ffp-contract=off and without any fast-math flag, so nothing fuses or
// reassociates them; the table comes from the host, so no device log10 is
// involved.
//
// pu_span_kernel: a lane per record: the clamped fields, one CIGAR pass for the
// covered bases, the reference end and "an aligned base beyond the contig";
// end[r] (or "adds nothing") and the position key of the records of the
// window's contig, and the maxima of both per 256 records.
// pu_span_kernel is built for 8 waves per SIMD.
//
// pu_offsets_kernel, pu_scan_kernel: the running maximum of the ends and of the
// positions over the records, in tiles of 256: the tiles' maxima scanned by one
// block, then every tile from its offset.  A position below the running
// maximum before it sets the order bit.  The running maximum of the ends does
// not decrease, so the first record a tile needs is found by binary search
// whatever a record spans (a 100 kbp N op included), without a max_span.
// pu_offsets_kernel is built for 8 waves per SIMD.
// pu_scan_kernel is built for 8 waves per SIMD.
//
// pu_pile_kernel: a block takes tiles of 256 loci in a block stride, a wave 64
// of them.  Per batch the wave's records are [lo, hi): lo the first whose
// running-maximum end lies beyond the wave's first locus, hi the first whose
// position reaches its end.  The record index, the record's fields and the
// CIGAR word are wave-uniform (the wave index is read as a scalar): they are
// loaded at one address for the whole wave and the walk's state lives in scalar
// registers; per lane there is a range test, one quality byte, one base byte,
// one table row from LDS and three double adds.  Then the lane writes its
// locus: depth, events, gl, the four counts and the site mark, and the block
// the tile's numbers of sites and SNVs.
// pu_pile_kernel is built for 7 waves per SIMD.
//
// pu_slots_kernel: the exclusive scans of the tiles' site and SNV counts by one
// block, the totals and the "more than the maximum" bits.
// pu_slots_kernel is built for 8 waves per SIMD.
//
// pu_emit_kernel: a lane per locus writes its site and its SNVs at the tile's
// slot plus its rank in the tile, so both lists ascend.
// pu_emit_kernel is built for 8 waves per SIMD.
//
// Every loop is bounded by n, a record's clamped CIGAR word count, len, or the
// tile count; no kernel uses scratch.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "fcship_internal.h"
#include "fcspu.h"
#include "pu_rules.h"
#include "rec_batch.h"

namespace fcs {

namespace {

constexpr int kPuBlock = 256;
constexpr int kPuWaves = kPuBlock / 64;
constexpr int kPuTile = FCSPU_TILE;
constexpr int kPuMaxBlocks = 2048;
constexpr int kPuTableWords = kPuTableRows * 3;
constexpr int64_t kPuNone = INT64_MIN;  // end[r] of a record that adds nothing; the key of a record of another contig

static_assert(kPuTile == kPuBlock, "a lane per locus of a tile");
static_assert(FCSPU_TABLE_ROWS == kPuTableRows, "fcspu.h and pu_rules.h");
static_assert(FCSPU_STATUS_FIELD == kPuStatusField && FCSPU_STATUS_REF == kPuStatusRef && FCSPU_STATUS_ORDER == kPuStatusOrder &&
                  FCSPU_STATUS_SITES == kPuStatusSites && FCSPU_STATUS_SNVS == kPuStatusSnvs &&
                  FCSPU_STATUS_LETTER == kPuStatusLetter,
              "fcspu.h and pu_rules.h");
static_assert(sizeof(fcspu_snv) == 12 && sizeof(fcspu_params) == 16, "device layouts");

__device__ __forceinline__ int64_t pu_max64(int64_t a, int64_t b) { return a > b ? a : b; }

// The inclusive running maximum of one value per lane of the block, and the
// block's maximum (ug.hip scans its records' ends the same way).
__device__ __forceinline__ int64_t pu_block_max_incl(int64_t v, int64_t& total, int64_t* wave_max) {
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  int64_t inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t up = __shfl_up(inc, d);
    if (lane >= d) inc = pu_max64(inc, up);
  }
  if (lane == 63) wave_max[wave] = inc;
  __syncthreads();
  total = kPuNone;
  for (int k = 0; k < kPuWaves; ++k) {
    const int64_t s = wave_max[k];
    if (k < wave) inc = pu_max64(inc, s);
    total = pu_max64(total, s);
  }
  __syncthreads();  // wave_max may be written again
  return inc;
}

__global__ __launch_bounds__(kPuBlock) void pu_span_kernel(fcspu_batch b, fcspu_window w, int64_t n_rtiles,
                                                           int64_t* __restrict__ end, int64_t* __restrict__ key,
                                                           int64_t* __restrict__ tile_end, int64_t* __restrict__ tile_key,
                                                           int32_t* __restrict__ status) {
  __shared__ int64_t wave_max[kPuWaves];
  for (int64_t t = blockIdx.x; t < n_rtiles; t += gridDim.x) {
    const int64_t r = t * kPuBlock + (int64_t)threadIdx.x;
    int64_t e = kPuNone, kp = kPuNone;
    if (r < b.n && b.ref_id[r] == w.ref_id) {
      const int64_t pos = b.pos[r];
      kp = pos;
      int64_t c0, c1, q0, q1;
      bool bad = !rec_fields(b, r, c0, c1, q0, q1);
      bool beyond = false;
      int64_t ref_len = 0;
      if (!bad) {
        int64_t covered;
        cigar_span(b.cigar + c0, c1 - c0, pos, w.contig_len, covered, ref_len, beyond);
        bad = covered != q1 - q0;
      }
      if (bad) {
        atomicOr(status, kPuStatusField);
      } else {
        e = pos + ref_len;
        if (beyond) atomicOr(status, kPuStatusRef);
      }
    }
    if (r < b.n) end[r] = e, key[r] = kp;
    int64_t te, tk;
    (void)pu_block_max_incl(e, te, wave_max);
    (void)pu_block_max_incl(kp, tk, wave_max);
    if (threadIdx.x == 0) tile_end[t] = te, tile_key[t] = tk;
  }
}

// tile_end and tile_key become the maxima of all earlier tiles.
__global__ __launch_bounds__(kPuBlock) void pu_offsets_kernel(int64_t* __restrict__ tile_end, int64_t* __restrict__ tile_key,
                                                              int64_t n_rtiles) {
  __shared__ int64_t wave_max[kPuWaves];
  __shared__ int64_t last_e[kPuWaves], last_k[kPuWaves];
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  int64_t carry_e = kPuNone, carry_k = kPuNone;
  for (int64_t t0 = 0; t0 < n_rtiles; t0 += kPuBlock) {
    const int64_t t = t0 + (int64_t)threadIdx.x;
    const int64_t ve = t < n_rtiles ? tile_end[t] : kPuNone, vk = t < n_rtiles ? tile_key[t] : kPuNone;
    int64_t te, tk;
    const int64_t ie = pu_block_max_incl(ve, te, wave_max), ik = pu_block_max_incl(vk, tk, wave_max);
    // exclusive: the inclusive maximum of the lane before
    const int64_t pe = __shfl_up(ie, 1), pk = __shfl_up(ik, 1);
    if (lane == 63) last_e[wave] = ie, last_k[wave] = ik;
    __syncthreads();
    const int64_t xe = lane ? pe : wave ? last_e[wave - 1] : kPuNone, xk = lane ? pk : wave ? last_k[wave - 1] : kPuNone;
    if (t < n_rtiles) tile_end[t] = pu_max64(carry_e, xe), tile_key[t] = pu_max64(carry_k, xk);
    carry_e = pu_max64(carry_e, te), carry_k = pu_max64(carry_k, tk);
    __syncthreads();  // last_e and last_k may be written again
  }
}

// max_end[r]: the running maximum of end[0 .. r].  key[r] becomes the running
// maximum of the keys [0 .. r]; a key below the maximum before it is out of order.
__global__ __launch_bounds__(kPuBlock) void pu_scan_kernel(const int64_t* __restrict__ end, int64_t* __restrict__ key, int64_t n,
                                                           int64_t n_rtiles, const int64_t* __restrict__ tile_end,
                                                           const int64_t* __restrict__ tile_key, int64_t* __restrict__ max_end,
                                                           int32_t* __restrict__ status) {
  __shared__ int64_t wave_max[kPuWaves];
  __shared__ int64_t last_k[kPuWaves];
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  for (int64_t t = blockIdx.x; t < n_rtiles; t += gridDim.x) {
    const int64_t r = t * kPuBlock + (int64_t)threadIdx.x;
    const int64_t e = r < n ? end[r] : kPuNone, kp = r < n ? key[r] : kPuNone;
    int64_t unused;
    const int64_t ie = pu_block_max_incl(e, unused, wave_max), ik = pu_block_max_incl(kp, unused, wave_max);
    const int64_t pk = __shfl_up(ik, 1);
    if (lane == 63) last_k[wave] = ik;
    __syncthreads();
    const int64_t before = pu_max64(tile_key[t], lane ? pk : wave ? last_k[wave - 1] : kPuNone);
    if (r < n) {
      max_end[r] = pu_max64(tile_end[t], ie);
      key[r] = pu_max64(tile_key[t], ik);
      if (kp != kPuNone && kp < before) atomicOr(status, kPuStatusOrder);
    }
    __syncthreads();  // last_k may be written again
  }
}

// The first r in [0, n) with v[r] > x (strict) or v[r] >= x, v non-decreasing; n without one.
__device__ __forceinline__ int64_t pu_first(const int64_t* __restrict__ v, int64_t n, int64_t x, bool strict) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    const int64_t m = v[mid];
    if (strict ? m > x : m >= x) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// A batch's scanned records in the workspace.
struct PuRecs {
  const int64_t *end, *max_end, *key;
};

struct PuPileArgs {
  fcspu_batch b0, b1;
  PuRecs r0, r1;
  int32_t n_batches;
  fcspu_params prm;
  fcspu_window w;
  const uint8_t* ref;
  const double* table;
  const int32_t* events_in;
  int32_t *depth, *events;
  double* gl;
  int32_t* cnt;   // [4][len]: the letters' non-reference counts
  uint8_t* site;  // [len]
  uint32_t *tile_sites, *tile_snvs;
  int64_t n_tiles;
  int32_t* status;
  unsigned long long* bad;  // nullable: the least (batch << 40 | record) with a letter that is refused
};

// What a lane keeps of its locus.
struct PuLocus {
  int depth = 0, events = 0;
  int a = 0, c = 0, g = 0, t = 0;
  double g0 = 0.0, g1 = 0.0, g2 = 0.0;
};

// The batch's records that reach the wave's loci [s, e), in batch order, and
// each record's CIGAR words in order; the lane's locus is p, its reference
// letter r.  Everything but p, r and L is wave-uniform.
template <bool kGl>
__device__ __forceinline__ void pu_walk(const fcspu_batch& b, const PuRecs& rs, int batch, int min_bq, const double* tab, int64_t s,
                                        int64_t e, int64_t p, char r, PuLocus& L, int32_t* status, unsigned long long* bad) {
  const int64_t lo = pu_first(rs.max_end, b.n, s, true), hi = pu_first(rs.key, b.n, e, false);
  for (int64_t rec = lo; rec < hi; ++rec) {
    const int64_t ev = rs.end[rec];
    if (ev == kPuNone || ev <= s) continue;
    const int64_t pos = b.pos[rec];
    if (pos >= e) continue;
    int64_t c0, c1, q0, q1;
    (void)rec_fields(b, rec, c0, c1, q0, q1);  // pu_span_kernel refused the record (ev == kPuNone) if a field was clamped
    int64_t rp = pos, q = q0;
    for (int64_t k = c0; k < c1 && rp < e; ++k) {
      const uint32_t word = b.cigar[k];
      const uint32_t op = word & 15u;
      const int64_t len = (int64_t)(word >> 4);
      const bool mine = p >= rp && p < rp + len && p < e;
      if (op == 0u || op == 7u || op == 8u) {
        if (mine) {
          const int64_t qi = q + (p - rp);  // < q1: the CIGAR covers exactly the record's q1 - q0 bases
          const int bq = b.qual[qi];
          if (pu_counted(bq, min_bq)) {
            const uint8_t letter = b.bases[qi];
            const int x = pu_letter(letter);
            if (x > 4) {
              atomicOr(status, kPuStatusLetter);
              if (bad) atomicMin(bad, ((unsigned long long)batch << 40) | (unsigned long long)rec);
            } else {
              ++L.depth;
              const bool nonref = pu_nonref((char)letter, r);
              if (nonref) {
                ++L.events;
                L.a += x == 0, L.c += x == 1, L.g += x == 2, L.t += x == 3;
              }
              if (kGl) {
                const double* t = tab + 3 * pu_row(bq);
                L.g0 += t[pu_col(nonref, 0)];
                L.g1 += t[pu_col(nonref, 1)];
                L.g2 += t[pu_col(nonref, 2)];
              }
            }
          }
        }
        rp += len, q += len;
      } else if (op == 1u || op == 4u) {
        q += len;
      } else if (op == 2u) {
        if (mine) ++L.depth;  // a deleted locus counts whatever the neighbours' qualities
        rp += len;
      } else if (op == 3u) {
        rp += len;
      }
    }
  }
}

__global__ __launch_bounds__(kPuBlock) void pu_pile_kernel(PuPileArgs a) {
  __shared__ double tab[kPuTableWords];
  __shared__ uint32_t wave_sums[kPuWaves];
  const int tid = (int)threadIdx.x, lane = tid % 64;
  const int wave = __builtin_amdgcn_readfirstlane(tid / 64);
  if (*a.status & kPuStatusOrder) return;
  for (int k = tid; k < kPuTableWords; k += kPuBlock) tab[k] = a.table[k];
  __syncthreads();
  const int64_t w_end = a.w.start + a.w.len;
  const bool want_gl = a.prm.want_gl != 0;
  for (int64_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
    const int64_t s = a.w.start + t * kPuTile + (int64_t)wave * 64;
    const int64_t e = s + 64 < w_end ? s + 64 : w_end;
    const int64_t p = s + lane, off = p - a.w.start;
    const bool live = p < e;
    const char r = live ? (char)a.ref[off] : 'N';
    PuLocus L;
    int d0 = 0, e0 = 0;
    if (s < e) {
      if (want_gl) pu_walk<true>(a.b0, a.r0, 0, a.prm.min_bq, tab, s, e, p, r, L, a.status, a.bad);
      else pu_walk<false>(a.b0, a.r0, 0, a.prm.min_bq, tab, s, e, p, r, L, a.status, a.bad);
      d0 = L.depth, e0 = L.events;
      if (a.n_batches > 1) pu_walk<false>(a.b1, a.r1, 1, a.prm.min_bq, tab, s, e, p, r, L, a.status, a.bad);
    }
    bool site = false;
    uint32_t n_snv = 0;
    if (live) {
      site = pu_active(e0 + (a.events_in ? a.events_in[off] : 0), d0, a.prm.frac);
      n_snv = (uint32_t)((L.a >= kPuMinSupport) + (L.c >= kPuMinSupport) + (L.g >= kPuMinSupport) + (L.t >= kPuMinSupport));
      a.depth[off] = L.depth, a.events[off] = L.events;
      if (want_gl) a.gl[3 * off] = L.g0, a.gl[3 * off + 1] = L.g1, a.gl[3 * off + 2] = L.g2;
      a.cnt[off] = L.a, a.cnt[a.w.len + off] = L.c, a.cnt[2 * a.w.len + off] = L.g, a.cnt[3 * a.w.len + off] = L.t;
      a.site[off] = site ? 1 : 0;
    }
    uint32_t total_sites, total_snvs;
    (void)block_scan_excl<kPuWaves>(site ? 1u : 0u, total_sites, wave_sums);
    (void)block_scan_excl<kPuWaves>(n_snv, total_snvs, wave_sums);
    if (tid == 0) a.tile_sites[t] = total_sites, a.tile_snvs[t] = total_snvs;
  }
}

// The tiles' counts become their first slots; *n_sites and *n_snvs are the totals.
__global__ __launch_bounds__(kPuBlock) void pu_slots_kernel(uint32_t* __restrict__ tile_sites, uint32_t* __restrict__ tile_snvs,
                                                            int64_t n_tiles, int64_t max_sites, int64_t max_snvs,
                                                            int64_t* __restrict__ n_sites, int64_t* __restrict__ n_snvs,
                                                            int32_t* __restrict__ status) {
  __shared__ uint32_t wave_sums[kPuWaves];
  uint32_t carry_s = 0, carry_v = 0;
  for (int64_t t0 = 0; t0 < n_tiles; t0 += kPuBlock) {
    const int64_t t = t0 + (int64_t)threadIdx.x;
    const uint32_t vs = t < n_tiles ? tile_sites[t] : 0, vv = t < n_tiles ? tile_snvs[t] : 0;
    uint32_t ts, tv;
    const uint32_t xs = block_scan_excl<kPuWaves>(vs, ts, wave_sums), xv = block_scan_excl<kPuWaves>(vv, tv, wave_sums);
    if (t < n_tiles) tile_sites[t] = carry_s + xs, tile_snvs[t] = carry_v + xv;
    carry_s += ts, carry_v += tv;
  }
  if (threadIdx.x == 0) {
    *n_sites = (int64_t)carry_s, *n_snvs = (int64_t)carry_v;
    if ((int64_t)carry_s > max_sites) atomicOr(status, kPuStatusSites);
    if ((int64_t)carry_v > max_snvs) atomicOr(status, kPuStatusSnvs);
  }
}

__global__ __launch_bounds__(kPuBlock) void pu_emit_kernel(const int32_t* __restrict__ cnt, const uint8_t* __restrict__ site,
                                                           int64_t len, int64_t n_tiles, const uint32_t* __restrict__ slot_sites,
                                                           const uint32_t* __restrict__ slot_snvs, int32_t* __restrict__ sites,
                                                           int64_t max_sites, fcspu_snv* __restrict__ snvs, int64_t max_snvs,
                                                           const int32_t* __restrict__ status) {
  __shared__ uint32_t wave_sums[kPuWaves];
  if (*status & kPuStatusOrder) return;
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t off = t * kPuTile + (int64_t)threadIdx.x;
    const bool live = off < len;
    const bool is_site = live && site[off] != 0;
    int n[4];
    uint32_t mine = 0;
    for (int x = 0; x < 4; ++x) {
      n[x] = live ? cnt[(int64_t)x * len + off] : 0;
      mine += n[x] >= kPuMinSupport;
    }
    uint32_t total;
    const int64_t at_site = (int64_t)slot_sites[t] + block_scan_excl<kPuWaves>(is_site ? 1u : 0u, total, wave_sums);
    int64_t at = (int64_t)slot_snvs[t] + block_scan_excl<kPuWaves>(mine, total, wave_sums);
    if (is_site && at_site < max_sites) sites[at_site] = (int32_t)off;
    for (int x = 0; x < 4; ++x) {
      if (n[x] < kPuMinSupport) continue;
      if (at < max_snvs) {
        fcspu_snv v;
        v.offset = (int32_t)off, v.alt = (uint8_t)("ACGT"[x]), v.reserved[0] = v.reserved[1] = v.reserved[2] = 0, v.count = n[x];
        snvs[at] = v;
      }
      ++at;
    }
  }
}

int pu_grid(int64_t items) { return (int)std::clamp<int64_t>(items, 1, kPuMaxBlocks); }

int64_t pu_rtiles(int64_t n) { return (n + kPuBlock - 1) / kPuBlock; }
int64_t pu_tiles(int64_t len) { return (len + kPuTile - 1) / kPuTile; }

// The workspace: per batch end, max_end and key per record and the record
// tiles' two maxima; per locus the four counts and the site mark; per tile the
// two counts (adjacent: one memset).
struct PuWorkspace {
  size_t end[FCSPU_BATCHES_MAX], max_end[FCSPU_BATCHES_MAX], key[FCSPU_BATCHES_MAX], tile_end[FCSPU_BATCHES_MAX],
      tile_key[FCSPU_BATCHES_MAX];
  size_t cnt, site, tile_counts, bytes;
};

PuWorkspace pu_workspace(const int64_t* n, int32_t n_batches, int64_t len) {
  PuWorkspace ws{};
  Arena A;
  for (int k = 0; k < n_batches; ++k) {
    ws.end[k] = A.add(8 * (size_t)n[k]), ws.max_end[k] = A.add(8 * (size_t)n[k]), ws.key[k] = A.add(8 * (size_t)n[k]);
    ws.tile_end[k] = A.add(8 * (size_t)pu_rtiles(n[k])), ws.tile_key[k] = A.add(8 * (size_t)pu_rtiles(n[k]));
  }
  ws.cnt = A.add(16 * (size_t)len), ws.site = A.add((size_t)len), ws.tile_counts = A.add(8 * (size_t)pu_tiles(len));
  ws.bytes = std::max<size_t>(A.total, 256);
  return ws;
}

int launch_pile(const fcspu_batch* b, int32_t n_batches, const fcspu_params& prm, const fcspu_window& w, const uint8_t* ref,
                const double* table, const int32_t* events_in, const fcspu_out& out, char* wsp, int32_t* status,
                unsigned long long* bad, hipStream_t s) {
  if (w.len <= 0) {
    FCS_HIP_CHECK(hipMemsetAsync(out.n_sites, 0, sizeof(int64_t), s));
    FCS_HIP_CHECK(hipMemsetAsync(out.n_snvs, 0, sizeof(int64_t), s));
    return FCS_OK;
  }
  int64_t n[FCSPU_BATCHES_MAX] = {0, 0};
  for (int k = 0; k < n_batches; ++k) n[k] = b[k].n;
  const PuWorkspace ws = pu_workspace(n, n_batches, w.len);
  const int64_t tiles = pu_tiles(w.len);
  PuPileArgs a{};
  for (int k = 0; k < n_batches; ++k) {
    int64_t* end = reinterpret_cast<int64_t*>(wsp + ws.end[k]);
    int64_t* max_end = reinterpret_cast<int64_t*>(wsp + ws.max_end[k]);
    int64_t* key = reinterpret_cast<int64_t*>(wsp + ws.key[k]);
    int64_t* tile_end = reinterpret_cast<int64_t*>(wsp + ws.tile_end[k]);
    int64_t* tile_key = reinterpret_cast<int64_t*>(wsp + ws.tile_key[k]);
    (k ? a.b1 : a.b0) = b[k];
    (k ? a.r1 : a.r0) = PuRecs{end, max_end, key};
    if (n[k] <= 0) continue;
    const int64_t rtiles = pu_rtiles(n[k]);
    hipLaunchKernelGGL(pu_span_kernel, dim3(pu_grid(rtiles)), dim3(kPuBlock), 0, s, b[k], w, rtiles, end, key, tile_end, tile_key,
                       status);
    FCS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pu_offsets_kernel, dim3(1), dim3(kPuBlock), 0, s, tile_end, tile_key, rtiles);
    FCS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pu_scan_kernel, dim3(pu_grid(rtiles)), dim3(kPuBlock), 0, s, end, key, n[k], rtiles, tile_end, tile_key,
                       max_end, status);
    FCS_HIP_CHECK(hipGetLastError());
  }
  a.n_batches = n_batches, a.prm = prm, a.w = w, a.ref = ref, a.table = table, a.events_in = events_in;
  a.depth = out.depth, a.events = out.events, a.gl = out.gl;
  a.cnt = reinterpret_cast<int32_t*>(wsp + ws.cnt), a.site = reinterpret_cast<uint8_t*>(wsp + ws.site);
  a.tile_sites = reinterpret_cast<uint32_t*>(wsp + ws.tile_counts), a.tile_snvs = a.tile_sites + tiles;
  a.n_tiles = tiles, a.status = status, a.bad = bad;
  FCS_HIP_CHECK(hipMemsetAsync(a.tile_sites, 0, 8 * (size_t)tiles, s));  // an order error leaves both totals 0
  hipLaunchKernelGGL(pu_pile_kernel, dim3(pu_grid(tiles)), dim3(kPuBlock), 0, s, a);
  FCS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(pu_slots_kernel, dim3(1), dim3(kPuBlock), 0, s, a.tile_sites, a.tile_snvs, tiles, out.max_sites, out.max_snvs,
                     out.n_sites, out.n_snvs, status);
  FCS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(pu_emit_kernel, dim3(pu_grid(tiles)), dim3(kPuBlock), 0, s, a.cnt, a.site, w.len, tiles, a.tile_sites,
                     a.tile_snvs, out.sites, out.max_sites, out.snvs, out.max_snvs, status);
  FCS_HIP_CHECK(hipGetLastError());
  return FCS_OK;
}

int check_window(const fcspu_window* w, const char* who) {
  if (!w) return fail_invalid(who, "null window");
  if (w->ref_id < 0) return fail_invalid(who, "window ref_id " + std::to_string(w->ref_id));
  if (w->len < 0 || w->len > FCSPU_WINDOW_MAX)
    return fail_invalid(who, "a window of " + std::to_string(w->len) + " loci (at most " + std::to_string(FCSPU_WINDOW_MAX) + ")");
  if (w->start < 0 || w->contig_len < 0 || w->start > w->contig_len - w->len)
    return fail_invalid(who, "the window " + std::to_string(w->start) + " + " + std::to_string(w->len) +
                                 " lies outside its contig of " + std::to_string(w->contig_len) + " bases");
  return FCS_OK;
}

// What both entry points check of their scalar arguments.
int check_scalars(const fcspu_batch* b, int32_t n_batches, const fcspu_params* prm, const fcspu_window* w, const fcspu_out* out,
                  const char* who) {
  if (n_batches < 1 || n_batches > FCSPU_BATCHES_MAX)
    return fail_invalid(who, std::to_string(n_batches) + " batches (1 .. " + std::to_string(FCSPU_BATCHES_MAX) + ")");
  if (!b) return fail_invalid(who, "null batch");
  int rc;
  for (int k = 0; k < n_batches; ++k)
    if ((rc = check_batch_scalars(b + k, true, who))) return rc;
  if (!prm) return fail_invalid(who, "null parameters");
  if (!(prm->frac >= 0.0)) return fail_invalid(who, "frac " + std::to_string(prm->frac));
  if ((rc = check_window(w, who))) return rc;
  if (!out) return fail_invalid(who, "null outputs");
  if (out->max_sites < 0 || out->max_snvs < 0)
    return fail_invalid(who, "max_sites " + std::to_string(out->max_sites) + ", max_snvs " + std::to_string(out->max_snvs));
  if (!out->n_sites || !out->n_snvs) return fail_invalid(who, "null counts");
  if (w->len > 0 && (!out->depth || !out->events || (prm->want_gl && !out->gl) || (out->max_sites > 0 && !out->sites) ||
                     (out->max_snvs > 0 && !out->snvs)))
    return fail_invalid(who, "null depth, events, gl, sites or snvs");
  return FCS_OK;
}

}  // namespace

}  // namespace fcs

using namespace fcs;

extern "C" {

int64_t fcspu_workspace_bytes(const int64_t* n_records, int32_t n_batches, int64_t len) {
  const char* who = "fcspu_workspace_bytes";
  if (!n_records || n_batches < 1 || n_batches > FCSPU_BATCHES_MAX || len < 0 || len > FCSPU_WINDOW_MAX)
    return fail_invalid(who, std::to_string(n_batches) + " batches and a window of " + std::to_string(len) + " loci");
  for (int k = 0; k < n_batches; ++k)
    if (n_records[k] < 0) return fail_invalid(who, std::to_string(n_records[k]) + " records");
  return (int64_t)pu_workspace(n_records, n_batches, len).bytes;
}

int fcspu_pile_dev(int32_t device, const fcspu_batch* batches, int32_t n_batches, const fcspu_params* params,
                   const fcspu_window* window, const uint8_t* dev_ref, const double* dev_table, const int32_t* dev_events_in,
                   const fcspu_out* out, void* dev_workspace, int64_t workspace_bytes, int32_t* dev_status, void* stream) {
  const char* who = "fcspu_pile_dev";
  int rc;
  if ((rc = check_scalars(batches, n_batches, params, window, out, who))) return rc;
  const bool work = window->len > 0;
  if (!dev_status || (work && (!dev_ref || !dev_table || !dev_workspace)))
    return fail_invalid(who, "null reference, table, workspace or status");
  int64_t n[FCSPU_BATCHES_MAX] = {0, 0};
  for (int k = 0; k < n_batches; ++k) n[k] = batches[k].n;
  const int64_t need = (int64_t)pu_workspace(n, n_batches, window->len).bytes;
  if (work && workspace_bytes < need)
    return fail_invalid(who, "the workspace holds " + std::to_string(workspace_bytes) + " bytes, the call needs " + std::to_string(need));
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  return launch_pile(batches, n_batches, *params, *window, dev_ref, dev_table, dev_events_in, *out, static_cast<char*>(dev_workspace),
                     dev_status, nullptr, static_cast<hipStream_t>(stream));
}

int fcspu_pile(int32_t device, const fcspu_batch* batches, int32_t n_batches, const fcspu_params* prm, const fcspu_window* w,
               const uint8_t* ref, const double* table, const int32_t* events_in, const fcspu_out* out) {
  const char* who = "fcspu_pile";
  int rc;
  if ((rc = check_scalars(batches, n_batches, prm, w, out, who))) return rc;
  if (!table || (w->len > 0 && !ref)) return fail_invalid(who, "null reference or table");
  for (int k = 0; k < n_batches; ++k)
    if ((rc = check_batch_offsets(batches + k, who))) return rc;
  // what the rules refuse, before any device work
  for (int k = 0; k < n_batches; ++k) {
    const fcspu_batch& b = batches[k];
    const std::string of = n_batches > 1 ? " of batch " + std::to_string(k) : "";
    int64_t last = -1, last_pos = 0;
    for (int64_t r = 0; r < b.n; ++r) {
      if (b.ref_id[r] != w->ref_id) continue;
      if (last >= 0 && b.pos[r] < last_pos)
        return fail_invalid(who, "record " + std::to_string(r) + of + " at position " + std::to_string(b.pos[r]) + " follows record " +
                                     std::to_string(last) + " at " + std::to_string(last_pos) + ": positions decrease");
      last = r, last_pos = b.pos[r];
      int64_t covered, ref_len;
      bool beyond;
      cigar_span(b.cigar + b.cigar_off[r], b.cigar_off[r + 1] - b.cigar_off[r], b.pos[r], w->contig_len, covered, ref_len, beyond);
      if (covered != b.base_off[r + 1] - b.base_off[r])
        return fail_invalid(who, "the CIGAR of record " + std::to_string(r) + of + " does not cover its bases");
      if (beyond) return fail_invalid(who, "record " + std::to_string(r) + of + " has an aligned base beyond its contig");
    }
  }
  if (w->len == 0) {
    *out->n_sites = 0, *out->n_snvs = 0;
    return FCS_OK;
  }
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  const size_t len = (size_t)w->len;
  const int64_t cap_sites = std::min<int64_t>(out->max_sites, w->len), cap_snvs = std::min<int64_t>(out->max_snvs, 4 * w->len);
  Arena A;
  BatchLayout l[FCSPU_BATCHES_MAX]{};
  int64_t n[FCSPU_BATCHES_MAX] = {0, 0};
  for (int k = 0; k < n_batches; ++k) {
    n[k] = batches[k].n;
    if (n[k] > 0) l[k] = layout_batch(batches[k], true, A);
  }
  const size_t oseq = A.add(len), otab = A.add(8 * (size_t)kPuTableWords), oev = A.add(events_in ? 4 * len : 0);
  const size_t in_bytes = A.total;
  const size_t oout = A.add(32);  // n_sites, n_snvs, status, the first refused record
  const size_t host_bytes = A.total;
  const size_t odepth = A.add(4 * len), oevents = A.add(4 * len), ogl = A.add(prm->want_gl ? 24 * len : 0);
  const size_t osites = A.add(4 * (size_t)cap_sites), osnvs = A.add(sizeof(fcspu_snv) * (size_t)cap_snvs);
  const size_t ows = A.add(pu_workspace(n, n_batches, w->len).bytes);
  CallSession S;
  if ((rc = call_session_acquire(device, host_bytes, A.total, S))) return rc;
  CallLease lease{S};
  fcspu_batch d[FCSPU_BATCHES_MAX]{};
  for (int k = 0; k < n_batches; ++k) d[k] = n[k] > 0 ? stage_batch(batches[k], l[k], S.host, S.dev) : batches[k];
  std::memcpy(S.host + oseq, ref, len);
  std::memcpy(S.host + otab, table, 8 * (size_t)kPuTableWords);
  if (events_in) std::memcpy(S.host + oev, events_in, 4 * len);
  fcspu_out o = *out;
  o.depth = reinterpret_cast<int32_t*>(S.dev + odepth), o.events = reinterpret_cast<int32_t*>(S.dev + oevents);
  o.gl = prm->want_gl ? reinterpret_cast<double*>(S.dev + ogl) : nullptr;
  o.sites = reinterpret_cast<int32_t*>(S.dev + osites), o.max_sites = cap_sites;
  o.snvs = reinterpret_cast<fcspu_snv*>(S.dev + osnvs), o.max_snvs = cap_snvs;
  o.n_sites = reinterpret_cast<int64_t*>(S.dev + oout), o.n_snvs = o.n_sites + 1;
  int32_t* status = reinterpret_cast<int32_t*>(S.dev + oout + 16);
  unsigned long long* bad = reinterpret_cast<unsigned long long*>(S.dev + oout + 24);
  FCS_HIP_CHECK(hipMemcpyAsync(S.dev, S.host, in_bytes, hipMemcpyHostToDevice, S.s));
  FCS_HIP_CHECK(hipMemsetAsync(S.dev + oout, 0, 24, S.s));
  FCS_HIP_CHECK(hipMemsetAsync(bad, 0xff, 8, S.s));
  if ((rc = launch_pile(d, n_batches, *prm, *w, reinterpret_cast<const uint8_t*>(S.dev + oseq),
                        reinterpret_cast<const double*>(S.dev + otab), events_in ? reinterpret_cast<const int32_t*>(S.dev + oev) : nullptr,
                        o, S.dev + ows, status, bad, S.s)))
    return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S.host + oout, S.dev + oout, 32, hipMemcpyDeviceToHost, S.s));
  FCS_HIP_CHECK(hipStreamSynchronize(S.s));
  int64_t found[2];
  int32_t st;
  unsigned long long first_bad;
  std::memcpy(found, S.host + oout, sizeof found);
  std::memcpy(&st, S.host + oout + 16, sizeof st);
  std::memcpy(&first_bad, S.host + oout + 24, sizeof first_bad);
  if (st & FCSPU_STATUS_LETTER)
    return fail_invalid(who, "record " + std::to_string(first_bad & ((1ull << 40) - 1)) + " of batch " + std::to_string(first_bad >> 40) +
                                 " has a counted read letter other than A C G T N");
  if ((st & (FCSPU_STATUS_SITES | FCSPU_STATUS_SNVS)) || found[0] > out->max_sites || found[1] > out->max_snvs)
    return fail_invalid(who, "the window has " + std::to_string(found[0]) + " sites and " + std::to_string(found[1]) +
                                 " SNVs, max_sites is " + std::to_string(out->max_sites) + " and max_snvs " + std::to_string(out->max_snvs));
  if (st) return fail(FCS_ERR_DEVICE, "[E::fcspu_pile] the device clamped a checked field (status " + std::to_string(st) + ")");
  FCS_HIP_CHECK(hipMemcpyAsync(out->depth, o.depth, 4 * len, hipMemcpyDeviceToHost, S.s));
  FCS_HIP_CHECK(hipMemcpyAsync(out->events, o.events, 4 * len, hipMemcpyDeviceToHost, S.s));
  if (prm->want_gl) FCS_HIP_CHECK(hipMemcpyAsync(out->gl, o.gl, 24 * len, hipMemcpyDeviceToHost, S.s));
  if (found[0] > 0) FCS_HIP_CHECK(hipMemcpyAsync(out->sites, o.sites, 4 * (size_t)found[0], hipMemcpyDeviceToHost, S.s));
  if (found[1] > 0) FCS_HIP_CHECK(hipMemcpyAsync(out->snvs, o.snvs, sizeof(fcspu_snv) * (size_t)found[1], hipMemcpyDeviceToHost, S.s));
  FCS_HIP_CHECK(hipStreamSynchronize(S.s));
  *out->n_sites = found[0], *out->n_snvs = found[1];
  return FCS_OK;
}

}  // extern "C"
