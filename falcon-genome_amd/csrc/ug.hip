// Pileup SNP genotyping on the device (include/fcsug.h; DESIGN §2 [EXT], §4.12).
// The per-base rules are csrc/ug_pile.h (one text for these kernels and
// tools/micro/ug_test.cpp).  All work of a call is queued on one stream,
// without a host round trip.  A tile is FCSUG_TILE loci of the window; all of a
// tile's sums live in LDS and no base costs a global atomic.
//
// ug_span_kernel: a lane per record: the clamped fields, the record filter, one
// CIGAR pass for the covered bases, the reference end and "an aligned base
// beyond the contig"; end[r] (or "adds nothing") and the position key of the
// records of the window's contig, and the maxima of both per 256 records.
// ug_span_kernel is built for 8 waves per SIMD.
//
// ug_offsets_kernel, ug_scan_kernel: the running maximum of the ends and of
// the positions over the records, in tiles of 256: the tiles' maxima scanned
// by one block, then every tile from its offset.  A position below the running
// maximum before it sets the order bit.
// ug_offsets_kernel is built for 8 waves per SIMD.
// ug_scan_kernel is built for 8 waves per SIMD.
//
// ug_count_kernel, ug_tile_kernel: a block takes tiles in a block stride.  Its
// records are [lo, hi): lo the first whose running-maximum end lies beyond the
// tile's start, hi the first whose position reaches the tile's end, by two
// binary searches.  A wave takes one record at a time in passes of 64 read
// bases, a lane per base: the base's locus, letter and effective quality, then
// LDS atomics into the tile's cells.  The count kernel only marks the loci
// where a non-reference letter was counted and stores the tile's number of
// sites; the tile kernel keeps n, qsum, the three table sums per letter, mq2
// and n_del (one walk, 140 bytes per locus), then a lane per locus applies the
// site predicate, chooses the alt, sums gl and writes the site at the tile's
// slot plus its rank among the tile's sites.
// ug_count_kernel is built for 7 waves per SIMD.
// ug_tile_kernel is built for 4 waves per SIMD.
//
// ug_slots_kernel: the exclusive scan of the tiles' site counts by one block,
// the total and the "more sites than max_sites" bit.
// ug_slots_kernel is built for 8 waves per SIMD.
//
// Every loop is bounded by n, a record's clamped CIGAR word count or base
// count, len, or the tile count; no kernel uses scratch.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "fcship_internal.h"
#include "fcsug.h"
#include "rec_batch.h"
#include "ug_pile.h"

namespace fcs {

namespace {

constexpr int kUgBlock = 256;
constexpr int kUgWaves = kUgBlock / 64;
constexpr int kUgTile = FCSUG_TILE;
constexpr int kUgMaxBlocks = 2048;
constexpr int64_t kUgNone = INT64_MIN;  // end[r] of a record that adds nothing; the key of a record of another contig

static_assert(kUgTile == kUgBlock, "a lane per locus of a tile");
static_assert((kUgTile & (kUgTile - 1)) == 0 && kUgTile >= 256, "fcsug.h: a power of two of at least 256");
static_assert(FCSUG_TABLE_ROWS == kUgTableRows, "fcsug.h and ug_pile.h");
static_assert(FCSUG_STATUS_FIELD == kUgStatusField && FCSUG_STATUS_REF == kUgStatusRef &&
                  FCSUG_STATUS_ORDER == kUgStatusOrder && FCSUG_STATUS_SITES == kUgStatusSites, "fcsug.h and ug_pile.h");
static_assert(sizeof(fcsug_site) == 80 && sizeof(fcsug_window) == 32, "device layouts");

__device__ __forceinline__ int64_t ug_max64(int64_t a, int64_t b) { return a > b ? a : b; }

// The inclusive running maximum of one value per lane of the block, and the block's maximum.
__device__ __forceinline__ int64_t block_max_incl(int64_t v, int64_t& total, int64_t* wave_max) {
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  int64_t inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t up = __shfl_up(inc, d);
    if (lane >= d) inc = ug_max64(inc, up);
  }
  if (lane == 63) wave_max[wave] = inc;
  __syncthreads();
  total = kUgNone;
  for (int k = 0; k < kUgWaves; ++k) {
    const int64_t s = wave_max[k];
    if (k < wave) inc = ug_max64(inc, s);
    total = ug_max64(total, s);
  }
  __syncthreads();  // wave_max may be written again
  return inc;
}

__global__ __launch_bounds__(kUgBlock) void ug_span_kernel(fcsug_batch b, fcsug_window w, int64_t n_rtiles,
                                                           int64_t* __restrict__ end, int64_t* __restrict__ key,
                                                           int64_t* __restrict__ tile_end, int64_t* __restrict__ tile_key,
                                                           int32_t* __restrict__ status) {
  __shared__ int64_t wave_max[kUgWaves];
  for (int64_t t = blockIdx.x; t < n_rtiles; t += gridDim.x) {
    const int64_t r = t * kUgBlock + (int64_t)threadIdx.x;
    int64_t e = kUgNone, kp = kUgNone;
    if (r < b.n && b.ref_id[r] == w.ref_id) {
      const int64_t pos = b.pos[r];
      kp = pos;
      int64_t c0, c1, q0, q1;
      bool bad = !rec_fields(b, r, c0, c1, q0, q1);
      bool counted = false, beyond = false;
      int64_t ref_len = 0;
      if (!bad && ug_counted(b.flag[r], b.ref_id[r], c1 - c0, b.mapq[r])) {
        int64_t covered;
        cigar_span(b.cigar + c0, c1 - c0, pos, w.contig_len, covered, ref_len, beyond);
        bad = covered != q1 - q0;
        counted = !bad;
      }
      if (bad) atomicOr(status, kUgStatusField);
      if (counted) {
        e = pos + ref_len;
        if (beyond) atomicOr(status, kUgStatusRef);
      }
    }
    if (r < b.n) end[r] = e, key[r] = kp;
    int64_t te, tk;
    (void)block_max_incl(e, te, wave_max);
    (void)block_max_incl(kp, tk, wave_max);
    if (threadIdx.x == 0) tile_end[t] = te, tile_key[t] = tk;
  }
}

// tile_end and tile_key become the maxima of all earlier tiles.
__global__ __launch_bounds__(kUgBlock) void ug_offsets_kernel(int64_t* __restrict__ tile_end, int64_t* __restrict__ tile_key,
                                                              int64_t n_rtiles) {
  __shared__ int64_t wave_max[kUgWaves];
  __shared__ int64_t last_e[kUgWaves], last_k[kUgWaves];
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  int64_t carry_e = kUgNone, carry_k = kUgNone;
  for (int64_t t0 = 0; t0 < n_rtiles; t0 += kUgBlock) {
    const int64_t t = t0 + (int64_t)threadIdx.x;
    const int64_t ve = t < n_rtiles ? tile_end[t] : kUgNone, vk = t < n_rtiles ? tile_key[t] : kUgNone;
    int64_t te, tk;
    const int64_t ie = block_max_incl(ve, te, wave_max), ik = block_max_incl(vk, tk, wave_max);
    // exclusive: the inclusive maximum of the lane before
    const int64_t pe = __shfl_up(ie, 1), pk = __shfl_up(ik, 1);
    if (lane == 63) last_e[wave] = ie, last_k[wave] = ik;
    __syncthreads();
    const int64_t xe = lane ? pe : wave ? last_e[wave - 1] : kUgNone, xk = lane ? pk : wave ? last_k[wave - 1] : kUgNone;
    if (t < n_rtiles) tile_end[t] = ug_max64(carry_e, xe), tile_key[t] = ug_max64(carry_k, xk);
    carry_e = ug_max64(carry_e, te), carry_k = ug_max64(carry_k, tk);
    __syncthreads();  // last_e and last_k may be written again
  }
}

// max_end[r]: the running maximum of end[0 .. r].  key[r] becomes the running
// maximum of the keys [0 .. r]; a key below the maximum before it is out of order.
__global__ __launch_bounds__(kUgBlock) void ug_scan_kernel(const int64_t* __restrict__ end, int64_t* __restrict__ key, int64_t n,
                                                           int64_t n_rtiles, const int64_t* __restrict__ tile_end,
                                                           const int64_t* __restrict__ tile_key, int64_t* __restrict__ max_end,
                                                           int32_t* __restrict__ status) {
  __shared__ int64_t wave_max[kUgWaves];
  __shared__ int64_t last_k[kUgWaves];
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  for (int64_t t = blockIdx.x; t < n_rtiles; t += gridDim.x) {
    const int64_t r = t * kUgBlock + (int64_t)threadIdx.x;
    const int64_t e = r < n ? end[r] : kUgNone, kp = r < n ? key[r] : kUgNone;
    int64_t unused;
    const int64_t ie = block_max_incl(e, unused, wave_max), ik = block_max_incl(kp, unused, wave_max);
    const int64_t pk = __shfl_up(ik, 1);
    if (lane == 63) last_k[wave] = ik;
    __syncthreads();
    const int64_t before = ug_max64(tile_key[t], lane ? pk : wave ? last_k[wave - 1] : kUgNone);
    if (r < n) {
      max_end[r] = ug_max64(tile_end[t], ie);
      key[r] = ug_max64(tile_key[t], ik);
      if (kp != kUgNone && kp < before) atomicOr(status, kUgStatusOrder);
    }
    __syncthreads();  // last_k may be written again
  }
}

// The first r in [0, n) with v[r] > x (strict) or v[r] >= x, v non-decreasing; n without one.
__device__ __forceinline__ int64_t ug_first(const int64_t* __restrict__ v, int64_t n, int64_t x, bool strict) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    const int64_t m = v[mid];
    if (strict ? m > x : m >= x) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// The records of the tile [s, e) of the contig, a wave per record and a lane
// per base: base(cell, letter, qe, mapq) for every counted base, del(cell) for
// every deleted locus of a record whose min(MAPQ, 93) reaches min_baseq.
template <class Base, class Del>
__device__ __forceinline__ void ug_walk(const fcsug_batch& b, int32_t min_baseq, const int64_t* __restrict__ end,
                                        const int64_t* __restrict__ max_end, const int64_t* __restrict__ key, int64_t s,
                                        int64_t e, Base&& base, Del&& del) {
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  const int64_t lo = ug_first(max_end, b.n, s, true), hi = ug_first(key, b.n, e, false);
  for (int64_t r = lo + wave; r < hi; r += kUgWaves) {  // r is the wave's
    const int64_t ev = end[r];
    if (ev == kUgNone || ev <= s) continue;
    const int64_t pos = b.pos[r];
    if (pos >= e) continue;
    int64_t c0, c1, q0, q1;
    (void)rec_fields(b, r, c0, c1, q0, q1);
    const uint32_t* cigar = b.cigar + c0;
    const int64_t n_ops = c1 - c0, L = q1 - q0;
    const int mapq = b.mapq[r];
    const bool absent = b.qual_absent[r] != 0;
    const uint8_t* bases = b.bases + q0;
    const uint8_t* qual = b.qual + q0;
    for (int64_t i0 = 0; i0 < L; i0 += 64) {
      const int64_t i = i0 + lane;
      int64_t p;
      if (i < L && cigar_site(cigar, n_ops, pos, i, p) && p >= s && p < e) {
        const int x = ug_code(bases[i]);
        const int qe = ug_qe(absent ? 0 : (int)qual[i], mapq);
        if (x < 4 && qe >= min_baseq) base((int)(p - s), x, qe, mapq);
      }
    }
    if (ug_qe(kUgMaxQ, mapq) < min_baseq) continue;
    int64_t p = pos;
    for (int64_t k = 0; k < n_ops; ++k) {
      const uint32_t op = cigar[k] & 15u;
      const int64_t len = (int64_t)(cigar[k] >> 4);
      if (op == 2u) {
        const int64_t d0 = clamp64(p, s, e), d1 = clamp64(p + len, d0, e);
        for (int64_t j = d0 + lane; j < d1; j += 64) del((int)(j - s));
      }
      if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) p += len;
    }
  }
}

__global__ __launch_bounds__(kUgBlock) void ug_count_kernel(fcsug_batch b, fcsug_params prm, fcsug_window w,
                                                            const uint8_t* __restrict__ ref, const int64_t* __restrict__ end,
                                                            const int64_t* __restrict__ max_end,
                                                            const int64_t* __restrict__ key, int64_t n_tiles,
                                                            uint32_t* __restrict__ counts, const int32_t* __restrict__ status) {
  __shared__ uint32_t marks[kUgTile / 32];
  __shared__ uint8_t rcode[kUgTile];
  __shared__ uint32_t wave_sums[kUgWaves];
  const int tid = (int)threadIdx.x;
  const bool order = (*status & kUgStatusOrder) != 0;
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t s = w.start + t * kUgTile, e = s + kUgTile < w.start + w.len ? s + kUgTile : w.start + w.len;
    if (tid < kUgTile / 32) marks[tid] = 0;
    rcode[tid] = s + tid < e ? (uint8_t)ug_code(ref[t * kUgTile + tid]) : 4;
    __syncthreads();
    if (!order)
      ug_walk(b, prm.min_baseq, end, max_end, key, s, e,
              [&](int cell, int x, int, int) {
                const int rc = rcode[cell];
                if (rc < 4 && x != rc) atomicOr(&marks[cell >> 5], 1u << (cell & 31));
              },
              [](int) {});
    __syncthreads();
    uint32_t total;
    (void)block_scan_excl<kUgWaves>(tid < kUgTile / 32 ? (uint32_t)__popc(marks[tid]) : 0u, total, wave_sums);
    if (tid == 0) counts[t] = total;
  }
}

// counts become the tiles' first slots; *n_sites is the total.
__global__ __launch_bounds__(kUgBlock) void ug_slots_kernel(uint32_t* __restrict__ counts, int64_t n_tiles, int64_t max_sites,
                                                            int64_t* __restrict__ n_sites, int32_t* __restrict__ status) {
  __shared__ uint32_t wave_sums[kUgWaves];
  uint32_t carry = 0;
  for (int64_t t0 = 0; t0 < n_tiles; t0 += kUgBlock) {
    const int64_t t = t0 + (int64_t)threadIdx.x;
    const uint32_t v = t < n_tiles ? counts[t] : 0;
    uint32_t total;
    const uint32_t ex = block_scan_excl<kUgWaves>(v, total, wave_sums);
    if (t < n_tiles) counts[t] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    *n_sites = (int64_t)carry;
    if ((int64_t)carry > max_sites) atomicOr(status, kUgStatusSites);
  }
}

__global__ __launch_bounds__(kUgBlock) void ug_tile_kernel(fcsug_batch b, fcsug_params prm, fcsug_window w,
                                                           const uint8_t* __restrict__ ref, const int64_t* __restrict__ table,
                                                           const int64_t* __restrict__ end, const int64_t* __restrict__ max_end,
                                                           const int64_t* __restrict__ key, int64_t n_tiles,
                                                           const uint32_t* __restrict__ slots, fcsug_site* __restrict__ sites,
                                                           int64_t max_sites, const int32_t* __restrict__ status) {
  // 140 bytes per locus: the three table sums and mq2 in 64 bits, n, qsum and n_del in 32
  __shared__ unsigned long long sumA[4][kUgTile], sumB[4][kUgTile], sumC[4][kUgTile], mq2[kUgTile];
  __shared__ uint32_t cnt[4][kUgTile], qsum[4][kUgTile], n_del[kUgTile];
  __shared__ int64_t tab[kUgTableRows * 3];
  __shared__ uint8_t rcode[kUgTile];
  __shared__ uint32_t wave_sums[kUgWaves];
  const int tid = (int)threadIdx.x;
  if (*status & kUgStatusOrder) return;
  for (int k = tid; k < kUgTableRows * 3; k += kUgBlock) tab[k] = table[k];
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t s = w.start + t * kUgTile, e = s + kUgTile < w.start + w.len ? s + kUgTile : w.start + w.len;
    for (int x = 0; x < 4; ++x) sumA[x][tid] = 0, sumB[x][tid] = 0, sumC[x][tid] = 0, cnt[x][tid] = 0, qsum[x][tid] = 0;
    mq2[tid] = 0, n_del[tid] = 0;
    rcode[tid] = s + tid < e ? (uint8_t)ug_code(ref[t * kUgTile + tid]) : 4;
    __syncthreads();
    ug_walk(b, prm.min_baseq, end, max_end, key, s, e,
            [&](int cell, int x, int qe, int mapq) {
              atomicAdd(&cnt[x][cell], 1u);
              atomicAdd(&qsum[x][cell], (uint32_t)qe);
              atomicAdd(&mq2[cell], (unsigned long long)(mapq * mapq));
              atomicAdd(&sumA[x][cell], (unsigned long long)tab[3 * qe]);
              atomicAdd(&sumB[x][cell], (unsigned long long)tab[3 * qe + 1]);
              atomicAdd(&sumC[x][cell], (unsigned long long)tab[3 * qe + 2]);
            },
            [&](int cell) { atomicAdd(&n_del[cell], 1u); });
    __syncthreads();
    const int rc = rcode[tid];
    uint32_t n[4], q[4];
    for (int x = 0; x < 4; ++x) n[x] = cnt[x][tid], q[x] = qsum[x][tid];
    const bool site = ug_is_site(rc, n);
    uint32_t total;
    const int64_t at = (int64_t)slots[t] + block_scan_excl<kUgWaves>(site ? 1u : 0u, total, wave_sums);
    if (site && at < max_sites) {
      int64_t A[4], B[4], C[4];
      for (int x = 0; x < 4; ++x) A[x] = (int64_t)sumA[x][tid], B[x] = (int64_t)sumB[x][tid], C[x] = (int64_t)sumC[x][tid];
      fcsug_site out;
      out.offset = (int32_t)(t * kUgTile + tid);
      out.ref = (uint8_t)rc, out.alt = (uint8_t)ug_alt(rc, q), out.reserved = 0;
      for (int x = 0; x < 4; ++x) out.n[x] = n[x], out.qsum[x] = q[x];
      out.n_del = n_del[tid], out.reserved2 = 0, out.mq2 = mq2[tid];
      ug_gl(rc, out.alt, A, B, C, out.gl);
      sites[at] = out;
    }
    __syncthreads();  // the cells are zeroed again
  }
}

int ug_grid(int64_t items) { return (int)std::clamp<int64_t>(items, 1, kUgMaxBlocks); }

int64_t ug_rtiles(int64_t n) { return (n + kUgBlock - 1) / kUgBlock; }
int64_t ug_tiles(int64_t len) { return (len + kUgTile - 1) / kUgTile; }

// The workspace: end, max_end and key per record, the record tiles' two maxima, a count per tile.
struct UgWorkspace {
  size_t end, max_end, key, tile_end, tile_key, counts, bytes;
};

UgWorkspace ug_workspace(int64_t n, int64_t len) {
  UgWorkspace ws{};
  Arena A;
  ws.end = A.add(8 * (size_t)n), ws.max_end = A.add(8 * (size_t)n), ws.key = A.add(8 * (size_t)n);
  ws.tile_end = A.add(8 * (size_t)ug_rtiles(n)), ws.tile_key = A.add(8 * (size_t)ug_rtiles(n));
  ws.counts = A.add(4 * (size_t)ug_tiles(len));
  ws.bytes = std::max<size_t>(A.total, 256);
  return ws;
}

int launch_sites(const fcsug_batch& b, const fcsug_params& prm, const fcsug_window& w, const uint8_t* ref, const int64_t* table,
                 fcsug_site* sites, int64_t max_sites, int64_t* n_sites, char* wsp, int32_t* status, hipStream_t s) {
  if (b.n <= 0 || w.len <= 0) {
    FCS_HIP_CHECK(hipMemsetAsync(n_sites, 0, sizeof(int64_t), s));
    return FCS_OK;
  }
  const UgWorkspace ws = ug_workspace(b.n, w.len);
  int64_t* end = reinterpret_cast<int64_t*>(wsp + ws.end);
  int64_t* max_end = reinterpret_cast<int64_t*>(wsp + ws.max_end);
  int64_t* key = reinterpret_cast<int64_t*>(wsp + ws.key);
  int64_t* tile_end = reinterpret_cast<int64_t*>(wsp + ws.tile_end);
  int64_t* tile_key = reinterpret_cast<int64_t*>(wsp + ws.tile_key);
  uint32_t* counts = reinterpret_cast<uint32_t*>(wsp + ws.counts);
  const int64_t rtiles = ug_rtiles(b.n), tiles = ug_tiles(w.len);
  hipLaunchKernelGGL(ug_span_kernel, dim3(ug_grid(rtiles)), dim3(kUgBlock), 0, s, b, w, rtiles, end, key, tile_end, tile_key,
                     status);
  FCS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(ug_offsets_kernel, dim3(1), dim3(kUgBlock), 0, s, tile_end, tile_key, rtiles);
  FCS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(ug_scan_kernel, dim3(ug_grid(rtiles)), dim3(kUgBlock), 0, s, end, key, b.n, rtiles, tile_end, tile_key,
                     max_end, status);
  FCS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(ug_count_kernel, dim3(ug_grid(tiles)), dim3(kUgBlock), 0, s, b, prm, w, ref, end, max_end, key, tiles,
                     counts, status);
  FCS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(ug_slots_kernel, dim3(1), dim3(kUgBlock), 0, s, counts, tiles, max_sites, n_sites, status);
  FCS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(ug_tile_kernel, dim3(ug_grid(tiles)), dim3(kUgBlock), 0, s, b, prm, w, ref, table, end, max_end, key, tiles,
                     counts, sites, max_sites, status);
  FCS_HIP_CHECK(hipGetLastError());
  return FCS_OK;
}

int check_window(const fcsug_window* w, const char* who) {
  if (!w) return fail_invalid(who, "null window");
  if (w->ref_id < 0) return fail_invalid(who, "window ref_id " + std::to_string(w->ref_id));
  if (w->len < 0 || w->len > FCSUG_WINDOW_MAX)
    return fail_invalid(who, "a window of " + std::to_string(w->len) + " loci (at most " + std::to_string(FCSUG_WINDOW_MAX) + ")");
  if (w->start < 0 || w->contig_len < 0 || w->start > w->contig_len - w->len)
    return fail_invalid(who, "the window " + std::to_string(w->start) + " + " + std::to_string(w->len) +
                                 " lies outside its contig of " + std::to_string(w->contig_len) + " bases");
  return FCS_OK;
}

}  // namespace

}  // namespace fcs

using namespace fcs;

extern "C" {

int fcsug_table(double pcr_error, int64_t* table) {
  const char* who = "fcsug_table";
  if (!table) return fail_invalid(who, "null table");
  if (!(pcr_error > 0.0 && pcr_error < 1.0)) return fail_invalid(who, "pcr_error " + std::to_string(pcr_error) + " is outside (0, 1)");
  const double eps = pcr_error;
  for (int q = 0; q < FCSUG_TABLE_ROWS; ++q) {
    const double e = std::pow(10.0, -q / 10.0);
    const double same = (1.0 - eps) * (1.0 - e) + eps * e / 3.0;
    const double diff = (1.0 - eps) * e / 3.0 + (eps / 3.0) * (1.0 - e) + 2.0 * (eps / 3.0) * (e / 3.0);
    const double p[3] = {same, 0.5 * same + 0.5 * diff, diff};
    for (int c = 0; c < 3; ++c) table[3 * q + c] = (int64_t)std::llround(std::log10(p[c]) * 4294967296.0);
  }
  return FCS_OK;
}

int64_t fcsug_workspace_bytes(int64_t n_records, int64_t len) {
  if (n_records < 0 || len < 0 || len > FCSUG_WINDOW_MAX)
    return fail_invalid("fcsug_workspace_bytes", std::to_string(n_records) + " records and a window of " + std::to_string(len) + " loci");
  return (int64_t)ug_workspace(n_records, len).bytes;
}

int fcsug_sites_dev(int32_t device, const fcsug_batch* batch, const fcsug_params* params, const fcsug_window* window,
                    const uint8_t* dev_ref, const int64_t* dev_table, fcsug_site* dev_sites, int64_t max_sites,
                    int64_t* dev_n_sites, void* dev_workspace, int64_t workspace_bytes, int32_t* dev_status, void* stream) {
  const char* who = "fcsug_sites_dev";
  int rc;
  if ((rc = check_batch_scalars(batch, true, who))) return rc;
  if (!params) return fail_invalid(who, "null parameters");
  if ((rc = check_window(window, who))) return rc;
  if (max_sites < 0) return fail_invalid(who, "max_sites " + std::to_string(max_sites));
  const bool work = batch->n > 0 && window->len > 0;
  if (!dev_status || !dev_n_sites || (work && (!dev_ref || !dev_table || !dev_workspace || (max_sites > 0 && !dev_sites))))
    return fail_invalid(who, "null reference, table, sites, count, workspace or status");
  const int64_t need = (int64_t)ug_workspace(batch->n, window->len).bytes;
  if (work && workspace_bytes < need)
    return fail_invalid(who, "the workspace holds " + std::to_string(workspace_bytes) + " bytes, the call needs " + std::to_string(need));
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  return launch_sites(*batch, *params, *window, dev_ref, dev_table, dev_sites, max_sites, dev_n_sites,
                      static_cast<char*>(dev_workspace), dev_status, static_cast<hipStream_t>(stream));
}

int fcsug_sites(int32_t device, const fcsug_batch* b, const fcsug_params* prm, const fcsug_window* w, const uint8_t* ref,
                const int64_t* table, fcsug_site* sites, int64_t max_sites, int64_t* n_sites) {
  const char* who = "fcsug_sites";
  int rc;
  if ((rc = check_batch_scalars(b, true, who))) return rc;
  if (!prm) return fail_invalid(who, "null parameters");
  if ((rc = check_window(w, who))) return rc;
  if (max_sites < 0) return fail_invalid(who, "max_sites " + std::to_string(max_sites));
  if (!n_sites || !table || (w->len > 0 && !ref) || (max_sites > 0 && !sites)) return fail_invalid(who, "null reference, table, sites or count");
  if ((rc = check_batch_offsets(b, who))) return rc;
  const int64_t n = b->n;
  // what the rules refuse, before any device work
  int64_t last = -1, last_pos = 0;
  for (int64_t r = 0; r < n; ++r) {
    if (b->ref_id[r] != w->ref_id) continue;
    if (last >= 0 && b->pos[r] < last_pos)
      return fail_invalid(who, "record " + std::to_string(r) + " at position " + std::to_string(b->pos[r]) + " follows record " +
                                   std::to_string(last) + " at " + std::to_string(last_pos) + ": positions decrease");
    last = r, last_pos = b->pos[r];
    const int64_t n_ops = b->cigar_off[r + 1] - b->cigar_off[r], L = b->base_off[r + 1] - b->base_off[r];
    if (!ug_counted(b->flag[r], b->ref_id[r], n_ops, b->mapq[r])) continue;
    int64_t covered, ref_len;
    bool beyond;
    cigar_span(b->cigar + b->cigar_off[r], n_ops, b->pos[r], w->contig_len, covered, ref_len, beyond);
    if (covered != L) return fail_invalid(who, "the CIGAR of record " + std::to_string(r) + " does not cover its bases");
    if (beyond) return fail_invalid(who, "record " + std::to_string(r) + " has an aligned base beyond its contig");
  }
  if (n == 0 || w->len == 0) {
    *n_sites = 0;
    return FCS_OK;
  }
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  const int64_t cap = std::min<int64_t>(max_sites, w->len);
  Arena A;
  const BatchLayout l = layout_batch(*b, true, A);
  const size_t oseq = A.add((size_t)w->len), otab = A.add(8 * 3 * (size_t)FCSUG_TABLE_ROWS);
  const size_t in_bytes = A.total;
  const size_t oout = A.add(16);  // n_sites, status
  const size_t host_bytes = A.total;
  const size_t osites = A.add(sizeof(fcsug_site) * (size_t)cap), ows = A.add(ug_workspace(n, w->len).bytes);
  CallSession S;
  if ((rc = call_session_acquire(device, host_bytes, A.total, S))) return rc;
  CallLease lease{S};
  const fcsug_batch d = stage_batch(*b, l, S.host, S.dev);
  std::memcpy(S.host + oseq, ref, (size_t)w->len);
  std::memcpy(S.host + otab, table, 8 * 3 * (size_t)FCSUG_TABLE_ROWS);
  int64_t* dn = reinterpret_cast<int64_t*>(S.dev + oout);
  int32_t* status = reinterpret_cast<int32_t*>(S.dev + oout + 8);
  fcsug_site* dsites = reinterpret_cast<fcsug_site*>(S.dev + osites);
  FCS_HIP_CHECK(hipMemcpyAsync(S.dev, S.host, in_bytes, hipMemcpyHostToDevice, S.s));
  FCS_HIP_CHECK(hipMemsetAsync(S.dev + oout, 0, 16, S.s));
  if ((rc = launch_sites(d, *prm, *w, reinterpret_cast<const uint8_t*>(S.dev + oseq), reinterpret_cast<const int64_t*>(S.dev + otab), dsites, cap, dn, S.dev + ows,
                         status, S.s)))
    return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S.host + oout, S.dev + oout, 16, hipMemcpyDeviceToHost, S.s));
  FCS_HIP_CHECK(hipStreamSynchronize(S.s));
  int64_t found;
  int32_t st;
  std::memcpy(&found, S.host + oout, sizeof found);
  std::memcpy(&st, S.host + oout + 8, sizeof st);
  if ((st & FCSUG_STATUS_SITES) || found > max_sites)
    return fail_invalid(who, "the window has " + std::to_string(found) + " sites, max_sites is " + std::to_string(max_sites));
  if (st) return fail(FCS_ERR_DEVICE, "[E::fcsug_sites] the device clamped a checked field (status " + std::to_string(st) + ")");
  if (found > 0) {
    FCS_HIP_CHECK(hipMemcpyAsync(sites, dsites, sizeof(fcsug_site) * (size_t)found, hipMemcpyDeviceToHost, S.s));
    FCS_HIP_CHECK(hipStreamSynchronize(S.s));
  }
  *n_sites = found;
  return FCS_OK;
}

}  // extern "C"
