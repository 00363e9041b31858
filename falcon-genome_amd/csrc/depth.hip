// Depth of coverage on the device (include/fcsdp.h; DESIGN §2 [EXT], §4.11).
// The per-base logic is csrc/dp_runs.h (one text for these kernels and
// tools/micro/depth_test.cpp).  All work of a call is queued on one stream,
// without a host round trip.
//
// dp_runs_kernel: a wave takes one record at a time, in passes of 64 read
// bases, a lane per base: one CIGAR pass by the wave finds the span, each lane
// locates its base's reference position and evaluates "counted and inside the
// window"; a ballot and the neighbours' window offsets mark the first and the
// last lane of each maximal run of counted bases at consecutive positions, and
// only those lanes add: +1 at the run's first window offset, -1 one past its
// last, into signed 32-bit cells [len + 1].  With include_deletions lane 0
// adds every D op as a run of its own.
// dp_runs_kernel is built for 8 waves per SIMD.
//
// dp_reduce_kernel, dp_offsets_kernel, dp_scan_kernel: the inclusive scan of
// the cells in place, in tiles of 1024 (256 lanes x 4 cells): the tiles' sums,
// their exclusive scan by one block, then every tile scanned from its offset.
// Sums wrap modulo 2^32, which leaves every depth below 2^31 exact; a negative
// depth sets the overflow bit.
// dp_reduce_kernel is built for 8 waves per SIMD.
// dp_offsets_kernel is built for 8 waves per SIMD.
// dp_scan_kernel is built for 8 waves per SIMD.
//
// dp_stats_kernel: a block takes one piece at a time: the depths and the
// participation bits of its loci, a 501-bin histogram in LDS by LDS atomics,
// total, loci and loci >= 15, and the three granular quantiles by a block scan
// of the bins (two per lane); one 32-byte summary per piece.  Non-empty bins
// are added to the sample histogram, and to the piece's long_hist row when it
// has one, by 64-bit global atomics.
// dp_stats_kernel is built for 8 waves per SIMD.
//
// Every loop is bounded by n, a record's clamped CIGAR word count or base
// count, len, or the piece count; no kernel uses scratch.
#include <algorithm>
#include <cstring>
#include <string>

#include "dp_runs.h"
#include "fcsdp.h"
#include "fcship_internal.h"
#include "rec_batch.h"

namespace fcs {

namespace {

constexpr int kDpBlock = 256;
constexpr int kDpWaves = kDpBlock / 64;
constexpr int kDpMaxBlocks = 4096;
constexpr int kDpTile = 4 * kDpBlock;

static_assert(FCSDP_BINS == kDpBins && FCSDP_PIECE_MAX == kDpPieceMax && FCSDP_ABOVE == kDpAbove, "fcsdp.h and dp_runs.h");
static_assert(FCSDP_STATUS_FIELD == kDpStatusField && FCSDP_STATUS_REF == kDpStatusRef &&
                  FCSDP_STATUS_OVERFLOW == kDpStatusOverflow, "fcsdp.h and dp_runs.h");
static_assert(sizeof(fcsdp_piece) == 16 && sizeof(fcsdp_summary) == 32, "device layouts");

__global__ __launch_bounds__(kDpBlock) void dp_runs_kernel(fcsdp_batch b, fcsdp_params prm, fcsdp_window w,
                                                           int32_t* __restrict__ cells, int32_t* __restrict__ status) {
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  const int64_t stride = (int64_t)gridDim.x * kDpWaves;
  const int64_t w0 = w.start, wlen = w.len, clen = w.contig_len;
  for (int64_t r = (int64_t)blockIdx.x * kDpWaves + wave; r < b.n; r += stride) {  // r is the wave's
    const int32_t c = b.ref_id[r];
    if (c != w.ref_id) continue;
    int64_t c0, c1, q0, q1;
    bool bad = !rec_fields(b, r, c0, c1, q0, q1);
    const uint32_t* cigar = b.cigar + c0;
    const int64_t n_ops = c1 - c0, L = q1 - q0;
    int64_t covered = 0, ref_len = 0;
    if (!bad) {
      if (!dp_counted(b.flag[r], c, n_ops, b.mapq[r], prm.min_mapq, prm.max_mapq)) continue;
      cigar_span(cigar, n_ops, covered, ref_len);
      bad = covered != L;
    }
    if (bad) {  // the record adds nothing
      if (lane == 0) atomicOr(status, kDpStatusField);
      continue;
    }
    const int64_t pos = b.pos[r];
    // wholly before the window, or wholly after it and inside the contig: nothing to add or to report
    if ((pos >= 0 && pos + ref_len <= w0) || (pos >= w0 + wlen && pos + ref_len <= clen)) continue;
    const bool absent = b.qual_absent[r] != 0;
    const uint8_t* qual = b.qual + q0;
    bool beyond = false;
    for (int64_t i0 = 0; i0 < L; i0 += 64) {
      const int64_t i = i0 + lane;
      int32_t off = -1;
      int64_t p;
      if (i < L && cigar_site(cigar, n_ops, pos, i, p)) {
        if (p < 0 || p >= clen) beyond = true;
        else if (dp_base_ok(absent ? 0 : (int)qual[i], prm.min_baseq, prm.max_baseq)) off = dp_in_window(p, w0, wlen, clen);
      }
      const unsigned long long counted = __ballot(off >= 0);
      if (!counted) continue;  // uniform: the ballot is the wave's
      const int32_t prev = __shfl_up(off, 1), next = __shfl_down(off, 1);
      if (dp_run_first(lane, counted, off, prev)) atomicAdd(cells + off, 1);
      if (dp_run_last(lane, counted, off, next)) atomicAdd(cells + off + 1, -1);
    }
    if (__any(beyond) && lane == 0) atomicOr(status, kDpStatusRef);
    if (prm.include_deletions && lane == 0) {
      int64_t p = pos;
      for (int64_t k = 0; k < n_ops; ++k) {
        const uint32_t op = cigar[k] & 15u;
        const int64_t len = (int64_t)(cigar[k] >> 4);
        if (op == 2u) {
          const int64_t lo = clamp64(p, w0 > 0 ? w0 : 0, p + len);
          const int64_t hi = clamp64(p + len, lo, w0 + wlen < clen ? w0 + wlen : clen);
          if (lo < hi) {
            atomicAdd(cells + (lo - w0), 1);
            atomicAdd(cells + (hi - w0), -1);
          }
        }
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) p += len;
      }
    }
  }
}

__global__ __launch_bounds__(kDpBlock) void dp_reduce_kernel(const int32_t* __restrict__ cells, int64_t len,
                                                             int64_t n_tiles, uint32_t* __restrict__ sums) {
  __shared__ uint32_t wave_sums[kDpWaves];
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t base = t * kDpTile + 4 * (int64_t)threadIdx.x;
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k)
      if (base + k < len) v += (uint32_t)cells[base + k];
    uint32_t total;
    (void)block_scan_excl<kDpWaves>(v, total, wave_sums);
    if (threadIdx.x == 0) sums[t] = total;
  }
}

__global__ __launch_bounds__(kDpBlock) void dp_offsets_kernel(uint32_t* __restrict__ sums, int64_t n_tiles) {
  __shared__ uint32_t wave_sums[kDpWaves];
  uint32_t carry = 0;
  for (int64_t t0 = 0; t0 < n_tiles; t0 += kDpBlock) {
    const int64_t t = t0 + threadIdx.x;
    const uint32_t v = t < n_tiles ? sums[t] : 0;
    uint32_t total;
    const uint32_t ex = block_scan_excl<kDpWaves>(v, total, wave_sums);
    if (t < n_tiles) sums[t] = carry + ex;
    carry += total;
  }
}

__global__ __launch_bounds__(kDpBlock) void dp_scan_kernel(int32_t* __restrict__ cells, int64_t len, int64_t n_tiles,
                                                           const uint32_t* __restrict__ offsets,
                                                           int32_t* __restrict__ status) {
  __shared__ uint32_t wave_sums[kDpWaves];
  bool negative = false;
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t base = t * kDpTile + 4 * (int64_t)threadIdx.x;
    uint32_t v[4], s = 0;
    for (int k = 0; k < 4; ++k) {
      v[k] = base + k < len ? (uint32_t)cells[base + k] : 0;
      s += v[k];
    }
    uint32_t total;
    uint32_t run = offsets[t] + block_scan_excl<kDpWaves>(s, total, wave_sums);
    for (int k = 0; k < 4; ++k) {
      run += v[k];
      if (base + k < len) {
        cells[base + k] = (int32_t)run;
        negative |= (int32_t)run < 0;
      }
    }
  }
  if (negative) atomicOr(status, kDpStatusOverflow);
}

__global__ __launch_bounds__(kDpBlock) void dp_stats_kernel(const uint32_t* __restrict__ depth,
                                                            const uint64_t* __restrict__ bitmap, int64_t len,
                                                            const fcsdp_piece* __restrict__ pieces, int64_t n_pieces,
                                                            int32_t n_long, unsigned long long* __restrict__ hist,
                                                            unsigned long long* __restrict__ long_hist,
                                                            fcsdp_summary* __restrict__ summary,
                                                            int32_t* __restrict__ status) {
  __shared__ uint32_t bins[2 * kDpBlock];  // 501 used; two per lane in the scan
  __shared__ uint32_t wave_sums[kDpWaves];
  __shared__ unsigned long long total;
  __shared__ uint32_t above, quant[3];
  const int tid = (int)threadIdx.x;
  for (int64_t pc = blockIdx.x; pc < n_pieces; pc += gridDim.x) {
    bins[tid] = 0, bins[tid + kDpBlock] = 0;
    if (tid == 0) total = 0, above = 0;
    if (tid < 3) quant[tid] = 1;
    __syncthreads();
    const fcsdp_piece p = pieces[pc];
    const int64_t start = clamp64(p.start, 0, len);
    const int64_t end = clamp64(p.end, start, start + kDpPieceMax < len ? start + kDpPieceMax : len);
    int32_t li = p.long_index;
    if (start != p.start || end != p.end || li < -1 || li >= n_long) {
      if (tid == 0) atomicOr(status, kDpStatusField);
      li = -1;
    }
    unsigned long long t = 0;
    uint32_t a = 0;
    for (int64_t i = start + tid; i < end; i += kDpBlock) {
      if (!((bitmap[i >> 6] >> (i & 63)) & 1u)) continue;
      const uint32_t d = depth[i];
      atomicAdd(&bins[dp_bin(d)], 1u);
      t += d;
      a += d >= (uint32_t)kDpAbove;
    }
    if (t) atomicAdd(&total, t);
    if (a) atomicAdd(&above, a);
    __syncthreads();
    const uint32_t h0 = bins[2 * tid], h1 = bins[2 * tid + 1];
    uint32_t n;
    const uint32_t before = block_scan_excl<kDpWaves>(h0 + h1, n, wave_sums);
    if (n > 0 && li < 0)
      for (int k = 1; k <= 3; ++k) {
        if (h0 && dp_is_quantile(before, before + h0, n, k)) quant[k - 1] = dp_reported(2 * tid);
        if (h1 && dp_is_quantile(before + h0, before + h0 + h1, n, k)) quant[k - 1] = dp_reported(2 * tid + 1);
      }
    for (int bin = tid; bin < kDpBins; bin += kDpBlock) {
      const uint32_t v = bins[bin];
      if (!v) continue;
      atomicAdd(hist + bin, (unsigned long long)v);
      if (li >= 0) atomicAdd(long_hist + (size_t)li * kDpBins + bin, (unsigned long long)v);
    }
    __syncthreads();
    if (tid == 0) {
      fcsdp_summary s;
      s.total = total, s.loci = n, s.above = above;
      s.q1 = li < 0 ? quant[0] : 0, s.median = li < 0 ? quant[1] : 0, s.q3 = li < 0 ? quant[2] : 0, s.reserved = 0;
      summary[pc] = s;
    }
    __syncthreads();  // the shared cells are zeroed again
  }
}

int dp_grid(int64_t items, int per_block) {
  return (int)std::clamp<int64_t>((items + per_block - 1) / per_block, 1, kDpMaxBlocks);
}

int64_t dp_tiles(int64_t len) { return (len + kDpTile - 1) / kDpTile; }
size_t dp_ws_bytes(int64_t len) { return std::max<size_t>(4 * (size_t)dp_tiles(len), 256); }

int launch_runs(const fcsdp_batch& b, const fcsdp_params& prm, const fcsdp_window& w, int32_t* cells, int32_t* status,
                hipStream_t s) {
  if (b.n <= 0 || w.len <= 0) return FCS_OK;
  hipLaunchKernelGGL(dp_runs_kernel, dim3(dp_grid(b.n, kDpWaves)), dim3(kDpBlock), 0, s, b, prm, w, cells, status);
  FCS_HIP_CHECK(hipGetLastError());
  return FCS_OK;
}

int launch_scan(int32_t* cells, int64_t len, char* ws, int32_t* status, hipStream_t s) {
  if (len <= 0) return FCS_OK;
  const int64_t tiles = dp_tiles(len);
  uint32_t* sums = reinterpret_cast<uint32_t*>(ws);
  hipLaunchKernelGGL(dp_reduce_kernel, dim3(dp_grid(tiles, 1)), dim3(kDpBlock), 0, s, cells, len, tiles, sums);
  FCS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(dp_offsets_kernel, dim3(1), dim3(kDpBlock), 0, s, sums, tiles);
  FCS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(dp_scan_kernel, dim3(dp_grid(tiles, 1)), dim3(kDpBlock), 0, s, cells, len, tiles, sums, status);
  FCS_HIP_CHECK(hipGetLastError());
  return FCS_OK;
}

int launch_stats(const uint32_t* depth, const uint64_t* bitmap, int64_t len, const fcsdp_piece* pieces, int64_t n_pieces,
                 int32_t n_long, uint64_t* hist, uint64_t* long_hist, fcsdp_summary* summary, int32_t* status,
                 hipStream_t s) {
  if (n_pieces <= 0) return FCS_OK;
  hipLaunchKernelGGL(dp_stats_kernel, dim3((unsigned)std::clamp<int64_t>(n_pieces, 1, 8 * kDpMaxBlocks)), dim3(kDpBlock), 0, s, depth, bitmap, len, pieces, n_pieces, n_long,
                     reinterpret_cast<unsigned long long*>(hist), reinterpret_cast<unsigned long long*>(long_hist), summary,
                     status);
  FCS_HIP_CHECK(hipGetLastError());
  return FCS_OK;
}

int check_params(const fcsdp_params* p, const char* who) {
  if (!p) return fail_invalid(who, "null parameters");
  if (p->min_mapq > p->max_mapq || p->min_baseq > p->max_baseq)
    return fail_invalid(who, "a lower bound above its upper bound (MAPQ " + std::to_string(p->min_mapq) + " .. " +
                                 std::to_string(p->max_mapq) + ", base quality " + std::to_string(p->min_baseq) + " .. " +
                                 std::to_string(p->max_baseq) + ")");
  return FCS_OK;
}

int check_window(const fcsdp_window* w, const char* who) {
  if (!w) return fail_invalid(who, "null window");
  if (w->ref_id < 0) return fail_invalid(who, "window ref_id " + std::to_string(w->ref_id));
  if (w->len < 0 || w->len > FCSDP_WINDOW_MAX)
    return fail_invalid(who, "a window of " + std::to_string(w->len) + " loci (at most " + std::to_string(FCSDP_WINDOW_MAX) + ")");
  if (w->start < 0 || w->contig_len < 0 || w->start + w->len > w->contig_len)
    return fail_invalid(who, "the window " + std::to_string(w->start) + " + " + std::to_string(w->len) +
                                 " lies outside its contig of " + std::to_string(w->contig_len) + " bases");
  return FCS_OK;
}

int check_stats_scalars(int64_t len, int64_t n_pieces, int32_t n_long, const char* who) {
  if (len < 0 || len > FCSDP_WINDOW_MAX) return fail_invalid(who, "a window of " + std::to_string(len) + " loci");
  if (n_pieces < 0 || n_pieces > FCSDP_WINDOW_MAX) return fail_invalid(who, "bad piece count " + std::to_string(n_pieces));
  if (n_long < 0 || n_long > (1 << 20)) return fail_invalid(who, "bad long interval count " + std::to_string(n_long));
  return FCS_OK;
}

}  // namespace

}  // namespace fcs

using namespace fcs;

extern "C" {

int64_t fcsdp_workspace_bytes(int64_t len) {
  if (len < 0 || len > FCSDP_WINDOW_MAX) return fail_invalid("fcsdp_workspace_bytes", "a window of " + std::to_string(len) + " loci");
  return (int64_t)dp_ws_bytes(len);
}

int fcsdp_runs_dev(int32_t device, const fcsdp_batch* batch, const fcsdp_params* params, const fcsdp_window* window,
                   int32_t* dev_cells, int32_t* dev_status, void* stream) {
  const char* who = "fcsdp_runs_dev";
  int rc;
  if ((rc = check_batch_scalars(batch, false, who)) || (rc = check_params(params, who)) || (rc = check_window(window, who))) return rc;
  if (!dev_status || (batch->n > 0 && window->len > 0 && !dev_cells)) return fail_invalid(who, "null cells or status");
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  return launch_runs(*batch, *params, *window, dev_cells, dev_status, static_cast<hipStream_t>(stream));
}

int fcsdp_scan_dev(int32_t device, int32_t* dev_cells, int64_t len, void* dev_workspace, int64_t workspace_bytes,
                   int32_t* dev_status, void* stream) {
  const char* who = "fcsdp_scan_dev";
  if (len < 0 || len > FCSDP_WINDOW_MAX) return fail_invalid(who, "a window of " + std::to_string(len) + " loci");
  if (!dev_status || (len > 0 && (!dev_cells || !dev_workspace))) return fail_invalid(who, "null cells, workspace or status");
  const int64_t need = (int64_t)dp_ws_bytes(len);
  if (len > 0 && workspace_bytes < need)
    return fail_invalid(who, "the workspace holds " + std::to_string(workspace_bytes) + " bytes, the call needs " + std::to_string(need));
  int rc;
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  return launch_scan(dev_cells, len, static_cast<char*>(dev_workspace), dev_status, static_cast<hipStream_t>(stream));
}

int fcsdp_stats_dev(int32_t device, const uint32_t* dev_depth, const uint64_t* dev_bitmap, int64_t len,
                    const fcsdp_piece* dev_pieces, int64_t n_pieces, int32_t n_long, uint64_t* dev_hist,
                    uint64_t* dev_long_hist, fcsdp_summary* dev_summary, int32_t* dev_status, void* stream) {
  const char* who = "fcsdp_stats_dev";
  int rc;
  if ((rc = check_stats_scalars(len, n_pieces, n_long, who))) return rc;
  if (!dev_status || (n_pieces > 0 && (!dev_pieces || !dev_hist || !dev_summary || (len > 0 && (!dev_depth || !dev_bitmap)) ||
                                        (n_long > 0 && !dev_long_hist))))
    return fail_invalid(who, "null input, table or status");
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  return launch_stats(dev_depth, dev_bitmap, len, dev_pieces, n_pieces, n_long, dev_hist, dev_long_hist, dev_summary,
                      dev_status, static_cast<hipStream_t>(stream));
}

int fcsdp_count(int32_t device, const fcsdp_batch* b, const fcsdp_params* prm, const fcsdp_window* w, uint32_t* depth) {
  const char* who = "fcsdp_count";
  int rc;
  if ((rc = check_batch_scalars(b, false, who)) || (rc = check_params(prm, who)) || (rc = check_window(w, who))) return rc;
  if (w->len > 0 && !depth) return fail_invalid(who, "null depth array");
  if ((rc = check_batch_offsets(b, who))) return rc;
  const int64_t n = b->n;
  // what the rules refuse, before any device work
  for (int64_t r = 0; r < n; ++r) {
    if (b->ref_id[r] != w->ref_id) continue;
    const uint32_t* cigar = b->cigar + b->cigar_off[r];
    const int64_t n_ops = b->cigar_off[r + 1] - b->cigar_off[r], L = b->base_off[r + 1] - b->base_off[r];
    if (!dp_counted(b->flag[r], b->ref_id[r], n_ops, b->mapq[r], prm->min_mapq, prm->max_mapq)) continue;
    int64_t covered, ref_len;
    bool beyond;
    cigar_span(cigar, n_ops, b->pos[r], w->contig_len, covered, ref_len, beyond);
    if (covered != L) return fail_invalid(who, "the CIGAR of record " + std::to_string(r) + " does not cover its bases");
    if (beyond) return fail_invalid(who, "record " + std::to_string(r) + " has an aligned base beyond its contig");
  }
  if (n == 0 || w->len == 0) return FCS_OK;
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  Arena A;
  const BatchLayout l = layout_batch(*b, false, A);
  const size_t in_bytes = A.total;
  const size_t ocells = A.add(4 * ((size_t)w->len + 1)), ostatus = A.add(4);
  const size_t host_bytes = A.total;
  const size_t ows = A.add(dp_ws_bytes(w->len));
  CallSession S;
  if ((rc = call_session_acquire(device, host_bytes, A.total, S))) return rc;
  CallLease lease{S};
  const fcsdp_batch d = stage_batch(*b, l, S.host, S.dev);
  int32_t* cells = reinterpret_cast<int32_t*>(S.dev + ocells);
  int32_t* status = reinterpret_cast<int32_t*>(S.dev + ostatus);
  FCS_HIP_CHECK(hipMemcpyAsync(S.dev, S.host, in_bytes, hipMemcpyHostToDevice, S.s));
  FCS_HIP_CHECK(hipMemsetAsync(S.dev + ocells, 0, host_bytes - ocells, S.s));
  if ((rc = launch_runs(d, *prm, *w, cells, status, S.s))) return rc;
  if ((rc = launch_scan(cells, w->len, S.dev + ows, status, S.s))) return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S.host + ocells, S.dev + ocells, host_bytes - ocells, hipMemcpyDeviceToHost, S.s));
  FCS_HIP_CHECK(hipStreamSynchronize(S.s));
  int32_t st;
  std::memcpy(&st, S.host + ostatus, sizeof st);
  if (st & FCSDP_STATUS_OVERFLOW) return fail_invalid(who, "a depth beyond 2^31 - 1");
  if (st) return fail(FCS_ERR_DEVICE, "[E::fcsdp_count] the device clamped a checked field (status " + std::to_string(st) + ")");
  const uint32_t* got = reinterpret_cast<const uint32_t*>(S.host + ocells);
  for (int64_t i = 0; i < w->len; ++i) depth[i] += got[i];
  return FCS_OK;
}

int fcsdp_stats(int32_t device, const uint32_t* depth, const uint64_t* bitmap, int64_t len, const fcsdp_piece* pieces,
                int64_t n_pieces, int32_t n_long, uint64_t* hist, uint64_t* long_hist, fcsdp_summary* summary) {
  const char* who = "fcsdp_stats";
  int rc;
  if ((rc = check_stats_scalars(len, n_pieces, n_long, who))) return rc;
  if (n_pieces > 0 && (!pieces || !hist || !summary || (len > 0 && (!depth || !bitmap)) || (n_long > 0 && !long_hist)))
    return fail_invalid(who, "null input or table");
  for (int64_t k = 0; k < n_pieces; ++k) {
    const fcsdp_piece& p = pieces[k];
    if (p.start < 0 || p.end < p.start || p.end > len || p.end - p.start > FCSDP_PIECE_MAX)
      return fail_invalid(who, "piece " + std::to_string(k) + " [" + std::to_string(p.start) + ", " + std::to_string(p.end) +
                                   ") is outside the window of " + std::to_string(len) + " loci or longer than " +
                                   std::to_string(FCSDP_PIECE_MAX));
    if (p.long_index < -1 || p.long_index >= n_long)
      return fail_invalid(who, "long_index " + std::to_string(p.long_index) + " of piece " + std::to_string(k) + " is outside [-1, " +
                                   std::to_string(n_long) + ")");
  }
  if (n_pieces == 0) return FCS_OK;
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  const size_t words = (size_t)(len + 63) / 64, np = (size_t)n_pieces;
  Arena A;
  const size_t odepth = A.add(4 * (size_t)len), obits = A.add(8 * words), opieces = A.add(sizeof(fcsdp_piece) * np);
  const size_t in_bytes = A.total;
  const size_t ohist = A.add(8 * (size_t)kDpBins), olong = A.add(8 * (size_t)kDpBins * (size_t)n_long);
  const size_t osum = A.add(sizeof(fcsdp_summary) * np), ostatus = A.add(4);
  const size_t total = A.total;
  CallSession S;
  if ((rc = call_session_acquire(device, total, total, S))) return rc;
  CallLease lease{S};
  if (len > 0) std::memcpy(S.host + odepth, depth, 4 * (size_t)len), std::memcpy(S.host + obits, bitmap, 8 * words);
  std::memcpy(S.host + opieces, pieces, sizeof(fcsdp_piece) * np);
  FCS_HIP_CHECK(hipMemcpyAsync(S.dev, S.host, in_bytes, hipMemcpyHostToDevice, S.s));
  FCS_HIP_CHECK(hipMemsetAsync(S.dev + ohist, 0, total - ohist, S.s));
  if ((rc = launch_stats(reinterpret_cast<const uint32_t*>(S.dev + odepth), reinterpret_cast<const uint64_t*>(S.dev + obits), len,
                         reinterpret_cast<const fcsdp_piece*>(S.dev + opieces), n_pieces, n_long,
                         reinterpret_cast<uint64_t*>(S.dev + ohist), reinterpret_cast<uint64_t*>(S.dev + olong),
                         reinterpret_cast<fcsdp_summary*>(S.dev + osum), reinterpret_cast<int32_t*>(S.dev + ostatus), S.s)))
    return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S.host + ohist, S.dev + ohist, total - ohist, hipMemcpyDeviceToHost, S.s));
  FCS_HIP_CHECK(hipStreamSynchronize(S.s));
  int32_t st;
  std::memcpy(&st, S.host + ostatus, sizeof st);
  if (st) return fail(FCS_ERR_DEVICE, "[E::fcsdp_stats] the device clamped a checked field (status " + std::to_string(st) + ")");
  const uint64_t* h = reinterpret_cast<const uint64_t*>(S.host + ohist);
  const uint64_t* lh = reinterpret_cast<const uint64_t*>(S.host + olong);
  for (int k = 0; k < kDpBins; ++k) hist[k] += h[k];
  for (size_t k = 0; k < (size_t)kDpBins * (size_t)n_long; ++k) long_hist[k] += lh[k];
  std::memcpy(summary, S.host + osum, sizeof(fcsdp_summary) * np);
  return FCS_OK;
}

}  // extern "C"
