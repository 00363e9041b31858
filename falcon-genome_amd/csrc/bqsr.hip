// Base quality recalibration on the device (include/fcsbq.h; DESIGN §2 [EXT],
// §4.10).  The per-base logic is csrc/bq_covars.h (one text for these kernels
// and tools/micro/bqsr_test.cpp).  All work of a call is queued on one stream,
// without a host round trip.
//
// bq_count_kernel: a block takes a contiguous slice of the records, a wave one
// record at a time, a lane one kept base: the wave finds the record's clips
// and low-quality ends (one CIGAR pass, ballots over the qualities), then each
// lane locates its base in the CIGAR, reads the reference byte and the
// known-sites word, and adds 1 | error << 32 to one context cell and one cycle
// cell.  The device table has one row of 16 + 1000 packed 64-bit cells per
// (read group, quality).  The contexts of the block's read group (that of its
// slice's first record; the host groups a batch by read group) are privatised
// in 94 x 16 LDS cells and flushed once per block; the cycles, and the contexts
// of any other read group, go to global 64-bit atomics in one of R replicas of
// the table, chosen by block index.  A call holds fewer than 2^32 bases, so
// the halves of a cell never carry.
// bq_count_kernel is built for 6 waves per SIMD.
//
// bq_fold_kernel: one lane per cell: the sum of the R replicas, split into
// (observations, errors) and added to the caller's tables -- unless the status
// word is set, in which case nothing is added.
// bq_fold_kernel is built for 8 waves per SIMD.
//
// bq_check_kernel: one lane per record: offsets, read group and the 500-base
// limit of apply, into the status word.
// bq_check_kernel is built for 8 waves per SIMD.
//
// bq_apply_kernel: a wave per record, a lane per base: the keys, three table
// reads, the fp64 sum in the rules' order, one byte.  Records that are not
// recalibrated are copied.  Nothing is written when bq_check_kernel set the
// status word.
// bq_apply_kernel is built for 8 waves per SIMD.
//
// Every loop is bounded by n, a record's clamped CIGAR word count or its clamped
// base count; no kernel uses scratch.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "bq_covars.h"
#include "fcsbq.h"
#include "fcship_internal.h"
#include "rec_batch.h"

struct fcsbq_ref {
  int32_t device = 0;
  int32_t n_ref = 0;
  uint8_t* bases = nullptr;
  int64_t* ref_off = nullptr;
  uint64_t* known = nullptr;
  std::vector<int64_t> host_off;  // ref_off, for the checks before the device
};

namespace fcs {

namespace {

constexpr int kBqBlock = 256;
constexpr int kBqWaves = kBqBlock / 64;
constexpr int kBqMaxBlocks = 2048;
constexpr int kBqMinSlice = 32;  // records per block at least

struct BqDevRef {
  const uint8_t* bases;
  const int64_t* ref_off;
  const uint64_t* known;
  int32_t n_ref;
};

// The low-quality ends of qual[0, k), k <= 500, found by the whole wave.
__device__ __forceinline__ void wave_low_ends(const uint8_t* qual, int64_t k, int lane, int64_t& nl, int64_t& nr) {
  int64_t first = k, last = -1;
  for (int64_t c0 = 0; c0 < k; c0 += 64) {
    const int64_t j = c0 + lane;
    const unsigned long long m = __ballot(j < k && qual[j] > 2);
    if (m) {
      if (first == k) first = c0 + __ffsll((long long)m) - 1;
      last = c0 + 63 - __clzll((long long)m);
    }
  }
  nl = first;
  nr = last < 0 ? k : k - 1 - last;
}

__global__ __launch_bounds__(kBqBlock) void bq_count_kernel(fcsbq_batch b, BqDevRef ref, int32_t n_rg, int64_t slice,
                                                            unsigned long long* __restrict__ tab, int32_t replicas,
                                                            int32_t* __restrict__ status) {
  __shared__ unsigned long long lds[kBqNq * kBqNctx];
  for (int i = (int)threadIdx.x; i < kBqNq * kBqNctx; i += kBqBlock) lds[i] = 0;
  const int64_t r_begin = (int64_t)blockIdx.x * slice;
  const int64_t r_end = r_begin + slice < b.n ? r_begin + slice : b.n;
  int32_t brg = r_begin < r_end ? b.rg[r_begin] : -1;
  if (brg >= n_rg) brg = -1;
  unsigned long long* rep = tab + (size_t)((int)blockIdx.x % replicas) * (size_t)n_rg * kBqNq * kBqCols;
  __syncthreads();
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  for (int64_t r = r_begin + wave; r < r_end; r += kBqWaves) {  // r is the wave's: its ballots see whole waves
    int bad = 0;
    int32_t rg = b.rg[r];
    if (rg < -1 || rg >= n_rg) bad |= FCSBQ_STATUS_FIELD, rg = -1;
    const uint16_t flag = b.flag[r];
    if (!bq_counted(flag, rg, b.mapq[r], b.qual_absent[r] != 0)) {
      if (bad && lane == 0) atomicOr(status, bad);
      continue;
    }
    // rec_fields' ranges in this kernel's own order (bases first): the shared order changes its machine code
    const int64_t o0 = b.base_off[r], o1 = b.base_off[r + 1];
    const int64_t q0 = clamp64(o0, 0, b.n_bases), q1 = clamp64(o1, q0, b.n_bases);
    const int64_t k0 = b.cigar_off[r], k1 = b.cigar_off[r + 1];
    const int64_t c0 = clamp64(k0, 0, b.n_cigar), c1 = clamp64(k1, c0, b.n_cigar);
    const int32_t c = b.ref_id[r];
    const uint32_t* cigar = b.cigar + c0;
    const int64_t n_ops = c1 - c0, L = q1 - q0;
    int64_t lead, trail, covered;
    bq_clips(cigar, n_ops, lead, trail, covered);
    if (q0 != o0 || q1 != o1 || c0 != k0 || c1 != k1 || c < 0 || c >= ref.n_ref || covered != L) bad |= FCSBQ_STATUS_FIELD;
    const int64_t k = L - lead - trail;
    if (!bad && k > kBqMaxCycle) bad |= FCSBQ_STATUS_LONG;
    if (bad) {  // the record adds nothing
      if (lane == 0) atomicOr(status, bad);
      continue;
    }
    const int64_t g0 = ref.ref_off[c], clen = ref.ref_off[c + 1] - g0;
    const uint8_t* seq = b.bases + q0 + lead;
    const uint8_t* qual = b.qual + q0 + lead;
    int64_t nl, nr;
    wave_low_ends(qual, k, lane, nl, nr);
    const bool reverse = flag & kBqFlagReverse, second = bq_second(flag);
    const int32_t pos = b.pos[r];
    for (int64_t j = lane; j < k; j += 64) {
      const int q = qual[j], code = bq_code(seq[j]);
      int64_t p;
      const int kind = bq_site(cigar, n_ops, pos, lead + j, p);
      if (bq_skipped(kind, code, q)) continue;
      const bool inside = p >= 0 && p < clen;
      if (kind == kBqAligned && !inside) {  // clamped: not counted
        atomicOr(status, FCSBQ_STATUS_REF);
        continue;
      }
      if (inside && bq_known(ref.known, g0 + p)) continue;
      const unsigned long long add = 1ull | ((unsigned long long)(bq_error(kind, code, inside ? ref.bases[g0 + p] : 0) ? 1 : 0) << 32);
      const int ck = bq_context(seq, k, j, nl, nr, reverse);
      const size_t row = ((size_t)rg * kBqNq + (size_t)q) * kBqCols;
      if (ck >= 0) {
        if (rg == brg) atomicAdd(&lds[q * kBqNctx + ck], add);
        else atomicAdd(rep + row + ck, add);
      }
      atomicAdd(rep + row + kBqNctx + bq_cycle(k, j, reverse, second), add);
    }
  }
  __syncthreads();
  if (brg >= 0)
    for (int i = (int)threadIdx.x; i < kBqNq * kBqNctx; i += kBqBlock) {
      const unsigned long long v = lds[i];
      if (v) atomicAdd(rep + ((size_t)brg * kBqNq + (size_t)(i / kBqNctx)) * kBqCols + (i % kBqNctx), v);
    }
}

__global__ __launch_bounds__(kBqBlock) void bq_fold_kernel(const unsigned long long* __restrict__ tab, int32_t replicas,
                                                           int64_t cells, const int32_t* __restrict__ status,
                                                           int64_t* __restrict__ ctx, int64_t* __restrict__ cyc) {
  if (*status != 0) return;
  const int64_t stride = (int64_t)gridDim.x * kBqBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBqBlock + threadIdx.x; i < cells; i += stride) {
    unsigned long long v = 0;
    for (int32_t k = 0; k < replicas; ++k) v += tab[(size_t)k * (size_t)cells + (size_t)i];
    if (!v) continue;
    const int64_t row = i / kBqCols;
    const int col = (int)(i % kBqCols);
    int64_t* out = col < kBqNctx ? ctx + 2 * (row * kBqNctx + col) : cyc + 2 * (row * kBqNcyc + (col - kBqNctx));
    out[0] += (int64_t)(v & 0xffffffffull);
    out[1] += (int64_t)(v >> 32);
  }
}

__global__ __launch_bounds__(kBqBlock) void bq_check_kernel(fcsbq_batch b, int32_t n_rg, int32_t* __restrict__ status) {
  const int64_t stride = (int64_t)gridDim.x * kBqBlock;
  for (int64_t r = (int64_t)blockIdx.x * kBqBlock + threadIdx.x; r < b.n; r += stride) {
    const int64_t o0 = b.base_off[r], o1 = b.base_off[r + 1];
    const int32_t rg = b.rg[r];
    int bad = 0;
    if (o0 < 0 || o1 < o0 || o1 > b.n_bases || rg < -1 || rg >= n_rg) bad |= FCSBQ_STATUS_FIELD;
    else if (bq_applied(rg, b.qual_absent[r] != 0) && o1 - o0 > kBqMaxCycle) bad |= FCSBQ_STATUS_LONG;
    if (bad) atomicOr(status, bad);
  }
}

__global__ __launch_bounds__(kBqBlock) void bq_apply_kernel(fcsbq_batch b, int32_t n_rg, const double* __restrict__ base,
                                                            const double* __restrict__ dctx,
                                                            const double* __restrict__ dcyc,
                                                            const int32_t* __restrict__ status,
                                                            uint8_t* __restrict__ out) {
  if (*status != 0) return;
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  const int64_t stride = (int64_t)gridDim.x * kBqWaves;
  for (int64_t r = (int64_t)blockIdx.x * kBqWaves + wave; r < b.n; r += stride) {
    const int64_t q0 = clamp64(b.base_off[r], 0, b.n_bases), q1 = clamp64(b.base_off[r + 1], q0, b.n_bases);
    const int64_t k = q1 - q0;
    const int32_t rg = b.rg[r];
    const uint8_t* seq = b.bases + q0;
    const uint8_t* qual = b.qual + q0;
    if (!bq_applied(rg, b.qual_absent[r] != 0) || rg >= n_rg || k > kBqMaxCycle) {  // copied (the latter two: flagged before)
      for (int64_t j = lane; j < k; j += 64) out[q0 + j] = qual[j];
      continue;
    }
    const uint16_t flag = b.flag[r];
    int64_t nl, nr;
    wave_low_ends(qual, k, lane, nl, nr);
    const bool reverse = flag & kBqFlagReverse, second = bq_second(flag);
    for (int64_t j = lane; j < k; j += 64) {
      const int q = qual[j];
      uint8_t v = (uint8_t)q;
      if (q >= 6 && q < kBqNq) {
        const int ck = bq_context(seq, k, j, nl, nr, reverse);
        const size_t row = (size_t)rg * kBqNq + (size_t)q;
        v = bq_new_quality(base[row], ck >= 0 ? dctx[row * kBqNctx + ck] : 0.0,
                           dcyc[row * kBqNcyc + bq_cycle(k, j, reverse, second)]);
      }
      out[q0 + j] = v;
    }
  }
}

// Replicas of the count table: 16 (1, 4, 8 and 16 were measured,
// each step faster), fewer when the read groups are many (64 MiB of replicas
// at most); FCS_BQ_REPLICAS (1 .. 64) sets it for measurements.
int32_t bq_replicas(int32_t n_rg) {
  const size_t one = (size_t)std::max(n_rg, 1) * kBqNq * kBqCols * 8;
  int64_t r = std::clamp<int64_t>((int64_t)(((size_t)64 << 20) / one), 1, 16);
  if (const char* e = std::getenv("FCS_BQ_REPLICAS")) {
    const long v = std::strtol(e, nullptr, 10);
    if (v >= 1 && v <= 64) r = v;
  }
  return (int32_t)r;
}

size_t bq_ws_bytes(int32_t n_rg) { return (size_t)bq_replicas(n_rg) * (size_t)std::max(n_rg, 1) * kBqNq * kBqCols * 8; }

int grid_for(int64_t items, int per_block) {
  return (int)std::clamp<int64_t>((items + per_block - 1) / per_block, 1, kBqMaxBlocks);
}

// The count of one batch on stream s: the replicas zeroed, counted and folded
// into ctx / cyc (device tables of (observations, errors) pairs).  status is zeroed here.
int launch_count(const fcsbq_batch& b, const BqDevRef& ref, int32_t n_rg, char* ws, int64_t* ctx, int64_t* cyc,
                 int32_t* status, hipStream_t s) {
  FCS_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), s));
  if (b.n <= 0 || n_rg <= 0) return FCS_OK;
  const int32_t R = bq_replicas(n_rg);
  FCS_HIP_CHECK(hipMemsetAsync(ws, 0, bq_ws_bytes(n_rg), s));
  const int blocks = grid_for(b.n, kBqMinSlice);
  const int64_t slice = (b.n + blocks - 1) / blocks;
  unsigned long long* tab = reinterpret_cast<unsigned long long*>(ws);
  hipLaunchKernelGGL(bq_count_kernel, dim3(blocks), dim3(kBqBlock), 0, s, b, ref, n_rg, slice, tab, R, status);
  FCS_HIP_CHECK(hipGetLastError());
  const int64_t cells = (int64_t)n_rg * kBqNq * kBqCols;
  hipLaunchKernelGGL(bq_fold_kernel, dim3(grid_for(cells, kBqBlock)), dim3(kBqBlock), 0, s, tab, R, cells, status, ctx, cyc);
  FCS_HIP_CHECK(hipGetLastError());
  return FCS_OK;
}

int launch_apply(const fcsbq_batch& b, int32_t n_rg, const double* base, const double* dctx, const double* dcyc,
                 uint8_t* out, int32_t* status, hipStream_t s) {
  FCS_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), s));
  if (b.n <= 0) return FCS_OK;
  hipLaunchKernelGGL(bq_check_kernel, dim3(grid_for(b.n, kBqBlock)), dim3(kBqBlock), 0, s, b, n_rg, status);
  FCS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(bq_apply_kernel, dim3(grid_for(b.n, kBqWaves)), dim3(kBqBlock), 0, s, b, n_rg, base, dctx, dcyc,
                     status, out);
  FCS_HIP_CHECK(hipGetLastError());
  return FCS_OK;
}

// The scalar fields of a batch, checked alike by every entry point: the shared
// check, with the two limits of this file where they have always stood, after
// its refusals of a null batch and of negative sizes.
int check_scalars(const fcsbq_batch* b, int32_t n_rg, const char* who) {
  if (b && b->n >= 0 && b->n_cigar >= 0 && b->n_bases >= 0) {
    if (b->n_bases > FCSBQ_MAX_BASES)
      return fail_invalid(who, std::to_string(b->n_bases) + " bases: a call holds fewer than 2^32");
    if (n_rg < 0 || n_rg > FCSBQ_MAX_RG)
      return fail_invalid(who, std::to_string(n_rg) + " read groups (at most " + std::to_string(FCSBQ_MAX_RG) + ")");
  }
  return check_batch_scalars(b, true, who);
}

// Every offset and read group of a batch of host arrays.
int check_arrays(const fcsbq_batch* b, int32_t n_rg, const char* who) {
  const int rc = check_batch_offsets(b, who);
  if (rc) return rc;
  for (int64_t r = 0; r < b->n; ++r)
    if (b->rg[r] < -1 || b->rg[r] >= n_rg)
      return fail_invalid(who, "read group " + std::to_string(b->rg[r]) + " of record " + std::to_string(r) + " is outside [-1, " +
                                        std::to_string(n_rg) + ")");
  return FCS_OK;
}

std::mutex g_ref_mu;
std::set<const fcsbq_ref*>& live_refs() {
  static std::set<const fcsbq_ref*>* s = new std::set<const fcsbq_ref*>;
  return *s;
}

const fcsbq_ref* live_ref(const fcsbq_ref* h, const char* who) {
  if (h) {
    std::lock_guard<std::mutex> lk(g_ref_mu);
    if (live_refs().count(h)) return h;
  }
  fail_invalid(who, h ? "the reference handle is not a live one" : "null reference handle");
  return nullptr;
}

// The shared layout and stage with the read groups, which only these batches hold, behind them.
struct BqLayout {
  BatchLayout batch;
  size_t rg;
};

BqLayout layout_of(const fcsbq_batch& b, Arena& a) {
  const BatchLayout l = layout_batch(b, true, a);
  return BqLayout{l, a.add(4 * (size_t)b.n)};
}

fcsbq_batch stage(const fcsbq_batch& b, const BqLayout& l, char* host, char* dev) {
  fcsbq_batch d = stage_batch(b, l.batch, host, dev);
  std::memcpy(host + l.rg, b.rg, 4 * (size_t)b.n);
  d.rg = reinterpret_cast<const int32_t*>(dev + l.rg);
  return d;
}

}  // namespace

}  // namespace fcs

using namespace fcs;

extern "C" {

int fcsbq_ref_create(int32_t device, const uint8_t* bases, const int64_t* ref_off, int32_t n_ref,
                     const uint64_t* known_bits, fcsbq_ref** handle) {
  const char* who = "fcsbq_ref_create";
  if (!handle) return fail_invalid(who, "null handle pointer");
  *handle = nullptr;
  if (n_ref < 0 || !ref_off || ref_off[0] != 0) return fail_invalid(who, "bad ref_off or contig count");
  for (int32_t k = 0; k < n_ref; ++k)
    if (ref_off[k + 1] < ref_off[k]) return fail_invalid(who, "ref_off is not non-decreasing at contig " + std::to_string(k));
  const int64_t total = ref_off[n_ref];
  if (total > 0 && (!bases || !known_bits)) return fail_invalid(who, "null bases or known-sites bitmap");
  int rc;
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  std::unique_ptr<fcsbq_ref> h(new fcsbq_ref);
  h->device = device, h->n_ref = n_ref;
  h->host_off.assign(ref_off, ref_off + n_ref + 1);
  const size_t words = (size_t)(total + 63) / 64;
  const size_t bytes[3] = {std::max<size_t>((size_t)total, 4), 8 * (size_t)(n_ref + 1), std::max<size_t>(8 * words, 8)};
  void* mem[3] = {nullptr, nullptr, nullptr};
  for (int k = 0; k < 3 && !rc; ++k)
    if (hipMalloc(&mem[k], bytes[k]) != hipSuccess)
      rc = fail(FCS_ERR_NOMEM, "[E::fcsbq_ref_create] hipMalloc of " + std::to_string(bytes[k]) + " bytes failed");
  if (!rc && ((total > 0 && hipMemcpy(mem[0], bases, (size_t)total, hipMemcpyHostToDevice) != hipSuccess) ||
              hipMemcpy(mem[1], ref_off, bytes[1], hipMemcpyHostToDevice) != hipSuccess ||
              (words > 0 && hipMemcpy(mem[2], known_bits, 8 * words, hipMemcpyHostToDevice) != hipSuccess)))
    rc = fail(FCS_ERR_DEVICE, "[E::fcsbq_ref_create] the copy to the device failed");
  if (rc) {
    for (void* m : mem)
      if (m) (void)hipFree(m);
    return rc;
  }
  h->bases = static_cast<uint8_t*>(mem[0]), h->ref_off = static_cast<int64_t*>(mem[1]), h->known = static_cast<uint64_t*>(mem[2]);
  {
    std::lock_guard<std::mutex> lk(g_ref_mu);
    live_refs().insert(h.get());
  }
  *handle = h.release();
  return FCS_OK;
}

int fcsbq_ref_destroy(fcsbq_ref* handle) {
  if (!handle) return FCS_OK;
  {
    std::lock_guard<std::mutex> lk(g_ref_mu);
    if (!live_refs().erase(handle)) return fail_invalid("fcsbq_ref_destroy", "the reference handle is not a live one");
  }
  std::unique_ptr<fcsbq_ref> h(handle);
  FCS_SET_DEVICE((h->device));
  (void)hipFree(h->bases), (void)hipFree(h->ref_off), (void)hipFree(h->known);
  return FCS_OK;
}

int64_t fcsbq_workspace_bytes(int32_t n_rg) {
  if (n_rg < 0 || n_rg > FCSBQ_MAX_RG) return fail_invalid("fcsbq_workspace_bytes", "bad read group count " + std::to_string(n_rg));
  return (int64_t)bq_ws_bytes(n_rg);
}

int fcsbq_count_dev(const fcsbq_ref* handle, const fcsbq_batch* batch, int32_t n_rg, void* dev_workspace,
                    int64_t workspace_bytes, int64_t* dev_ctx, int64_t* dev_cyc, int32_t* dev_status, void* stream) {
  const char* who = "fcsbq_count_dev";
  int rc = check_scalars(batch, n_rg, who);
  if (rc) return rc;
  if (!dev_status || (batch->n > 0 && n_rg > 0 && (!dev_ctx || !dev_cyc || !dev_workspace)))
    return fail_invalid(who, "null output or workspace");
  const int64_t need = (int64_t)bq_ws_bytes(n_rg);
  if (batch->n > 0 && n_rg > 0 && workspace_bytes < need)
    return fail_invalid(who, "the workspace holds " + std::to_string(workspace_bytes) + " bytes, the call needs " + std::to_string(need));
  const fcsbq_ref* h = live_ref(handle, who);
  if (!h) return FCS_ERR_INVALID;
  FCS_SET_DEVICE((h->device));
  return launch_count(*batch, BqDevRef{h->bases, h->ref_off, h->known, h->n_ref}, n_rg, static_cast<char*>(dev_workspace),
                      dev_ctx, dev_cyc, dev_status, static_cast<hipStream_t>(stream));
}

int fcsbq_apply_dev(int32_t device, const fcsbq_batch* batch, int32_t n_rg, const double* dev_base,
                    const double* dev_dctx, const double* dev_dcyc, uint8_t* dev_out_qual, int32_t* dev_status,
                    void* stream) {
  const char* who = "fcsbq_apply_dev";
  int rc = check_scalars(batch, n_rg, who);
  if (rc) return rc;
  if (!dev_status || (batch->n > 0 && n_rg > 0 && (!dev_base || !dev_dctx || !dev_dcyc)) ||
      (batch->n_bases > 0 && batch->n > 0 && !dev_out_qual))
    return fail_invalid(who, "null table or output");
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  return launch_apply(*batch, n_rg, dev_base, dev_dctx, dev_dcyc, dev_out_qual, dev_status, static_cast<hipStream_t>(stream));
}

int fcsbq_count(const fcsbq_ref* handle, const fcsbq_batch* b, int32_t n_rg, int64_t* ctx, int64_t* cyc) {
  const char* who = "fcsbq_count";
  int rc = check_scalars(b, n_rg, who);
  if (rc) return rc;
  if (n_rg > 0 && (!ctx || !cyc)) return fail_invalid(who, "null table");
  if ((rc = check_arrays(b, n_rg, who))) return rc;
  const fcsbq_ref* h = live_ref(handle, who);
  if (!h) return FCS_ERR_INVALID;
  const int64_t n = b->n;
  // what the rules refuse, before any device work
  for (int64_t r = 0; r < n; ++r) {
    if (!bq_counted(b->flag[r], b->rg[r], b->mapq[r], b->qual_absent[r] != 0)) continue;
    const uint32_t* cigar = b->cigar + b->cigar_off[r];
    const int64_t n_ops = b->cigar_off[r + 1] - b->cigar_off[r], L = b->base_off[r + 1] - b->base_off[r];
    int64_t lead, trail, covered;
    bq_clips(cigar, n_ops, lead, trail, covered);
    if (covered != L) return fail_invalid(who, "the CIGAR of record " + std::to_string(r) + " does not cover its bases");
    const int32_t c = b->ref_id[r];
    if (c < 0 || c >= h->n_ref)
      return fail_invalid(who, "ref_id " + std::to_string(c) + " of record " + std::to_string(r) + " is outside [0, " +
                                   std::to_string(h->n_ref) + ")");
    if (L - lead - trail > FCSBQ_MAX_CYCLE)
      return fail_invalid(who, "record " + std::to_string(r) + " has " + std::to_string(L - lead - trail) +
                                   " kept bases, more than " + std::to_string(FCSBQ_MAX_CYCLE));
    const int64_t clen = h->host_off[(size_t)c + 1] - h->host_off[(size_t)c];
    int64_t ref_len;
    bool beyond;
    cigar_span(cigar, n_ops, b->pos[r], clen, covered, ref_len, beyond);
    if (beyond) return fail_invalid(who, "record " + std::to_string(r) + " has an aligned base beyond its contig");
  }
  if (n == 0 || n_rg == 0) return FCS_OK;
  FCS_SET_DEVICE((h->device));
  Arena A;
  const BqLayout l = layout_of(*b, A);
  const size_t in_bytes = A.total;
  const size_t nctx = 16 * (size_t)n_rg * kBqNq * kBqNctx, ncyc = 16 * (size_t)n_rg * kBqNq * kBqNcyc;
  const size_t octx = A.add(nctx), ocyc = A.add(ncyc), ostatus = A.add(4);
  const size_t host_bytes = A.total;
  const size_t ows = A.add(bq_ws_bytes(n_rg));
  CallSession S;
  if ((rc = call_session_acquire(h->device, host_bytes, A.total, S))) return rc;
  CallLease lease{S};
  const fcsbq_batch d = stage(*b, l, S.host, S.dev);
  FCS_HIP_CHECK(hipMemcpyAsync(S.dev, S.host, in_bytes, hipMemcpyHostToDevice, S.s));
  FCS_HIP_CHECK(hipMemsetAsync(S.dev + octx, 0, ostatus - octx, S.s));
  if ((rc = launch_count(d, BqDevRef{h->bases, h->ref_off, h->known, h->n_ref}, n_rg, S.dev + ows,
                         reinterpret_cast<int64_t*>(S.dev + octx), reinterpret_cast<int64_t*>(S.dev + ocyc),
                         reinterpret_cast<int32_t*>(S.dev + ostatus), S.s)))
    return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S.host + octx, S.dev + octx, host_bytes - octx, hipMemcpyDeviceToHost, S.s));
  FCS_HIP_CHECK(hipStreamSynchronize(S.s));
  int32_t status;
  std::memcpy(&status, S.host + ostatus, sizeof status);
  if (status & FCSBQ_STATUS_LONG) return fail_invalid(who, "a record has more than " + std::to_string(FCSBQ_MAX_CYCLE) + " kept bases");
  if (status) return fail(FCS_ERR_DEVICE, "[E::fcsbq_count] the device clamped a checked field (status " + std::to_string(status) + ")");
  const int64_t* dc = reinterpret_cast<const int64_t*>(S.host + octx);
  const int64_t* dy = reinterpret_cast<const int64_t*>(S.host + ocyc);
  for (size_t i = 0; i < nctx / 8; ++i) ctx[i] += dc[i];
  for (size_t i = 0; i < ncyc / 8; ++i) cyc[i] += dy[i];
  return FCS_OK;
}

int fcsbq_apply(int32_t device, const fcsbq_batch* b, int32_t n_rg, const double* base, const double* dctx,
                const double* dcyc, uint8_t* out_qual) {
  const char* who = "fcsbq_apply";
  int rc = check_scalars(b, n_rg, who);
  if (rc) return rc;
  if (n_rg > 0 && (!base || !dctx || !dcyc)) return fail_invalid(who, "null table");
  if ((rc = check_arrays(b, n_rg, who))) return rc;
  const int64_t n = b->n;
  if (n > 0 && b->base_off[n] > b->base_off[0] && !out_qual) return fail_invalid(who, "null output");
  for (int64_t r = 0; r < n; ++r)
    if (bq_applied(b->rg[r], b->qual_absent[r] != 0) && b->base_off[r + 1] - b->base_off[r] > FCSBQ_MAX_CYCLE)
      return fail_invalid(who, "record " + std::to_string(r) + " has " + std::to_string(b->base_off[r + 1] - b->base_off[r]) +
                                   " bases, more than " + std::to_string(FCSBQ_MAX_CYCLE));
  if (n == 0 || b->base_off[n] == b->base_off[0]) return FCS_OK;
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  Arena A;
  const BqLayout l = layout_of(*b, A);
  const size_t nbase = 8 * (size_t)std::max(n_rg, 1) * kBqNq;
  const size_t obase = A.add(nbase), odctx = A.add(nbase * kBqNctx), odcyc = A.add(nbase * kBqNcyc);
  const size_t in_bytes = A.total;
  const size_t nb = (size_t)b->base_off[n];  // the output is indexed by the caller's offsets
  const size_t oout = A.add(nb), ostatus = A.add(4);
  const size_t total = A.total;
  CallSession S;
  if ((rc = call_session_acquire(device, total, total, S))) return rc;
  CallLease lease{S};
  const fcsbq_batch d = stage(*b, l, S.host, S.dev);
  if (n_rg > 0) {
    std::memcpy(S.host + obase, base, 8 * (size_t)n_rg * kBqNq);
    std::memcpy(S.host + odctx, dctx, 8 * (size_t)n_rg * kBqNq * kBqNctx);
    std::memcpy(S.host + odcyc, dcyc, 8 * (size_t)n_rg * kBqNq * kBqNcyc);
  }
  FCS_HIP_CHECK(hipMemcpyAsync(S.dev, S.host, in_bytes, hipMemcpyHostToDevice, S.s));
  if ((rc = launch_apply(d, n_rg, reinterpret_cast<const double*>(S.dev + obase), reinterpret_cast<const double*>(S.dev + odctx),
                         reinterpret_cast<const double*>(S.dev + odcyc), reinterpret_cast<uint8_t*>(S.dev + oout),
                         reinterpret_cast<int32_t*>(S.dev + ostatus), S.s)))
    return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S.host + oout, S.dev + oout, total - oout, hipMemcpyDeviceToHost, S.s));
  FCS_HIP_CHECK(hipStreamSynchronize(S.s));
  int32_t status;
  std::memcpy(&status, S.host + ostatus, sizeof status);
  if (status) return fail(FCS_ERR_DEVICE, "[E::fcsbq_apply] the device clamped a checked field (status " + std::to_string(status) + ")");
  const size_t first = (size_t)b->base_off[0];
  std::memcpy(out_qual + first, S.host + oout + first, nb - first);
  return FCS_OK;
}

}  // extern "C"
