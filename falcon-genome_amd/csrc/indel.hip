// Indel realignment's scoring step on the device (include/fcsir.h; DESIGN §2
// [EXT], §4.14).  The rules are csrc/ir_rules.h (one text for these kernels,
// host/indel.cpp and tools/micro/ir_test.cpp).  All work of a call is queued on
// one stream, without a host round trip.
//
// ir_pairs_kernel: the exclusive scan of the bins' pair counts C_b R_b by one
// block, in passes of 256 bins; the total and the "more pairs than max_pairs"
// bit.
// ir_pairs_kernel is built for 8 waves per SIMD.
//
// ir_score_kernel: a block per (bin, consensus) over a bounded grid.  The
// consensus is staged once in LDS as ir_mask bytes (zero beyond its end), four
// to a dword.  A wave takes every fourth alt read of the bin and stages it in
// its own LDS rows as (ir_hot bytes, quality bytes) per four bases; a lane is
// the candidate offset o = 64 t + lane of tile t and walks the read four bases
// at a time: one LDS dword of the consensus per step (the dword above it is
// kept from the step before) and a byte align by o & 3, one AND against the
// read's hot bytes, three operations that turn "non-zero byte" into 0 / 1 bytes,
// and one 4 x u8 dot product with the qualities.  The read's dwords are read at
// a wave-uniform address.  The original offset, the only candidate that may
// overhang the consensus, is scored once per read with a lane per base.  The
// (score, not-orig, offset) key is reduced across the wave once per read.
// ir_score_kernel is built for 8 waves per SIMD.
//
// Every loop is bounded by a count of bins, sequences, reads, bases or offsets;
// no kernel uses scratch.
#include <algorithm>
#include <cstring>
#include <string>

#include "fcship_internal.h"
#include "fcsir.h"
#include "ir_rules.h"
#include "rec_batch.h"

namespace fcs {

namespace {

constexpr int kIrBlock = 256;
constexpr int kIrWaves = kIrBlock / 64;
// launch cap of ir_score_kernel's stride loop over the sequences
constexpr int kIrMaxBlocks = 2048;
// the consensus in LDS: a lane reads up to the dword above its last base's
constexpr int kIrSeqWords = kIrSeqMax / 4 + 4;

static_assert(FCSIR_READ_MAX == kIrReadMax && FCSIR_SEQ_MAX == kIrSeqMax && FCSIR_OVERHANG == kIrOverhang &&
                  FCSIR_ORIG_MAX == kIrOrigMax && FCSIR_STATUS_FIELD == kIrStatusField && FCSIR_STATUS_PAIRS == kIrStatusPairs,
              "fcsir.h and ir_rules.h");
static_assert(sizeof(fcsir_batch) == 104, "argument layout");
static_assert(kIrReadMax % 4 == 0 && kIrSeqMax % 4 == 0, "four bases to a dword");

// The clamped range [lo, hi) of off[k], off[k + 1] within [0, total], at most max_len long; false when clamped.
__device__ __forceinline__ bool ir_range(const int64_t* off, int64_t k, int64_t total, int64_t max_len, int64_t& lo, int64_t& hi) {
  const int64_t a = off[k], b = off[k + 1];
  lo = clamp64(a, 0, total), hi = clamp64(b, lo, total);
  bool ok = lo == a && hi == b;
  if (hi - lo > max_len) hi = lo + max_len, ok = false;
  return ok;
}

// pair_first[b]: the pairs before bin b; pair_first[n_bins] and *n_pairs the total.
__global__ __launch_bounds__(kIrBlock) void ir_pairs_kernel(fcsir_batch b, int64_t max_pairs, int64_t* __restrict__ pair_first,
                                                            int64_t* __restrict__ n_pairs, int32_t* __restrict__ status) {
  __shared__ int64_t wave_sums[kIrWaves];
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  int64_t carry = 0;
  bool clamped = false;
  for (int64_t t0 = 0; t0 < b.n_bins; t0 += kIrBlock) {
    const int64_t t = t0 + (int64_t)threadIdx.x;
    int64_t v = 0;
    if (t < b.n_bins) {
      int64_t s0, s1, r0, r1;
      if (!ir_range(b.bin_seq, t, b.n_seq, INT32_MAX, s0, s1)) clamped = true;
      if (!ir_range(b.bin_read, t, b.n_reads, INT32_MAX, r0, r1)) clamped = true;
      v = (s1 - s0) * (r1 - r0);
    }
    int64_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t up = __shfl_up(inc, d);
      if (lane >= d) inc += up;
    }
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    int64_t before = 0, total = 0;
    for (int k = 0; k < kIrWaves; ++k) {
      const int64_t s = wave_sums[k];
      if (k < wave) before += s;
      total += s;
    }
    __syncthreads();  // wave_sums is written again
    if (t < b.n_bins) pair_first[t] = carry + before + inc - v;
    carry += total;
  }
  if (clamped) atomicOr(status, kIrStatusField);
  if (threadIdx.x == 0) {
    pair_first[b.n_bins] = carry;
    *n_pairs = carry;
    if (carry > max_pairs) atomicOr(status, kIrStatusPairs);
  }
}

__device__ __forceinline__ uint32_t ir_wave_sum(uint32_t v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

__device__ __forceinline__ uint64_t ir_wave_min(uint64_t v) {
  for (int d = 32; d >= 1; d >>= 1) {
    const uint64_t o = __shfl_xor(v, d);
    if (o < v) v = o;
  }
  return v;
}

__global__ __launch_bounds__(kIrBlock) void ir_score_kernel(fcsir_batch b, const int64_t* __restrict__ pair_first, int64_t max_pairs,
                                                            uint32_t* __restrict__ best, int32_t* __restrict__ off,
                                                            int32_t* __restrict__ status) {
  __shared__ uint32_t seq_w[kIrSeqWords];               // ir_mask bytes, zero beyond the end
  __shared__ uint2 read_w[kIrWaves][kIrReadMax / 4];    // (ir_hot bytes, quality bytes) of four bases
  const int tid = (int)threadIdx.x, wave = tid / 64, lane = tid % 64;
  for (int64_t s = blockIdx.x; s < b.n_seq; s += gridDim.x) {
    // the last bin with bin_seq[bin] <= s; every value of this part is the same in the whole block
    int64_t lo = 0, hi = b.n_bins;
    while (lo < hi) {
      const int64_t mid = (lo + hi) / 2;
      if (b.bin_seq[mid + 1] > s) hi = mid;
      else lo = mid + 1;
    }
    const int64_t bin = lo;
    if (bin >= b.n_bins || b.bin_seq[bin] > s || b.bin_seq[bin] < 0) {  // no bin holds the sequence
      if (tid == 0) atomicOr(status, kIrStatusField);
      continue;
    }
    bool clamped = false;
    int64_t q0, q1, r0, r1;
    if (!ir_range(b.seq_off, s, b.n_seq_bytes, kIrSeqMax, q0, q1)) clamped = true;
    if (!ir_range(b.bin_read, bin, b.n_reads, INT32_MAX, r0, r1)) clamped = true;
    const int len = (int)(q1 - q0);
    const int64_t R = r1 - r0;
    const int64_t base = pair_first[bin] + (s - b.bin_seq[bin]) * R;
    __syncthreads();  // the sequence before is not read any more
    for (int w = tid; w < kIrSeqWords; w += kIrBlock) {
      uint32_t v = 0;
      for (int k = 0; k < 4; ++k)
        if (4 * w + k < len) v |= ir_mask(b.seq[q0 + 4 * w + k]) << (8 * k);
      seq_w[w] = v;
    }
    for (int64_t rr = 0; rr < R; rr += kIrWaves) {  // the same trips in every wave, for the barriers
      const bool have = rr + wave < R;
      const int64_t r = r0 + rr + wave;
      int64_t p0 = 0, p1 = 0;
      int32_t orig = 0;
      if (have) {
        if (!ir_range(b.read_off, r, b.n_read_bytes, kIrReadMax, p0, p1)) clamped = true;
        const int32_t og = b.orig[r];
        orig = og < 0 ? 0 : og > kIrOrigMax ? kIrOrigMax : og;
        if (orig != og) clamped = true;
      }
      const int L = (int)(p1 - p0), steps = (L + 3) / 4;
      __syncthreads();  // the sequence is staged; the wave's read before is not read any more
      for (int j = lane; j < steps; j += 64) {
        uint32_t h = 0, q = 0;
        for (int k = 0; k < 4; ++k)
          if (4 * j + k < L) h |= ir_hot(b.read[p0 + 4 * j + k]) << (8 * k), q |= (uint32_t)b.qual[p0 + 4 * j + k] << (8 * k);
        read_w[wave][j] = make_uint2(h, q);
      }
      __syncthreads();
      if (!have) continue;
      // the original offset, a lane per base
      uint32_t so = 0;
      for (int i = lane; i < L; i += 64) {
        const int64_t p = (int64_t)orig + i;
        const uint2 hq = read_w[wave][i >> 2];
        if (p >= len) so += kIrOverhang;
        else if ((seq_w[p >> 2] >> (8 * (p & 3))) & (hq.x >> (8 * (i & 3))) & 0xFFu) so += (hq.y >> (8 * (i & 3))) & 0xFFu;
      }
      uint64_t key = ir_key(ir_wave_sum(so), true, orig);
      // every offset at which the read fits, a lane per offset
      const int n_off = (int)ir_offsets(len, L);
      for (int o0 = 0; o0 < n_off; o0 += 64) {
        const int o = o0 + lane;
        const bool fits = o < n_off;
        const int oc = fits ? o : 0;
        const uint32_t* sw = seq_w + (oc >> 2);
        const uint32_t sh = (uint32_t)oc & 3u;
        uint32_t below = sw[0], acc = 0;
        for (int j = 0; j < steps; ++j) {
          const uint32_t above = sw[j + 1];
          const uint32_t s4 = __builtin_amdgcn_alignbyte(above, below, sh);  // the mask bytes at o + 4 j ..
          const uint2 hq = read_w[wave][j];
          const uint32_t t = s4 & hq.x;                                     // non-zero bytes: differing bases
          const uint32_t n = ((t + 0x7F7F7F7Fu) >> 7) & 0x01010101u;        // as 0 / 1 bytes (a byte of t is at most 8)
          acc = __builtin_amdgcn_udot4(n, hq.y, acc, false);
          below = above;
        }
        const uint64_t k = ir_key(acc, false, o);
        if (fits && k < key) key = k;
      }
      key = ir_wave_min(key);
      const int64_t p = base + (r - r0);
      if (lane == 0 && p >= 0 && p < max_pairs) best[p] = ir_key_score(key), off[p] = ir_key_offset(key);
    }
    if (clamped && lane == 0) atomicOr(status, kIrStatusField);
  }
}

size_t ir_workspace(int64_t n_bins) { return pad256(8 * ((size_t)n_bins + 1)); }

// Device pointers in b; n_seq > 0 and n_bins > 0.
int launch_score(const fcsir_batch& b, uint32_t* best, int32_t* off, int64_t max_pairs, int64_t* n_pairs, char* wsp, int32_t* status,
                 hipStream_t s) {
  int64_t* pair_first = reinterpret_cast<int64_t*>(wsp);
  hipLaunchKernelGGL(ir_pairs_kernel, dim3(1), dim3(kIrBlock), 0, s, b, max_pairs, pair_first, n_pairs, status);
  FCS_HIP_CHECK(hipGetLastError());
  const int grid = (int)std::clamp<int64_t>(b.n_seq, 1, kIrMaxBlocks);
  hipLaunchKernelGGL(ir_score_kernel, dim3(grid), dim3(kIrBlock), 0, s, b, pair_first, max_pairs, best, off, status);
  FCS_HIP_CHECK(hipGetLastError());
  return FCS_OK;
}

int check_scalars(const fcsir_batch* b, const void* best, const void* off, int64_t max_pairs, const void* n_pairs, const char* who) {
  if (!b) return fail_invalid(who, "null batch");
  if (b->n_bins < 0 || b->n_seq < 0 || b->n_reads < 0)
    return fail_invalid(who, "negative count: " + std::to_string(b->n_bins) + " bins, " + std::to_string(b->n_seq) + " sequences, " +
                                 std::to_string(b->n_reads) + " reads");
  if (b->n_bins > INT32_MAX || b->n_seq > INT32_MAX || b->n_reads > INT32_MAX) return fail_invalid(who, "a count above 2^31 - 1");
  if (b->n_seq_bytes < 0 || b->n_read_bytes < 0) return fail_invalid(who, "negative sequence or read size");
  if (max_pairs < 0) return fail_invalid(who, "max_pairs " + std::to_string(max_pairs));
  if (!n_pairs) return fail_invalid(who, "null pair count");
  if (!b->bin_seq || !b->bin_read || !b->seq_off || !b->read_off || (b->n_reads > 0 && !b->orig)) return fail_invalid(who, "null offset array");
  if ((b->n_seq_bytes > 0 && !b->seq) || (b->n_read_bytes > 0 && (!b->read || !b->qual)))
    return fail_invalid(who, "null sequence, read or quality bytes");
  if (max_pairs > 0 && (!best || !off)) return fail_invalid(who, "null output arrays");
  return FCS_OK;
}

// bin_x[0 .. n_bins] runs from 0 to n without a step back.
int check_bins(const char* who, const char* what, const int64_t* bin, int64_t n_bins, int64_t n) {
  if (bin[0] != 0) return fail_invalid(who, std::string("bin ") + what + " offsets start at " + std::to_string(bin[0]) + ", not at zero");
  const int rc = check_offsets(who, (std::string("bin ") + what).c_str(), bin, n_bins, n);
  if (rc) return rc;
  if (bin[n_bins] != n)
    return fail_invalid(who, std::string("bin ") + what + " offsets end at " + std::to_string(bin[n_bins]) + ", there are " + std::to_string(n));
  return FCS_OK;
}

}  // namespace

}  // namespace fcs

using namespace fcs;

extern "C" {

int64_t fcsir_workspace_bytes(int64_t n_bins) {
  if (n_bins < 0 || n_bins > INT32_MAX) return fail_invalid("fcsir_workspace_bytes", std::to_string(n_bins) + " bins");
  return (int64_t)ir_workspace(n_bins);
}

int fcsir_score_dev(int32_t device, const fcsir_batch* batch, uint32_t* dev_best, int32_t* dev_off, int64_t max_pairs,
                    int64_t* dev_n_pairs, void* dev_workspace, int64_t workspace_bytes, int32_t* dev_status, void* stream) {
  const char* who = "fcsir_score_dev";
  int rc;
  if ((rc = check_scalars(batch, dev_best, dev_off, max_pairs, dev_n_pairs, who))) return rc;
  if (!dev_status || !dev_workspace) return fail_invalid(who, "null workspace or status");
  const int64_t need = (int64_t)ir_workspace(batch->n_bins);
  if (workspace_bytes < need)
    return fail_invalid(who, "the workspace holds " + std::to_string(workspace_bytes) + " bytes, the call needs " + std::to_string(need));
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (batch->n_bins == 0 || batch->n_seq == 0) {
    FCS_HIP_CHECK(hipMemsetAsync(dev_n_pairs, 0, sizeof(int64_t), s));
    return FCS_OK;
  }
  return launch_score(*batch, dev_best, dev_off, max_pairs, dev_n_pairs, static_cast<char*>(dev_workspace), dev_status, s);
}

int fcsir_score(int32_t device, const fcsir_batch* b, uint32_t* best, int32_t* off, int64_t max_pairs, int64_t* n_pairs) {
  const char* who = "fcsir_score";
  int rc;
  if ((rc = check_scalars(b, best, off, max_pairs, n_pairs, who))) return rc;
  // what the rules refuse, before any device work
  if ((rc = check_bins(who, "sequence", b->bin_seq, b->n_bins, b->n_seq))) return rc;
  if ((rc = check_bins(who, "read", b->bin_read, b->n_bins, b->n_reads))) return rc;
  if ((rc = check_offsets(who, "sequence", b->seq_off, b->n_seq, b->n_seq_bytes, FCSIR_SEQ_MAX))) return rc;
  if ((rc = check_offsets(who, "read", b->read_off, b->n_reads, b->n_read_bytes, FCSIR_READ_MAX))) return rc;
  for (int64_t s = 0; s < b->n_seq; ++s) {
    if (b->seq_off[s + 1] == b->seq_off[s]) return fail_invalid(who, "sequence " + std::to_string(s) + " is empty");
    for (int64_t k = b->seq_off[s]; k < b->seq_off[s + 1]; ++k)
      if (b->seq[k] > 4)
        return fail_invalid(who, "sequence " + std::to_string(s) + " has code " + std::to_string(b->seq[k]) + " at base " + std::to_string(k - b->seq_off[s]));
  }
  for (int64_t r = 0; r < b->n_reads; ++r) {
    if (b->read_off[r + 1] == b->read_off[r]) return fail_invalid(who, "read " + std::to_string(r) + " is empty");
    for (int64_t k = b->read_off[r]; k < b->read_off[r + 1]; ++k)
      if (b->read[k] > 4)
        return fail_invalid(who, "read " + std::to_string(r) + " has code " + std::to_string(b->read[k]) + " at base " + std::to_string(k - b->read_off[r]));
    if (b->orig[r] < 0 || b->orig[r] > FCSIR_ORIG_MAX)
      return fail_invalid(who, "read " + std::to_string(r) + " has the original offset " + std::to_string(b->orig[r]) + " (0 to " + std::to_string(FCSIR_ORIG_MAX) + ")");
  }
  int64_t pairs = 0;
  for (int64_t k = 0; k < b->n_bins; ++k) pairs += (b->bin_seq[k + 1] - b->bin_seq[k]) * (b->bin_read[k + 1] - b->bin_read[k]);
  if (pairs > max_pairs) return fail_invalid(who, "the batch has " + std::to_string(pairs) + " pairs, max_pairs is " + std::to_string(max_pairs));
  if (pairs == 0) {
    *n_pairs = 0;
    return FCS_OK;
  }
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  const size_t NB = (size_t)b->n_bins, NS = (size_t)b->n_seq, NR = (size_t)b->n_reads, NP = (size_t)pairs;
  const size_t s_lo = (size_t)b->seq_off[0], s_n = (size_t)b->seq_off[NS] - s_lo;
  const size_t r_lo = (size_t)b->read_off[0], r_n = (size_t)b->read_off[NR] - r_lo;
  Arena A;
  const size_t oseq = A.add(s_n), oseqoff = A.add(8 * (NS + 1)), obinseq = A.add(8 * (NB + 1)), oread = A.add(r_n), oqual = A.add(r_n),
               oreadoff = A.add(8 * (NR + 1)), obinread = A.add(8 * (NB + 1)), oorig = A.add(4 * NR);
  const size_t in_bytes = A.total;
  const size_t otail = A.add(16), obest = A.add(4 * NP), ooff = A.add(4 * NP);  // n_pairs, status; the outputs: one copy back
  const size_t host_bytes = A.total;
  const size_t ows = A.add(ir_workspace(b->n_bins));
  CallSession S;
  if ((rc = call_session_acquire(device, host_bytes, A.total, S))) return rc;
  CallLease lease{S};
  std::memcpy(S.host + oseq, b->seq + s_lo, s_n), std::memcpy(S.host + oseqoff, b->seq_off, 8 * (NS + 1));
  std::memcpy(S.host + obinseq, b->bin_seq, 8 * (NB + 1)), std::memcpy(S.host + obinread, b->bin_read, 8 * (NB + 1));
  std::memcpy(S.host + oread, b->read + r_lo, r_n), std::memcpy(S.host + oqual, b->qual + r_lo, r_n);
  std::memcpy(S.host + oreadoff, b->read_off, 8 * (NR + 1)), std::memcpy(S.host + oorig, b->orig, 4 * NR);
  auto dev = [&](size_t o) { return S.dev + o; };
  fcsir_batch d = *b;
  d.seq = reinterpret_cast<const uint8_t*>(dev(oseq)) - s_lo, d.seq_off = reinterpret_cast<const int64_t*>(dev(oseqoff));
  d.bin_seq = reinterpret_cast<const int64_t*>(dev(obinseq)), d.bin_read = reinterpret_cast<const int64_t*>(dev(obinread));
  d.read = reinterpret_cast<const uint8_t*>(dev(oread)) - r_lo, d.qual = reinterpret_cast<const uint8_t*>(dev(oqual)) - r_lo;
  d.read_off = reinterpret_cast<const int64_t*>(dev(oreadoff)), d.orig = reinterpret_cast<const int32_t*>(dev(oorig));
  d.n_seq_bytes = b->seq_off[NS], d.n_read_bytes = b->read_off[NR];
  FCS_HIP_CHECK(hipMemcpyAsync(S.dev, S.host, in_bytes, hipMemcpyHostToDevice, S.s));
  FCS_HIP_CHECK(hipMemsetAsync(dev(otail), 0, 16, S.s));
  if ((rc = launch_score(d, reinterpret_cast<uint32_t*>(dev(obest)), reinterpret_cast<int32_t*>(dev(ooff)), pairs,
                         reinterpret_cast<int64_t*>(dev(otail)), dev(ows), reinterpret_cast<int32_t*>(dev(otail) + 8), S.s)))
    return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S.host + otail, dev(otail), host_bytes - otail, hipMemcpyDeviceToHost, S.s));
  FCS_HIP_CHECK(hipStreamSynchronize(S.s));
  int64_t found;
  int32_t stw;
  std::memcpy(&found, S.host + otail, sizeof found);
  std::memcpy(&stw, S.host + otail + 8, sizeof stw);
  if (stw || found != pairs)
    return fail(FCS_ERR_DEVICE, "[E::fcsir_score] the device clamped a checked field (status " + std::to_string(stw) + ", " +
                                    std::to_string(found) + " pairs of " + std::to_string(pairs) + ")");
  std::memcpy(best, S.host + obest, 4 * NP), std::memcpy(off, S.host + ooff, 4 * NP);
  *n_pairs = pairs;
  return FCS_OK;
}

}  // extern "C"
