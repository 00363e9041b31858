// The chaining recurrence of minimizer seeding on the device (include/fcsmm.h;
// DESIGN §2 [EXT] "minimizer seeding and chaining", §4.16).  The rules are
// csrc/mm_rules.h (one text for this kernel, host/minimizer.cpp and
// tools/micro/mm_test.cpp).  All work of a call is queued on one stream, without
// a host round trip.
//
// mm_chain_kernel: a wave per read over a bounded grid; the lanes own
// successors, not predecessors.  Lane i % 64 holds anchor i and its running best
// (f, p).  At step j the wave reads anchor j's final (t, q, f) out of lane
// j % 64 with a wave-uniform readlane; that lane puts its (f, p) aside and takes
// anchor j + 64 with a fresh best; then every lane applies j as a candidate
// predecessor of the anchor it holds.  "Read, replace, apply" is what lets the
// lane that just took anchor j + 64 see j, 64 back; the anchors in the other
// lanes are j + 1 .. j + 63.  There is no reduction and no LDS, and a read may
// have any number of anchors.  Memory is touched once per 64 steps: the anchors
// of the next 64 steps are loaded, one per lane, before the steps of this block
// run, and the 64 results are stored after them.
// mm_chain_kernel is built for 8 waves per SIMD.
//
// Every loop is bounded by a count of reads or anchors; the kernel uses no
// scratch.
#include <algorithm>
#include <cstring>
#include <string>

#include "fcship_internal.h"
#include "fcsmm.h"
#include "mm_rules.h"
#include "rec_batch.h"

namespace fcs {

namespace {

constexpr int kMmBlock = 256;
constexpr int kMmWaves = kMmBlock / 64;
// launch cap of mm_chain_kernel's stride loop over the reads
constexpr int kMmMaxBlocks = 2048;

static_assert(FCSMM_LOOKBACK == kMmLookback && kMmLookback == 64, "the lookback is the wave");
static_assert(FCSMM_SPAN_MAX == kMmSpanMax && FCSMM_GAP_MAX == kMmGapMax && FCSMM_READ_ANCHORS == kMmReadAnchors &&
                  FCSMM_STATUS_FIELD == kMmStatusField && FCSMM_STATUS_ORDER == kMmStatusOrder,
              "fcsmm.h and mm_rules.h");
static_assert(sizeof(fcsmm_batch) == 56, "argument layout");

__device__ __forceinline__ int64_t read_lane64(int64_t v, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)((uint64_t)v >> 32), lane);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Anchor i of the n at (t, q), or (0, 0) beyond them; `sorted` goes false when it is out of order after anchor i - 1.
__device__ __forceinline__ void mm_load(const int64_t* __restrict__ t, const int32_t* __restrict__ q, int i, int n, int64_t& ti,
                                        int32_t& qi, bool& sorted) {
  ti = 0, qi = 0;
  if (i < n) {
    ti = t[i], qi = q[i];
    if (i > 0 && !mm_in_order(t[i - 1], q[i - 1], ti, qi)) sorted = false;
  }
}

__global__ __launch_bounds__(kMmBlock) void mm_chain_kernel(fcsmm_batch b, int32_t* __restrict__ f, int32_t* __restrict__ p,
                                                            int32_t* __restrict__ status) {
  const int lane = (int)threadIdx.x % 64;
  const int64_t wave = (int64_t)blockIdx.x * kMmWaves + (int)threadIdx.x / 64, n_waves = (int64_t)gridDim.x * kMmWaves;
  const MmParams P{b.max_gap, b.bw, b.span};
  for (int64_t r = wave; r < b.n_reads; r += n_waves) {
    const int64_t a0 = b.read_off[r], a1 = b.read_off[r + 1];
    if (a0 < 0 || a1 < a0 || a1 > b.n_anchors || a1 - a0 > kMmReadAnchors) {  // the same in the whole wave: the read is skipped
      if (lane == 0) atomicOr(status, kMmStatusField);
      continue;
    }
    const int n = (int)(a1 - a0);
    const int64_t* __restrict__ T = b.t + a0;
    const int32_t* __restrict__ Q = b.q + a0;
    bool sorted = true;
    int64_t ti, tn;
    int32_t qi, qn;
    mm_load(T, Q, lane, n, ti, qi, sorted);
    int32_t best = P.span, from = -1;
    for (int base = 0; base < n; base += 64) {
      mm_load(T, Q, base + 64 + lane, n, tn, qn, sorted);  // used from this block's step `lane` on
      const int steps = n - base < 64 ? n - base : 64;
      int32_t f_out = 0, p_out = 0;
      for (int s = 0; s < steps; ++s) {  // s is the same in the whole wave
        const int64_t tj = read_lane64(ti, s);
        const int32_t qj = read_lane(qi, s), fj = read_lane(best, s);
        if (lane == s) f_out = best, p_out = from, ti = tn, qi = qn, best = P.span, from = -1;
        int32_t sc;
        if (mm_candidate(ti, qi, tj, qj, fj, P, sc)) mm_take(sc, base + s, P.span, best, from);
      }
      if (base + lane < n) f[a0 + base + lane] = f_out, p[a0 + base + lane] = p_out;
    }
    if (!sorted) atomicOr(status, kMmStatusOrder);
  }
}

// Device pointers in b; n_reads > 0.
int launch_chain(const fcsmm_batch& b, int32_t* f, int32_t* p, int32_t* status, hipStream_t s) {
  const int grid = (int)std::clamp<int64_t>((b.n_reads + kMmWaves - 1) / kMmWaves, 1, kMmMaxBlocks);
  hipLaunchKernelGGL(mm_chain_kernel, dim3(grid), dim3(kMmBlock), 0, s, b, f, p, status);
  FCS_HIP_CHECK(hipGetLastError());
  return FCS_OK;
}

int check_scalars(const fcsmm_batch* b, const void* f, const void* p, const char* who) {
  if (!b) return fail_invalid(who, "null batch");
  if (b->n_reads < 0 || b->n_anchors < 0)
    return fail_invalid(who, "negative count: " + std::to_string(b->n_reads) + " reads, " + std::to_string(b->n_anchors) + " anchors");
  if (b->n_reads > INT32_MAX || b->n_anchors > INT32_MAX) return fail_invalid(who, "a count above 2^31 - 1");
  if (b->max_gap < 0 || b->max_gap > FCSMM_GAP_MAX) return fail_invalid(who, "max_gap " + std::to_string(b->max_gap) + " (0 to " + std::to_string(FCSMM_GAP_MAX) + ")");
  if (b->bw < 0 || b->bw > FCSMM_GAP_MAX) return fail_invalid(who, "bw " + std::to_string(b->bw) + " (0 to " + std::to_string(FCSMM_GAP_MAX) + ")");
  if (b->span < 1 || b->span > FCSMM_SPAN_MAX) return fail_invalid(who, "span " + std::to_string(b->span) + " (1 to " + std::to_string(FCSMM_SPAN_MAX) + ")");
  if (b->reserved != 0) return fail_invalid(who, "the reserved field is not zero");
  if (!b->read_off) return fail_invalid(who, "null read offsets");
  if (b->n_anchors > 0 && (!b->t || !b->q)) return fail_invalid(who, "null anchor arrays");
  if (b->n_anchors > 0 && (!f || !p)) return fail_invalid(who, "null output arrays");
  return FCS_OK;
}

}  // namespace

}  // namespace fcs

using namespace fcs;

extern "C" {

int64_t fcsmm_workspace_bytes(int64_t n_reads, int64_t n_anchors) {
  if (n_reads < 0 || n_reads > INT32_MAX || n_anchors < 0 || n_anchors > INT32_MAX)
    return fail_invalid("fcsmm_workspace_bytes", std::to_string(n_reads) + " reads, " + std::to_string(n_anchors) + " anchors");
  return 0;  // a wave keeps a read's state in its registers
}

int fcsmm_chain_dev(int32_t device, const fcsmm_batch* batch, int32_t* dev_f, int32_t* dev_p, void* dev_workspace,
                    int64_t workspace_bytes, int32_t* dev_status, void* stream) {
  const char* who = "fcsmm_chain_dev";
  int rc;
  if ((rc = check_scalars(batch, dev_f, dev_p, who))) return rc;
  if (!dev_status) return fail_invalid(who, "null status");
  if (workspace_bytes < 0) return fail_invalid(who, "the workspace holds " + std::to_string(workspace_bytes) + " bytes");
  (void)dev_workspace;
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  if (batch->n_reads == 0) return FCS_OK;
  return launch_chain(*batch, dev_f, dev_p, dev_status, static_cast<hipStream_t>(stream));
}

int fcsmm_chain(int32_t device, const fcsmm_batch* b, int32_t* f, int32_t* p) {
  const char* who = "fcsmm_chain";
  int rc;
  if ((rc = check_scalars(b, f, p, who))) return rc;
  // what the rules refuse, before any device work
  if ((rc = check_offsets(who, "anchor", b->read_off, b->n_reads, b->n_anchors, FCSMM_READ_ANCHORS))) return rc;
  for (int64_t r = 0; r < b->n_reads; ++r)
    for (int64_t i = b->read_off[r]; i < b->read_off[r + 1]; ++i) {
      if (b->t[i] < 0 || b->q[i] < 0) return fail_invalid(who, "read " + std::to_string(r) + " has a negative t or q at anchor " + std::to_string(i - b->read_off[r]));
      if (i > b->read_off[r] && !mm_in_order(b->t[i - 1], b->q[i - 1], b->t[i], b->q[i]))
        return fail_invalid(who, "read " + std::to_string(r) + " is not sorted by (t, q) at anchor " + std::to_string(i - b->read_off[r]));
    }
  if (b->n_reads == 0) return FCS_OK;
  const size_t NR = (size_t)b->n_reads;
  const size_t lo = (size_t)b->read_off[0], n = (size_t)b->read_off[NR] - lo;  // the anchors the reads hold
  if (n == 0) return FCS_OK;
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  Arena A;
  const size_t ot = A.add(8 * n), oq = A.add(4 * n), ooff = A.add(8 * (NR + 1));
  const size_t in_bytes = A.total;
  const size_t otail = A.add(4), of = A.add(4 * n), op = A.add(4 * n);  // status; the outputs: one copy back
  CallSession S;
  if ((rc = call_session_acquire(device, A.total, A.total, S))) return rc;
  CallLease lease{S};
  std::memcpy(S.host + ot, b->t + lo, 8 * n), std::memcpy(S.host + oq, b->q + lo, 4 * n);
  int64_t* off = reinterpret_cast<int64_t*>(S.host + ooff);
  for (size_t r = 0; r <= NR; ++r) off[r] = b->read_off[r] - (int64_t)lo;
  fcsmm_batch d = *b;
  d.t = reinterpret_cast<const int64_t*>(S.dev + ot), d.q = reinterpret_cast<const int32_t*>(S.dev + oq);
  d.read_off = reinterpret_cast<const int64_t*>(S.dev + ooff), d.n_anchors = (int64_t)n;
  FCS_HIP_CHECK(hipMemcpyAsync(S.dev, S.host, in_bytes, hipMemcpyHostToDevice, S.s));
  FCS_HIP_CHECK(hipMemsetAsync(S.dev + otail, 0, 4, S.s));
  if ((rc = launch_chain(d, reinterpret_cast<int32_t*>(S.dev + of), reinterpret_cast<int32_t*>(S.dev + op),
                         reinterpret_cast<int32_t*>(S.dev + otail), S.s)))
    return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S.host + otail, S.dev + otail, A.total - otail, hipMemcpyDeviceToHost, S.s));
  FCS_HIP_CHECK(hipStreamSynchronize(S.s));
  int32_t stw;
  std::memcpy(&stw, S.host + otail, sizeof stw);
  if (stw) return fail(FCS_ERR_DEVICE, "[E::fcsmm_chain] the device met a checked field again (status " + std::to_string(stw) + ")");
  std::memcpy(f + lo, S.host + of, 4 * n), std::memcpy(p + lo, S.host + op, 4 * n);
  return FCS_OK;
}

}  // extern "C"
