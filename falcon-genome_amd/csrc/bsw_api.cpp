// Banded Smith-Waterman calls of the C-ABI (include/fcship.h): extension,
// global alignment with CIGARs and local alignment, over host tasks, host
// batches and device batches, and bwa's single-task signature twins.
#include <rocprim/device/device_radix_sort.hpp>

#include <cstring>
#include <map>
#include <memory>

#include "session.h"

struct fcs_bsw_plan {
  int device = 0;
  fcs::BswWorkspace ws;
};

namespace fcs {

// Stable LSD radix sort of (32-bit key, index) pairs.  rocPRIM's default picks
// a block sort + ~20 merge passes for n <= 2^20 (the C2 / C3 batch sizes:
// 0.16 ms of 7 us launches); a merge-sort limit of 0 forces its onesweep path
// (histogram + one pass per 8-bit digit) at every size.  Same order either way.
// The onesweep kernels' default tile (1024 threads x ~16 items) gives a 1M-key
// sort 62 workgroups on a 256-CU chip; 256 x 8 tiles give it ~490 but measured
// slower (C2 2.86 vs 2.93 TCUPS, C3 1.95 vs 2.05, profiles/r2/abt_*).
#ifndef FCS_SORT_BITS
#define FCS_SORT_BITS 0  // 0: rocPRIM's default onesweep config for the target
#endif
#ifndef FCS_SORT_BLOCK
#define FCS_SORT_BLOCK 1024
#endif
#ifndef FCS_SORT_ITEMS
#define FCS_SORT_ITEMS 8
#endif
#if FCS_SORT_BITS
using OnesweepConfig = rocprim::radix_sort_onesweep_config<rocprim::kernel_config<256, 12>,
                                                           rocprim::kernel_config<FCS_SORT_BLOCK, FCS_SORT_ITEMS>,
                                                           FCS_SORT_BITS, rocprim::block_radix_rank_algorithm::match>;
using SortConfig = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, OnesweepConfig, 0>;
#else
using SortConfig = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 0>;
#endif
hipError_t sort_pairs_u32(void* tmp, size_t& bytes, const uint32_t* kin, uint32_t* kout, const int32_t* vin,
                          int32_t* vout, int n, hipStream_t s, int end_bit) {
  return rocprim::radix_sort_pairs<SortConfig>(tmp, bytes, kin, kout, vin, vout, (size_t)n, 0, (unsigned)end_bit, s);
}

void ws_free(BswWorkspace& ws) {
  void* bufs[6] = {ws.keys_in, ws.keys_out, ws.idx_in, ws.idx_out, ws.bounds, ws.tmp};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  ws = BswWorkspace();
}

namespace {

BswParams to_params(const fcs_bsw_params* p) {
  BswParams q{{}, p->o_del, p->e_del, p->o_ins, p->e_ins, p->end_bonus, p->zdrop};
  std::memcpy(q.mat, p->mat, 25);
  int mx = 0;
  for (int i = 0; i < 25; ++i) mx = std::max<int>(mx, p->mat[i]);
  q.max_mat = mx;
  q.lane_ok = 1;
  for (int t = 0; t < 5; ++t) {
    uint32_t pk = 0;
    for (int c = 0; c < 5; ++c) {
      const int v = p->mat[t * 5 + c];
      if (v < -16 || v > 15) q.lane_ok = 0;
      pk |= ((uint32_t)v & 31u) << (5 * c);
    }
    q.matpack[t] = (int32_t)pk;
  }
  int mn4 = 0, mx4 = 0;
  for (int t = 0; t < 5; ++t)  // target rows A..N, query columns A..T (the pair kernel's tables)
    for (int c = 0; c < 4; ++c) mn4 = std::min<int>(mn4, p->mat[t * 5 + c]), mx4 = std::max<int>(mx4, p->mat[t * 5 + c]);
  q.pair_bias = -mn4;
  q.pair_cg = mx4 + q.pair_bias + 1;
  // the pair kernel's 16-bit z-drop arithmetic: |row distance| * e stays below 2^15
  q.pair_ok = (q.pair_cg <= 128 && p->e_del <= 16 && p->e_ins <= 16) ? 1 : 0;
  q.pair_k256 = 0x01000100;
  q.pair_one = 0x00010001;
  return q;
}

// Workspace for one SW schedule of up to cap tasks (plain hipMalloc: the
// library never uses the stream-ordered pool, see stream_workspace).
int ws_alloc(BswWorkspace& ws, int64_t cap) {
  ws.cap = cap;
  const size_t n = (size_t)std::max<int64_t>(cap, 1);
  size_t tmp = 0;
  FCS_HIP_CHECK(sort_pairs_u32(nullptr, tmp, nullptr, nullptr, nullptr, nullptr, (int)n, nullptr));
  ws.tmp_bytes = std::max<size_t>(tmp, 16);
  void** bufs[6] = {(void**)&ws.keys_in, (void**)&ws.keys_out, (void**)&ws.idx_in, (void**)&ws.idx_out,
                    (void**)&ws.bounds, &ws.tmp};
  const size_t sz[6] = {4 * n, 4 * n, 4 * n, 4 * n, (kBswWideBucket + 2) * sizeof(int64_t), ws.tmp_bytes};
  for (int i = 0; i < 6; ++i) FCS_HIP_CHECK(hipMalloc(bufs[i], sz[i]));
  return FCS_OK;
}

// The SW workspace of a caller's launch stream (fcs_bsw_extend_dev), kept per
// (device, stream) like the fork sets and grown with plain hipMalloc.  Round 5
// took it from the stream-ordered pool (hipMallocAsync / hipFreeAsync), as
// fcs_bgzf_inflate once took its scratch: on this runtime that pool hands
// memory still in use on one stream to an allocation on another.
// tools/micro/pin_reuse.hip (profiles/r6/r6b_pin_reuse.log) finds overlapping
// live allocations with 16 threads x 16 streams in every configuration tried
// (default attributes, the stream synchronised before each free, reuse
// attributes off, every pool call under one mutex) and from one thread over 16
// streams; hipMalloc / hipFree and pageable copies never.  That is the cause of
// the round-5 inflate corruption (member 0 of a call: the start of its input
// scratch, overwritten by another call).  The caller uses a stream for one call
// at a time, so one workspace per stream is enough.
std::map<std::pair<int, hipStream_t>, BswWorkspace>* g_stream_ws = new std::map<std::pair<int, hipStream_t>, BswWorkspace>();

int stream_workspace(int device, hipStream_t s, int64_t n, BswWorkspace** out) {
  std::lock_guard<std::mutex> lk(g_fork_mu);
  BswWorkspace& ws = (*g_stream_ws)[{device, s}];
  if (ws.cap < n || !ws.keys_in) {
    if (ws.keys_in) {
      FCS_HIP_CHECK(hipStreamSynchronize(s));  // the stream's last call may still read the old one
      ws_free(ws);
    }
    const int rc = ws_alloc(ws, std::max<int64_t>(n + n / 4, 4096));
    if (rc) {
      ws_free(ws);
      return rc;
    }
  }
  *out = &ws;
  return FCS_OK;
}

int check_params(const fcs_bsw_params* p) {
  if (!p) return fail(FCS_ERR_INVALID, "[E::fcship] null SW params");
  if (p->e_del <= 0 || p->e_ins <= 0 || p->o_del < 0 || p->o_ins < 0)
    return fail(FCS_ERR_INVALID, "[E::fcship] gap penalties must satisfy o >= 0, e > 0");
  return FCS_OK;
}

BswDevBatch bsw_dev(const fcs_bsw_batch* b) {
  return BswDevBatch{b->qbuf, b->qoff, b->qlen, b->tbuf, b->toff, b->tlen, b->h0, b->w, b->n};
}

int check_bsw_batch(const fcs_bsw_batch* b) {
  if (!b || b->n < 0) return fail(FCS_ERR_INVALID, "[E::fcship] bad SW batch");
  // byte buffers may be null when empty: a batch whose every target (or query)
  // is empty, e.g. left extensions of seeds that start at their window's edge
  // (bwa calls ksw_extend2 with tlen 0 there)
  if (b->n > 0 && ((!b->qbuf && b->qbytes > 0) || !b->qoff || !b->qlen || (!b->tbuf && b->tbytes > 0) || !b->toff ||
                   !b->tlen || !b->h0 || !b->w))
    return fail(FCS_ERR_INVALID, "[E::fcship] null pointer in SW batch");
  return FCS_OK;
}

// `what` is "query" or "target".
int check_codes(const char* who, const uint8_t* buf, int64_t n, const char* what) {
  for (int64_t i = 0; i < n; ++i)
    if (buf[i] > 4) return fail_invalid(who, std::string(what) + " base code > 4");
  return FCS_OK;
}

// Where a host batch's task arrays lie in a session's arenas: the start of
// every call's contiguous inputs, so a call adds its own inputs after them,
// marks in_bytes, then adds its outputs.  Local alignment has no h0 / w.
struct BswLayout {
  size_t q, qoff, qlen, t, toff, tlen, h0, w;
  bool with_band;
};

BswLayout layout_tasks(const fcs_bsw_batch& b, bool with_band, Arena& a) {
  const size_t n = (size_t)b.n;
  BswLayout l{};
  l.with_band = with_band;
  l.q = a.add((size_t)b.qbytes), l.qoff = a.add(8 * n), l.qlen = a.add(4 * n);
  l.t = a.add((size_t)b.tbytes), l.toff = a.add(8 * n), l.tlen = a.add(4 * n);
  if (with_band) l.h0 = a.add(4 * n), l.w = a.add(4 * n);
  return l;
}

// Copies the task arrays into the host arena and answers the device view.
BswDevBatch stage_tasks(const fcs_bsw_batch& b, const BswLayout& l, char* host, char* dev) {
  const size_t n = (size_t)b.n;
  if (b.qbytes) std::memcpy(host + l.q, b.qbuf, (size_t)b.qbytes);
  std::memcpy(host + l.qoff, b.qoff, 8 * n);
  std::memcpy(host + l.qlen, b.qlen, 4 * n);
  if (b.tbytes) std::memcpy(host + l.t, b.tbuf, (size_t)b.tbytes);
  std::memcpy(host + l.toff, b.toff, 8 * n);
  std::memcpy(host + l.tlen, b.tlen, 4 * n);
  if (l.with_band) {
    std::memcpy(host + l.h0, b.h0, 4 * n);
    std::memcpy(host + l.w, b.w, 4 * n);
  }
  auto i32 = [&](size_t off) { return reinterpret_cast<const int32_t*>(dev + off); };
  auto i64 = [&](size_t off) { return reinterpret_cast<const int64_t*>(dev + off); };
  return BswDevBatch{reinterpret_cast<const uint8_t*>(dev + l.q), i64(l.qoff), i32(l.qlen),
                     reinterpret_cast<const uint8_t*>(dev + l.t), i64(l.toff), i32(l.tlen),
                     l.with_band ? i32(l.h0) : nullptr,           l.with_band ? i32(l.w) : nullptr, b.n};
}

// Packs AoS tasks into an SoA host batch.
struct PackedTasks {
  std::vector<uint8_t> q, t;
  std::vector<int64_t> qoff, toff;
  std::vector<int32_t> qlen, tlen, h0, w;
  fcs_bsw_batch b{};
};

int pack_tasks(const fcs_bsw_task* tasks, int32_t n, PackedTasks& pk) {
  pk.qoff.resize(n), pk.toff.resize(n);
  for (auto* v : {&pk.qlen, &pk.tlen, &pk.h0, &pk.w}) v->resize(n);
  for (int32_t k = 0; k < n; ++k) {
    const fcs_bsw_task& t = tasks[k];
    if (t.qlen < 0 || t.tlen < 0 || (t.qlen > 0 && !t.query) || (t.tlen > 0 && !t.target))
      return fail(FCS_ERR_INVALID, "[E::fcship] malformed SW task");
    pk.qoff[k] = (int64_t)pk.q.size();
    pk.toff[k] = (int64_t)pk.t.size();
    pk.q.insert(pk.q.end(), t.query, t.query + t.qlen);
    pk.t.insert(pk.t.end(), t.target, t.target + t.tlen);
    pk.qlen[k] = t.qlen;
    pk.tlen[k] = t.tlen;
    pk.h0[k] = t.h0;
    pk.w[k] = t.w;
  }
  pk.b = fcs_bsw_batch{pk.q.data(),    pk.qoff.data(), pk.qlen.data(), pk.t.data(),          pk.toff.data(),
                       pk.tlen.data(), pk.h0.data(),   pk.w.data(),    n,                    (int64_t)pk.q.size(),
                       (int64_t)pk.t.size()};  // max_qlen / max_tlen stay 0: the host calls take their own
  return FCS_OK;
}

// The parameters of a bwa signature twin, or false with the error set.
bool ksw_params(const char* who, int m, const int8_t* mat, int o_del, int e_del, int o_ins, int e_ins, int end_bonus,
                int zdrop, fcs_bsw_params& p) {
  if (m != 5)
    return (void)fail(FCS_ERR_UNSUPPORTED, std::string("[E::") + who + "] only m == 5 (bwa's alphabet) is supported"), false;
  if (!mat) return (void)fail_invalid(who, "null matrix"), false;
  p = fcs_bsw_params{{}, o_del, e_del, o_ins, e_ins, end_bonus, zdrop};
  std::memcpy(p.mat, mat, 25);
  return true;
}

}  // namespace

BswWorkspace bsw_take_stream(int device, hipStream_t s) {
  BswWorkspace ws;
  auto wi = g_stream_ws->find({device, s});
  if (wi != g_stream_ws->end()) {
    ws = wi->second;
    g_stream_ws->erase(wi);
  }
  return ws;
}

void bsw_drop_device(int device) {
  for (auto it = g_stream_ws->begin(); it != g_stream_ws->end();)
    it = it->first.first == device ? g_stream_ws->erase(it) : std::next(it);
}

int Session::ensure_bsw(int64_t tasks) {
  if (bsw && bsw->ws.cap >= tasks) return FCS_OK;
  FCS_HIP_CHECK(hipStreamSynchronize(s));
  fcs_bsw_plan_destroy(bsw);
  bsw = nullptr;
  return fcs_bsw_plan_create(device, (int64_t)grown((size_t)tasks, 0), &bsw);
}

}  // namespace fcs

using namespace fcs;

extern "C" {

void fcs_bsw_params_default(fcs_bsw_params* p) {
  if (!p) return;
  // bwa_fill_scmat(a=1, b=4, -1): match a, mismatch -b, anything with N -1.
  for (int i = 0, k = 0; i < 4; ++i) {
    for (int j = 0; j < 4; ++j) p->mat[k++] = (int8_t)(i == j ? 1 : -4);
    p->mat[k++] = -1;
  }
  for (int j = 0; j < 5; ++j) p->mat[20 + j] = -1;
  p->o_del = p->o_ins = 6, p->e_del = p->e_ins = 1, p->end_bonus = 5, p->zdrop = 100;
}

int fcs_bsw_extend_dev(const fcs_bsw_batch* b, const fcs_bsw_params* params, int32_t* res, int64_t* cells,
                       int32_t device, void* stream) {
  int rc = check_bsw_batch(b);
  if (rc) return rc;
  if ((rc = check_params(params))) return rc;
  if (b->n > 0 && !res) return fail(FCS_ERR_INVALID, "[E::fcs_bsw_extend_dev] null result buffer");
  if ((rc = check_device(device))) return rc;
  if (b->n == 0) return FCS_OK;
  FCS_SET_DEVICE((device));
  hipStream_t s = (hipStream_t)stream;
  BswWorkspace* ws = nullptr;
  if ((rc = stream_workspace(device, s, b->n, &ws))) return rc;
  return launch_bsw_extend_sorted(bsw_dev(b), to_params(params), std::max(b->max_qlen, 0), std::max(b->max_tlen, 0),
                                  res, cells, *ws, s);
}

int fcs_bsw_plan_create(int32_t device, int64_t max_tasks, fcs_bsw_plan** plan) {
  if (!plan || max_tasks < 0) return fail(FCS_ERR_INVALID, "[E::fcs_bsw_plan_create] bad arguments");
  int rc = check_device(device);
  if (rc) return rc;
  FCS_SET_DEVICE((device));
  std::unique_ptr<fcs_bsw_plan> p(new fcs_bsw_plan());
  p->device = device;
  if ((rc = ws_alloc(p->ws, max_tasks))) {
    ws_free(p->ws);
    return rc;
  }
  *plan = p.release();
  return FCS_OK;
}

int fcs_bsw_plan_destroy(fcs_bsw_plan* plan) {
  if (!plan) return FCS_OK;
  ::fcs::DeviceScope dev_scope;
  (void)hipSetDevice(plan->device);
  ws_free(plan->ws);
  delete plan;
  return FCS_OK;
}

int fcs_bsw_extend_plan(fcs_bsw_plan* plan, const fcs_bsw_batch* b, const fcs_bsw_params* params, int32_t* res,
                        int64_t* cells, void* stream) {
  if (!plan) return fail(FCS_ERR_INVALID, "[E::fcs_bsw_extend_plan] null plan");
  int rc = check_bsw_batch(b);
  if (rc) return rc;
  if ((rc = check_params(params))) return rc;
  if (b->n > plan->ws.cap) return fail(FCS_ERR_INVALID, "[E::fcs_bsw_extend_plan] batch exceeds plan");
  if (b->n > 0 && !res) return fail(FCS_ERR_INVALID, "[E::fcs_bsw_extend_plan] null result buffer");
  if (b->n == 0) return FCS_OK;
  FCS_SET_DEVICE((plan->device));
  return launch_bsw_extend_sorted(bsw_dev(b), to_params(params), std::max(b->max_qlen, 0), std::max(b->max_tlen, 0),
                                  res, cells, plan->ws, (hipStream_t)stream);
}

int fcs_bsw_extend_batch(const fcs_bsw_batch* b, const fcs_bsw_params* params, int32_t* res, int64_t* cells,
                         int32_t device) {
  static const char* who = "fcs_bsw_extend_batch";
  int rc = check_bsw_batch(b);
  if (rc) return rc;
  if ((rc = check_params(params))) return rc;
  if (b->n == 0) return FCS_OK;
  if (!res) return fail_invalid(who, "null result buffer");
  int32_t mq = 0, mt = 0;
  for (int64_t k = 0; k < b->n; ++k) {
    if (b->qlen[k] < 0 || b->tlen[k] < 0 || b->qoff[k] < 0 || b->toff[k] < 0 ||
        b->qoff[k] + b->qlen[k] > b->qbytes || b->toff[k] + b->tlen[k] > b->tbytes)
      return fail_invalid(who, "task extent outside buffers");
    if (b->h0[k] <= 0) return fail_invalid(who, "h0 must be > 0 (ksw_extend2 assert)");
    if (b->w[k] < 0) return fail_invalid(who, "negative band");
    mq = std::max(mq, b->qlen[k]);
    mt = std::max(mt, b->tlen[k]);
  }
  if ((rc = check_codes(who, b->qbuf, b->qbytes, "query")) || (rc = check_codes(who, b->tbuf, b->tbytes, "target")))
    return rc;
  if ((rc = check_device(device))) return rc;
  FCS_SET_DEVICE((device));
  SessionLease lease;
  if ((rc = lease.acquire(device))) return rc;
  Session* S = lease.get();
  const size_t n = (size_t)b->n;
  Arena L;
  const BswLayout T = layout_tasks(*b, true, L);
  const size_t in_bytes = L.total, ors = L.add(24 * n), ocl = L.add(8 * n);
  // pinned: the staged inputs, then results and cells at their device offsets
  if ((rc = S->ensure_host(L.total)) || (rc = S->ensure_dev(L.total)) || (rc = S->ensure_bsw(b->n))) return rc;
  const BswDevBatch d = stage_tasks(*b, T, S->hbase(), S->dbase());
  hipStream_t s = S->s;
  const StreamDrain drain{s};
  FCS_HIP_CHECK(hipMemcpyAsync(S->dev, S->host, in_bytes, hipMemcpyHostToDevice, s));
  if ((rc = launch_bsw_extend_sorted(d, to_params(params), mq, mt, S->d<int32_t>(ors), S->d<int64_t>(ocl),
                                     S->bsw->ws, s)))
    return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S->h<void>(ors), S->d<void>(ors), ocl + 8 * n - ors, hipMemcpyDeviceToHost, s));
  FCS_HIP_CHECK(hipStreamSynchronize(s));
  std::memcpy(res, S->h<void>(ors), 24 * n);
  if (cells) std::memcpy(cells, S->h<void>(ocl), 8 * n);
  return FCS_OK;
}

int fcs_bsw_extend_multi(const fcs_bsw_task* tasks, int32_t n, const fcs_bsw_params* params,
                         fcs_bsw_result* results, const int32_t* devices, int32_t n_devices) {
  if (n < 0 || (n > 0 && (!tasks || !results)) || n_devices <= 0 || !devices)
    return fail(FCS_ERR_INVALID, "[E::fcs_bsw_extend_multi] bad arguments");
  // slices of about equal qlen * tlen
  std::vector<double> cum((size_t)n);
  double run = 0;
  for (int32_t i = 0; i < n; ++i) cum[i] = (run += (double)std::max(tasks[i].qlen, 0) * std::max(tasks[i].tlen, 0));
  std::vector<int64_t> cuts((size_t)n_devices + 1);
  balanced_cuts(cum, n, n_devices, cuts.data());
  return run_slices(cuts, [&](int32_t k) {
    return fcs_bsw_extend(tasks + cuts[k], (int32_t)(cuts[k + 1] - cuts[k]), params, results + cuts[k], devices[k]);
  });
}

int fcs_bsw_extend(const fcs_bsw_task* tasks, int32_t n, const fcs_bsw_params* params, fcs_bsw_result* results,
                   int32_t device) {
  if (n < 0 || (n > 0 && (!tasks || !results))) return fail(FCS_ERR_INVALID, "[E::fcs_bsw_extend] bad arguments");
  if (n == 0) return FCS_OK;
  PackedTasks pk;
  int rc = pack_tasks(tasks, n, pk);
  if (rc) return rc;
  static_assert(sizeof(fcs_bsw_result) == 24, "result layout");
  return fcs_bsw_extend_batch(&pk.b, params, reinterpret_cast<int32_t*>(results), nullptr, device);
}

int fcs_bsw_global(const fcs_bsw_task* tasks, int32_t n, const fcs_bsw_params* params, int32_t* scores,
                   uint32_t* cigar_arena, const int64_t* cigar_off, const int32_t* cigar_cap, int32_t* n_cigar,
                   int32_t device) {
  static const char* who = "fcs_bsw_global";
  if (n < 0 || (n > 0 && (!tasks || !scores))) return fail_invalid(who, "bad arguments");
  const bool want_cigar = cigar_arena != nullptr;
  if (want_cigar && (!cigar_off || !cigar_cap || !n_cigar))
    return fail_invalid(who, "CIGAR arena needs offsets, caps and counts");
  int rc = check_params(params);
  if (rc) return rc;
  if (n == 0) return FCS_OK;
  PackedTasks pk;
  if ((rc = pack_tasks(tasks, n, pk))) return rc;
  int32_t mq = 0, mt = 0;
  std::vector<int64_t> zoff(n);
  int64_t zt = 0, ct = 0;
  for (int32_t k = 0; k < n; ++k) {
    if (pk.w[k] < 0) return fail_invalid(who, "negative band");
    mq = std::max(mq, pk.qlen[k]);
    mt = std::max(mt, pk.tlen[k]);
    const int64_t ncol = std::min<int64_t>(pk.qlen[k], 2LL * pk.w[k] + 1);
    zoff[k] = zt;
    if (want_cigar) {
      zt += ncol * pk.tlen[k];
      if (cigar_cap[k] < 0 || cigar_off[k] < 0) return fail_invalid(who, "bad CIGAR extent");
      ct = std::max<int64_t>(ct, cigar_off[k] + cigar_cap[k]);
    }
  }
  if ((rc = check_codes(who, pk.q.data(), pk.b.qbytes, "query")) || (rc = check_codes(who, pk.t.data(), pk.b.tbytes, "target")))
    return rc;
  if ((rc = check_device(device))) return rc;
  FCS_SET_DEVICE((device));
  SessionLease lease;
  if ((rc = lease.acquire(device))) return rc;
  Session* S = lease.get();
  const size_t nn = (size_t)n;
  // The direction matrix (and its offsets) only when CIGARs are wanted: a
  // scores-only batch needs none of it.
  Arena L;
  const BswLayout T = layout_tasks(pk.b, true, L);
  const size_t ozo = want_cigar ? L.add(8 * nn) : 0, oco = want_cigar ? L.add(8 * nn) : 0,
               occ = want_cigar ? L.add(4 * nn) : 0;
  const size_t in_bytes = L.total, osc = L.add(4 * nn), onc = L.add(4 * nn), ocg = L.add(4 * (size_t)ct),
               ozb = want_cigar ? L.add((size_t)zt) : 0;
  // pinned: the staged inputs, then at in_bytes (not at their device offsets: the direction matrix stays on the
  // device) scores | counts | CIGAR arena, two padded n-word arrays (<= 8n + 510) and 4 ct bytes
  if ((rc = S->ensure_host(in_bytes + 8 * nn + 4 * (size_t)ct + 1024)) || (rc = S->ensure_dev(L.total))) return rc;
  const BswDevBatch d = stage_tasks(pk.b, T, S->hbase(), S->dbase());
  if (want_cigar) {
    std::memcpy(S->h<void>(ozo), zoff.data(), 8 * nn);
    std::memcpy(S->h<void>(oco), cigar_off, 8 * nn);
    std::memcpy(S->h<void>(occ), cigar_cap, 4 * nn);
  }
  hipStream_t s = S->s;
  const StreamDrain drain{s};
  FCS_HIP_CHECK(hipMemcpyAsync(S->dev, S->host, in_bytes, hipMemcpyHostToDevice, s));
  rc = launch_bsw_global(d, to_params(params), mq, mt, S->d<int32_t>(osc), want_cigar ? S->d<uint8_t>(ozb) : nullptr,
                         zt, want_cigar ? S->d<int64_t>(ozo) : nullptr, want_cigar ? S->d<uint32_t>(ocg) : nullptr,
                         want_cigar ? S->d<int64_t>(oco) : nullptr, want_cigar ? S->d<int32_t>(occ) : nullptr,
                         want_cigar ? S->d<int32_t>(onc) : nullptr, s);
  if (rc) return rc;
  // scores, counts and the CIGAR arena are contiguous in the layout
  const size_t back = want_cigar ? ocg + 4 * (size_t)ct - osc : 4 * nn;
  FCS_HIP_CHECK(hipMemcpyAsync(S->h<void>(in_bytes), S->d<void>(osc), back, hipMemcpyDeviceToHost, s));
  FCS_HIP_CHECK(hipStreamSynchronize(s));
  const char* hb = S->h<char>(in_bytes);
  std::memcpy(scores, hb, 4 * nn);
  if (want_cigar) {
    std::memcpy(n_cigar, hb + (onc - osc), 4 * nn);
    if (ct) std::memcpy(cigar_arena, hb + (ocg - osc), 4 * (size_t)ct);
    for (int32_t k = 0; k < n; ++k)
      if (n_cigar[k] > cigar_cap[k]) return fail_invalid(who, "CIGAR longer than its arena slot");
  }
  return FCS_OK;
}

int fcs_bsw_global_dev(const fcs_bsw_batch* b, const fcs_bsw_params* params, int32_t* dev_scores, uint8_t* dev_zbuf,
                       int64_t zbytes, const int64_t* dev_zoff, uint32_t* dev_cigar, const int64_t* dev_cigar_off,
                       const int32_t* dev_cigar_cap, int32_t* dev_n_cigar, int32_t device, void* stream) {
  if (!b || b->n < 0 || (b->n > 0 && !dev_scores)) return fail(FCS_ERR_INVALID, "[E::fcs_bsw_global_dev] bad arguments");
  const bool want_cigar = dev_cigar != nullptr;
  if (want_cigar && (!dev_zbuf || !dev_zoff || !dev_cigar_off || !dev_cigar_cap || !dev_n_cigar))
    return fail(FCS_ERR_INVALID, "[E::fcs_bsw_global_dev] CIGARs need the direction matrix, offsets, caps and counts");
  int rc = check_params(params);
  if (rc) return rc;
  if (b->n == 0) return FCS_OK;
  if (b->n > 0x7FFFFFFF) return fail(FCS_ERR_UNSUPPORTED, "[E::fcs_bsw_global_dev] more than 2^31-1 tasks");
  if ((rc = check_device(device))) return rc;
  FCS_SET_DEVICE((device));
  return launch_bsw_global(bsw_dev(b), to_params(params), std::max(b->max_qlen, 1), std::max(b->max_tlen, 1),
                           dev_scores, want_cigar ? dev_zbuf : nullptr, want_cigar ? zbytes : 0,
                           want_cigar ? dev_zoff : nullptr, dev_cigar, want_cigar ? dev_cigar_off : nullptr,
                           want_cigar ? dev_cigar_cap : nullptr, want_cigar ? dev_n_cigar : nullptr,
                           (hipStream_t)stream);
}

int fcs_bsw_align(const fcs_bsw_task* tasks, int32_t n, const fcs_bsw_params* params, const int32_t* xtra,
                  fcs_kswr* out, int32_t device) {
  static const char* who = "fcs_bsw_align";
  if (n < 0 || (n > 0 && (!tasks || !xtra || !out))) return fail_invalid(who, "bad arguments");
  int rc = check_params(params);
  if (rc) return rc;
  if (n == 0) return FCS_OK;
  PackedTasks pk;
  if ((rc = pack_tasks(tasks, n, pk))) return rc;
  int32_t mq = 0, mt = 0;
  for (int32_t k = 0; k < n; ++k) mq = std::max(mq, pk.qlen[k]), mt = std::max(mt, pk.tlen[k]);
  if ((rc = check_codes(who, pk.q.data(), pk.b.qbytes, "query")) || (rc = check_codes(who, pk.t.data(), pk.b.tbytes, "target")))
    return rc;
  if ((rc = check_device(device))) return rc;
  FCS_SET_DEVICE((device));
  SessionLease lease;
  if ((rc = lease.acquire(device))) return rc;
  Session* S = lease.get();
  const size_t nn = (size_t)n;
  Arena L;
  const BswLayout T = layout_tasks(pk.b, false, L);
  const size_t ox = L.add(4 * nn), in_bytes = L.total, oo = L.add(sizeof(fcs_kswr) * nn);
  // pinned: the staged inputs, then the results at their device offset, all within L.total; the 1024 bytes
  // beyond it are never touched and stay so that sessions grow at the sizes they always did
  if ((rc = S->ensure_host(L.total + 1024)) || (rc = S->ensure_dev(L.total))) return rc;
  const BswDevBatch d = stage_tasks(pk.b, T, S->hbase(), S->dbase());
  std::memcpy(S->h<void>(ox), xtra, 4 * nn);
  hipStream_t s = S->s;
  const StreamDrain drain{s};
  FCS_HIP_CHECK(hipMemcpyAsync(S->dev, S->host, in_bytes, hipMemcpyHostToDevice, s));
  bool all_u8 = true;
  for (int32_t k = 0; k < n; ++k) all_u8 = all_u8 && (xtra[k] & FCS_KSW_XBYTE);
  if ((rc = launch_bsw_align(d, to_params(params), S->d<int32_t>(ox), mq, mt, S->d<int32_t>(oo), s, all_u8)))
    return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S->h<void>(oo), S->d<void>(oo), sizeof(fcs_kswr) * nn, hipMemcpyDeviceToHost, s));
  FCS_HIP_CHECK(hipStreamSynchronize(s));
  std::memcpy(out, S->h<void>(oo), sizeof(fcs_kswr) * nn);
  return FCS_OK;
}

int fcs_bsw_align_dev(const fcs_bsw_batch* b, const fcs_bsw_params* params, const int32_t* dev_xtra, fcs_kswr* dev_out,
                      int32_t device, void* stream) {
  if (!b || b->n < 0 || (b->n > 0 && (!dev_xtra || !dev_out)))
    return fail(FCS_ERR_INVALID, "[E::fcs_bsw_align_dev] bad arguments");
  int rc = check_params(params);
  if (rc) return rc;
  if (b->n == 0) return FCS_OK;
  if (b->n > 0x7FFFFFFF) return fail(FCS_ERR_UNSUPPORTED, "[E::fcs_bsw_align_dev] more than 2^31-1 tasks");
  if ((rc = check_device(device))) return rc;
  FCS_SET_DEVICE((device));
  return launch_bsw_align(bsw_dev(b), to_params(params), dev_xtra, std::max(b->max_qlen, 1), std::max(b->max_tlen, 1),
                          reinterpret_cast<int32_t*>(dev_out), (hipStream_t)stream, false);
}

fcs_kswr fcs_ksw_align2(int qlen, const uint8_t* query, int tlen, const uint8_t* target, int m, const int8_t* mat,
                        int o_del, int e_del, int o_ins, int e_ins, int xtra, void** qry) {
  fcs_kswr r{FCS_KSW_FAILED, -1, -1, -1, -1, -1, -1};
  fcs_bsw_params p;
  if (!ksw_params("fcs_ksw_align2", m, mat, o_del, e_del, o_ins, e_ins, 0, 0, p)) return r;
  if (qry && *qry) return (void)fail(FCS_ERR_UNSUPPORTED, "[E::fcs_ksw_align2] cached query profiles unsupported"), r;
  fcs_bsw_task t{qlen, tlen, 0, 0, query, target};
  fcs_kswr out;
  if (fcs_bsw_align(&t, 1, &p, &xtra, &out, default_device())) return r;
  return out;
}

int fcs_ksw_extend2(int qlen, const uint8_t* query, int tlen, const uint8_t* target, int m, const int8_t* mat,
                    int o_del, int e_del, int o_ins, int e_ins, int w, int end_bonus, int zdrop, int h0, int* qle,
                    int* tle, int* gtle, int* gscore, int* max_off) {
  fcs_bsw_params p;
  if (!ksw_params("fcs_ksw_extend2", m, mat, o_del, e_del, o_ins, e_ins, end_bonus, zdrop, p)) return FCS_KSW_FAILED;
  fcs_bsw_task t{qlen, tlen, h0, w, query, target};
  fcs_bsw_result r;
  int rc = fcs_bsw_extend(&t, 1, &p, &r, default_device());
  if (rc) return FCS_KSW_FAILED;
  if (qle) *qle = r.qle;
  if (tle) *tle = r.tle;
  if (gtle) *gtle = r.gtle;
  if (gscore) *gscore = r.gscore;
  if (max_off) *max_off = r.max_off;
  return r.score;
}

int fcs_ksw_global2(int qlen, const uint8_t* query, int tlen, const uint8_t* target, int m, const int8_t* mat,
                    int o_del, int e_del, int o_ins, int e_ins, int w, int* n_cigar, uint32_t** cigar) {
  fcs_bsw_params p;
  if (!ksw_params("fcs_ksw_global2", m, mat, o_del, e_del, o_ins, e_ins, 0, 0, p)) return FCS_KSW_FAILED;
  fcs_bsw_task t{qlen, tlen, 1, w, query, target};
  int32_t score = 0;
  const bool want = n_cigar && cigar;
  const int32_t cap = qlen + tlen + 2;
  std::vector<uint32_t> arena(want ? cap : 0);
  int64_t off = 0;
  int32_t nc = 0;
  int rc = fcs_bsw_global(&t, 1, &p, &score, want ? arena.data() : nullptr, want ? &off : nullptr,
                          want ? &cap : nullptr, want ? &nc : nullptr, default_device());
  if (rc) return FCS_KSW_FAILED;
  if (want) {
    *n_cigar = nc;
    *cigar = nc ? static_cast<uint32_t*>(std::malloc(sizeof(uint32_t) * nc)) : nullptr;
    if (nc && !*cigar) return (void)fail(FCS_ERR_NOMEM, "[E::fcs_ksw_global2] malloc failed"), FCS_KSW_FAILED;
    if (nc) std::memcpy(*cigar, arena.data(), sizeof(uint32_t) * nc);
  }
  return score;
}

}  // extern "C"
