// PairHMM calls of the C-ABI (include/fcship.h): the plan and its stream-level
// stages, the staged host calls and the static multi-device partition.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#include "session.h"

using namespace fcs;

static thread_local int64_t g_last_rescued = 0;
static thread_local double g_last_device_ms = 0, g_last_rescue_ms = 0;

struct fcs_phmm_plan {
  int device = 0;
  int64_t max_pairs = 0;
  int32_t* idx_out = nullptr;  // the schedule: pair indices, launch class by class
  int32_t* rescue_list = nullptr;
  int32_t* fb_list = nullptr;                  // pairs the streamed kernel hands back (bytes outside ACGTN)
  // [0] rescue count, [1] fallback count, [2 ..] the column classes' queue heads (kPhmmCounters words, zeroed
  // together), then the int64 class bounds
  unsigned long long* rescue_count = nullptr;
  unsigned long long* fb_count = nullptr;
  int64_t* bounds = nullptr;
  uint32_t* bin_hist = nullptr;    // the bin schedule's histogram (kept zero between schedules)
  uint32_t* bin_cursor = nullptr;  // and its running bin starts
  bool bin_zeroed = false;         // bin_hist zeroed on a schedule stream (then kept zero by the scan)
  int64_t scheduled = -1;  // n_pairs of the last schedule
  bool counters_zeroed = false;  // the last schedule's count kernel zeroed rescue_count[0 .. kPhmmCounters - 1]
};

int Session::ensure_phmm(int64_t pairs) {
  if (phmm && phmm->max_pairs >= pairs) return FCS_OK;
  FCS_HIP_CHECK(hipStreamSynchronize(s));
  fcs_phmm_plan_destroy(phmm);
  phmm = nullptr;
  return fcs_phmm_plan_create(device, (int64_t)grown((size_t)pairs, 0), &phmm);
}

// FCSHIP_TEST_FAULT=drop_schedule: the PairHMM schedule publishes empty class
// ranges, as the round-1 null-stream memset race once did, so the forward
// pass computes nothing (tests/test_pairhmm_gpu.py checks it is reported).
static bool fault_drop_schedule() {
  static const bool on = [] {
    const char* e = std::getenv("FCSHIP_TEST_FAULT");
    return e && std::strcmp(e, "drop_schedule") == 0;
  }();
  return on;
}

static PhmmDevBatch to_dev(const fcs_phmm_batch* b) {
  return PhmmDevBatch{b->read_bases, b->read_bq,  b->read_iq, b->read_dq,   b->read_gcp, b->read_off, b->read_len,
                      b->hap_bases,  b->hap_off,  b->hap_len, b->pair_read, b->pair_hap, b->n_pairs};
}

static int check_batch_shape(const fcs_phmm_batch* b) {
  if (!b) return fail(FCS_ERR_INVALID, "[E::fcship] null PairHMM batch");
  if (b->n_pairs < 0 || b->n_reads < 0 || b->n_haps < 0)
    return fail(FCS_ERR_INVALID, "[E::fcship] negative PairHMM batch size");
  if (b->n_pairs > 0x7FFFFFFF) return fail(FCS_ERR_UNSUPPORTED, "[E::fcship] more than 2^31-1 pairs per batch");
  if (b->n_pairs > 0 && (!b->read_bases || !b->read_bq || !b->read_iq || !b->read_dq || !b->read_gcp ||
                         !b->read_off || !b->read_len || !b->hap_bases || !b->hap_off || !b->hap_len ||
                         !b->pair_read || !b->pair_hap))
    return fail(FCS_ERR_INVALID, "[E::fcship] null pointer in PairHMM batch");
  if (b->max_hap_len < 0 || b->max_read_len < 0)
    return fail(FCS_ERR_INVALID, "[E::fcship] negative max length in PairHMM batch");
  return FCS_OK;
}

static fcs_phmm_opts opts_or_default(const fcs_phmm_opts* opts_in) {
  fcs_phmm_opts opts;
  if (opts_in) opts = *opts_in;
  else fcs_phmm_opts_default(&opts);
  return opts;
}

extern "C" {

void fcs_phmm_opts_default(fcs_phmm_opts* o) {
  if (o) *o = fcs_phmm_opts{0, 1, 1e-28f, 0};  // device 0, fp64 rescue below GKL's MIN_ACCEPTED, fast order
}

int fcs_phmm_plan_create(int32_t device, int64_t max_pairs, fcs_phmm_plan** plan) {
  if (!plan || max_pairs < 0) return fail(FCS_ERR_INVALID, "[E::fcs_phmm_plan_create] bad arguments");
  int rc = check_device(device);
  if (rc) return rc;
  FCS_SET_DEVICE((device));
  DeviceTables* t = nullptr;
  rc = get_device_tables(device, &t);
  if (rc) return rc;
  std::unique_ptr<fcs_phmm_plan> p(new fcs_phmm_plan());
  p->device = device;
  p->max_pairs = max_pairs;
  const size_t n = (size_t)std::max<int64_t>(max_pairs, 1);
  FCS_HIP_CHECK(hipMalloc(&p->idx_out, n * 4));
  FCS_HIP_CHECK(hipMalloc(&p->rescue_list, n * 4));
  FCS_HIP_CHECK(hipMalloc(&p->fb_list, n * 4));
  FCS_HIP_CHECK(hipMalloc(&p->rescue_count, (kPhmmCounters + kPhmmLaunchClasses + 1) * sizeof(unsigned long long)));
  // Nothing is initialised here: every run writes the class bounds (the bounds
  // kernel stores all kPhmmClasses + 1 of them) and zeroes the rescue count on
  // the caller's stream.  (Round 1 zeroed them with a null-stream hipMemset,
  // which does not order against the non-blocking streams the plan runs on and
  // once landed after a schedule, so class launches computed nothing.)
  p->fb_count = p->rescue_count + 1;
  p->bounds = reinterpret_cast<int64_t*>(p->rescue_count + kPhmmCounters);
  constexpr size_t kBins = (size_t)1 << (kPhmmKeyBits - 4);
  FCS_HIP_CHECK(hipMalloc(&p->bin_hist, 2 * kBins * sizeof(uint32_t)));
  p->bin_cursor = p->bin_hist + kBins;
  *plan = p.release();  // (the bin histogram is zeroed on the first schedule's stream)
  return FCS_OK;
}

int fcs_phmm_plan_destroy(fcs_phmm_plan* p) {
  if (!p) return FCS_OK;
  ::fcs::DeviceScope dev_scope;
  (void)hipSetDevice(p->device);
  (void)hipFree(p->idx_out);
  (void)hipFree(p->rescue_list);
  (void)hipFree(p->fb_list);
  (void)hipFree(p->rescue_count);
  (void)hipFree(p->bin_hist);
  delete p;
  return FCS_OK;
}

int fcs_phmm_dev_schedule(fcs_phmm_plan* plan, const fcs_phmm_batch* b, void* stream) {
  if (!plan) return fail(FCS_ERR_INVALID, "[E::fcs_phmm_dev_schedule] null plan");
  int rc = check_batch_shape(b);
  if (rc) return rc;
  if (b->n_pairs > plan->max_pairs) return fail(FCS_ERR_INVALID, "[E::fcs_phmm_dev_schedule] batch exceeds plan");
  FCS_SET_DEVICE((plan->device));
  hipStream_t s = (hipStream_t)stream;
  const PhmmDevBatch d = to_dev(b);
  // The bin schedule: a counting sort on the key's top 12 bits in three
  // kernels (count, scan, scatter).  It replaced a 16-bit rocPRIM radix sort
  // (eight launches and look-back state fills, ≈ 0.15 ms of a 1M-pair C2 step;
  // A/B in profiles/r5/r5av_phmm_schedule_ab.log).  The histogram is zeroed
  // stream-ordered, once per plan (a synchronous hipMemset at plan creation
  // waited behind other shards' kernels on the device: htc PairHMM call time
  // 0.45 -> 2.2 thread-s in r5aw), and the scan kernel leaves it zero.  Any
  // failure before the scan ran may leave it dirty: the next schedule zeroes
  // it again.
  plan->scheduled = -1;
  if (!plan->bin_zeroed)
    FCS_HIP_CHECK(hipMemsetAsync(plan->bin_hist, 0, ((size_t)1 << (kPhmmKeyBits - 4)) * sizeof(uint32_t), s));
  plan->bin_zeroed = false;  // until the scan has been launched
  if ((rc = launch_phmm_bin_schedule(d, plan->idx_out, plan->bounds, plan->rescue_count, plan->bin_hist,
                                     plan->bin_cursor, s)))
    return rc;
  plan->bin_zeroed = true;
  plan->counters_zeroed = true;
  if (fault_drop_schedule()) FCS_HIP_CHECK(hipMemsetAsync(plan->bounds, 0, (kPhmmLaunchClasses + 1) * sizeof(int64_t), s));
  plan->scheduled = b->n_pairs;
  return FCS_OK;
}

int fcs_phmm_dev_forward(fcs_phmm_plan* plan, const fcs_phmm_batch* b, double* out, const fcs_phmm_opts* opts,
                         void* stream) {
  if (!plan || !opts) return fail(FCS_ERR_INVALID, "[E::fcs_phmm_dev_forward] null plan/opts");
  int rc = check_batch_shape(b);
  if (rc) return rc;
  if (plan->scheduled != b->n_pairs)
    return fail(FCS_ERR_INVALID, "[E::fcs_phmm_dev_forward] batch not scheduled (call fcs_phmm_dev_schedule)");
  if (b->n_pairs > 0 && !out) return fail(FCS_ERR_INVALID, "[E::fcs_phmm_dev_forward] null output");
  FCS_SET_DEVICE((plan->device));
  DeviceTables* t = nullptr;
  rc = get_device_tables(plan->device, &t);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  // rescue + fallback counts and the queue heads: zeroed by the schedule's count
  // kernel for the first forward pass after it, by a memset for any further pass
  if (!plan->counters_zeroed)
    FCS_HIP_CHECK(hipMemsetAsync(plan->rescue_count, 0, kPhmmCounters * sizeof(unsigned long long), s));
  plan->counters_zeroed = false;
  return launch_phmm_forward(to_dev(b), plan->idx_out, b->n_pairs, std::max(b->max_hap_len, 1), plan->bounds, *t,
                             opts->exact_order != 0, out, plan->rescue_list, plan->rescue_count,
                             opts->rescue_threshold, opts->use_fp64_rescue != 0, plan->fb_list, plan->fb_count,
                             plan->rescue_count + kPhmmQueueHead0, s);
}

int fcs_phmm_dev_rescue(fcs_phmm_plan* plan, const fcs_phmm_batch* b, double* out, const fcs_phmm_opts* opts,
                        void* stream) {
  if (!plan || !opts) return fail(FCS_ERR_INVALID, "[E::fcs_phmm_dev_rescue] null plan/opts");
  int rc = check_batch_shape(b);
  if (rc) return rc;
  if (!opts->use_fp64_rescue) return FCS_OK;
  FCS_SET_DEVICE((plan->device));
  DeviceTables* t = nullptr;
  rc = get_device_tables(plan->device, &t);
  if (rc) return rc;
  return launch_phmm_rescue(to_dev(b), plan->rescue_list, plan->rescue_count, b->n_pairs,
                            std::max(b->max_hap_len, 1), *t, opts->exact_order != 0, out, (hipStream_t)stream);
}

int fcs_phmm_dev_run(fcs_phmm_plan* plan, const fcs_phmm_batch* b, double* out, const fcs_phmm_opts* opts,
                     void* stream) {
  int rc = fcs_phmm_dev_schedule(plan, b, stream);
  if (rc) return rc;
  rc = fcs_phmm_dev_forward(plan, b, out, opts, stream);
  if (rc) return rc;
  return fcs_phmm_dev_rescue(plan, b, out, opts, stream);
}

int fcs_phmm_last_device_ms(double* device_ms, double* rescue_ms) {
  if (!device_ms || !rescue_ms) return fail(FCS_ERR_INVALID, "[E::fcs_phmm_last_device_ms] null output");
  *device_ms = g_last_device_ms;
  *rescue_ms = g_last_rescue_ms;
  return FCS_OK;
}

int fcs_phmm_last_rescued(int64_t* count) {
  if (!count) return fail(FCS_ERR_INVALID, "[E::fcs_phmm_last_rescued] null count");
  *count = g_last_rescued;
  return FCS_OK;
}

int fcs_phmm_plan_rescue_count(fcs_phmm_plan* plan, void* stream, int64_t* count) {
  if (!plan || !count) return fail(FCS_ERR_INVALID, "[E::fcs_phmm_plan_rescue_count] bad arguments");
  FCS_SET_DEVICE((plan->device));
  unsigned long long v = 0;
  FCS_HIP_CHECK(hipMemcpyAsync(&v, plan->rescue_count, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream));
  FCS_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  *count = (int64_t)v;
  return FCS_OK;
}

}  // extern "C"

namespace {

// Host side of one synchronous PairHMM pass: `fill` writes the batch's SoA
// arrays into the session's pinned staging at the offsets of `off` (order of
// PhmmStage), then one H2D copy, schedule + forward + rescue on the thread's
// stream into an output pre-filled with NaN, one D2H copy, and a check that
// every pair's result was written (a pair the schedule or a class launch
// skipped would otherwise go downstream as garbage).  Returns the results in
// pinned memory (valid while the caller holds the lease).
struct PhmmStage {
  int64_t n_reads = 0, n_haps = 0, n_pairs = 0, read_bytes = 0, hap_bytes = 0;
  int32_t max_read_len = 0, max_hap_len = 0;
};
enum { kRb, kBq, kIq, kDq, kGq, kRo, kRl, kHb, kHo, kHl, kPr, kPh, kNArr };

template <typename Fill>
int phmm_staged(const PhmmStage& g, const fcs_phmm_opts& opts, SessionLease& lease, Fill&& fill,
                const double** host_out) {
  int rc = check_device(opts.device);
  if (rc) return rc;
  FCS_SET_DEVICE((opts.device));
  // FCS_PHMM_TRACE=1: one stderr line per call with its host-side phases (ms)
  static const bool trace = std::getenv("FCS_PHMM_TRACE") != nullptr;
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  static const auto t_load = t0;  // the first call
  auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  if ((rc = lease.acquire(opts.device))) return rc;
  const auto t_lease = clk::now();
  Session* S = lease.get();
  const size_t RB = (size_t)g.read_bytes, HB = (size_t)g.hap_bytes, nr = (size_t)g.n_reads, nh = (size_t)g.n_haps,
               np = (size_t)g.n_pairs;
  Arena L;
  size_t off[kNArr];
  for (int k = kRb; k <= kGq; ++k) off[k] = L.add(RB);
  off[kRo] = L.add(8 * nr);
  off[kRl] = L.add(4 * nr);
  off[kHb] = L.add(HB);
  off[kHo] = L.add(8 * nh);
  off[kHl] = L.add(4 * nh);
  off[kPr] = L.add(4 * np);
  off[kPh] = L.add(4 * np);
  const size_t in_bytes = L.total, out_off = L.add(8 * np);
  const bool grew = L.total > S->host_cap || L.total > S->dev_cap || !S->phmm || S->phmm->max_pairs < g.n_pairs;
  if ((rc = S->ensure_host(L.total)) || (rc = S->ensure_dev(L.total)) || (rc = S->ensure_phmm(g.n_pairs))) return rc;
  const auto t_ensure = clk::now();
  fill(S, off);
  const auto t_fill = clk::now();
  hipStream_t s = S->s;
  const StreamDrain drain{s};
  FCS_HIP_CHECK(hipMemcpyAsync(S->dev, S->host, in_bytes, hipMemcpyHostToDevice, s));
  const fcs_phmm_batch d{S->d<uint8_t>(off[kRb]), S->d<uint8_t>(off[kBq]), S->d<uint8_t>(off[kIq]),
                         S->d<uint8_t>(off[kDq]), S->d<uint8_t>(off[kGq]), S->d<int64_t>(off[kRo]),
                         S->d<int32_t>(off[kRl]), g.n_reads,               S->d<uint8_t>(off[kHb]),
                         S->d<int64_t>(off[kHo]), S->d<int32_t>(off[kHl]), g.n_haps,
                         S->d<int32_t>(off[kPr]), S->d<int32_t>(off[kPh]), g.n_pairs,
                         g.read_bytes,            g.hap_bytes,             g.max_read_len,
                         g.max_hap_len};
  double* dout = S->d<double>(out_off);
  FCS_HIP_CHECK(hipMemsetAsync(dout, 0xFF, 8 * np, s));  // all-ones = NaN: "not written"
  for (hipEvent_t& e : S->ev)
    if (!e) FCS_HIP_CHECK(hipEventCreate(&e));
  FCS_HIP_CHECK(hipEventRecord(S->ev[0], s));
  if ((rc = fcs_phmm_dev_schedule(S->phmm, &d, s)) || (rc = fcs_phmm_dev_forward(S->phmm, &d, dout, &opts, s)))
    return rc;
  FCS_HIP_CHECK(hipEventRecord(S->ev[1], s));
  if ((rc = fcs_phmm_dev_rescue(S->phmm, &d, dout, &opts, s))) return rc;
  FCS_HIP_CHECK(hipEventRecord(S->ev[2], s));
  double* hout = S->h<double>(out_off);
  FCS_HIP_CHECK(hipMemcpyAsync(hout, dout, 8 * np, hipMemcpyDeviceToHost, s));
  // into the input staging: its H2D copy is stream-ordered before this copy
  unsigned long long* hres = S->h<unsigned long long>(0);
  g_last_rescued = 0;
  if (opts.use_fp64_rescue)
    FCS_HIP_CHECK(hipMemcpyAsync(hres, S->phmm->rescue_count, sizeof(*hres), hipMemcpyDeviceToHost, s));
  const auto t_issue = clk::now();
  FCS_HIP_CHECK(hipStreamSynchronize(s));
  const auto t_sync = clk::now();
  if (opts.use_fp64_rescue) g_last_rescued = (int64_t)*hres;
  float ms_all = 0.f, ms_res = 0.f;
  FCS_HIP_CHECK(hipEventElapsedTime(&ms_all, S->ev[0], S->ev[2]));
  FCS_HIP_CHECK(hipEventElapsedTime(&ms_res, S->ev[1], S->ev[2]));
  g_last_device_ms = ms_all;
  g_last_rescue_ms = ms_res;
  if (trace)
    std::fprintf(stderr,
                 "[fcs_phmm_trace] at %.1f pairs %lld bytes %zu lease %.3f ensure %.3f%s fill %.3f issue %.3f sync %.3f "
                 "device %.3f total %.3f\n",
                 ms(t_load, t0), (long long)np, in_bytes, ms(t0, t_lease), ms(t_lease, t_ensure), grew ? " (grew)" : "",
                 ms(t_ensure, t_fill), ms(t_fill, t_issue), ms(t_issue, t_sync), (double)ms_all, ms(t0, t_sync));
  int64_t missing = 0;
  for (size_t k = 0; k < np; ++k) missing += std::isnan(hout[k]);
  if (missing)
    return fail(FCS_ERR_DEVICE, "[E::fcship] PairHMM: " + std::to_string(missing) + " of " + std::to_string(np) +
                                    " results were not written by the device pass");
  *host_out = hout;
  return FCS_OK;
}

// Runs f(k0, k1) over contiguous region ranges: on the calling thread for a
// small batch, on up to 8 threads for a large one (a pass merged from many
// shards' batches, host/caller.cpp, stages ~100 MB through per-read memcpys;
// on one thread that serialised the shards waiting for it).
template <class F>
void for_region_ranges(int32_t n, int64_t bytes, F&& f) {
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const int nt = (int)std::min<int64_t>({8, (int64_t)hw, n, bytes / (4 << 20)});
  if (nt <= 1) {
    f(0, n);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(nt - 1);
  const int32_t chunk = (n + nt - 1) / nt;
  for (int t = 1; t < nt; ++t) {
    const int32_t a = t * chunk, b = std::min(n, a + chunk);
    if (a < b) th.emplace_back([&f, a, b] { f(a, b); });
  }
  f(0, std::min(n, chunk));
  for (auto& x : th) x.join();
}

}  // namespace

extern "C" {

int fcs_phmm_partition(const fcs_phmm_batch* b, int32_t n_slices, int64_t* cuts) {
  int rc = check_batch_shape(b);
  if (rc) return rc;
  if (n_slices <= 0 || !cuts) return fail(FCS_ERR_INVALID, "[E::fcs_phmm_partition] need n_slices > 0 and cuts");
  const int64_t n = b->n_pairs;
  std::vector<double> cum((size_t)n);
  double run = 0;
  for (int64_t p = 0; p < n; ++p) {
    const int32_t ri = b->pair_read[p], hi = b->pair_hap[p];
    if (ri < 0 || ri >= b->n_reads || hi < 0 || hi >= b->n_haps)
      return fail(FCS_ERR_INVALID, "[E::fcs_phmm_partition] pair index out of range");
    cum[p] = (run += (double)b->read_len[ri] * (double)b->hap_len[hi]);
  }
  balanced_cuts(cum, n, n_slices, cuts);
  return FCS_OK;
}

int fcs_phmm_compute_pairs_multi(const fcs_phmm_batch* b, double* out_log10, const fcs_phmm_opts* opts_in,
                                 const int32_t* devices, int32_t n_devices) {
  if (n_devices <= 0 || !devices) return fail(FCS_ERR_INVALID, "[E::fcs_phmm_compute_pairs_multi] no devices");
  std::vector<int64_t> cuts((size_t)n_devices + 1);
  int rc = fcs_phmm_partition(b, n_devices, cuts.data());
  if (rc) return rc;
  if (b->n_pairs > 0 && !out_log10) return fail(FCS_ERR_INVALID, "[E::fcs_phmm_compute_pairs_multi] null output");
  const fcs_phmm_opts opts = opts_or_default(opts_in);
  std::vector<int64_t> resc((size_t)n_devices, 0);
  rc = run_slices(cuts, [&](int32_t k) {
    fcs_phmm_batch sub = *b;
    sub.pair_read = b->pair_read + cuts[k];
    sub.pair_hap = b->pair_hap + cuts[k];
    sub.n_pairs = cuts[k + 1] - cuts[k];
    fcs_phmm_opts o = opts;
    o.device = devices[k];
    const int rck = fcs_phmm_compute_pairs(&sub, out_log10 + cuts[k], &o);
    int64_t r = 0;
    if (fcs_phmm_last_rescued(&r) == FCS_OK) resc[k] = r;
    return rck;
  });
  if (rc) return rc;
  int64_t tot = 0;
  for (int64_t r : resc) tot += r;
  g_last_rescued = tot;
  return FCS_OK;
}

int fcs_phmm_compute_pairs(const fcs_phmm_batch* b, double* out_log10, const fcs_phmm_opts* opts_in) {
  int rc = check_batch_shape(b);
  if (rc) return rc;
  const fcs_phmm_opts opts = opts_or_default(opts_in);
  if (b->n_pairs == 0) return FCS_OK;
  if (!out_log10) return fail(FCS_ERR_INVALID, "[E::fcs_phmm_compute_pairs] null output");
  // Validate indices and lengths on the host (the device path trusts its caller).
  PhmmStage g;
  g.n_reads = b->n_reads;
  g.n_haps = b->n_haps;
  g.n_pairs = b->n_pairs;
  g.read_bytes = b->read_bytes;
  g.hap_bytes = b->hap_bytes;
  for (int64_t p = 0; p < b->n_pairs; ++p) {
    const int32_t ri = b->pair_read[p], hi = b->pair_hap[p];
    if (ri < 0 || ri >= b->n_reads || hi < 0 || hi >= b->n_haps)
      return fail(FCS_ERR_INVALID, "[E::fcs_phmm_compute_pairs] pair index out of range");
  }
  for (int64_t r = 0; r < b->n_reads; ++r) {
    if (b->read_len[r] < 0 || b->read_off[r] < 0 || b->read_off[r] + b->read_len[r] > b->read_bytes)
      return fail(FCS_ERR_INVALID, "[E::fcs_phmm_compute_pairs] read extent outside read arrays");
    g.max_read_len = std::max(g.max_read_len, b->read_len[r]);
  }
  for (int64_t h = 0; h < b->n_haps; ++h) {
    if (b->hap_len[h] < 0 || b->hap_off[h] < 0 || b->hap_off[h] + b->hap_len[h] > b->hap_bytes)
      return fail(FCS_ERR_INVALID, "[E::fcs_phmm_compute_pairs] hap extent outside hap array");
    g.max_hap_len = std::max(g.max_hap_len, b->hap_len[h]);
  }
  const size_t RB = (size_t)b->read_bytes, HB = (size_t)b->hap_bytes, nr = (size_t)b->n_reads,
               nh = (size_t)b->n_haps, np = (size_t)b->n_pairs;
  const double* res = nullptr;
  SessionLease lease;  // holds the pinned results until they are copied out
  rc = phmm_staged(g, opts, lease, [&](Session* S, const size_t* off) {
    std::memcpy(S->h<void>(off[kRb]), b->read_bases, RB);
    std::memcpy(S->h<void>(off[kBq]), b->read_bq, RB);
    std::memcpy(S->h<void>(off[kIq]), b->read_iq, RB);
    std::memcpy(S->h<void>(off[kDq]), b->read_dq, RB);
    std::memcpy(S->h<void>(off[kGq]), b->read_gcp, RB);
    std::memcpy(S->h<void>(off[kRo]), b->read_off, 8 * nr);
    std::memcpy(S->h<void>(off[kRl]), b->read_len, 4 * nr);
    std::memcpy(S->h<void>(off[kHb]), b->hap_bases, HB);
    std::memcpy(S->h<void>(off[kHo]), b->hap_off, 8 * nh);
    std::memcpy(S->h<void>(off[kHl]), b->hap_len, 4 * nh);
    std::memcpy(S->h<void>(off[kPr]), b->pair_read, 4 * np);
    std::memcpy(S->h<void>(off[kPh]), b->pair_hap, 4 * np);
  }, &res);
  if (rc) return rc;
  std::memcpy(out_log10, res, 8 * np);
  return FCS_OK;
}

int fcs_phmm_compute(const fcs_phmm_read* reads, int32_t n_reads, const fcs_phmm_hap* haps, int32_t n_haps,
                     double* out_log10, const fcs_phmm_opts* opts) {
  if (n_reads < 0 || n_haps < 0 || (n_reads > 0 && !reads) || (n_haps > 0 && !haps))
    return fail(FCS_ERR_INVALID, "[E::fcs_phmm_compute] bad arguments");
  if ((int64_t)n_reads * n_haps == 0) return FCS_OK;
  if (!out_log10) return fail(FCS_ERR_INVALID, "[E::fcs_phmm_compute] null output");
  fcs_phmm_region r{reads, n_reads, haps, n_haps, out_log10};
  return fcs_phmm_compute_regions(&r, 1, opts);
}

// Many active regions in one device pass: the regions' reads and haplotypes
// are concatenated (straight into the pinned staging) into one SoA batch whose
// pair list is region-major and read-major within a region, so the flat
// result splits back into each region's read-major matrix by a running offset.
int fcs_phmm_compute_regions(const fcs_phmm_region* regions, int32_t n_regions, const fcs_phmm_opts* opts_in) {
  if (n_regions < 0 || (n_regions > 0 && !regions))
    return fail(FCS_ERR_INVALID, "[E::fcs_phmm_compute_regions] bad arguments");
  PhmmStage g;
  // per-region starts in the packed batch (reads, haplotypes, pairs, read and
  // hap bytes): regions are staged independently, in parallel when large
  std::vector<int64_t> r_at(n_regions + 1), h_at(n_regions + 1), p_at(n_regions + 1), rb_at(n_regions + 1),
      hb_at(n_regions + 1);
  for (int32_t k = 0; k < n_regions; ++k) {
    const fcs_phmm_region& R = regions[k];
    r_at[k] = g.n_reads, h_at[k] = g.n_haps, p_at[k] = g.n_pairs, rb_at[k] = g.read_bytes, hb_at[k] = g.hap_bytes;
    if (R.n_reads < 0 || R.n_haps < 0 || (R.n_reads > 0 && !R.reads) || (R.n_haps > 0 && !R.haps))
      return fail(FCS_ERR_INVALID, "[E::fcs_phmm_compute_regions] malformed region");
    const int64_t pairs = (int64_t)R.n_reads * R.n_haps;
    if (pairs > 0 && !R.out_log10) return fail(FCS_ERR_INVALID, "[E::fcs_phmm_compute_regions] null region output");
    for (int32_t r = 0; r < R.n_reads; ++r) {
      const fcs_phmm_read& x = R.reads[r];
      if (x.len < 0 || (x.len > 0 && (!x.bases || !x.base_q || !x.ins_q || !x.del_q || !x.gcp)))
        return fail(FCS_ERR_INVALID, "[E::fcs_phmm_compute_regions] malformed read");
      g.read_bytes += x.len;
      g.max_read_len = std::max(g.max_read_len, x.len);
    }
    for (int32_t h = 0; h < R.n_haps; ++h) {
      if (R.haps[h].len < 0 || (R.haps[h].len > 0 && !R.haps[h].bases))
        return fail(FCS_ERR_INVALID, "[E::fcs_phmm_compute_regions] malformed haplotype");
      g.hap_bytes += R.haps[h].len;
      g.max_hap_len = std::max(g.max_hap_len, R.haps[h].len);
    }
    g.n_reads += R.n_reads;
    g.n_haps += R.n_haps;
    g.n_pairs += pairs;
  }
  if (g.n_pairs == 0) return FCS_OK;
  if (g.n_reads > INT32_MAX || g.n_haps > INT32_MAX || g.n_pairs > INT32_MAX)
    return fail(FCS_ERR_INVALID, "[E::fcs_phmm_compute_regions] more than 2^31 reads, haplotypes or pairs");
  const fcs_phmm_opts opts = opts_or_default(opts_in);
  const double* res = nullptr;
  SessionLease lease;  // holds the pinned results until they are copied out
  const int rc = phmm_staged(g, opts, lease, [&](Session* S, const size_t* off) {
    uint8_t *rb = S->h<uint8_t>(off[kRb]), *bq = S->h<uint8_t>(off[kBq]), *iq = S->h<uint8_t>(off[kIq]),
            *dq = S->h<uint8_t>(off[kDq]), *gq = S->h<uint8_t>(off[kGq]), *hb = S->h<uint8_t>(off[kHb]);
    int64_t *roff = S->h<int64_t>(off[kRo]), *hoff = S->h<int64_t>(off[kHo]);
    int32_t *rlen = S->h<int32_t>(off[kRl]), *hlen = S->h<int32_t>(off[kHl]), *pr = S->h<int32_t>(off[kPr]),
            *ph = S->h<int32_t>(off[kPh]);
    for_region_ranges(n_regions, g.read_bytes + 8 * g.n_pairs, [&](int32_t k0, int32_t k1) {
      for (int32_t k = k0; k < k1; ++k) {
        const fcs_phmm_region& R = regions[k];
        int64_t ri = r_at[k], hi = h_at[k], pi = p_at[k], ro = rb_at[k], ho = hb_at[k];
        const int64_t r0 = ri, h0 = hi;
        for (int32_t r = 0; r < R.n_reads; ++r, ++ri) {
          const fcs_phmm_read& x = R.reads[r];
          roff[ri] = ro;
          rlen[ri] = x.len;
          if (x.len) {
            std::memcpy(rb + ro, x.bases, x.len);
            std::memcpy(bq + ro, x.base_q, x.len);
            std::memcpy(iq + ro, x.ins_q, x.len);
            std::memcpy(dq + ro, x.del_q, x.len);
            std::memcpy(gq + ro, x.gcp, x.len);
          }
          ro += x.len;
        }
        for (int32_t h = 0; h < R.n_haps; ++h, ++hi) {
          hoff[hi] = ho;
          hlen[hi] = R.haps[h].len;
          if (R.haps[h].len) std::memcpy(hb + ho, R.haps[h].bases, R.haps[h].len);
          ho += R.haps[h].len;
        }
        for (int32_t r = 0; r < R.n_reads; ++r)
          for (int32_t h = 0; h < R.n_haps; ++h, ++pi) {
            pr[pi] = (int32_t)(r0 + r);
            ph[pi] = (int32_t)(h0 + h);
          }
      }
    });
  }, &res);
  if (rc) return rc;
  for_region_ranges(n_regions, 8 * g.n_pairs, [&](int32_t k0, int32_t k1) {
    for (int32_t k = k0; k < k1; ++k) {
      const int64_t pairs = (int64_t)regions[k].n_reads * regions[k].n_haps;
      if (pairs) std::memcpy(regions[k].out_log10, res + p_at[k], 8 * (size_t)pairs);
    }
  });
  return FCS_OK;
}

}  // extern "C"
