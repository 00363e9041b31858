// The shared core of libfcship.so's C-ABI (include/fcship.h): the error
// plumbing, device state, fork streams and the session pools, with the entry
// points that manage them.  The feature calls live in phmm_api.cpp,
// bsw_api.cpp, bgzf_api.cpp and fmd_api.cpp.
//
// Error behaviour mirrors the reference's contract: a failing
// call returns a negative code and leaves a "[E::fcship] ..." message (the
// prefix the reference's LogUtils::findError scans task logs for) retrievable
// with fcs_last_error().
#include "session.h"

#include <cmath>
#include <condition_variable>
#include <map>
#include <memory>

namespace fcs {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
int fail(int code, const std::string& msg) {
  set_error(msg);
  return code;
}

namespace {

std::mutex g_dev_mu;
std::map<int, std::unique_ptr<DeviceTables>> g_tables;
int g_default_device = 0;

struct ForkSet {
  hipStream_t side[kForkStreams - 1] = {};
  hipEvent_t fork = nullptr;
  hipEvent_t join[kForkStreams - 1] = {};
};

// Side streams and events of a launch stream on the current device, created
// on the stream's first fork and kept for the process (a stream costs about
// 3.5 ms to create on gfx950, so they are made once per launch stream, not
// per call or per thread).  A launch stream is used by one call at a time:
// a pooled session's stream by its lease holder, a caller's stream by the
// caller.
auto* g_fork_sets = new std::map<std::pair<int, hipStream_t>, ForkSet>();  // outlives static teardown

ForkSet* fork_set(hipStream_t s) {
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(g_fork_mu);
  auto* sets = g_fork_sets;
  auto it = sets->find({device, s});
  if (it != sets->end()) return &it->second;
  ForkSet f;
  if (hipEventCreateWithFlags(&f.fork, hipEventDisableTiming) != hipSuccess) return nullptr;
  for (int i = 0; i < kForkStreams - 1; ++i)
    if (hipStreamCreateWithFlags(&f.side[i], hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&f.join[i], hipEventDisableTiming) != hipSuccess)
      return nullptr;
  return &((*sets)[{device, s}] = f);
}

}  // namespace

std::mutex g_fork_mu;

int check_device(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(FCS_ERR_DEVICE, "[E::fcship] no HIP device available (libfcship requires an MI355X / gfx950)");
  if (device < 0 || device >= n) return fail(FCS_ERR_INVALID, "[E::fcship] device ordinal out of range");
  return FCS_OK;
}

int device_ok(int device) { return check_device(device); }
int default_device() { return g_default_device; }

int fork_streams(hipStream_t s, hipStream_t (&fs)[kForkStreams]) {
  ForkSet* f = fork_set(s);
  if (!f) return fail(FCS_ERR_DEVICE, "[E::fcship] cannot create side streams");
  FCS_HIP_CHECK(hipEventRecord(f->fork, s));
  fs[0] = s;
  for (int i = 0; i < kForkStreams - 1; ++i) {
    FCS_HIP_CHECK(hipStreamWaitEvent(f->side[i], f->fork, 0));
    fs[i + 1] = f->side[i];
  }
  return FCS_OK;
}

int join_streams(hipStream_t s, const hipStream_t (&fs)[kForkStreams]) {
  ForkSet* f = fork_set(s);
  if (!f) return fail(FCS_ERR_DEVICE, "[E::fcship] cannot create side streams");
  for (int i = 0; i < kForkStreams - 1; ++i) {
    FCS_HIP_CHECK(hipEventRecord(f->join[i], fs[i + 1]));
    FCS_HIP_CHECK(hipStreamWaitEvent(s, f->join[i], 0));
  }
  return FCS_OK;
}

int sessions_per_device(int kind) {
  static const int n[2] = {[] {
                             const char* e = std::getenv("FCS_SESSIONS_PER_DEVICE");
                             const int v = e && *e ? std::atoi(e) : 4;
                             return std::max(1, std::min(v, 64));
                           }(),
                           [] {
                             const char* e = std::getenv("FCS_BGZF_SESSIONS_PER_DEVICE");
                             const int v = e && *e ? std::atoi(e) : 16;
                             return std::max(1, std::min(v, 64));
                           }()};
  return n[kind];
}

struct SessionPool {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<Session*> all, idle;  // never freed: the pools outlive static teardown and the HIP runtime
  int creating = 0;
  bool releasing = false;  // fcs_device_release is resetting the device: leases are refused
};

namespace {

SessionPool& session_pool(int device, int kind = kComputeSession) {
  static std::mutex mu;
  static auto* pools = new std::map<std::pair<int, int>, SessionPool*>();
  std::lock_guard<std::mutex> lk(mu);
  SessionPool*& p = (*pools)[{device, kind}];
  if (!p) p = new SessionPool();
  return *p;
}

// A new session on `device` (the current device), or null.
Session* create_session(int device, int kind = kComputeSession) {
  auto* S = new Session();
  S->device = device;
  if (hipStreamCreateWithFlags(&S->s, hipStreamNonBlocking) != hipSuccess ||
      (kind == kComputeSession && !fork_set(S->s))) {
    delete S;  // a failed stream is not reused; nothing else was created
    return nullptr;
  }
  // FCS_SESSION_PRESIZE_MB (default 24, 0 = off): a compute session starts
  // with staging of that size and a PairHMM plan for FCS_SESSION_PRESIZE_PAIRS
  // (default 120000), so the first passes of a run (an htc shard's pass is
  // ~17 MB and ~90K pairs on the 30x panel) do not allocate pinned and device
  // memory while other threads' passes are in flight; sessions are created by
  // the warm-up, off the callers' path.  A failed presize only leaves the
  // session to grow on demand.
  static const size_t presize = (size_t)env_int("FCS_SESSION_PRESIZE_MB", 24) << 20;
  static const int64_t presize_pairs = env_int("FCS_SESSION_PRESIZE_PAIRS", 120000);
  if (kind == kComputeSession && presize > 0) {
    (void)(S->ensure_host(presize) || S->ensure_dev(presize) || (presize_pairs > 0 && S->ensure_phmm(presize_pairs)));
  }
  return S;
}

// Grows the pool of `device` (the current device) to n idle-or-busy sessions.
int prefill_sessions(int device, int n) {
  SessionPool& P = session_pool(device);
  n = std::min(n, sessions_per_device());
  for (;;) {
    {
      std::lock_guard<std::mutex> lk(P.mu);
      if (P.releasing) return fail(FCS_ERR_INVALID, "[E::fcship] the device is being released");
      if ((int)P.all.size() + P.creating >= n) return FCS_OK;
      ++P.creating;
    }
    Session* S = create_session(device);
    {
      std::lock_guard<std::mutex> lk(P.mu);
      --P.creating;
      if (S) P.all.push_back(S), P.idle.push_back(S);
    }
    P.cv.notify_one();
    if (!S) return fail(FCS_ERR_DEVICE, "[E::fcship] stream creation failed");
  }
}

}  // namespace

int SessionLease::acquire(int device, int kind) {
  release();
  SessionPool& P = session_pool(device, kind);
  std::unique_lock<std::mutex> lk(P.mu);
  for (;;) {
    if (P.releasing) return fail(FCS_ERR_INVALID, "[E::fcship] the device is being released");
    if (!P.idle.empty()) {
      s_ = P.idle.back();
      P.idle.pop_back();
      pool_ = &P;
      return FCS_OK;
    }
    if ((int)P.all.size() + P.creating < sessions_per_device(kind)) break;
    P.cv.wait(lk);
  }
  ++P.creating;
  lk.unlock();
  Session* S = create_session(device, kind);
  lk.lock();
  --P.creating;
  if (!S) {
    P.cv.notify_one();
    return fail(FCS_ERR_DEVICE, "[E::fcship] stream creation failed");
  }
  P.all.push_back(S);
  s_ = S;
  pool_ = &P;
  return FCS_OK;
}

bool SessionLease::try_acquire(int device, int kind, size_t host_bytes, size_t dev_bytes) {
  release();
  SessionPool& P = session_pool(device, kind);
  std::lock_guard<std::mutex> lk(P.mu);
  if (P.releasing) return false;
  for (size_t i = 0; i < P.idle.size(); ++i) {
    Session* S = P.idle[i];
    if (S->host_cap >= host_bytes && S->dev_cap >= dev_bytes) {
      P.idle.erase(P.idle.begin() + (long)i);
      s_ = S;
      pool_ = &P;
      return true;
    }
  }
  return false;
}

void SessionLease::release() {
  if (!s_) return;
  {
    std::lock_guard<std::mutex> lk(pool_->mu);
    pool_->idle.push_back(s_);
  }
  pool_->cv.notify_one();
  s_ = nullptr;
  pool_ = nullptr;
}

int Session::ensure_dev(size_t bytes) {
  if (bytes <= dev_cap) return FCS_OK;
  FCS_HIP_CHECK(hipStreamSynchronize(s));
  if (dev) (void)hipFree(dev);
  dev = nullptr;
  dev_cap = 0;
  const size_t cap = grown(bytes, dev_cap);
  if (hipMalloc(&dev, cap) != hipSuccess) {
    dev = nullptr;
    return fail(FCS_ERR_NOMEM, "[E::fcship] hipMalloc of " + std::to_string(cap) + " bytes failed");
  }
  dev_cap = cap;
  return FCS_OK;
}

int Session::ensure_host(size_t bytes) {
  if (bytes <= host_cap) return FCS_OK;
  FCS_HIP_CHECK(hipStreamSynchronize(s));
  if (host) (void)hipHostFree(host);
  host = nullptr;
  host_cap = 0;
  const size_t cap = grown(bytes, host_cap);
  if (hipHostMalloc(&host, cap, hipHostMallocDefault) != hipSuccess) {
    host = nullptr;
    return fail(FCS_ERR_NOMEM, "[E::fcship] hipHostMalloc of " + std::to_string(cap) + " bytes failed");
  }
  host_cap = cap;
  return FCS_OK;
}

int get_device_tables(int device, DeviceTables** out) {
  std::lock_guard<std::mutex> lk(g_dev_mu);
  auto& slot = g_tables[device];
  if (!slot) slot.reset(new DeviceTables());
  DeviceTables& t = *slot;
  if (!t.ready) {
    FCS_SET_DEVICE((device));
    const size_t n = 3 * 128 + kMmEntries;
    std::vector<float> hf(n);
    std::vector<double> hd(n);
    build_phmm_tables_f(hf.data(), hf.data() + 128, hf.data() + 256, hf.data() + 384);
    build_phmm_tables_d(hd.data(), hd.data() + 128, hd.data() + 256, hd.data() + 384);
    FCS_HIP_CHECK(hipMalloc(&t.f_tabs, n * sizeof(float)));
    FCS_HIP_CHECK(hipMalloc(&t.d_tabs, n * sizeof(double)));
    FCS_HIP_CHECK(hipMemcpy(t.f_tabs, hf.data(), n * sizeof(float), hipMemcpyHostToDevice));
    FCS_HIP_CHECK(hipMemcpy(t.d_tabs, hd.data(), n * sizeof(double), hipMemcpyHostToDevice));
    t.tf = PhmmTables<float>{t.f_tabs, t.f_tabs + 128, t.f_tabs + 256, t.f_tabs + 384, ldexpf(1.f, 120),
                             log10f(ldexpf(1.f, 120))};
    t.td = PhmmTables<double>{t.d_tabs, t.d_tabs + 128, t.d_tabs + 256, t.d_tabs + 384, ldexp(1.0, 1020),
                              log10(ldexp(1.0, 1020))};
    t.ready = true;
  }
  *out = &t;
  return FCS_OK;
}

int call_session_acquire(int device, size_t host_bytes, size_t dev_bytes, CallSession& c) {
  auto lease = std::make_unique<SessionLease>();
  int rc = lease->acquire(device);
  if (rc) return rc;
  Session* S = lease->get();
  if ((rc = S->ensure_host(host_bytes)) || (rc = S->ensure_dev(dev_bytes))) return rc;
  c.s = S->s;
  c.host = S->hbase();
  c.dev = S->dbase();
  c.lease = lease.release();
  return FCS_OK;
}

void call_session_release(CallSession& c) {
  if (!c.lease) return;
  (void)hipStreamSynchronize(c.s);  // StreamDrain's reason: the next holder refills the pinned staging
  delete static_cast<SessionLease*>(c.lease);
  c = CallSession();
}

}  // namespace fcs

using namespace fcs;

extern "C" {

const char* fcs_last_error(void) { return g_last_error.c_str(); }
const char* fcs_version(void) { return "fcship 0.1.0 (gfx950)"; }

int fcs_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int fcs_set_default_device(int32_t device) {
  int rc = check_device(device);
  if (rc) return rc;
  g_default_device = device;
  return FCS_OK;
}

int fcs_stream_release(int32_t device, void* stream) {
  int rc = check_device(device);
  if (rc) return rc;
  FCS_SET_DEVICE((device));
  ForkSet f;
  BswWorkspace ws;
  bool have_fork = false;
  {
    std::lock_guard<std::mutex> lk(g_fork_mu);
    ws = bsw_take_stream(device, (hipStream_t)stream);
    auto it = g_fork_sets->find({device, (hipStream_t)stream});
    if (it != g_fork_sets->end()) {
      f = it->second;
      g_fork_sets->erase(it);
      have_fork = true;
    }
  }
  if (ws.keys_in) {
    (void)hipStreamSynchronize((hipStream_t)stream);
    ws_free(ws);
  }
  if (!have_fork) return FCS_OK;
  // tear down every side stream and event (best effort), then report the
  // first failure: an early return would leak the rest unreachably
  hipError_t first = hipSuccess;
  const char* what = nullptr;
  auto note = [&](hipError_t e, const char* w) {
    if (e != hipSuccess && first == hipSuccess) first = e, what = w;
  };
  for (int i = 0; i < kForkStreams - 1; ++i) {
    note(hipStreamSynchronize(f.side[i]), "hipStreamSynchronize");
    note(hipStreamDestroy(f.side[i]), "hipStreamDestroy");
    note(hipEventDestroy(f.join[i]), "hipEventDestroy");
  }
  note(hipEventDestroy(f.fork), "hipEventDestroy");
  if (first != hipSuccess)
    return fail(FCS_ERR_DEVICE, std::string("[E::fcs_stream_release] ") + what + ": " + hipGetErrorString(first));
  return FCS_OK;
}

int fcs_device_warmup(int32_t device, int32_t sessions) {
  int rc = check_device(device);
  if (rc) return rc;
  // a 1x1 PairHMM call: runtime, code objects, GKL tables and one session
  static const uint8_t b[1] = {'A'}, q[1] = {30}, g[1] = {10}, iq[1] = {45};
  const fcs_phmm_read r{b, q, iq, iq, g, 1};
  const fcs_phmm_hap h{b, 1};
  double out = 0;
  fcs_phmm_opts o;
  fcs_phmm_opts_default(&o);
  o.device = device;
  if ((rc = fcs_phmm_compute(&r, 1, &h, 1, &out, &o))) return rc;
  FCS_SET_DEVICE((device));
  return prefill_sessions(device, sessions <= 0 ? sessions_per_device() : sessions);
}

int fcs_bgzf_warmup(int32_t device, int32_t sessions, int64_t arena_bytes) {
  if (sessions < 0 || arena_bytes < 0) return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_warmup] bad arguments");
  int rc = check_device(device);
  if (rc) return rc;
  FCS_SET_DEVICE((device));
  sessions = std::min(sessions, sessions_per_device(kInflateSession));
  // lease them all at once (so each is a different session), size, return
  std::vector<std::unique_ptr<SessionLease>> held;
  for (int k = 0; k < sessions; ++k) {
    auto L = std::make_unique<SessionLease>();
    if ((rc = L->acquire(device, kInflateSession))) return rc;
    if ((rc = (*L)->ensure_host((size_t)arena_bytes)) || (rc = (*L)->ensure_dev((size_t)arena_bytes))) return rc;
    held.push_back(std::move(L));
  }
  return FCS_OK;
}

int fcs_device_release(int32_t device) {
  int rc = check_device(device);
  if (rc) return rc;
  SessionPool& C = session_pool(device, kComputeSession);
  SessionPool& I = session_pool(device, kInflateSession);
  {
    // one critical section from the idle check to the drop: a lease between
    // them would hold a session the reset destroys.  `releasing` then refuses
    // every lease (FCS_ERR_INVALID, or busy for a try) until the reset is done.
    std::scoped_lock lk(C.mu, I.mu);
    for (SessionPool* P : {&C, &I})
      if (P->releasing || P->creating || P->idle.size() != P->all.size())
        return fail(FCS_ERR_INVALID, "[E::fcs_device_release] a call on this device is still running");
    // the handles die with the reset below: the pools, fork sets and tables
    // are dropped (not destroyed one by one) and made again on the next call
    for (SessionPool* P : {&C, &I}) {
      P->all.clear();
      P->idle.clear();
      P->releasing = true;
    }
  }
  struct Reopen {  // leases are accepted again once the reset has returned (or failed)
    SessionPool *c, *i;
    ~Reopen() {
      std::scoped_lock lk(c->mu, i->mu);
      c->releasing = i->releasing = false;
    }
  } reopen{&C, &I};
  {
    std::lock_guard<std::mutex> lk(g_fork_mu);
    for (auto it = g_fork_sets->begin(); it != g_fork_sets->end();)
      it = it->first.first == device ? g_fork_sets->erase(it) : std::next(it);
    bsw_drop_device(device);
  }
  fmd_drop_device(device);  // FMD-index handles of this device lose their memory below
  {
    std::lock_guard<std::mutex> lk(g_dev_mu);
    auto it = g_tables.find(device);
    if (it != g_tables.end()) {
      (void)it->second.release();
      g_tables.erase(it);
    }
  }
  FCS_SET_DEVICE((device));
  FCS_HIP_CHECK(hipDeviceSynchronize());
  FCS_HIP_CHECK(hipDeviceReset());
  return FCS_OK;
}

int fcs_abi_symbol_count(void) { return 61; }

}  // extern "C"
