// The core the C-ABI files (session.cpp and the *_api.cpp files, which alone
// include this header) share: device checks, pooled sessions and their
// leases, and the static multi-device partition.  fcship_internal.h stays
// what the kernels see.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "fcship_internal.h"

namespace fcs {
// nothing here leaves the library: the exported set stays the C-ABI and what fcship_internal.h declares
#pragma GCC visibility push(hidden)

int check_device(int device);
int default_device();  // fcs_set_default_device's, for the bwa signature twins

// State of the synchronous host-pointer entry points on one device: a stream,
// a PairHMM plan and an SW plan grown to the largest batch seen, one device
// arena for the batch's inputs and outputs and one pinned host arena it is
// staged through (one H2D and one D2H copy per call).  After warm-up a call
// allocates nothing: no hipMalloc/hipFree (hipFree synchronises the whole
// device, so per-call frees serialised the Executor's concurrent shard
// threads on one GPU) and no null-stream operation.
//
// Sessions live in a per-device pool and a call leases one for its duration.
// Creating one costs four streams (its own and three fork side streams,
// about 14 ms together); with one session per calling thread, the htc stage's
// 16 shard threads spent 0.22 s creating 64 streams, serialised inside the
// runtime, before their first PairHMM call.  The pool holds at most
// FCS_SESSIONS_PER_DEVICE (default 4) sessions, which fcs_device_warmup
// creates ahead of time; a call finding all of them busy waits for one.
struct __attribute__((visibility("default"))) Session {  // exported since it was one file's: kept so
  int device = 0;
  hipStream_t s = nullptr;
  fcs_phmm_plan* phmm = nullptr;
  fcs_bsw_plan* bsw = nullptr;
  void* dev = nullptr;
  size_t dev_cap = 0;
  void* host = nullptr;
  size_t host_cap = 0;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // PairHMM call: start, after forward, after rescue
  hipEvent_t done = nullptr;                        // inflate sessions: a blocking-sync event (no host spin)
  int ensure_dev(size_t bytes);
  int ensure_host(size_t bytes);
  int ensure_phmm(int64_t pairs);  // phmm_api.cpp
  int ensure_bsw(int64_t tasks);   // bsw_api.cpp
  char* hbase() const { return static_cast<char*>(host); }
  char* dbase() const { return static_cast<char*>(dev); }
  template <typename T> T* d(size_t off) const { return reinterpret_cast<T*>(dbase() + off); }
  template <typename T> T* h(size_t off) const { return reinterpret_cast<T*>(hbase() + off); }
};

inline size_t grown(size_t need, size_t cap) { return std::max(need + need / 4, std::min<size_t>(2 * cap, need + (1u << 30))); }

inline int64_t env_int(const char* name, int64_t dflt) {
  const char* e = std::getenv(name);
  return e && *e ? std::max<int64_t>(0, std::atoll(e)) : dflt;
}

// Pool kinds: the compute sessions (PairHMM / SW entry points) and the BGZF
// inflate sessions, a pool of their own so the htc shards' many small inflate
// calls (one per 4 MiB of compressed BAM) neither wait behind PairHMM passes
// nor pay for fork streams they never use.
enum SessionKind : int { kComputeSession = 0, kInflateSession = 1 };
int sessions_per_device(int kind = kComputeSession);

// Synchronises a session's stream when it goes out of scope (before the
// lease returns the session to the pool): an error path must not hand the
// next holder a session whose H2D copy is still reading the pinned staging
// that holder is about to refill.
struct StreamDrain {
  hipStream_t s;
  ~StreamDrain() { (void)hipStreamSynchronize(s); }
};

struct SessionPool;

// A session of `device` (the current device) held for one call.
class SessionLease {
 public:
  SessionLease() = default;
  SessionLease(const SessionLease&) = delete;
  SessionLease& operator=(const SessionLease&) = delete;
  ~SessionLease() { release(); }
  int acquire(int device, int kind = kComputeSession);
  // An idle session whose arenas already hold `bytes` (host and device), or
  // false at once: no waiting, no session created, no arena grown.
  bool try_acquire(int device, int kind, size_t bytes) { return try_acquire(device, kind, bytes, bytes); }
  bool try_acquire(int device, int kind, size_t host_bytes, size_t dev_bytes);
  Session* operator->() const { return s_; }
  Session* get() const { return s_; }

 private:
  void release();
  Session* s_ = nullptr;
  SessionPool* pool_ = nullptr;
};

// What fcs_stream_release and fcs_device_release drop in the feature files.
// The fork sets and the per-stream SW workspaces (bsw_api.cpp) share
// g_fork_mu: bsw_take_stream and bsw_drop_device are called with it held.
extern std::mutex g_fork_mu;
BswWorkspace bsw_take_stream(int device, hipStream_t s);  // out of the map; empty when the stream had none
void bsw_drop_device(int device);                         // forgotten, not freed: a device reset follows
void ws_free(BswWorkspace& ws);
void fmd_drop_device(int device);  // fmd_api.cpp: the device's index handles lose their memory

// ------------------------------------------------------------ static partition
// contiguous slices of about equal cost, one device and one host
// thread each.  cum holds the n running costs; cuts[0 .. k] get the cut where
// the running cost first reaches j/k of the total (tests/sharding.py
// balanced_slices, its test oracle), or even counts when nothing costs.
inline void balanced_cuts(const std::vector<double>& cum, int64_t n, int32_t k, int64_t* cuts) {
  const double run = n > 0 ? cum[(size_t)n - 1] : 0;
  cuts[0] = 0;
  for (int32_t j = 1; j < k; ++j) {
    const int64_t c = run > 0 ? (int64_t)(std::lower_bound(cum.begin(), cum.end(), run * j / k) - cum.begin()) + 1
                              : n * j / k;
    cuts[j] = std::max(cuts[j - 1], std::min(c, n));
  }
  cuts[k] = n;
}

// f(j) on a thread of its own for every non-empty slice j; the code and
// message of the first slice that failed.
template <class F>
int run_slices(const std::vector<int64_t>& cuts, F&& f) {
  const size_t k = cuts.size() - 1;
  std::vector<int> rcs(k, FCS_OK);
  std::vector<std::string> errs(k);
  std::vector<std::thread> th;
  for (size_t j = 0; j < k; ++j) {
    if (cuts[j + 1] == cuts[j]) continue;
    th.emplace_back([&, j] {
      rcs[j] = f((int32_t)j);
      if (rcs[j] != FCS_OK) errs[j] = fcs_last_error();
    });
  }
  for (auto& t : th) t.join();
  for (size_t j = 0; j < k; ++j)
    if (rcs[j] != FCS_OK) return fail(rcs[j], errs[j]);
  return FCS_OK;
}

#pragma GCC visibility pop
}  // namespace fcs
