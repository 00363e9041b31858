// What the runners of the record-walking commands (markdup_run.cpp,
// bqsr_run.cpp, depth_run.cpp, ug_run.cpp) share on the way to the device:
// records flattened into the arrays of an fcsdp_batch / fcsug_batch /
// fcsbq_batch (the same field names), the host pool's width, the device entry
// points looked up in whatever libfcship the process loaded, the choice between
// the device and the host path, and a device call's failure as failedCommand.
// How the records get here is bam_stream.h.
#pragma once

#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "bam.h"
#include "common.h"
#include "fcship.h"

namespace fcsg {

inline int host_threads() { return (int)std::min<unsigned>(host_cpus(), 16); }

// A device entry point of the loaded libfcship, or null when it has none of that name.
template <class Fn>
Fn device_entry(const char* name) {
  return reinterpret_cast<Fn>(dlsym(RTLD_DEFAULT, name));
}
#define FCSG_DEVICE_ENTRY(fn) ::fcsg::device_entry<decltype(&fn)>(#fn)

using LastErrorFn = const char* (*)();
inline LastErrorFn last_error_entry() {
  static const LastErrorFn f = device_entry<LastErrorFn>("fcs_last_error");
  return f;
}

// The device a job runs on, or -1 for the host: job_device when the library
// has the entry points, else -1 with log_line on stderr, once per process.
inline int device_or_host(int job_device, bool available, const char* log_line) {
  if (job_device < 0) return -1;
  if (available) return job_device;
  static std::mutex mu;
  static std::set<std::string> said;
  std::lock_guard<std::mutex> lk(mu);
  if (said.insert(log_line).second) std::fputs(log_line, stderr);
  return -1;
}

// A device call's status: anything but FCS_OK is a failedCommand that names the command, the call and the library's error.
inline void device_check(int rc, const char* command, const char* call) {
  if (rc != FCS_OK) throw failedCommand(std::string("[E::fcs-genome ") + command + "] " + call + ": " + last_error_entry()());
}

// Records as the arrays of a batch; absent qualities are 0xff bytes.
struct FlatRecords {
  std::vector<uint16_t> flag;
  std::vector<int32_t> ref_id, pos;
  std::vector<uint8_t> mapq, absent, qual, bases;  // bases: filled on request
  std::vector<uint32_t> cigar;
  std::vector<int64_t> cigar_off, base_off;
  size_t size() const { return flag.size(); }
  // Records [lo, hi) as a batch that keeps the offsets of the whole.
  template <class Batch>
  Batch view(size_t lo, size_t hi) const {
    Batch b{};
    b.n = (int64_t)(hi - lo);
    b.flag = flag.data() + lo, b.ref_id = ref_id.data() + lo, b.pos = pos.data() + lo, b.mapq = mapq.data() + lo;
    b.cigar = cigar.data(), b.cigar_off = cigar_off.data() + lo, b.n_cigar = (int64_t)cigar.size();
    b.bases = bases.empty() ? nullptr : bases.data(), b.qual = qual.data(), b.base_off = base_off.data() + lo;
    b.n_bases = (int64_t)qual.size();
    b.qual_absent = absent.data() + lo;
    return b;
  }
};

// The first n records, or with `order` the records order[0 .. n), into f.
inline void flatten(const std::vector<BamRecord>& recs, size_t n, bool with_bases, FlatRecords& f,
                    const uint32_t* order = nullptr) {
  auto rec = [&](size_t k) -> const BamRecord& { return recs[order ? order[k] : k]; };
  f.flag.resize(n), f.ref_id.resize(n), f.pos.resize(n), f.mapq.resize(n), f.absent.resize(n);
  f.cigar_off.assign(n + 1, 0), f.base_off.assign(n + 1, 0);
  for (size_t k = 0; k < n; ++k) {
    const BamRecord& r = rec(k);
    f.flag[k] = r.flag, f.ref_id[k] = r.ref_id, f.pos[k] = r.pos, f.mapq[k] = r.mapq;
    f.absent[k] = r.qual.size() != r.seq.size() || r.seq.empty();
    f.cigar_off[k + 1] = f.cigar_off[k] + (int64_t)r.cigar.size();
    f.base_off[k + 1] = f.base_off[k] + (int64_t)r.seq.size();
  }
  f.cigar.resize((size_t)f.cigar_off[n]);
  f.qual.resize((size_t)f.base_off[n]);
  f.bases.resize(with_bases ? (size_t)f.base_off[n] : 0);
  parallel_for(n, host_threads(), [&](size_t k) {
    const BamRecord& r = rec(k);
    if (!r.cigar.empty()) std::memcpy(f.cigar.data() + f.cigar_off[k], r.cigar.data(), 4 * r.cigar.size());
    if (!r.seq.empty()) {
      if (with_bases) std::memcpy(f.bases.data() + f.base_off[k], r.seq.data(), r.seq.size());
      if (f.absent[k]) std::memset(f.qual.data() + f.base_off[k], 0xff, r.seq.size());
      else std::memcpy(f.qual.data() + f.base_off[k], r.qual.data(), r.seq.size());
    }
  });
}

}  // namespace fcsg
