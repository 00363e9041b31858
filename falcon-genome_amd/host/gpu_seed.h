// The aligner's seeding on the GPU (bwa.gpu_seed): the SMEMs of
// a chunk's reads from one fcs_fmd_collect call and the suffix-array lookups
// of their sampled occurrences from one fcs_fmd_locate call, on a device copy
// of the FmdIndex.  Every SMEM and position is the one FmdIndex::collect /
// locate gives; reads and rows the device hands back (more SMEMs than slots, an
// LF walk past the step cap) are done on the host.  The entry points are
// looked up in the loaded libfcship at run time, so a library without them
// (the tests' CPU mock) leaves seeding on the host.
//
// Fused mode (bwa.gpu_seed_fused, with a libfcship that has fcs_fmd_seed): one
// call per chunk that orders, expands and locates on the device and returns
// one compacted SMEM array and one position array with per-read offsets; the
// batch keeps them flat, and chain_read reads each read's range in place.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "fcship.h"
#include "fmindex.h"

namespace fcsg {

struct SeedParams {
  int min_len = 19, split_len = 28, split_width = 10;  // bwa -k, (int)(k * 1.5 + .499), 10
  int64_t max_mem_intv = 20;                           // bwa -y
  int max_occ = 500;                                   // bwa -c: occurrences located per SMEM (sampled beyond)
  int max_mems = FCS_FMD_MAX_MEMS_DEFAULT;             // device output slots per read
  // fused mode: the device's LF-step cap (0: 32 * sa_intv) and the capacities
  // of the first call (0: max(16 n, 4096) SMEMs and max(64 n, 65536) rows)
  int max_steps = 0;
  int64_t mem_cap = 0, row_cap = 0;
};

static_assert(sizeof(BiInterval) == sizeof(fcs_fmd_mem) && sizeof(BiInterval) == 32 &&
                  offsetof(BiInterval, k) == offsetof(fcs_fmd_mem, k) && offsetof(BiInterval, l) == offsetof(fcs_fmd_mem, l) &&
                  offsetof(BiInterval, s) == offsetof(fcs_fmd_mem, s) && offsetof(BiInterval, qb) == offsetof(fcs_fmd_mem, qb) &&
                  offsetof(BiInterval, qe) == offsetof(fcs_fmd_mem, qe),
              "the fused call's SMEM array is read as BiInterval without a copy");

// The fcs_fmd_* entry points were found in the loaded libfcship.
bool gpu_seed_available();
// fcs_fmd_seed was found too: the fused mode can run.
bool gpu_seed_fused_available();

// Device copies of one FmdIndex, one per device, made on first use and shared
// (read-only) by every thread that seeds on that device.
class FmdDeviceCopies {
 public:
  explicit FmdDeviceCopies(const FmdIndex& fmd);
  ~FmdDeviceCopies();
  FmdDeviceCopies(const FmdDeviceCopies&) = delete;
  FmdDeviceCopies& operator=(const FmdDeviceCopies&) = delete;
  fcs_fmd_index* get(int device);  // throws when the copy cannot be made
  void release();                  // destroys the copies (made again on the next get)

 private:
  const FmdIndex& fmd_;
  std::mutex mu_;
  std::map<int, fcs_fmd_index*> dev_;
};
// Destroys the device copies of every live FmdDeviceCopies: before
// fcs_device_release resets a device (gpu.release_early).
void release_fmd_device_copies();

// Text position -> (contig, forward-strand offset of the match start, strand):
// FmdIndex::locate's conversion of SA values.
class TextMap {
 public:
  TextMap(const std::vector<std::vector<uint8_t>>& contigs);
  void locate(int64_t p, int len, int& contig, int64_t& off, bool& rev) const;

 private:
  std::vector<int64_t> cstart_;
  int64_t flen_ = 0;
};

// Uninitialised storage for an output of a capacity chosen before its size is
// known: only the pages the call writes are ever touched.
template <class T>
class RawBuf {
 public:
  RawBuf() = default;
  RawBuf(const RawBuf&) = delete;
  RawBuf& operator=(const RawBuf&) = delete;
  ~RawBuf() { std::free(p_); }
  void reset(size_t n) {
    std::free(p_);
    p_ = n ? static_cast<T*>(std::malloc(n * sizeof(T))) : nullptr;
    if (n && !p_) throw std::bad_alloc();
  }
  T* data() { return p_; }
  const T* data() const { return p_; }

 private:
  T* p_ = nullptr;
};

struct SeedBatch {
  std::vector<std::vector<BiInterval>> mems;  // per read, FmdIndex::collect's list
  // per read: SA[m.k + j] of the occurrences seed_read samples (SMEM by SMEM,
  // j = 0, step, 2 step, .. with step = s / max_occ beyond max_occ, at most max_occ)
  std::vector<std::vector<int64_t>> pos;
  // fused mode: every read's SMEMs and positions in one array each, read r's
  // at [mem_off[r], mem_off[r + 1]) and [row_off[r], row_off[r + 1]) (empty for
  // a read the device handed back: that one is in mems[r], located by chain_read)
  bool fused = false;
  RawBuf<BiInterval> flat_mems;
  RawBuf<int64_t> flat_pos;
  std::vector<int64_t> mem_off, row_off;
  std::vector<int32_t> overflow;
  int64_t retries = 0;     // fused calls repeated with larger capacities
  // read r's SMEM list and its positions (null: chain_read locates on the host index)
  const BiInterval* mems_of(size_t r) const {
    return fused && !overflow[r] ? flat_mems.data() + mem_off[r] : mems[r].data();
  }
  size_t n_mems_of(size_t r) const {
    return fused && !overflow[r] ? (size_t)(mem_off[r + 1] - mem_off[r]) : mems[r].size();
  }
  const int64_t* pos_of(size_t r) const {
    return fused ? (overflow[r] ? nullptr : flat_pos.data() + row_off[r]) : pos[r].data();
  }
  int64_t host_reads = 0;  // reads collected on the host (overflow)
  int64_t host_rows = 0;   // rows located on the host (step cap)
  int64_t rows = 0;
  double collect_seconds = 0, locate_seconds = 0;
};

// q[r] / qlen[r]: the reads as codes 0..4.  gpu_seed_available() must hold;
// fused: the one-call mode (gpu_seed_fused_available() must hold).
void gpu_seed_batch(const FmdIndex& fmd, fcs_fmd_index* dev, const uint8_t* const* q, const int* qlen, size_t n,
                    const SeedParams& P, int threads, SeedBatch& out, bool fused = false);

}  // namespace fcsg
