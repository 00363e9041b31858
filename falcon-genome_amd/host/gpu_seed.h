// The aligner's seeding on the GPU (bwa.gpu_seed): the SMEMs of
// a chunk's reads from one fcs_fmd_collect call and the suffix-array lookups
// of their sampled occurrences from one fcs_fmd_locate call, on a device copy
// of the FmdIndex.  Every SMEM and position is the one FmdIndex::collect /
// locate gives; reads and rows the device hands back (more SMEMs than slots, an
// LF walk past the step cap) are done on the host.  The entry points are
// looked up in the loaded libfcship at run time, so a library without them
// (the tests' CPU mock) leaves seeding on the host.
#pragma once

#include <cstdint>
#include <map>
#include <mutex>
#include <vector>

#include "fcship.h"
#include "fmindex.h"

namespace fcsg {

struct SeedParams {
  int min_len = 19, split_len = 28, split_width = 10;  // bwa -k, (int)(k * 1.5 + .499), 10
  int64_t max_mem_intv = 20;                           // bwa -y
  int max_occ = 500;                                   // bwa -c: occurrences located per SMEM (sampled beyond)
  int max_mems = FCS_FMD_MAX_MEMS_DEFAULT;             // device output slots per read
};

// The fcs_fmd_* entry points were found in the loaded libfcship.
bool gpu_seed_available();

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

struct SeedBatch {
  std::vector<std::vector<BiInterval>> mems;  // per read, FmdIndex::collect's list
  // per read: SA[m.k + j] of the occurrences seed_read samples (SMEM by SMEM,
  // j = 0, step, 2 step, .. with step = s / max_occ beyond max_occ, at most max_occ)
  std::vector<std::vector<int64_t>> pos;
  int64_t host_reads = 0;  // reads collected on the host (overflow)
  int64_t host_rows = 0;   // rows located on the host (step cap)
  int64_t rows = 0;
  double collect_seconds = 0, locate_seconds = 0;
};

// q[r] / qlen[r]: the reads as codes 0..4.  gpu_seed_available() must hold.
void gpu_seed_batch(const FmdIndex& fmd, fcs_fmd_index* dev, const uint8_t* const* q, const int* qlen, size_t n,
                    const SeedParams& P, int threads, SeedBatch& out);

}  // namespace fcsg
