// The depth command around the rules of depth.h: the sorted stream, the sample,
// the reference and the windows come from bam_stream.h; here a chunk of records
// is counted into every window it overlaps by the device calls
// (include/fcsdp.h) or the host path, a window the stream has passed is
// summarised, and the seven text files are written.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace fcsg {

struct DepthJob {
  std::string ref;        // FASTA
  std::string input;      // a coordinate-sorted BAM, or a directory whose part BAMs in name order form one
  std::string output;     // <output> and <output>.sample_*
  std::string intervals;  // -L: BED or interval list ("" = every header contig)
  bool omit_base = false, omit_intervals = false, omit_summary = false;  // -b, -v, -s
  int device = -1;        // < 0: the host path
};

struct DepthRunStats {
  std::string sample;
  int64_t records = 0, windows = 0, intervals = 0;
  uint64_t loci = 0, total = 0;
  double seconds = 0;
  bool on_device = false;
};

// The loaded libfcship has the fcsdp_* entry points (the tests' CPU mock has not).
bool gpu_depth_available();

// The files the job writes, in the order of DESIGN §2.
std::vector<std::string> depth_output_files(const DepthJob& job);

DepthRunStats depth_run(const DepthJob& job);

}  // namespace fcsg
