// The depth command around the rules of depth.h: the sample, the reference and
// the intervals, the streamed BAM chunks cut over windows of the genome, the
// device calls (include/fcsdp.h) or the host path, and the seven text files.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace fcsg {

struct BamHeader;

// What the commands that stream one sorted BAM over windows of the genome share (depth, ug).
// The input BAM, or the part BAMs of a directory in name order.
std::vector<std::string> sorted_bam_inputs(const std::string& input);
// The single distinct SM of the header's @RG lines; invalidParam without one or with several.
std::string single_sample(const BamHeader& h, const std::string& command);
struct GenomeInterval {
  int32_t ref;
  int64_t start, end;  // 0-based half-open
};
// -L sorted by header contig order with overlapping and abutting intervals merged, or one interval per contig.
std::vector<GenomeInterval> merged_intervals(const std::string& path, const BamHeader& h);

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
