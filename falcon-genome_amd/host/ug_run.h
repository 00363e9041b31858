// The ug command around the rules of ug.h: the sample, the reference and the
// intervals, the streamed BAM chunks gathered per window of the genome, the
// device call (include/fcsug.h) or the host path, the shared genotype step and
// the VCF with its bgzipped copy and tabix index.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace fcsg {

struct UgJob {
  std::string ref;        // FASTA
  std::string input;      // a coordinate-sorted BAM, or a directory whose part BAMs in name order form one
  std::string output;     // <output>, <output>.gz and <output>.gz.tbi
  std::string intervals;  // -L: BED or interval list ("" = every header contig)
  int device = -1;        // < 0: the host path
};

struct UgRunStats {
  std::string sample;
  int64_t records = 0, windows = 0, intervals = 0, sites = 0, calls = 0;
  double seconds = 0;
  bool on_device = false;
};

// The loaded libfcship has the fcsug_* entry points (the tests' CPU mock has not).
bool gpu_ug_available();

// The files the job writes.
std::vector<std::string> ug_output_files(const UgJob& job);

UgRunStats ug_run(const UgJob& job);

}  // namespace fcsg
