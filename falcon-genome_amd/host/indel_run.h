// The indel command around the rules of indel.h: three passes over the sorted
// BAM (the targets; the bins, scored on the device through include/fcsir.h or
// on the host, and decided into an update table; the updates applied, the mates
// fixed and the records written back in coordinate order through a reorder heap).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace fcsg {

struct IndelJob {
  std::string ref;                 // FASTA
  std::string input;               // a coordinate-sorted BAM, or a directory of part-*.bam
  std::string output;              // one BAM
  std::string intervals;           // -L: a target is kept when it overlaps one ("" = all)
  std::vector<std::string> known;  // -K: VCF or VCF.gz
  std::string targets_out;         // --targets-out ("" = not written)
  int device = -1;                 // < 0: the host path
};

struct IndelRunStats {
  int64_t records = 0, known = 0, targets = 0, bins = 0, untouched = 0, alt_reads = 0, pairs = 0, cleaned = 0, realigned = 0, mates = 0;
  double seconds = 0;
  bool on_device = false;
};

// The loaded libfcship has the fcsir_* entry points (the tests' CPU mock has not).
bool gpu_indel_available();

IndelRunStats indel_run(const IndelJob& job);

}  // namespace fcsg
