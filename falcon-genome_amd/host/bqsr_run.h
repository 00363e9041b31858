// The baserecal / printreads / bqsr commands around the rules of bqsr.h: the
// reference and known sites, the streaming BAM passes, the flattening, and the
// device calls (include/fcsbq.h) or the host path.
#pragma once

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace fcsg {

struct BqsrJob {
  std::string ref;                  // FASTA
  std::string input;                // a BAM, or a directory of part-*.bam
  std::vector<std::string> known;   // VCF or VCF.gz (baserecal, bqsr)
  std::string intervals;            // -L: only records overlapping these are read ("" = all)
  std::string report;               // written by baserecal (and bqsr when not empty), read by printreads
  std::string output;               // the recalibrated BAM (printreads, bqsr)
  int device = -1;                  // < 0: the host path
};

struct BqsrStats {
  int64_t records = 0, counted = 0, observations = 0, errors = 0, recalibrated = 0;
  int64_t known_sites = 0, known_skipped = 0;  // VCF records loaded / on contigs the reference lacks
  double seconds = 0;
  bool on_device = false;
};

// The loaded libfcship has the fcsbq_* entry points (the tests' CPU mock has not).
bool gpu_bqsr_available();

// The known-sites reader: the data lines of a plain or bgzipped VCF, one call each (also indel_run.cpp's -K).
void known_sites_lines(const std::string& path, const std::function<void(const std::string&)>& take);

BqsrStats baserecal_run(const BqsrJob& job);   // input -> report
BqsrStats printreads_run(const BqsrJob& job);  // report + input -> output
BqsrStats bqsr_run(const BqsrJob& job);        // both, the tables kept in memory

}  // namespace fcsg
