// Depth of coverage (DESIGN §2 [EXT] "Depth of coverage", §4.11): GATK 3's
// DepthOfCoverage with COUNT_READS, one sample (the reference's depth command
// runs GATK per shard and merges the text: src/worker-depth.cpp,
// src/workers/DepthWorker.cpp, src/workers/DepthCombineWorker.cpp).  [EXT]
// parity is unpinned: GATK is not vendored.
//
// This file states the rules with plain loops over a flat batch and a window
// (include/fcsdp.h): the oracle of the device path and the path taken without
// it.  The command around it is in depth_run.cpp.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "fcsdp.h"

namespace fcsg {

// Adds the batch's depths over the window to depth[w.len].  Throws
// failedCommand, with nothing added, on offsets out of order, a counted record
// whose CIGAR does not cover its bases or an aligned base beyond the contig.
// threads > 1: slices of the batch are counted into private arrays over their
// own spans, which are then summed.
void depth_count_host(const fcsdp_batch& b, const fcsdp_params& prm, const fcsdp_window& w, uint32_t* depth,
                      int threads = 1);

// fcsdp_stats on the host: adds to hist[501] and long_hist[n_long][501], writes summary[n_pieces].
void depth_stats_host(const uint32_t* depth, const uint64_t* bitmap, int64_t len, const fcsdp_piece* pieces,
                      int64_t n_pieces, int32_t n_long, uint64_t* hist, uint64_t* long_hist, fcsdp_summary* summary,
                      int threads = 1);

// The reported granular quantile k / 4 (k = 1, 2, 3) of a 501-bin histogram: max(bin, 1), and 1 without loci.
uint32_t depth_quantile(const uint64_t* hist, int k);

// One row of <out>.sample_interval_summary.
struct DepthInterval {
  std::string name;  // contig:start-end, 1-based inclusive, or contig:pos
  uint64_t total = 0, loci = 0, above = 0;
  uint32_t q1 = 1, median = 1, q3 = 1;
};

std::string depth_mean_text(uint64_t total, uint64_t loci);          // %.2f, or NaN
std::string depth_percent_text(uint64_t above, uint64_t loci);       // %.1f, or NaN
std::string depth_locus_header(const std::string& sample);
// The lines of the participating loci among window loci [begin, end): <contig>:<pos1>\t<d>\t<d>.00\t<d>
void depth_locus_lines(const std::string& contig, int64_t window_start, const uint32_t* depth, const uint64_t* bitmap,
                       int64_t begin, int64_t end, std::string& out);
std::string depth_sample_summary_text(const std::string& sample, const uint64_t* hist, uint64_t total);
std::string depth_sample_statistics_text(const std::string& sample, const uint64_t* hist);
std::string depth_cumulative_counts_text(const uint64_t* hist);
std::string depth_cumulative_proportions_text(const std::string& sample, const uint64_t* hist);
std::string depth_interval_summary_text(const std::string& sample, const std::vector<DepthInterval>& rows);
std::string depth_interval_statistics_text(const std::vector<DepthInterval>& rows);

}  // namespace fcsg
