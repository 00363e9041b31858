// Pileup SNP genotyping (DESIGN §2 [EXT] "UnifiedGenotyper, SNP model", §4.12):
// GATK 3's UnifiedGenotyper at its defaults (-glm SNP), one sample (the
// reference's ug command runs GATK per shard and concatenates the VCFs:
// src/worker-ug.cpp, src/workers/UGWorker.cpp).  [EXT] parity is unpinned:
// GATK is not vendored.
//
// This file states the rules with plain loops over a flat batch and a window
// (include/fcsug.h): the oracle of the device path and the path taken without
// it, and the genotype step both paths share.  The command around it is in
// ug_run.cpp.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "fcsug.h"
#include "vcf.h"

namespace fcsg {

// T[94][3] of DESIGN §2 (what fcsug_table computes, without libfcship).  Throws on pcr_error outside (0, 1).
std::vector<int64_t> ug_table(double pcr_error);

// The window's sites, ascending by offset.  Throws failedCommand on offsets out
// of order, a counted record whose CIGAR does not cover its bases or with an
// aligned base beyond the contig, and positions that decrease among the
// records of the window's contig.  threads > 1: ranges of loci, each with a
// private pileup.
std::vector<fcsug_site> ug_sites_host(const fcsug_batch& b, const fcsug_params& prm, const fcsug_window& w, const uint8_t* ref,
                                      const int64_t* table, int threads = 1);

struct UgGenotypeParams {
  double heterozygosity = 1e-3, stand_call_conf = 10.0, max_deletion_fraction = 0.05;
};

// The call of a site of the window that starts at window_start, or false: too
// many deletions, GT 0/0 or QUAL below stand_call_conf.
bool ug_genotype(const fcsug_site& s, const UgGenotypeParams& g, const std::string& chrom, int64_t window_start, VcfRecord& out);

VcfHeader ug_vcf_header(const std::string& sample, const std::vector<std::pair<std::string, int64_t>>& contigs);

}  // namespace fcsg
