// Joint genotyping of one-sample GVCFs (DESIGN §2 [EXT] "GenotypeGVCFs, round
// 20", §4.13): the combine step that builds a contig's site table, the host
// statement of the rules the device runs (include/fcsjg.h, csrc/jg_model.h),
// and the shared step that formats records from either path's outputs.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "fcsjg.h"
#include "gvcf.h"
#include "vcf.h"

namespace fcsg {

struct JointParams {
  double stand_call_conf = 10.0, heterozygosity = 1e-3;
  int max_alt = FCSJG_ALTS_MAX;
};

// fcsjg_tables' tables for a cohort, and the threshold in units.
struct JointTables {
  std::vector<int32_t> S, LG, LP;
  int64_t min_qual = 0;
  fcsjg_model view() const { return fcsjg_model{S.data(), LG.data(), LP.data(), min_qual}; }
};
JointTables joint_tables(const JointParams& p, int n_samples);

// One contig of the cohort, samples in column order, and its sites.
struct JointContig {
  int n_samples = 0;
  std::vector<int64_t> rec_off;
  std::vector<int32_t> beg, end, dp, pl;
  std::vector<uint8_t> kind, alt;
  std::vector<int32_t> pos;
  std::vector<uint8_t> n_alt;
  std::vector<std::string> ref;   // per site
  std::vector<std::string> alts;  // per site, FCSJG_ALTS_MAX each
  int64_t cut = 0;                // call records whose ALT fell beyond max_alt
  size_t n_sites() const { return pos.size(); }
};

// The sites are the positions with a call record: REF the longest, every ALT
// extended by the REF suffix it lacks, distinct ALTs by the number of samples
// naming them (ties: first appearance in column order), the first max_alt kept.
void joint_combine(const std::vector<GvcfContig>& samples, int max_alt, JointContig& out);

// Sites [lo, hi) of a contig and the records that can be a source there, as
// arrays of their own (a call's arguments).
struct JointSlice {
  std::vector<int64_t> rec_off;
  std::vector<int32_t> beg, end, dp, pl;
  std::vector<uint8_t> kind, alt;
  int n_samples = 0;
  const int32_t* pos = nullptr;
  const uint8_t* n_alt = nullptr;
  int64_t n_sites = 0;
  fcsjg_cohort cohort() const;
  fcsjg_sites sites() const { return fcsjg_sites{n_sites, pos, n_alt}; }
};
void joint_slice(const JointContig& c, size_t lo, size_t hi, JointSlice& out);

// fcsjg_out's arrays.
struct JointOutputs {
  std::vector<int64_t> q, qual, dp, pl_off, src;
  std::vector<int32_t> mle, ac, an, pl;
  std::vector<uint8_t> kept, gt, gq;
  int64_t n_pl = 0;
  void resize(int64_t n_sites, int n_samples, int64_t max_pl);
  fcsjg_out view();
};

// The rules on `threads` threads; what fcsjg_genotype writes.  max_pl as there:
// failedCommand when the written sites have more PLs.
void joint_genotype_host(const fcsjg_cohort& c, const fcsjg_sites& s, const fcsjg_model& m, int threads, const fcsjg_out& out);

// The records of the written sites among [lo, lo + n_sites) of the contig, appended to text; their number is
// returned.  records: the cohort the call was given (src indexes its arrays).
int64_t joint_emit(const std::string& chrom, const JointContig& c, size_t lo, const fcsjg_cohort& records, int64_t n_sites, const fcsjg_out& o,
                   std::string& text);

VcfHeader joint_vcf_header(const std::vector<std::string>& samples, const std::vector<std::pair<std::string, int64_t>>& contigs);

}  // namespace fcsg
