// One-sample GVCFs in htc's dialect (DESIGN §2 [EXT] "GenotypeGVCFs, round
// 20"): <NON_REF> reference blocks (GT:DP:GQ:MIN_DP:PL, three PLs, END=) and
// one-ALT-plus-<NON_REF> call records (six PLs).  A reader streams one contig
// at a time into flat arrays; anything else in the file is refused with its
// file and line.
#pragma once

#include <cstdint>
#include <fstream>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "bgzf.h"

namespace fcsg {

// One contig of one sample.  beg is 0-based, end one past the last position.
struct GvcfContig {
  std::vector<int32_t> beg, end, dp, pl;  // pl: six per record; a block's last three are zero
  std::vector<uint8_t> kind;              // FCSJG_KIND_*
  std::vector<int32_t> call;              // the record's index into ref / alt, -1 for a block
  std::vector<std::string> ref, alt;      // of the call records
  size_t size() const { return beg.size(); }
  void clear();
};

class GvcfReader {
 public:
  // The header is read and checked: its ##contig lines are `contigs` (the
  // reference's, in its order) and its #CHROM line names one sample.
  GvcfReader(const std::string& path, const std::vector<std::pair<std::string, int64_t>>& contigs);
  const std::string& path() const { return path_; }
  const std::string& sample() const { return sample_; }
  // The records of contig ci; contigs are asked for in ascending order.
  void read_contig(int ci, GvcfContig& out);
  // After the last contig: the file holds nothing more.
  void finish();
  int64_t clamped() const { return clamped_; }  // PLs above FCSJG_PL_MAX
  int64_t ignored() const { return ignored_; }  // second and later call records at one POS

 private:
  bool next_line();
  [[noreturn]] void refuse(const std::string& what) const;
  void parse(GvcfContig& out);

  std::string path_, sample_, line_;
  std::vector<std::pair<std::string, int64_t>> contigs_;
  std::unique_ptr<BgzfReader> gz_;
  std::ifstream txt_;
  int64_t line_no_ = 0, clamped_ = 0, ignored_ = 0;
  bool have_ = false;     // line_ holds a record not yet taken
  int cur_ = -1;          // the contig of line_
  int64_t last_pos_ = 0;  // of the last record of contig last_ci_
  int last_ci_ = -1;
  int64_t last_call_pos_ = -1;
};

// The GVCFs of a directory (*.gvcf.gz, *.g.vcf.gz, *.gvcf, *.g.vcf), in name order.
std::vector<std::string> gvcf_files(const std::string& dir);

}  // namespace fcsg
