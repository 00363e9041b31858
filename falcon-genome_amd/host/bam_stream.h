// What the runners of the commands that walk a BAM's records (markdup_run.cpp,
// bqsr_run.cpp, depth_run.cpp, ug_run.cpp) share on the way in: the part BAMs
// of an input, their records as one stream with the coordinate-order check,
// the header's @RG lines and its single sample, the reference in the header's
// contig order, and -L cut into windows of the genome.  What a runner does with
// a chunk of records and with a window stays in the runner.
#pragma once

#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "bam.h"

namespace fcsg {

// The input's BAM files: the file itself, or a directory's *.bam in name order.
std::vector<std::string> bam_inputs(const std::string& input);

// The sort key of a record: unmapped records without a contig come last.
inline std::pair<int64_t, int64_t> key_of(int32_t ref_id, int32_t pos) {
  return {ref_id < 0 ? (int64_t)INT32_MAX + 1 : ref_id, pos};
}

// The records of bam_inputs(input) as one stream under the first file's header.
class BamStream {
 public:
  // check_sorted: a record whose key_of lies before its predecessor's is an invalidParam.
  BamStream(const std::string& input, bool check_sorted);
  const BamHeader& header() const { return header_; }
  // Appends up to n more records that `keep` accepts (all, without one) to out; the number appended.
  // The order check sees the records `keep` drops as well.
  size_t read(std::vector<BamRecord>& out, size_t n, const std::function<bool(const BamRecord&)>& keep = {});
  bool eof() const { return eof_; }  // a read has come to the end of the last file

 private:
  std::vector<std::string> bams_;
  std::unique_ptr<BamReader> reader_;
  size_t file_ = 0;
  bool check_sorted_, eof_ = false;
  BamHeader header_;
  std::pair<int64_t, int64_t> last_key_{-1, -1};
};

// One @RG line of the header: its TAG:value fields in order.
struct RgLine {
  std::vector<std::pair<std::string, std::string>> fields;
  std::string get(const char* tag) const;  // the last value of tag, "" without one
};
std::vector<RgLine> rg_lines(const BamHeader& h);
// The single distinct non-empty SM of the @RG lines; invalidParam without one or with several.
std::string single_sample(const BamHeader& h, const std::string& command);

// The FASTA's sequences in the header's contig order (moved out of the loaded file, not copied); invalidParam
// for a header contig the FASTA lacks and, with check_lengths, for one whose length differs.
std::vector<std::string> header_contigs(const std::string& fasta, const BamHeader& h, bool check_lengths);

struct GenomeInterval {
  int32_t ref;
  int64_t start, end;  // 0-based half-open
};
// -L sorted by header contig order with overlapping and abutting intervals merged, or one interval per contig.
std::vector<GenomeInterval> merged_intervals(const std::string& path, const BamHeader& h);

// A window of at most window_bp loci of one contig (the fields of fcsdp_window / fcsug_window) with the
// parts of the intervals that lie in it.
struct GenomeWindow {
  struct Part {
    size_t interval;
    int64_t start, end;  // window offsets
  };
  int32_t ref_id;
  int64_t start, len, contig_len;
  std::vector<Part> parts;
  template <class W>  // as the device call's window
  W as() const {
    W w;
    w.ref_id = ref_id, w.reserved = 0, w.start = start, w.len = len, w.contig_len = contig_len;
    return w;
  }
};
// Windows from each contig's first interval start to its last interval end; those without a part are left out.
std::vector<GenomeWindow> cut_windows(const std::vector<GenomeInterval>& intervals, const std::vector<int64_t>& contig_lengths,
                                      int64_t window_bp);

}  // namespace fcsg
