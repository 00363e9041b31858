#include "bam_stream.h"

#include <algorithm>
#include <set>
#include <sstream>

#include "common.h"
#include "fasta.h"
#include "intervals.h"

namespace fcsg {

std::vector<std::string> bam_inputs(const std::string& input) {
  if (is_regular_file(input)) return {input};
  if (!is_directory(input)) throw fileNotFound(input);
  std::vector<std::string> names = list_dir(input, ".bam");
  std::sort(names.begin(), names.end());
  std::vector<std::string> out;
  for (const std::string& n : names) out.push_back(n.find('/') == std::string::npos ? input + "/" + n : n);
  if (out.empty()) throw fileNotFound(input + "/*.bam");
  return out;
}

BamStream::BamStream(const std::string& input, bool check_sorted)
    : bams_(bam_inputs(input)), reader_(new BamReader(bams_[0])), check_sorted_(check_sorted), header_(reader_->header()) {}

size_t BamStream::read(std::vector<BamRecord>& out, size_t n, const std::function<bool(const BamRecord&)>& keep) {
  size_t got = 0;
  BamRecord r;
  while (got < n && !eof_) {
    if (!reader_->next(r)) {
      if (++file_ >= bams_.size()) eof_ = true;
      else reader_.reset(new BamReader(bams_[file_]));
      continue;
    }
    const auto key = key_of(r.ref_id, r.pos);
    if (check_sorted_ && key < last_key_) {
      auto where = [&](int64_t ref, int64_t pos) {
        return (ref >= 0 && ref < (int64_t)header_.names.size() ? header_.names[(size_t)ref] : std::string("*")) + ":" +
               std::to_string(pos + 1);
      };
      throw invalidParam("the input is not coordinate-sorted: record " + r.name + " at " + where(r.ref_id, r.pos) +
                         " follows one at " + where(last_key_.first, last_key_.second));
    }
    last_key_ = key;
    if (keep && !keep(r)) continue;
    out.push_back(std::move(r));
    ++got;
  }
  return got;
}

std::string RgLine::get(const char* tag) const {
  for (auto f = fields.rbegin(); f != fields.rend(); ++f)
    if (f->first == tag) return f->second;
  return "";
}

std::vector<RgLine> rg_lines(const BamHeader& h) {
  std::vector<RgLine> out;
  std::istringstream ss(h.text);
  for (std::string line; std::getline(ss, line);) {
    if (line.rfind("@RG", 0) != 0) continue;
    out.emplace_back();
    for (size_t p = 0; p < line.size();) {
      const size_t e = std::min(line.find('\t', p), line.size());
      if (e >= p + 3 && line[p + 2] == ':') out.back().fields.emplace_back(line.substr(p, 2), line.substr(p + 3, e - p - 3));
      p = e + 1;
    }
  }
  return out;
}

std::string single_sample(const BamHeader& h, const std::string& command) {
  std::set<std::string> sm;
  for (const RgLine& rg : rg_lines(h))
    for (const auto& f : rg.fields)
      if (f.first == "SM" && !f.second.empty()) sm.insert(f.second);
  if (sm.empty()) throw invalidParam("the BAM header names no sample (no @RG line with SM)");
  if (sm.size() > 1) {
    std::string all;
    for (const std::string& s : sm) all += (all.empty() ? "" : ", ") + s;
    throw invalidParam("the BAM header names " + std::to_string(sm.size()) + " samples (" + all + "); " + command + " takes one");
  }
  return *sm.begin();
}

std::vector<std::string> header_contigs(const std::string& fasta, const BamHeader& h, bool check_lengths) {
  Reference ref = load_fasta(fasta);
  std::vector<std::string> out(h.names.size());
  for (size_t k = 0; k < h.names.size(); ++k) {
    const int c = ref.index(h.names[k]);
    if (c < 0) throw invalidParam("contig " + h.names[k] + " of the BAM header is not in " + fasta);
    out[k] = std::move(ref.contigs[(size_t)c].seq);
    if (check_lengths && (int64_t)out[k].size() != h.lengths[k])
      throw invalidParam("contig " + h.names[k] + " has " + std::to_string(h.lengths[k]) + " bases in the BAM header and " +
                         std::to_string(out[k].size()) + " in " + fasta);
  }
  return out;
}

std::vector<GenomeInterval> merged_intervals(const std::string& path, const BamHeader& h) {
  std::vector<GenomeInterval> iv;
  if (path.empty()) {
    for (size_t c = 0; c < h.names.size(); ++c) iv.push_back({(int32_t)c, 0, h.lengths[c]});
    return iv;
  }
  for (const Interval& i : read_regions(path)) {
    const int c = h.ref_index(i.chrom);
    if (c < 0) throw invalidParam("contig " + i.chrom + " of " + path + " is not in the BAM header");
    const int64_t s = std::max<int64_t>(i.lb - 1, 0), e = std::min<int64_t>(i.ub, h.lengths[(size_t)c]);
    if (s >= e) throw invalidParam("interval " + i.chrom + ":" + std::to_string(i.lb) + "-" + std::to_string(i.ub) + " of " + path +
                                   " is empty or beyond its contig");
    iv.push_back({(int32_t)c, s, e});
  }
  std::sort(iv.begin(), iv.end(), [](const GenomeInterval& a, const GenomeInterval& b) { return a.ref != b.ref ? a.ref < b.ref : a.start < b.start; });
  std::vector<GenomeInterval> out;
  for (const GenomeInterval& i : iv) {
    if (!out.empty() && out.back().ref == i.ref && i.start <= out.back().end) out.back().end = std::max(out.back().end, i.end);
    else out.push_back(i);
  }
  return out;
}

std::vector<GenomeWindow> cut_windows(const std::vector<GenomeInterval>& iv, const std::vector<int64_t>& contig_lengths,
                                      int64_t window_bp) {
  std::vector<GenomeWindow> out;
  for (size_t a = 0; a < iv.size();) {
    size_t b = a;
    while (b < iv.size() && iv[b].ref == iv[a].ref) ++b;
    size_t k = a;
    for (int64_t s = iv[a].start; s < iv[b - 1].end; s += window_bp) {
      GenomeWindow w{iv[a].ref, s, std::min(window_bp, iv[b - 1].end - s), contig_lengths[(size_t)iv[a].ref], {}};
      const int64_t e = s + w.len;
      while (k < b && iv[k].end <= s) ++k;
      for (size_t j = k; j < b && iv[j].start < e; ++j)
        w.parts.push_back({j, std::max(iv[j].start, s) - s, std::min(iv[j].end, e) - s});
      if (!w.parts.empty()) out.push_back(std::move(w));
    }
    a = b;
  }
  return out;
}

}  // namespace fcsg
