// gvcf.h: the header check, the line parser and the per-contig stream.
#include "gvcf.h"

#include <algorithm>
#include <charconv>
#include <string_view>

#include "common.h"
#include "fcsjg.h"

namespace fcsg {

namespace {

bool ends_with(const std::string& s, const char* suffix) {
  const size_t n = std::char_traits<char>::length(suffix);
  return s.size() >= n && s.compare(s.size() - n, n, suffix) == 0;
}

std::vector<std::string_view> split(std::string_view s, char sep) {
  std::vector<std::string_view> out;
  size_t p = 0;
  for (;;) {
    const size_t e = s.find(sep, p);
    if (e == std::string_view::npos) {
      out.push_back(s.substr(p));
      return out;
    }
    out.push_back(s.substr(p, e - p));
    p = e + 1;
  }
}

bool to_int(std::string_view s, int64_t& v) {
  if (s.empty()) return false;
  const auto r = std::from_chars(s.data(), s.data() + s.size(), v);
  return r.ec == std::errc() && r.ptr == s.data() + s.size();
}

}  // namespace

void GvcfContig::clear() {
  beg.clear(), end.clear(), dp.clear(), pl.clear(), kind.clear(), call.clear(), ref.clear(), alt.clear();
}

std::vector<std::string> gvcf_files(const std::string& dir) {
  std::vector<std::string> out;
  for (const std::string& f : list_dir(dir))
    if (ends_with(f, ".gvcf.gz") || ends_with(f, ".g.vcf.gz") || ends_with(f, ".gvcf") || ends_with(f, ".g.vcf")) out.push_back(f);
  return out;
}

void GvcfReader::refuse(const std::string& what) const {
  throw failedCommand("[E::joint] " + path_ + ":" + std::to_string(line_no_) + ": " + what);
}

bool GvcfReader::next_line() {
  const bool ok = gz_ ? gz_->getline(line_) : (bool)std::getline(txt_, line_);
  if (ok) ++line_no_;
  return ok;
}

GvcfReader::GvcfReader(const std::string& path, const std::vector<std::pair<std::string, int64_t>>& contigs)
    : path_(path), contigs_(contigs) {
  if (ends_with(path, ".gz")) {
    gz_.reset(new BgzfReader(path));
  } else {
    txt_.open(path);
    if (!txt_) throw fileNotFound(path);
  }
  size_t seen = 0;
  bool columns = false;
  while (next_line()) {
    if (line_.rfind("##contig=<ID=", 0) == 0) {
      const size_t c = line_.find(",length="), e = line_.rfind('>');
      int64_t len = -1;
      if (c == std::string::npos || e == std::string::npos || e < c || !to_int(std::string_view(line_).substr(c + 8, e - c - 8), len))
        refuse("a ##contig line without ID and length");
      const std::string name = line_.substr(13, c - 13);
      if (seen >= contigs_.size() || contigs_[seen].first != name || contigs_[seen].second != len)
        refuse("contig " + name + " of " + std::to_string(len) + " bases is not contig " + std::to_string(seen + 1) + " of the reference");
      ++seen;
    } else if (line_.rfind("#CHROM", 0) == 0) {
      const auto f = split(line_, '\t');
      if (f.size() != 10) refuse("the #CHROM line names " + std::to_string(f.size() < 9 ? 0 : f.size() - 9) + " samples, not one");
      sample_ = std::string(f[9]);
      columns = true;
      break;
    } else if (line_.rfind("##", 0) != 0) {
      refuse("a line before the #CHROM line that is no ## line");
    }
  }
  if (!columns) refuse("no #CHROM line");
  if (seen != contigs_.size())
    refuse("the header has " + std::to_string(seen) + " ##contig lines, the reference " + std::to_string(contigs_.size()) + " contigs");
  if (sample_.empty()) refuse("an empty sample name");
}

void GvcfReader::read_contig(int ci, GvcfContig& out) {
  out.clear();
  last_call_pos_ = -1;
  for (;;) {
    if (!have_) {
      if (!next_line()) return;
      if (line_.empty()) refuse("an empty line");
      const size_t t = line_.find('\t');
      const std::string_view chrom = std::string_view(line_).substr(0, t);
      cur_ = -1;
      for (size_t k = 0; k < contigs_.size(); ++k)
        if (chrom == contigs_[k].first) cur_ = (int)k;
      if (cur_ < 0) refuse("contig " + std::string(chrom) + " is not in the reference");
      if (cur_ < last_ci_) refuse("contig " + std::string(chrom) + " follows " + contigs_[(size_t)last_ci_].first + ": unsorted contigs");
      have_ = true;
    }
    if (cur_ < ci) refuse("a record of contig " + contigs_[(size_t)cur_].first + " after that contig was read");
    if (cur_ > ci) return;
    parse(out);
    have_ = false;
  }
}

void GvcfReader::finish() {
  if (have_ || next_line()) refuse("a record beyond the reference's last contig");
}

void GvcfReader::parse(GvcfContig& out) {
  const auto f = split(line_, '\t');
  if (f.size() != 10) refuse(std::to_string(f.size()) + " columns, not 10");
  int64_t pos = 0;
  if (!to_int(f[1], pos) || pos < 1 || pos > contigs_[(size_t)cur_].second) refuse("POS " + std::string(f[1]));
  if (cur_ == last_ci_ && pos < last_pos_)
    refuse("POS " + std::to_string(pos) + " follows " + std::to_string(last_pos_) + ": unsorted positions");
  last_ci_ = cur_, last_pos_ = pos;
  const std::string_view ref = f[3];
  if (ref.empty() || ref.find('<') != std::string_view::npos) refuse("REF " + std::string(ref));
  const auto alts = split(f[4], ',');
  if (alts.back() != "<NON_REF>") refuse("ALT " + std::string(f[4]) + " does not end in <NON_REF>");
  if (alts.size() > 2) refuse("ALT " + std::string(f[4]) + " has more than one allele beside <NON_REF>");
  const bool block = alts.size() == 1;
  if (!block && (alts[0].empty() || alts[0].find('<') != std::string_view::npos || alts[0] == "*" || alts[0] == "."))
    refuse("ALT " + std::string(f[4]) + ": a symbolic or missing allele");
  int64_t end = pos - 1 + (int64_t)ref.size();
  if (block) {
    int64_t e = -1;
    for (const std::string_view kv : split(f[7], ';'))
      if (kv.substr(0, 4) == "END=" && !to_int(kv.substr(4), e)) refuse("INFO " + std::string(f[7]));
    if (e < 0) refuse("a <NON_REF> block without END=");
    if (e < pos || e > contigs_[(size_t)cur_].second) refuse("END=" + std::to_string(e) + " at POS " + std::to_string(pos));
    end = e;
  }
  const auto keys = split(f[8], ':'), vals = split(f[9], ':');
  int kgt = -1, kdp = -1, kpl = -1;
  for (size_t k = 0; k < keys.size(); ++k) {
    if (keys[k] == "GT") kgt = (int)k;
    if (keys[k] == "DP") kdp = (int)k;
    if (keys[k] == "PL") kpl = (int)k;
  }
  if (kgt < 0 || (size_t)kgt >= vals.size()) refuse("no GT");
  {
    const std::string_view gt = vals[(size_t)kgt];
    size_t seps = 0;
    for (char ch : gt) seps += ch == '/' || ch == '|';
    if (seps != 1) refuse("GT " + std::string(gt) + ": ploidy is not 2");
  }
  if (kpl < 0 || (size_t)kpl >= vals.size() || vals[(size_t)kpl] == ".") refuse("no PL");
  const auto pls = split(vals[(size_t)kpl], ',');
  if (pls.size() != (block ? 3u : 6u))
    refuse(std::to_string(pls.size()) + " PLs, a " + (block ? "block has 3" : "call has 6"));
  int64_t dp = 0;
  if (kdp >= 0 && (size_t)kdp < vals.size() && vals[(size_t)kdp] != "." && (!to_int(vals[(size_t)kdp], dp) || dp < 0 || dp > INT32_MAX))
    refuse("DP " + std::string(vals[(size_t)kdp]));
  int32_t pl[6] = {0, 0, 0, 0, 0, 0};
  int64_t clamped = 0;
  for (size_t k = 0; k < pls.size(); ++k) {
    int64_t v = 0;
    if (!to_int(pls[k], v) || v < 0) refuse("PL " + std::string(pls[k]));
    if (v > FCSJG_PL_MAX) v = FCSJG_PL_MAX, ++clamped;
    pl[k] = (int32_t)v;
  }
  if (!block) {
    if (pos == last_call_pos_) {
      ++ignored_;
      return;
    }
    last_call_pos_ = pos;
  }
  clamped_ += clamped;
  out.beg.push_back((int32_t)(pos - 1)), out.end.push_back((int32_t)end), out.dp.push_back((int32_t)dp);
  out.kind.push_back(block ? FCSJG_KIND_BLOCK : FCSJG_KIND_CALL);
  out.pl.insert(out.pl.end(), pl, pl + 6);
  if (block) {
    out.call.push_back(-1);
  } else {
    out.call.push_back((int32_t)out.ref.size());
    out.ref.emplace_back(ref), out.alt.emplace_back(alts[0]);
  }
}

}  // namespace fcsg
