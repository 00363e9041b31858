// The depth command (depth_run.h): the BAM streams in chunks of
// depth.chunk_records; the genome is walked in windows of at most
// depth.window_bp loci over the contigs that hold intervals; a chunk's records
// are given to every window they overlap and clipped to it; a window is
// summarised and written once the stream has passed its end.
#include "depth_run.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>

#include "bam_stream.h"
#include "common.h"
#include "config.h"
#include "depth.h"
#include "fcship.h"
#include "flat_batch.h"

namespace fcsg {

namespace {

struct DpApi {
  decltype(&fcsdp_count) count = FCSG_DEVICE_ENTRY(fcsdp_count);
  decltype(&fcsdp_stats) stats = FCSG_DEVICE_ENTRY(fcsdp_stats);
};

const DpApi& dp_api() {
  static const DpApi A;
  return A;
}

// max_end[k]: the running maximum of the ends of records [.., k] on their contig.
void running_max_end(const std::vector<BamRecord>& recs, std::vector<int64_t>& max_end) {
  max_end.resize(recs.size());
  for (size_t k = 0; k < recs.size(); ++k) {
    const int64_t end = recs[k].end();
    max_end[k] = k > 0 && recs[k - 1].ref_id == recs[k].ref_id ? std::max(max_end[k - 1], end) : end;
  }
}

class Run {
 public:
  explicit Run(const DepthJob& job)
      : job_(job),
        device_(device_or_host(job.device, gpu_depth_available(),
                               "[fcs-genome depth] depth.gpu: the loaded libfcship has no fcsdp_count entry point; "
                               "depths are counted on the host\n")),
        in_(job.input, true),
        header_(in_.header()) {
    st_.sample = single_sample(header_, "depth");
    contigs_ = header_contigs(job.ref, header_, true);
    Config& cf = conf();
    prm_.min_mapq = cf.get_int("depth.min_mapq"), prm_.max_mapq = cf.get_int("depth.max_mapq");
    prm_.min_baseq = cf.get_int("depth.min_baseq"), prm_.max_baseq = cf.get_int("depth.max_baseq");
    prm_.include_deletions = cf.get_bool("depth.include_deletions");
    if (prm_.min_mapq > prm_.max_mapq || prm_.min_baseq > prm_.max_baseq)
      throw invalidParam("depth.min_mapq / max_mapq or depth.min_baseq / max_baseq: a lower bound above its upper bound");
    include_ref_n_ = cf.get_bool("depth.include_ref_n");
    chunk_ = (size_t)std::max(cf.get_int("depth.chunk_records"), 1);
    const int64_t window_bp = std::clamp<int64_t>(cf.get_int("depth.window_bp"), 1, FCSDP_WINDOW_MAX);
    intervals_ = merged_intervals(job.intervals, header_);
    windows_ = cut_windows(intervals_, header_.lengths, window_bp);
    name_rows();
    hist_.assign(FCSDP_BINS, 0);
    long_hist_.assign((size_t)FCSDP_BINS * n_long_, 0);
  }

  DepthRunStats run() {
    const uint64_t t0 = now_us();
    if (!job_.omit_base) {
      locus_.open(job_.output, std::ios::binary | std::ios::trunc);
      if (!locus_) throw failedCommand("[E::fcs-genome depth] cannot write " + job_.output);
      locus_ << depth_locus_header(st_.sample);
    }
    try {
      stream();
    } catch (...) {  // a refused run leaves no partial per-locus file
      if (!job_.omit_base) locus_.close(), remove_path(job_.output);
      throw;
    }
    st_.windows = (int64_t)windows_.size(), st_.intervals = (int64_t)intervals_.size();
    st_.total = total_;
    for (uint64_t v : hist_) st_.loci += v;
    st_.on_device = device_ >= 0;
    st_.seconds = (now_us() - t0) / 1e6;
    return st_;
  }

 private:
  // The chunks in order: each is counted into the windows it overlaps, and every window the stream has passed is finished.
  void stream() {
    std::vector<BamRecord> recs;
    FlatRecords f;
    std::vector<int64_t> max_end;
    while (recs.clear(), in_.read(recs, chunk_) > 0) {
      st_.records += (int64_t)recs.size();
      flatten(recs, recs.size(), false, f);
      running_max_end(recs, max_end);
      count_chunk(f, max_end);
      const auto last = key_of(f.ref_id.back(), f.pos.back());
      while (cur_ < windows_.size() && (windows_[cur_].ref_id < last.first ||
                                        (windows_[cur_].ref_id == last.first &&
                                         windows_[cur_].start + windows_[cur_].len <= last.second)))
        finish_window(cur_++);
      if (interrupted()) throw interruptedError();
    }
    while (cur_ < windows_.size()) finish_window(cur_++);
    write_files();
  }

  // The intervals' rows; an interval cut by a window edge or longer than a piece gets a row of long_hist.
  void name_rows() {
    rows_.resize(intervals_.size());
    long_index_.assign(intervals_.size(), -1);
    std::vector<int> n_parts(intervals_.size(), 0);
    for (const GenomeWindow& w : windows_)
      for (const GenomeWindow::Part& p : w.parts) ++n_parts[p.interval];
    for (size_t j = 0; j < intervals_.size(); ++j) {
      const GenomeInterval& i = intervals_[j];
      if (n_parts[j] > 1 || i.end - i.start > FCSDP_PIECE_MAX) long_index_[j] = n_long_++;
      rows_[j].name = header_.names[(size_t)i.ref] + ":" + std::to_string(i.start + 1) +
                      (i.end - i.start > 1 ? "-" + std::to_string(i.end) : "");
    }
  }

  // The chunk's records given to every window they overlap.
  void count_chunk(const FlatRecords& f, const std::vector<int64_t>& max_end) {
    const size_t n = f.size();
    struct Seg {
      int32_t ref;
      size_t a, b;
    };
    std::vector<Seg> segs;  // the chunk's runs of records on one contig, in contig order
    for (size_t k = 0; k < n && f.ref_id[k] >= 0; ++k) {
      if (segs.empty() || segs.back().ref != f.ref_id[k]) segs.push_back({f.ref_id[k], k, k});
      segs.back().b = k + 1;
    }
    if (segs.empty()) return;
    size_t si = 0;
    for (size_t wi = cur_; wi < windows_.size(); ++wi) {
      const fcsdp_window w = windows_[wi].as<fcsdp_window>();
      while (si < segs.size() && segs[si].ref < w.ref_id) ++si;
      if (si == segs.size()) break;
      if (segs[si].ref > w.ref_id) continue;
      const size_t a = segs[si].a, b = segs[si].b;
      if (si + 1 == segs.size() && max_end[b - 1] <= w.start) break;  // later windows hold nothing of this chunk
      // the records that start before the window's end and whose running maximum end lies beyond its start
      const size_t hi = (size_t)(std::lower_bound(f.pos.begin() + (long)a, f.pos.begin() + (long)b, w.start + w.len,
                                                  [](int32_t p, int64_t e) { return (int64_t)p < e; }) - f.pos.begin());
      const size_t lo = (size_t)(std::upper_bound(max_end.begin() + (long)a, max_end.begin() + (long)hi, w.start) -
                                 max_end.begin());
      if (lo >= hi) continue;
      std::vector<uint32_t>& depth = open_[wi];
      if (depth.empty()) depth.assign((size_t)w.len, 0);
      const fcsdp_batch view = f.view<fcsdp_batch>(lo, hi);
      if (device_ >= 0) device_check(dp_api().count(device_, &view, &prm_, &w, depth.data()), "depth", "fcsdp_count");
      else depth_count_host(view, prm_, w, depth.data(), host_threads());
    }
  }

  void finish_window(size_t wi) {
    const GenomeWindow& w = windows_[wi];
    std::vector<uint32_t> depth = std::move(open_[wi]);
    open_.erase(wi);
    if (depth.empty()) depth.assign((size_t)w.len, 0);
    const std::string& seq = contigs_[(size_t)w.ref_id];
    std::vector<uint64_t> bitmap((size_t)(w.len + 63) / 64, 0);
    std::vector<fcsdp_piece> pieces;
    for (const GenomeWindow::Part& p : w.parts) {
      for (int64_t i = p.start; i < p.end; ++i) {
        const char c = seq[(size_t)(w.start + i)];
        if (include_ref_n_ || (c != 'N' && c != 'n')) bitmap[(size_t)(i >> 6)] |= (uint64_t)1 << (i & 63);
      }
      for (int64_t s = p.start; s < p.end; s += FCSDP_PIECE_MAX)
        pieces.push_back({(int32_t)s, (int32_t)std::min<int64_t>(p.end, s + FCSDP_PIECE_MAX), long_index_[p.interval], 0});
    }
    std::vector<fcsdp_summary> sum(pieces.size());
    if (device_ >= 0) {
      device_check(dp_api().stats(device_, depth.data(), bitmap.data(), w.len, pieces.data(), (int64_t)pieces.size(),
                                  (int32_t)n_long_, hist_.data(), long_hist_.data(), sum.data()),
                   "depth", "fcsdp_stats");
    } else {
      depth_stats_host(depth.data(), bitmap.data(), w.len, pieces.data(), (int64_t)pieces.size(), (int32_t)n_long_, hist_.data(),
                       long_hist_.data(), sum.data(), host_threads());
    }
    size_t k = 0;
    for (const GenomeWindow::Part& p : w.parts)
      for (int64_t s = p.start; s < p.end; s += FCSDP_PIECE_MAX, ++k) {
        DepthInterval& row = rows_[p.interval];
        row.total += sum[k].total, row.loci += sum[k].loci, row.above += sum[k].above;
        if (long_index_[p.interval] < 0) row.q1 = sum[k].q1, row.median = sum[k].median, row.q3 = sum[k].q3;
        total_ += sum[k].total;
      }
    if (!job_.omit_base) {  // the per-locus text, formatted on the host pool piece by piece
      constexpr int64_t kGroupLoci = 4 << 20;  // loci formatted at once: their text is what is held in memory
      std::vector<std::string> text;
      for (size_t g = 0; g < pieces.size();) {
        size_t n = 0;
        for (int64_t loci = 0; g + n < pieces.size() && loci < kGroupLoci; ++n) loci += pieces[g + n].end - pieces[g + n].start;
        text.resize(std::max(text.size(), n));
        parallel_tasks(n, host_threads(), [&](size_t i) {
          text[i].clear();
          depth_locus_lines(header_.names[(size_t)w.ref_id], w.start, depth.data(), bitmap.data(), pieces[g + i].start,
                            pieces[g + i].end, text[i]);
        });
        for (size_t i = 0; i < n; ++i) locus_.write(text[i].data(), (std::streamsize)text[i].size());
        g += n;
      }
    }
  }

  void write_files() {
    for (size_t j = 0; j < intervals_.size(); ++j)
      if (long_index_[j] >= 0) {
        const uint64_t* h = long_hist_.data() + (size_t)long_index_[j] * FCSDP_BINS;
        rows_[j].q1 = depth_quantile(h, 1), rows_[j].median = depth_quantile(h, 2), rows_[j].q3 = depth_quantile(h, 3);
      }
    const std::string& out = job_.output;
    const std::string& sm = st_.sample;
    if (!job_.omit_base) {
      locus_.close();
      if (!locus_) throw failedCommand("[E::fcs-genome depth] writing " + out + " failed");
    }
    if (!job_.omit_summary) {
      write_file(out + ".sample_summary", depth_sample_summary_text(sm, hist_.data(), total_));
      write_file(out + ".sample_statistics", depth_sample_statistics_text(sm, hist_.data()));
    }
    write_file(out + ".sample_cumulative_coverage_counts", depth_cumulative_counts_text(hist_.data()));
    write_file(out + ".sample_cumulative_coverage_proportions", depth_cumulative_proportions_text(sm, hist_.data()));
    if (!job_.omit_intervals) {
      write_file(out + ".sample_interval_summary", depth_interval_summary_text(sm, rows_));
      write_file(out + ".sample_interval_statistics", depth_interval_statistics_text(rows_));
    }
  }

  const DepthJob& job_;
  int device_;
  BamStream in_;
  const BamHeader& header_;
  size_t chunk_ = 1;
  std::vector<std::string> contigs_;
  fcsdp_params prm_{};
  bool include_ref_n_ = false;
  std::vector<GenomeInterval> intervals_;
  std::vector<GenomeWindow> windows_;
  std::vector<DepthInterval> rows_;
  std::vector<int32_t> long_index_;
  size_t n_long_ = 0, cur_ = 0;
  std::map<size_t, std::vector<uint32_t>> open_;
  std::vector<uint64_t> hist_, long_hist_;
  uint64_t total_ = 0;
  std::ofstream locus_;
  DepthRunStats st_;
};

}  // namespace

bool gpu_depth_available() {
  const DpApi& a = dp_api();
  return a.count && a.stats && last_error_entry();
}

std::vector<std::string> depth_output_files(const DepthJob& job) {
  std::vector<std::string> out;
  if (!job.omit_base) out.push_back(job.output);
  if (!job.omit_summary) out.push_back(job.output + ".sample_summary"), out.push_back(job.output + ".sample_statistics");
  out.push_back(job.output + ".sample_cumulative_coverage_counts");
  out.push_back(job.output + ".sample_cumulative_coverage_proportions");
  if (!job.omit_intervals)
    out.push_back(job.output + ".sample_interval_summary"), out.push_back(job.output + ".sample_interval_statistics");
  return out;
}

DepthRunStats depth_run(const DepthJob& job) { return Run(job).run(); }

}  // namespace fcsg
