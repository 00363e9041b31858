// The rules of depth.h with plain loops: the record and base filters, the
// window clip, the piece statistics and the text of the seven files.
#include "depth.h"

#include <algorithm>
#include <cstdio>
#include <mutex>

#include "common.h"

namespace fcsg {

namespace {

constexpr uint16_t kFilter = 0x4 | 0x100 | 0x200 | 0x400;
constexpr int kBins = FCSDP_BINS;

bool ref_op(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
bool aligned_op(uint32_t op) { return op == 0 || op == 7 || op == 8; }
bool read_op(uint32_t op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }

struct Rec {
  const uint32_t* cigar;
  int64_t n_ops, q0, L, pos;
  bool absent;
};

// The record's view when it is counted in this window's contig; false otherwise.
bool counted_record(const fcsdp_batch& b, const fcsdp_params& prm, const fcsdp_window& w, int64_t r, Rec& rec) {
  if (b.ref_id[r] < 0 || b.ref_id[r] != w.ref_id) return false;
  rec.n_ops = b.cigar_off[r + 1] - b.cigar_off[r];
  if (rec.n_ops <= 0 || (b.flag[r] & kFilter)) return false;
  const int32_t mapq = b.mapq[r];
  if (mapq < prm.min_mapq || mapq > prm.max_mapq) return false;
  rec.cigar = b.cigar + b.cigar_off[r];
  rec.q0 = b.base_off[r], rec.L = b.base_off[r + 1] - b.base_off[r], rec.pos = b.pos[r];
  rec.absent = b.qual_absent[r] != 0;
  return true;
}

void check_record(const Rec& rec, const fcsdp_window& w, int64_t r) {
  int64_t covered = 0, p = rec.pos;
  for (int64_t k = 0; k < rec.n_ops; ++k) {
    const uint32_t op = rec.cigar[k] & 15u;
    const int64_t len = rec.cigar[k] >> 4;
    if (read_op(op)) covered += len;
    if (aligned_op(op) && len > 0 && (p < 0 || p + len > w.contig_len))
      throw failedCommand("[E::depth] record " + std::to_string(r) + " has an aligned base beyond its contig");
    if (ref_op(op)) p += len;
  }
  if (covered != rec.L) throw failedCommand("[E::depth] the CIGAR of record " + std::to_string(r) + " does not cover its bases");
}

// Adds the record's depths to cells, which stand for positions [lo, hi).
void count_record(const fcsdp_batch& b, const fcsdp_params& prm, const Rec& rec, int64_t lo, int64_t hi, uint32_t* cells) {
  int64_t i = 0, p = rec.pos;
  for (int64_t k = 0; k < rec.n_ops; ++k) {
    const uint32_t op = rec.cigar[k] & 15u;
    const int64_t len = rec.cigar[k] >> 4;
    if (aligned_op(op)) {
      for (int64_t j = 0; j < len; ++j) {
        const int q = rec.absent ? 0 : b.qual[rec.q0 + i + j];
        if (q >= prm.min_baseq && q <= prm.max_baseq && p + j >= lo && p + j < hi) ++cells[p + j - lo];
      }
    } else if (op == 2 && prm.include_deletions) {
      for (int64_t j = std::max<int64_t>(0, lo - p); j < len && p + j < hi; ++j) ++cells[p + j - lo];
    }
    if (read_op(op)) i += len;
    if (ref_op(op)) p += len;
  }
}

std::string fmt(const char* f, double v) {
  char buf[64];
  std::snprintf(buf, sizeof buf, f, v);
  return buf;
}

std::string statistics_header() {
  std::string s = "Source_of_reads";
  for (int k = 0; k < kBins - 1; ++k) s += "\tfrom_" + std::to_string(k) + "_to_" + std::to_string(k + 1) + ")";
  return s + "\tfrom_500_to_inf\n";
}

std::string cumulative_header() {
  std::string s;
  for (int k = 0; k < kBins; ++k) s += "\tgte_" + std::to_string(k);
  return s + "\n";
}

}  // namespace

void depth_count_host(const fcsdp_batch& b, const fcsdp_params& prm, const fcsdp_window& w, uint32_t* depth, int threads) {
  if (b.n < 0 || w.len < 0 || w.start < 0 || w.start + w.len > w.contig_len)
    throw failedCommand("[E::depth] bad record count or window");
  for (int k = 0; k < 2; ++k) {
    const int64_t* off = k ? b.base_off : b.cigar_off;
    const int64_t total = k ? b.n_bases : b.n_cigar;
    if (b.n > 0 && off[0] < 0) throw failedCommand("[E::depth] offsets start below zero");
    for (int64_t r = 0; r < b.n; ++r)
      if (off[r + 1] < off[r]) throw failedCommand("[E::depth] offsets out of order at record " + std::to_string(r));
    if (b.n > 0 && off[b.n] > total) throw failedCommand("[E::depth] offsets end beyond the bytes given");
  }
  const size_t nt = (size_t)std::max<int64_t>(1, std::min<int64_t>(threads, b.n / 1024));
  auto range = [&](size_t t, int64_t& r0, int64_t& r1) {
    r0 = b.n * (int64_t)t / (int64_t)nt, r1 = b.n * (int64_t)(t + 1) / (int64_t)nt;
  };
  // every refusal first (the first record's, whatever the thread count), so that nothing is added on one
  std::vector<std::string> refused(nt);
  std::vector<std::pair<int64_t, int64_t>> span(nt, {w.start + w.len, w.start});
  parallel_tasks(nt, (int)nt, [&](size_t t) {
    int64_t r0, r1;
    range(t, r0, r1);
    try {
      Rec rec;
      for (int64_t r = r0; r < r1; ++r) {
        if (!counted_record(b, prm, w, r, rec)) continue;
        check_record(rec, w, r);
        int64_t ref_len = 0;
        for (int64_t k = 0; k < rec.n_ops; ++k)
          if (ref_op(rec.cigar[k] & 15u)) ref_len += rec.cigar[k] >> 4;
        span[t].first = std::min(span[t].first, std::max(rec.pos, w.start));
        span[t].second = std::max(span[t].second, std::min(rec.pos + ref_len, w.start + w.len));
      }
    } catch (const failedCommand& e) {
      refused[t] = e.what();
    }
  });
  for (const std::string& what : refused)
    if (!what.empty()) throw failedCommand(what);
  std::vector<std::vector<uint32_t>> part(nt);
  parallel_tasks(nt, (int)nt, [&](size_t t) {
    int64_t r0, r1;
    range(t, r0, r1);
    const int64_t lo = span[t].first, hi = span[t].second;
    if (lo >= hi) return;
    uint32_t* cells = depth + (lo - w.start);
    if (nt > 1) part[t].assign((size_t)(hi - lo), 0), cells = part[t].data();
    Rec rec;
    for (int64_t r = r0; r < r1; ++r)
      if (counted_record(b, prm, w, r, rec)) count_record(b, prm, rec, lo, hi, cells);
  });
  for (size_t t = 0; t < nt && nt > 1; ++t)
    for (size_t i = 0; i < part[t].size(); ++i) depth[(size_t)(span[t].first - w.start) + i] += part[t][i];
}

uint32_t depth_quantile(const uint64_t* hist, int k) {
  uint64_t n = 0, cum = 0;
  for (int b = 0; b < kBins; ++b) n += hist[b];
  if (n == 0) return 1;
  for (int b = 0; b < kBins; ++b) {
    cum += hist[b];
    if (4 * cum >= (uint64_t)k * n) return (uint32_t)std::max(b, 1);
  }
  return kBins - 1;
}

void depth_stats_host(const uint32_t* depth, const uint64_t* bitmap, int64_t len, const fcsdp_piece* pieces,
                      int64_t n_pieces, int32_t n_long, uint64_t* hist, uint64_t* long_hist, fcsdp_summary* summary,
                      int threads) {
  for (int64_t k = 0; k < n_pieces; ++k) {
    const fcsdp_piece& p = pieces[k];
    if (p.start < 0 || p.end < p.start || p.end > len || p.end - p.start > FCSDP_PIECE_MAX || p.long_index < -1 ||
        p.long_index >= n_long)
      throw failedCommand("[E::depth] piece " + std::to_string(k) + " is outside the window or the long table");
  }
  const size_t nt = (size_t)std::max<int64_t>(1, std::min<int64_t>(threads, n_pieces / 16));
  std::mutex mu;
  parallel_tasks(nt, (int)nt, [&](size_t t) {
    std::vector<uint64_t> mine(kBins, 0), h(kBins);
    for (int64_t k = n_pieces * (int64_t)t / (int64_t)nt; k < n_pieces * (int64_t)(t + 1) / (int64_t)nt; ++k) {
      const fcsdp_piece& p = pieces[k];
      std::fill(h.begin(), h.end(), 0);
      fcsdp_summary s{};
      for (int64_t i = p.start; i < p.end; ++i) {
        if (!((bitmap[i >> 6] >> (i & 63)) & 1u)) continue;
        const uint32_t d = depth[i];
        ++h[std::min<uint32_t>(d, kBins - 1)];
        s.total += d, ++s.loci, s.above += d >= FCSDP_ABOVE;
      }
      if (p.long_index < 0) {
        s.q1 = depth_quantile(h.data(), 1), s.median = depth_quantile(h.data(), 2), s.q3 = depth_quantile(h.data(), 3);
      } else {
        std::lock_guard<std::mutex> lk(mu);
        for (int bin = 0; bin < kBins; ++bin) long_hist[(size_t)p.long_index * kBins + bin] += h[bin];
      }
      for (int bin = 0; bin < kBins; ++bin) mine[bin] += h[bin];
      summary[k] = s;
    }
    std::lock_guard<std::mutex> lk(mu);
    for (int bin = 0; bin < kBins; ++bin) hist[bin] += mine[bin];
  });
}

std::string depth_mean_text(uint64_t total, uint64_t loci) {
  return loci ? fmt("%.2f", (double)total / (double)loci) : "NaN";
}

std::string depth_percent_text(uint64_t above, uint64_t loci) {
  return loci ? fmt("%.1f", 100.0 * (double)above / (double)loci) : "NaN";
}

std::string depth_locus_header(const std::string& sample) {
  return "Locus\tTotal_Depth\tAverage_Depth_sample\tDepth_for_" + sample + "\n";
}

void depth_locus_lines(const std::string& contig, int64_t window_start, const uint32_t* depth, const uint64_t* bitmap,
                       int64_t begin, int64_t end, std::string& out) {
  char buf[96];
  for (int64_t i = begin; i < end; ++i) {
    if (!((bitmap[i >> 6] >> (i & 63)) & 1u)) continue;
    const int n = std::snprintf(buf, sizeof buf, ":%lld\t%u\t%u.00\t%u\n", (long long)(window_start + i + 1), depth[i], depth[i],
                                depth[i]);
    out += contig;
    out.append(buf, (size_t)n);
  }
}

std::string depth_sample_summary_text(const std::string& sample, const uint64_t* hist, uint64_t total) {
  uint64_t n = 0, above = 0;
  for (int b = 0; b < kBins; ++b) n += hist[b], above += b >= FCSDP_ABOVE ? hist[b] : 0;
  const std::string mean = depth_mean_text(total, n);
  return "sample_id\ttotal\tmean\tgranular_third_quartile\tgranular_median\tgranular_first_quartile\t%_bases_above_15\n" +
         sample + "\t" + std::to_string(total) + "\t" + mean + "\t" + std::to_string(depth_quantile(hist, 3)) + "\t" +
         std::to_string(depth_quantile(hist, 2)) + "\t" + std::to_string(depth_quantile(hist, 1)) + "\t" +
         depth_percent_text(above, n) + "\nTotal\t" + std::to_string(total) + "\t" + mean + "\tN/A\tN/A\tN/A\n";
}

std::string depth_sample_statistics_text(const std::string& sample, const uint64_t* hist) {
  std::string s = statistics_header() + "sample_" + sample;
  for (int b = 0; b < kBins; ++b) s += "\t" + std::to_string(hist[b]);
  return s + "\n";
}

std::string depth_cumulative_counts_text(const uint64_t* hist) {
  std::vector<uint64_t> c(kBins + 1, 0);
  for (int b = kBins - 1; b >= 0; --b) c[b] = c[b + 1] + hist[b];
  std::string s = cumulative_header() + "NSamples_1";
  for (int b = 0; b < kBins; ++b) s += "\t" + std::to_string(c[b]);
  return s + "\n";
}

std::string depth_cumulative_proportions_text(const std::string& sample, const uint64_t* hist) {
  std::vector<uint64_t> c(kBins + 1, 0);
  for (int b = kBins - 1; b >= 0; --b) c[b] = c[b + 1] + hist[b];
  std::string s = cumulative_header() + sample;
  for (int b = 0; b < kBins; ++b) s += "\t" + (c[0] ? fmt("%.2f", (double)c[b] / (double)c[0]) : std::string("NaN"));
  return s + "\n";
}

std::string depth_interval_summary_text(const std::string& sample, const std::vector<DepthInterval>& rows) {
  std::string s = "Target\ttotal_coverage\taverage_coverage\t" + sample + "_total_cvg\t" + sample + "_mean_cvg\t" + sample +
                  "_granular_Q1\t" + sample + "_granular_median\t" + sample + "_granular_Q3\t" + sample + "_%_above_15\n";
  for (const DepthInterval& r : rows) {
    const std::string total = std::to_string(r.total), mean = depth_mean_text(r.total, r.loci);
    s += r.name + "\t" + total + "\t" + mean + "\t" + total + "\t" + mean + "\t" + std::to_string(r.q1) + "\t" +
         std::to_string(r.median) + "\t" + std::to_string(r.q3) + "\t" + depth_percent_text(r.above, r.loci) + "\n";
  }
  return s;
}

std::string depth_interval_statistics_text(const std::vector<DepthInterval>& rows) {
  std::vector<uint64_t> cells(kBins, 0);
  for (const DepthInterval& r : rows) ++cells[r.loci ? (size_t)std::min<uint64_t>(r.total / r.loci, kBins - 1) : 0];
  std::string s = statistics_header() + "At_least_1_samples";
  for (int b = 0; b < kBins; ++b) s += "\t" + std::to_string(cells[b]);
  return s + "\n";
}

}  // namespace fcsg
