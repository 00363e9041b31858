// Base quality recalibration, the host statement of the rules (bqsr.h).
#include "bqsr.h"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <sstream>

#include "common.h"

namespace fcsg {

namespace {

constexpr uint16_t kFlagPaired = 0x1, kFlagReverse = 0x10, kFlagRead2 = 0x80;
constexpr uint16_t kFlagFilter = 0x4 | 0x100 | 0x200 | 0x400;
constexpr int kMaxQe = 60;
constexpr int64_t kMaxObs = 2147483646;  // 2^31 - 2

int code(uint8_t b) {
  switch (b & 0xDF) {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    case 'T': return 3;
  }
  return -1;
}

bool counted(const fcsbq_batch& b, int64_t r) {
  return b.rg[r] >= 0 && !b.qual_absent[r] && !(b.flag[r] & kFlagFilter) && b.mapq[r] != 0 && b.mapq[r] != 255;
}
bool applied(const fcsbq_batch& b, int64_t r) { return b.rg[r] >= 0 && !b.qual_absent[r]; }

[[noreturn]] void refuse(const std::string& what) { throw failedCommand("[E::fcsg] bqsr: " + what); }

void check_offsets(const fcsbq_batch& b, int32_t n_rg) {
  if (b.n < 0) refuse("negative record count");
  if (n_rg < 0 || n_rg > FCSBQ_MAX_RG) refuse("bad read group count " + std::to_string(n_rg));
  if (b.n_bases < 0 || b.n_cigar < 0 || b.n_bases > FCSBQ_MAX_BASES) refuse("bad base or CIGAR size");
  if (b.n == 0) return;
  if (b.base_off[0] < 0 || b.cigar_off[0] < 0) refuse("offsets start below zero");
  for (int64_t r = 0; r < b.n; ++r) {
    if (b.base_off[r + 1] < b.base_off[r]) refuse("base offsets out of order at record " + std::to_string(r));
    if (b.cigar_off[r + 1] < b.cigar_off[r]) refuse("CIGAR offsets out of order at record " + std::to_string(r));
    if (b.rg[r] < -1 || b.rg[r] >= n_rg)
      refuse("read group " + std::to_string(b.rg[r]) + " of record " + std::to_string(r) + " is outside [-1, " +
             std::to_string(n_rg) + ")");
  }
  if (b.base_off[b.n] > b.n_bases || b.cigar_off[b.n] > b.n_cigar) refuse("offsets end beyond the arrays");
}

// Per read base of record r: kind 0 aligned (p its reference position), 1
// inserted (p the aligned position before the insertion), 2 soft-clipped.
struct Site {
  int kind;
  int64_t p;
};

void walk(const fcsbq_batch& b, int64_t r, std::vector<Site>& st, int64_t& lead, int64_t& trail) {
  st.clear();
  lead = trail = 0;
  bool seen = false;
  int64_t p = b.pos[r];
  for (int64_t k = b.cigar_off[r]; k < b.cigar_off[r + 1]; ++k) {
    const uint32_t op = b.cigar[k] & 15u;
    const int64_t len = b.cigar[k] >> 4;
    if (op == 0 || op == 7 || op == 8) {
      for (int64_t i = 0; i < len; ++i) st.push_back({0, p + i});
      p += len;
    } else if (op == 1) {
      for (int64_t i = 0; i < len; ++i) st.push_back({1, p - 1});
    } else if (op == 4) {
      for (int64_t i = 0; i < len; ++i) st.push_back({2, 0});
      (seen ? trail : lead) += len;
    } else if (op == 2 || op == 3) {
      p += len;
    }
    if (op == 0 || op == 1 || op == 7 || op == 8) seen = true, trail = 0;
  }
}

// Context and cycle keys of the k bases at seq / qual (the kept read in count, the whole read in apply).
void covariates(const uint8_t* seq, const uint8_t* qual, int64_t k, bool reverse, bool second, std::vector<int>& ctx,
                std::vector<int>& cyc) {
  ctx.assign((size_t)k, -1);
  cyc.assign((size_t)k, 0);
  int64_t nl = 0, nr = 0;
  while (nl < k && qual[nl] <= 2) ++nl;
  while (nr < k && qual[k - 1 - nr] <= 2) ++nr;
  for (int64_t j = 0; j < k; ++j) {
    const int64_t jp = reverse ? j + 1 : j - 1;
    int cc = -1, cp = -1;
    if (j >= nl && j < k - nr) cc = code(seq[j]);
    if (jp >= 0 && jp < k && jp >= nl && jp < k - nr) cp = code(seq[jp]);
    if (reverse) {
      cc = cc >= 0 ? 3 - cc : -1;
      cp = cp >= 0 ? 3 - cp : -1;
    }
    const int64_t cycle = reverse ? k - j : j + 1;
    ctx[(size_t)j] = cc >= 0 && cp >= 0 ? 4 * cp + cc : -1;
    cyc[(size_t)j] = (int)(2 * (cycle - 1) + (second ? 1 : 0));
  }
}

bool is_second(uint16_t flag) { return (flag & kFlagPaired) && (flag & kFlagRead2); }

// What record r adds (check_only: the refusals alone).
void count_record(const BqRefView& ref, const fcsbq_batch& b, int64_t r, bool check_only, int64_t* ctx, int64_t* cyc,
                  std::vector<Site>& st, std::vector<int>& ck, std::vector<int>& yk) {
  if (!counted(b, r)) return;
  const int64_t o = b.base_off[r], L = b.base_off[r + 1] - o;
  int64_t lead, trail;
  walk(b, r, st, lead, trail);
  const int32_t c = b.ref_id[r];
  if (check_only) {
    if ((int64_t)st.size() != L) refuse("the CIGAR of record " + std::to_string(r) + " does not cover its bases");
    if (c < 0 || c >= ref.n_ref) refuse("ref_id " + std::to_string(c) + " of record " + std::to_string(r) + " is outside the reference");
    if (L - lead - trail > FCSBQ_MAX_CYCLE)
      refuse("record " + std::to_string(r) + " has " + std::to_string(L - lead - trail) + " kept bases, more than " +
             std::to_string(FCSBQ_MAX_CYCLE));
    const int64_t clen = ref.ref_off[c + 1] - ref.ref_off[c];
    for (int64_t i = lead; i < L - trail; ++i)
      if (st[(size_t)i].kind == 0 && (st[(size_t)i].p < 0 || st[(size_t)i].p >= clen))
        refuse("record " + std::to_string(r) + " has an aligned base beyond its contig");
    return;
  }
  const int64_t k = L - lead - trail, clen = ref.ref_off[c + 1] - ref.ref_off[c];
  const uint8_t* seq = b.bases + o;
  const uint8_t* qual = b.qual + o;
  covariates(seq + lead, qual + lead, k, b.flag[r] & kFlagReverse, is_second(b.flag[r]), ck, yk);
  const int32_t rg = b.rg[r];
  for (int64_t j = 0; j < k; ++j) {
    const int64_t i = lead + j;
    const Site s = st[(size_t)i];
    const int q = qual[i], bc = code(seq[i]);
    if (s.kind == 2 || bc < 0 || q < 6 || q >= FCSBQ_NQ) continue;
    if (s.p >= 0 && s.p < clen) {
      const int64_t g = ref.ref_off[c] + s.p;
      if ((ref.known[g >> 6] >> (g & 63)) & 1) continue;
    }
    const int64_t err = s.kind == 0 && code(ref.bases[ref.ref_off[c] + s.p]) != bc ? 1 : 0;
    if (ck[(size_t)j] >= 0) {
      int64_t* cell = ctx + 2 * (((size_t)rg * FCSBQ_NQ + q) * FCSBQ_NCTX + ck[(size_t)j]);
      cell[0] += 1, cell[1] += err;
    }
    int64_t* cell = cyc + 2 * (((size_t)rg * FCSBQ_NQ + q) * FCSBQ_NCYC + yk[(size_t)j]);
    cell[0] += 1, cell[1] += err;
  }
}

double log10_prior(double qe, double prior) {
  const int d = std::min(std::abs((int)(qe - prior)), 40);
  const double v = std::log10(0.9 * std::exp(-(double)(d * d) / 0.5));
  return std::isfinite(v) ? v : -DBL_MAX;
}

}  // namespace

void bqsr_count_host(const BqRefView& ref, const fcsbq_batch& b, int32_t n_rg, int64_t* ctx, int64_t* cyc, int threads) {
  check_offsets(b, n_rg);
  const size_t nt = (size_t)std::max<int64_t>(1, std::min<int64_t>(threads, b.n / 1024));
  auto slice = [&](size_t t, bool check_only, int64_t* c, int64_t* y) {
    std::vector<Site> st;
    std::vector<int> ck, yk;
    for (int64_t r = b.n * (int64_t)t / (int64_t)nt; r < b.n * (int64_t)(t + 1) / (int64_t)nt; ++r)
      count_record(ref, b, r, check_only, c, y, st, ck, yk);
  };
  // every refusal first (the first record's, whatever the thread count), so that nothing is added on one
  std::vector<std::string> refused(nt);
  parallel_tasks(nt, (int)nt, [&](size_t t) {
    try {
      slice(t, true, nullptr, nullptr);
    } catch (const failedCommand& e) {
      refused[t] = e.what();
    }
  });
  for (const std::string& what : refused)
    if (!what.empty()) throw failedCommand(what);
  if (nt == 1) {
    slice(0, false, ctx, cyc);
    return;
  }
  const size_t nctx = 2 * kBqCtxCells * (size_t)n_rg, ncyc = 2 * kBqCycCells * (size_t)n_rg;
  std::vector<std::vector<int64_t>> part(nt);
  parallel_tasks(nt, (int)nt, [&](size_t t) {
    part[t].assign(nctx + ncyc, 0);
    slice(t, false, part[t].data(), part[t].data() + nctx);
  });
  for (size_t t = 0; t < nt; ++t) {
    for (size_t i = 0; i < nctx; ++i) ctx[i] += part[t][i];
    for (size_t i = 0; i < ncyc; ++i) cyc[i] += part[t][nctx + i];
  }
}

double bqsr_emp_q(int64_t obs, int64_t err, double prior) {
  int64_t n = obs + 2, m = err + 1;
  if (n > kMaxObs) {
    m = (int64_t)std::floor((double)m * ((double)kMaxObs / (double)n) + 0.5);
    n = kMaxObs;
  }
  const double coeff = (std::lgamma((double)n + 1.0) - std::lgamma((double)m + 1.0) - std::lgamma((double)(n - m) + 1.0)) /
                       std::log(10.0);
  int best = 0;
  double best_v = 0;
  for (int qe = 0; qe <= kMaxQe; ++qe) {
    const double p = std::pow(10.0, -(double)qe / 10.0);
    double lik = coeff + (m ? (double)m * (-(double)qe / 10.0) : 0.0);
    if (n - m) lik = lik + (1.0 - p > 0 ? (double)(n - m) * std::log10(1.0 - p) : -INFINITY);
    if (!std::isfinite(lik)) lik = -DBL_MAX;
    const double v = log10_prior((double)qe, prior) + lik;
    if (qe == 0 || v > best_v) best = qe, best_v = v;
  }
  return (double)std::min(best, FCSBQ_NQ - 1);
}

namespace {

// Per-quality (observations, errors) of read group rg: the sum of cyc over the cycles.
void quality_table(const int64_t* cyc, int32_t rg, int64_t qt[FCSBQ_NQ][2]) {
  for (int q = 0; q < FCSBQ_NQ; ++q) {
    qt[q][0] = qt[q][1] = 0;
    const int64_t* row = cyc + 2 * (((size_t)rg * FCSBQ_NQ + q) * FCSBQ_NCYC);
    for (int k = 0; k < FCSBQ_NCYC; ++k) qt[q][0] += row[2 * k], qt[q][1] += row[2 * k + 1];
  }
}

// The read group's totals and its estimated reported quality; false without observations.
bool read_group_datum(const int64_t qt[FCSBQ_NQ][2], int64_t& obs, int64_t& err, double& eps) {
  obs = err = 0;
  double exp_err = 0.0;
  for (int q = 0; q < FCSBQ_NQ; ++q) {
    obs += qt[q][0], err += qt[q][1];
    exp_err += (double)qt[q][0] * std::pow(10.0, -(double)q / 10.0);
  }
  if (obs == 0) return false;
  eps = -10.0 * std::log10(exp_err / (double)obs);
  return true;
}

}  // namespace

BqTables bqsr_finalize(int32_t n_rg, const int64_t* ctx, const int64_t* cyc) {
  BqTables t;
  t.n_rg = n_rg;
  t.base.assign((size_t)n_rg * FCSBQ_NQ, 0.0);
  t.dctx.assign((size_t)n_rg * kBqCtxCells, 0.0);
  t.dcyc.assign((size_t)n_rg * kBqCycCells, 0.0);
  for (int32_t rg = 0; rg < n_rg; ++rg) {
    int64_t qt[FCSBQ_NQ][2], obs, err;
    double eps;
    quality_table(cyc, rg, qt);
    if (!read_group_datum(qt, obs, err, eps)) {
      for (int q = 0; q < FCSBQ_NQ; ++q) t.base[(size_t)rg * FCSBQ_NQ + q] = q;
      continue;
    }
    const double prior_q = eps + (bqsr_emp_q(obs, err, eps) - eps);
    for (int q = 0; q < FCSBQ_NQ; ++q) {
      double bq = prior_q;
      if (qt[q][0] > 0) bq = prior_q + (bqsr_emp_q(qt[q][0], qt[q][1], prior_q) - prior_q);
      t.base[(size_t)rg * FCSBQ_NQ + q] = bq;
      const size_t row = (size_t)rg * FCSBQ_NQ + q;
      for (int k = 0; k < FCSBQ_NCTX; ++k) {
        const int64_t* c = ctx + 2 * (row * FCSBQ_NCTX + k);
        if (c[0] > 0) t.dctx[row * FCSBQ_NCTX + k] = bqsr_emp_q(c[0], c[1], bq) - bq;
      }
      for (int k = 0; k < FCSBQ_NCYC; ++k) {
        const int64_t* c = cyc + 2 * (row * FCSBQ_NCYC + k);
        if (c[0] > 0) t.dcyc[row * FCSBQ_NCYC + k] = bqsr_emp_q(c[0], c[1], bq) - bq;
      }
    }
  }
  return t;
}

void bqsr_apply_host(const fcsbq_batch& b, const BqTables& t, uint8_t* out_qual, int threads) {
  check_offsets(b, t.n_rg);
  for (int64_t r = 0; r < b.n; ++r)
    if (applied(b, r) && b.base_off[r + 1] - b.base_off[r] > FCSBQ_MAX_CYCLE)
      refuse("record " + std::to_string(r) + " has " + std::to_string(b.base_off[r + 1] - b.base_off[r]) +
             " bases, more than " + std::to_string(FCSBQ_MAX_CYCLE));
  const size_t nt = (size_t)std::max<int64_t>(1, std::min<int64_t>(threads, b.n / 1024));
  parallel_tasks(nt, (int)nt, [&](size_t th) {
    std::vector<int> ck, yk;
    for (int64_t r = b.n * (int64_t)th / (int64_t)nt; r < b.n * (int64_t)(th + 1) / (int64_t)nt; ++r) {
      const int64_t o = b.base_off[r], L = b.base_off[r + 1] - o;
      if (!applied(b, r)) {
        if (L) std::memcpy(out_qual + o, b.qual + o, (size_t)L);
        continue;
      }
      covariates(b.bases + o, b.qual + o, L, b.flag[r] & kFlagReverse, is_second(b.flag[r]), ck, yk);
      const size_t rg = (size_t)b.rg[r];
      for (int64_t i = 0; i < L; ++i) {
        const int q = b.qual[o + i];
        if (q < 6 || q >= FCSBQ_NQ) {
          out_qual[o + i] = (uint8_t)q;
          continue;
        }
        const size_t row = rg * FCSBQ_NQ + (size_t)q;
        const double dc = ck[(size_t)i] >= 0 ? t.dctx[row * FCSBQ_NCTX + (size_t)ck[(size_t)i]] : 0.0;
        const double v = ((t.base[row] + dc) + t.dcyc[row * FCSBQ_NCYC + (size_t)yk[(size_t)i]]) + 0.5;
        out_qual[o + i] = (uint8_t)(!(v >= 1.0) ? 1 : v > 93.0 ? 93 : (int)v);
      }
    }
  });
}

// ------------------------------------------------------------------ the report
namespace {

struct Column {
  const char* name;
  const char* fmt;  // %s flush left, everything else flush right
};

std::string table_text(const std::string& name, const std::string& desc, const std::vector<Column>& cols,
                       const std::vector<std::vector<std::string>>& rows) {
  std::vector<size_t> width(cols.size());
  for (size_t k = 0; k < cols.size(); ++k) {
    width[k] = std::strlen(cols[k].name);
    for (const auto& row : rows) width[k] = std::max(width[k], row[k].size());
  }
  std::string out = "#:GATKTable:" + std::to_string(cols.size()) + ":" + std::to_string(rows.size()) + ":";
  for (const Column& c : cols) out += std::string(c.fmt) + ":";
  out += ";\n#:GATKTable:" + name + ":" + desc + "\n";
  auto line = [&](const std::vector<std::string>& vals) {
    std::string s;
    for (size_t k = 0; k < cols.size(); ++k) {
      if (k) s += "  ";
      const std::string pad(width[k] - vals[k].size(), ' ');
      s += std::strcmp(cols[k].fmt, "%s") == 0 ? vals[k] + pad : pad + vals[k];
    }
    while (!s.empty() && s.back() == ' ') s.pop_back();
    return s + "\n";
  };
  std::vector<std::string> head;
  for (const Column& c : cols) head.push_back(c.name);
  out += line(head);
  for (const auto& row : rows) out += line(row);
  return out + "\n";
}

std::string fmt_f(const char* f, double v) {
  char buf[64];
  std::snprintf(buf, sizeof buf, f, v);
  return buf;
}

const char* const kArguments[][2] = {
    {"binary_tag_name", "null"},
    {"covariate", "ReadGroupCovariate,QualityScoreCovariate,ContextCovariate,CycleCovariate"},
    {"default_platform", "null"},
    {"deletions_default_quality", "45"},
    {"force_platform", "null"},
    {"indels_context_size", "3"},
    {"insertions_default_quality", "45"},
    {"low_quality_tail", "2"},
    {"maximum_cycle_value", "500"},
    {"mismatches_context_size", "2"},
    {"mismatches_default_quality", "-1"},
    {"no_standard_covs", "false"},
    {"quantizing_levels", "16"},
    {"recalibration_report", "null"},
    {"run_without_dbsnp", "false"},
    {"solid_nocall_strategy", "THROW_EXCEPTION"},
    {"solid_recal_mode", "SET_Q_ZERO"}};

}  // namespace

std::string bqsr_report_text(int32_t n_rg, const int64_t* ctx, const int64_t* cyc, const std::vector<std::string>& names) {
  using Rows = std::vector<std::vector<std::string>>;
  std::string text = "#:GATKReport.v1.1:5\n";
  Rows args;
  for (const auto& a : kArguments) args.push_back({a[0], a[1]});
  text += table_text("Arguments", "Recalibration argument collection values used in this run",
                     {{"Argument", "%s"}, {"Value", "%s"}}, args);
  Rows quant, t0, t1, t2;
  std::vector<int64_t> per_q(FCSBQ_NQ, 0);
  for (int32_t rg = 0; rg < n_rg; ++rg) {
    int64_t qt[FCSBQ_NQ][2];
    quality_table(cyc, rg, qt);
    for (int q = 0; q < FCSBQ_NQ; ++q) per_q[(size_t)q] += qt[q][0];
  }
  for (int q = 0; q < FCSBQ_NQ; ++q)
    quant.push_back({std::to_string(q), std::to_string(per_q[(size_t)q]), std::to_string(q)});
  text += table_text("Quantized", "Quality quantization map",
                     {{"QualityScore", "%d"}, {"Count", "%d"}, {"QuantizedScore", "%d"}}, quant);
  for (int32_t rg = 0; rg < n_rg; ++rg) {
    int64_t qt[FCSBQ_NQ][2], obs, err;
    double eps;
    quality_table(cyc, rg, qt);
    if (!read_group_datum(qt, obs, err, eps)) continue;
    const std::string& name = names[(size_t)rg];
    t0.push_back({name, "M", fmt_f("%.4f", bqsr_emp_q(obs, err, eps)), fmt_f("%.4f", eps), std::to_string(obs),
                  fmt_f("%.2f", (double)err)});
    for (int q = 0; q < FCSBQ_NQ; ++q) {
      if (qt[q][0] > 0)
        t1.push_back({name, std::to_string(q), "M", fmt_f("%.4f", bqsr_emp_q(qt[q][0], qt[q][1], (double)q)),
                      std::to_string(qt[q][0]), fmt_f("%.2f", (double)qt[q][1])});
      const size_t row = (size_t)rg * FCSBQ_NQ + (size_t)q;
      for (int k = 0; k < FCSBQ_NCTX; ++k) {
        const int64_t* c = ctx + 2 * (row * FCSBQ_NCTX + k);
        if (c[0] > 0)
          t2.push_back({name, std::to_string(q), std::string(1, "ACGT"[k / 4]) + "ACGT"[k % 4], "Context", "M",
                        fmt_f("%.4f", bqsr_emp_q(c[0], c[1], (double)q)), std::to_string(c[0]),
                        fmt_f("%.2f", (double)c[1])});
      }
      for (int k = 0; k < FCSBQ_NCYC; ++k) {
        const int64_t* c = cyc + 2 * (row * FCSBQ_NCYC + k);
        if (c[0] > 0)
          t2.push_back({name, std::to_string(q), std::to_string((k / 2 + 1) * (k % 2 ? -1 : 1)), "Cycle", "M",
                        fmt_f("%.4f", bqsr_emp_q(c[0], c[1], (double)q)), std::to_string(c[0]),
                        fmt_f("%.2f", (double)c[1])});
      }
    }
  }
  text += table_text("RecalTable0", "",
                     {{"ReadGroup", "%s"}, {"EventType", "%s"}, {"EmpiricalQuality", "%.4f"},
                      {"EstimatedQReported", "%.4f"}, {"Observations", "%d"}, {"Errors", "%.2f"}}, t0);
  text += table_text("RecalTable1", "",
                     {{"ReadGroup", "%s"}, {"QualityScore", "%d"}, {"EventType", "%s"}, {"EmpiricalQuality", "%.4f"},
                      {"Observations", "%d"}, {"Errors", "%.2f"}}, t1);
  text += table_text("RecalTable2", "",
                     {{"ReadGroup", "%s"}, {"QualityScore", "%d"}, {"CovariateValue", "%s"}, {"CovariateName", "%s"},
                      {"EventType", "%s"}, {"EmpiricalQuality", "%.4f"}, {"Observations", "%d"}, {"Errors", "%.2f"}}, t2);
  return text;
}

void bqsr_report_parse(const std::string& text, const std::vector<std::string>& names, std::vector<int64_t>& ctx,
                       std::vector<int64_t>& cyc) {
  const size_t n_rg = names.size();
  ctx.assign(2 * kBqCtxCells * n_rg, 0);
  cyc.assign(2 * kBqCycCells * n_rg, 0);
  std::vector<int64_t> t1(2 * (size_t)FCSBQ_NQ * n_rg, 0);
  if (text.rfind("#:GATKReport.v1.1", 0) != 0) throw formatError("bqsr report: not a GATKReport v1.1");
  std::istringstream in(text);
  int table = -1;  // 1 or 2 inside RecalTable1 / 2's rows
  bool header = false;
  bool saw2 = false;
  auto rg_of = [&](const std::string& s) {
    for (size_t k = 0; k < n_rg; ++k)
      if (names[k] == s) return k;
    throw formatError("bqsr report: read group " + s + " is not in the BAM header");
  };
  for (std::string line; std::getline(in, line);) {
    if (line.rfind("#:GATKTable:", 0) == 0) {
      table = line.rfind("#:GATKTable:RecalTable1:", 0) == 0 ? 1 : line.rfind("#:GATKTable:RecalTable2:", 0) == 0 ? 2 : -1;
      header = table > 0;
      saw2 |= table == 2;
      continue;
    }
    if (line.empty()) {
      table = -1;
      continue;
    }
    if (table < 0) continue;
    if (header) {
      header = false;
      continue;
    }
    std::istringstream ls(line);
    std::vector<std::string> f;
    for (std::string tok; ls >> tok;) f.push_back(tok);
    try {
      if (table == 1) {
        if (f.size() != 6) throw formatError("bqsr report: a RecalTable1 row of " + std::to_string(f.size()) + " fields");
        const int q = std::stoi(f[1]);
        if (q < 0 || q >= FCSBQ_NQ) throw formatError("bqsr report: quality " + f[1]);
        int64_t* c = t1.data() + 2 * (rg_of(f[0]) * FCSBQ_NQ + (size_t)q);
        c[0] += std::stoll(f[4]), c[1] += std::llround(std::stod(f[5]));
      } else {
        if (f.size() != 8) throw formatError("bqsr report: a RecalTable2 row of " + std::to_string(f.size()) + " fields");
        const int q = std::stoi(f[1]);
        if (q < 0 || q >= FCSBQ_NQ) throw formatError("bqsr report: quality " + f[1]);
        const size_t row = rg_of(f[0]) * FCSBQ_NQ + (size_t)q;
        int64_t* c;
        if (f[3] == "Context") {
          const int a = f[2].size() == 2 ? code((uint8_t)f[2][0]) : -1, d = f[2].size() == 2 ? code((uint8_t)f[2][1]) : -1;
          if (a < 0 || d < 0) throw formatError("bqsr report: context " + f[2]);
          c = ctx.data() + 2 * (row * FCSBQ_NCTX + (size_t)(4 * a + d));
        } else if (f[3] == "Cycle") {
          const int cy = std::stoi(f[2]);
          if (cy == 0 || std::abs(cy) > FCSBQ_MAX_CYCLE) throw formatError("bqsr report: cycle " + f[2]);
          c = cyc.data() + 2 * (row * FCSBQ_NCYC + (size_t)(2 * (std::abs(cy) - 1) + (cy < 0)));
        } else {
          throw formatError("bqsr report: covariate " + f[3]);
        }
        c[0] += std::stoll(f[6]), c[1] += std::llround(std::stod(f[7]));
      }
    } catch (const std::logic_error&) {  // stoi / stoll / stod
      throw formatError("bqsr report: a number was expected in \"" + line + "\"");
    }
  }
  if (!saw2) throw formatError("bqsr report: no RecalTable2");
  for (size_t rg = 0; rg < n_rg; ++rg) {
    int64_t qt[FCSBQ_NQ][2];
    quality_table(cyc.data(), (int32_t)rg, qt);
    for (int q = 0; q < FCSBQ_NQ; ++q)
      if (qt[q][0] != t1[2 * (rg * FCSBQ_NQ + (size_t)q)] || qt[q][1] != t1[2 * (rg * FCSBQ_NQ + (size_t)q) + 1])
        throw formatError("bqsr report: RecalTable1 and the cycle rows of RecalTable2 disagree at quality " + std::to_string(q));
  }
}

}  // namespace fcsg
