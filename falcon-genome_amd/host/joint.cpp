// joint.h: the tables, the combine step, the rules of csrc/jg_model.h with
// plain loops over sites on threads, and the record text.
#include "joint.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "common.h"
#include "jg_model.h"

namespace fcsg {

using namespace fcs;

JointTables joint_tables(const JointParams& p, int n_samples) {
  if (n_samples < 1 || n_samples > FCSJG_SAMPLES_MAX)
    throw invalidParam("a cohort of " + std::to_string(n_samples) + " samples (1 to " + std::to_string(FCSJG_SAMPLES_MAX) + ")");
  if (!(p.heterozygosity > 0.0 && p.heterozygosity < 1.0))
    throw invalidParam("joint.heterozygosity " + std::to_string(p.heterozygosity) + " is outside (0, 1)");
  if (!(p.stand_call_conf >= 0.0 && p.stand_call_conf <= 1e6))
    throw invalidParam("joint.stand_call_conf " + std::to_string(p.stand_call_conf) + " is outside 0 .. 1e6");
  JointTables t;
  double rest = 1.0;
  for (int k = 1; k <= 2 * n_samples; ++k) rest -= p.heterozygosity / k;
  if (!(rest > 0.0)) throw invalidParam("joint.heterozygosity " + std::to_string(p.heterozygosity) + " leaves no prior for k = 0");
  t.S.resize(FCSJG_S_ROWS), t.LG.resize(4 * (size_t)n_samples + 1), t.LP.resize(2 * (size_t)n_samples + 1);
  for (int i = 0; i < FCSJG_S_ROWS; ++i)
    t.S[(size_t)i] = (int32_t)std::llround(10.0 * std::log10(1.0 + std::pow(10.0, -i / 160.0)) * 1048576.0);
  t.LG[0] = 0;
  for (int n = 1; n <= 4 * n_samples; ++n) t.LG[(size_t)n] = (int32_t)std::llround(10.0 * std::log10((double)n) * 1048576.0);
  t.LP[0] = (int32_t)std::llround(10.0 * std::log10(rest) * 1048576.0);
  for (int k = 1; k <= 2 * n_samples; ++k) t.LP[(size_t)k] = (int32_t)std::llround(10.0 * std::log10(p.heterozygosity / k) * 1048576.0);
  t.min_qual = (int64_t)std::llround(p.stand_call_conf * 1048576.0);
  return t;
}

void joint_combine(const std::vector<GvcfContig>& samples, int max_alt, JointContig& out) {
  max_alt = std::clamp(max_alt, 1, FCSJG_ALTS_MAX);
  out = JointContig{};
  out.n_samples = (int)samples.size();
  out.rec_off.assign(samples.size() + 1, 0);
  for (size_t s = 0; s < samples.size(); ++s) out.rec_off[s + 1] = out.rec_off[s] + (int64_t)samples[s].size();
  const size_t total = (size_t)out.rec_off.back();
  out.beg.reserve(total), out.end.reserve(total), out.dp.reserve(total), out.kind.reserve(total), out.pl.reserve(6 * total);
  struct Call {
    int32_t pos;
    int32_t sample;
    int64_t rec;  // in the cohort's arrays
    int32_t call;
  };
  std::vector<Call> calls;
  for (size_t s = 0; s < samples.size(); ++s) {
    const GvcfContig& g = samples[s];
    out.beg.insert(out.beg.end(), g.beg.begin(), g.beg.end()), out.end.insert(out.end.end(), g.end.begin(), g.end.end());
    out.dp.insert(out.dp.end(), g.dp.begin(), g.dp.end()), out.kind.insert(out.kind.end(), g.kind.begin(), g.kind.end());
    out.pl.insert(out.pl.end(), g.pl.begin(), g.pl.end());
    for (size_t r = 0; r < g.size(); ++r)
      if (g.call[r] >= 0) calls.push_back(Call{g.beg[r], (int32_t)s, out.rec_off[s] + (int64_t)r, g.call[r]});
  }
  out.alt.assign(total, 0);
  std::stable_sort(calls.begin(), calls.end(), [](const Call& a, const Call& b) { return a.pos < b.pos; });  // column order within a position
  struct Alt {
    std::string text;
    int count, first;
  };
  std::vector<Alt> alts;
  std::vector<int> of;  // the call's entry of alts
  for (size_t a = 0; a < calls.size();) {
    size_t b = a;
    while (b < calls.size() && calls[b].pos == calls[a].pos) ++b;
    const std::string* ref = nullptr;
    for (size_t k = a; k < b; ++k) {
      const std::string& r = samples[(size_t)calls[k].sample].ref[(size_t)calls[k].call];
      if (!ref || r.size() > ref->size()) ref = &r;
    }
    alts.clear(), of.clear();
    for (size_t k = a; k < b; ++k) {
      const GvcfContig& g = samples[(size_t)calls[k].sample];
      const std::string& r = g.ref[(size_t)calls[k].call];
      const std::string text = g.alt[(size_t)calls[k].call] + ref->substr(r.size());
      size_t at = 0;
      while (at < alts.size() && alts[at].text != text) ++at;
      if (at == alts.size()) alts.push_back(Alt{text, 0, (int)at});
      ++alts[at].count;
      of.push_back((int)at);
    }
    std::vector<int> order(alts.size());
    for (size_t k = 0; k < order.size(); ++k) order[k] = (int)k;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return alts[(size_t)x].count > alts[(size_t)y].count; });
    std::vector<int> rank(alts.size());
    for (size_t k = 0; k < order.size(); ++k) rank[(size_t)order[k]] = (int)k;
    const int kept = (int)std::min<size_t>(alts.size(), (size_t)max_alt);
    out.pos.push_back(calls[a].pos), out.n_alt.push_back((uint8_t)kept), out.ref.push_back(*ref);
    for (int i = 0; i < FCSJG_ALTS_MAX; ++i) out.alts.push_back(i < kept ? alts[(size_t)order[(size_t)i]].text : std::string());
    for (size_t k = a; k < b; ++k) {
      const int rk = rank[(size_t)of[k - a]];
      out.alt[(size_t)calls[k].rec] = rk < kept ? (uint8_t)(rk + 1) : 0;
      out.cut += rk >= kept;
    }
    a = b;
  }
}

fcsjg_cohort JointSlice::cohort() const {
  fcsjg_cohort c{};
  c.n_samples = n_samples, c.n_records = (int64_t)beg.size(), c.rec_off = rec_off.data();
  c.beg = beg.data(), c.end = end.data(), c.kind = kind.data(), c.alt = alt.data(), c.dp = dp.data(), c.pl = pl.data();
  return c;
}

void joint_slice(const JointContig& c, size_t lo, size_t hi, JointSlice& out) {
  out.n_samples = c.n_samples;
  out.pos = c.pos.data() + lo, out.n_alt = c.n_alt.data() + lo, out.n_sites = (int64_t)(hi - lo);
  out.rec_off.assign((size_t)c.n_samples + 1, 0);
  out.beg.clear(), out.end.clear(), out.dp.clear(), out.pl.clear(), out.kind.clear(), out.alt.clear();
  if (lo >= hi) return;
  const int32_t first = c.pos[lo], last = c.pos[hi - 1];
  for (int s = 0; s < c.n_samples; ++s) {
    const int32_t* b0 = c.beg.data() + c.rec_off[(size_t)s];
    const int32_t* b1 = c.beg.data() + c.rec_off[(size_t)s + 1];
    const int32_t* a = std::upper_bound(b0, b1, first);  // the records before it with the last beg <= first may be a source
    if (a != b0) a = std::lower_bound(b0, a, a[-1]);
    const int32_t* e = std::upper_bound(a, b1, last);
    const size_t r0 = (size_t)(a - c.beg.data()), r1 = (size_t)(e - c.beg.data());
    out.beg.insert(out.beg.end(), c.beg.begin() + (long)r0, c.beg.begin() + (long)r1);
    out.end.insert(out.end.end(), c.end.begin() + (long)r0, c.end.begin() + (long)r1);
    out.dp.insert(out.dp.end(), c.dp.begin() + (long)r0, c.dp.begin() + (long)r1);
    out.kind.insert(out.kind.end(), c.kind.begin() + (long)r0, c.kind.begin() + (long)r1);
    out.alt.insert(out.alt.end(), c.alt.begin() + (long)r0, c.alt.begin() + (long)r1);
    out.pl.insert(out.pl.end(), c.pl.begin() + (long)(6 * r0), c.pl.begin() + (long)(6 * r1));
    out.rec_off[(size_t)s + 1] = (int64_t)out.beg.size();
  }
}

void JointOutputs::resize(int64_t n_sites, int n_samples, int64_t max_pl) {
  const size_t ns = (size_t)n_sites, cells = ns * (size_t)n_samples;
  q.resize(ns * FCSJG_ALTS_MAX), mle.resize(ns * FCSJG_ALTS_MAX), qual.resize(ns), kept.resize(ns), ac.resize(ns * FCSJG_ALTS_MAX);
  an.resize(ns), dp.resize(ns), pl_off.resize(ns), src.resize(cells), gt.resize(2 * cells), gq.resize(cells);
  pl.resize((size_t)max_pl);
}

fcsjg_out JointOutputs::view() {
  fcsjg_out o{};
  o.q = q.data(), o.mle = mle.data(), o.qual = qual.data(), o.kept = kept.data(), o.ac = ac.data(), o.an = an.data();
  o.dp = dp.data(), o.pl_off = pl_off.data(), o.src = src.data(), o.gt = gt.data(), o.gq = gq.data(), o.pl = pl.data();
  o.max_pl = (int64_t)pl.size(), o.n_pl = &n_pl;
  return o;
}

void joint_genotype_host(const fcsjg_cohort& c, const fcsjg_sites& st, const fcsjg_model& m, int threads, const fcsjg_out& o) {
  const int n = c.n_samples;
  if (n < 1 || n > FCSJG_SAMPLES_MAX || st.n_sites < 0 || c.n_records < 0 || o.max_pl < 0)
    throw failedCommand("[E::joint] bad cohort, site count or max_pl");
  for (int s = 0; s < n; ++s) {
    if (c.rec_off[s] < 0 || c.rec_off[s + 1] < c.rec_off[s] || c.rec_off[s + 1] > c.n_records)
      throw failedCommand("[E::joint] record offsets out of order at sample " + std::to_string(s));
    for (int64_t r = c.rec_off[s]; r < c.rec_off[s + 1]; ++r) {
      const std::string at = "record " + std::to_string(r - c.rec_off[s]) + " of sample " + std::to_string(s);
      if (c.beg[r] < 0 || c.end[r] <= c.beg[r]) throw failedCommand("[E::joint] " + at + " spans " + std::to_string(c.beg[r]) + " to " + std::to_string(c.end[r]));
      if (r > c.rec_off[s] && c.beg[r] < c.beg[r - 1]) throw failedCommand("[E::joint] " + at + ": positions decrease");
      if (c.kind[r] > FCSJG_KIND_CALL || c.alt[r] > FCSJG_ALTS_MAX || c.dp[r] < 0) throw failedCommand("[E::joint] " + at + " has a kind, ALT index or DP out of range");
      for (int g = 0; g < (c.kind[r] == FCSJG_KIND_BLOCK ? 3 : 6); ++g)
        if (c.pl[6 * r + g] < 0 || c.pl[6 * r + g] > FCSJG_PL_MAX) throw failedCommand("[E::joint] " + at + " has a PL of " + std::to_string(c.pl[6 * r + g]));
    }
  }
  for (int64_t k = 0; k < st.n_sites; ++k)
    if (st.pos[k] < 0 || (k > 0 && st.pos[k] <= st.pos[k - 1]) || st.n_alt[k] < 1 || st.n_alt[k] > FCSJG_ALTS_MAX)
      throw failedCommand("[E::joint] site " + std::to_string(k) + ": positions do not ascend, or ALTs outside 1 .. 6");
  const size_t ns = (size_t)st.n_sites;
  std::vector<int64_t> counts(ns);
  // the sources, the model per ALT and the site decision
  parallel_for(ns, threads, [&](size_t site) {
    thread_local std::vector<int64_t> z, z_new;
    int64_t* src = o.src + site * (size_t)n;
    for (int s = 0; s < n; ++s) src[s] = jg_source(c.beg, c.end, c.kind, c.rec_off[s], c.rec_off[s + 1], st.pos[site]);
    const int n_alt = st.n_alt[site];
    int mask = 0;
    int64_t qual = 0;
    for (int i = 1; i <= FCSJG_ALTS_MAX; ++i) {
      int64_t& q = o.q[site * FCSJG_ALTS_MAX + (size_t)i - 1];
      int32_t& mle = o.mle[site * FCSJG_ALTS_MAX + (size_t)i - 1];
      q = 0, mle = 0;
      if (i > n_alt) continue;
      z.assign(2 * (size_t)n + 1, 0), z_new.assign(2 * (size_t)n + 1, 0);
      int j = 0;
      for (int s = 0; s < n; ++s) {
        const int64_t r = src[s];
        if (r < 0) continue;
        int32_t cc[3];
        jg_collapse(c.kind[r], c.alt[r], n_alt, i, jg_load_pl(c.pl + 6 * r, c.kind[r]), cc);
        ++j;
        for (int k = 0; k <= 2 * j; ++k)
          z_new[(size_t)k] = jg_cell(j, k, z[(size_t)k], k >= 1 ? z[(size_t)k - 1] : 0, k >= 2 ? z[(size_t)k - 2] : 0,
                                     -((int64_t)cc[0] << kJgUnitBits), -((int64_t)cc[1] << kJgUnitBits),
                                     -((int64_t)cc[2] << kJgUnitBits), m.LG, m.S);
        z.swap(z_new);
      }
      int64_t acc = 0, best = 0;
      for (int k = 0; k <= 2 * j; ++k) {
        const int64_t post = z[(size_t)k] + m.LP[k];
        if (k == 0) acc = best = post;
        else acc = jg_lse(acc, post, m.S);
        if (post > best) best = post, mle = k;
      }
      q = acc - (z[0] + m.LP[0]);
      if (mle > 0) mask |= 1 << (i - 1), qual += q;
    }
    const int K = __builtin_popcount((unsigned)mask);
    o.qual[site] = qual, o.kept[site] = (uint8_t)mask;
    counts[site] = mask && qual >= m.min_qual ? (int64_t)n * ((K + 1) * (K + 2) / 2) : 0;
  });
  int64_t total = 0;
  for (size_t k = 0; k < ns; ++k) o.pl_off[k] = counts[k] > 0 ? total : -1, total += counts[k];
  if (total > o.max_pl)
    throw failedCommand("[E::joint] the sites written have " + std::to_string(total) + " PLs, max_pl is " + std::to_string(o.max_pl));
  *o.n_pl = total;
  parallel_for(ns, threads, [&](size_t site) {
    int32_t* ac = o.ac + site * FCSJG_ALTS_MAX;
    std::fill(ac, ac + FCSJG_ALTS_MAX, 0);
    o.an[site] = 0, o.dp[site] = 0;
    const int64_t off = o.pl_off[site];
    int K = 0;
    const uint32_t a = jg_kept(o.kept[site], &K);
    const int G = (K + 1) * (K + 2) / 2;
    for (int s = 0; s < n; ++s) {
      const size_t i = site * (size_t)n + (size_t)s;
      const int64_t r = o.src[i];
      int gt[2] = {kJgNoCall, kJgNoCall}, gq = 0;
      if (off >= 0) {
        int32_t* out = o.pl + off + (int64_t)s * G;
        if (r >= 0) {
          o.dp[site] += c.dp[r];
          if (jg_genotype(c.kind[r], c.alt[r], jg_load_pl(c.pl + 6 * r, c.kind[r]), a, K, [&](int g, int32_t v) { out[g] = v; }, gt, &gq)) {
            o.an[site] += 2;
            if (gt[0] > 0) ++ac[gt[0] - 1];
            if (gt[1] > 0) ++ac[gt[1] - 1];
          }
        } else {
          std::fill(out, out + G, 0);
        }
      }
      o.gt[2 * i] = (uint8_t)gt[0], o.gt[2 * i + 1] = (uint8_t)gt[1], o.gq[i] = (uint8_t)gq;
    }
  });
}

int64_t joint_emit(const std::string& chrom, const JointContig& c, size_t lo, const fcsjg_cohort& records, int64_t n_sites, const fcsjg_out& o,
                   std::string& text) {
  const int n = c.n_samples;
  int64_t written = 0;
  char b[64];
  for (int64_t k = 0; k < n_sites; ++k) {
    const int64_t off = o.pl_off[k];
    if (off < 0) continue;
    ++written;
    const size_t site = lo + (size_t)k;
    int K = 0;
    const uint32_t a = jg_kept(o.kept[k], &K);
    const int G = (K + 1) * (K + 2) / 2;
    int rank[FCSJG_ALTS_MAX + 1] = {0, 0, 0, 0, 0, 0, 0};
    for (int x = 0; x <= K; ++x) rank[jg_kept_at(a, x)] = x;
    text += chrom, text += '\t', text += std::to_string((int64_t)c.pos[site] + 1), text += "\t.\t", text += c.ref[site], text += '\t';
    for (int x = 1; x <= K; ++x) {
      if (x > 1) text += ',';
      text += c.alts[site * FCSJG_ALTS_MAX + (size_t)jg_kept_at(a, x) - 1];
    }
    std::snprintf(b, sizeof b, "\t%.2f\t.\t", (double)o.qual[k] / 1048576.0);
    text += b;
    text += "AC=";
    for (int x = 1; x <= K; ++x) text += (x > 1 ? "," : "") + std::to_string(o.ac[k * FCSJG_ALTS_MAX + jg_kept_at(a, x) - 1]);
    text += ";AF=";
    for (int x = 1; x <= K; ++x) {
      const int32_t ac = o.ac[k * FCSJG_ALTS_MAX + jg_kept_at(a, x) - 1], an = o.an[k];
      if (an > 0 && ac == an) std::snprintf(b, sizeof b, "1.00");
      else std::snprintf(b, sizeof b, "%.3f", an > 0 ? (double)ac / (double)an : 0.0);
      if (x > 1) text += ',';
      text += b;
    }
    text += ";AN=" + std::to_string(o.an[k]) + ";DP=" + std::to_string(o.dp[k]) + "\tGT:DP:GQ:PL";
    for (int s = 0; s < n; ++s) {
      const size_t i = (size_t)k * (size_t)n + (size_t)s;
      text += '\t';
      if (o.gt[2 * i] == kJgNoCall) {
        text += "./.";
        continue;
      }
      text += std::to_string(rank[o.gt[2 * i]]) + "/" + std::to_string(rank[o.gt[2 * i + 1]]) + ":" +
              std::to_string(records.dp[o.src[i]]) + ":" + std::to_string(o.gq[i]) + ":";
      const int32_t* pl = o.pl + off + (int64_t)s * G;
      for (int g = 0; g < G; ++g) {
        if (g) text += ',';
        text += std::to_string(pl[g]);
      }
    }
    text += '\n';
  }
  return written;
}

VcfHeader joint_vcf_header(const std::vector<std::string>& samples, const std::vector<std::pair<std::string, int64_t>>& contigs) {
  VcfHeader h;
  h.contigs = contigs;
  h.samples = samples;
  h.source = "fcs-genome joint (exact allele-frequency model)";
  h.meta = {"##INFO=<ID=AC,Number=A,Type=Integer,Description=\"Allele count in genotypes\">",
            "##INFO=<ID=AF,Number=A,Type=Float,Description=\"Allele frequency\">",
            "##INFO=<ID=AN,Number=1,Type=Integer,Description=\"Total number of alleles in called genotypes\">",
            "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Sum of the samples' DP\">",
            "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">",
            "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Read depth of the sample's GVCF record\">",
            "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality\">",
            "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scaled genotype likelihoods\">"};
  return h;
}

}  // namespace fcsg
