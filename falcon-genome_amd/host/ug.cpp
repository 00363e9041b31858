// The rules of ug.h with plain loops: the table, the record and base filters,
// the window clip, a private pileup per range of loci, the site predicate, and
// the genotype step over a site's integers.
#include "ug.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "common.h"

namespace fcsg {

namespace {

constexpr uint16_t kFilter = 0x4 | 0x100 | 0x200 | 0x400;
constexpr int kMaxQ = 93;

bool ref_op(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
bool aligned_op(uint32_t op) { return op == 0 || op == 7 || op == 8; }
bool read_op(uint32_t op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }

int letter(uint8_t c) {
  switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
  }
}

struct Rec {
  const uint32_t* cigar;
  int64_t n_ops, q0, L, pos, end;
  int mapq;
  bool absent;
};

// The record's view when it is counted in this window's contig; false otherwise.
bool counted_record(const fcsug_batch& b, const fcsug_window& w, int64_t r, Rec& rec) {
  if (b.ref_id[r] < 0 || b.ref_id[r] != w.ref_id) return false;
  rec.n_ops = b.cigar_off[r + 1] - b.cigar_off[r];
  if (rec.n_ops <= 0 || (b.flag[r] & kFilter) || b.mapq[r] == 255) return false;
  rec.cigar = b.cigar + b.cigar_off[r];
  rec.q0 = b.base_off[r], rec.L = b.base_off[r + 1] - b.base_off[r], rec.pos = b.pos[r], rec.mapq = b.mapq[r];
  rec.absent = b.qual_absent[r] != 0;
  rec.end = rec.pos;
  for (int64_t k = 0; k < rec.n_ops; ++k)
    if (ref_op(rec.cigar[k] & 15u)) rec.end += rec.cigar[k] >> 4;
  return true;
}

void check_record(const Rec& rec, const fcsug_window& w, int64_t r) {
  int64_t covered = 0, p = rec.pos;
  for (int64_t k = 0; k < rec.n_ops; ++k) {
    const uint32_t op = rec.cigar[k] & 15u;
    const int64_t len = rec.cigar[k] >> 4;
    if (read_op(op)) covered += len;
    if (aligned_op(op) && len > 0 && (p < 0 || p + len > w.contig_len))
      throw failedCommand("[E::ug] record " + std::to_string(r) + " has an aligned base beyond its contig");
    if (ref_op(op)) p += len;
  }
  if (covered != rec.L) throw failedCommand("[E::ug] the CIGAR of record " + std::to_string(r) + " does not cover its bases");
}

struct Cell {
  uint32_t n[4] = {0, 0, 0, 0}, qsum[4] = {0, 0, 0, 0}, n_del = 0;
  uint64_t mq2 = 0;
  int64_t A[4] = {0, 0, 0, 0}, B[4] = {0, 0, 0, 0}, C[4] = {0, 0, 0, 0};
};

// Adds the record to cells, which stand for positions [lo, hi).
void pile_record(const fcsug_batch& b, int min_baseq, const int64_t* table, const Rec& rec, int64_t lo, int64_t hi, Cell* cells) {
  int64_t i = 0, p = rec.pos;
  for (int64_t k = 0; k < rec.n_ops; ++k) {
    const uint32_t op = rec.cigar[k] & 15u;
    const int64_t len = rec.cigar[k] >> 4;
    if (aligned_op(op)) {
      for (int64_t j = std::max<int64_t>(0, lo - p); j < len && p + j < hi; ++j) {
        const int x = letter(b.bases[rec.q0 + i + j]);
        const int q = rec.absent ? 0 : b.qual[rec.q0 + i + j];
        const int qe = std::min({q, rec.mapq, kMaxQ});
        if (x > 3 || qe < min_baseq) continue;
        Cell& c = cells[p + j - lo];
        ++c.n[x], c.qsum[x] += (uint32_t)qe, c.mq2 += (uint64_t)(rec.mapq * rec.mapq);
        c.A[x] += table[3 * qe], c.B[x] += table[3 * qe + 1], c.C[x] += table[3 * qe + 2];
      }
    } else if (op == 2 && std::min(rec.mapq, kMaxQ) >= min_baseq) {
      for (int64_t j = std::max<int64_t>(0, lo - p); j < len && p + j < hi; ++j) ++cells[p + j - lo].n_del;
    }
    if (read_op(op)) i += len;
    if (ref_op(op)) p += len;
  }
}

bool make_site(const Cell& c, uint8_t ref_byte, int64_t offset, fcsug_site& s) {
  const int r = letter(ref_byte);
  if (r > 3) return false;
  bool any = false;
  for (int x = 0; x < 4; ++x) any |= x != r && c.n[x] > 0;
  if (!any) return false;
  int a = -1;
  for (int x = 0; x < 4; ++x)
    if (x != r && (a < 0 || c.qsum[x] > c.qsum[a])) a = x;
  s = fcsug_site{};
  s.offset = (int32_t)offset, s.ref = (uint8_t)r, s.alt = (uint8_t)a;
  for (int x = 0; x < 4; ++x) s.n[x] = c.n[x], s.qsum[x] = c.qsum[x];
  s.n_del = c.n_del, s.mq2 = c.mq2;
  s.gl[0] = c.A[r], s.gl[1] = c.B[r] + c.B[a], s.gl[2] = c.A[a];
  for (int x = 0; x < 4; ++x) {
    if (x != r) s.gl[0] += c.C[x];
    if (x != r && x != a) s.gl[1] += c.C[x];
    if (x != a) s.gl[2] += c.C[x];
  }
  return true;
}

// caller.cpp's log10_add.
double log10_sum(double a, double b) {
  const double m = std::max(a, b);
  if (m == -INFINITY) return m;
  return m + std::log10(std::pow(10.0, a - m) + std::pow(10.0, b - m));
}

}  // namespace

std::vector<int64_t> ug_table(double pcr_error) {
  if (!(pcr_error > 0.0 && pcr_error < 1.0)) throw invalidParam("ug.pcr_error " + std::to_string(pcr_error) + " is outside (0, 1)");
  std::vector<int64_t> t(3 * (kMaxQ + 1));
  const double eps = pcr_error;
  for (int q = 0; q <= kMaxQ; ++q) {
    const double e = std::pow(10.0, -q / 10.0);
    const double same = (1.0 - eps) * (1.0 - e) + eps * e / 3.0;
    const double diff = (1.0 - eps) * e / 3.0 + (eps / 3.0) * (1.0 - e) + 2.0 * (eps / 3.0) * (e / 3.0);
    const double p[3] = {same, 0.5 * same + 0.5 * diff, diff};
    for (int c = 0; c < 3; ++c) t[(size_t)(3 * q + c)] = (int64_t)std::llround(std::log10(p[c]) * 4294967296.0);
  }
  return t;
}

std::vector<fcsug_site> ug_sites_host(const fcsug_batch& b, const fcsug_params& prm, const fcsug_window& w, const uint8_t* ref,
                                      const int64_t* table, int threads) {
  if (b.n < 0 || w.len < 0 || w.len > FCSUG_WINDOW_MAX || w.start < 0 || w.start + w.len > w.contig_len)
    throw failedCommand("[E::ug] bad record count or window");
  for (int k = 0; k < 2; ++k) {
    const int64_t* off = k ? b.base_off : b.cigar_off;
    const int64_t total = k ? b.n_bases : b.n_cigar;
    if (b.n > 0 && off[0] < 0) throw failedCommand("[E::ug] offsets start below zero");
    for (int64_t r = 0; r < b.n; ++r)
      if (off[r + 1] < off[r]) throw failedCommand("[E::ug] offsets out of order at record " + std::to_string(r));
    if (b.n > 0 && off[b.n] > total) throw failedCommand("[E::ug] offsets end beyond the bytes given");
  }
  // every refusal first, so that nothing is returned on one
  Rec rec;
  int64_t last = -1;
  for (int64_t r = 0; r < b.n; ++r) {
    if (b.ref_id[r] != w.ref_id) continue;
    if (last >= 0 && b.pos[r] < b.pos[last])
      throw failedCommand("[E::ug] record " + std::to_string(r) + " at position " + std::to_string(b.pos[r]) +
                          " follows record " + std::to_string(last) + " at " + std::to_string(b.pos[last]) +
                          ": positions decrease");
    last = r;
    if (counted_record(b, w, r, rec)) check_record(rec, w, r);
  }
  const size_t nt = (size_t)std::max<int64_t>(1, std::min<int64_t>(std::min(threads, 16), w.len / 1024));
  std::vector<std::vector<fcsug_site>> part(nt);
  parallel_tasks(nt, (int)nt, [&](size_t t) {
    const int64_t lo = w.start + w.len * (int64_t)t / (int64_t)nt, hi = w.start + w.len * (int64_t)(t + 1) / (int64_t)nt;
    if (lo >= hi) return;
    std::vector<Cell> cells((size_t)(hi - lo));
    Rec rc;
    for (int64_t r = 0; r < b.n; ++r) {
      if (b.ref_id[r] != w.ref_id) continue;
      if (b.pos[r] >= hi) break;  // positions do not decrease
      if (counted_record(b, w, r, rc) && rc.end > lo) pile_record(b, prm.min_baseq, table, rc, lo, hi, cells.data());
    }
    fcsug_site s;
    for (int64_t p = lo; p < hi; ++p)
      if (make_site(cells[(size_t)(p - lo)], ref[p - w.start], p - w.start, s)) part[t].push_back(s);
  });
  std::vector<fcsug_site> out;
  for (const auto& v : part) out.insert(out.end(), v.begin(), v.end());
  return out;
}

bool ug_genotype(const fcsug_site& s, const UgGenotypeParams& g, const std::string& chrom, int64_t window_start, VcfRecord& out) {
  static const char kLetters[] = "ACGT";
  const uint64_t depth = (uint64_t)s.n[0] + s.n[1] + s.n[2] + s.n[3];
  if ((double)s.n_del > g.max_deletion_fraction * (double)(depth + s.n_del)) return false;
  const double prior[3] = {std::log10(1.0 - 1.5 * g.heterozygosity), std::log10(g.heterozygosity),
                           std::log10(g.heterozygosity / 2.0)};
  double post[3];
  for (int k = 0; k < 3; ++k) post[k] = (double)s.gl[k] * (1.0 / 4294967296.0) + prior[k];
  double norm = -INFINITY;
  for (int k = 0; k < 3; ++k) norm = log10_sum(norm, post[k]);
  const double qual = std::min(-10.0 * (post[0] - norm), 9999.0);
  int gt = 0;
  for (int k = 1; k < 3; ++k)
    if (s.gl[k] > s.gl[gt]) gt = k;
  if (gt == 0 || qual < g.stand_call_conf) return false;
  int64_t pl[3];
  for (int k = 0; k < 3; ++k) pl[k] = (10 * (s.gl[gt] - s.gl[k]) + ((int64_t)1 << 31)) >> 32;
  int64_t sorted[3] = {pl[0], pl[1], pl[2]};
  std::sort(sorted, sorted + 3);
  const int64_t gq = std::min<int64_t>(99, sorted[1]);
  char mq[32];
  std::snprintf(mq, sizeof mq, "%.2f", std::sqrt((double)s.mq2 / (double)depth));
  out = VcfRecord{};
  out.chrom = chrom;
  out.pos = window_start + s.offset + 1;
  out.ref = std::string(1, kLetters[s.ref & 3]);
  out.alts = {std::string(1, kLetters[s.alt & 3])};
  out.qual = qual;
  out.info = std::string(gt == 1 ? "AC=1;AF=0.500" : "AC=2;AF=1.00") + ";AN=2;DP=" + std::to_string(depth) + ";MQ=" + mq;
  out.format = "GT:AD:DP:GQ:PL";
  out.samples = {std::string(gt == 1 ? "0/1:" : "1/1:") + std::to_string(s.n[s.ref & 3]) + "," + std::to_string(s.n[s.alt & 3]) +
                 ":" + std::to_string(depth) + ":" + std::to_string(gq) + ":" + std::to_string(pl[0]) + "," +
                 std::to_string(pl[1]) + "," + std::to_string(pl[2])};
  return true;
}

VcfHeader ug_vcf_header(const std::string& sample, const std::vector<std::pair<std::string, int64_t>>& contigs) {
  VcfHeader h;
  h.contigs = contigs;
  h.samples = {sample};
  h.source = "fcs-genome ug (pileup SNP model)";
  h.meta = {"##INFO=<ID=AC,Number=A,Type=Integer,Description=\"Allele count in genotypes\">",
            "##INFO=<ID=AF,Number=A,Type=Float,Description=\"Allele frequency\">",
            "##INFO=<ID=AN,Number=1,Type=Integer,Description=\"Total number of alleles in called genotypes\">",
            "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Counted bases at the locus\">",
            "##INFO=<ID=MQ,Number=1,Type=Float,Description=\"RMS mapping quality of the counted bases\">",
            "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">",
            "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Counted bases of the ref and alt letters\">",
            "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Counted bases\">",
            "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality\">",
            "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scaled genotype likelihoods\">",
            "##FILTER=<ID=PASS,Description=\"All filters passed\">"};
  return h;
}

}  // namespace fcsg
