// indel.h: the targets, left alignment, clean(bin) around the scoring step, and
// the scoring step's oracle by plain loops over csrc/ir_rules.h.
#include "indel.h"

#include <algorithm>
#include <tuple>

#include "common.h"
#include "ir_rules.h"

namespace fcsg {

using namespace fcs;

// ------------------------------------------------------------------ targets
void ir_cigar_events(int32_t ref, int64_t pos, const std::vector<uint32_t>& cigar, std::vector<IrInterval>& out) {
  int64_t p = pos;
  for (const uint32_t c : cigar) {
    const int64_t n = ir_len(c);
    switch (ir_op(c)) {
      case kIrI: out.push_back({ref, std::max<int64_t>(p - 1, 0), p + 1}); break;
      case kIrD: out.push_back({ref, std::max<int64_t>(p - 1, 0), p + n}), p += n; break;
      case kIrM: case kIrEq: case kIrX: case kIrN: p += n; break;
      default: break;
    }
  }
}

std::vector<IrInterval> ir_merge_targets(std::vector<IrInterval> ev) {
  std::sort(ev.begin(), ev.end(), [](const IrInterval& a, const IrInterval& b) {
    return std::tie(a.ref, a.start, a.end) < std::tie(b.ref, b.start, b.end);
  });
  std::vector<IrInterval> merged, out;
  for (const IrInterval& e : ev) {
    if (!merged.empty() && merged.back().ref == e.ref && e.start <= merged.back().end) merged.back().end = std::max(merged.back().end, e.end);
    else merged.push_back(e);
  }
  for (const IrInterval& t : merged)
    if (t.end - t.start <= kIrTargetMax) out.push_back(t);
  return out;
}

std::string ir_target_text(const std::string& chrom, const IrInterval& t) {
  std::string s = chrom + ":" + std::to_string(t.start + 1);
  if (t.end - t.start > 1) s += "-" + std::to_string(t.end);
  return s;
}

// ------------------------------------------------------------------ left alignment
bool ir_one_indel(const std::vector<uint32_t>& cigar, const std::vector<uint8_t>& codes, IrIndel& out) {
  int64_t run[3] = {0, 0, 0};
  int part = 0;  // 0: the first M run, 1: the indel, 2: the second M run
  bool ins = false;
  for (const uint32_t c : cigar) {
    const uint32_t op = ir_op(c);
    if (ir_len(c) == 0) continue;
    if (ir_is_match(op)) {
      if (part == 1) part = 2;
      run[part] += ir_len(c);
    } else if ((op == kIrI || op == kIrD) && part == 0 && run[0] > 0) {
      part = 1, ins = op == kIrI, run[1] = ir_len(c);
    } else {
      return false;
    }
  }
  if (part != 2) return false;
  out.a = (int)run[0], out.k = (int)run[1], out.ins = ins;
  out.bases.clear();
  if (ins) {
    if ((size_t)(run[0] + run[1]) > codes.size()) return false;
    out.bases.assign(codes.begin() + run[0], codes.begin() + run[0] + run[1]);
  }
  return true;
}

void ir_left_align(const uint8_t* ref, int64_t at, IrIndel& d) {
  int64_t p = at + d.a;
  if (d.ins) {
    while (d.a > 1 && ref[p - 1] == d.bases[(size_t)d.k - 1]) {
      std::rotate(d.bases.begin(), d.bases.end() - 1, d.bases.end());
      --d.a, --p;
    }
  } else {
    while (d.a > 1 && ref[p - 1] == ref[p + d.k - 1]) --d.a, --p;
  }
}

// ------------------------------------------------------------------ clean(bin)
namespace {

// S along a CIGAR: the M bases against the window, 99 for one beyond its end.
uint32_t aligner_score(const IrRead& r, const std::vector<uint32_t>& cigar, const std::vector<uint8_t>& ref, int64_t at) {
  uint32_t sum = 0;
  int64_t x = at;
  size_t i = 0;
  for (const uint32_t c : cigar) {
    const uint32_t op = ir_op(c), n = ir_len(c);
    if (ir_is_match(op)) {
      for (uint32_t k = 0; k < n && i < r.codes.size(); ++k, ++i, ++x) {
        if (x >= (int64_t)ref.size()) sum += kIrOverhang;
        else if (ir_differ(r.codes[i], ref[(size_t)x])) sum += r.quals[i];
      }
    } else if (op == kIrI) {
      i += n;
    } else if (op == kIrD || op == kIrN) {
      x += n;
    }
  }
  return sum;
}

// The window with the indel applied at offset u.
IrConsensus make_consensus(const std::vector<uint8_t>& ref, int u, const IrIndel& d) {
  IrConsensus c;
  c.u = u, c.k = d.k, c.ins = d.ins;
  c.seq.assign(ref.begin(), ref.begin() + u);
  if (d.ins) c.seq.insert(c.seq.end(), d.bases.begin(), d.bases.end());
  c.seq.insert(c.seq.end(), ref.begin() + u + (d.ins ? 0 : d.k), ref.end());
  return c;
}

// The alignment of a read of L bases at consensus columns [o, o + L); false when it keeps no M.
bool restrict_alignment(const IrConsensus& c, int64_t lo, int o, int L, int64_t& start, std::vector<uint32_t>& cigar) {
  cigar.clear();
  const int u = c.u, k = c.k;
  if (!c.ins) {
    start = o < u ? lo + o : lo + o + k;
    if (o < u && u < o + L) cigar = {ir_pack((uint32_t)(u - o), kIrM), ir_pack((uint32_t)k, kIrD), ir_pack((uint32_t)(o + L - u), kIrM)};
    else cigar = {ir_pack((uint32_t)L, kIrM)};
    return true;
  }
  const int m1 = std::clamp(u - o, 0, L);
  const int i0 = std::max(o, u), i1 = std::min(o + L, u + k);
  const int il = std::max(i1 - i0, 0), m2 = L - m1 - il;
  if (m1 + m2 == 0) return false;
  start = o <= u ? lo + o : o < u + k ? lo + u : lo + o - k;
  if (m1) cigar.push_back(ir_pack((uint32_t)m1, kIrM));
  if (il) cigar.push_back(ir_pack((uint32_t)il, kIrI));
  if (m2) cigar.push_back(ir_pack((uint32_t)m2, kIrM));
  return true;
}

// Adds a read's differing and total qualities per window column along an alignment; the differing M bases plus I and D lengths.
int walk_columns(const IrRead& r, int64_t at, const std::vector<uint32_t>& cigar, const std::vector<uint8_t>& ref, int64_t* differing,
                 int64_t* total) {
  int nm = 0;
  int64_t x = at;
  size_t i = 0;
  for (const uint32_t c : cigar) {
    const uint32_t op = ir_op(c), n = ir_len(c);
    if (ir_is_match(op)) {
      for (uint32_t k = 0; k < n && i < r.codes.size(); ++k, ++i, ++x) {
        if (x < 0 || x >= (int64_t)ref.size()) continue;
        const bool d = ir_differ(r.codes[i], ref[(size_t)x]);
        nm += d;
        if (total) total[x] += r.quals[i], differing[x] += d ? r.quals[i] : 0;
      }
    } else if (op == kIrI) {
      i += n, nm += (int)n;
    } else if (op == kIrD) {
      x += n, nm += (int)n;
    } else if (op == kIrN) {
      x += n;
    }
  }
  return nm;
}

bool has_indel(const std::vector<uint32_t>& cigar) {
  for (const uint32_t c : cigar)
    if (ir_op(c) == kIrI || ir_op(c) == kIrD) return true;
  return false;
}

}  // namespace

IrPlan ir_prepare(const IrBin& bin, const IrParams& prm) {
  IrPlan plan;
  const int64_t W = (int64_t)bin.ref.size();
  plan.cigar.resize(bin.reads.size());
  for (size_t i = 0; i < bin.reads.size(); ++i) plan.cigar[i] = bin.reads[i].cigar;
  if ((int64_t)bin.reads.size() > prm.max_reads || W > FCSIR_SEQ_MAX) {
    plan.skip = true;
    return plan;
  }
  std::vector<std::pair<int, IrIndel>> proposed;  // (u, the indel) of the reads, in read order
  for (size_t i = 0; i < bin.reads.size(); ++i) {
    const IrRead& r = bin.reads[i];
    const int64_t at = r.start - bin.lo;
    IrIndel d;
    const bool one = ir_one_indel(r.cigar, r.codes, d);
    if (one) {
      const int a0 = d.a;
      int64_t m = 0;
      for (const uint32_t c : r.cigar)
        if (ir_is_match(ir_op(c))) m += ir_len(c);
      ir_left_align(bin.ref.data(), at, d);
      if (d.a != a0)
        plan.cigar[i] = {ir_pack((uint32_t)d.a, kIrM), ir_pack((uint32_t)d.k, d.ins ? kIrI : kIrD), ir_pack((uint32_t)(m - d.a), kIrM)};
    }
    const uint32_t raw = ir_score(r.codes.data(), r.quals.data(), (int)r.codes.size(), bin.ref.data(), W, at);
    if (raw == 0) continue;
    plan.alt.push_back((int)i);
    plan.raw.push_back(raw);
    plan.aligner.push_back(aligner_score(r, plan.cigar[i], bin.ref, at));
    if (!r.duplicate) plan.total_raw += raw;
    if (one && (!d.ins || std::all_of(d.bases.begin(), d.bases.end(), [](uint8_t b) { return b < 4; })))
      proposed.emplace_back((int)at + d.a, d);
  }
  auto add = [&](const IrConsensus& c) {
    if ((int)plan.cons.size() >= prm.max_consensuses) return;
    for (const IrConsensus& have : plan.cons)
      if (have.seq == c.seq) return;
    if (c.seq.size() > (size_t)FCSIR_SEQ_MAX) plan.skip = true;
    plan.cons.push_back(c);
  };
  for (const IrKnown& kn : bin.known) {
    const int64_t ev0 = kn.pos - 1, ev1 = kn.indel.ins ? kn.pos : kn.pos + kn.indel.k;
    if (ev0 < bin.lo + 1 || ev1 > bin.hi - 1) continue;
    IrIndel d = kn.indel;
    d.a = (int)(kn.pos - bin.lo);
    ir_left_align(bin.ref.data(), 0, d);
    add(make_consensus(bin.ref, d.a, d));
  }
  for (const auto& [u, d] : proposed) add(make_consensus(bin.ref, u, d));
  return plan;
}

std::vector<IrUpdate> ir_decide(const IrBin& bin, const IrPlan& plan, const IrParams& prm, const uint32_t* best, const int32_t* off) {
  std::vector<IrUpdate> out;
  const size_t C = plan.cons.size(), R = plan.alt.size();
  if (plan.skip || C == 0 || R == 0) return out;
  auto my_score = [&](size_t c, size_t j, bool& listed) {
    const uint32_t my = best[c * R + j];
    listed = !(my > plan.aligner[j] || my >= plan.raw[j]);
    return listed ? my : plan.raw[j];
  };
  size_t pick = 0;
  int64_t pick_sum = -1;
  for (size_t c = 0; c < C; ++c) {
    int64_t sum = 0;
    for (size_t j = 0; j < R; ++j) {
      bool listed;
      const uint32_t my = my_score(c, j, listed);
      if (!bin.reads[(size_t)plan.alt[j]].duplicate) sum += my;
    }
    if (pick_sum < 0 || sum < pick_sum) pick = c, pick_sum = sum;
  }
  if (plan.total_raw - pick_sum < prm.lod_tenths) return out;
  const IrConsensus& cons = plan.cons[pick];
  std::vector<int> update_of(R, -1);
  for (size_t j = 0; j < R; ++j) {
    bool listed;
    my_score(pick, j, listed);
    if (!listed) continue;
    const IrRead& r = bin.reads[(size_t)plan.alt[j]];
    IrUpdate u;
    u.read = plan.alt[j];
    if (!restrict_alignment(cons, bin.lo, off[pick * R + j], (int)r.codes.size(), u.start, u.cigar)) continue;
    if (u.start == r.start && u.cigar == r.cigar) continue;
    u.nm = walk_columns(r, u.start - bin.lo, u.cigar, bin.ref, nullptr, nullptr);
    update_of[j] = (int)out.size();
    out.push_back(std::move(u));
  }
  // the column check over the alt reads that had no indel
  const size_t W = bin.ref.size();
  std::vector<int64_t> om(W, 0), ot(W, 0), cm(W, 0), ct(W, 0);
  for (size_t j = 0; j < R; ++j) {
    const IrRead& r = bin.reads[(size_t)plan.alt[j]];
    if (r.duplicate || has_indel(r.cigar)) continue;
    walk_columns(r, r.start - bin.lo, r.cigar, bin.ref, om.data(), ot.data());
    if (update_of[j] >= 0) walk_columns(r, out[(size_t)update_of[j]].start - bin.lo, out[(size_t)update_of[j]].cigar, bin.ref, cm.data(), ct.data());
    else walk_columns(r, r.start - bin.lo, r.cigar, bin.ref, cm.data(), ct.data());
  }
  int orig_cols = 0, clean_cols = 0;
  for (size_t x = 0; x < W; ++x) {
    if (cm[x] == om[x]) continue;
    if (100 * om[x] > 15 * ot[x]) ++orig_cols, clean_cols += 100 * cm[x] > 15 * ct[x];
    else if (100 * cm[x] > 15 * ct[x]) ++clean_cols;
  }
  if (!(orig_cols == 0 || clean_cols < orig_cols)) out.clear();
  return out;
}

// ------------------------------------------------------------------ the scoring step
void IrBatch::clear() {
  seq.clear(), read.clear(), qual.clear(), orig.clear();
  seq_off.assign(1, 0), bin_seq.assign(1, 0), read_off.assign(1, 0), bin_read.assign(1, 0), pair_first.assign(1, 0);
}

void IrBatch::add(const IrBin& bin, const IrPlan& plan) {
  for (const IrConsensus& c : plan.cons) seq.insert(seq.end(), c.seq.begin(), c.seq.end()), seq_off.push_back((int64_t)seq.size());
  for (const int i : plan.alt) {
    const IrRead& r = bin.reads[(size_t)i];
    read.insert(read.end(), r.codes.begin(), r.codes.end()), qual.insert(qual.end(), r.quals.begin(), r.quals.end());
    read_off.push_back((int64_t)read.size());
    orig.push_back((int32_t)(r.start - bin.lo));
  }
  bin_seq.push_back((int64_t)seq_off.size() - 1), bin_read.push_back((int64_t)read_off.size() - 1);
  pair_first.push_back(pair_first.back() + (int64_t)(plan.cons.size() * plan.alt.size()));
}

fcsir_batch IrBatch::view() const {
  fcsir_batch b{};
  b.n_bins = (int64_t)bin_seq.size() - 1, b.n_seq = (int64_t)seq_off.size() - 1, b.n_reads = (int64_t)read_off.size() - 1;
  b.n_seq_bytes = (int64_t)seq.size(), b.n_read_bytes = (int64_t)read.size();
  b.seq = seq.data(), b.seq_off = seq_off.data(), b.bin_seq = bin_seq.data();
  b.read = read.data(), b.qual = qual.data(), b.read_off = read_off.data(), b.bin_read = bin_read.data(), b.orig = orig.data();
  return b;
}

void ir_score_host(const fcsir_batch& b, int threads, uint32_t* best, int32_t* off) {
  std::vector<int64_t> first((size_t)b.n_bins + 1, 0);
  for (int64_t k = 0; k < b.n_bins; ++k)
    first[(size_t)k + 1] = first[(size_t)k] + (b.bin_seq[k + 1] - b.bin_seq[k]) * (b.bin_read[k + 1] - b.bin_read[k]);
  parallel_tasks((size_t)b.n_bins, threads, [&](size_t k) {
    const int64_t s0 = b.bin_seq[k], C = b.bin_seq[k + 1] - s0, r0 = b.bin_read[k], R = b.bin_read[k + 1] - r0;
    for (int64_t c = 0; c < C; ++c)
      for (int64_t r = 0; r < R; ++r) {
        const int64_t so = b.seq_off[s0 + c], ro = b.read_off[r0 + r];
        const uint64_t key = ir_best(b.read + ro, b.qual + ro, (int)(b.read_off[r0 + r + 1] - ro), b.seq + so, b.seq_off[s0 + c + 1] - so,
                                     b.orig[r0 + r]);
        const int64_t p = first[k] + c * R + r;
        best[p] = ir_key_score(key), off[p] = ir_key_offset(key);
      }
  });
}

}  // namespace fcsg
