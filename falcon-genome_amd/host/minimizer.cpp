#include "minimizer.h"

#include <algorithm>
#include <numeric>
#include <string>
#include <utility>

#include "common.h"
#include "mm_rules.h"

namespace fcsg {

using namespace fcs;

void mm_check_options(const MmOptions& o) {
  if (o.k < 4 || o.k > 31 || o.k > kMmSpanMax) throw invalidParam("minimap.k must be in [4, 31]");
  if (o.w < 1 || o.w > 256) throw invalidParam("minimap.w must be in [1, 256]");
  if (o.max_occ < 1) throw invalidParam("minimap.max_occ must be positive");
  if (o.max_gap < 0 || o.max_gap > kMmGapMax || o.bw < 0 || o.bw > kMmGapMax)
    throw invalidParam("minimap.max_gap and minimap.bw must be in [0, " + std::to_string(kMmGapMax) + "]");
  if (o.min_cnt < 1) throw invalidParam("minimap.min_cnt must be positive");
}

void mm_sketch(const uint8_t* codes, int64_t n, int k, int w, std::vector<MmMini>& out) {
  if (k < 1 || k > 31 || w < 1 || w > 256) throw invalidParam("mm_sketch: k in [1, 31] and w in [1, 256]");
  if (n > INT32_MAX) throw invalidParam("mm_sketch: a sequence of more than 2^31 - 1 bases");
  constexpr uint64_t kNone = ~0ull;  // a skipped k-mer: above every hash
  const uint64_t mask = (1ull << (2 * k)) - 1;
  const int shift = 2 * (k - 1);
  std::vector<uint64_t> hb((size_t)w, kNone);
  std::vector<uint8_t> sb((size_t)w, 0);
  uint64_t fwd = 0, rc = 0, mv = kNone;
  int64_t l = 0, left = -1, last = -1;  // valid bases in a row; the leftmost minimum of the window; the last one emitted
  bool have = false;                    // mv and left describe the window before this one
  auto emit = [&](int64_t pos) {
    out.push_back({hb[(size_t)(pos % w)], (int32_t)pos, sb[(size_t)(pos % w)]});
    last = pos;
  };
  for (int64_t i = 0; i < n; ++i) {
    const uint8_t c = codes[i];
    if (c > 3) {
      l = 0, have = false;
      continue;
    }
    fwd = (fwd << 2 | c) & mask;
    rc = rc >> 2 | (uint64_t)(3 - c) << shift;
    if (++l < k) continue;
    const uint64_t hv = fwd == rc ? kNone : mm_hash64(fwd < rc ? fwd : rc, mask);
    hb[(size_t)(i % w)] = hv, sb[(size_t)(i % w)] = fwd < rc ? 0 : 1;
    if (l < (int64_t)k + w - 1) continue;  // fewer than w k-mers since the restart
    const int64_t ws = i - w + 1;
    if (!have || left < ws) {  // the first window of a stretch, or its leftmost minimum left: look at all w
      mv = kNone;
      for (int64_t pos = ws; pos <= i; ++pos) mv = std::min(mv, hb[(size_t)(pos % w)]);
      left = ws;
      bool first = true;
      for (int64_t pos = ws; pos <= i && mv != kNone; ++pos)
        if (hb[(size_t)(pos % w)] == mv) {
          if (first) left = pos, first = false;
          if (pos > last) emit(pos);
        }
      have = true;
    } else if (hv < mv) {
      mv = hv, left = i;
      emit(i);
    } else if (hv == mv && mv != kNone) {
      emit(i);
    }
  }
}

MmIndex::MmIndex(const std::vector<std::vector<uint8_t>>& contigs, int k, int w, int threads) : k_(k), w_(w) {
  std::vector<std::vector<MmMini>> per(contigs.size());
  for (const auto& c : contigs)
    if (c.size() >= (1ull << 31)) throw invalidParam("a contig of 2^31 bases or more");
  parallel_tasks(contigs.size(), threads, [&](size_t c) { mm_sketch(contigs[c].data(), (int64_t)contigs[c].size(), k, w, per[c]); });
  size_t total = 0;
  for (const auto& v : per) total += v.size();
  std::vector<std::pair<uint64_t, uint64_t>> kv;
  kv.reserve(total);
  for (size_t c = 0; c < per.size(); ++c) {
    for (const MmMini& m : per[c]) kv.emplace_back(m.h, (uint64_t)c << 33 | (uint64_t)m.pos << 1 | m.strand);
    std::vector<MmMini>().swap(per[c]);
  }
  std::sort(kv.begin(), kv.end());
  keys_.resize(total), vals_.resize(total);
  for (size_t i = 0; i < total; ++i) keys_[i] = kv[i].first, vals_[i] = kv[i].second;
}

const uint64_t* MmIndex::find(uint64_t h, size_t& n) const {
  const auto r = std::equal_range(keys_.begin(), keys_.end(), h);
  n = (size_t)(r.second - r.first);
  return vals_.data() + (r.first - keys_.begin());
}

void mm_read_anchors(const MmIndex& idx, const uint8_t* codes, int L, int max_occ, std::vector<int64_t>& t,
                     std::vector<int32_t>& q, double& frac_rep) {
  t.clear(), q.clear();
  frac_rep = 0;
  const int k = idx.k();
  std::vector<MmMini> mini;
  mm_sketch(codes, L, k, idx.w(), mini);
  std::vector<std::pair<int64_t, int32_t>> a;
  int e = 0, l_rep = 0;  // minimizers come in ascending position: the union of the over-frequent spans in one pass
  for (const MmMini& m : mini) {
    size_t n;
    const uint64_t* occ = idx.find(m.h, n);
    if (n > (size_t)max_occ) {
      const int b = m.pos - k + 1;
      l_rep += m.pos + 1 - std::max(b, e);
      e = m.pos + 1;
      continue;
    }
    for (size_t j = 0; j < n; ++j) {
      const bool rev = (occ[j] & 1) != m.strand;
      const int64_t pos = (int64_t)(occ[j] >> 1 & 0xFFFFFFFFu);
      a.emplace_back(mm_target((int)(occ[j] >> 33), rev, pos), rev ? L - m.pos + k - 2 : m.pos);
    }
  }
  frac_rep = L ? (double)l_rep / L : 0.;
  std::sort(a.begin(), a.end());
  t.reserve(a.size()), q.reserve(a.size());
  for (const auto& [ti, qi] : a) t.push_back(ti), q.push_back(qi);
}

void mm_chain_host(const fcsmm_batch& b, int threads, int32_t* f, int32_t* p) {
  const char* who = "mm_chain_host: ";
  if (b.n_reads < 0 || b.n_anchors < 0 || b.n_reads > INT32_MAX || b.n_anchors > INT32_MAX) throw invalidParam(std::string(who) + "bad counts");
  if (b.max_gap < 0 || b.max_gap > kMmGapMax || b.bw < 0 || b.bw > kMmGapMax || b.span < 1 || b.span > kMmSpanMax)
    throw invalidParam(std::string(who) + "a parameter outside its range");
  for (int64_t r = 0; r < b.n_reads; ++r) {
    const int64_t a0 = b.read_off[r], a1 = b.read_off[r + 1];
    if (a0 < 0 || a1 < a0 || a1 > b.n_anchors || a1 - a0 > kMmReadAnchors)
      throw invalidParam(std::string(who) + "bad offsets of read " + std::to_string(r));
    for (int64_t i = a0; i < a1; ++i)
      if (b.t[i] < 0 || b.q[i] < 0 || (i > a0 && !mm_in_order(b.t[i - 1], b.q[i - 1], b.t[i], b.q[i])))
        throw invalidParam(std::string(who) + "read " + std::to_string(r) + " is not sorted by (t, q) at anchor " + std::to_string(i - a0));
  }
  const MmParams P{b.max_gap, b.bw, b.span};
  parallel_for((size_t)b.n_reads, threads, [&](size_t r) {
    const int64_t a0 = b.read_off[r];
    const int n = (int)(b.read_off[r + 1] - a0);
    const int64_t* T = b.t + a0;
    const int32_t* Q = b.q + a0;
    int32_t *F = f + a0, *Pr = p + a0;
    for (int i = 0; i < n; ++i) {
      int32_t best = P.span, from = -1, sc;
      for (int j = std::max(0, i - kMmLookback); j < i; ++j)
        if (mm_candidate(T[i], Q[i], T[j], Q[j], F[j], P, sc)) mm_take(sc, j, P.span, best, from);
      F[i] = best, Pr[i] = from;
    }
  });
}

void mm_backtrack(const int32_t* f, const int32_t* p, int n, int min_cnt, int min_score, std::vector<MmChain>& out) {
  for (int i = 0; i < n; ++i)
    if (p[i] < -1 || p[i] >= i) throw invalidParam("mm_backtrack: anchor " + std::to_string(i) + " has the predecessor " + std::to_string(p[i]));
  std::vector<int32_t> heads((size_t)n);
  std::iota(heads.begin(), heads.end(), 0);
  // descending f; among equal f the larger index first
  std::sort(heads.begin(), heads.end(), [&](int32_t a, int32_t b) { return f[a] != f[b] ? f[a] > f[b] : a > b; });
  std::vector<uint8_t> used((size_t)n, 0);
  for (int32_t h : heads) {
    if (used[h]) continue;
    MmChain c;
    int32_t i = h;
    for (; i >= 0 && !used[i]; i = p[i]) c.anchors.push_back(i), used[i] = 1;
    c.score = f[h] - (i >= 0 ? f[i] : 0);
    if ((int)c.anchors.size() < min_cnt || c.score < min_score) continue;
    std::reverse(c.anchors.begin(), c.anchors.end());
    out.push_back(std::move(c));
  }
}

}  // namespace fcsg
