// mm_test — csrc/mm_rules.h and host/minimizer.cpp under the sanitizers, on the host.
//
//   g++ -O1 -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude -Ifalcon-genome_amd/csrc -Ifalcon-genome_amd/host \
//       tools/micro/mm_test.cpp falcon-genome_amd/host/minimizer.cpp -o mm_test
//   ./mm_test <seed> <reads>
//
// 1. mm_sketch against the plain statement (every window's minima, by looking at
//    all w k-mers of every window) on seeded random sequences with N runs and
//    repeats, for several (k, w), an even k among them.
// 2. A seeded random reference, its index, and reads cut from it (both strands,
//    with substitutions): every anchor is an exact k-mer match of the oriented
//    read on the reference, and the anchors are sorted.
// 3. mm_chain_host against a host build of the kernel's protocol: 64 lanes, a
//    lane per successor, "read lane j % 64, replace it with anchor j + 64, apply
//    j to every lane", results put aside and written per block of 64.
// 4. mm_backtrack: chains are disjoint, ascending, follow p, and meet min_cnt and
//    min_score.
// Prints "minimizers N anchors N chained N chains N ok", or MISMATCH lines and exit code 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "minimizer.h"
#include "mm_rules.h"

using namespace fcs;
using namespace fcsg;

namespace {

int g_bad = 0;
#define EXPECT(cond, ...)            \
  do {                               \
    if (!(cond)) {                   \
      std::printf("MISMATCH ");      \
      std::printf(__VA_ARGS__);      \
      std::printf("\n");             \
      ++g_bad;                       \
    }                                \
  } while (0)

// The sketch by the plain statement.
std::vector<MmMini> plain_sketch(const std::vector<uint8_t>& c, int k, int w) {
  const int64_t n = (int64_t)c.size();
  const uint64_t mask = (1ull << (2 * k)) - 1, none = ~0ull;
  std::vector<uint64_t> h((size_t)n, none);
  std::vector<uint8_t> st((size_t)n, 0), have((size_t)n, 0);
  for (int64_t i = k - 1; i < n; ++i) {
    uint64_t fwd = 0, rc = 0;
    bool ok = true;
    for (int64_t j = i - k + 1; j <= i; ++j) {
      if (c[j] > 3) ok = false;
      fwd = fwd << 2 | (c[j] & 3);
    }
    for (int64_t j = i; j > i - k; --j) rc = rc << 2 | (3 - (c[j] & 3));
    if (!ok) continue;
    have[i] = 1;
    if (fwd != rc) h[i] = mm_hash64(std::min(fwd, rc), mask), st[i] = fwd < rc ? 0 : 1;
  }
  std::set<int64_t> chosen;
  for (int64_t e = w - 1; e < n; ++e) {
    bool full = true;
    uint64_t m = none;
    for (int64_t i = e - w + 1; i <= e; ++i) full = full && have[i], m = std::min(m, h[i]);
    if (!full || m == none) continue;
    for (int64_t i = e - w + 1; i <= e; ++i)
      if (h[i] == m) chosen.insert(i);
  }
  std::vector<MmMini> out;
  for (int64_t i : chosen) out.push_back({h[i], (int32_t)i, st[i]});
  return out;
}

// f and p of one read as mm_chain_kernel computes them.
void kernel_chain(const int64_t* T, const int32_t* Q, int n, const MmParams& P, int32_t* f, int32_t* p) {
  int64_t ti[64], tn[64];
  int32_t qi[64], qn[64], best[64], from[64], f_out[64], p_out[64];
  auto load = [&](int i, int64_t& t, int32_t& q) { t = i < n ? T[i] : 0, q = i < n ? Q[i] : 0; };
  for (int l = 0; l < 64; ++l) load(l, ti[l], qi[l]), best[l] = P.span, from[l] = -1;
  for (int base = 0; base < n; base += 64) {
    for (int l = 0; l < 64; ++l) load(base + 64 + l, tn[l], qn[l]), f_out[l] = p_out[l] = 0;
    const int steps = std::min(64, n - base);
    for (int s = 0; s < steps; ++s) {
      const int64_t tj = ti[s];
      const int32_t qj = qi[s], fj = best[s];
      f_out[s] = best[s], p_out[s] = from[s], ti[s] = tn[s], qi[s] = qn[s], best[s] = P.span, from[s] = -1;
      for (int l = 0; l < 64; ++l) {
        int32_t sc;
        if (mm_candidate(ti[l], qi[l], tj, qj, fj, P, sc)) mm_take(sc, base + s, P.span, best[l], from[l]);
      }
    }
    for (int l = 0; l < 64 && base + l < n; ++l) f[base + l] = f_out[l], p[base + l] = p_out[l];
  }
}

std::vector<uint8_t> random_codes(std::mt19937_64& rng, int n, bool with_n) {
  std::vector<uint8_t> c((size_t)n);
  for (auto& x : c) x = (uint8_t)(rng() % 4);
  if (with_n)
    for (int r = 0; r < 3; ++r) {
      const int at = (int)(rng() % n), len = 1 + (int)(rng() % 5);
      for (int i = at; i < std::min(n, at + len); ++i) c[i] = 4;
    }
  return c;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
  const int n_reads = argc > 2 ? std::atoi(argv[2]) : 200;
  std::mt19937_64 rng(seed);
  long n_mini = 0, n_anchors = 0, n_chained = 0, n_chains = 0;

  // 1. the sketch
  for (const auto& kw : {std::pair<int, int>{21, 11}, {15, 10}, {6, 4}, {4, 3}, {5, 1}, {31, 5}})
    for (int rep = 0; rep < 6; ++rep) {
      std::vector<uint8_t> c = random_codes(rng, 50 + (int)(rng() % 400), rep % 2 == 1);
      if (rep >= 4) {  // a repeat: equal minima in a window
        const int half = (int)c.size() / 2;
        for (int i = 0; i + half < (int)c.size(); ++i) c[i + half] = c[i];
      }
      if (kw.first <= 6)  // low complexity: palindromic k-mers and ties
        for (auto& x : c) x = x == 4 ? 4 : (x & 1) * 3;
      std::vector<MmMini> got;
      mm_sketch(c.data(), (int64_t)c.size(), kw.first, kw.second, got);
      const std::vector<MmMini> want = plain_sketch(c, kw.first, kw.second);
      EXPECT(got.size() == want.size(), "sketch k %d w %d rep %d: %zu minimizers, the plain statement has %zu", kw.first, kw.second, rep,
             got.size(), want.size());
      for (size_t i = 0; i < std::min(got.size(), want.size()); ++i)
        EXPECT(got[i].h == want[i].h && got[i].pos == want[i].pos && got[i].strand == want[i].strand, "sketch k %d w %d rep %d at %zu", kw.first,
               kw.second, rep, i);
      n_mini += (long)got.size();
    }

  // 2. the index and the anchors
  const int k = 21, w = 11;
  std::vector<std::vector<uint8_t>> contigs{random_codes(rng, 20000, true), random_codes(rng, 8000, false)};
  for (int i = 0; i < 3000; ++i) contigs[1][(size_t)(4000 + i)] = contigs[0][(size_t)(1000 + i)];  // a repeat across contigs
  const MmIndex idx(contigs, k, w, 2);
  std::vector<int64_t> t_all;
  std::vector<int32_t> q_all;
  std::vector<int64_t> off{0};
  for (int r = 0; r < n_reads; ++r) {
    const int c = (int)(rng() % 2), L = 60 + (int)(rng() % 200);
    const int at = (int)(rng() % (contigs[c].size() - L));
    std::vector<uint8_t> read(contigs[c].begin() + at, contigs[c].begin() + at + L);
    for (auto& x : read)
      if (rng() % 50 == 0) x = (uint8_t)(rng() % 4);
    if (r % 2) {
      std::reverse(read.begin(), read.end());
      for (auto& x : read) x = x > 3 ? 4 : 3 - x;
    }
    std::vector<uint8_t> rc(read.rbegin(), read.rend());
    for (auto& x : rc) x = x > 3 ? 4 : 3 - x;
    std::vector<int64_t> t;
    std::vector<int32_t> q;
    double frac = -1;
    mm_read_anchors(idx, read.data(), L, r % 7 == 0 ? 1 : 500, t, q, frac);
    EXPECT(frac >= 0 && frac <= 1, "read %d: frac_rep %g", r, frac);
    for (size_t i = 0; i < t.size(); ++i) {
      EXPECT(i == 0 || mm_in_order(t[i - 1], q[i - 1], t[i], q[i]), "read %d: anchors out of order at %zu", r, i);
      const std::vector<uint8_t>& seq = mm_target_rev(t[i]) ? rc : read;
      const std::vector<uint8_t>& ref = contigs[(size_t)mm_target_contig(t[i])];
      const int64_t pos = mm_target_pos(t[i]);
      bool same = q[i] >= k - 1 && q[i] < L && pos >= k - 1 && pos < (int64_t)ref.size();
      for (int j = 0; same && j < k; ++j) same = seq[(size_t)(q[i] - j)] == ref[(size_t)(pos - j)];
      EXPECT(same, "read %d: anchor %zu is no exact match", r, i);
    }
    t_all.insert(t_all.end(), t.begin(), t.end()), q_all.insert(q_all.end(), q.begin(), q.end());
    off.push_back((int64_t)t_all.size());
  }
  // synthetic long reads: more than one block of 64, with gaps and diagonal steps
  for (int r = 0; r < 20; ++r) {
    const int n = (int)(rng() % 300);
    int64_t t = 1000;
    int32_t q = 20;
    for (int i = 0; i < n; ++i) {
      t_all.push_back(t), q_all.push_back(q);
      const int step = 1 + (int)(rng() % 40);
      t += step + (int)(rng() % 4 == 0 ? rng() % 60 : 0), q += step;
    }
    off.push_back((int64_t)t_all.size());
  }
  n_anchors = (long)t_all.size();

  // 3. the recurrence: the host statement against the kernel's protocol
  fcsmm_batch b{};
  b.n_reads = (int64_t)off.size() - 1, b.n_anchors = (int64_t)t_all.size(), b.t = t_all.data(), b.q = q_all.data(), b.read_off = off.data();
  b.max_gap = 100, b.bw = 50, b.span = k;
  std::vector<int32_t> f(t_all.size() + 1, -7), p(t_all.size() + 1, -7), fk(t_all.size() + 1, -7), pk(t_all.size() + 1, -7);
  mm_chain_host(b, 3, f.data(), p.data());
  const MmParams P{b.max_gap, b.bw, b.span};
  for (int64_t r = 0; r < b.n_reads; ++r) {
    const int64_t a0 = off[(size_t)r];
    const int n = (int)(off[(size_t)r + 1] - a0);
    kernel_chain(t_all.data() + a0, q_all.data() + a0, n, P, fk.data() + a0, pk.data() + a0);
    for (int i = 0; i < n; ++i) {
      EXPECT(f[(size_t)(a0 + i)] == fk[(size_t)(a0 + i)] && p[(size_t)(a0 + i)] == pk[(size_t)(a0 + i)], "read %lld anchor %d: host (%d, %d), kernel protocol (%d, %d)",
             (long long)r, i, f[(size_t)(a0 + i)], p[(size_t)(a0 + i)], fk[(size_t)(a0 + i)], pk[(size_t)(a0 + i)]);
      n_chained += p[(size_t)(a0 + i)] >= 0;
    }
    // 4. the backtrack
    std::vector<MmChain> ch;
    mm_backtrack(f.data() + a0, p.data() + a0, n, 2, 20, ch);
    std::set<int32_t> seen;
    for (const MmChain& c : ch) {
      EXPECT((int)c.anchors.size() >= 2 && c.score >= 20, "read %lld: a chain of %zu anchors, score %d", (long long)r, c.anchors.size(), c.score);
      for (size_t i = 0; i < c.anchors.size(); ++i) {
        EXPECT(seen.insert(c.anchors[i]).second, "read %lld: anchor %d in two chains", (long long)r, c.anchors[i]);
        EXPECT(i == 0 || p[(size_t)(a0 + c.anchors[i])] == c.anchors[i - 1], "read %lld: a chain does not follow p", (long long)r);
      }
    }
    n_chains += (long)ch.size();
  }
  EXPECT(f.back() == -7 && p.back() == -7, "a write beyond the anchors");
  std::printf("minimizers %ld anchors %ld chained %ld chains %ld %s\n", n_mini, n_anchors, n_chained, n_chains, g_bad ? "FAILED" : "ok");
  return g_bad ? 1 : 0;
}
