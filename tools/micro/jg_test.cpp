// csrc/jg_model.h and host/joint.cpp on random cohorts, as a stand-alone host
// program (tests/test_joint_cpu.py builds it with -fsanitize=address,undefined
// and runs it directly):
//   - the exact model as jg_model_kernel lays it out (allele count k = 64 p +
//     lane, passes in ascending order, k - 1 and k - 2 by a rotation of the
//     row before with the carry from the pass below, the sum over k lane by
//     lane, the arg-max with ties to the smaller k) against joint_genotype_host's
//     plain loops;
//   - jg_source's two binary searches against a linear scan;
//   - joint_genotype_host on 1 thread against 4 threads.
// usage: jg_test SEED N_SAMPLES N_SITES; prints the figures and "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "jg_model.h"
#include "joint.h"

using namespace fcs;
using namespace fcsg;

namespace {

int fails = 0;
#define CHECK(cond, ...)              \
  do {                                \
    if (!(cond)) {                    \
      if (++fails < 20) {             \
        std::printf("MISMATCH ");     \
        std::printf(__VA_ARGS__);     \
        std::printf("\n");            \
      }                               \
    }                                 \
  } while (0)

// One (site, ALT) the way a wave of jg_model_kernel<NP> runs it.
void wave_model(const fcsjg_cohort& c, const int64_t* src, int n_alt, int i, const fcsjg_model& m, int NP, int64_t* q, int32_t* mle) {
  std::vector<int64_t> z((size_t)NP * 64, 0), r1(64), r2(64), below1(64), below2(64);
  int j = 0;
  for (int s = 0; s < c.n_samples; ++s) {
    const int64_t r = src[s];
    if (r < 0) continue;
    int32_t cc[3];
    jg_collapse(c.kind[r], c.alt[r], n_alt, i, jg_load_pl(c.pl + 6 * r, c.kind[r]), cc);
    ++j;
    const int64_t g0 = -((int64_t)cc[0] << kJgUnitBits), g1 = -((int64_t)cc[1] << kJgUnitBits), g2 = -((int64_t)cc[2] << kJgUnitBits);
    std::fill(below1.begin(), below1.end(), 0), std::fill(below2.begin(), below2.end(), 0);
    for (int p = 0; p < NP; ++p) {
      if (64 * p > 2 * j) continue;
      int64_t* zp = z.data() + 64 * (size_t)p;
      for (int lane = 0; lane < 64; ++lane) r1[(size_t)lane] = zp[(lane - 1) & 63], r2[(size_t)lane] = zp[(lane - 2) & 63];
      for (int lane = 0; lane < 64; ++lane) {
        const int64_t z1 = lane >= 1 ? r1[(size_t)lane] : below1[(size_t)lane], z2 = lane >= 2 ? r2[(size_t)lane] : below2[(size_t)lane];
        const int k = 64 * p + lane;
        if (k <= 2 * j) zp[lane] = jg_cell(j, k, zp[lane], z1, z2, g0, g1, g2, m.LG, m.S);
      }
      below1 = r1, below2 = r2;
    }
  }
  int64_t acc = 0, post0 = 0, best = INT64_MIN;
  int best_k = INT32_MAX;
  for (int k = 0; k <= 2 * j; ++k) {
    const int64_t post = z[(size_t)k] + m.LP[k];
    if (k == 0) acc = post0 = post;
    else acc = jg_lse(acc, post, m.S);
  }
  for (int lane = 0; lane < 64; ++lane) {  // a lane's best over its passes, then the wave's
    int64_t b = INT64_MIN;
    int bk = INT32_MAX;
    for (int p = 0; p < NP; ++p) {
      const int k = 64 * p + lane;
      if (k > 2 * j) continue;
      const int64_t post = z[(size_t)k] + m.LP[k];
      if (post > b) b = post, bk = k;
    }
    if (b > best || (b == best && bk < best_k)) best = b, best_k = bk;
  }
  *q = acc - post0, *mle = best_k;
}

int64_t linear_source(const fcsjg_cohort& c, int s, int32_t p) {
  int64_t at = -1;
  for (int64_t r = c.rec_off[s]; r < c.rec_off[s + 1]; ++r)
    if (c.beg[r] <= p && (at < 0 || c.beg[r] > c.beg[at])) at = r;
  if (at < 0 || p >= c.end[at] || (c.kind[at] == kJgKindCall && c.beg[at] < p)) return -1;
  return at;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: jg_test SEED N_SAMPLES N_SITES\n");
    return 2;
  }
  const int n = std::atoi(argv[2]), ns = std::atoi(argv[3]);
  std::mt19937_64 rng((uint64_t)std::atoll(argv[1]));
  auto below = [&](int64_t v) { return (int64_t)(rng() % (uint64_t)v); };
  const int span = std::max(4 * ns, 64), max_alt = 3;
  JointContig c;
  c.n_samples = n;
  c.rec_off.push_back(0);
  for (int s = 0; s < n; ++s) {
    int32_t at = (int32_t)below(4);
    while (at < span) {
      const bool call = below(10) < 6;
      c.beg.push_back(at), c.end.push_back(at + 1 + (int32_t)below(call ? 3 : 12)), c.kind.push_back(call ? kJgKindCall : kJgKindBlock);
      c.alt.push_back(call ? (uint8_t)below(max_alt + 1) : 0), c.dp.push_back((int32_t)below(60));
      int32_t pl[6];
      for (int g = 0; g < 6; ++g) pl[g] = below(20) == 0 ? 0 : below(100) == 0 ? kJgPlMax : (int32_t)below(400);
      pl[call ? below(3) : 0] = 0;
      if (below(30) == 0) std::fill(pl, pl + 6, pl[0]);
      c.pl.insert(c.pl.end(), pl, pl + 6);
      at += (int32_t)below(6);  // equal begs, overlaps and gaps
    }
    c.rec_off.push_back((int64_t)c.beg.size());
  }
  for (int p = 0; p < span && (int)c.pos.size() < ns; ++p)
    if (below(span) < 2 * ns || span - p <= ns - (int)c.pos.size()) c.pos.push_back(p), c.n_alt.push_back((uint8_t)(1 + below(max_alt)));
  JointSlice whole;
  joint_slice(c, 0, c.n_sites(), whole);
  const fcsjg_cohort co = whole.cohort();
  const fcsjg_sites st = whole.sites();
  JointParams prm;
  const JointTables tab = joint_tables(prm, n);
  const fcsjg_model m = tab.view();
  JointOutputs a, b;
  a.resize(st.n_sites, n, st.n_sites * n * FCSJG_GENOTYPES_MAX), b.resize(st.n_sites, n, st.n_sites * n * FCSJG_GENOTYPES_MAX);
  joint_genotype_host(co, st, m, 1, a.view());
  joint_genotype_host(co, st, m, 4, b.view());
  CHECK(a.q == b.q && a.mle == b.mle && a.qual == b.qual && a.kept == b.kept && a.ac == b.ac && a.an == b.an && a.dp == b.dp &&
            a.pl_off == b.pl_off && a.src == b.src && a.gt == b.gt && a.gq == b.gq && a.n_pl == b.n_pl &&
            (a.n_pl == 0 || std::memcmp(a.pl.data(), b.pl.data(), 4 * (size_t)a.n_pl) == 0),
        "1 thread and 4 threads differ");
  int NP = 1;
  for (int np : {33, 17, 9, 5, 3, 2, 1})
    if (2 * n + 1 <= 64 * np) NP = np;
  int64_t written = 0, called = 0, kept = 0;
  for (int64_t k = 0; k < st.n_sites; ++k) {
    for (int s = 0; s < n; ++s) {
      const int64_t want = linear_source(co, s, st.pos[k]);
      CHECK(a.src[(size_t)(k * n + s)] == want, "source of site %lld sample %d: %lld, linear scan %lld", (long long)k, s,
            (long long)a.src[(size_t)(k * n + s)], (long long)want);
      called += want >= 0;
    }
    for (int i = 1; i <= st.n_alt[k]; ++i) {
      int64_t q;
      int32_t mle;
      wave_model(co, a.src.data() + k * n, st.n_alt[k], i, m, NP, &q, &mle);
      CHECK(q == a.q[(size_t)(k * 6 + i - 1)] && mle == a.mle[(size_t)(k * 6 + i - 1)], "site %lld ALT %d: wave q %lld mle %d, host q %lld mle %d",
            (long long)k, i, (long long)q, mle, (long long)a.q[(size_t)(k * 6 + i - 1)], a.mle[(size_t)(k * 6 + i - 1)]);
    }
    written += a.pl_off[(size_t)k] >= 0, kept += a.kept[(size_t)k] != 0;
  }
  std::printf("samples %d sites %lld passes %d sources %lld kept %lld written %lld pls %lld\n", n, (long long)st.n_sites, NP,
              (long long)called, (long long)kept, (long long)written, (long long)a.n_pl);
  if (fails) {
    std::printf("%d mismatches\n", fails);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
