// Host check of csrc/fmd_expand.h (the text the gfx950 kernels of
// csrc/fmd_seeds.hip run after the collect): for every read, the SMEMs of
// FmdIndex::collect are put back into emission order (so that the ranks have a
// permutation to undo), ranked and expanded with the header's functions as the
// kernels call them, one SMEM at a time over tiles of the read's keys, and the
// result is compared with std::stable_sort by (qb, qe) and bwa's sampling loop
// written out plainly.
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Ifalcon-genome_amd/csrc -Ifalcon-genome_amd/host tools/micro/fmd_expand_test.cpp \
//       falcon-genome_amd/host/fmindex.cpp -o fmd_expand_test
//   fmd_expand_test [MAX_OCC]          built-in references and queries (fmd_smem_test.cpp's)
//   fmd_expand_test FILE [MAX_OCC]     lines ">ACGT..." are contigs, other lines queries
// MAX_OCC defaults to 500.  Prints, per parameter set, the reads, SMEMs, rows
// and the SMEMs with more occurrences than MAX_OCC (whose rows are sampled).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "fmd_expand.h"
#include "fmindex.h"

using namespace fcsg;

namespace {

std::vector<uint8_t> encode(const std::string& s) {
  std::vector<uint8_t> v(s.size());
  for (size_t i = 0; i < s.size(); ++i) {
    const char b = s[i];
    v[i] = b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 4;
  }
  return v;
}

std::string revcomp(const std::string& s) {
  std::string r(s.rbegin(), s.rend());
  for (char& b : r) b = b == 'A' ? 'T' : b == 'C' ? 'G' : b == 'G' ? 'C' : b == 'T' ? 'A' : 'N';
  return r;
}

std::string random_bases(std::mt19937_64& rng, size_t n) {
  std::string s(n, 'A');
  for (char& b : s) b = "ACGT"[rng() & 3];
  return s;
}

struct Params {
  int min_len, split_len, split_width, max_mem_intv;
};
const Params kParams[] = {{19, 28, 10, 20}, {1, 28, 10, 20}, {19, 1000000000, 10, 20}, {19, 28, 10, 0}};
constexpr int kTile = 64;  // the kernel's

int failures = 0;

void check(const std::vector<std::string>& contigs, const std::vector<std::string>& queries, int max_occ,
           const char* what) {
  std::vector<std::vector<uint8_t>> codes;
  for (const std::string& c : contigs) codes.push_back(encode(c));
  const FmdIndex fmd(codes, 1);
  std::mt19937_64 rng(7);
  for (const Params& P : kParams) {
    long long smems = 0, rows = 0, sampled = 0;
    for (const std::string& qs : queries) {
      const std::vector<uint8_t> q = encode(qs);
      std::vector<BiInterval> sorted;
      fmd.collect(q.data(), (int)q.size(), P.min_len, P.split_len, P.split_width, P.max_mem_intv, sorted);
      // an emission order: a shuffle that keeps SMEMs of equal (qb, qe) in their order (the sort is stable)
      const int k = (int)sorted.size();
      std::vector<fcs::FmdIv> slots(sorted.size());
      {
        std::vector<int> perm(sorted.size());
        std::iota(perm.begin(), perm.end(), 0);
        std::shuffle(perm.begin(), perm.end(), rng);
        for (int a = 0; a < k; ++a)  // restore the order within groups of equal keys
          for (int b = a + 1; b < k; ++b)
            if (sorted[perm[a]].qb == sorted[perm[b]].qb && sorted[perm[a]].qe == sorted[perm[b]].qe && perm[a] > perm[b])
              std::swap(perm[a], perm[b]);
        for (int a = 0; a < k; ++a) {
          const BiInterval& m = sorted[perm[a]];
          slots[a].k = m.k, slots[a].l = m.l, slots[a].s = m.s, slots[a].qb = m.qb, slots[a].qe = m.qe;
        }
      }
      // ---- the plain definition
      std::vector<fcs::FmdIv> want = slots;
      std::stable_sort(want.begin(), want.end(),
                       [](const fcs::FmdIv& a, const fcs::FmdIv& b) { return a.qb != b.qb ? a.qb < b.qb : a.qe < b.qe; });
      std::vector<int64_t> want_rows;
      for (const fcs::FmdIv& m : want) {
        const int64_t step = m.s > max_occ ? m.s / max_occ : 1;
        for (int64_t j = 0, kept = 0; j < m.s && kept < max_occ; j += step, ++kept) want_rows.push_back(m.k + j);
        sampled += m.s > max_occ;
      }
      // ---- the header, as the kernels run it: keys and counts, a place per SMEM from tiles, then the stores
      std::vector<uint64_t> keys(slots.size());
      std::vector<int32_t> counts(slots.size());
      int64_t n_rows = 0;
      for (int i = 0; i < k; ++i) {
        keys[i] = fcs::fmd_seed_key(slots[i].qb, slots[i].qe);
        counts[i] = fcs::fmd_seed_count(slots[i].s, max_occ);
        n_rows += counts[i];
      }
      std::vector<fcs::FmdIv> got(slots.size());
      std::vector<int64_t> got_rows((size_t)n_rows, -1), enc_rows((size_t)n_rows, 0);
      std::vector<int> hits(slots.size(), 0);
      bool ok = n_rows == (int64_t)want_rows.size();
      for (int i = 0; i < k && ok; ++i) {
        int32_t rank = 0;
        int64_t row0 = 0;
        for (int t0 = 0; t0 < k; t0 += kTile)
          fcs::fmd_seed_rank_span(keys[i], i, t0, std::min(kTile, k - t0), keys.data() + t0, counts.data() + t0, rank,
                                  row0);
        if (rank < 0 || rank >= k || row0 < 0 || row0 + counts[i] > n_rows) {
          ok = false;
          break;
        }
        ++hits[rank];
        got[rank] = slots[i];
        fcs::fmd_seed_rows(slots[i].k, slots[i].s, max_occ, counts[i], false, got_rows.data(), row0, n_rows);
        fcs::fmd_seed_rows(slots[i].k, slots[i].s, max_occ, counts[i], true, enc_rows.data(), row0, n_rows);
      }
      for (int i = 0; i < k && ok; ++i)
        ok = hits[i] == 1 && got[i].k == want[i].k && got[i].l == want[i].l && got[i].s == want[i].s &&
             got[i].qb == want[i].qb && got[i].qe == want[i].qe && got[i].k == sorted[i].k && got[i].qb == sorted[i].qb &&
             got[i].qe == sorted[i].qe;
      for (int64_t i = 0; i < n_rows && ok; ++i) ok = got_rows[i] == want_rows[i] && enc_rows[i] == -1 - want_rows[i];
      if (ok && n_rows > 0) {  // no store at or beyond a capacity
        std::vector<int64_t> small((size_t)n_rows, -7);
        const int64_t cap = n_rows / 2;
        for (int i = 0; i < k; ++i) {
          int32_t rank = 0;
          int64_t row0 = 0;
          fcs::fmd_seed_rank_span(keys[i], i, 0, k, keys.data(), counts.data(), rank, row0);
          fcs::fmd_seed_rows(slots[i].k, slots[i].s, max_occ, counts[i], false, small.data(), row0, cap);
        }
        for (int64_t i = 0; i < n_rows && ok; ++i) ok = small[i] == (i < cap ? want_rows[i] : -7);
      }
      smems += k;
      rows += n_rows;
      if (!ok) {
        std::printf("MISMATCH expand %s max_occ %d min_len %d split_len %d max_mem_intv %d: %d SMEMs, %lld rows want %zu: %s\n",
                    what, max_occ, P.min_len, P.split_len, P.max_mem_intv, k, (long long)n_rows, want_rows.size(),
                    qs.c_str());
        ++failures;
      }
    }
    std::printf("%s max_occ %d min_len %d split_len %d max_mem_intv %d: reads %zu smems %lld rows %lld sampled_smems %lld\n",
                what, max_occ, P.min_len, P.split_len, P.max_mem_intv, queries.size(), smems, rows, sampled);
  }
}

bool is_number(const char* s) {
  if (!*s) return false;
  for (; *s; ++s)
    if (*s < '0' || *s > '9') return false;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  int max_occ = 500;
  const char* file = nullptr;
  for (int a = 1; a < argc; ++a) {
    if (is_number(argv[a])) max_occ = std::atoi(argv[a]);
    else file = argv[a];
  }
  if (max_occ < 1) {
    std::fprintf(stderr, "MAX_OCC must be at least 1\n");
    return 2;
  }
  if (file) {
    std::ifstream in(file);
    if (!in) {
      std::fprintf(stderr, "cannot read %s\n", file);
      return 2;
    }
    std::vector<std::string> contigs, queries;
    for (std::string line; std::getline(in, line);) {
      if (!line.empty() && line[0] == '>') contigs.push_back(line.substr(1));
      else queries.push_back(line);  // an empty line is an empty query
    }
    check(contigs, queries, max_occ, "file");
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
  }
  std::mt19937_64 rng(20240607);
  {
    std::vector<std::string> contigs = {random_bases(rng, 6000), random_bases(rng, 3000), random_bases(rng, 4500)};
    contigs[0].replace(1000, 40, contigs[1].substr(500, 40));           // a repeat across contigs
    contigs[0].replace(3000, 60, revcomp(contigs[2].substr(100, 60)));  // a reverse-strand repeat
    std::vector<std::string> queries;
    for (int len : {1, 2, 18, 19, 20, 63, 64, 65, 151, 251}) {
      for (int k = 0; k < 12; ++k) {
        const std::string& c = contigs[k % 3];
        std::string q = c.substr(rng() % (c.size() - len), len);
        for (int e = (int)(rng() % 6); e > 0; --e) {
          char& b = q[rng() % q.size()];
          b = b == 'A' ? 'C' : b == 'C' ? 'G' : b == 'G' ? 'T' : 'A';
        }
        if (k % 4 == 1) q = revcomp(q);
        queries.push_back(q);
      }
    }
    queries.push_back(std::string(40, 'N'));
    queries.push_back(contigs[1].substr(480, 80));
    queries.push_back("");
    check(contigs, queries, max_occ, "plain");
  }
  {
    std::string acg;
    for (int i = 0; i < 40; ++i) acg += "ACG";
    std::vector<std::string> contigs = {random_bases(rng, 800) + std::string(100, 'A') + random_bases(rng, 700),
                                        random_bases(rng, 500) + acg + random_bases(rng, 600)};
    std::vector<std::string> queries = {std::string(150, 'A'), contigs[0].substr(740, 251),
                                        revcomp(contigs[0].substr(760, 200)), contigs[1].substr(450, 251)};
    std::string q;
    for (int i = 0; i < 50; ++i) q += "ACG";
    queries.push_back(q);
    check(contigs, queries, max_occ, "low-complexity");
  }
  std::printf("%s\n", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
