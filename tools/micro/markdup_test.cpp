// Host check of csrc/md_keys.h (the text the gfx950 kernels of csrc/markdup.hip
// run): random batches go through the header's functions the way the kernels
// call them (scores from aligned dwords with masked head and tail bytes, the
// one-pass CIGAR walk, packed keys, winner words, a stable sort by the packed
// keys and a max per segment) and every u5, score and flag is compared with
// host/markdup.cpp, which states the rules with tuples and std::sort.
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude -Ifalcon-genome_amd/csrc -Ifalcon-genome_amd/host tools/micro/markdup_test.cpp \
//       falcon-genome_amd/host/markdup.cpp -o markdup_test
//   markdup_test [SEED [RECORDS]]
// Prints the batch's figures and "ok", or MISMATCH lines and exit status 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "markdup.h"
#include "md_keys.h"

using namespace fcsg;

namespace {

int failures = 0;

struct Batch {
  std::vector<uint16_t> flag;
  std::vector<int32_t> ref_id, pos, mate, lib;
  std::vector<uint32_t> cigar;
  std::vector<int64_t> cigar_off{0}, qual_off{0};
  std::vector<uint8_t> qual;
  fcsdup_batch view() const {
    fcsdup_batch b;
    b.n = (int64_t)flag.size();
    b.flag = flag.data(), b.ref_id = ref_id.data(), b.pos = pos.data(), b.mate = mate.data(), b.lib = lib.data();
    b.cigar = cigar.data(), b.cigar_off = cigar_off.data(), b.n_cigar = (int64_t)cigar.size();
    b.qual = qual.data(), b.qual_off = qual_off.data(), b.n_qual = (int64_t)qual.size();
    b.n_ref = 3, b.n_lib = 3;
    return b;
  }
};

void add_record(Batch& B, std::mt19937_64& rng, uint16_t flag, int32_t ref, int32_t pos, int32_t lib) {
  B.flag.push_back(flag), B.ref_id.push_back(ref), B.pos.push_back(pos), B.mate.push_back(-1), B.lib.push_back(lib);
  auto op = [&](uint32_t len, uint32_t o) { B.cigar.push_back((len << 4) | o); };
  const int shape = (int)(rng() % 8);
  if (shape == 0) op(3, 5), op(4, 4), op(93, 0);                 // H S M
  else if (shape == 1) op(90, 0), op(6, 4), op(4, 5);            // M S H
  else if (shape == 2) op(5, 4), op(40, 0), op(3, 2), op(50, 0), op(5, 4);
  else if (shape == 3) op(40, 0), op(2, 1), op(30, 0), op(10, 3), op(28, 0);
  else if (shape == 4) op(7, 4), op(3, 5);                       // clips only
  else if (shape == 5) op(50, 7), op(1, 8), op(49, 7);
  else if (shape != 6) op(100, 0);                               // shape 6: no CIGAR at all
  B.cigar_off.push_back((int64_t)B.cigar.size());
  const int len = (int)(rng() % 6 == 0 ? rng() % 9 : 90 + rng() % 20);  // short ones: every head / tail mask
  for (int i = 0; i < len; ++i) B.qual.push_back((uint8_t)(rng() % 5 == 0 ? rng() % 15 : 15 + rng() % 30));
  B.qual_off.push_back((int64_t)B.qual.size());
}

Batch make_batch(uint64_t seed, int n_templates) {
  std::mt19937_64 rng(seed);
  Batch B;
  for (int t = 0; t < n_templates; ++t) {
    const int32_t ref = (int32_t)(rng() % 3), lib = (int32_t)(rng() % 3), p1 = (int32_t)(rng() % 40);
    const int kind = (int)(rng() % 10);
    if (kind < 6) {  // a pair, either read first
      const bool rev1 = rng() & 1, swap = rng() & 1;
      const int32_t a = (int32_t)B.flag.size();
      const uint16_t f1 = (uint16_t)(0x1 | 0x40 | (rev1 ? 0x10 : 0x20)), f2 = (uint16_t)(0x1 | 0x80 | (rev1 ? 0x20 : 0x10));
      add_record(B, rng, swap ? f2 : f1, ref, swap ? p1 + 5 : p1, lib);
      add_record(B, rng, swap ? f1 : f2, rng() % 8 ? ref : (ref + 1) % 3, swap ? p1 : p1 + 5, lib);
      B.mate[a] = a + 1, B.mate[a + 1] = a;
      if (rng() % 12 == 0) B.flag[a] |= 0x4, B.flag[a + 1] |= 0x8;  // read unmapped: its mate is a fragment
    } else if (kind < 9) {
      add_record(B, rng, (uint16_t)((rng() & 1 ? 0x10 : 0) | (rng() % 4 ? 0 : 0x400)), ref, p1 - 3, lib);
    } else {
      const uint16_t odd[3] = {0x4, 0x100, 0x800};
      add_record(B, rng, odd[rng() % 3], ref, p1, lib);
    }
  }
  return B;
}

// The kernels' route, on the host.
void by_keys(const fcsdup_batch& b, std::vector<int64_t>& u5, std::vector<uint32_t>& score, std::vector<uint8_t>& dup) {
  const size_t n = (size_t)b.n;
  u5.assign(n, 0), score.assign(n, 0), dup.assign(n, 0);
  // the quality bytes in a buffer that starts 4-byte aligned and is padded with 0xff, as the device's arena pads
  std::vector<uint32_t> words(((size_t)b.n_qual + 3) / 4 + 1, 0xffffffffu);
  if (b.n_qual) std::memcpy(words.data(), b.qual, (size_t)b.n_qual);
  std::vector<uint64_t> endk(n, fcs::kMdSentinel), wfrag(n, 0), wpair(n, 0), phi(n, fcs::kMdSentinel), plo(n, 0);
  std::vector<uint8_t> ex(n);
  for (size_t r = 0; r < n; ++r) {
    ex[r] = fcs::md_examined(b.flag[r]);
    const int64_t a0 = b.qual_off[r], a1 = b.qual_off[r + 1];
    uint32_t s = 0;
    for (int64_t w = a0 / 4; a1 > a0 && w < (a1 + 3) / 4; ++w) {
      const int64_t wa = 4 * w;
      s += fcs::md_score_word(words[(size_t)w], wa < a0 ? (int)(a0 - wa) : 0, wa + 4 > a1 ? (int)(a1 - wa) : 4);
    }
    score[r] = s;
    if (s != fcs::md_score(b.qual + a0, a1 - a0)) ++failures, std::printf("MISMATCH record %zu: dword and byte scores\n", r);
    const bool rev = b.flag[r] & 0x10;
    u5[r] = fcs::md_u5(b.pos[r], rev, b.cigar + b.cigar_off[r], b.cigar_off[r + 1] - b.cigar_off[r]);
    if (!fcs::md_fits_u5(u5[r])) ++failures, std::printf("MISMATCH record %zu: u5 does not fit\n", r);
    if (ex[r]) endk[r] = fcs::md_frag_key(b.lib[r], fcs::md_end_word(b.ref_id[r], u5[r], rev));
  }
  const uint64_t mask = ((uint64_t)1 << fcs::kMdEndBits) - 1;
  for (size_t r = 0; r < n; ++r) {
    if (!ex[r]) continue;
    const int32_t m = b.mate[r];
    const bool paired = (b.flag[r] & 1) && !(b.flag[r] & 8) && m >= 0 && ex[m];
    wfrag[r] = fcs::md_winner(score[r], (int32_t)r) | (paired ? fcs::kMdPairedBit : 0);
    if (paired && (int32_t)r < m && (b.flag[m] & 1) && !(b.flag[m] & 8) && b.mate[m] == (int32_t)r) {
      const bool first = fcs::md_end_before(endk[r] & mask, (int32_t)r, endk[m] & mask, m);
      fcs::md_pair_key(first ? endk[r] : endk[m], first ? endk[m] : endk[r], phi[r], plo[r]);
      wpair[r] = fcs::md_winner(score[r] + score[m], (int32_t)r);
    }
  }
  std::vector<int32_t> order(n);
  for (size_t r = 0; r < n; ++r) order[r] = (int32_t)r;
  auto resolve = [&](bool pairs) {
    std::vector<int32_t> v = order;
    if (pairs) {
      std::stable_sort(v.begin(), v.end(), [&](int32_t x, int32_t y) { return plo[x] < plo[y]; });
      std::stable_sort(v.begin(), v.end(), [&](int32_t x, int32_t y) { return phi[x] < phi[y]; });
    } else {
      std::stable_sort(v.begin(), v.end(), [&](int32_t x, int32_t y) { return endk[x] < endk[y]; });
    }
    const std::vector<uint64_t>& key = pairs ? phi : endk;
    const std::vector<uint64_t>& win = pairs ? wpair : wfrag;
    for (size_t i = 0; i < n;) {
      size_t j = i;
      uint64_t best = 0;
      while (j < n && key[v[j]] == key[v[i]] && (!pairs || plo[v[j]] == plo[v[i]])) best = std::max(best, win[v[j++]]);
      for (size_t k = i; k < j && key[v[i]] != fcs::kMdSentinel; ++k) {
        const int32_t r = v[k];
        if (pairs) {
          if (win[r] != best) dup[r] = dup[b.mate[r]] = 1;
        } else if (!(win[r] & fcs::kMdPairedBit) && ((best & fcs::kMdPairedBit) || win[r] != best)) {
          dup[r] = 1;
        }
      }
      i = j;
    }
  };
  resolve(false);
  resolve(true);
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 20261020;
  const int templates = argc > 2 ? std::atoi(argv[2]) : 4000;
  const Batch B = make_batch(seed, templates);
  const fcsdup_batch b = B.view();
  std::vector<int64_t> u5h, u5k;
  std::vector<uint32_t> sh, sk;
  std::vector<uint8_t> dh((size_t)b.n), dk;
  markdup_host_ends(b, u5h, sh);
  const MarkdupStats st = mark_duplicates_host(b, dh.data());
  by_keys(b, u5k, sk, dk);
  for (size_t r = 0; r < (size_t)b.n; ++r) {
    if (u5h[r] != u5k[r]) ++failures, std::printf("MISMATCH record %zu: u5 %lld vs %lld\n", r, (long long)u5h[r], (long long)u5k[r]);
    if (sh[r] != sk[r]) ++failures, std::printf("MISMATCH record %zu: score %u vs %u\n", r, sh[r], sk[r]);
    if (dh[r] != dk[r]) ++failures, std::printf("MISMATCH record %zu: flag %d vs %d\n", r, dh[r], dk[r]);
  }
  std::printf("records %lld examined %lld pairs %lld fragments %lld duplicates %lld\n", (long long)b.n,
              (long long)st.examined, (long long)st.pairs, (long long)st.fragments, (long long)st.duplicates);
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
