// Host check of csrc/bq_covars.h (the text the gfx950 kernels of csrc/bqsr.hip
// run): random batches go through the header's functions the way the kernels
// call them (one base at a time: the clips, the base's site in the CIGAR, the
// low-quality ends, the keys, the predicates and the apply formula) and every
// count and every new quality is compared with host/bqsr.cpp, which states the
// rules with per-record arrays.
//   g++ -O1 -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude -Ifalcon-genome_amd/csrc -Ifalcon-genome_amd/host tools/micro/bqsr_test.cpp \
//       falcon-genome_amd/host/bqsr.cpp -o bqsr_test
//   bqsr_test [SEED [RECORDS]]
// Prints the batch's figures and "ok", or MISMATCH lines and exit status 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "bq_covars.h"
#include "bqsr.h"

using namespace fcsg;
using namespace fcs;

namespace {

constexpr int kRg = 3;

struct World {
  std::vector<uint8_t> bases;
  std::vector<int64_t> ref_off{0};
  std::vector<uint64_t> known;
  BqRefView view() const {
    BqRefView v;
    v.bases = bases.data(), v.ref_off = ref_off.data(), v.n_ref = (int32_t)ref_off.size() - 1, v.known = known.data();
    return v;
  }
};

struct Batch {
  std::vector<uint16_t> flag;
  std::vector<int32_t> ref_id, pos, rg;
  std::vector<uint8_t> mapq, absent, bases, qual;
  std::vector<uint32_t> cigar;
  std::vector<int64_t> cigar_off{0}, base_off{0};
  fcsbq_batch view() const {
    fcsbq_batch b;
    b.n = (int64_t)flag.size();
    b.flag = flag.data(), b.ref_id = ref_id.data(), b.pos = pos.data(), b.mapq = mapq.data(), b.rg = rg.data();
    b.cigar = cigar.data(), b.cigar_off = cigar_off.data(), b.n_cigar = (int64_t)cigar.size();
    b.bases = bases.data(), b.qual = qual.data(), b.base_off = base_off.data(), b.n_bases = (int64_t)bases.size();
    b.qual_absent = absent.data();
    return b;
  }
};

World make_world(std::mt19937_64& rnd) {
  World w;
  for (int c = 0; c < 2; ++c) {
    for (int i = 0; i < 6000; ++i) {
      const unsigned v = (unsigned)(rnd() % 400);
      w.bases.push_back(v < 2 ? 'N' : v < 6 ? "acgt"[v - 2] : "ACGT"[rnd() % 4]);
    }
    w.ref_off.push_back((int64_t)w.bases.size());
  }
  w.known.assign((w.bases.size() + 63) / 64, 0);
  for (size_t g = 0; g < w.bases.size(); ++g)
    if (rnd() % 100 < 3) w.known[g >> 6] |= (uint64_t)1 << (g & 63);
  return w;
}

void add_record(std::mt19937_64& rnd, const World& w, Batch& b) {
  static const int lengths[] = {1, 2, 15, 16, 17, 63, 64, 65, 151, 151, 151, 500};
  static const uint8_t quals[] = {1, 2, 2, 5, 6, 11, 25, 25, 37, 37, 40, 93};
  static const uint16_t flags[] = {0, 0x10, 0x41, 0x81, 0x91, 0x51};
  const int len = lengths[rnd() % 12];
  const int c = (int)(rnd() % 2);
  int lead = len > 12 && rnd() % 4 == 0 ? (int)(rnd() % 9) + 1 : 0;
  int trail = len - lead > 12 && rnd() % 4 == 0 ? (int)(rnd() % 7) + 1 : 0;
  int left = len - lead - trail;
  const int32_t pos = 20 + (int32_t)(rnd() % (4000 - 600));
  if (rnd() % 10 == 0) b.cigar.push_back((5u << 4) | 5u);
  if (lead) b.cigar.push_back(((uint32_t)lead << 4) | 4u);
  for (int i = 0; i < lead; ++i) b.bases.push_back("ACGT"[rnd() % 4]);
  int64_t p = pos;
  while (left > 0) {
    const int n = rnd() % 2 ? left : 1 + (int)(rnd() % (unsigned)left);
    static const uint32_t mops[] = {0, 0, 0, 7, 8};
    b.cigar.push_back(((uint32_t)n << 4) | mops[rnd() % 5]);
    for (int i = 0; i < n; ++i) {
      const uint8_t r = w.bases[(size_t)(w.ref_off[(size_t)c] + p + i)] & 0xDF;
      b.bases.push_back(rnd() % 25 == 0 ? "ACGTN"[rnd() % 5] : r);
    }
    p += n, left -= n;
    if (left > 1 && rnd() % 3 == 0) {
      if (rnd() % 2) {
        const int m = 1 + (int)(rnd() % (unsigned)std::min(3, left));
        b.cigar.push_back(((uint32_t)m << 4) | 1u);
        for (int i = 0; i < m; ++i) b.bases.push_back("ACGT"[rnd() % 4]);
        left -= m;
      } else {
        const int d = 1 + (int)(rnd() % 4);
        b.cigar.push_back(((uint32_t)d << 4) | (rnd() % 2 ? 2u : 3u));
        p += d;
      }
    }
  }
  if (trail) b.cigar.push_back(((uint32_t)trail << 4) | 4u);
  for (int i = 0; i < trail; ++i) b.bases.push_back("ACGT"[rnd() % 4]);
  for (int i = 0; i < len; ++i) b.qual.push_back(quals[rnd() % 12]);
  if (rnd() % 5 == 0)
    for (int i = 0; i < std::min(len, (int)(rnd() % 4)); ++i) b.qual[b.qual.size() - 1 - (size_t)i] = 2, b.qual[b.qual.size() - (size_t)len + (size_t)i] = 2;
  uint16_t flag = flags[rnd() % 6];
  if (rnd() % 12 == 0) flag |= (uint16_t[]){0x4, 0x100, 0x200, 0x400, 0x800}[rnd() % 5];
  b.flag.push_back(flag);
  b.ref_id.push_back(c), b.pos.push_back(pos);
  b.rg.push_back(rnd() % 20 == 0 ? -1 : (int32_t)(rnd() % kRg));
  b.mapq.push_back((uint8_t[]){0, 255, 20, 60, 60, 60, 60, 60}[rnd() % 8]);
  b.absent.push_back(rnd() % 30 == 0);
  b.cigar_off.push_back((int64_t)b.cigar.size());
  b.base_off.push_back((int64_t)b.bases.size());
}

// The count the way bq_count_kernel runs it, one base at a time.
void count_covars(const World& w, const fcsbq_batch& b, std::vector<int64_t>& ctx, std::vector<int64_t>& cyc) {
  for (int64_t r = 0; r < b.n; ++r) {
    if (!bq_counted(b.flag[r], b.rg[r], b.mapq[r], b.qual_absent[r] != 0)) continue;
    const uint32_t* cigar = b.cigar + b.cigar_off[r];
    const int64_t n_ops = b.cigar_off[r + 1] - b.cigar_off[r], L = b.base_off[r + 1] - b.base_off[r];
    int64_t lead, trail, covered;
    bq_clips(cigar, n_ops, lead, trail, covered);
    if (covered != L) {
      std::printf("MISMATCH record %lld: the CIGAR covers %lld of %lld bases\n", (long long)r, (long long)covered, (long long)L);
      std::exit(1);
    }
    const int64_t k = L - lead - trail;
    const int32_t c = b.ref_id[r];
    const int64_t g0 = w.ref_off[(size_t)c], clen = w.ref_off[(size_t)c + 1] - g0;
    const uint8_t* seq = b.bases + b.base_off[r] + lead;
    const uint8_t* qual = b.qual + b.base_off[r] + lead;
    int64_t nl, nr;
    bq_low_ends(qual, k, nl, nr);
    const bool reverse = b.flag[r] & kBqFlagReverse, second = bq_second(b.flag[r]);
    for (int64_t j = 0; j < k; ++j) {
      const int q = qual[j], code = bq_code(seq[j]);
      int64_t p;
      const int kind = bq_site(cigar, n_ops, b.pos[r], lead + j, p);
      if (bq_skipped(kind, code, q)) continue;
      const bool inside = p >= 0 && p < clen;
      if (kind == kBqAligned && !inside) continue;
      if (inside && bq_known(w.known.data(), g0 + p)) continue;
      const int64_t err = bq_error(kind, code, inside ? w.bases[(size_t)(g0 + p)] : 0) ? 1 : 0;
      const int ck = bq_context(seq, k, j, nl, nr, reverse);
      const size_t row = (size_t)b.rg[r] * kBqNq + (size_t)q;
      if (ck >= 0) ctx[2 * (row * kBqNctx + (size_t)ck)] += 1, ctx[2 * (row * kBqNctx + (size_t)ck) + 1] += err;
      const size_t yk = (size_t)bq_cycle(k, j, reverse, second);
      cyc[2 * (row * kBqNcyc + yk)] += 1, cyc[2 * (row * kBqNcyc + yk) + 1] += err;
    }
  }
}

// The apply the way bq_apply_kernel runs it.
void apply_covars(const fcsbq_batch& b, const BqTables& t, std::vector<uint8_t>& out) {
  for (int64_t r = 0; r < b.n; ++r) {
    const int64_t q0 = b.base_off[r], k = b.base_off[r + 1] - q0;
    const uint8_t* seq = b.bases + q0;
    const uint8_t* qual = b.qual + q0;
    if (!bq_applied(b.rg[r], b.qual_absent[r] != 0)) {
      for (int64_t j = 0; j < k; ++j) out[(size_t)(q0 + j)] = qual[j];
      continue;
    }
    int64_t nl, nr;
    bq_low_ends(qual, k, nl, nr);
    const bool reverse = b.flag[r] & kBqFlagReverse, second = bq_second(b.flag[r]);
    for (int64_t j = 0; j < k; ++j) {
      const int q = qual[j];
      uint8_t v = (uint8_t)q;
      if (q >= 6 && q < kBqNq) {
        const int ck = bq_context(seq, k, j, nl, nr, reverse);
        const size_t row = (size_t)b.rg[r] * kBqNq + (size_t)q;
        v = bq_new_quality(t.base[row], ck >= 0 ? t.dctx[row * kBqNctx + (size_t)ck] : 0.0,
                           t.dcyc[row * kBqNcyc + (size_t)bq_cycle(k, j, reverse, second)]);
      }
      out[(size_t)(q0 + j)] = v;
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
  const int n = argc > 2 ? std::atoi(argv[2]) : 2000;
  std::mt19937_64 rnd(seed);
  const World w = make_world(rnd);
  Batch batch;
  for (int i = 0; i < n; ++i) add_record(rnd, w, batch);
  batch.bases.push_back('N'), batch.qual.push_back(0);  // data() of an empty batch is not null
  batch.cigar.push_back(0);
  fcsbq_batch b = batch.view();
  b.n_bases -= 1, b.n_cigar -= 1;
  const size_t nctx = 2 * kBqCtxCells * kRg, ncyc = 2 * kBqCycCells * kRg;
  std::vector<int64_t> ctx_h(nctx, 0), cyc_h(ncyc, 0), ctx_c(nctx, 0), cyc_c(ncyc, 0);
  bqsr_count_host(w.view(), b, kRg, ctx_h.data(), cyc_h.data(), 1);
  count_covars(w, b, ctx_c, cyc_c);
  int failures = 0;
  for (size_t i = 0; i < nctx && failures < 20; ++i)
    if (ctx_h[i] != ctx_c[i]) std::printf("MISMATCH ctx[%zu]: host %lld, header %lld\n", i, (long long)ctx_h[i], (long long)ctx_c[i]), ++failures;
  for (size_t i = 0; i < ncyc && failures < 20; ++i)
    if (cyc_h[i] != cyc_c[i]) std::printf("MISMATCH cyc[%zu]: host %lld, header %lld\n", i, (long long)cyc_h[i], (long long)cyc_c[i]), ++failures;
  int64_t obs = 0, err = 0, with_ctx = 0;
  for (size_t i = 0; i < ncyc; i += 2) obs += cyc_h[i], err += cyc_h[i + 1];
  for (size_t i = 0; i < nctx; i += 2) with_ctx += ctx_h[i];
  const BqTables t = bqsr_finalize(kRg, ctx_h.data(), cyc_h.data());
  std::vector<uint8_t> out_h((size_t)b.n_bases + 1, 0xEE), out_c((size_t)b.n_bases + 1, 0xEE);
  bqsr_apply_host(b, t, out_h.data(), 1);
  apply_covars(b, t, out_c);
  int64_t changed = 0;
  for (size_t i = 0; i < (size_t)b.n_bases; ++i) {
    changed += out_h[i] != batch.qual[i];
    if (out_h[i] != out_c[i] && failures < 20)
      std::printf("MISMATCH quality[%zu]: host %d, header %d\n", i, out_h[i], out_c[i]), ++failures;
  }
  std::printf("records %d observations %lld errors %lld contexts %lld changed %lld\n", n, (long long)obs, (long long)err,
              (long long)with_ctx, (long long)changed);
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
