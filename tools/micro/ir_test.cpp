// ir_test — csrc/ir_rules.h and host/indel.cpp under the sanitizers, on the host.
//
//   g++ -O1 -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude -Ifalcon-genome_amd/csrc -Ifalcon-genome_amd/host \
//       tools/micro/ir_test.cpp falcon-genome_amd/host/indel.cpp -o ir_test
//   ./ir_test <seed> <bins>
//
// 1. ir_hot & ir_mask is non-zero exactly where ir_differ holds, for every pair of codes.
// 2. Seeded random bins around a planted indel go through ir_prepare, the scoring
//    step and ir_decide.  Every pair is scored twice: by ir_score_host (the plain
//    statement) and by a host build of the kernel's arithmetic (mask and hot bytes
//    four to a dword, a byte align of two dwords, the 0 / 1 bytes and the dot
//    product, a lane's offsets in ascending order, the original offset scored
//    base by base); the two must agree on score and offset.
// 3. The updates are checked for what must hold of any of them: a read keeps its
//    length, has an M, and starts inside the window.
// Prints "pairs N alt N consensuses N cleaned N updates N ok", or MISMATCH lines and exit code 1.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "indel.h"
#include "ir_rules.h"

using namespace fcs;
using namespace fcsg;

namespace {

uint32_t align_byte(uint32_t above, uint32_t below, uint32_t sh) { return (uint32_t)((((uint64_t)above << 32) | below) >> (8 * sh)); }

uint32_t dot4(uint32_t a, uint32_t b, uint32_t acc) {
  for (int k = 0; k < 4; ++k) acc += ((a >> (8 * k)) & 0xFF) * ((b >> (8 * k)) & 0xFF);
  return acc;
}

// best(c, r) as ir_score_kernel computes it.
uint64_t kernel_best(const uint8_t* rc, const uint8_t* rq, int L, const uint8_t* s, int len, int32_t orig) {
  std::vector<uint32_t> seq_w((size_t)kIrSeqMax / 4 + 4, 0), hot_w((size_t)kIrReadMax / 4, 0), q_w((size_t)kIrReadMax / 4, 0);
  for (int p = 0; p < len; ++p) seq_w[(size_t)p >> 2] |= ir_mask(s[p]) << (8 * (p & 3));
  for (int i = 0; i < L; ++i) hot_w[(size_t)i >> 2] |= ir_hot(rc[i]) << (8 * (i & 3)), q_w[(size_t)i >> 2] |= (uint32_t)rq[i] << (8 * (i & 3));
  uint32_t so = 0;
  for (int i = 0; i < L; ++i) {
    const int64_t p = (int64_t)orig + i;
    if (p >= len) so += kIrOverhang;
    else if ((seq_w[(size_t)p >> 2] >> (8 * (p & 3))) & (hot_w[(size_t)i >> 2] >> (8 * (i & 3))) & 0xFFu) so += rq[i];
  }
  uint64_t key = ir_key(so, true, orig);
  const int steps = (L + 3) / 4, n_off = (int)ir_offsets(len, L);
  for (int o = 0; o < n_off; ++o) {
    uint32_t below = seq_w[(size_t)o >> 2], acc = 0;
    for (int j = 0; j < steps; ++j) {
      const uint32_t above = seq_w[((size_t)o >> 2) + (size_t)j + 1];
      const uint32_t t = align_byte(above, below, (uint32_t)o & 3u) & hot_w[(size_t)j];
      acc = dot4(((t + 0x7F7F7F7Fu) >> 7) & 0x01010101u, q_w[(size_t)j], acc);
      below = above;
    }
    const uint64_t k = ir_key(acc, false, o);
    if (k < key) key = k;
  }
  return key;
}

}  // namespace

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1;
  const int n_bins = argc > 2 ? std::atoi(argv[2]) : 20;
  int bad = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b)
      if (((ir_hot(a) & ir_mask(b)) != 0) != ir_differ(a, b)) std::printf("MISMATCH codes %d %d\n", a, b), ++bad;
  for (int c = 0; c < 256; ++c) {
    const int want = c == 'A' || c == 'a' ? 0 : c == 'C' || c == 'c' ? 1 : c == 'G' || c == 'g' ? 2 : c == 'T' || c == 't' ? 3 : 4;
    if (ir_code((uint8_t)c) != want) std::printf("MISMATCH code of byte %d\n", c), ++bad;
  }
  std::mt19937 rng(seed);
  auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  int64_t pairs = 0, alt = 0, cons = 0, cleaned = 0, updates = 0;
  IrParams prm;
  for (int b = 0; b < n_bins; ++b) {
    IrBin bin;
    const int W = pick(80, 400);
    bin.lo = pick(0, 1000), bin.hi = bin.lo + W;
    bin.ref.resize((size_t)W);
    for (auto& x : bin.ref) x = (uint8_t)(rng() % 64 == 0 ? 4 : rng() % 4);
    // the planted indel, and a haplotype that carries it
    IrIndel d;
    d.k = pick(1, 8), d.ins = rng() % 2, d.a = pick(35, W - 45);
    for (int i = 0; i < d.k; ++i) d.bases.push_back((uint8_t)(rng() % 4));
    std::vector<uint8_t> hap(bin.ref.begin(), bin.ref.begin() + d.a);
    if (d.ins) hap.insert(hap.end(), d.bases.begin(), d.bases.end());
    hap.insert(hap.end(), bin.ref.begin() + d.a + (d.ins ? 0 : d.k), bin.ref.end());
    const int n_reads = pick(0, 24);
    for (int i = 0; i < n_reads; ++i) {
      IrRead r;
      const int L = pick(1, 60);
      const int o = pick(30, std::max(30, (int)hap.size() - L - 30));
      for (int t = 0; t < L; ++t) r.codes.push_back(o + t < (int)hap.size() ? hap[(size_t)(o + t)] : (uint8_t)0), r.quals.push_back((uint8_t)pick(0, 60));
      if (rng() % 8 == 0) r.codes[(size_t)pick(0, L - 1)] = (uint8_t)(rng() % 5);
      r.duplicate = rng() % 10 == 0;
      const bool spans = o + 1 < d.a && o + L > d.a + (d.ins ? d.k : 0) + 1;
      if (spans && rng() % 2) {  // aligned with the indel
        const int m1 = d.a - o;
        r.start = bin.lo + o;
        if (d.ins) r.cigar = {ir_pack((uint32_t)m1, kIrM), ir_pack((uint32_t)d.k, kIrI), ir_pack((uint32_t)(L - m1 - d.k), kIrEq)};
        else r.cigar = {ir_pack((uint32_t)m1, kIrM), ir_pack((uint32_t)d.k, kIrD), ir_pack((uint32_t)(L - m1), kIrM)};
      } else {  // aligned without it, where its left end lies
        r.start = bin.lo + (o <= d.a ? o : d.ins ? std::max(o - d.k, d.a) : o + d.k);
        r.cigar = {ir_pack((uint32_t)L, kIrM)};
      }
      if (r.start + L + d.k + 1 >= bin.hi) continue;
      bin.reads.push_back(r);
    }
    if (rng() % 3 == 0) {
      IrKnown kn;
      kn.pos = bin.lo + d.a, kn.indel = d;
      bin.known.push_back(kn);
    }
    const IrPlan plan = ir_prepare(bin, prm);
    if (plan.skip || plan.cons.empty() || plan.alt.empty()) continue;
    IrBatch batch;
    batch.add(bin, plan);
    const fcsir_batch v = batch.view();
    std::vector<uint32_t> best((size_t)batch.pairs());
    std::vector<int32_t> off((size_t)batch.pairs());
    ir_score_host(v, 2, best.data(), off.data());
    for (int64_t c = 0; c < v.n_seq; ++c)
      for (int64_t r = 0; r < v.n_reads; ++r) {
        const uint64_t key = kernel_best(v.read + v.read_off[r], v.qual + v.read_off[r], (int)(v.read_off[r + 1] - v.read_off[r]),
                                         v.seq + v.seq_off[c], (int)(v.seq_off[c + 1] - v.seq_off[c]), v.orig[r]);
        const int64_t p = c * v.n_reads + r;
        if (ir_key_score(key) != best[(size_t)p] || ir_key_offset(key) != off[(size_t)p])
          std::printf("MISMATCH bin %d pair %lld: %u at %d, the kernel's arithmetic gives %u at %d\n", b, (long long)p, best[(size_t)p],
                      off[(size_t)p], ir_key_score(key), ir_key_offset(key)), ++bad;
      }
    pairs += batch.pairs(), alt += (int64_t)plan.alt.size(), cons += (int64_t)plan.cons.size();
    const std::vector<IrUpdate> ups = ir_decide(bin, plan, prm, best.data(), off.data());
    cleaned += !ups.empty(), updates += (int64_t)ups.size();
    for (const IrUpdate& u : ups) {
      int64_t q = 0, m = 0;
      for (const uint32_t cw : u.cigar) {
        if (ir_op(cw) != kIrD) q += ir_len(cw);
        if (ir_op(cw) == kIrM) m += ir_len(cw);
      }
      if (q != (int64_t)bin.reads[(size_t)u.read].codes.size() || m == 0 || u.start < bin.lo || u.start >= bin.hi)
        std::printf("MISMATCH bin %d: the update of read %d\n", b, u.read), ++bad;
    }
  }
  std::printf("pairs %lld alt %lld consensuses %lld cleaned %lld updates %lld %s\n", (long long)pairs, (long long)alt, (long long)cons,
              (long long)cleaned, (long long)updates, bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
