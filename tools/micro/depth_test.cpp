// Host check of csrc/dp_runs.h (the text the gfx950 kernels of csrc/depth.hip
// run): random batches go through the header's functions the way the kernels
// call them (a record in passes of 64 lanes: the span, each lane's site and
// window offset, the ballot, the neighbours' offsets, +1 / -1 at the run ends,
// then the scan; a piece's bins and the quantile predicate over their running
// sums) and every depth and every summary is compared with host/depth.cpp,
// which states the rules with plain loops.
//   g++ -O1 -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude -Ifalcon-genome_amd/csrc -Ifalcon-genome_amd/host tools/micro/depth_test.cpp \
//       falcon-genome_amd/host/depth.cpp -o depth_test
//   depth_test [SEED [RECORDS]]
// Prints the batch's figures and "ok", or MISMATCH lines and exit status 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "depth.h"
#include "dp_runs.h"

using namespace fcsg;
using namespace fcs;

namespace {

constexpr int64_t kContig = 6000;

struct Batch {
  std::vector<uint16_t> flag;
  std::vector<int32_t> ref_id, pos;
  std::vector<uint8_t> mapq, absent, qual;
  std::vector<uint32_t> cigar;
  std::vector<int64_t> cigar_off{0}, base_off{0};
  fcsdp_batch view() const {
    fcsdp_batch b;
    b.n = (int64_t)flag.size();
    b.flag = flag.data(), b.ref_id = ref_id.data(), b.pos = pos.data(), b.mapq = mapq.data();
    b.cigar = cigar.data(), b.cigar_off = cigar_off.data(), b.n_cigar = (int64_t)cigar.size();
    b.bases = nullptr, b.qual = qual.data(), b.base_off = base_off.data(), b.n_bases = (int64_t)qual.size();
    b.qual_absent = absent.data();
    return b;
  }
};

void add_record(std::mt19937_64& rnd, Batch& b) {
  static const int lengths[] = {1, 2, 15, 63, 64, 65, 127, 128, 129, 151, 151, 200};
  static const uint8_t quals[] = {0, 2, 5, 9, 10, 11, 25, 30, 31, 37, 40, 41};
  static const uint16_t flags[] = {0, 0, 0, 0x10, 0x41, 0x91, 0x800, 0x4, 0x100, 0x200, 0x400};
  static const uint8_t mapqs[] = {0, 19, 20, 30, 60, 60, 255};
  int left = lengths[rnd() % 12];
  const int32_t pos = (int32_t)(rnd() % (kContig - 900));
  if (rnd() % 10 == 0) b.cigar.push_back((5u << 4) | 5u);
  int bases = 0;
  if (left > 12 && rnd() % 4 == 0) {
    const int lead = (int)(rnd() % 9) + 1;
    b.cigar.push_back(((uint32_t)lead << 4) | 4u);
    left -= lead, bases += lead;
  }
  const int trail = left > 12 && rnd() % 4 == 0 ? (int)(rnd() % 7) + 1 : 0;
  left -= trail;
  bool first = true;
  int gaps = 0;
  while (left > 0) {
    if (!first && gaps++ < 8) {  // at most 8 gaps: the span stays inside the contig
      const unsigned gap = (unsigned)(rnd() % 10);
      if (gap < 3) b.cigar.push_back(((uint32_t)(1 + rnd() % 5) << 4) | 2u);
      else if (gap < 4) b.cigar.push_back(((uint32_t)(1 + rnd() % 40) << 4) | 3u);
      else if (gap < 5) b.cigar.push_back((1u << 4) | 6u);
      else if (gap < 8 && left > 1) {
        const int n = 1 + (int)(rnd() % (unsigned)std::min(left - 1, 7));
        b.cigar.push_back(((uint32_t)n << 4) | 1u);
        left -= n, bases += n;
      }
    }
    const int n = rnd() % 2 ? left : 1 + (int)(rnd() % (unsigned)left);
    static const uint32_t mops[] = {0, 0, 0, 7, 8};
    b.cigar.push_back(((uint32_t)n << 4) | mops[rnd() % 5]);
    left -= n, bases += n;
    first = false;
  }
  if (trail) b.cigar.push_back(((uint32_t)trail << 4) | 4u), bases += trail;
  const bool absent = rnd() % 30 == 0;
  for (int i = 0; i < bases; ++i) b.qual.push_back(absent ? 0xff : quals[rnd() % 12]);
  b.flag.push_back(flags[rnd() % 11]);
  b.ref_id.push_back((int32_t)(rnd() % 2));
  b.pos.push_back(pos);
  b.mapq.push_back(mapqs[rnd() % 7]);
  b.absent.push_back(absent);
  b.cigar_off.push_back((int64_t)b.cigar.size());
  b.base_off.push_back((int64_t)b.qual.size());
}

// dp_runs_kernel and the scan, lane by lane.
void count_shared(const fcsdp_batch& b, const fcsdp_params& prm, const fcsdp_window& w, std::vector<uint32_t>& depth,
                  int64_t& run_ends) {
  std::vector<int32_t> cells((size_t)w.len + 1, 0);
  for (int64_t r = 0; r < b.n; ++r) {
    if (b.ref_id[r] != w.ref_id) continue;
    const uint32_t* cigar = b.cigar + b.cigar_off[r];
    const int64_t n_ops = b.cigar_off[r + 1] - b.cigar_off[r], L = b.base_off[r + 1] - b.base_off[r];
    if (!dp_counted(b.flag[r], b.ref_id[r], n_ops, b.mapq[r], prm.min_mapq, prm.max_mapq)) continue;
    int64_t covered, ref_len;
    cigar_span(cigar, n_ops, covered, ref_len);
    if (covered != L) continue;
    const bool absent = b.qual_absent[r] != 0;
    const uint8_t* qual = b.qual + b.base_off[r];
    for (int64_t i0 = 0; i0 < L; i0 += 64) {
      int32_t off[64];
      unsigned long long counted = 0;
      for (int lane = 0; lane < 64; ++lane) {
        const int64_t i = i0 + lane;
        int64_t p;
        off[lane] = -1;
        if (i < L && cigar_site(cigar, n_ops, b.pos[r], i, p) && p >= 0 && p < w.contig_len &&
            dp_base_ok(absent ? 0 : qual[i], prm.min_baseq, prm.max_baseq))
          off[lane] = dp_in_window(p, w.start, w.len, w.contig_len);
        if (off[lane] >= 0) counted |= 1ull << lane;
      }
      for (int lane = 0; lane < 64; ++lane) {
        if (dp_run_first(lane, counted, off[lane], lane ? off[lane - 1] : -1)) ++cells[(size_t)off[lane]], ++run_ends;
        if (dp_run_last(lane, counted, off[lane], lane < 63 ? off[lane + 1] : -1)) --cells[(size_t)off[lane] + 1], ++run_ends;
      }
    }
    if (prm.include_deletions) {
      int64_t p = b.pos[r];
      for (int64_t k = 0; k < n_ops; ++k) {
        const uint32_t op = cigar[k] & 15u;
        const int64_t len = cigar[k] >> 4;
        if (op == 2u) {
          const int64_t lo = std::max<int64_t>(std::max(p, w.start), 0), hi = std::min(std::min(p + len, w.start + w.len), w.contig_len);
          if (lo < hi) ++cells[(size_t)(lo - w.start)], --cells[(size_t)(hi - w.start)];
        }
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) p += len;
      }
    }
  }
  int32_t run = 0;
  for (int64_t i = 0; i < w.len; ++i) run += cells[(size_t)i], depth[(size_t)i] += (uint32_t)run;
}

// dp_stats_kernel's piece, bin by bin.
fcsdp_summary piece_shared(const uint32_t* depth, const uint64_t* bitmap, const fcsdp_piece& p, uint64_t* hist) {
  uint32_t bins[kDpBins] = {0};
  fcsdp_summary s{};
  for (int64_t i = p.start; i < p.end; ++i) {
    if (!((bitmap[i >> 6] >> (i & 63)) & 1u)) continue;
    ++bins[dp_bin(depth[i])];
    s.total += depth[i], ++s.loci, s.above += depth[i] >= (uint32_t)kDpAbove;
  }
  s.q1 = s.median = s.q3 = 1;
  uint64_t cum = 0;
  for (int bin = 0; bin < kDpBins; ++bin) {
    if (bins[bin] && s.loci)
      for (int k = 1; k <= 3; ++k)
        if (dp_is_quantile(cum, cum + bins[bin], s.loci, k)) (k == 1 ? s.q1 : k == 2 ? s.median : s.q3) = dp_reported(bin);
    cum += bins[bin];
    hist[bin] += bins[bin];
  }
  return s;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
  const int n = argc > 2 ? std::atoi(argv[2]) : 3000;
  std::mt19937_64 rnd(seed);
  Batch batch;
  for (int r = 0; r < n; ++r) add_record(rnd, batch);
  const fcsdp_batch b = batch.view();
  int bad = 0;
  int64_t counted_bases = 0, run_ends = 0, loci = 0;
  const fcsdp_params prms[] = {{-1, 2147483647, -1, 127, 0}, {20, 60, 10, 40, 1}, {-1, 2147483647, 1, 127, 1}};
  const fcsdp_window windows[] = {{0, 0, 0, kContig, kContig}, {1, 0, 1000, 4096, kContig}, {0, 0, 63, 65, kContig},
                                  {1, 0, kContig - 1, 1, kContig}};
  for (const fcsdp_params& prm : prms)
    for (const fcsdp_window& w : windows) {
      std::vector<uint32_t> want((size_t)w.len, 0), got((size_t)w.len, 0);
      depth_count_host(b, prm, w, want.data(), 1);
      std::vector<uint32_t> want4((size_t)w.len, 0);
      depth_count_host(b, prm, w, want4.data(), 4);
      count_shared(b, prm, w, got, run_ends);
      for (int64_t i = 0; i < w.len; ++i) {
        counted_bases += want[(size_t)i];
        if ((want[(size_t)i] != got[(size_t)i] || want[(size_t)i] != want4[(size_t)i]) && bad++ < 10)
          std::printf("MISMATCH depth at %lld of window %lld+%lld: host %u (4 threads %u), shared %u\n", (long long)i,
                      (long long)w.start, (long long)w.len, want[(size_t)i], want4[(size_t)i], got[(size_t)i]);
      }
      // the window's loci as pieces of several lengths, every fifth locus left out
      std::vector<uint64_t> bitmap((size_t)(w.len + 63) / 64 + 1, 0);
      for (int64_t i = 0; i < w.len; ++i)
        if (i % 5 != 3) bitmap[(size_t)(i >> 6)] |= (uint64_t)1 << (i & 63);
      std::vector<fcsdp_piece> pieces;
      static const int lens[] = {1, 63, 64, 65, 255, 256, 257, 1000};
      for (int64_t s = 0, k = 0; s < w.len; ++k) {
        const int64_t e = std::min<int64_t>(w.len, s + lens[k % 8]);
        pieces.push_back({(int32_t)s, (int32_t)e, -1, 0});
        s = e;
      }
      std::vector<fcsdp_summary> sum(pieces.size());
      std::vector<uint64_t> hist(kDpBins, 0), hist2(kDpBins, 0);
      depth_stats_host(want.data(), bitmap.data(), w.len, pieces.data(), (int64_t)pieces.size(), 0, hist.data(), nullptr,
                       sum.data(), 2);
      for (size_t k = 0; k < pieces.size(); ++k) {
        const fcsdp_summary s = piece_shared(want.data(), bitmap.data(), pieces[k], hist2.data());
        loci += s.loci;
        if ((s.total != sum[k].total || s.loci != sum[k].loci || s.above != sum[k].above || s.q1 != sum[k].q1 ||
             s.median != sum[k].median || s.q3 != sum[k].q3) && bad++ < 10)
          std::printf("MISMATCH piece %zu: host %llu %u %u %u %u %u, shared %llu %u %u %u %u %u\n", k,
                      (unsigned long long)sum[k].total, sum[k].loci, sum[k].above, sum[k].q1, sum[k].median, sum[k].q3,
                      (unsigned long long)s.total, s.loci, s.above, s.q1, s.median, s.q3);
      }
      if (hist != hist2 && bad++ < 10) std::printf("MISMATCH sample histogram\n");
    }
  std::printf("records %d counted_bases %lld run_ends %lld loci %lld\n", n, (long long)counted_bases, (long long)run_ends,
              (long long)loci);
  if (bad) return 1;
  std::printf("ok\n");
  return 0;
}
