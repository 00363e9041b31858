// Minimizer seeding and chaining, the aligner's second seeder (DESIGN §2 [EXT]
// "minimizer seeding and chaining"; the front end of the reference's
// minimap-flow, /root/reference/src/workers/Minimap2Worker.cpp).  The sketch, the
// in-memory index, the anchors of a read, the host statement of the chaining
// recurrence (the oracle of include/fcsmm.h's kernel) and the backtrack that
// both paths share.  The rules common with the device are csrc/mm_rules.h.
// [EXT] minimap2 is not vendored, so this is a restatement (parity unpinned
// against minimap2 itself); DESIGN §9 lists where it knowingly differs.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "fcsmm.h"

namespace fcsg {

struct MmOptions {
  int k = 21, w = 11;    // minimap.k, minimap.w
  int max_occ = 500;     // minimap.max_occ: a minimizer with more occurrences yields no anchors
  int max_gap = 100;     // minimap.max_gap
  int bw = 50;           // minimap.bw
  int min_cnt = 2;       // minimap.min_cnt: anchors of a kept chain
  int min_score = 20;    // minimap.min_score
};
// throws invalidParam outside the rules' ranges
void mm_check_options(const MmOptions& o);

// A selected k-mer: its hash, the position of its last base and its strand
// (0: the forward k-mer is the canonical one).
struct MmMini {
  uint64_t h;
  int32_t pos;
  uint8_t strand;
};

// The minimizers of n codes (0 .. 3 for A C G T, anything else restarts the
// k-mer) in ascending position, appended to out.  1 <= k <= 31, 1 <= w <= 256.
void mm_sketch(const uint8_t* codes, int64_t n, int k, int w, std::vector<MmMini>& out);

// hash -> occurrences (contig, position of the last base, strand), built in
// memory from the contigs' codes.
class MmIndex {
 public:
  MmIndex(const std::vector<std::vector<uint8_t>>& contigs, int k, int w, int threads = 1);
  int k() const { return k_; }
  int w() const { return w_; }
  size_t size() const { return keys_.size(); }
  // the occurrences of h in (contig, position) order: contig << 33 | pos << 1 | strand
  const uint64_t* find(uint64_t h, size_t& n) const;

 private:
  int k_, w_;
  std::vector<uint64_t> keys_, vals_;
};

// The anchors (t, q) of a read of L codes sorted by (t, q), and the read's
// frac_rep: the fraction of its bases under minimizers with more than max_occ
// occurrences.
void mm_read_anchors(const MmIndex& idx, const uint8_t* codes, int L, int max_occ, std::vector<int64_t>& t,
                     std::vector<int32_t>& q, double& frac_rep);

// The recurrence over a batch in host memory (fcsmm_chain's arguments and
// checks; throws invalidParam where it refuses).
void mm_chain_host(const fcsmm_batch& b, int threads, int32_t* f, int32_t* p);

struct MmChain {
  int32_t score = 0;
  std::vector<int32_t> anchors;  // indices within the read, ascending
};
// The kept chains of one read's n anchors, in the order their heads are taken.
void mm_backtrack(const int32_t* f, const int32_t* p, int n, int min_cnt, int min_score, std::vector<MmChain>& out);

}  // namespace fcsg
