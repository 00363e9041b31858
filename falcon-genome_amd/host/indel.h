// Indel realignment on the host (DESIGN §2 [EXT] "RealignerTargetCreator and
// IndelRealigner, round 22", §4.14): the targets, left alignment, and clean(bin)
// around the scoring step.  ir_prepare (steps 1 and 2: the reads classified and
// the consensuses collected) and ir_decide (steps 4 to 8: the best consensus,
// the new alignments and the column check) are shared by both paths; only step
// 3, the score of every (consensus, alt read) pair, has two implementations:
// ir_score_host here, the oracle, and fcsir_score (include/fcsir.h).  The rules
// both share are csrc/ir_rules.h.  Nothing here knows a BAM record: a read is
// its start, its CIGAR without clips, its codes and its qualities.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "fcsir.h"

namespace fcsg {

constexpr int kIrTargetMax = 500;  // a merged target longer than this is dropped
constexpr int kIrPad = 30;         // the window beyond the reads' spans

// BAM CIGAR words (bam.h's packing), restated so that this file stands without bam.h.
enum IrOp : uint32_t { kIrM = 0, kIrI = 1, kIrD = 2, kIrN = 3, kIrS = 4, kIrH = 5, kIrP = 6, kIrEq = 7, kIrX = 8 };
inline uint32_t ir_pack(uint32_t len, uint32_t op) { return (len << 4) | op; }
inline uint32_t ir_len(uint32_t c) { return c >> 4; }
inline uint32_t ir_op(uint32_t c) { return c & 0xf; }
inline bool ir_is_match(uint32_t op) { return op == kIrM || op == kIrEq || op == kIrX; }

struct IrParams {
  int max_reads = 20000, max_consensuses = 30, max_isize = 3000, lod_tenths = 50;
};

// ------------------------------------------------------------------ targets
struct IrInterval {
  int32_t ref;
  int64_t start, end;  // 0-based half-open
};
// The events of a record's CIGAR at pos: [p - 1, p + 1) for an I between p - 1 and p, [d - 1, d + k) for a D over [d, d + k).
void ir_cigar_events(int32_t ref, int64_t pos, const std::vector<uint32_t>& cigar, std::vector<IrInterval>& out);
// Sorted; events that overlap or abut merged; a merged target longer than kIrTargetMax dropped.
std::vector<IrInterval> ir_merge_targets(std::vector<IrInterval> events);
// chr:start-end, 1-based closed, chr:pos for one base.
std::string ir_target_text(const std::string& chrom, const IrInterval& t);

// ------------------------------------------------------------------ left alignment
// A one-indel alignment aM kI bM or aM kD bM.
struct IrIndel {
  int a = 0, k = 0;
  bool ins = false;
  std::vector<uint8_t> bases;  // the inserted codes
};
// The indel of a one-indel CIGAR (= and X count as M), its inserted codes taken from the read; false for any other CIGAR.
bool ir_one_indel(const std::vector<uint32_t>& cigar, const std::vector<uint8_t>& codes, IrIndel& out);
// Moves the indel left while a > 1 and the spelled sequence stays the same; ref[at + a] is the reference code after the first M run.
void ir_left_align(const uint8_t* ref, int64_t at, IrIndel& d);

// ------------------------------------------------------------------ a bin
struct IrRead {
  int64_t start = 0;            // on the contig
  std::vector<uint32_t> cigar;  // without S and H
  std::vector<uint8_t> codes, quals;
  bool duplicate = false;
};
struct IrKnown {
  int64_t pos = 0;  // a deletion of the contig's [pos, pos + k); an insertion before pos
  IrIndel indel;    // a is not used
};
struct IrBin {
  int64_t lo = 0, hi = 0;           // the window
  std::vector<uint8_t> ref;         // its codes
  std::vector<IrRead> reads;        // the cleanable records, in order
  std::vector<IrKnown> known;       // in VCF order
};
struct IrConsensus {
  std::vector<uint8_t> seq;
  int u = 0, k = 0;  // the indel at window offset u
  bool ins = false;
};
struct IrPlan {
  bool skip = false;                  // the bin is left untouched
  std::vector<std::vector<uint32_t>> cigar;  // per read: its CIGAR, left-aligned where it had the one-indel form
  std::vector<int> alt;               // the alt reads
  std::vector<uint32_t> raw, aligner; // per alt read
  int64_t total_raw = 0;
  std::vector<IrConsensus> cons;
};
IrPlan ir_prepare(const IrBin& bin, const IrParams& p);

struct IrUpdate {
  int read = 0;  // index into the bin's reads
  int64_t start = 0;
  std::vector<uint32_t> cigar;  // without clips
  int nm = 0;                   // differing M bases plus I and D lengths
};
// best, off: cons.size() x alt.size(), consensus-major.  The updates in read order; none when the bin does not change.
std::vector<IrUpdate> ir_decide(const IrBin& bin, const IrPlan& plan, const IrParams& p, const uint32_t* best, const int32_t* off);

// ------------------------------------------------------------------ the scoring step
// Plans flattened into the arrays of an fcsir_batch.
struct IrBatch {
  std::vector<uint8_t> seq, read, qual;
  std::vector<int64_t> seq_off{0}, bin_seq{0}, read_off{0}, bin_read{0}, pair_first{0};
  std::vector<int32_t> orig;
  void clear();
  void add(const IrBin& bin, const IrPlan& plan);
  int64_t pairs() const { return pair_first.back(); }
  fcsir_batch view() const;
};
// The oracle: best and off of every pair by csrc/ir_rules.h's plain statement, bins spread over threads.
void ir_score_host(const fcsir_batch& b, int threads, uint32_t* best, int32_t* off);

}  // namespace fcsg
