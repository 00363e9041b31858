// The pileup in front of htc's and mutect2's PairHMM (caller.h): one walk over
// a window's reads gives every locus its depth, its mismatch and indel events,
// the alleles the reads carry and, in GVCF mode, the reference model's three
// sums; the active sites and the alleles at least two reads support come from
// those.  The walk has two parts:
//
//   per base      M / = / X bases and the depth of D spans: depth, the mismatch
//                 events, the SNV events and gl.  Its decisions are
//                 csrc/pu_rules.h, shared with the device kernels
//                 (csrc/pileup.hip, include/fcspu.h).
//   per CIGAR op  the indel alleles, their events at the anchor and the
//                 contig-end test of deletions.  Cheap; host code in both paths.
//
// build_pileup does both in one walk: the host path, and the oracle of the
// device's.  pileup_window_device sends the per-base part to fcspu_pile in
// chunks of loci and keeps the per-op part here.
#pragma once

#include <cstdint>
#include <string>
#include <string_view>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "fcspu.h"
#include "hugebuf.h"

namespace fcsg {

// A read of the window: its CIGAR, bases, qualities and BI / BD strings live
// in the window's HugeSlab (no per-read heap blocks).
template <typename T>
struct View {
  const T* p = nullptr;
  size_t n = 0;
  const T* begin() const { return p; }
  const T* end() const { return p + n; }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
  const T& operator[](size_t i) const { return p[i]; }
};
struct Read {
  int32_t pos = 0;
  int64_t end = 0;
  View<uint32_t> cigar;
  std::string_view seq;
  View<uint8_t> qual;
  int mapq = 0;
  std::string_view bi, bd;
};
static_assert(std::is_trivially_copyable_v<Read>, "Read lives in a HugeVec");

struct Allele {
  int64_t pos;  // 0-based anchor
  std::string ref, alt;
  bool operator<(const Allele& o) const { return std::tie(pos, ref, alt) < std::tie(o.pos, o.ref, o.alt); }
  int64_t ref_end() const { return pos + (int64_t)ref.size(); }
};

struct Pileup {
  int64_t wb = 0;
  HugeArray<int> depth, events;
  // allele events of the reads — SNVs as packed (pos, ref, alt) keys, indels
  // as Alleles — then (finish_support) sorted and counted: the support of
  // each distinct allele in (pos, ref, alt) order
  HugeVec<uint64_t> snv_events;
  std::vector<Allele> indel_events;
  // SNV keys already counted (at least two reads each), ascending: the device's chunks
  std::vector<std::pair<uint64_t, int>> snv_counted;
  std::vector<std::pair<Allele, int>> support;
  // GVCF reference model: per position, sum over bases of log10 P(base | 0/0,
  // 0/1, 1/1) with 1 = <NON_REF> (any other base)
  HugeArray<double> gl;  // 3 per position; empty unless GVCF
};

// log10 P(base | genotype) per base quality: [q][0] ref base under 0/0 (1 - e),
// [q][1] any base under 0/1 (0.5 (1 - e) + 0.5 e / 3), [q][2] non-ref base
// under 0/0 (e / 3); a ref base under 1/1 is e / 3, a non-ref base 1 - e.
struct RefModel {
  double t[FCSPU_TABLE_ROWS][3];
  RefModel();
};
const RefModel& ref_model();

inline uint64_t snv_key(int64_t pos, char ref, char alt) {
  return ((uint64_t)pos << 16) | ((uint64_t)(uint8_t)ref << 8) | (uint8_t)alt;
}

// Walks every read's CIGAR once, both parts: depth, mismatch / indel events and
// allele events over the whole window of pu.  ref is the contig.
void build_pileup(const std::string& ref, const Read* reads, size_t n, int min_bq, Pileup& pu);

// The per-base part alone over loci [lo, hi) of pu's window; ref_window holds
// the window's reference letters (locus p at ref_window[p - pu.wb]).
void pileup_bases(const char* ref_window, const Read* reads, size_t n, int min_bq, int64_t lo, int64_t hi, Pileup& pu);

// The per-op part alone over the whole window of pu.
void pileup_ops(const std::string& ref, const Read* reads, size_t n, Pileup& pu);

// The loci of [lo, hi) where pu's events and depth meet the site predicate, appended in order.
void active_sites(const Pileup& pu, int64_t lo, int64_t hi, double frac, std::vector<int64_t>& sites);

// The distinct alleles of the pileup's events seen in at least two reads
// (the least support a candidate allele needs), with their read counts, in
// (pos, ref, alt) order.
void finish_support(Pileup& pu);

// The host statement of fcspu_pile's results over its arguments (the oracle
// of the device path; exported by capi.cpp): the per-base part of every batch,
// the sites of batch 0 with events_in, the SNVs of all batches.  The table is
// ref_model()'s.  Throws when a maximum is too small.
void pileup_host(const fcspu_batch* batches, int n_batches, const fcspu_params& prm, const fcspu_window& w, const uint8_t* ref,
                 const int32_t* events_in, const fcspu_out& out);

// The per-op part's events of a batch over the window (the events_in of batch
// 0), added to events[len]; contig is the window's whole contig.
void pileup_ops_host(const fcspu_batch& batch, const fcspu_window& w, const std::string& contig, int32_t* events);

struct PileupRunStats {
  int64_t gpu_chunks = 0, host_chunks = 0;
  double device_seconds = 0;  // inside fcspu_pile
  double flatten_seconds = 0;
};

// Whether the loaded libfcship has the fcspu_pile entry point.
bool gpu_pileup_available();

// The window of pu (depth, events and gl zeroed) piled up with the per-base
// part on `device`, in chunks of chunk_bp loci: reads[0 .. n_sets) are the
// window's reads in coordinate order (the tumor's, then the normal's), flattened
// once and viewed per chunk.  Leaves in pu and in `sites` what build_pileup of
// reads[0], active_sites and build_pileup of reads[1] leave, with the SNVs
// counted already.  A chunk with a read letter the device does not count
// (an IUPAC code), or a record that reaches beyond its contig, takes the host's
// per-base part.  `command` names the caller in errors.
void pileup_window_device(int device, int64_t chunk_bp, const std::string& ref, int32_t ref_id, const HugeVec<Read>* reads,
                          int n_sets, int min_bq, double frac, Pileup& pu, std::vector<int64_t>& sites, PileupRunStats& st,
                          const char* command);

}  // namespace fcsg
