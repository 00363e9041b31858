// The indel command (indel_run.h).  Pass 1 collects the events of the CIGARs
// and of the known indels into targets.  Pass 2 gathers each target's cleanable
// records into a bin as the stream passes the target's end (bins complete in
// target order, since a record belongs to the first target it overlaps),
// prepares it, and scores and decides the prepared bins in calls of at most
// indel.chunk_pairs pairs (a bin is never split).  Pass 3 applies the table.
#include "indel_run.h"

#include <algorithm>
#include <cstdlib>
#include <deque>
#include <fstream>
#include <queue>
#include <unordered_map>

#include "bam_stream.h"
#include "bqsr_run.h"
#include "common.h"
#include "config.h"
#include "fcship.h"
#include "fcsir.h"
#include "flat_batch.h"
#include "indel.h"
#include "ir_rules.h"

namespace fcsg {

namespace {

struct IrApi {
  decltype(&fcsir_score) score = FCSG_DEVICE_ENTRY(fcsir_score);
};

const IrApi& ir_api() {
  static const IrApi A;
  return A;
}

constexpr size_t kChunkRecords = 1 << 16;

struct KnownSite {
  IrKnown known;
  int64_t ev0, ev1;  // its event
};

// A record's new place: by ordinal for the record itself, by (name, end) for its mate.
struct Moved {
  int32_t start = 0;
  int64_t end = 0;
  std::vector<uint32_t> cigar;  // with the clips
  int nm = 0;
  bool reverse = false;
};

// A bin on its way through pass 2: the cleanable records beside the reads made of them.
struct Pending {
  int32_t ref = 0;
  IrBin bin;
  IrPlan plan;
  std::vector<BamRecord> recs;
  std::vector<int64_t> ordinal;
  std::vector<std::pair<size_t, size_t>> clips;  // CIGAR words before and after the stripped part
};

bool mapped(const BamRecord& r) { return !(r.flag & kUnmapped) && r.ref_id >= 0 && r.pos >= 0; }

std::string mate_key(const BamRecord& r, bool other) {
  const int end = (r.flag & kRead1 ? 1 : 0) | (r.flag & kRead2 ? 2 : 0);
  const int k = other ? (end == 1 ? 2 : end == 2 ? 1 : 0) : end;
  return r.name + '\t' + (char)('0' + k);
}

// The stripped read of a cleanable record; false for a record that passes through untouched.
bool strip_read(const BamRecord& r, int max_isize, IrRead& out, std::pair<size_t, size_t>& clips) {
  if (!mapped(r) || (r.flag & (kSecondary | kSupplementary | kQcFail)) || r.mapq == 0 || r.seq.empty() || r.cigar.empty()) return false;
  if ((r.flag & kPaired) && !(r.flag & kMateUnmapped) && (r.next_ref_id != r.ref_id || std::abs((int64_t)r.tlen) > max_isize)) return false;
  size_t lead = 0, tail = r.cigar.size();
  int64_t lead_bases = 0, tail_bases = 0, query = 0;
  while (lead < tail && (cigar_op(r.cigar[lead]) == kS || cigar_op(r.cigar[lead]) == kH)) {
    if (cigar_op(r.cigar[lead]) == kS) lead_bases += cigar_len(r.cigar[lead]);
    ++lead;
  }
  while (tail > lead && (cigar_op(r.cigar[tail - 1]) == kS || cigar_op(r.cigar[tail - 1]) == kH)) {
    if (cigar_op(r.cigar[tail - 1]) == kS) tail_bases += cigar_len(r.cigar[tail - 1]);
    --tail;
  }
  for (size_t k = lead; k < tail; ++k) {
    const CigarOp op = cigar_op(r.cigar[k]);
    if (op == kN || op == kP || op == kS || op == kH) return false;
    if (op != kD) query += cigar_len(r.cigar[k]);
  }
  if (query < 1 || query > FCSIR_READ_MAX || lead_bases + query + tail_bases != (int64_t)r.seq.size()) return false;
  out.start = r.pos, out.duplicate = (r.flag & kDuplicate) != 0;
  out.cigar.assign(r.cigar.begin() + (std::ptrdiff_t)lead, r.cigar.begin() + (std::ptrdiff_t)tail);
  out.codes.resize((size_t)query), out.quals.assign((size_t)query, 0);
  const bool has_qual = r.qual.size() == r.seq.size();
  for (int64_t i = 0; i < query; ++i) {
    out.codes[(size_t)i] = (uint8_t)fcs::ir_code((uint8_t)r.seq[(size_t)(lead_bases + i)]);
    if (has_qual) out.quals[(size_t)i] = r.qual[(size_t)(lead_bases + i)];
  }
  clips = {lead, r.cigar.size() - tail};
  return true;
}

class Run {
 public:
  explicit Run(const IndelJob& job)
      : job_(job),
        device_(device_or_host(job.device, gpu_indel_available(),
                               "[fcs-genome indel] indel.gpu: the loaded libfcship has no fcsir_score entry point; "
                               "pairs are scored on the host\n")) {
    Config& cf = conf();
    prm_.max_reads = cf.get_int("indel.max_reads"), prm_.max_consensuses = cf.get_int("indel.max_consensuses");
    prm_.max_isize = cf.get_int("indel.max_isize"), prm_.lod_tenths = cf.get_int("indel.lod_tenths");
    chunk_pairs_ = cf.get_int("indel.chunk_pairs");
    if (prm_.max_reads < 1) throw invalidParam("indel.max_reads " + std::to_string(prm_.max_reads));
    if (prm_.max_consensuses < 1) throw invalidParam("indel.max_consensuses " + std::to_string(prm_.max_consensuses));
    if (prm_.max_isize < 0) throw invalidParam("indel.max_isize " + std::to_string(prm_.max_isize));
    if (chunk_pairs_ < 1) throw invalidParam("indel.chunk_pairs " + std::to_string(chunk_pairs_));
  }

  IndelRunStats run() {
    const uint64_t t0 = now_us();
    try {
      find_targets();
      if (!job_.targets_out.empty()) {
        std::string text;
        for (const IrInterval& t : targets_) text += ir_target_text(header_.names[(size_t)t.ref], t) + "\n";
        write_file(job_.targets_out, text);
      }
      clean_bins();
      write_output();
    } catch (...) {  // a refused run leaves no partial file
      remove_path(job_.output), remove_path(job_.output + ".bai");
      if (!job_.targets_out.empty()) remove_path(job_.targets_out);
      throw;
    }
    st_.targets = (int64_t)targets_.size();
    st_.on_device = device_ >= 0;
    st_.seconds = (now_us() - t0) / 1e6;
    return st_;
  }

 private:
  // ---------------------------------------------------------------- pass 1
  void load_known(const std::string& path) {
    known_sites_lines(path, [&](const std::string& line) {
      std::vector<std::string> f;
      for (size_t p = 0; f.size() < 5 && p <= line.size();) {
        const size_t e = std::min(line.find('\t', p), line.size());
        f.push_back(line.substr(p, e - p));
        p = e + 1;
      }
      if (f.size() < 5) throw formatError("known sites " + path + ": a record of fewer than 5 fields");
      const int c = header_.ref_index(f[0]);
      if (c < 0) return;
      int64_t pos;
      try {
        pos = std::stoll(f[1]);
      } catch (const std::logic_error&) {
        throw formatError("known sites " + path + ": POS of \"" + line.substr(0, std::min<size_t>(line.size(), 60)) + "\"");
      }
      const std::string &ref = f[3], &alt = f[4];
      if (pos < 1 || ref.empty() || alt.empty() || alt.find(',') != std::string::npos || ref.size() == alt.size()) return;
      if (std::min(ref.size(), alt.size()) != 1 || std::toupper((unsigned char)ref[0]) != std::toupper((unsigned char)alt[0])) return;
      if (alt[0] == '<' || alt[0] == '*' || alt[0] == '.') return;
      KnownSite k;
      k.known.pos = pos, k.known.indel.ins = alt.size() > ref.size();
      k.known.indel.k = (int)(std::max(ref.size(), alt.size()) - 1);
      if (k.known.indel.ins)
        for (size_t i = 1; i < alt.size(); ++i) k.known.indel.bases.push_back((uint8_t)fcs::ir_code((uint8_t)alt[i]));
      k.ev0 = pos - 1, k.ev1 = pos - 1 + (int64_t)ref.size();
      known_[(size_t)c].push_back(k);
      ++st_.known;
    });
  }

  void find_targets() {
    BamStream in(job_.input, true);
    header_ = in.header();
    contigs_ = header_contigs(job_.ref, header_, true);
    known_.resize(header_.names.size()), known_by_start_.resize(header_.names.size());
    for (const std::string& k : job_.known) load_known(k);
    std::vector<IrInterval> events;
    for (size_t c = 0; c < known_.size(); ++c) {
      for (size_t k = 0; k < known_[c].size(); ++k) {
        events.push_back({(int32_t)c, known_[c][k].ev0, known_[c][k].ev1});
        known_by_start_[c].emplace_back(known_[c][k].ev0, k);
      }
      std::sort(known_by_start_[c].begin(), known_by_start_[c].end());
    }
    std::vector<BamRecord> buf;
    for (;;) {
      buf.clear();
      if (in.read(buf, kChunkRecords) == 0) break;
      for (const BamRecord& r : buf)
        if (mapped(r) && !(r.flag & (kSecondary | kSupplementary | kDuplicate | kQcFail)) && r.mapq > 0)
          ir_cigar_events(r.ref_id, r.pos, r.cigar, events);
      if (interrupted()) throw interruptedError();
    }
    targets_ = ir_merge_targets(std::move(events));
    if (!job_.intervals.empty()) {
      const std::vector<GenomeInterval> keep = merged_intervals(job_.intervals, header_);
      std::vector<IrInterval> kept;
      size_t k = 0;
      for (const IrInterval& t : targets_) {
        while (k < keep.size() && (keep[k].ref < t.ref || (keep[k].ref == t.ref && keep[k].end <= t.start))) ++k;
        if (k < keep.size() && keep[k].ref == t.ref && keep[k].start < t.end) kept.push_back(t);
      }
      targets_.swap(kept);
    }
  }

  // ---------------------------------------------------------------- pass 2
  void clean_bins() {
    BamStream in(job_.input, true);
    std::vector<BamRecord> buf;
    std::deque<Open> open;  // the bins that still take records, in target order
    size_t t = 0;           // the first target that ends after the stream's position
    int64_t ordinal = 0;
    for (;;) {
      buf.clear();
      if (in.read(buf, kChunkRecords) == 0) break;
      for (BamRecord& r : buf) {
        const int64_t ord = ordinal++;
        if (r.ref_id < 0 || r.pos < 0) continue;
        while (t < targets_.size() && (targets_[t].ref < r.ref_id || (targets_[t].ref == r.ref_id && targets_[t].end <= r.pos))) ++t;
        // bins of targets the stream has passed take no more records
        while (!open.empty() && open.front().ref_target < t) close_bin(open);
        if (t == targets_.size() || targets_[t].ref != r.ref_id) continue;
        const int64_t end = std::max<int64_t>(r.end(), (int64_t)r.pos + 1);
        if (targets_[t].start >= end) continue;  // overlaps no target
        IrRead read;
        std::pair<size_t, size_t> clips;
        if (!strip_read(r, prm_.max_isize, read, clips)) continue;
        if (open.empty() || open.back().ref_target != t) {
          open.emplace_back();
          open.back().ref_target = t, open.back().p.ref = r.ref_id;
        }
        Pending& p = open.back().p;
        p.bin.reads.push_back(std::move(read)), p.clips.push_back(clips), p.ordinal.push_back(ord), p.recs.push_back(std::move(r));
      }
      if (interrupted()) throw interruptedError();
    }
    while (!open.empty()) close_bin(open);
    flush();
    st_.records = ordinal;
  }

  struct Open {
    size_t ref_target = 0;
    Pending p;
  };

  // The window, its codes and its known indels; the bin prepared and queued for scoring.
  void close_bin(std::deque<Open>& open) {
    Pending p = std::move(open.front().p);
    open.pop_front();
    ++st_.bins;
    const std::string& contig = contigs_[(size_t)p.ref];
    int64_t lo = INT64_MAX, hi = 0;
    for (const BamRecord& r : p.recs) lo = std::min<int64_t>(lo, r.pos), hi = std::max<int64_t>(hi, r.end());
    lo = std::max<int64_t>(0, lo - kIrPad), hi = std::min<int64_t>((int64_t)contig.size(), hi + kIrPad);
    p.bin.lo = lo, p.bin.hi = std::max(hi, lo);
    if (p.bin.hi - p.bin.lo <= FCSIR_SEQ_MAX) {
      p.bin.ref.resize((size_t)(p.bin.hi - p.bin.lo));
      for (int64_t x = lo; x < p.bin.hi; ++x) p.bin.ref[(size_t)(x - lo)] = (uint8_t)fcs::ir_code((uint8_t)contig[(size_t)x]);
      const auto& idx = known_by_start_[(size_t)p.ref];
      std::vector<size_t> in_window;
      for (auto it = std::lower_bound(idx.begin(), idx.end(), std::make_pair(lo + 1, (size_t)0)); it != idx.end() && it->first < p.bin.hi - 1; ++it)
        if (known_[(size_t)p.ref][it->second].ev1 <= p.bin.hi - 1) in_window.push_back(it->second);
      std::sort(in_window.begin(), in_window.end());  // VCF order
      for (const size_t k : in_window) p.bin.known.push_back(known_[(size_t)p.ref][k].known);
      p.plan = ir_prepare(p.bin, prm_);
    } else {
      p.plan.skip = true;
    }
    if (p.plan.skip || p.plan.cons.empty() || p.plan.alt.empty()) {
      st_.untouched += p.plan.skip;
      return;
    }
    const int64_t pairs = (int64_t)(p.plan.cons.size() * p.plan.alt.size());
    if (!queued_.empty() && batch_.pairs() + pairs > chunk_pairs_) flush();
    batch_.add(p.bin, p.plan);
    queued_.push_back(std::move(p));
  }

  // One scoring call over the queued bins, each then decided into the table.
  void flush() {
    if (queued_.empty()) return;
    const fcsir_batch view = batch_.view();
    const int64_t pairs = batch_.pairs();
    best_.resize((size_t)pairs), off_.resize((size_t)pairs);
    if (device_ >= 0) {
      int64_t n = 0;
      device_check(ir_api().score(device_, &view, best_.data(), off_.data(), pairs, &n), "indel", "fcsir_score");
    } else {
      ir_score_host(view, host_threads(), best_.data(), off_.data());
    }
    st_.pairs += pairs;
    for (size_t k = 0; k < queued_.size(); ++k) {
      Pending& p = queued_[k];
      st_.alt_reads += (int64_t)p.plan.alt.size();
      const int64_t first = batch_.pair_first[k];
      const std::vector<IrUpdate> ups = ir_decide(p.bin, p.plan, prm_, best_.data() + first, off_.data() + first);
      st_.cleaned += !ups.empty();
      for (const IrUpdate& u : ups) {
        const BamRecord& r = p.recs[(size_t)u.read];
        Moved m;
        m.start = (int32_t)u.start, m.nm = u.nm, m.reverse = (r.flag & kReverse) != 0;
        const auto [lead, tail] = p.clips[(size_t)u.read];
        m.cigar.assign(r.cigar.begin(), r.cigar.begin() + (std::ptrdiff_t)lead);
        m.cigar.insert(m.cigar.end(), u.cigar.begin(), u.cigar.end());
        m.cigar.insert(m.cigar.end(), r.cigar.end() - (std::ptrdiff_t)tail, r.cigar.end());
        m.end = u.start + cigar_ref_len(m.cigar);
        horizon_ = std::max<int64_t>(horizon_, std::abs(u.start - (int64_t)r.pos));
        if (r.flag & kPaired) by_mate_[mate_key(r, false)] = m;
        by_ordinal_[p.ordinal[(size_t)u.read]] = std::move(m);
        ++st_.realigned;
      }
    }
    queued_.clear(), batch_.clear();
  }

  // ---------------------------------------------------------------- pass 3
  struct Out {
    std::pair<int64_t, int64_t> key;
    int64_t ordinal;
    BamRecord rec;
  };
  struct Later {
    bool operator()(const Out& a, const Out& b) const { return std::tie(a.key, a.ordinal) > std::tie(b.key, b.ordinal); }
  };

  void apply(BamRecord& r, const Moved& m) {
    const std::string oc = cigar_string(r.cigar);
    const int32_t old_pos = r.pos;
    r.pos = m.start, r.cigar = m.cigar;
    r.mapq = (uint8_t)std::min<int>(r.mapq + 10, 254);
    r.set_aux_string("OC", oc);
    if (m.start != old_pos) r.set_aux_int("OP", old_pos + 1);
    int64_t nm;
    if (r.get_aux_int("NM", nm)) r.set_aux_int("NM", m.nm);
    r.remove_aux("MD"), r.remove_aux("UQ");
  }

  void fix_mate(BamRecord& r, bool self_moved) {
    if (!(r.flag & kPaired) || (r.flag & (kSecondary | kSupplementary))) return;
    const auto it = by_mate_.find(mate_key(r, true));
    const Moved* m = it == by_mate_.end() ? nullptr : &it->second;
    if (!m && !self_moved) return;
    std::string mc;
    const bool has_mc = r.get_aux_string("MC", mc);
    if (m) {
      r.next_pos = m->start;
      if (has_mc) r.set_aux_string("MC", cigar_string(m->cigar));
      ++st_.mates;
    }
    if (!mapped(r) || (r.flag & kMateUnmapped) || r.next_ref_id != r.ref_id) return;
    int64_t mate_start, mate_end;
    bool mate_rev;
    if (m) mate_start = m->start, mate_end = m->end, mate_rev = m->reverse;
    else if (has_mc) mate_start = r.next_pos, mate_end = r.next_pos + cigar_ref_len(parse_cigar(mc)), mate_rev = (r.flag & kMateReverse) != 0;
    else return;
    const int64_t self5 = (r.flag & kReverse) ? r.end() - 1 : r.pos, mate5 = mate_rev ? mate_end - 1 : mate_start;
    r.tlen = (int32_t)(mate5 - self5 + (mate5 >= self5 ? 1 : -1));
  }

  void write_output() {
    BamStream in(job_.input, true);
    BamWriter w(job_.output, header_);
    if (header_.text.find("SO:coordinate") != std::string::npos) w.index_on_close();
    std::priority_queue<Out, std::vector<Out>, Later> heap;
    std::vector<BamRecord> buf;
    int64_t ordinal = 0;
    for (;;) {
      buf.clear();
      if (in.read(buf, kChunkRecords) == 0) break;
      for (BamRecord& r : buf) {
        const int64_t ord = ordinal++;
        const std::pair<int64_t, int64_t> here = key_of(r.ref_id, r.pos);
        const auto it = by_ordinal_.find(ord);
        if (it != by_ordinal_.end()) apply(r, it->second);
        fix_mate(r, it != by_ordinal_.end());
        heap.push(Out{key_of(r.ref_id, r.pos), ord, std::move(r)});
        // no later record comes out before (here.first, here.second - horizon)
        const std::pair<int64_t, int64_t> safe{here.first, here.second - horizon_};
        while (!heap.empty() && heap.top().key < safe) w.write(heap.top().rec), heap.pop();
      }
      if (interrupted()) throw interruptedError();
    }
    while (!heap.empty()) w.write(heap.top().rec), heap.pop();
    w.close();
  }

  const IndelJob& job_;
  int device_;
  IrParams prm_;
  int64_t chunk_pairs_ = 1;
  BamHeader header_;
  std::vector<std::string> contigs_;
  std::vector<std::vector<KnownSite>> known_;                          // per contig, in VCF order
  std::vector<std::vector<std::pair<int64_t, size_t>>> known_by_start_;  // (event start, index), sorted
  std::vector<IrInterval> targets_;
  std::vector<Pending> queued_;
  IrBatch batch_;
  std::vector<uint32_t> best_;
  std::vector<int32_t> off_;
  std::unordered_map<int64_t, Moved> by_ordinal_;
  std::unordered_map<std::string, Moved> by_mate_;
  int64_t horizon_ = 0;
  IndelRunStats st_;
};

}  // namespace

bool gpu_indel_available() {
  const IrApi& a = ir_api();
  return a.score && last_error_entry();
}

IndelRunStats indel_run(const IndelJob& job) { return Run(job).run(); }

}  // namespace fcsg
