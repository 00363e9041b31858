// pileup.h: the walk, its two parts, the host statement of fcspu_pile and the
// runner that sends a window's per-base part to the device in chunks.
#include "pileup.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <memory>

#include "bam.h"
#include "common.h"
#include "flat_batch.h"
#include "pu_rules.h"

namespace fcsg {

RefModel::RefModel() {
  for (int q = 0; q < FCSPU_TABLE_ROWS; ++q) {
    const double e = std::min(0.75, std::pow(10.0, -q / 10.0));
    t[q][0] = std::log10(1.0 - e);
    t[q][1] = std::log10(0.5 * (1.0 - e) + 0.5 * e / 3.0);
    t[q][2] = std::log10(e / 3.0);
  }
}

const RefModel& ref_model() {
  static const RefModel m;
  return m;
}

namespace {

// One walk over the reads' CIGARs.  kBases: the per-base part over loci
// [lo, hi), with the window's letters in refw.  kOps: the per-op part over the
// whole window, with the contig in *ref.
template <bool kBases, bool kOps>
void walk(const char* refw, const std::string* ref, const Read* reads, size_t n_reads, int min_bq, int64_t lo_w, int64_t hi_w,
          Pileup& pu) {
  const int64_t n = (int64_t)pu.depth.size();
  const int64_t wb = pu.wb, we = pu.wb + n;
  auto in = [&](int64_t p) { return p >= wb && p < we; };
  const RefModel& M = ref_model();
  int* depth = pu.depth.data();
  int* events = pu.events.data();
  double* gl = pu.gl.empty() ? nullptr : pu.gl.data();
  for (size_t k = 0; k < n_reads; ++k) {
    const Read& rd = reads[k];
    int64_t rp = rd.pos;
    size_t q = 0;
    for (uint32_t c : rd.cigar) {
      const uint32_t len = cigar_len(c);
      switch (cigar_op(c)) {
        case kM: case kEq: case kX: {
          if (kBases) {
            // only the bases inside the window
            const int64_t lo = std::max<int64_t>(rp, lo_w), hi = std::min<int64_t>(rp + len, hi_w);
            for (int64_t p = lo; p < hi; ++p) {
              const size_t qi = q + (size_t)(p - rp);
              const uint8_t bq = rd.qual[qi];
              if (!fcs::pu_counted(bq, min_bq)) continue;
              ++depth[p - wb];
              const char b = rd.seq[qi], r = refw[p - wb];
              const bool nonref = fcs::pu_nonref(b, r);
              if (nonref) {
                ++events[p - wb];
                pu.snv_events.emplace_back() = snv_key(p, r, b);
              }
              if (gl) {
                const double* t = M.t[fcs::pu_row(bq)];
                double* g = gl + 3 * (p - wb);
                g[0] += t[fcs::pu_col(nonref, 0)];
                g[1] += t[fcs::pu_col(nonref, 1)];
                g[2] += t[fcs::pu_col(nonref, 2)];
              }
            }
          }
          rp += len;
          q += len;
          break;
        }
        case kI:
          if (kOps && rp > rd.pos && in(rp - 1)) {
            ++events[rp - 1 - wb];
            pu.indel_events.push_back(
                {rp - 1, std::string(1, (*ref)[rp - 1]), std::string(1, (*ref)[rp - 1]).append(rd.seq.substr(q, len))});
          }
          q += len;
          break;
        case kD:
          if (kOps && rp > rd.pos && in(rp - 1) && rp + len <= (int64_t)ref->size()) {
            ++events[rp - 1 - wb];
            pu.indel_events.push_back({rp - 1, ref->substr(rp - 1, len + 1), std::string(1, (*ref)[rp - 1])});
          }
          if (kBases)
            for (int64_t p = std::max<int64_t>(rp, lo_w), hi = std::min<int64_t>(rp + len, hi_w); p < hi; ++p) ++depth[p - wb];
          rp += len;
          break;
        case kN: rp += len; break;
        case kS: q += len; break;
        default: break;
      }
    }
  }
}

}  // namespace

void build_pileup(const std::string& ref, const Read* reads, size_t n, int min_bq, Pileup& pu) {
  walk<true, true>(ref.data() + pu.wb, &ref, reads, n, min_bq, pu.wb, pu.wb + (int64_t)pu.depth.size(), pu);
}

void pileup_bases(const char* ref_window, const Read* reads, size_t n, int min_bq, int64_t lo, int64_t hi, Pileup& pu) {
  walk<true, false>(ref_window, nullptr, reads, n, min_bq, lo, hi, pu);
}

void pileup_ops(const std::string& ref, const Read* reads, size_t n, Pileup& pu) {
  walk<false, true>(nullptr, &ref, reads, n, 0, 0, 0, pu);
}

void active_sites(const Pileup& pu, int64_t lo, int64_t hi, double frac, std::vector<int64_t>& sites) {
  for (int64_t p = lo; p < hi; ++p)
    if (fcs::pu_active(pu.events[p - pu.wb], pu.depth[p - pu.wb], frac)) sites.push_back(p);
}

// The SNV keys sort as integers (a one-base REF and ALT compare as their
// bytes), the indels as Alleles, and the two runs merge (an indel never equals
// an SNV: its REF or ALT is longer than one base).
void finish_support(Pileup& pu) {
  std::sort(pu.snv_events.begin(), pu.snv_events.end());
  std::sort(pu.indel_events.begin(), pu.indel_events.end());
  // the SNVs seen at least twice join those counted already; chunks of both kinds hold different loci
  const size_t had = pu.snv_counted.size(), ne = pu.snv_events.size();
  for (size_t i = 0; i < ne;) {
    size_t e = i + 1;
    while (e < ne && pu.snv_events[e] == pu.snv_events[i]) ++e;
    if (e - i >= (size_t)fcs::kPuMinSupport) pu.snv_counted.emplace_back(pu.snv_events[i], (int)(e - i));
    i = e;
  }
  if (had && pu.snv_counted.size() > had) std::sort(pu.snv_counted.begin(), pu.snv_counted.end());
  pu.support.clear();
  size_t i = 0, j = 0;
  const size_t ns = pu.snv_counted.size(), ni = pu.indel_events.size();
  auto next_indel = [&] {  // skip indels seen once
    while (j < ni && (j + 1 >= ni || pu.indel_events[j] < pu.indel_events[j + 1])) ++j;
  };
  next_indel();
  while (i < ns || j < ni) {
    if (i < ns) {
      const uint64_t k = pu.snv_counted[i].first;
      Allele a{(int64_t)(k >> 16), std::string(1, (char)((k >> 8) & 0xff)), std::string(1, (char)(k & 0xff))};
      if (j >= ni || a < pu.indel_events[j]) {
        pu.support.emplace_back(std::move(a), pu.snv_counted[i].second);
        ++i;
        continue;
      }
    }
    Allele& a = pu.indel_events[j];
    size_t e = j + 1;
    while (e < ni && !(a < pu.indel_events[e])) ++e;
    pu.support.emplace_back(std::move(a), (int)(e - j));
    j = e;
    next_indel();
  }
  pu.snv_events = HugeVec<uint64_t>();
  std::vector<std::pair<uint64_t, int>>().swap(pu.snv_counted);
  std::vector<Allele>().swap(pu.indel_events);
}

namespace {

// The records of the window's contig as Reads over the batch's own arrays.
std::vector<Read> reads_of(const fcspu_batch& b, int32_t ref_id) {
  std::vector<Read> out;
  for (int64_t r = 0; r < b.n; ++r) {
    if (b.ref_id[r] != ref_id) continue;
    Read x;
    x.pos = b.pos[r];
    x.cigar = {b.cigar + b.cigar_off[r], (size_t)(b.cigar_off[r + 1] - b.cigar_off[r])};
    const size_t o = (size_t)b.base_off[r], L = (size_t)(b.base_off[r + 1] - b.base_off[r]);
    x.seq = std::string_view(reinterpret_cast<const char*>(b.bases) + o, L);
    x.qual = {b.qual + o, L};
    x.mapq = b.mapq[r];
    out.push_back(x);
  }
  return out;
}

}  // namespace

void pileup_host(const fcspu_batch* batches, int n_batches, const fcspu_params& prm, const fcspu_window& w, const uint8_t* ref,
                 const int32_t* events_in, const fcspu_out& out) {
  const size_t len = (size_t)w.len;
  Pileup pu;
  pu.wb = w.start;
  pu.depth = HugeArray<int>(len), pu.events = HugeArray<int>(len);
  if (prm.want_gl) pu.gl = HugeArray<double>(3 * len);
  std::vector<int64_t> sites;
  std::vector<int> mismatches;
  for (int k = 0; k < n_batches; ++k) {
    const std::vector<Read> reads = reads_of(batches[k], w.ref_id);
    if (k > 0) {  // gl is batch 0's alone
      HugeArray<double> gl = std::move(pu.gl);
      pu.gl = HugeArray<double>();
      pileup_bases(reinterpret_cast<const char*>(ref), reads.data(), reads.size(), prm.min_bq, w.start, w.start + w.len, pu);
      pu.gl = std::move(gl);
      continue;
    }
    pileup_bases(reinterpret_cast<const char*>(ref), reads.data(), reads.size(), prm.min_bq, w.start, w.start + w.len, pu);
    // the predicate sees batch 0's mismatch events plus events_in
    mismatches.assign(pu.events.data(), pu.events.data() + len);
    if (events_in)
      for (size_t i = 0; i < len; ++i) pu.events[i] += events_in[i];
    active_sites(pu, w.start, w.start + w.len, prm.frac, sites);
    std::copy(mismatches.begin(), mismatches.end(), pu.events.data());
  }
  finish_support(pu);  // no indel events here: the support is the SNVs in (offset, alt) order
  if ((int64_t)sites.size() > out.max_sites || (int64_t)pu.support.size() > out.max_snvs)
    throw failedCommand("[E::pileup] the window has " + std::to_string(sites.size()) + " sites and " +
                        std::to_string(pu.support.size()) + " SNVs, max_sites is " + std::to_string(out.max_sites) +
                        " and max_snvs " + std::to_string(out.max_snvs));
  for (size_t i = 0; i < len; ++i) out.depth[i] = pu.depth[i], out.events[i] = pu.events[i];
  if (prm.want_gl) std::memcpy(out.gl, pu.gl.data(), 24 * len);
  for (size_t i = 0; i < sites.size(); ++i) out.sites[i] = (int32_t)(sites[i] - w.start);
  for (size_t i = 0; i < pu.support.size(); ++i) {
    fcspu_snv v{};
    v.offset = (int32_t)(pu.support[i].first.pos - w.start), v.alt = (uint8_t)pu.support[i].first.alt[0], v.count = pu.support[i].second;
    out.snvs[i] = v;
  }
  *out.n_sites = (int64_t)sites.size(), *out.n_snvs = (int64_t)pu.support.size();
}

void pileup_ops_host(const fcspu_batch& batch, const fcspu_window& w, const std::string& contig, int32_t* events) {
  Pileup pu;
  pu.wb = w.start;
  pu.depth = HugeArray<int>((size_t)w.len), pu.events = HugeArray<int>((size_t)w.len);
  const std::vector<Read> reads = reads_of(batch, w.ref_id);
  pileup_ops(contig, reads.data(), reads.size(), pu);
  for (int64_t i = 0; i < w.len; ++i) events[i] += pu.events[(size_t)i];
}

// ------------------------------------------------------------------ the device path
namespace {

struct PuApi {
  decltype(&fcspu_pile) pile = FCSG_DEVICE_ENTRY(fcspu_pile);
};
const PuApi& pu_api() {
  static const PuApi A;
  return A;
}

// A window's reads as a flat batch, the running maximum of their ends, and how
// many of the records before each one the device cannot take.
struct FlatReads {
  FlatRecords f;
  std::vector<int64_t> max_end;
  std::vector<int32_t> refused;  // [n + 1] prefix counts
};

void flatten_reads(const HugeVec<Read>& reads, int32_t ref_id, int64_t contig_len, FlatReads& out) {
  static const auto letter_ok = [] {
    std::array<uint8_t, 256> t{};
    for (const char c : {'A', 'C', 'G', 'T', 'N'}) t[(uint8_t)c] = 1;
    return t;
  }();
  const size_t n = reads.size();
  FlatRecords& f = out.f;
  f.flag.assign(n, 0), f.ref_id.assign(n, ref_id), f.pos.resize(n), f.mapq.resize(n), f.absent.assign(n, 0);
  f.cigar_off.assign(n + 1, 0), f.base_off.assign(n + 1, 0);
  out.max_end.resize(n), out.refused.assign(n + 1, 0);
  int64_t me = INT64_MIN;
  for (size_t k = 0; k < n; ++k) {
    const Read& r = reads[k];
    f.pos[k] = r.pos, f.mapq[k] = (uint8_t)r.mapq;
    f.cigar_off[k + 1] = f.cigar_off[k] + (int64_t)r.cigar.size();
    f.base_off[k + 1] = f.base_off[k] + (int64_t)r.seq.size();
    out.max_end[k] = me = std::max(me, r.end);
  }
  f.cigar.resize((size_t)f.cigar_off[n]), f.qual.resize((size_t)f.base_off[n]), f.bases.resize((size_t)f.base_off[n]);
  for (size_t k = 0; k < n; ++k) {
    const Read& r = reads[k];
    if (!r.cigar.empty()) std::memcpy(f.cigar.data() + f.cigar_off[k], r.cigar.p, 4 * r.cigar.size());
    const size_t L = r.seq.size();
    uint8_t* b = f.bases.data() + f.base_off[k];
    if (L) std::memcpy(b, r.seq.data(), L), std::memcpy(f.qual.data() + f.base_off[k], r.qual.p, L);
    uint8_t ok = 1;
    for (size_t i = 0; i < L; ++i) ok &= letter_ok[b[i]];
    out.refused[k + 1] = out.refused[k] + (!ok || r.pos < 0 || r.end > contig_len || r.qual.size() != L);
  }
}

}  // namespace

bool gpu_pileup_available() { return pu_api().pile && last_error_entry(); }

void pileup_window_device(int device, int64_t chunk_bp, const std::string& ref, int32_t ref_id, const HugeVec<Read>* reads,
                          int n_sets, int min_bq, double frac, Pileup& pu, std::vector<int64_t>& sites, PileupRunStats& st,
                          const char* command) {
  const int64_t wb = pu.wb, we = wb + (int64_t)pu.depth.size();
  chunk_bp = std::clamp<int64_t>(chunk_bp, 1, FCSPU_WINDOW_MAX);
  // batch 0's per-op part first: its events at the anchors are what the predicate adds
  pileup_ops(ref, reads[0].data(), reads[0].size(), pu);
  const uint64_t tf = now_us();
  FlatReads flat[FCSPU_BATCHES_MAX];
  for (int s = 0; s < n_sets; ++s) flatten_reads(reads[s], ref_id, (int64_t)ref.size(), flat[s]);
  st.flatten_seconds += (now_us() - tf) / 1e6;
  const size_t room = (size_t)std::min<int64_t>(chunk_bp, we - wb);
  // not zeroed: only what a call reports is read
  std::unique_ptr<int32_t[]> ev(new int32_t[room]), site_off(new int32_t[room]);
  std::unique_ptr<fcspu_snv[]> snvs(new fcspu_snv[4 * room]);
  fcspu_params prm{};
  prm.min_bq = min_bq, prm.want_gl = pu.gl.empty() ? 0 : 1, prm.frac = frac;
  for (int64_t cb = wb; cb < we; cb += chunk_bp) {
    const int64_t ce = std::min(we, cb + chunk_bp), len = ce - cb;
    // the records that reach the chunk: from the first whose running-maximum end lies beyond cb to the last that starts before ce
    size_t lo[FCSPU_BATCHES_MAX] = {0, 0}, hi[FCSPU_BATCHES_MAX] = {0, 0};
    bool host = false;
    for (int s = 0; s < n_sets; ++s) {
      const FlatReads& F = flat[s];
      lo[s] = (size_t)(std::upper_bound(F.max_end.begin(), F.max_end.end(), cb) - F.max_end.begin());
      hi[s] = (size_t)(std::lower_bound(F.f.pos.begin(), F.f.pos.end(), ce, [](int32_t p, int64_t x) { return p < x; }) - F.f.pos.begin());
      hi[s] = std::max(hi[s], lo[s]);
      host |= F.refused[hi[s]] != F.refused[lo[s]];
    }
    if (host) {
      pileup_bases(ref.data() + wb, reads[0].data() + lo[0], hi[0] - lo[0], min_bq, cb, ce, pu);
      active_sites(pu, cb, ce, frac, sites);
      if (n_sets > 1) pileup_bases(ref.data() + wb, reads[1].data() + lo[1], hi[1] - lo[1], min_bq, cb, ce, pu);
      ++st.host_chunks;
      continue;
    }
    fcspu_batch b[FCSPU_BATCHES_MAX];
    for (int s = 0; s < n_sets; ++s) b[s] = flat[s].f.view<fcspu_batch>(lo[s], hi[s]);
    const fcspu_window w{ref_id, 0, cb, len, (int64_t)ref.size()};
    int64_t n_sites = 0, n_snvs = 0;
    fcspu_out out{};
    out.depth = pu.depth.data() + (cb - wb), out.events = ev.get();
    out.gl = prm.want_gl ? pu.gl.data() + 3 * (cb - wb) : nullptr;
    out.sites = site_off.get(), out.max_sites = len, out.n_sites = &n_sites;
    out.snvs = snvs.get(), out.max_snvs = 4 * len, out.n_snvs = &n_snvs;
    const uint64_t td = now_us();
    device_check(pu_api().pile(device, b, n_sets, &prm, &w, reinterpret_cast<const uint8_t*>(ref.data()) + cb, &ref_model().t[0][0],
                               pu.events.data() + (cb - wb), &out),
                 command, "fcspu_pile");
    st.device_seconds += (now_us() - td) / 1e6;
    int* events = pu.events.data() + (cb - wb);
    for (int64_t i = 0; i < len; ++i) events[i] += ev[(size_t)i];
    for (int64_t i = 0; i < n_sites; ++i) sites.push_back(cb + site_off[(size_t)i]);
    for (int64_t i = 0; i < n_snvs; ++i) {
      const fcspu_snv& v = snvs[(size_t)i];
      const int64_t p = cb + v.offset;
      pu.snv_counted.emplace_back(snv_key(p, ref[(size_t)p], (char)v.alt), v.count);
    }
    ++st.gpu_chunks;
  }
  if (n_sets > 1) pileup_ops(ref, reads[1].data(), reads[1].size(), pu);
}

}  // namespace fcsg
