// The baserecal / printreads / bqsr commands (bqsr_run.h): the reference and
// its known-sites bitmap, the streaming passes over the BAM in chunks of
// bqsr.chunk_records, the flattening, and the device calls or the host rules.
#include "bqsr_run.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <unordered_map>

#include "bam_stream.h"
#include "bgzf.h"
#include "bqsr.h"
#include "common.h"
#include "config.h"
#include "fcship.h"
#include "flat_batch.h"
#include "intervals.h"

namespace fcsg {

namespace {

struct BqApi {
  decltype(&fcsbq_ref_create) ref_create = FCSG_DEVICE_ENTRY(fcsbq_ref_create);
  decltype(&fcsbq_ref_destroy) ref_destroy = FCSG_DEVICE_ENTRY(fcsbq_ref_destroy);
  decltype(&fcsbq_count) count = FCSG_DEVICE_ENTRY(fcsbq_count);
  decltype(&fcsbq_apply) apply = FCSG_DEVICE_ENTRY(fcsbq_apply);
};

const BqApi& bq_api() {
  static const BqApi A;
  return A;
}

// The device the job runs on, or -1 (with one log line when the library lacks the entry points).
int device_of(const BqsrJob& job) {
  return device_or_host(job.device, gpu_bqsr_available(),
                        "[fcs-genome bqsr] bqsr.gpu: the loaded libfcship has no fcsbq_count entry point; "
                        "qualities are recalibrated on the host\n");
}

// The header's read groups: ids[k] the @RG ID, names[k] its PU when present, else the ID.
void read_groups(const BamHeader& h, std::vector<std::string>& ids, std::vector<std::string>& names) {
  for (const RgLine& rg : rg_lines(h)) {
    const std::string id = rg.get("ID"), pu = rg.get("PU");
    if (id.empty()) continue;
    ids.push_back(id);
    names.push_back(pu.empty() ? id : pu);
  }
}

// The reference in the BAM header's contig order, with the known-sites bitmap.
struct BqGenome {
  std::vector<uint8_t> bases;
  std::vector<int64_t> ref_off;
  std::vector<uint64_t> known;
  BqRefView view() const {
    BqRefView v;
    v.bases = bases.data(), v.ref_off = ref_off.data(), v.n_ref = (int32_t)ref_off.size() - 1, v.known = known.data();
    return v;
  }
};

BqGenome load_genome(const std::string& fasta, const BamHeader& h) {
  BqGenome g;
  g.ref_off.assign(1, 0);
  for (const std::string& s : header_contigs(fasta, h, false)) {  // a length that differs from the header's is taken as it is
    g.bases.insert(g.bases.end(), s.begin(), s.end());
    g.ref_off.push_back((int64_t)g.bases.size());
  }
  g.known.assign((g.bases.size() + 63) / 64 + 1, 0);
  return g;
}

// CHROM, POS and REF of every record of a plain or bgzipped VCF: the bits POS-1 .. POS-1+len(REF)-1.
void load_known_sites(const std::string& path, const BamHeader& h, BqGenome& g, BqsrStats& st) {
  std::unordered_map<std::string, int> index;
  for (size_t k = 0; k < h.names.size(); ++k) index[h.names[k]] = (int)k;
  known_sites_lines(path, [&](const std::string& line) {
    const size_t t1 = line.find('\t');
    const size_t t2 = t1 == std::string::npos ? t1 : line.find('\t', t1 + 1);
    const size_t t3 = t2 == std::string::npos ? t2 : line.find('\t', t2 + 1);
    const size_t t4 = t3 == std::string::npos ? t3 : line.find('\t', t3 + 1);
    if (t3 == std::string::npos) throw formatError("known sites " + path + ": a record of fewer than 4 fields");
    const auto it = index.find(line.substr(0, t1));
    if (it == index.end()) {
      ++st.known_skipped;
      return;
    }
    int64_t pos;
    try {
      pos = std::stoll(line.substr(t1 + 1, t2 - t1 - 1));
    } catch (const std::logic_error&) {
      throw formatError("known sites " + path + ": POS of \"" + line.substr(0, std::min<size_t>(line.size(), 60)) + "\"");
    }
    const int64_t len = (int64_t)((t4 == std::string::npos ? line.size() : t4) - t3 - 1);
    const int64_t g0 = g.ref_off[(size_t)it->second], clen = g.ref_off[(size_t)it->second + 1] - g0;
    for (int64_t p = std::max<int64_t>(pos - 1, 0); p < pos - 1 + len && p < clen; ++p)
      g.known[(size_t)((g0 + p) >> 6)] |= (uint64_t)1 << ((g0 + p) & 63);
    ++st.known_sites;
  });
}

// -L: the intervals by contig index, sorted; a record is kept when it overlaps one.
struct Regions {
  bool all = true;
  std::vector<std::vector<std::pair<int64_t, int64_t>>> by_ref;  // 0-based half-open
  bool keep(const BamRecord& r) const {
    if (all) return true;
    if (r.ref_id < 0 || (size_t)r.ref_id >= by_ref.size() || r.pos < 0) return false;
    const int64_t beg = r.pos, end = std::max<int64_t>(r.end(), (int64_t)r.pos + 1);
    for (const auto& iv : by_ref[(size_t)r.ref_id]) {
      if (iv.first >= end) break;
      if (iv.second > beg) return true;
    }
    return false;
  }
};

Regions load_regions(const std::string& path, const BamHeader& h) {
  Regions rg;
  if (path.empty()) return rg;
  if (!is_regular_file(path)) throw fileNotFound(path);
  rg.all = false;
  rg.by_ref.resize(h.names.size());
  for (const Interval& iv : read_regions(path)) {
    const int c = h.ref_index(iv.chrom);
    if (c >= 0) rg.by_ref[(size_t)c].emplace_back(iv.lb - 1, iv.ub);
  }
  for (auto& v : rg.by_ref) std::sort(v.begin(), v.end());
  return rg;
}

// One chunk of records in the order `order` as an fcsbq_batch over f and its own read groups.
fcsbq_batch flat_view(const std::vector<BamRecord>& recs, const std::vector<int32_t>& rg, const std::vector<uint32_t>& order,
                      FlatRecords& f, std::vector<int32_t>& flat_rg) {
  flatten(recs, order.size(), true, f, order.data());
  flat_rg.resize(order.size());
  for (size_t k = 0; k < order.size(); ++k) flat_rg[k] = rg[order[k]];
  fcsbq_batch b = f.view<fcsbq_batch>(0, order.size());
  b.rg = flat_rg.data();
  return b;
}

// The job's input, read chunk by chunk: the records -L keeps, with their read group indices.
class ChunkReader {
 public:
  ChunkReader(const BqsrJob& job) : in_(job.input, false) {
    std::vector<std::string> ids;
    read_groups(header(), ids, names_);
    for (size_t k = 0; k < ids.size(); ++k) rg_index_.emplace(ids[k], (int32_t)k);
    regions_ = load_regions(job.intervals, header());
    chunk_ = (size_t)std::max(conf().get_int("bqsr.chunk_records"), 1);
  }
  const BamHeader& header() const { return in_.header(); }
  const std::vector<std::string>& rg_names() const { return names_; }
  bool next(std::vector<BamRecord>& recs, std::vector<int32_t>& rg) {
    recs.clear();
    in_.read(recs, chunk_, [&](const BamRecord& r) { return regions_.keep(r); });
    rg.assign(recs.size(), -1);
    std::string id;
    for (size_t k = 0; k < recs.size(); ++k)
      if (recs[k].get_aux_string("RG", id)) {
        const auto it = rg_index_.find(id);
        if (it != rg_index_.end()) rg[k] = it->second;
      }
    return !recs.empty();
  }

 private:
  BamStream in_;
  size_t chunk_ = 1;
  std::vector<std::string> names_;
  std::unordered_map<std::string, int32_t> rg_index_;
  Regions regions_;
};

// A device copy of the genome for the job's lifetime.
struct DeviceRef {
  fcsbq_ref* h = nullptr;
  DeviceRef(int device, const BqGenome& g) {
    if (device < 0) return;
    device_check(bq_api().ref_create(device, g.bases.data(), g.ref_off.data(), (int32_t)g.ref_off.size() - 1, g.known.data(), &h),
                 "bqsr", "fcsbq_ref_create");
  }
  ~DeviceRef() {
    if (h) bq_api().ref_destroy(h);
  }
  DeviceRef(const DeviceRef&) = delete;
  DeviceRef& operator=(const DeviceRef&) = delete;
};

struct CountTables {
  int32_t n_rg = 0;
  std::vector<int64_t> ctx, cyc;
  explicit CountTables(int32_t n) : n_rg(n), ctx(2 * kBqCtxCells * (size_t)n, 0), cyc(2 * kBqCycCells * (size_t)n, 0) {}
};

void sum_tables(const CountTables& t, BqsrStats& st) {
  for (size_t i = 0; i < t.cyc.size(); i += 2) st.observations += t.cyc[i], st.errors += t.cyc[i + 1];
}

// Pass 1: every chunk grouped by read group (stable) and counted into t.
void count_pass(const BqsrJob& job, int device, CountTables& t, std::vector<std::string>& rg_names, BqsrStats& st) {
  ChunkReader in(job);
  rg_names = in.rg_names();
  t = CountTables((int32_t)rg_names.size());
  BqGenome g = load_genome(job.ref, in.header());
  for (const std::string& k : job.known) load_known_sites(k, in.header(), g, st);
  DeviceRef dref(device, g);
  std::vector<BamRecord> recs;
  std::vector<int32_t> rg;
  std::vector<uint32_t> order;
  FlatRecords f;
  std::vector<int32_t> flat_rg;
  while (in.next(recs, rg)) {
    order.resize(recs.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return rg[a] < rg[b]; });
    const fcsbq_batch b = flat_view(recs, rg, order, f, flat_rg);
    for (int64_t r = 0; r < b.n; ++r)
      st.counted += b.rg[r] >= 0 && !b.qual_absent[r] && !(b.flag[r] & 0x704) && b.mapq[r] != 0 && b.mapq[r] != 255;
    st.records += b.n;
    if (device >= 0) device_check(bq_api().count(dref.h, &b, t.n_rg, t.ctx.data(), t.cyc.data()), "bqsr", "fcsbq_count");
    else bqsr_count_host(g.view(), b, t.n_rg, t.ctx.data(), t.cyc.data(), host_threads());
  }
  sum_tables(t, st);
}

// Pass 2: every chunk's qualities rewritten from the tables, the records written in input order.
void apply_pass(const BqsrJob& job, int device, const BqTables& tables, BqsrStats& st) {
  ChunkReader in(job);
  BamWriter w(job.output, in.header());
  if (in.header().text.find("SO:coordinate") != std::string::npos) w.index_on_close();
  std::vector<BamRecord> recs;
  std::vector<int32_t> rg;
  std::vector<uint32_t> order;
  std::vector<uint8_t> out;
  std::vector<const BamRecord*> ptrs;
  FlatRecords f;
  std::vector<int32_t> flat_rg;
  st.records = 0;
  while (in.next(recs, rg)) {
    order.resize(recs.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (uint32_t)i;
    const fcsbq_batch b = flat_view(recs, rg, order, f, flat_rg);
    out.assign((size_t)b.n_bases + 1, 0);
    if (device >= 0) {
      device_check(bq_api().apply(device, &b, tables.n_rg, tables.base.data(), tables.dctx.data(), tables.dcyc.data(), out.data()),
                   "bqsr", "fcsbq_apply");
    } else {
      bqsr_apply_host(b, tables, out.data(), host_threads());
    }
    parallel_for(recs.size(), host_threads(), [&](size_t k) {
      if (b.rg[k] >= 0 && !b.qual_absent[k]) std::memcpy(recs[k].qual.data(), out.data() + b.base_off[k], recs[k].qual.size());
    });
    for (int64_t r = 0; r < b.n; ++r) st.recalibrated += b.rg[r] >= 0 && !b.qual_absent[r];
    st.records += b.n;
    ptrs.resize(recs.size());
    for (size_t i = 0; i < recs.size(); ++i) ptrs[i] = &recs[i];
    w.write_all(ptrs);
  }
  w.close();
}

std::vector<std::string> header_rg_names(const BqsrJob& job) {
  BamReader in(bam_inputs(job.input)[0]);
  std::vector<std::string> ids, names;
  read_groups(in.header(), ids, names);
  return names;
}

}  // namespace

void known_sites_lines(const std::string& path, const std::function<void(const std::string&)>& take) {
  if (!is_regular_file(path)) throw fileNotFound(path);
  auto data = [&](const std::string& line) {
    if (!line.empty() && line[0] != '#') take(line);
  };
  std::string line;
  if (is_bgzf_file(path)) {
    BgzfReader in(path);
    while (in.getline(line)) data(line);
  } else {
    std::ifstream in(path);
    while (std::getline(in, line)) {
      if (!line.empty() && line.back() == '\r') line.pop_back();
      data(line);
    }
  }
}

bool gpu_bqsr_available() {
  const BqApi& a = bq_api();
  return a.ref_create && a.ref_destroy && a.count && a.apply && last_error_entry();
}

BqsrStats baserecal_run(const BqsrJob& job) {
  const uint64_t t0 = now_us();
  BqsrStats st;
  const int device = device_of(job);
  CountTables t(0);
  std::vector<std::string> names;
  count_pass(job, device, t, names, st);
  write_file(job.report, bqsr_report_text(t.n_rg, t.ctx.data(), t.cyc.data(), names));
  st.on_device = device >= 0;
  st.seconds = (now_us() - t0) / 1e6;
  return st;
}

BqsrStats printreads_run(const BqsrJob& job) {
  const uint64_t t0 = now_us();
  BqsrStats st;
  const int device = device_of(job);
  const std::vector<std::string> names = header_rg_names(job);
  std::vector<int64_t> ctx, cyc;
  bqsr_report_parse(read_file(job.report), names, ctx, cyc);
  const BqTables tables = bqsr_finalize((int32_t)names.size(), ctx.data(), cyc.data());
  apply_pass(job, device, tables, st);
  st.on_device = device >= 0;
  st.seconds = (now_us() - t0) / 1e6;
  return st;
}

BqsrStats bqsr_run(const BqsrJob& job) {
  const uint64_t t0 = now_us();
  BqsrStats st;
  const int device = device_of(job);
  CountTables t(0);
  std::vector<std::string> names;
  count_pass(job, device, t, names, st);
  if (!job.report.empty()) write_file(job.report, bqsr_report_text(t.n_rg, t.ctx.data(), t.cyc.data(), names));
  const BqTables tables = bqsr_finalize(t.n_rg, t.ctx.data(), t.cyc.data());
  apply_pass(job, device, tables, st);
  st.on_device = device >= 0;
  st.seconds = (now_us() - t0) / 1e6;
  return st;
}

}  // namespace fcsg
