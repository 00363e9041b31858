#include "gpu_seed.h"

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <set>

#include "common.h"
#include "fmd_smem.h"

namespace fcsg {

namespace {

// Looked up at run time (as bgzf.cpp does for the deflate entry points): a
// libfcship without them, the tests' CPU mock for one, leaves seeding on the host.
struct SeedApi {
  decltype(&fcs_fmd_index_create) create = nullptr;
  decltype(&fcs_fmd_index_destroy) destroy = nullptr;
  decltype(&fcs_fmd_collect) collect = nullptr;
  decltype(&fcs_fmd_locate) locate = nullptr;
  decltype(&fcs_fmd_seed) seed = nullptr;  // optional: the fused mode
  const char* (*last_error)() = nullptr;
  bool ok() const { return create && destroy && collect && locate && last_error; }
};

const SeedApi& seed_api() {
  static const SeedApi A = [] {
    SeedApi a;
    a.create = reinterpret_cast<decltype(a.create)>(dlsym(RTLD_DEFAULT, "fcs_fmd_index_create"));
    a.destroy = reinterpret_cast<decltype(a.destroy)>(dlsym(RTLD_DEFAULT, "fcs_fmd_index_destroy"));
    a.collect = reinterpret_cast<decltype(a.collect)>(dlsym(RTLD_DEFAULT, "fcs_fmd_collect"));
    a.locate = reinterpret_cast<decltype(a.locate)>(dlsym(RTLD_DEFAULT, "fcs_fmd_locate"));
    a.seed = reinterpret_cast<decltype(a.seed)>(dlsym(RTLD_DEFAULT, "fcs_fmd_seed"));
    a.last_error = reinterpret_cast<decltype(a.last_error)>(dlsym(RTLD_DEFAULT, "fcs_last_error"));
    return a;
  }();
  return A;
}

std::mutex g_copies_mu;
std::set<FmdDeviceCopies*>& live_copies() {
  static auto* s = new std::set<FmdDeviceCopies*>();  // outlives static teardown
  return *s;
}

}  // namespace

bool gpu_seed_available() { return seed_api().ok(); }
bool gpu_seed_fused_available() { return seed_api().ok() && seed_api().seed; }

FmdDeviceCopies::FmdDeviceCopies(const FmdIndex& fmd) : fmd_(fmd) {
  std::lock_guard<std::mutex> g(g_copies_mu);
  live_copies().insert(this);
}

FmdDeviceCopies::~FmdDeviceCopies() {
  {
    std::lock_guard<std::mutex> g(g_copies_mu);
    live_copies().erase(this);
  }
  release();
}

fcs_fmd_index* FmdDeviceCopies::get(int device) {
  std::lock_guard<std::mutex> g(mu_);
  auto it = dev_.find(device);
  if (it != dev_.end()) return it->second;
  const SeedApi& A = seed_api();
  if (!A.ok()) throw internalError("[E::fcsg] GPU seeding without its entry points");
  const FmdView v = fmd_.view();
  std::vector<int64_t> rows((size_t)v.n_special), sas((size_t)v.n_special);
  for (int64_t i = 0; i < v.n_special; ++i) rows[i] = v.special[2 * i], sas[i] = v.special[2 * i + 1];
  fcs_fmd_index* h = nullptr;
  // the full suffix array (sa_intv 1) stays on the host: its rows are read here, not walked to
  const bool sampled = v.sa_intv > 1;
  if (A.create(device, v.occ, v.n_occ_words, v.C, v.n_rows, sampled ? v.sa : nullptr, sampled ? v.n_sa : 0, v.sa_intv,
               rows.data(), sas.data(), v.n_special, v.flen, &h) != FCS_OK)
    throw failedCommand(std::string("[E::fcs-genome align] FMD-index copy to GPU ") + std::to_string(device) + ": " +
                        A.last_error());
  dev_[device] = h;
  return h;
}

void FmdDeviceCopies::release() {
  std::lock_guard<std::mutex> g(mu_);
  for (auto& [d, h] : dev_) (void)seed_api().destroy(h);
  dev_.clear();
}

void release_fmd_device_copies() {
  std::lock_guard<std::mutex> g(g_copies_mu);
  for (FmdDeviceCopies* c : live_copies()) c->release();
}

TextMap::TextMap(const std::vector<std::vector<uint8_t>>& contigs) {
  int64_t p = 1;  // F = 5 C_1 5 C_2 ... 5 C_n 5
  for (const auto& c : contigs) {
    cstart_.push_back(p);
    p += (int64_t)c.size() + 1;
  }
  flen_ = p;
}

void TextMap::locate(int64_t p, int len, int& contig, int64_t& off, bool& rev) const {
  rev = p >= flen_;
  if (rev) p = 2 * flen_ - p - len;  // start of the reverse-strand match on F
  const auto it = std::upper_bound(cstart_.begin(), cstart_.end(), p);
  contig = (int)(it - cstart_.begin()) - 1;
  off = p - cstart_[contig];
}

namespace {

// One fcs_fmd_seed call for the chunk (a second one when the first reports
// larger totals than its capacities), then one pass over the reads for what
// the device left: rows it did not locate, reads it handed back.
void gpu_seed_fused(const FmdIndex& fmd, fcs_fmd_index* dev, const uint8_t* const* q, const int* qlen, size_t n,
                    const SeedParams& P, int threads, SeedBatch& out) {
  const SeedApi& A = seed_api();
  const uint64_t t0 = now_us();
  out.fused = true;
  out.mems.assign(n, {});
  out.pos.clear();
  out.mem_off.assign(n + 1, 0);
  out.row_off.assign(n + 1, 0);
  out.overflow.assign(n, 0);
  std::vector<int64_t> q_off(n + 1, 0);
  std::vector<int32_t> q_len(n);
  for (size_t r = 0; r < n; ++r) q_len[r] = qlen[r], q_off[r + 1] = q_off[r] + qlen[r];
  std::vector<uint8_t> codes((size_t)q_off[n]);
  parallel_for(n, threads, [&](size_t r) {
    if (qlen[r]) std::memcpy(codes.data() + q_off[r], q[r], (size_t)qlen[r]);
  });
  fcs_fmd_seed_params sp;
  sp.collect.min_len = P.min_len;
  sp.collect.split_len = P.split_len;
  sp.collect.split_width = P.split_width;
  sp.collect.max_mems = P.max_mems;
  sp.collect.max_mem_intv = P.max_mem_intv;
  sp.max_occ = P.max_occ;
  sp.max_steps = P.max_steps;
  int64_t mem_cap = P.mem_cap > 0 ? P.mem_cap : std::max<int64_t>(16 * (int64_t)n, 4096);
  int64_t row_cap = P.row_cap > 0 ? P.row_cap : std::max<int64_t>(64 * (int64_t)n, 65536);
  for (int attempt = 0;; ++attempt) {
    out.flat_mems.reset((size_t)mem_cap);
    out.flat_pos.reset((size_t)row_cap);
    const int rc = A.seed(dev, codes.data(), (int64_t)codes.size(), q_off.data(), q_len.data(), (int32_t)n, &sp,
                          reinterpret_cast<fcs_fmd_mem*>(out.flat_mems.data()), mem_cap, out.mem_off.data(),
                          out.flat_pos.data(), row_cap, out.row_off.data(), out.overflow.data());
    if (rc == FCS_OK) break;
    if (rc != FCS_FMD_SEED_MORE) throw failedCommand(std::string("[E::fcs-genome align] fcs_fmd_seed: ") + A.last_error());
    if (attempt > 0) throw internalError("[E::fcsg] fcs_fmd_seed asked for more room twice");
    mem_cap = std::max(mem_cap, out.mem_off[n]);  // the totals it reported
    row_cap = std::max(row_cap, out.row_off[n]);
    ++out.retries;
  }
  out.rows = out.row_off[n];
  const uint64_t t1 = now_us();
  out.collect_seconds = (t1 - t0) / 1e6;
  const FmdView v = fmd.view();
  fcs::FmdIx<fcs::FmdHostFetch> ix;
  ix.f.occ = v.occ;
  ix.n = v.n_rows;
  ix.C = v.C;
  std::vector<int64_t> host_rows(n, 0);
  std::atomic<int64_t> lost{-1};  // a row neither side can locate (the pass runs on threads: reported after it)
  parallel_for(n, threads, [&](size_t r) {
    if (out.overflow[r]) {  // its positions come from FmdIndex::locate in chain_read
      fmd.collect(q[r], qlen[r], P.min_len, P.split_len, P.split_width, P.max_mem_intv, out.mems[r]);
      return;
    }
    for (int64_t i = out.row_off[r]; i < out.row_off[r + 1]; ++i) {
      int64_t& p = out.flat_pos.data()[i];
      if (p >= 0) continue;
      const int64_t row = -1 - p;
      if (v.sa_intv == 1) {  // the full suffix array stayed on the host
        if (row >= v.n_sa) lost = row;
        else p = (int64_t)v.sa[row];
        continue;
      }
      int32_t steps;
      if (fcs::fmd_sa_walk(ix, v.sa, v.n_sa, v.sa_intv, v.special, v.n_special, row, INT32_MAX, p, steps) !=
          fcs::kFmdLocated)
        lost = row;
      ++host_rows[r];
    }
  });
  if (lost >= 0) throw internalError("[E::fcsg] FMD-index row " + std::to_string(lost.load()) + " cannot be located");
  for (size_t r = 0; r < n; ++r) out.host_reads += out.overflow[r] != 0, out.host_rows += host_rows[r];
  out.locate_seconds = (now_us() - t1) / 1e6;
}

}  // namespace

void gpu_seed_batch(const FmdIndex& fmd, fcs_fmd_index* dev, const uint8_t* const* q, const int* qlen, size_t n,
                    const SeedParams& P, int threads, SeedBatch& out, bool fused) {
  const SeedApi& A = seed_api();
  if (!A.ok()) throw internalError("[E::fcsg] GPU seeding without its entry points");
  if (P.max_mems < 1 || P.max_occ < 1) throw invalidParam("GPU seeding: max_mems and max_occ must be at least 1");
  if (fused) {
    if (!A.seed) throw internalError("[E::fcsg] fused GPU seeding without fcs_fmd_seed");
    return gpu_seed_fused(fmd, dev, q, qlen, n, P, threads, out);
  }
  const uint64_t t0 = now_us();
  out.mems.assign(n, {});
  out.pos.assign(n, {});
  std::vector<int64_t> q_off(n + 1, 0);
  std::vector<int32_t> q_len(n);
  for (size_t r = 0; r < n; ++r) q_len[r] = qlen[r], q_off[r + 1] = q_off[r] + qlen[r];
  std::vector<uint8_t> codes((size_t)q_off[n]);
  parallel_for(n, threads, [&](size_t r) {
    if (qlen[r]) std::memcpy(codes.data() + q_off[r], q[r], (size_t)qlen[r]);
  });
  std::vector<fcs_fmd_mem> mems(n * (size_t)P.max_mems);
  std::vector<int32_t> n_mems(n), overflow(n);
  fcs_fmd_params fp;
  fp.min_len = P.min_len;
  fp.split_len = P.split_len;
  fp.split_width = P.split_width;
  fp.max_mems = P.max_mems;
  fp.max_mem_intv = P.max_mem_intv;
  if (A.collect(dev, codes.data(), (int64_t)codes.size(), q_off.data(), q_len.data(), (int32_t)n, &fp, mems.data(),
                n_mems.data(), overflow.data()) != FCS_OK)
    throw failedCommand(std::string("[E::fcs-genome align] fcs_fmd_collect: ") + A.last_error());
  // the SMEM lists (reads the device handed back are collected here), and how many rows each read locates
  std::vector<int64_t> row0(n + 1, 0);
  parallel_for(n, threads, [&](size_t r) {
    std::vector<BiInterval>& v = out.mems[r];
    if (overflow[r]) {
      fmd.collect(q[r], qlen[r], P.min_len, P.split_len, P.split_width, P.max_mem_intv, v);
    } else {
      v.resize((size_t)n_mems[r]);
      const fcs_fmd_mem* m = mems.data() + r * (size_t)P.max_mems;
      for (int32_t i = 0; i < n_mems[r]; ++i) v[i].k = m[i].k, v[i].l = m[i].l, v[i].s = m[i].s, v[i].qb = m[i].qb, v[i].qe = m[i].qe;
    }
    int64_t rows = 0;
    for (const BiInterval& m : v) rows += std::min<int64_t>(m.s, P.max_occ);
    row0[r + 1] = rows;
  });
  for (size_t r = 0; r < n; ++r) out.host_reads += overflow[r] != 0, row0[r + 1] += row0[r];
  std::vector<fcs_fmd_mem>().swap(mems);
  const uint64_t t1 = now_us();
  out.collect_seconds = (t1 - t0) / 1e6;
  // the sampled occurrences' rows, in seed_read's order
  const int64_t total = row0[n];
  std::vector<int64_t> rows((size_t)total), pos((size_t)total);
  parallel_for(n, threads, [&](size_t r) {
    int64_t* w = rows.data() + row0[r];
    for (const BiInterval& m : out.mems[r]) {
      const int64_t step = m.s > P.max_occ ? m.s / P.max_occ : 1;
      for (int64_t j = 0, kept = 0; j < m.s && kept < P.max_occ; j += step, ++kept) *w++ = m.k + j;
    }
  });
  const FmdView v = fmd.view();
  if (v.sa_intv == 1) {  // the full suffix array: no walk, read on the host
    parallel_for((size_t)total, threads, [&](size_t i) { pos[i] = (int64_t)v.sa[rows[i]]; });
  } else if (total > 0) {
    std::vector<int32_t> status((size_t)total);
    if (A.locate(dev, rows.data(), total, 0, pos.data(), status.data()) != FCS_OK)
      throw failedCommand(std::string("[E::fcs-genome align] fcs_fmd_locate: ") + A.last_error());
    fcs::FmdIx<fcs::FmdHostFetch> ix;
    ix.f.occ = v.occ;
    ix.n = v.n_rows;
    ix.C = v.C;
    for (int64_t i = 0; i < total; ++i) {  // rows past the device's step cap: the same walk without one
      if (status[i] == FCS_FMD_LOCATED) continue;
      int32_t steps;
      if (fcs::fmd_sa_walk(ix, v.sa, v.n_sa, v.sa_intv, v.special, v.n_special, rows[i], INT32_MAX, pos[i], steps) !=
          fcs::kFmdLocated)
        throw internalError("[E::fcsg] FMD-index row " + std::to_string(rows[i]) + " cannot be located");
      ++out.host_rows;
    }
  }
  for (size_t r = 0; r < n; ++r) out.pos[r].assign(pos.begin() + row0[r], pos.begin() + row0[r + 1]);
  out.rows = total;
  out.locate_seconds = (now_us() - t1) / 1e6;
}

}  // namespace fcsg
