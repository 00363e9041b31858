// FMD-index seeding calls of the C-ABI (include/fcship.h): the device copy of
// an index, SMEM collection, suffix-array lookup and the fused seeding call.
#include <cstring>
#include <map>
#include <memory>

#include "session.h"
// after the HIP runtime, which session.h brings: the two headers are the kernels' own
#include "fmd_expand.h"
#include "fmd_smem.h"

// A device copy of an FMD-index.  Live handles are registered, so a call can
// tell a handle that was never made, destroyed, or lost its device memory to
// fcs_device_release from a good one before it touches the device.
struct fcs_fmd_index {
  int device = 0;
  bool released = false;  // fcs_device_release reset the device: the pointers are gone
  fcs::FmdDevIndex dx{};
  void* mem[4] = {nullptr, nullptr, nullptr, nullptr};  // occ, C, sa, special
};

namespace fcs {
namespace {

std::mutex g_fmd_mu;
auto* g_fmd_live = new std::map<const fcs_fmd_index*, fcs_fmd_index*>();  // outlives static teardown

// The registered handle behind `h`, or null (with the error set).
const fcs_fmd_index* fmd_handle(const fcs_fmd_index* h, const char* who) {
  if (h) {
    std::lock_guard<std::mutex> lk(g_fmd_mu);
    auto it = g_fmd_live->find(h);
    if (it != g_fmd_live->end() && !it->second->released) return it->second;
  }
  fail_invalid(who, h ? "the index handle is not a live one" : "null index handle");
  return nullptr;
}

int fmd_params_check(const fcs_fmd_params* p, const char* who, int32_t& max_mems) {
  if (!p) return fail_invalid(who, "null params");
  if (p->max_mems < 1) return fail_invalid(who, "max_mems " + std::to_string(p->max_mems) + " < 1");
  if (p->min_len < 0 || p->max_mem_intv < 0) return fail_invalid(who, "negative min_len or max_mem_intv");
  max_mems = p->max_mems;
  return FCS_OK;
}

FmdCollectParams fmd_params(const fcs_fmd_params* p) {
  return FmdCollectParams{p->min_len, p->split_len, p->split_width, p->max_mem_intv};
}

static_assert(sizeof(fcs_fmd_mem) == sizeof(FmdIv) && sizeof(FmdIv) == 32, "fcs_fmd_mem is the kernels' interval");

// The step cap of an LF walk when the caller leaves it at 0.
int32_t fmd_default_steps(const fcs_fmd_index* h, int32_t max_steps) {
  return max_steps ? max_steps : (int32_t)std::min<int64_t>(32 * (int64_t)h->dx.sa_intv, INT32_MAX);
}

// The reads of a host call (fcs_fmd_collect, fcs_fmd_seed): checked against
// the code bytes, then planned first in the call's arena and staged as its one
// H2D copy: codes, offsets, lengths and the launch order.
struct FmdReads {
  const uint8_t* codes;
  int64_t n_code_bytes;
  const int64_t* q_off;
  const int32_t* q_len;
  int32_t n;
  int32_t max_len = 0;
  size_t o_codes = 0, o_off = 0, o_len = 0, o_ord = 0;

  int check(const char* who) {
    for (int32_t r = 0; r < n; ++r) {
      if (q_len[r] < 0)
        return fail_invalid(who, "read " + std::to_string(r) + " has negative length " + std::to_string(q_len[r]));
      if (q_off[r] < 0 || q_off[r] > n_code_bytes - q_len[r])
        return fail_invalid(who, "read " + std::to_string(r) + " at offset " + std::to_string(q_off[r]) + " leaves the " +
                                     std::to_string(n_code_bytes) + " code bytes");
      max_len = std::max(max_len, q_len[r]);
    }
    return FCS_OK;
  }
  void plan(Arena& a) {
    const size_t N = (size_t)n;
    o_codes = a.add((size_t)n_code_bytes), o_off = a.add(8 * N), o_len = a.add(4 * N), o_ord = a.add(4 * N);
  }
  void fill(char* host) const {
    const size_t N = (size_t)n;
    if (n_code_bytes) std::memcpy(host + o_codes, codes, (size_t)n_code_bytes);
    std::memcpy(host + o_off, q_off, 8 * N);
    std::memcpy(host + o_len, q_len, 4 * N);
    // longest first (counting sort by length): the grid's last quads do not end on the long reads
    std::vector<int32_t> start((size_t)max_len + 2, 0);
    for (size_t r = 0; r < N; ++r) ++start[(size_t)(max_len - q_len[r]) + 1];
    for (size_t k = 1; k < start.size(); ++k) start[k] += start[k - 1];
    int32_t* ord = reinterpret_cast<int32_t*>(host + o_ord);
    for (size_t r = 0; r < N; ++r) ord[start[(size_t)(max_len - q_len[r])]++] = (int32_t)r;
  }
};

int fmd_locate_check(const fcs_fmd_index* index, const void* rows, int64_t n, int32_t& max_steps, const void* pos,
                     const void* status, const char* who, const fcs_fmd_index*& h) {
  if (n < 0 || max_steps < 0 || (n > 0 && (!rows || !pos || !status))) return fail_invalid(who, "bad arguments");
  if (!(h = fmd_handle(index, who))) return FCS_ERR_INVALID;
  if (!h->dx.sa) return fail_invalid(who, "the index was made without its suffix array (sa_intv 1)");
  max_steps = fmd_default_steps(h, max_steps);
  return FCS_OK;
}

// The device scratch of a fused seeding call, as fcship.h lists its parts.
struct FmdSeedWs {
  size_t arena, slots, place, n_mems, n_eff, n_rows, rows;
};
FmdSeedWs fmd_seed_ws(Arena& L, int32_t n_reads, int32_t max_q_len, int32_t max_mems, int64_t row_cap) {
  const size_t n = (size_t)n_reads;
  FmdSeedWs w;
  w.arena = L.add((size_t)fcs_fmd_collect_arena_bytes(n_reads, max_q_len));
  w.slots = L.add(n * (size_t)max_mems * sizeof(FmdIv));
  w.place = L.add(n * (size_t)max_mems * sizeof(FmdSeedPlace));
  w.n_mems = L.add(4 * n);
  w.n_eff = L.add(4 * n);
  w.n_rows = L.add(8 * n);
  w.rows = L.add(8 * (size_t)row_cap);
  return w;
}

// What fcs_fmd_seed and fcs_fmd_seed_dev check alike, before any device work.
int fmd_seed_check(const fcs_fmd_seed_params* p, int64_t mem_cap, int64_t row_cap, const void* mems, const void* mem_off,
                   const void* pos, const void* row_off, const void* overflow, int32_t n_reads, const char* who,
                   int32_t& max_mems) {
  if (!p) return fail_invalid(who, "null params");
  int rc = fmd_params_check(&p->collect, who, max_mems);
  if (rc) return rc;
  if (p->max_occ < 1) return fail_invalid(who, "max_occ " + std::to_string(p->max_occ) + " < 1");
  if (p->max_steps < 0) return fail_invalid(who, "negative max_steps");
  if (mem_cap < 0 || row_cap < 0)
    return fail_invalid(who, "negative capacity (mem_cap " + std::to_string(mem_cap) + ", row_cap " +
                                 std::to_string(row_cap) + ")");
  if (!mem_off || !row_off || (n_reads > 0 && !overflow) || (mem_cap > 0 && !mems) || (row_cap > 0 && !pos))
    return fail_invalid(who, "null output");
  return FCS_OK;
}

}  // namespace

void fmd_drop_device(int device) {
  std::lock_guard<std::mutex> lk(g_fmd_mu);
  for (auto& [k, h] : *g_fmd_live)
    if (h->device == device) h->released = true;
}

}  // namespace fcs

using namespace fcs;

extern "C" {

int fcs_fmd_index_create(int32_t device, const uint64_t* occ, int64_t n_occ_words, const int64_t* C, int64_t n_rows,
                         const uint64_t* sa, int64_t n_sa, int32_t sa_intv, const int64_t* special_rows,
                         const int64_t* special_sa, int64_t n_special, int64_t flen, fcs_fmd_index** handle) {
  if (!handle) return fail(FCS_ERR_INVALID, "[E::fcs_fmd_index_create] null handle pointer");
  *handle = nullptr;
  if (!occ || !C || n_rows < 1 || flen < 0 || sa_intv < 1 || n_sa < 0 || n_special < 0 ||
      (n_special > 0 && (!special_rows || !special_sa)))
    return fail(FCS_ERR_INVALID, "[E::fcs_fmd_index_create] bad arguments");
  // the layout FmdIndex builds: a line per 64 rows and one of totals; a sample per sa_intv rows
  if (n_occ_words != 8 * ((n_rows + 63) / 64 + 1))
    return fail(FCS_ERR_INVALID, "[E::fcs_fmd_index_create] n_occ_words " + std::to_string(n_occ_words) +
                                     " is not 8 * ((n_rows + 63) / 64 + 1)");
  if (sa ? n_sa != (n_rows + sa_intv - 1) / sa_intv : (sa_intv != 1 || n_sa != 0))
    return fail(FCS_ERR_INVALID, "[E::fcs_fmd_index_create] n_sa " + std::to_string(n_sa) + " does not fit n_rows and sa_intv" +
                                     (sa ? "" : " (the suffix array may be left out with sa_intv 1 only)"));
  for (int c = 0; c < 5; ++c)
    if (C[c] < 0 || C[c + 1] < C[c] || C[c + 1] > n_rows)
      return fail(FCS_ERR_INVALID, "[E::fcs_fmd_index_create] C is not a non-decreasing sequence within [0, n_rows]");
  for (int64_t i = 0; i < n_special; ++i)
    if (special_rows[i] < 0 || special_rows[i] >= n_rows || (i > 0 && special_rows[i] <= special_rows[i - 1]))
      return fail(FCS_ERR_INVALID, "[E::fcs_fmd_index_create] special_rows is not sorted within [0, n_rows)");
  int rc = check_device(device);
  if (rc) return rc;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(FCS_ERR_DEVICE, "[E::fcs_fmd_index_create] device " + std::to_string(device) + " is not a gfx950");
  FCS_SET_DEVICE((device));
  auto h = std::make_unique<fcs_fmd_index>();
  h->device = device;
  std::vector<int64_t> pairs(2 * (size_t)n_special);
  for (int64_t i = 0; i < n_special; ++i) pairs[2 * i] = special_rows[i], pairs[2 * i + 1] = special_sa[i];
  const void* src[4] = {occ, C, sa, pairs.data()};
  const size_t bytes[4] = {8 * (size_t)n_occ_words, 8 * 6, sa ? 8 * (size_t)n_sa : 0, 16 * (size_t)n_special};
  for (int k = 0; k < 4 && !rc; ++k) {
    if (!bytes[k]) continue;
    // plain hipMalloc: the stream-ordered pool is not used in this library
    if (hipMalloc(&h->mem[k], bytes[k]) != hipSuccess) {
      h->mem[k] = nullptr;
      rc = fail(FCS_ERR_NOMEM, "[E::fcs_fmd_index_create] hipMalloc of " + std::to_string(bytes[k]) + " bytes failed");
    } else if (hipMemcpy(h->mem[k], src[k], bytes[k], hipMemcpyHostToDevice) != hipSuccess) {
      rc = fail(FCS_ERR_DEVICE, "[E::fcs_fmd_index_create] the copy to the device failed");
    }
  }
  if (rc) {
    for (void* m : h->mem)
      if (m) (void)hipFree(m);
    return rc;
  }
  h->dx = FmdDevIndex{static_cast<const uint64_t*>(h->mem[0]), n_occ_words, static_cast<const int64_t*>(h->mem[1]), n_rows,
                      static_cast<const uint64_t*>(h->mem[2]), n_sa, sa_intv, static_cast<const int64_t*>(h->mem[3]),
                      n_special, flen};
  fcs_fmd_index* raw = h.release();
  {
    std::lock_guard<std::mutex> lk(g_fmd_mu);
    (*g_fmd_live)[raw] = raw;
  }
  *handle = raw;
  return FCS_OK;
}

int fcs_fmd_index_destroy(fcs_fmd_index* handle) {
  if (!handle) return FCS_OK;
  {
    std::lock_guard<std::mutex> lk(g_fmd_mu);
    auto it = g_fmd_live->find(handle);
    if (it == g_fmd_live->end())
      return fail(FCS_ERR_INVALID, "[E::fcs_fmd_index_destroy] the index handle is not a live one");
    g_fmd_live->erase(it);
  }
  std::unique_ptr<fcs_fmd_index> h(handle);
  if (h->released) return FCS_OK;  // its memory went with the device reset
  FCS_SET_DEVICE((h->device));
  for (void* m : h->mem)
    if (m) FCS_HIP_CHECK(hipFree(m));
  return FCS_OK;
}

int64_t fcs_fmd_collect_arena_bytes(int32_t n_reads, int32_t max_q_len) {
  if (n_reads < 0 || max_q_len < 0) return fail(FCS_ERR_INVALID, "[E::fcs_fmd_collect_arena_bytes] bad arguments");
  return fmd_collect_units(n_reads) * 2 * ((int64_t)max_q_len + 1) * (int64_t)sizeof(FmdIv);
}

int fcs_fmd_collect(const fcs_fmd_index* index, const uint8_t* codes, int64_t n_code_bytes, const int64_t* q_off,
                    const int32_t* q_len, int32_t n_reads, const fcs_fmd_params* params, fcs_fmd_mem* mems,
                    int32_t* n_mems, int32_t* overflow) {
  static const char* who = "fcs_fmd_collect";
  if (n_reads < 0 || n_code_bytes < 0 || (n_code_bytes > 0 && !codes) ||
      (n_reads > 0 && (!q_off || !q_len || !mems || !n_mems || !overflow)))
    return fail_invalid(who, "bad arguments");
  int32_t max_mems = 0;
  int rc = fmd_params_check(params, who, max_mems);
  if (rc) return rc;
  FmdReads R{codes, n_code_bytes, q_off, q_len, n_reads};
  if ((rc = R.check(who))) return rc;
  const fcs_fmd_index* h = fmd_handle(index, who);
  if (!h) return FCS_ERR_INVALID;
  if (n_reads == 0) return FCS_OK;
  if ((rc = check_device(h->device))) return rc;
  FCS_SET_DEVICE((h->device));
  const size_t n = (size_t)n_reads;
  // one H2D copy (the reads), one D2H copy (counts, flags, SMEMs)
  Arena L;
  R.plan(L);
  const size_t in_bytes = L.total;
  const size_t onm = L.add(4 * n), oovf = L.add(4 * n), omems = L.add(n * (size_t)max_mems * sizeof(FmdIv));
  const size_t host_bytes = L.total;
  const size_t oarena = L.add((size_t)fcs_fmd_collect_arena_bytes(n_reads, R.max_len));
  SessionLease lease;
  if ((rc = lease.acquire(h->device))) return rc;
  Session* S = lease.get();
  if ((rc = S->ensure_host(host_bytes)) || (rc = S->ensure_dev(L.total))) return rc;
  R.fill(S->hbase());
  hipStream_t s = S->s;
  const StreamDrain drain{s};
  FCS_HIP_CHECK(hipMemcpyAsync(S->d<void>(0), S->h<void>(0), in_bytes, hipMemcpyHostToDevice, s));
  if ((rc = launch_fmd_collect(h->dx, S->d<uint8_t>(R.o_codes), n_code_bytes, S->d<int64_t>(R.o_off),
                               S->d<int32_t>(R.o_len), S->d<int32_t>(R.o_ord), n_reads, fmd_params(params),
                               S->d<FmdIv>(oarena), R.max_len + 1, S->d<FmdIv>(omems), max_mems, S->d<int32_t>(onm),
                               S->d<int32_t>(oovf), s)))
    return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S->h<void>(onm), S->d<void>(onm), host_bytes - onm, hipMemcpyDeviceToHost, s));
  FCS_HIP_CHECK(hipStreamSynchronize(s));
  std::memcpy(n_mems, S->h<void>(onm), 4 * n);
  std::memcpy(overflow, S->h<void>(oovf), 4 * n);
  const FmdIv* hm = S->h<FmdIv>(omems);
  for (size_t r = 0; r < n; ++r) {  // only the slots a read filled, in bwa's final order
    const int32_t k = n_mems[r];
    if (k < 0 || k > max_mems) return fail(FCS_ERR_DEVICE, "[E::fcs_fmd_collect] read " + std::to_string(r) + " came back with " + std::to_string(k) + " SMEMs");
    fcs_fmd_mem* dst = mems + r * (size_t)max_mems;
    std::memcpy(dst, hm + r * (size_t)max_mems, (size_t)k * sizeof(FmdIv));
    std::stable_sort(dst, dst + k, [](const fcs_fmd_mem& a, const fcs_fmd_mem& b) { return a.qb != b.qb ? a.qb < b.qb : a.qe < b.qe; });
  }
  return FCS_OK;
}

int fcs_fmd_collect_dev(const fcs_fmd_index* index, const uint8_t* dev_codes, int64_t n_code_bytes,
                        const int64_t* dev_q_off, const int32_t* dev_q_len, const int32_t* dev_order, int32_t n_reads,
                        int32_t max_q_len, const fcs_fmd_params* params, void* dev_arena, int64_t arena_bytes,
                        fcs_fmd_mem* dev_mems, int32_t* dev_n_mems, int32_t* dev_overflow, void* stream) {
  if (n_reads < 0 || n_code_bytes < 0 || max_q_len < 0 || (n_code_bytes > 0 && !dev_codes) ||
      (n_reads > 0 && (!dev_q_off || !dev_q_len || !dev_mems || !dev_n_mems || !dev_overflow || !dev_arena)))
    return fail(FCS_ERR_INVALID, "[E::fcs_fmd_collect_dev] bad arguments");
  int32_t max_mems = 0;
  int rc = fmd_params_check(params, "fcs_fmd_collect_dev", max_mems);
  if (rc) return rc;
  if (n_reads > 0 && arena_bytes < fcs_fmd_collect_arena_bytes(n_reads, max_q_len))
    return fail(FCS_ERR_INVALID, "[E::fcs_fmd_collect_dev] the arena holds " + std::to_string(arena_bytes) +
                                     " bytes, the call needs " +
                                     std::to_string(fcs_fmd_collect_arena_bytes(n_reads, max_q_len)));
  const fcs_fmd_index* h = fmd_handle(index, "fcs_fmd_collect_dev");
  if (!h) return FCS_ERR_INVALID;
  if (n_reads == 0) return FCS_OK;
  if ((rc = check_device(h->device))) return rc;
  FCS_SET_DEVICE((h->device));
  return launch_fmd_collect(h->dx, dev_codes, n_code_bytes, dev_q_off, dev_q_len, dev_order, n_reads, fmd_params(params),
                            static_cast<FmdIv*>(dev_arena), max_q_len + 1, reinterpret_cast<FmdIv*>(dev_mems), max_mems,
                            dev_n_mems, dev_overflow, static_cast<hipStream_t>(stream));
}

int fcs_fmd_locate(const fcs_fmd_index* index, const int64_t* rows, int64_t n, int32_t max_steps, int64_t* pos,
                   int32_t* status) {
  const fcs_fmd_index* h = nullptr;
  int rc = fmd_locate_check(index, rows, n, max_steps, pos, status, "fcs_fmd_locate", h);
  if (rc || n == 0) return rc;
  if ((rc = check_device(h->device))) return rc;
  FCS_SET_DEVICE((h->device));
  const size_t m = (size_t)n;
  Arena L;
  const size_t orows = L.add(8 * m), opos = L.add(8 * m), ost = L.add(4 * m);
  SessionLease lease;
  if ((rc = lease.acquire(h->device))) return rc;
  Session* S = lease.get();
  if ((rc = S->ensure_host(L.total)) || (rc = S->ensure_dev(L.total))) return rc;
  std::memcpy(S->h<void>(orows), rows, 8 * m);
  hipStream_t s = S->s;
  const StreamDrain drain{s};
  FCS_HIP_CHECK(hipMemcpyAsync(S->d<void>(orows), S->h<void>(orows), 8 * m, hipMemcpyHostToDevice, s));
  if ((rc = launch_fmd_locate(h->dx, S->d<int64_t>(orows), n, max_steps, S->d<int64_t>(opos), S->d<int32_t>(ost), s)))
    return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S->h<void>(opos), S->d<void>(opos), L.total - opos, hipMemcpyDeviceToHost, s));
  FCS_HIP_CHECK(hipStreamSynchronize(s));
  std::memcpy(pos, S->h<void>(opos), 8 * m);
  std::memcpy(status, S->h<void>(ost), 4 * m);
  return FCS_OK;
}

int fcs_fmd_locate_dev(const fcs_fmd_index* index, const int64_t* dev_rows, int64_t n, int32_t max_steps,
                       int64_t* dev_pos, int32_t* dev_status, void* stream) {
  const fcs_fmd_index* h = nullptr;
  int rc = fmd_locate_check(index, dev_rows, n, max_steps, dev_pos, dev_status, "fcs_fmd_locate_dev", h);
  if (rc || n == 0) return rc;
  if ((rc = check_device(h->device))) return rc;
  FCS_SET_DEVICE((h->device));
  return launch_fmd_locate(h->dx, dev_rows, n, max_steps, dev_pos, dev_status, static_cast<hipStream_t>(stream));
}

int64_t fcs_fmd_seed_workspace_bytes(int32_t n_reads, int32_t max_q_len, int32_t max_mems, int64_t row_cap) {
  if (n_reads < 0 || max_q_len < 0 || max_mems < 1 || row_cap < 0)
    return fail(FCS_ERR_INVALID, "[E::fcs_fmd_seed_workspace_bytes] bad arguments");
  Arena L;
  (void)fmd_seed_ws(L, n_reads, max_q_len, max_mems, row_cap);
  return (int64_t)L.total;
}

int fcs_fmd_seed(const fcs_fmd_index* index, const uint8_t* codes, int64_t n_code_bytes, const int64_t* q_off,
                 const int32_t* q_len, int32_t n_reads, const fcs_fmd_seed_params* params, fcs_fmd_mem* mems,
                 int64_t mem_cap, int64_t* mem_off, int64_t* pos, int64_t row_cap, int64_t* row_off,
                 int32_t* overflow) {
  static const char* who = "fcs_fmd_seed";
  if (n_reads < 0 || n_code_bytes < 0 || (n_code_bytes > 0 && !codes) || (n_reads > 0 && (!q_off || !q_len)))
    return fail_invalid(who, "bad arguments");
  int32_t max_mems = 0;
  int rc = fmd_seed_check(params, mem_cap, row_cap, mems, mem_off, pos, row_off, overflow, n_reads, who, max_mems);
  if (rc) return rc;
  FmdReads R{codes, n_code_bytes, q_off, q_len, n_reads};
  if ((rc = R.check(who))) return rc;
  const fcs_fmd_index* h = fmd_handle(index, who);
  if (!h) return FCS_ERR_INVALID;
  if (n_reads == 0) {
    mem_off[0] = row_off[0] = 0;
    return FCS_OK;
  }
  if ((rc = check_device(h->device))) return rc;
  FCS_SET_DEVICE((h->device));
  const size_t n = (size_t)n_reads;
  // one H2D copy (the reads); back come the offsets and flags, then the SMEMs
  // and positions the totals count: nothing of the size of n_reads x max_mems
  // leaves the device
  Arena L;
  R.plan(L);
  const size_t in_bytes = L.total;
  const size_t omoff = L.add(8 * (n + 1)), oroff = L.add(8 * (n + 1)), oovf = L.add(4 * n);
  const size_t host_bytes = L.total;
  const size_t omems = L.add((size_t)mem_cap * sizeof(FmdIv)), opos = L.add(8 * (size_t)row_cap);
  const FmdSeedWs W = fmd_seed_ws(L, n_reads, R.max_len, max_mems, row_cap);
  SessionLease lease;
  if ((rc = lease.acquire(h->device))) return rc;
  Session* S = lease.get();
  if ((rc = S->ensure_host(host_bytes)) || (rc = S->ensure_dev(L.total))) return rc;
  R.fill(S->hbase());
  hipStream_t s = S->s;
  const StreamDrain drain{s};
  FCS_HIP_CHECK(hipMemcpyAsync(S->d<void>(0), S->h<void>(0), in_bytes, hipMemcpyHostToDevice, s));
  // every kernel is enqueued before the first sync: the host's look at the totals does not idle the device
  if ((rc = launch_fmd_collect(h->dx, S->d<uint8_t>(R.o_codes), n_code_bytes, S->d<int64_t>(R.o_off),
                               S->d<int32_t>(R.o_len), S->d<int32_t>(R.o_ord), n_reads, fmd_params(&params->collect),
                               S->d<FmdIv>(W.arena), R.max_len + 1, S->d<FmdIv>(W.slots), max_mems,
                               S->d<int32_t>(W.n_mems), S->d<int32_t>(oovf), s)) ||
      (rc = launch_fmd_seed(h->dx, S->d<FmdIv>(W.slots), max_mems, S->d<int32_t>(W.n_mems), S->d<int32_t>(oovf), n_reads,
                            params->max_occ, fmd_default_steps(h, params->max_steps), S->d<FmdSeedPlace>(W.place),
                            S->d<int32_t>(W.n_eff), S->d<int64_t>(W.n_rows), S->d<int64_t>(omoff), S->d<int64_t>(oroff),
                            S->d<FmdIv>(omems), mem_cap, S->d<int64_t>(W.rows), S->d<int64_t>(opos), row_cap, s)))
    return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S->h<void>(omoff), S->d<void>(omoff), host_bytes - omoff, hipMemcpyDeviceToHost, s));
  FCS_HIP_CHECK(hipStreamSynchronize(s));
  std::memcpy(mem_off, S->h<void>(omoff), 8 * (n + 1));
  std::memcpy(row_off, S->h<void>(oroff), 8 * (n + 1));
  std::memcpy(overflow, S->h<void>(oovf), 4 * n);
  const int64_t tm = mem_off[n], tr = row_off[n];
  if (tm < 0 || tr < 0 || tm > (int64_t)n * max_mems)
    return fail(FCS_ERR_DEVICE, "[E::fcs_fmd_seed] the totals came back as " + std::to_string(tm) + " SMEMs and " +
                                    std::to_string(tr) + " rows");
  if (tm > mem_cap || tr > row_cap) return FCS_FMD_SEED_MORE;
  if (tm == 0 && tr == 0) return FCS_OK;
  Arena B;
  const size_t bmems = B.add((size_t)tm * sizeof(FmdIv)), bpos = B.add(8 * (size_t)tr);
  if ((rc = S->ensure_host(B.total))) return rc;  // the staged inputs and offsets are spent
  if (tm) FCS_HIP_CHECK(hipMemcpyAsync(S->h<void>(bmems), S->d<void>(omems), (size_t)tm * sizeof(FmdIv), hipMemcpyDeviceToHost, s));
  if (tr) FCS_HIP_CHECK(hipMemcpyAsync(S->h<void>(bpos), S->d<void>(opos), 8 * (size_t)tr, hipMemcpyDeviceToHost, s));
  FCS_HIP_CHECK(hipStreamSynchronize(s));
  if (tm) std::memcpy(mems, S->h<void>(bmems), (size_t)tm * sizeof(FmdIv));
  if (tr) std::memcpy(pos, S->h<void>(bpos), 8 * (size_t)tr);
  return FCS_OK;
}

int fcs_fmd_seed_dev(const fcs_fmd_index* index, const uint8_t* dev_codes, int64_t n_code_bytes,
                     const int64_t* dev_q_off, const int32_t* dev_q_len, const int32_t* dev_order, int32_t n_reads,
                     int32_t max_q_len, const fcs_fmd_seed_params* params, void* dev_workspace,
                     int64_t workspace_bytes, fcs_fmd_mem* dev_mems, int64_t mem_cap, int64_t* dev_mem_off,
                     int64_t* dev_pos, int64_t row_cap, int64_t* dev_row_off, int32_t* dev_overflow, void* stream) {
  if (n_reads < 0 || n_code_bytes < 0 || max_q_len < 0 || (n_code_bytes > 0 && !dev_codes) ||
      (n_reads > 0 && (!dev_q_off || !dev_q_len || !dev_workspace)))
    return fail(FCS_ERR_INVALID, "[E::fcs_fmd_seed_dev] bad arguments");
  int32_t max_mems = 0;
  int rc = fmd_seed_check(params, mem_cap, row_cap, dev_mems, dev_mem_off, dev_pos, dev_row_off, dev_overflow, n_reads,
                          "fcs_fmd_seed_dev", max_mems);
  if (rc) return rc;
  Arena L;
  const FmdSeedWs W = fmd_seed_ws(L, n_reads, max_q_len, max_mems, row_cap);
  if (n_reads > 0 && workspace_bytes < (int64_t)L.total)
    return fail(FCS_ERR_INVALID, "[E::fcs_fmd_seed_dev] the workspace holds " + std::to_string(workspace_bytes) +
                                     " bytes, the call needs " + std::to_string(L.total));
  const fcs_fmd_index* h = fmd_handle(index, "fcs_fmd_seed_dev");
  if (!h) return FCS_ERR_INVALID;
  if ((rc = check_device(h->device))) return rc;
  FCS_SET_DEVICE((h->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(dev_workspace);
  auto at = [&](size_t off) { return static_cast<void*>(ws + off); };
  if (n_reads > 0 &&
      (rc = launch_fmd_collect(h->dx, dev_codes, n_code_bytes, dev_q_off, dev_q_len, dev_order, n_reads,
                               fmd_params(&params->collect), static_cast<FmdIv*>(at(W.arena)), max_q_len + 1,
                               static_cast<FmdIv*>(at(W.slots)), max_mems, static_cast<int32_t*>(at(W.n_mems)),
                               dev_overflow, s)))
    return rc;
  if (n_reads == 0)  // only the two zero totals are written
    return launch_fmd_seed(h->dx, nullptr, max_mems, nullptr, nullptr, 0, params->max_occ, 1, nullptr, nullptr, nullptr,
                           dev_mem_off, dev_row_off, nullptr, mem_cap, nullptr, dev_pos, row_cap, s);
  return launch_fmd_seed(h->dx, static_cast<FmdIv*>(at(W.slots)), max_mems, static_cast<int32_t*>(at(W.n_mems)),
                         dev_overflow, n_reads, params->max_occ, fmd_default_steps(h, params->max_steps),
                         static_cast<FmdSeedPlace*>(at(W.place)), static_cast<int32_t*>(at(W.n_eff)),
                         static_cast<int64_t*>(at(W.n_rows)), dev_mem_off, dev_row_off,
                         reinterpret_cast<FmdIv*>(dev_mems), mem_cap, static_cast<int64_t*>(at(W.rows)), dev_pos, row_cap, s);
}

}  // extern "C"
