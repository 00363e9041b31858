// BGZF calls of the C-ABI (include/fcship.h): the member index, inflate and
// deflate through the BGZF session pool (fcs_bgzf_warmup, which fills that
// pool, is in session.cpp with the other warm-ups).
#include <chrono>
#include <cstdio>
#include <cstring>

#include "session.h"

using namespace fcs;

extern "C" {

int fcs_bgzf_index(const uint8_t* comp, int64_t comp_bytes, int64_t* coff, int64_t* uoff, int32_t cap,
                   int32_t* n_members, int64_t* comp_used) {
  if (!n_members || !comp_used || comp_bytes < 0 || cap < 0 || (comp_bytes > 0 && !comp) || !coff || !uoff)
    return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_index] bad arguments");
  auto le16 = [&](int64_t at) { return (uint32_t)comp[at] | (uint32_t)comp[at + 1] << 8; };
  int64_t at = 0, u = 0;
  int32_t k = 0;
  while (k < cap && comp_bytes - at >= 18) {
    // gzip member with FEXTRA (RFC 1952) carrying the BGZF "BC" subfield
    if (comp[at] != 31 || comp[at + 1] != 139 || comp[at + 2] != 8 || !(comp[at + 3] & 4))
      return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_index] no BGZF header at byte " + std::to_string(at));
    const int64_t xlen = le16(at + 10);
    if (comp_bytes - at < 12 + xlen) break;
    int64_t bsize = -1;
    for (int64_t x = at + 12; x + 4 <= at + 12 + xlen;) {
      const int64_t slen = le16(x + 2);
      if (comp[x] == 'B' && comp[x + 1] == 'C' && slen == 2 && x + 6 <= at + 12 + xlen) bsize = le16(x + 4);
      x += 4 + slen;
    }
    if (bsize < 0 || bsize + 1 < 12 + xlen + 8)
      return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_index] no BGZF block size at byte " + std::to_string(at));
    const int64_t len = bsize + 1;
    if (comp_bytes - at < len) break;  // incomplete: left for the next call
    const int64_t isize = (int64_t)(le16(at + len - 4) | le16(at + len - 2) << 16);
    if (isize > 65536)
      return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_index] member at byte " + std::to_string(at) + " inflates past 64 KiB");
    coff[k] = at;
    uoff[k] = u;
    at += len;
    u += isize;
    ++k;
  }
  coff[k] = at;
  uoff[k] = u;
  *n_members = k;
  *comp_used = at;
  return FCS_OK;
}

int fcs_bgzf_inflate_dev(const uint8_t* dev_comp, const int64_t* dev_coff, const int64_t* dev_uoff, int32_t n,
                         uint8_t* dev_out, int32_t* dev_status, int32_t device, void* stream) {
  if (n < 0 || (n > 0 && (!dev_comp || !dev_coff || !dev_uoff || !dev_out || !dev_status)))
    return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_inflate_dev] bad arguments");
  if (n == 0) return FCS_OK;
  int rc = check_device(device);
  if (rc) return rc;
  FCS_SET_DEVICE((device));
  return launch_bgzf_inflate(dev_comp, dev_coff, dev_uoff, n, dev_out, dev_status, static_cast<hipStream_t>(stream));
}

}  // extern "C"

namespace {

// fcs_bgzf_inflate / fcs_bgzf_inflate_try: `try_only` takes an idle inflate
// session whose arenas already fit the call, or returns FCS_BGZF_BUSY.
int bgzf_inflate_host(const uint8_t* comp, int64_t comp_bytes, uint8_t* out, int64_t out_cap, int64_t* comp_used,
                      int64_t* out_bytes, int32_t device, bool try_only) {
  if (!comp_used || !out_bytes || comp_bytes < 0 || (comp_bytes > 0 && !comp) || out_cap < 0 || (out_cap > 0 && !out))
    return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_inflate] bad arguments");
  *comp_used = 0;
  *out_bytes = 0;
  // a member is at least 28 bytes (18 of header / trailer, 2 of DEFLATE); the
  // offset tables are this thread's, kept between calls (no fresh zeroed
  // pages per call)
  const int64_t most = std::min<int64_t>(comp_bytes / 20 + 1, 0x7FFFFFFE);
  static thread_local std::vector<int64_t> coff, uoff;
  if (coff.size() < (size_t)most + 1) {
    coff.resize((size_t)most + 1);
    uoff.resize((size_t)most + 1);
  }
  int32_t n = 0;
  int64_t used = 0;
  int rc = fcs_bgzf_index(comp, comp_bytes, coff.data(), uoff.data(), (int32_t)most, &n, &used);
  if (rc) return rc;
  const int64_t total = uoff[(size_t)n];
  if (total > out_cap)
    return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_inflate] output needs " + std::to_string(total) + " bytes, capacity " +
                                     std::to_string(out_cap));
  *comp_used = used;
  if (n == 0) return FCS_OK;
  if ((rc = check_device(device))) return rc;
  FCS_SET_DEVICE((device));
  // FCS_BGZF_TRACE=1: one stderr line per call with its phases (ms)
  static const bool trace = std::getenv("FCS_BGZF_TRACE") != nullptr;
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  auto ms = [&](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
  const size_t nn = (size_t)n;
  Arena L;
  const size_t oco = L.add(8 * (nn + 1)), ouo = L.add(8 * (nn + 1)), ocp = L.add((size_t)used + 16);
  const size_t in_bytes = L.total, ost = L.add(4 * nn), oout = L.add((size_t)total);
  SessionLease lease;
  if (try_only) {
    if (!lease.try_acquire(device, kInflateSession, L.total)) {
      *comp_used = 0;
      return FCS_BGZF_BUSY;
    }
  } else if ((rc = lease.acquire(device, kInflateSession))) {
    return rc;
  }
  Session* S = lease.get();
  // Through the session's pinned staging arena.  Copies straight from and to
  // the caller's pageable buffers with device scratch from the stream-ordered
  // pool were tried: with 16 shard threads calling at once, member 0 of a
  // call came out corrupt in about one htc run in four (r5ae, r5al, r5am),
  // never with the pinned arena.
  const double t_lease = ms(t0);
  if ((rc = S->ensure_host(L.total)) || (rc = S->ensure_dev(L.total))) return rc;
  const double t_alloc = ms(t0);
  std::memcpy(S->h<void>(oco), coff.data(), 8 * (nn + 1));
  std::memcpy(S->h<void>(ouo), uoff.data(), 8 * (nn + 1));
  std::memcpy(S->h<void>(ocp), comp, (size_t)used);
  const double t_in = ms(t0);
  hipStream_t s = S->s;
  const StreamDrain drain{s};
  FCS_HIP_CHECK(hipMemcpyAsync(S->dev, S->host, in_bytes, hipMemcpyHostToDevice, s));
  if ((rc = launch_bgzf_inflate(S->d<uint8_t>(ocp), S->d<int64_t>(oco), S->d<int64_t>(ouo), n, S->d<uint8_t>(oout),
                                S->d<int32_t>(ost), s)))
    return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S->h<void>(ost), S->d<void>(ost), L.total - ost, hipMemcpyDeviceToHost, s));
  // the calling shard thread sleeps until the copy lands: a spinning wait of
  // 16 shard threads costs more host time than the inflate saves
  if (!S->done) FCS_HIP_CHECK(hipEventCreateWithFlags(&S->done, hipEventBlockingSync | hipEventDisableTiming));
  FCS_HIP_CHECK(hipEventRecord(S->done, s));
  FCS_HIP_CHECK(hipEventSynchronize(S->done));
  const double t_gpu = ms(t0);
  const int32_t* st = S->h<int32_t>(ost);
  for (size_t k = 0; k < nn; ++k)
    if (st[k] != FCS_BGZF_OK) {
      static const char* what[4] = {"ok", "corrupt DEFLATE stream", "inflates past its ISIZE", "CRC-32 mismatch"};
      return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_inflate] member " + std::to_string(k) + " at byte " +
                                       std::to_string(coff[k]) + ": " + what[st[k] & 3]);
    }
  std::memcpy(out, S->h<void>(oout), (size_t)total);
  *out_bytes = total;
  if (trace)
    std::fprintf(stderr, "[fcs_bgzf_inflate] %d members, %lld -> %lld bytes: lease %.2f alloc %.2f in %.2f gpu %.2f out %.2f ms\n",
                 n, (long long)used, (long long)total, t_lease, t_alloc - t_lease, t_in - t_alloc, t_gpu - t_in,
                 ms(t0) - t_gpu);
  return FCS_OK;
}

const uint8_t kBgzfEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43,
                              0x02, 0,    0x1b, 0,    0x03, 0, 0, 0, 0, 0, 0,    0, 0,    0};

// fcs_bgzf_deflate / fcs_bgzf_deflate_try (`try_only`: an idle BGZF session
// whose arenas already fit the call, or FCS_BGZF_BUSY).
int bgzf_deflate_host(const uint8_t* data, int64_t n_bytes, int32_t block_bytes, int32_t eof, uint8_t* out,
                      int64_t out_cap, int64_t* out_bytes, int64_t* coff, int32_t* n_members, int32_t device,
                      bool try_only) {
  if (!out_bytes || !n_members || n_bytes < 0 || (n_bytes > 0 && !data) || out_cap < 0 || (out_cap > 0 && !out))
    return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_deflate] bad arguments");
  if (block_bytes < 1 || block_bytes > FCS_BGZF_BLOCK_MAX)
    return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_deflate] block_bytes " + std::to_string(block_bytes) + " outside 1.." +
                                     std::to_string(FCS_BGZF_BLOCK_MAX));
  *out_bytes = 0;
  *n_members = 0;
  const int64_t members = (n_bytes + block_bytes - 1) / block_bytes, tail = eof ? 28 : 0;
  if (members > 0x7FFFFFFE)
    return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_deflate] " + std::to_string(members) + " members in one call");
  if (members == 0) {
    if (tail > out_cap)
      return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_deflate] output needs 28 bytes, capacity " + std::to_string(out_cap));
    if (tail) std::memcpy(out, kBgzfEof, 28);
    if (coff) coff[0] = 0;
    *out_bytes = tail;
    return FCS_OK;
  }
  int rc = check_device(device);
  if (rc) return rc;
  FCS_SET_DEVICE((device));
  const size_t nm = (size_t)members;
  // staged through the host arena: the input, the member starts, the compacted
  // members; on the device alone: the member sizes and the 64 KiB slots
  Arena L;
  const size_t odata = L.add((size_t)n_bytes), ocoff = L.add(8 * (nm + 1));
  const size_t oout = L.add((size_t)n_bytes + nm * 31);  // a member is at most its stored form: 18 + 5 + n + 8
  const size_t host_bytes = L.total, oclen = L.add(4 * nm), oslots = L.add(nm * 65536);
  SessionLease lease;
  if (try_only) {
    if (!lease.try_acquire(device, kInflateSession, host_bytes, L.total)) return FCS_BGZF_BUSY;
  } else if ((rc = lease.acquire(device, kInflateSession))) {
    return rc;
  }
  Session* S = lease.get();
  if ((rc = S->ensure_host(host_bytes)) || (rc = S->ensure_dev(L.total))) return rc;
  std::memcpy(S->h<void>(odata), data, (size_t)n_bytes);
  hipStream_t s = S->s;
  const StreamDrain drain{s};
  FCS_HIP_CHECK(hipMemcpyAsync(S->d<void>(odata), S->h<void>(odata), (size_t)n_bytes, hipMemcpyHostToDevice, s));
  if ((rc = launch_bgzf_deflate(S->d<uint8_t>(odata), n_bytes, block_bytes, S->d<uint8_t>(oslots), S->d<int32_t>(oclen), s)) ||
      (rc = launch_bgzf_compact(S->d<uint8_t>(oslots), S->d<int32_t>(oclen), (int32_t)members, S->d<int64_t>(ocoff),
                                S->d<uint8_t>(oout), s)))
    return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S->h<void>(ocoff), S->d<void>(ocoff), 8 * (nm + 1), hipMemcpyDeviceToHost, s));
  if (!S->done) FCS_HIP_CHECK(hipEventCreateWithFlags(&S->done, hipEventBlockingSync | hipEventDisableTiming));
  FCS_HIP_CHECK(hipEventRecord(S->done, s));
  FCS_HIP_CHECK(hipEventSynchronize(S->done));
  const int64_t* hc = S->h<int64_t>(ocoff);
  for (size_t k = 0; k < nm; ++k)
    if (hc[k + 1] - hc[k] < 28 || hc[k + 1] - hc[k] > 65536)  // a failed member counts 0 bytes
      return fail(FCS_ERR_DEVICE, "[E::fcs_bgzf_deflate] member " + std::to_string(k) + " was not encoded");
  const int64_t total = hc[nm];
  if (total + tail > out_cap)
    return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_deflate] output needs " + std::to_string(total + tail) +
                                     " bytes, capacity " + std::to_string(out_cap));
  // one copy of the compressed bytes alone
  FCS_HIP_CHECK(hipMemcpyAsync(S->h<void>(oout), S->d<void>(oout), (size_t)total, hipMemcpyDeviceToHost, s));
  FCS_HIP_CHECK(hipEventRecord(S->done, s));
  FCS_HIP_CHECK(hipEventSynchronize(S->done));
  std::memcpy(out, S->h<void>(oout), (size_t)total);
  if (tail) std::memcpy(out + total, kBgzfEof, 28);
  if (coff) std::memcpy(coff, hc, 8 * (nm + 1));
  *out_bytes = total + tail;
  *n_members = (int32_t)members;
  return FCS_OK;
}

}  // namespace

extern "C" {

int fcs_bgzf_inflate(const uint8_t* comp, int64_t comp_bytes, uint8_t* out, int64_t out_cap, int64_t* comp_used,
                     int64_t* out_bytes, int32_t device) {
  return bgzf_inflate_host(comp, comp_bytes, out, out_cap, comp_used, out_bytes, device, false);
}

int fcs_bgzf_inflate_try(const uint8_t* comp, int64_t comp_bytes, uint8_t* out, int64_t out_cap, int64_t* comp_used,
                         int64_t* out_bytes, int32_t device) {
  return bgzf_inflate_host(comp, comp_bytes, out, out_cap, comp_used, out_bytes, device, true);
}

int64_t fcs_bgzf_deflate_bound(int64_t n_bytes, int32_t block_bytes, int32_t eof) {
  if (n_bytes < 0 || block_bytes < 1 || block_bytes > FCS_BGZF_BLOCK_MAX)
    return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_deflate_bound] bad arguments");
  return (n_bytes + block_bytes - 1) / block_bytes * 65536 + (eof ? 28 : 0);
}

int fcs_bgzf_deflate(const uint8_t* data, int64_t n_bytes, int32_t block_bytes, int32_t eof, uint8_t* out,
                     int64_t out_cap, int64_t* out_bytes, int64_t* coff, int32_t* n_members, int32_t device) {
  return bgzf_deflate_host(data, n_bytes, block_bytes, eof, out, out_cap, out_bytes, coff, n_members, device, false);
}

int fcs_bgzf_deflate_try(const uint8_t* data, int64_t n_bytes, int32_t block_bytes, int32_t eof, uint8_t* out,
                         int64_t out_cap, int64_t* out_bytes, int64_t* coff, int32_t* n_members, int32_t device) {
  return bgzf_deflate_host(data, n_bytes, block_bytes, eof, out, out_cap, out_bytes, coff, n_members, device, true);
}

int fcs_bgzf_deflate_dev(const uint8_t* dev_data, int64_t n_bytes, int32_t block_bytes, uint8_t* dev_slots,
                         int32_t* dev_clen, int32_t device, void* stream) {
  if (n_bytes < 0 || (n_bytes > 0 && (!dev_data || !dev_slots || !dev_clen)) || ((uintptr_t)dev_slots & 3))
    return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_deflate_dev] bad arguments");
  if (block_bytes < 1 || block_bytes > FCS_BGZF_BLOCK_MAX)
    return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_deflate_dev] block_bytes " + std::to_string(block_bytes) +
                                     " outside 1.." + std::to_string(FCS_BGZF_BLOCK_MAX));
  if ((n_bytes + block_bytes - 1) / block_bytes > 0x7FFFFFFE)
    return fail(FCS_ERR_INVALID, "[E::fcs_bgzf_deflate_dev] too many members in one call");
  if (n_bytes == 0) return FCS_OK;
  int rc = check_device(device);
  if (rc) return rc;
  FCS_SET_DEVICE((device));
  return launch_bgzf_deflate(dev_data, n_bytes, block_bytes, dev_slots, dev_clen, static_cast<hipStream_t>(stream));
}

}  // extern "C"
