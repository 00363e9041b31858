// Duplicate marking of BAM records (markdup.h): mate matching, flattening,
// the device call or the host rules (markdup.cpp), flags, and the markdup command.
#include "markdup.h"

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <string_view>
#include <unordered_map>

#include "bam_stream.h"
#include "common.h"
#include "fcship.h"
#include "flat_batch.h"

namespace fcsg {

namespace {
bool examined(uint16_t flag) { return (flag & (kUnmapped | kSecondary | kSupplementary)) == 0; }
}  // namespace

std::vector<int32_t> match_mates(const std::vector<BamRecord>& recs) {
  std::vector<int32_t> mate(recs.size(), -1);
  // name -> the first primary record of read 1 and of read 2
  std::unordered_map<std::string_view, std::array<int32_t, 2>> by_name;
  by_name.reserve(recs.size());
  for (size_t r = 0; r < recs.size(); ++r) {
    const uint16_t f = recs[r].flag;
    if (!(f & kPaired) || (f & (kSecondary | kSupplementary))) continue;
    const bool r1 = f & kRead1, r2 = f & kRead2;
    if (r1 == r2) continue;  // neither or both: not one end of a pair
    auto it = by_name.try_emplace(std::string_view(recs[r].name), std::array<int32_t, 2>{-1, -1}).first;
    int32_t& slot = it->second[r2 ? 1 : 0];
    if (slot < 0) slot = (int32_t)r;
  }
  for (const auto& kv : by_name) {
    const int32_t a = kv.second[0], c = kv.second[1];
    if (a >= 0 && c >= 0) mate[a] = c, mate[c] = a;
  }
  return mate;
}

namespace {

struct DupApi {
  decltype(&fcsdup_mark) mark = FCSG_DEVICE_ENTRY(fcsdup_mark);
};

const DupApi& dup_api() {
  static const DupApi A;
  return A;
}

}  // namespace

bool gpu_markdup_available() { return dup_api().mark && last_error_entry(); }

MarkdupStats mark_duplicates(std::vector<BamRecord>& recs, const std::vector<int32_t>& lib, int32_t n_lib, int32_t n_ref,
                             int device) {
  const uint64_t t0 = now_us();
  const size_t n = recs.size();
  if (lib.size() != n) throw internalError("[E::fcsg] markdup: one library index per record");
  const std::vector<int32_t> mate = match_mates(recs);
  std::vector<uint16_t> flag(n);
  std::vector<int32_t> ref_id(n), pos(n);
  std::vector<int64_t> cigar_off(n + 1, 0), qual_off(n + 1, 0);
  for (size_t r = 0; r < n; ++r) {
    flag[r] = recs[r].flag, ref_id[r] = recs[r].ref_id, pos[r] = recs[r].pos;
    cigar_off[r + 1] = cigar_off[r] + (int64_t)recs[r].cigar.size();
    qual_off[r + 1] = qual_off[r] + (int64_t)recs[r].qual.size();
  }
  std::vector<uint32_t> cigar((size_t)cigar_off[n]);
  std::vector<uint8_t> qual((size_t)qual_off[n]);
  parallel_for(n, host_threads(), [&](size_t r) {
    if (!recs[r].cigar.empty()) std::memcpy(cigar.data() + cigar_off[r], recs[r].cigar.data(), 4 * recs[r].cigar.size());
    if (!recs[r].qual.empty()) std::memcpy(qual.data() + qual_off[r], recs[r].qual.data(), recs[r].qual.size());
  });
  fcsdup_batch b;
  b.n = (int64_t)n;
  b.flag = flag.data(), b.ref_id = ref_id.data(), b.pos = pos.data(), b.mate = mate.data(), b.lib = lib.data();
  b.cigar = cigar.data(), b.cigar_off = cigar_off.data(), b.n_cigar = cigar_off[n];
  b.qual = qual.data(), b.qual_off = qual_off.data(), b.n_qual = qual_off[n];
  b.n_ref = n_ref, b.n_lib = n_lib;
  std::vector<uint8_t> dup(n, 0);
  MarkdupStats st;
  const bool on_device =
      device_or_host(device, gpu_markdup_available(),
                     "[fcs-genome markdup] markdup.gpu: the loaded libfcship has no fcsdup_mark entry point; "
                     "duplicates are marked on the host\n") >= 0;
  if (on_device) {
    fcsdup_stats ds;
    device_check(dup_api().mark(device, &b, dup.data(), &ds), "markdup", "fcsdup_mark");
    st.examined = ds.examined, st.pairs = ds.pairs, st.fragments = ds.fragments, st.duplicates = ds.duplicates;
  } else {
    st = mark_duplicates_host(b, dup.data());
  }
  for (size_t r = 0; r < n; ++r)
    if (examined(recs[r].flag))
      recs[r].flag = (uint16_t)(dup[r] ? recs[r].flag | kDuplicate : recs[r].flag & ~kDuplicate);
  st.on_device = on_device;
  st.seconds = (now_us() - t0) / 1e6;
  return st;
}

int32_t libraries_of(const BamHeader& h, const std::vector<BamRecord>& recs, std::vector<int32_t>& lib) {
  std::unordered_map<std::string, int32_t> lib_of_name, lib_of_rg;
  for (const RgLine& line : rg_lines(h)) {
    const std::string id = line.get("ID"), lb = line.get("LB");
    if (id.empty()) continue;
    int32_t k = 0;
    if (!lb.empty()) k = lib_of_name.try_emplace(lb, (int32_t)lib_of_name.size() + 1).first->second;
    lib_of_rg[id] = k;
  }
  lib.assign(recs.size(), 0);
  std::string rg;
  for (size_t r = 0; r < recs.size(); ++r)
    if (recs[r].get_aux_string("RG", rg)) {
      const auto it = lib_of_rg.find(rg);
      if (it != lib_of_rg.end()) lib[r] = it->second;
    }
  return (int32_t)lib_of_name.size() + 1;
}

MarkdupStats markdup_bam(const std::string& input, const std::string& output, int device) {
  BamStream in(input, false);
  const BamHeader& h = in.header();
  std::vector<BamRecord> recs;
  in.read(recs, SIZE_MAX);
  std::vector<int32_t> lib;
  const int32_t n_lib = libraries_of(h, recs, lib);
  const MarkdupStats st = mark_duplicates(recs, lib, n_lib, (int32_t)h.names.size(), device);
  BamWriter w(output, h);
  if (h.text.find("SO:coordinate") != std::string::npos) w.index_on_close();
  std::vector<const BamRecord*> all(recs.size());
  for (size_t i = 0; i < recs.size(); ++i) all[i] = &recs[i];
  w.write_all(all);
  w.close();
  return st;
}

}  // namespace fcsg
