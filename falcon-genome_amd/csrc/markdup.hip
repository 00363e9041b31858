// Duplicate marking on the device (include/fcsdup.h; DESIGN §2 [EXT], §4.9).
// The per-record and per-pair logic is csrc/md_keys.h (one text for these
// kernels, host/markdup.cpp and tools/micro/markdup_test.cpp).  All work of a
// call is queued on one stream, without a host round trip:
//
// md_ends_kernel: one record per 16-lane DPP row, four per wave.  The row's
// lanes read the record's quality bytes as aligned dwords (the head and tail
// dwords masked to the record's bytes, at any byte offset), add the bytes >=
// 15 and sum across the row with four DPP rotations; lane 0 of the row walks
// the CIGAR (at most the record's word count, itself clamped to n_cigar) and
// writes the record's fragment key E, its score and its examined bit.
// md_ends_kernel is built for 8 waves per SIMD.
//
// md_keys_kernel: one lane per record.  The class from the mate's examined bit;
// the fragment-list entry (E, winner word, bit 63 for a paired record) of every
// examined record and the all-ones sentinel for the others; the pair-list entry
// (K as two words, the pair's winner word) at the lesser record index of each
// pair, the sentinel elsewhere.
// md_keys_kernel is built for 8 waves per SIMD.
//
// Sorts: rocPRIM stable radix sorts of (key, record) pairs: the fragment list
// once by E; the pair list by K's low word, then (md_gather_kernel carries the
// high words along) by its high word.
// md_gather_kernel is built for 8 waves per SIMD.
//
// md_resolve_heads_kernel, a rocPRIM inclusive scan, md_resolve_best_kernel and
// md_resolve_mark_kernel: a head flag where the sorted key changes, segment
// ids by the scan, one 64-bit atomicMax of the winner word per element into
// best[segment] (a max does not depend on arrival order), then every element
// that is not its segment's winner is marked, and every fragment whose
// segment's winner is a paired record.  Only ones are stored into dup (zeroed
// first); a pair stores both its records.
// md_resolve_heads_kernel is built for 8 waves per SIMD.
// md_resolve_best_kernel is built for 8 waves per SIMD.
// md_resolve_mark_kernel is built for 8 waves per SIMD.
//
// Every loop is bounded by n, a record's clamped CIGAR word count or its
// clamped quality length; no kernel uses scratch or LDS.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstring>
#include <string>

#include "fcsdup.h"
#include "fcship_internal.h"
#include "md_keys.h"
#include "rec_batch.h"

namespace fcs {

namespace {

constexpr int kMdRow = 16;
constexpr int kMdBlock = 256;
constexpr int kMdMaxBlocks = 256 * 8;

// Where a call's device scratch lies (fcsdup_workspace_bytes).
struct MdWs {
  size_t endk, score, ex, wfrag, wpair, fkey, fval, phi, plo, pval, k64a, k64b, v32a, v32b, head, seg, best, tmp;
  size_t tmp_bytes, total;
};

MdWs md_ws(int64_t n_records) {
  const size_t n = (size_t)std::max<int64_t>(n_records, 1);
  Arena A;
  MdWs w;
  w.endk = A.add(8 * n), w.score = A.add(4 * n), w.ex = A.add(n), w.wfrag = A.add(8 * n), w.wpair = A.add(8 * n);
  w.fkey = A.add(8 * n), w.fval = A.add(4 * n), w.phi = A.add(8 * n), w.plo = A.add(8 * n), w.pval = A.add(4 * n);
  w.k64a = A.add(8 * n), w.k64b = A.add(8 * n), w.v32a = A.add(4 * n), w.v32b = A.add(4 * n);
  w.head = A.add(4 * n), w.seg = A.add(4 * n), w.best = A.add(8 * n);
  // rocPRIM's scratch for a sort of n (64-bit key, 32-bit value) pairs with
  // separate outputs: a second key and value array, histograms and look-back
  // states.  Reserved by a formula so that the size is known without a device;
  // every launch checks what rocPRIM asks for against it.
  w.tmp_bytes = 24 * n + ((size_t)4 << 20);
  w.tmp = A.add(w.tmp_bytes);
  w.total = A.total;
  return w;
}

__device__ __forceinline__ uint32_t row_sum(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kDppRowRor8, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kDppRowRor4, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kDppRowRor2, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kDppRowRor1, 0xF, 0xF, false);
  return v;
}

__global__ __launch_bounds__(kMdBlock) void md_ends_kernel(MdDevBatch b, int32_t n_ref, int32_t n_lib,
                                                           uint64_t* __restrict__ endk, uint32_t* __restrict__ score,
                                                           uint8_t* __restrict__ ex, int32_t* __restrict__ status) {
  constexpr int kRows = kMdBlock / kMdRow;
  const int g = (int)threadIdx.x / kMdRow, l = (int)threadIdx.x % kMdRow;
  const int64_t stride = (int64_t)gridDim.x * kRows;
  for (int64_t r0 = (int64_t)blockIdx.x * kRows; r0 < b.n; r0 += stride) {  // the same rounds for the whole block
    const int64_t r = r0 + g;
    const bool live = r < b.n;
    const uint16_t flag = live ? b.flag[r] : kMdFlagUnmapped;
    const bool exm = live && md_examined(flag);
    int bad = 0;
    uint32_t s = 0;
    if (exm) {
      const int64_t o0 = b.qual_off[r], o1 = b.qual_off[r + 1];
      const int64_t q0 = clamp64(o0, 0, b.n_qual), q1 = clamp64(o1, q0, clamp64(q0 + kMdMaxQual, q0, b.n_qual));
      bad |= (q0 != o0 || q1 != o1) ? FCSDUP_STATUS_FIELD : 0;
      if (q1 > q0) {
        const uintptr_t a0 = (uintptr_t)b.qual + (uintptr_t)q0, a1 = (uintptr_t)b.qual + (uintptr_t)q1;
        const uintptr_t w0 = a0 & ~(uintptr_t)3;
        const int64_t n_words = (int64_t)((((a1 + 3) & ~(uintptr_t)3) - w0) >> 2);  // <= kMdMaxQual / 4 + 1
        for (int64_t w = l; w < n_words; w += kMdRow) {
          const uintptr_t wa = w0 + 4 * (uintptr_t)w;
          const uint32_t v = *reinterpret_cast<const uint32_t*>(wa);
          const int lo = wa < a0 ? (int)(a0 - wa) : 0;
          const int hi = wa + 4 > a1 ? (int)(a1 - wa) : 4;
          s += md_score_word(v, lo, hi);
        }
      }
    }
    s = row_sum(s);  // every lane of the wave is here: the trip count above is the block's
    if (l == 0 && live) {
      uint64_t key = kMdSentinel;
      if (exm) {
        const int64_t o0 = b.cigar_off[r], o1 = b.cigar_off[r + 1];
        const int64_t c0 = clamp64(o0, 0, b.n_cigar), c1 = clamp64(o1, c0, b.n_cigar);
        bad |= (c0 != o0 || c1 != o1) ? FCSDUP_STATUS_FIELD : 0;
        const bool rev = (flag & kMdFlagReverse) != 0;
        int64_t u5 = md_u5(b.pos[r], rev, b.cigar + c0, c1 - c0);
        if (!md_fits_u5(u5)) bad |= FCSDUP_STATUS_POS, u5 = 0;
        int32_t ref = b.ref_id[r], lib = b.lib[r];
        if (ref < -1 || ref >= n_ref || lib < 0 || lib >= n_lib) bad |= FCSDUP_STATUS_FIELD, ref = -1, lib = 0;
        key = md_frag_key(lib, md_end_word(ref, u5, rev));
      }
      endk[r] = key;
      score[r] = s;
      ex[r] = exm ? 1 : 0;
    }
    if (bad) atomicOr(status, bad);
  }
}

// What md_keys_kernel adds to the statistics: one atomic per wave and counter.
__device__ __forceinline__ void count_lanes(bool pred, unsigned long long* counter) {
  const unsigned long long m = __ballot(pred);
  if (m && (int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(counter, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(kMdBlock) void md_keys_kernel(MdDevBatch b, const uint64_t* __restrict__ endk,
                                                           const uint32_t* __restrict__ score,
                                                           const uint8_t* __restrict__ ex, uint64_t* __restrict__ fkey,
                                                           int32_t* __restrict__ fval, uint64_t* __restrict__ wfrag,
                                                           uint64_t* __restrict__ phi, uint64_t* __restrict__ plo,
                                                           int32_t* __restrict__ pval, uint64_t* __restrict__ wpair,
                                                           unsigned long long* __restrict__ stats) {
  const int64_t stride = (int64_t)gridDim.x * kMdBlock;
  const int64_t rounds = (b.n + stride - 1) / stride;
  int64_t r = (int64_t)blockIdx.x * kMdBlock + threadIdx.x;
  for (int64_t k = 0; k < rounds; ++k, r += stride) {  // the same rounds for every lane: the ballots see whole waves
    const bool live = r < b.n;
    const bool exm = live && ex[r] != 0;
    bool paired = false, emits = false;
    uint64_t fk = kMdSentinel, wf = 0, hi = kMdSentinel, lo = 0, wp = 0;
    if (exm) {
      const uint16_t flag = b.flag[r];
      int32_t m = b.mate[r];
      if (m < 0 || m >= b.n || m == r) m = -1;
      paired = (flag & kMdFlagPaired) && !(flag & kMdFlagMateUnmapped) && m >= 0 && ex[m] != 0;
      fk = endk[r];
      const uint32_t sr = score[r];
      wf = md_winner(sr, (int32_t)r) | (paired ? kMdPairedBit : 0);
      if (paired && r < m) {
        const uint16_t fm = b.flag[m];
        // the mate is paired too, with this record (which is examined)
        emits = (fm & kMdFlagPaired) && !(fm & kMdFlagMateUnmapped) && b.mate[m] == (int32_t)r;
        if (emits) {
          const uint64_t km = endk[m];
          const uint64_t mask = ((uint64_t)1 << kMdEndBits) - 1;
          const bool first = md_end_before(fk & mask, (int32_t)r, km & mask, m);
          md_pair_key(first ? fk : km, first ? km : fk, hi, lo);
          wp = md_winner(sr + score[m], (int32_t)r);
        }
      }
    }
    if (live) {
      fkey[r] = fk, fval[r] = (int32_t)r, wfrag[r] = wf;
      phi[r] = hi, plo[r] = lo, pval[r] = (int32_t)r, wpair[r] = wp;
    }
    count_lanes(exm, stats + 0);
    count_lanes(emits, stats + 1);
    count_lanes(exm && !paired, stats + 2);
  }
}

__global__ __launch_bounds__(kMdBlock) void md_gather_kernel(const uint64_t* __restrict__ by_record,
                                                             const int32_t* __restrict__ val, int64_t n,
                                                             uint64_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * kMdBlock;
  for (int64_t i = (int64_t)blockIdx.x * kMdBlock + threadIdx.x; i < n; i += stride) {
    const int32_t r = val[i];
    out[i] = (r >= 0 && r < n) ? by_record[r] : kMdSentinel;
  }
}

// lo_by_record: null for the fragment list; the pair list's second key word, by record.
__global__ __launch_bounds__(kMdBlock) void md_resolve_heads_kernel(const uint64_t* __restrict__ key,
                                                                    const int32_t* __restrict__ val,
                                                                    const uint64_t* __restrict__ lo_by_record, int64_t n,
                                                                    uint32_t* __restrict__ head) {
  const int64_t stride = (int64_t)gridDim.x * kMdBlock;
  for (int64_t i = (int64_t)blockIdx.x * kMdBlock + threadIdx.x; i < n; i += stride) {
    bool h = i == 0 || key[i] != key[i - 1];
    if (!h && lo_by_record) {
      const int32_t a = val[i], c = val[i - 1];
      h = a < 0 || a >= n || c < 0 || c >= n || lo_by_record[a] != lo_by_record[c];
    }
    head[i] = h ? 1u : 0u;
  }
}

__global__ __launch_bounds__(kMdBlock) void md_resolve_best_kernel(const uint64_t* __restrict__ key,
                                                                   const int32_t* __restrict__ val,
                                                                   const uint32_t* __restrict__ seg,
                                                                   const uint64_t* __restrict__ winner, int64_t n,
                                                                   unsigned long long* __restrict__ best) {
  const int64_t stride = (int64_t)gridDim.x * kMdBlock;
  for (int64_t i = (int64_t)blockIdx.x * kMdBlock + threadIdx.x; i < n; i += stride) {
    const int32_t r = val[i];
    const uint32_t sg = seg[i];
    if (key[i] == kMdSentinel || r < 0 || r >= n || sg < 1 || sg > n) continue;
    atomicMax(best + (sg - 1), (unsigned long long)winner[r]);
  }
}

// mate: null for the fragment list (a fragment is marked alone); else a pair's two records are.
__global__ __launch_bounds__(kMdBlock) void md_resolve_mark_kernel(const uint64_t* __restrict__ key,
                                                                   const int32_t* __restrict__ val,
                                                                   const uint32_t* __restrict__ seg,
                                                                   const uint64_t* __restrict__ winner,
                                                                   const unsigned long long* __restrict__ best,
                                                                   const int32_t* __restrict__ mate, int64_t n,
                                                                   uint8_t* __restrict__ dup,
                                                                   unsigned long long* __restrict__ stats) {
  const int64_t stride = (int64_t)gridDim.x * kMdBlock;
  const int64_t rounds = (n + stride - 1) / stride;
  int64_t i = (int64_t)blockIdx.x * kMdBlock + threadIdx.x;
  for (int64_t k = 0; k < rounds; ++k, i += stride) {
    bool marked = false;
    if (i < n) {
      const int32_t r = val[i];
      const uint32_t sg = seg[i];
      if (key[i] != kMdSentinel && r >= 0 && r < n && sg >= 1 && sg <= n) {
        const uint64_t w = winner[r], bst = best[sg - 1];
        if (mate) {
          const int32_t m = mate[r];
          if (w != bst && m >= 0 && m < n) dup[r] = 1, dup[m] = 1, marked = true;
        } else if (!(w & kMdPairedBit) && ((bst & kMdPairedBit) || w != bst)) {
          dup[r] = 1, marked = true;
        }
      }
    }
    const unsigned long long m = __ballot(marked);
    if (m && (int)__lane_id() == __ffsll((long long)m) - 1)
      atomicAdd(stats + 3, (unsigned long long)__popcll(m) * (mate ? 2u : 1u));
  }
}

int grid_for(int64_t items) { return (int)std::min<int64_t>((items + kMdBlock - 1) / kMdBlock, kMdMaxBlocks); }

#define MD_ROCPRIM(expr)                                                                                     \
  do {                                                                                                       \
    hipError_t _e = (expr);                                                                                  \
    if (_e != hipSuccess)                                                                                    \
      return fail(FCS_ERR_DEVICE, std::string("[E::fcsdup_mark] ") + #expr + ": " + hipGetErrorString(_e)); \
  } while (0)

int sort_u64(const MdWs& W, char* ws, const uint64_t* kin, uint64_t* kout, const int32_t* vin, int32_t* vout, int64_t n,
             int bits, hipStream_t s) {
  size_t need = 0;
  MD_ROCPRIM(rocprim::radix_sort_pairs(nullptr, need, kin, kout, vin, vout, (size_t)n, 0u, (unsigned)bits, s));
  if (need > W.tmp_bytes)
    return fail(FCS_ERR_DEVICE, "[E::fcsdup_mark] the sort asks for " + std::to_string(need) + " bytes of scratch, " +
                                    std::to_string(W.tmp_bytes) + " are reserved");
  MD_ROCPRIM(rocprim::radix_sort_pairs(ws + W.tmp, need, kin, kout, vin, vout, (size_t)n, 0u, (unsigned)bits, s));
  return FCS_OK;
}

// Heads, segment ids, best and marks of one sorted list.
int resolve(const MdWs& W, char* ws, const uint64_t* key, const int32_t* val, const uint64_t* lo_by_record,
            const uint64_t* winner, const int32_t* mate, int64_t n, uint8_t* dup, unsigned long long* stats,
            hipStream_t s) {
  uint32_t* head = reinterpret_cast<uint32_t*>(ws + W.head);
  uint32_t* seg = reinterpret_cast<uint32_t*>(ws + W.seg);
  unsigned long long* best = reinterpret_cast<unsigned long long*>(ws + W.best);
  const int grid = grid_for(n);
  hipLaunchKernelGGL(md_resolve_heads_kernel, dim3(grid), dim3(kMdBlock), 0, s, key, val, lo_by_record, n, head);
  FCS_HIP_CHECK(hipGetLastError());
  size_t need = 0;
  MD_ROCPRIM(rocprim::inclusive_scan(nullptr, need, head, seg, (size_t)n, rocprim::plus<uint32_t>(), s));
  if (need > W.tmp_bytes) return fail(FCS_ERR_DEVICE, "[E::fcsdup_mark] the scan's scratch exceeds the reserved bytes");
  MD_ROCPRIM(rocprim::inclusive_scan(ws + W.tmp, need, head, seg, (size_t)n, rocprim::plus<uint32_t>(), s));
  FCS_HIP_CHECK(hipMemsetAsync(best, 0, 8 * (size_t)n, s));
  hipLaunchKernelGGL(md_resolve_best_kernel, dim3(grid), dim3(kMdBlock), 0, s, key, val, seg, winner, n, best);
  FCS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(md_resolve_mark_kernel, dim3(grid), dim3(kMdBlock), 0, s, key, val, seg, winner, best, mate, n, dup,
                     stats);
  FCS_HIP_CHECK(hipGetLastError());
  return FCS_OK;
}

// Everything of one call on stream s.  stats: 4 words, status: 1 word, both zeroed here.
int launch_markdup(const MdDevBatch& b, int32_t n_ref, int32_t n_lib, char* ws, uint8_t* dup, unsigned long long* stats,
                   int32_t* status, hipStream_t s) {
  FCS_HIP_CHECK(hipMemsetAsync(stats, 0, 4 * sizeof(unsigned long long), s));
  FCS_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), s));
  const int64_t n = b.n;
  if (n <= 0) return FCS_OK;
  FCS_HIP_CHECK(hipMemsetAsync(dup, 0, (size_t)n, s));
  const MdWs W = md_ws(n);
  auto at64 = [&](size_t off) { return reinterpret_cast<uint64_t*>(ws + off); };
  auto at32 = [&](size_t off) { return reinterpret_cast<int32_t*>(ws + off); };
  uint64_t* endk = at64(W.endk);
  uint32_t* score = reinterpret_cast<uint32_t*>(ws + W.score);
  uint8_t* ex = reinterpret_cast<uint8_t*>(ws + W.ex);
  constexpr int kRows = kMdBlock / kMdRow;
  hipLaunchKernelGGL(md_ends_kernel, dim3((int)std::min<int64_t>((n + kRows - 1) / kRows, 256 * 32)), dim3(kMdBlock), 0,
                     s, b, n_ref, n_lib, endk, score, ex, status);
  FCS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(md_keys_kernel, dim3(grid_for(n)), dim3(kMdBlock), 0, s, b, endk, score, ex, at64(W.fkey),
                     at32(W.fval), at64(W.wfrag), at64(W.phi), at64(W.plo), at32(W.pval), at64(W.wpair), stats);
  FCS_HIP_CHECK(hipGetLastError());
  int rc;
  // fragments: one sort by E
  if ((rc = sort_u64(W, ws, at64(W.fkey), at64(W.k64a), at32(W.fval), at32(W.v32a), n, 64, s)) ||
      (rc = resolve(W, ws, at64(W.k64a), at32(W.v32a), nullptr, at64(W.wfrag), nullptr, n, dup, stats, s)))
    return rc;
  // pairs: by K's low word, then (stable) by its high word
  if ((rc = sort_u64(W, ws, at64(W.plo), at64(W.k64a), at32(W.pval), at32(W.v32a), n, kMdEndBits, s))) return rc;
  hipLaunchKernelGGL(md_gather_kernel, dim3(grid_for(n)), dim3(kMdBlock), 0, s, at64(W.phi), at32(W.v32a), n,
                     at64(W.k64b));
  FCS_HIP_CHECK(hipGetLastError());
  if ((rc = sort_u64(W, ws, at64(W.k64b), at64(W.k64a), at32(W.v32a), at32(W.v32b), n, 64, s)) ||
      (rc = resolve(W, ws, at64(W.k64a), at32(W.v32b), at64(W.plo), at64(W.wpair), b.mate, n, dup, stats, s)))
    return rc;
  return FCS_OK;
}

// The scalar fields of a batch, checked alike by both entry points.
int check_scalars(const fcsdup_batch* b, const char* who) {
  if (!b) return fail_invalid(who, "null batch");
  if (b->n < 0) return fail_invalid(who, "negative record count " + std::to_string(b->n));
  if (b->n > kMdMaxRecords)
    return fail_invalid(who, std::to_string(b->n) + " records: more than the " + std::to_string(kMdMaxRecords) + " a batch holds");
  if (b->n_cigar < 0 || b->n_qual < 0) return fail_invalid(who, "negative CIGAR or quality size");
  if (b->n_ref < 0 || b->n_ref > kMdMaxRefs)
    return fail_invalid(who, std::to_string(b->n_ref) + " reference sequences do not fit the key's " +
                                 std::to_string(kMdRefBits) + " bits (at most " + std::to_string(kMdMaxRefs) + ")");
  if (b->n_lib < 0 || b->n_lib > kMdMaxLibs)
    return fail_invalid(who, std::to_string(b->n_lib) + " libraries do not fit the key's " + std::to_string(kMdLibBits) +
                                 " bits (at most " + std::to_string(kMdMaxLibs) + ")");
  if (b->n > 0 && (!b->flag || !b->ref_id || !b->pos || !b->mate || !b->lib || !b->cigar_off || !b->qual_off))
    return fail_invalid(who, "null array");
  if ((b->n_cigar > 0 && !b->cigar) || (b->n_qual > 0 && !b->qual)) return fail_invalid(who, "null CIGAR or quality bytes");
  return FCS_OK;
}

MdDevBatch dev_batch(const fcsdup_batch* b) {
  return MdDevBatch{b->n,     b->flag,      b->ref_id,  b->pos,  b->mate,     b->lib,
                    b->cigar, b->cigar_off, b->n_cigar, b->qual, b->qual_off, b->n_qual};
}

}  // namespace

}  // namespace fcs

using namespace fcs;

extern "C" {

int64_t fcsdup_workspace_bytes(int64_t n) {
  if (n < 0 || n > kMdMaxRecords) return fail_invalid("fcsdup_workspace_bytes", "bad record count " + std::to_string(n));
  return (int64_t)md_ws(n).total;
}

int fcsdup_mark_dev(int32_t device, const fcsdup_batch* batch, void* dev_workspace, int64_t workspace_bytes,
                    uint8_t* dev_dup, fcsdup_stats* dev_stats, int32_t* dev_status, void* stream) {
  static_assert(sizeof(fcsdup_stats) == 4 * sizeof(unsigned long long), "fcsdup_stats is four 64-bit counters");
  int rc = check_scalars(batch, "fcsdup_mark_dev");
  if (rc) return rc;
  if (!dev_stats || !dev_status || (batch->n > 0 && (!dev_dup || !dev_workspace)))
    return fail_invalid("fcsdup_mark_dev", "null output or workspace");
  const int64_t need = (int64_t)md_ws(batch->n).total;
  if (batch->n > 0 && workspace_bytes < need)
    return fail_invalid("fcsdup_mark_dev", "the workspace holds " + std::to_string(workspace_bytes) + " bytes, the call needs " +
                                               std::to_string(need));
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  return launch_markdup(dev_batch(batch), batch->n_ref, batch->n_lib, static_cast<char*>(dev_workspace), dev_dup,
                        reinterpret_cast<unsigned long long*>(dev_stats), dev_status, static_cast<hipStream_t>(stream));
}

int fcsdup_mark(int32_t device, const fcsdup_batch* b, uint8_t* dup, fcsdup_stats* stats) {
  const char* who = "fcsdup_mark";
  int rc = check_scalars(b, who);
  if (rc) return rc;
  if (!stats || (b->n > 0 && !dup)) return fail_invalid(who, "null output");
  const int64_t n = b->n;
  // every offset and index, before any device work
  if ((rc = check_offsets(who, "CIGAR", b->cigar_off, n, b->n_cigar)) ||
      (rc = check_offsets(who, "quality", b->qual_off, n, b->n_qual, kMdMaxQual)))
    return rc;
  for (int64_t r = 0; r < n; ++r) {
    const int32_t m = b->mate[r];
    if (m < -1 || m >= n || m == r || (m >= 0 && b->mate[m] != r))
      return fail_invalid(who, "mate " + std::to_string(m) + " of record " + std::to_string(r) +
                                   " is out of range or not its mate in turn");
    if (b->ref_id[r] < -1 || b->ref_id[r] >= b->n_ref)
      return fail_invalid(who, "ref_id " + std::to_string(b->ref_id[r]) + " of record " + std::to_string(r) + " is outside [-1, " +
                                   std::to_string(b->n_ref) + ")");
    if (b->lib[r] < 0 || b->lib[r] >= b->n_lib)
      return fail_invalid(who, "library " + std::to_string(b->lib[r]) + " of record " + std::to_string(r) + " is outside [0, " +
                                   std::to_string(b->n_lib) + ")");
  }
  if (n == 0) {
    std::memset(stats, 0, sizeof *stats);
    return FCS_OK;
  }
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  const size_t N = (size_t)n, c_lo = (size_t)b->cigar_off[0], nc = (size_t)b->cigar_off[n] - c_lo;
  const size_t q_lo = (size_t)b->qual_off[0], nq = (size_t)b->qual_off[n] - q_lo;
  Arena A;
  // one H2D copy of the inputs, one D2H copy of dup | stats | status
  const size_t oflag = A.add(2 * N), oref = A.add(4 * N), opos = A.add(4 * N), omate = A.add(4 * N), olib = A.add(4 * N);
  const size_t ocoff = A.add(8 * (N + 1)), oqoff = A.add(8 * (N + 1)), ocig = A.add(4 * nc), oqual = A.add(nq);
  const size_t in_bytes = A.total;
  const size_t odup = A.add(N), ostats = A.add(sizeof(fcsdup_stats)), ostatus = A.add(sizeof(int32_t));
  const size_t host_bytes = A.total;
  const size_t ows = A.add(md_ws(n).total);
  CallSession S;
  if ((rc = call_session_acquire(device, host_bytes, A.total, S))) return rc;
  CallLease lease{S};
  std::memcpy(S.host + oflag, b->flag, 2 * N);
  std::memcpy(S.host + oref, b->ref_id, 4 * N);
  std::memcpy(S.host + opos, b->pos, 4 * N);
  std::memcpy(S.host + omate, b->mate, 4 * N);
  std::memcpy(S.host + olib, b->lib, 4 * N);
  std::memcpy(S.host + ocoff, b->cigar_off, 8 * (N + 1));
  std::memcpy(S.host + oqoff, b->qual_off, 8 * (N + 1));
  if (nc) std::memcpy(S.host + ocig, b->cigar + c_lo, 4 * nc);
  if (nq) std::memcpy(S.host + oqual, b->qual + q_lo, nq);
  FCS_HIP_CHECK(hipMemcpyAsync(S.dev, S.host, in_bytes, hipMemcpyHostToDevice, S.s));
  // the device view keeps the caller's offsets: its CIGAR and quality bases are shifted down by the first ones
  MdDevBatch d;
  d.n = n;
  d.flag = reinterpret_cast<const uint16_t*>(S.dev + oflag);
  d.ref_id = reinterpret_cast<const int32_t*>(S.dev + oref);
  d.pos = reinterpret_cast<const int32_t*>(S.dev + opos);
  d.mate = reinterpret_cast<const int32_t*>(S.dev + omate);
  d.lib = reinterpret_cast<const int32_t*>(S.dev + olib);
  d.cigar = reinterpret_cast<const uint32_t*>(S.dev + ocig) - c_lo;
  d.cigar_off = reinterpret_cast<const int64_t*>(S.dev + ocoff);
  d.n_cigar = b->cigar_off[n];
  d.qual = reinterpret_cast<const uint8_t*>(S.dev + oqual) - q_lo;
  d.qual_off = reinterpret_cast<const int64_t*>(S.dev + oqoff);
  d.n_qual = b->qual_off[n];
  if ((rc = launch_markdup(d, b->n_ref, b->n_lib, S.dev + ows, reinterpret_cast<uint8_t*>(S.dev + odup),
                           reinterpret_cast<unsigned long long*>(S.dev + ostats),
                           reinterpret_cast<int32_t*>(S.dev + ostatus), S.s)))
    return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S.host + odup, S.dev + odup, host_bytes - odup, hipMemcpyDeviceToHost, S.s));
  FCS_HIP_CHECK(hipStreamSynchronize(S.s));
  int32_t status;
  std::memcpy(&status, S.host + ostatus, sizeof status);
  if (status & FCSDUP_STATUS_POS)
    return fail_invalid(who, "an unclipped 5' position does not fit the key's " + std::to_string(kMdPosBits) +
                                 " bits (|u5| < " + std::to_string(kMdPosBias) + ")");
  if (status) return fail(FCS_ERR_DEVICE, "[E::fcsdup_mark] the device clamped a checked field (status " + std::to_string(status) + ")");
  std::memcpy(dup, S.host + odup, N);
  std::memcpy(stats, S.host + ostats, sizeof *stats);
  return FCS_OK;
}

}  // extern "C"
