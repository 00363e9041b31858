// The middle of the fused seeding call (fcs_fmd_seed): from the
// slots fmd_collect_kernel (fmd_seed.hip) fills to a compacted list of sorted
// SMEMs and located positions, all on one stream and without a host round
// trip.  The per-read logic is csrc/fmd_expand.h (one text for these kernels
// and the host check tools/micro/fmd_expand_test.cpp).
//
// fmd_seed_order_kernel: one read per 16-lane DPP row, four reads per wave, one
// wave per block (so a block barrier is the wave's own and every loop that
// holds one runs to the wave's largest SMEM count).  Lane c of a row takes the
// read's SMEMs c, c + 16, ..; for each it counts the SMEMs that sort before it
// under (qb, qe, slot) and sums their row counts min(s, max_occ), reading the
// read's packed keys and counts from LDS, where the row stages them in tiles
// of 64 (one tile, loaded once, for the usual read of at most 14 SMEMs; the
// 2,700 SMEMs of a low-complexity read take 43 tiles per 16 SMEMs).  Writes
// each SMEM's place {rank, first row}, and per read the SMEM count (0 for a
// read collect handed back) and the row count.  3 KB of LDS per wave.
// fmd_seed_order_kernel is built for 8 waves per SIMD.
//
// fmd_seed_scan_kernel: one block of 1024 lanes; lane t sums a contiguous run
// of reads, the 1024 sums are scanned in LDS, and the lane writes its run's
// exclusive prefix sums: mem_off[0 .. n] and row_off[0 .. n], the totals last.
// fmd_seed_scan_kernel is built for 4 waves per SIMD (its one block is 16 waves).
//
// fmd_seed_expand_kernel: one read per DPP row again, no LDS; lane c copies
// SMEM c, c + 16, .. to mems[mem_off[r] + rank] and writes its sampled rows k +
// j step from row_off[r] + its first row on.  When a total exceeds its
// capacity the kernel writes nothing, and every single store is bounded by the
// capacity besides.  For an index without a device suffix array the rows go
// straight to the positions, encoded -1 - row.
// fmd_seed_expand_kernel is built for 8 waves per SIMD.
//
// fmd_seed_locate_kernel: fmd_locate_kernel's walk (fmd_smem.h fmd_sa_walk)
// over a row count it reads from device memory; a row that is not located
// (step cap, bad row) comes back as -1 - row.
// fmd_seed_locate_kernel is built for 8 waves per SIMD.
#include <algorithm>

#include "fcship_internal.h"
#include "fmd_expand.h"

namespace fcs {

namespace {

constexpr int kSeedRow = 16;         // lanes per read
constexpr int kSeedOrderBlock = 64;  // one wave
constexpr int kSeedTile = 64;        // SMEMs of a read staged in LDS at a time
constexpr int kSeedBlock = 256;
constexpr int kSeedScanBlock = 1024;
constexpr int kSeedOrderMaxBlocks = 256 * 64;  // fmd_seed_order_kernel: a wave of four reads per block
constexpr int kSeedExpandMaxBlocks = 256 * 8;  // fmd_seed_expand_kernel: 16 reads per block
constexpr int kSeedLocateMaxBlocks = 256 * 8;  // fmd_seed_locate_kernel: a lane per located row

// One lane reads the whole occ line (fmd_seed.hip's policy for its locate kernel).
struct FmdLaneWords {
  const uint64_t* occ;
  __device__ __forceinline__ void counts(int64_t blk, uint64_t mask, int64_t o[4]) const {
    const uint64_t* B = occ + 8 * blk;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = (int64_t)(B[c] + (uint64_t)__builtin_popcountll(B[4 + c] & mask));
  }
  __device__ __forceinline__ uint64_t word(int64_t w) const { return occ[w]; }
};

__global__ __launch_bounds__(kSeedOrderBlock) void fmd_seed_order_kernel(
    const FmdIv* __restrict__ slots, int32_t max_mems, const int32_t* __restrict__ n_mems,
    const int32_t* __restrict__ overflow, int32_t n_reads, int32_t max_occ, FmdSeedPlace* __restrict__ place,
    int32_t* __restrict__ n_eff, int64_t* __restrict__ n_rows) {
  __shared__ uint64_t tkey[kSeedOrderBlock / kSeedRow][kSeedTile];
  __shared__ int32_t tcnt[kSeedOrderBlock / kSeedRow][kSeedTile];
  constexpr int kRows = kSeedOrderBlock / kSeedRow;
  const int g = (int)threadIdx.x / kSeedRow, l = (int)threadIdx.x % kSeedRow;
  const int64_t stride = (int64_t)gridDim.x * kRows;
  for (int64_t r0 = (int64_t)blockIdx.x * kRows; r0 < n_reads; r0 += stride) {  // the same rounds for the whole wave
    const int64_t r = r0 + g;
    int32_t k = 0;  // read once and clamped: every loop below is bounded by it
    if (r < n_reads && !overflow[r]) k = min(max(n_mems[r], 0), max_mems);
    int32_t kmax = max(k, __shfl_xor(k, 16));
    kmax = max(kmax, __shfl_xor(kmax, 32));
    const FmdIv* rs = slots + (size_t)r * (size_t)max_mems;
    FmdSeedPlace* rp = place + (size_t)r * (size_t)max_mems;
    const bool one_tile = kmax <= kSeedTile;
    auto stage = [&](int32_t t0) {
      for (int t = l; t < kSeedTile; t += kSeedRow) {
        const int32_t j = t0 + t;
        if (j < k) {
          tkey[g][t] = fmd_seed_key(rs[j].qb, rs[j].qe);
          tcnt[g][t] = fmd_seed_count(rs[j].s, max_occ);
        }
      }
    };
    if (one_tile) {
      stage(0);
      __syncthreads();
    }
    int64_t rows = 0;
    for (int32_t i0 = 0; i0 < kmax; i0 += kSeedRow) {
      const int32_t i = i0 + l;
      const bool mine = i < k;
      uint64_t key = 0;
      int32_t cnt = 0;
      if (mine) {
        key = fmd_seed_key(rs[i].qb, rs[i].qe);
        cnt = fmd_seed_count(rs[i].s, max_occ);
      }
      int32_t rank = 0;
      int64_t row0 = 0;
      for (int32_t t0 = 0; t0 < kmax; t0 += kSeedTile) {
        if (!one_tile) {
          __syncthreads();  // the tile before is read
          stage(t0);
          __syncthreads();
        }
        const int32_t nt = min(kSeedTile, k - t0);
        if (mine) fmd_seed_rank_span(key, i, t0, nt, tkey[g], tcnt[g], rank, row0);
      }
      if (mine) {
        rp[i].rank = rank;
        rp[i].pad = 0;
        rp[i].row0 = row0;
        rows += cnt;
      }
    }
    rows += __shfl_xor(rows, 8);
    rows += __shfl_xor(rows, 4);
    rows += __shfl_xor(rows, 2);
    rows += __shfl_xor(rows, 1);
    if (l == 0 && r < n_reads) {
      n_eff[r] = k;
      n_rows[r] = rows;
    }
    __syncthreads();  // before the next round's reads overwrite the tile
  }
}

__global__ __launch_bounds__(kSeedScanBlock) void fmd_seed_scan_kernel(const int32_t* __restrict__ n_eff,
                                                                       const int64_t* __restrict__ n_rows, int32_t n,
                                                                       int64_t* __restrict__ mem_off,
                                                                       int64_t* __restrict__ row_off) {
  __shared__ int64_t pm[kSeedScanBlock], pr[kSeedScanBlock];
  const int t = (int)threadIdx.x;
  const int64_t per = ((int64_t)n + kSeedScanBlock - 1) / kSeedScanBlock;
  const int64_t b0 = min((int64_t)n, t * per), b1 = min((int64_t)n, b0 + per);
  int64_t sm = 0, sr = 0;
  for (int64_t k = b0; k < b1; ++k) sm += max(n_eff[k], 0), sr += max(n_rows[k], (int64_t)0);
  pm[t] = sm, pr[t] = sr;
  __syncthreads();
  for (int d = 1; d < kSeedScanBlock; d <<= 1) {
    const int64_t am = t >= d ? pm[t - d] : 0, ar = t >= d ? pr[t - d] : 0;
    __syncthreads();
    pm[t] += am, pr[t] += ar;
    __syncthreads();
  }
  int64_t rm = pm[t] - sm, rr = pr[t] - sr;
  if (t == kSeedScanBlock - 1) mem_off[n] = pm[t], row_off[n] = pr[t];
  for (int64_t k = b0; k < b1; ++k) {
    mem_off[k] = rm, row_off[k] = rr;
    rm += max(n_eff[k], 0), rr += max(n_rows[k], (int64_t)0);
  }
}

__global__ __launch_bounds__(kSeedBlock) void fmd_seed_expand_kernel(
    const FmdIv* __restrict__ slots, int32_t max_mems, const int32_t* __restrict__ n_eff,
    const FmdSeedPlace* __restrict__ place, int32_t n_reads, int32_t max_occ, const int64_t* __restrict__ mem_off,
    const int64_t* __restrict__ row_off, FmdIv* __restrict__ mems, int64_t mem_cap, int64_t* __restrict__ rows,
    int64_t row_cap, int encode) {
  if (mem_off[n_reads] > mem_cap || row_off[n_reads] > row_cap) return;  // the caller learns the totals and calls again
  const int tid = (int)(blockIdx.x * kSeedBlock + threadIdx.x);
  const int l = tid % kSeedRow;
  const int64_t stride = (int64_t)gridDim.x * (kSeedBlock / kSeedRow);
  for (int64_t r = tid / kSeedRow; r < n_reads; r += stride) {
    const int32_t k = min(max(n_eff[r], 0), max_mems);
    const int64_t m0 = mem_off[r], w0 = row_off[r];
    const FmdIv* rs = slots + (size_t)r * (size_t)max_mems;
    const FmdSeedPlace* rp = place + (size_t)r * (size_t)max_mems;
    for (int32_t i = l; i < k; i += kSeedRow) {
      const int64_t mk = rs[i].k, ml = rs[i].l, ms = rs[i].s;
      const int32_t qb = rs[i].qb, qe = rs[i].qe;
      const int32_t rank = rp[i].rank;
      const int64_t at = m0 + rank;
      if (rank >= 0 && rank < k && m0 >= 0 && at < mem_cap) {
        FmdIv& o = mems[at];
        o.k = mk, o.l = ml, o.s = ms, o.qb = qb, o.qe = qe;
      }
      const int64_t row0 = rp[i].row0;
      if (w0 >= 0 && row0 >= 0)
        fmd_seed_rows(mk, ms, max_occ, fmd_seed_count(ms, max_occ), encode != 0, rows, w0 + row0, row_cap);
    }
  }
}

__global__ __launch_bounds__(kSeedBlock) void fmd_seed_locate_kernel(FmdDevIndex dx, const int64_t* __restrict__ rows,
                                                                     const int64_t* __restrict__ mem_total,
                                                                     int64_t mem_cap,
                                                                     const int64_t* __restrict__ row_total,
                                                                     int64_t row_cap, int32_t max_steps,
                                                                     int64_t* __restrict__ pos) {
  const int64_t n = *mem_total > mem_cap || *row_total > row_cap ? 0 : min(max(*row_total, (int64_t)0), row_cap);
  FmdIx<FmdLaneWords> ix;
  ix.f.occ = dx.occ;
  ix.n = dx.n_rows;
  ix.C = dx.C;
  const int64_t stride = (int64_t)gridDim.x * kSeedBlock;
  for (int64_t i = (int64_t)blockIdx.x * kSeedBlock + threadIdx.x; i < n; i += stride) {
    const int64_t row = rows[i];
    int64_t p;
    int32_t steps;
    const int rc = fmd_sa_walk(ix, dx.sa, dx.n_sa, dx.sa_intv, dx.special, dx.n_special, row, max_steps, p, steps);
    pos[i] = rc == kFmdLocated ? p : -1 - row;
  }
}

}  // namespace

int launch_fmd_seed(const FmdDevIndex& dx, const FmdIv* slots, int32_t max_mems, const int32_t* n_mems,
                    const int32_t* overflow, int32_t n_reads, int32_t max_occ, int32_t max_steps, FmdSeedPlace* place,
                    int32_t* n_eff, int64_t* n_rows, int64_t* mem_off, int64_t* row_off, FmdIv* mems, int64_t mem_cap,
                    int64_t* rows, int64_t* pos, int64_t row_cap, hipStream_t s) {
  if (n_reads > 0) {
    const int blocks = (int)std::min<int64_t>(((int64_t)n_reads + 3) / 4, kSeedOrderMaxBlocks);
    hipLaunchKernelGGL(fmd_seed_order_kernel, dim3(blocks), dim3(kSeedOrderBlock), 0, s, slots, max_mems, n_mems,
                       overflow, n_reads, max_occ, place, n_eff, n_rows);
    FCS_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(fmd_seed_scan_kernel, dim3(1), dim3(kSeedScanBlock), 0, s, n_eff, n_rows, n_reads, mem_off,
                     row_off);
  FCS_HIP_CHECK(hipGetLastError());
  if (n_reads <= 0) return FCS_OK;
  const bool walk = dx.sa != nullptr;  // without a device suffix array the encoded rows are the answer
  constexpr int per_block = kSeedBlock / kSeedRow;
  const int blocks = (int)std::min<int64_t>(((int64_t)n_reads + per_block - 1) / per_block, kSeedExpandMaxBlocks);
  hipLaunchKernelGGL(fmd_seed_expand_kernel, dim3(blocks), dim3(kSeedBlock), 0, s, slots, max_mems, n_eff, place,
                     n_reads, max_occ, mem_off, row_off, mems, mem_cap, walk ? rows : pos, row_cap, walk ? 0 : 1);
  FCS_HIP_CHECK(hipGetLastError());
  if (walk && row_cap > 0) {
    const int lblocks = (int)std::min<int64_t>((row_cap + kSeedBlock - 1) / kSeedBlock, kSeedLocateMaxBlocks);
    hipLaunchKernelGGL(fmd_seed_locate_kernel, dim3(lblocks), dim3(kSeedBlock), 0, s, dx, rows, mem_off + n_reads,
                       mem_cap, row_off + n_reads, row_cap, max_steps, pos);
    FCS_HIP_CHECK(hipGetLastError());
  }
  return FCS_OK;
}

}  // namespace fcs
