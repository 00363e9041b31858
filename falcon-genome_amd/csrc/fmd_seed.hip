// FMD-index seeding on gfx950: the SMEM
// collection and the suffix-array lookups of the aligner's seed_read, whose
// per-read logic is csrc/fmd_smem.h (one text for these kernels and the host
// check tools/micro/fmd_smem_test.cpp; the oracle is host/fmindex.cpp).
//
// fmd_collect_kernel: one read per quad, four reads per DPP row, 16 per wave.
// An occ query is one 64-byte line (four counts, four bit vectors); lane c of
// the quad loads B[c] and B[4 + c], adds the popcount under the mask, and the
// four lanes exchange their counts with quad_perm DPP, so a quad's two 8-byte
// loads cover exactly the line and every extension has all four sizes (the
// forward extension needs them for the cumulative l).  Everything else (the
// query bytes, the interval, the loop state) is replicated across the quad and
// a function of the counts alone, so a quad never diverges; quads of a wave
// do, each at its own read.  The prev / curr interval stacks live in a global
// arena of 2 x (longest read + 1) intervals per quad (a stack is as deep as
// the read is long on low-complexity reads: 100 entries for a 150-base poly-A
// read over a 100-base homopolymer), each lane of the quad writing the same
// value and reading back what it wrote itself.  The SMEMs go to max_mems
// fixed slots per read; a read with more sets its overflow flag and is redone
// on the host.  The grid is bounded (kFmdMaxUnits quads) and strides over the
// reads, which the host orders longest first.  No LDS, no scratch.
// fmd_collect_kernel is built for 2 waves per SIMD (8 per CU): the arena, not
// the registers, bounds the quads in flight (32768 quads x 9.7 KB at 151-base
// reads).
//
// fmd_locate_kernel: one lane per BWT row; LF steps (one occ line each: the
// four bit-vector words, then the count of the row's symbol) until the row is
// sampled or special (binary search in the device copy of the sorted table),
// at most max_steps of them; a row that hits the cap is flagged and located
// on the host.  fmd_locate_kernel is built for 8 waves per SIMD (32 per CU).
#include <algorithm>

#include "fcship_internal.h"
#include "fmd_smem.h"

namespace fcs {

namespace {

constexpr int kFmdBlock = 256;
constexpr int kFmdMaxUnits = 32768;  // quads in flight: 256 CUs x 8 waves x 16
constexpr int kFmdLocateMaxBlocks = 256 * 8;  // fmd_locate_kernel: a lane per row

template <int C>
__device__ __forceinline__ int64_t quad_bcast(int64_t v) {
  constexpr int ctrl = C | (C << 2) | (C << 4) | (C << 6);  // quad_perm:[C, C, C, C]
  const int lo = __builtin_amdgcn_update_dpp(0, (int)v, ctrl, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(v >> 32), ctrl, 0xF, 0xF, false);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// Lane c of a quad reads words c and 4 + c of the line.
struct FmdQuadFetch {
  const uint64_t* occ;
  int c;
  __device__ __forceinline__ void counts(int64_t blk, uint64_t mask, int64_t o[4]) const {
    const uint64_t* B = occ + 8 * blk;
    const int64_t v = (int64_t)(B[c] + (uint64_t)__builtin_popcountll(B[4 + c] & mask));
    o[0] = quad_bcast<0>(v);
    o[1] = quad_bcast<1>(v);
    o[2] = quad_bcast<2>(v);
    o[3] = quad_bcast<3>(v);
  }
  __device__ __forceinline__ uint64_t word(int64_t w) const { return occ[w]; }
};

struct FmdLaneFetch {
  const uint64_t* occ;
  __device__ __forceinline__ void counts(int64_t blk, uint64_t mask, int64_t o[4]) const {
    const uint64_t* B = occ + 8 * blk;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = (int64_t)(B[c] + (uint64_t)__builtin_popcountll(B[4 + c] & mask));
  }
  __device__ __forceinline__ uint64_t word(int64_t w) const { return occ[w]; }
};

__global__ __launch_bounds__(kFmdBlock) void fmd_collect_kernel(FmdDevIndex dx, const uint8_t* __restrict__ codes,
                                                                int64_t n_code_bytes,
                                                                const int64_t* __restrict__ q_off,
                                                                const int32_t* __restrict__ q_len,
                                                                const int32_t* __restrict__ order, int32_t n_reads,
                                                                FmdCollectParams P, FmdIv* arena, int32_t cap,
                                                                FmdIv* out, int32_t max_mems,
                                                                int32_t* __restrict__ n_mems,
                                                                int32_t* __restrict__ overflow) {
  const int tid = (int)(blockIdx.x * kFmdBlock + threadIdx.x);
  const int unit = tid >> 2, n_units = (int)(gridDim.x * kFmdBlock) >> 2;
  FmdIx<FmdQuadFetch> ix;
  ix.f.occ = dx.occ;
  ix.f.c = tid & 3;
  ix.n = dx.n_rows;
  ix.C = dx.C;
  FmdIv* stack = arena + (size_t)unit * 2 * (size_t)cap;
  for (int r = unit; r < n_reads; r += n_units) {
    const int rd = order ? order[r] : r;
    if (rd < 0 || rd >= n_reads) continue;
    const int64_t off = q_off[rd];
    const int len = q_len[rd];
    FmdCollectState st;
    // a read outside the code bytes, or longer than the stacks were sized for, goes to the host
    if (off < 0 || len < 0 || len >= cap || off > n_code_bytes - len) st.overflow = true;
    else fmd_collect(ix, codes + off, len, P, stack, cap, out + (size_t)rd * (size_t)max_mems, max_mems, st);
    if ((tid & 3) == 0) {
      n_mems[rd] = st.overflow ? 0 : st.n_out;
      overflow[rd] = st.overflow ? 1 : 0;
    }
  }
}

__global__ __launch_bounds__(kFmdBlock) void fmd_locate_kernel(FmdDevIndex dx, const int64_t* __restrict__ rows,
                                                               int64_t n_rows_req, int32_t max_steps,
                                                               int64_t* __restrict__ pos,
                                                               int32_t* __restrict__ status) {
  FmdIx<FmdLaneFetch> ix;
  ix.f.occ = dx.occ;
  ix.n = dx.n_rows;
  ix.C = dx.C;
  const int64_t stride = (int64_t)gridDim.x * kFmdBlock;
  for (int64_t i = (int64_t)blockIdx.x * kFmdBlock + threadIdx.x; i < n_rows_req; i += stride) {
    int64_t p;
    int32_t steps;
    const int rc = fmd_sa_walk(ix, dx.sa, dx.n_sa, dx.sa_intv, dx.special, dx.n_special, rows[i], max_steps, p, steps);
    pos[i] = p;
    status[i] = rc;
  }
}

}  // namespace

// Quads of the grid a collect launch over n_reads uses (whole blocks): the
// arena holds 2 * cap intervals for each.
int64_t fmd_collect_units(int32_t n_reads) {
  constexpr int64_t per_block = kFmdBlock / 4;
  return std::min<int64_t>(kFmdMaxUnits, (std::max<int64_t>(n_reads, 1) + per_block - 1) / per_block * per_block);
}

int launch_fmd_collect(const FmdDevIndex& dx, const uint8_t* codes, int64_t n_code_bytes, const int64_t* q_off,
                       const int32_t* q_len, const int32_t* order, int32_t n_reads, const FmdCollectParams& P,
                       FmdIv* arena, int32_t cap, FmdIv* out, int32_t max_mems, int32_t* n_mems, int32_t* overflow,
                       hipStream_t s) {
  if (n_reads <= 0) return FCS_OK;
  const int64_t units = fmd_collect_units(n_reads);
  const int blocks = (int)(units * 4 / kFmdBlock);
  hipLaunchKernelGGL(fmd_collect_kernel, dim3(blocks), dim3(kFmdBlock), 0, s, dx, codes, n_code_bytes, q_off, q_len,
                     order, n_reads, P, arena, cap, out, max_mems, n_mems, overflow);
  FCS_HIP_CHECK(hipGetLastError());
  return FCS_OK;
}

int launch_fmd_locate(const FmdDevIndex& dx, const int64_t* rows, int64_t n, int32_t max_steps, int64_t* pos,
                      int32_t* status, hipStream_t s) {
  if (n <= 0) return FCS_OK;
  const int blocks = (int)std::min<int64_t>((n + kFmdBlock - 1) / kFmdBlock, kFmdLocateMaxBlocks);
  hipLaunchKernelGGL(fmd_locate_kernel, dim3(blocks), dim3(kFmdBlock), 0, s, dx, rows, n, max_steps, pos, status);
  FCS_HIP_CHECK(hipGetLastError());
  return FCS_OK;
}

}  // namespace fcs
