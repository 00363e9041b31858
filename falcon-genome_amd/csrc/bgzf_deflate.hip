// BGZF member compression on gfx950 (the writing side:
// `fcs-genome` bgzips its VCF and writes BAM; bgzf_kernels.hip is the reader).
//
// One 64-lane wave per member (<= 0xff00 input bytes), the member's state in
// LDS: the matcher's table of last positions (2^13 words, 32 KiB), the
// histograms, code tables and header scratch of bgzf_deflate.h (4.9 KiB) and a
// 640-byte staging buffer for output bits: 38.2 KiB, so 4 members per CU (one
// wave per SIMD; the 160 KiB of LDS is the limit, not the ~50 VGPRs).  The
// input stays in global memory (read-only, served by the vector L1 / L2).
//
// LZ77, 64 positions (one per lane) at a time:
// - a lane hashes the 4 bytes at its position and has two candidates: the
//   nearest earlier lane of this chunk with the same hash (64 readlane
//   compares), and the table's entry, which holds the last position with that
//   hash among the chunks before this one.  It extends both (8 bytes per step,
//   up to 258) and keeps the longer, the nearer on a tie.  Positions inside a
//   match already taken do not search.
// - then every lane enters its position into the table with an LDS atomic max:
//   reads and writes of a chunk are separated by a wave barrier and the max
//   does not depend on the order of the lanes, so the table, and with it every
//   match, is a function of the input bytes alone.
// - the greedy parse is wave-uniform scalar work on the ballot of lanes that
//   hold a match: literals up to the next match, the match, skip its length.
// The parse runs twice, since a member's tokens (up to 65,280) have no place to
// wait for their code: the first pass counts symbols (LDS atomic adds), lane 0
// and the wave build the dynamic code and choose the member's form
// (bgzf_deflate.h: stored, fixed or dynamic, the smallest), the second pass
// finds the same tokens again and emits them.  A token's bits go to their place
// in the stream by a prefix sum of the lanes' bit counts and LDS atomic ORs
// into the staging words; whole words leave with one vector store per lane.
// The CRC-32 is bgzf_inflate.h's lane-chunk CRC recombined with crc_shift.
//
// A member's bytes depend on its block's bytes and nothing else: not on the
// batch, the block's place in it, or the order in which lanes or waves ran.
#include <hip/hip_runtime.h>

#include "bgzf_deflate.h"
#include "bgzf_inflate.h"
#include "fcship_internal.h"

namespace fcs {
namespace {

constexpr int kSlot = 65536;       // a member's output slot (and BGZF's member limit)
constexpr int kStageWords = 160;   // the dynamic header (<= 4,498 bits) or 64 tokens (<= 3,072) plus a carried word
constexpr uint32_t kSlotWords = (kSlot - 16) / 4;

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

struct DefLanes {
  __device__ static int id() { return (int)threadIdx.x; }
  __device__ static constexpr int n() { return 64; }
  __device__ static void sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
};

struct DeflateLds {
  uint32_t table[1 << kDefHashBits];  // position + 1 of the last entry, 0: none
  DefWork w;
  uint32_t stage[kStageWords];
};

// The member's bit stream from its byte 16 on (a word boundary of the slot):
// 16 bits of BSIZE, then the payload.  `stage` holds the bits from the last
// word boundary; word 0 is kept back until BSIZE is known.
struct BitOut {
  uint32_t* stage;
  uint32_t* out;
  uint32_t bitpos, word0;
};

// lane 0 writes the block header's bits behind the bits already staged
struct StageSink {
  uint32_t* stage;
  uint32_t at;
  __device__ void put(uint32_t v, int n) {
    if (n == 0) return;
    const uint32_t wd = at >> 5, sh = at & 31;
    stage[wd] |= v << sh;
    if (sh + (uint32_t)n > 32) stage[wd + 1] |= v >> (32 - sh);
    at += (uint32_t)n;
  }
};

// `added` bits were staged behind bitpos: the whole words leave, the rest is
// carried to the front of the cleared stage.
__device__ __forceinline__ void stage_flush(BitOut& b, uint32_t added) {
  DefLanes::sync();
  const int lane = DefLanes::id();
  const uint32_t bw = b.bitpos >> 5, full = ((b.bitpos & 31) + added) >> 5;
  for (uint32_t i = (uint32_t)lane; i < full; i += 64)
    if (bw + i != 0 && bw + i < kSlotWords) b.out[bw + i] = b.stage[i];
  if (bw == 0 && full > 0) b.word0 = rfl(b.stage[0]);
  const uint32_t carry = rfl(b.stage[full]);
  DefLanes::sync();
  for (int i = lane; i < kStageWords; i += 64) b.stage[i] = i == 0 ? carry : 0u;
  DefLanes::sync();
  b.bitpos += added;
}

// bytes c.. and p.. (c < p) alike, up to `most`
__device__ __forceinline__ int match_len(const uint8_t* __restrict__ in, uint32_t c, uint32_t p, int most) {
  int l = 0;
  while (l + 8 <= most) {
    uint64_t x = 0, y = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      x |= (uint64_t)in[c + l + k] << (8 * k);
      y |= (uint64_t)in[p + l + k] << (8 * k);
    }
    const uint64_t diff = x ^ y;
    if (diff) return l + (__builtin_ctzll(diff) >> 3);
    l += 8;
  }
  while (l < most && in[c + l] == in[p + l]) ++l;
  return l;
}

// One pass over the block's tokens: kEmit false counts their symbols into
// w.freq, true writes their bits.
template <bool kEmit>
__device__ __forceinline__ void deflate_pass(const uint8_t* __restrict__ in, const uint32_t n, DeflateLds& S, BitOut& b) {
  const int lane = DefLanes::id();
  for (int i = lane; i < (1 << kDefHashBits); i += 64) S.table[i] = 0;
  DefLanes::sync();
  uint32_t next = 0;  // where the next token starts (uniform)
  for (uint32_t base = 0; base < n; base += kDefChunk) {
    const uint32_t p = base + (uint32_t)lane;
    const bool hashable = p + kDefHashBytes <= n;
    uint32_t h = 0;
    if (hashable) {
      uint32_t v = 0;
#pragma unroll
      for (int k = 0; k < kDefHashBytes; ++k) v |= (uint32_t)in[p + k] << (8 * k);
      h = def_hash(v);
    }
    int len = 0, dist = 0;
    if (base + kDefChunk > next) {  // uniform: some position of the chunk starts a token
      // the nearest earlier lane with the same hash (lanes that cannot hash match nobody)
      const uint32_t hk = hashable ? h : 0x80000000u | (uint32_t)lane;
      int near = -1;
#pragma unroll
      for (int j = 0; j < 63; ++j) {
        const uint32_t hj = (uint32_t)__builtin_amdgcn_readlane((int)hk, j);
        if (hj == hk && j < lane) near = j;
      }
      if (hashable && p >= next) {
        const int most = (int)min((uint32_t)kDefMaxMatch, n - p);
        const uint32_t t = S.table[h];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const uint32_t c1 = k == 0 ? (near >= 0 ? base + (uint32_t)near + 1 : 0u) : t;
          if (!c1) continue;
          const uint32_t c = c1 - 1, d = p - c;
          if (d > (uint32_t)kDefWindow) continue;
          const int m = match_len(in, c, p, most);
          if (m >= kDefMinMatch && !(m == kDefMinMatch && d > (uint32_t)kDefTooFar) && m > len) len = m, dist = (int)d;
        }
      }
    }
    DefLanes::sync();  // every lane has read the table
    if (hashable) atomicMax(&S.table[h], p + 1);
    // the greedy parse: S = lanes whose position starts a token
    const uint64_t M = __ballot(len != 0);
    uint32_t cur = (next > base ? next : base) - base;
    uint64_t T = 0;
    while (cur < (uint32_t)kDefChunk) {
      const uint64_t mm = M >> cur;
      if (!mm) {
        T |= ~0ull << cur;
        cur = kDefChunk;
        break;
      }
      const uint32_t j = cur + (uint32_t)__builtin_ctzll(mm);
      T |= (~0ull << cur) & ((2ull << j) - 1);
      cur = j + rfl((uint32_t)__builtin_amdgcn_readlane(len, (int)rfl(j)));
    }
    next = base + cur;
    const bool token = ((T >> lane) & 1) && p < n;
    const int v = len ? len : (token ? (int)in[p] : 0);
    if constexpr (!kEmit) {
      if (token) {
        int ls, ds;
        def_token_syms(v, dist, ls, ds);
        atomicAdd(&S.w.freq[ls], 1u);
        if (ds >= 0) atomicAdd(&S.w.freq[kDefLl + ds], 1u);
      }
    } else {
      uint64_t bits = 0;
      int nb = 0;
      if (token) def_token_bits(S.w, v, dist, bits, nb);
      int x = nb;  // inclusive prefix sum of the lanes' bit counts
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
      }
      const uint32_t added = (uint32_t)__builtin_amdgcn_readlane(x, 63);
      if (nb) {
        const uint32_t at = (b.bitpos & 31) + (uint32_t)(x - nb), wd = at >> 5, sh = at & 31;
        const uint64_t lo = bits << sh;
        const uint32_t hi = sh ? (uint32_t)(bits >> (64 - sh)) : 0u;
        if ((uint32_t)lo) atomicOr(&b.stage[wd], (uint32_t)lo);
        if ((uint32_t)(lo >> 32)) atomicOr(&b.stage[wd + 1], (uint32_t)(lo >> 32));
        if (hi) atomicOr(&b.stage[wd + 2], hi);
      }
      stage_flush(b, added);
    }
    if constexpr (!kEmit) DefLanes::sync();
  }
}

}  // namespace

// Block k of data (block_bytes each, the last one shorter) -> one BGZF member
// at slots + k * 65536, its size in clen[k] (-1: the encoder disagreed with
// its own plan; nothing outside the slot is written either way).
__global__ __launch_bounds__(64) void bgzf_deflate_kernel(const uint8_t* __restrict__ data, int64_t n_bytes,
                                                          int32_t block_bytes, uint8_t* __restrict__ slots,
                                                          int32_t* __restrict__ clen) {
  __shared__ DeflateLds S;
  const int lane = (int)threadIdx.x;
  const int64_t at = (int64_t)blockIdx.x * block_bytes;
  if (at >= n_bytes) return;
  const uint8_t* __restrict__ in = data + at;
  const uint32_t n = (uint32_t)min((int64_t)block_bytes, n_bytes - at);
  uint8_t* const mem = slots + (int64_t)blockIdx.x * kSlot;

  for (int i = lane; i < kDefLl + kDefD; i += 64) S.w.freq[i] = 0;
  for (int i = lane; i < kStageWords; i += 64) S.stage[i] = 0;
  DefLanes::sync();
  BitOut b{S.stage, reinterpret_cast<uint32_t*>(mem + 16), 16, 0};
  deflate_pass<false>(in, n, S, b);
  if (lane == 0) S.w.freq[kDefEob] = 1;
  DefLanes::sync();
  def_plan<DefLanes>(S.w, n);
  const int form = (int)rfl((uint32_t)S.w.form);
  const uint32_t plen = rfl(def_payload_bytes(S.w, n));

  // CRC-32 of the block: contiguous lane chunks, each shifted past the bytes after it
  const int ng = (int)n, chunk = (ng + 63) / 64;
  const int cb = min(ng, lane * chunk), ce = min(ng, cb + chunk);
  uint32_t c = 0xFFFFFFFFu;
  for (int q = cb; q < ce; ++q) {
    c ^= in[q];
#pragma unroll
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
  }
  uint32_t crc = ce > cb ? crc_shift(~c, (uint64_t)(ng - ce)) : 0u;
  for (int off = 32; off > 0; off >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, off, 64);

  const uint32_t total = kDefMemberHead + plen + kDefMemberTail, bsize = total - 1;
  bool ok = true;
  if (lane < 4) reinterpret_cast<uint32_t*>(mem)[lane] = def_member_head_word(lane);
  if (form == kDefStored) {
    if (lane < 7) {
      const uint32_t hd[7] = {bsize & 255, bsize >> 8, 1, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255};
      uint32_t v = 0;
#pragma unroll
      for (int k = 0; k < 7; ++k) v = lane == k ? hd[k] : v;
      mem[16 + lane] = (uint8_t)v;
    }
    for (uint32_t i = (uint32_t)lane; i < n; i += 64) mem[kDefMemberHead + 5 + i] = in[i];
  } else {
    if (lane == 0) {
      StageSink sink{S.stage, 16};
      def_put_header(S.w, sink);
      S.w.n_rle = (int32_t)(sink.at - 16);  // the header's bits (the run list is spent)
    }
    DefLanes::sync();
    stage_flush(b, rfl((uint32_t)S.w.n_rle));
    deflate_pass<true>(in, n, S, b);
    // the end-of-block symbol
    if (lane == 0) {
      uint64_t bits;
      int nb;
      def_token_bits(S.w, kDefEob, 0, bits, nb);
      StageSink sink{S.stage, b.bitpos & 31};
      sink.put((uint32_t)bits, nb);
      S.w.n_rle = nb;
    }
    DefLanes::sync();
    stage_flush(b, rfl((uint32_t)S.w.n_rle));
    ok = b.bitpos == 16 + (form == kDefFixed ? S.w.bits_fixed : S.w.bits_dynamic);
    // the bytes of the last, partial word, and word 0 with BSIZE in front
    const uint32_t bw = b.bitpos >> 5, end = 16 + ((b.bitpos + 7) >> 3);  // the payload's end in the member
    const uint32_t last = rfl(S.stage[0]);
    const uint32_t w0 = (bw == 0 ? last : b.word0) | bsize;
    if (ok && lane < 4) {
      if (16u + (uint32_t)lane < end) mem[16 + lane] = (uint8_t)(w0 >> (8 * lane));
      const uint32_t q = 16 + 4 * bw + (uint32_t)lane;
      if (bw > 0 && q < end) mem[q] = (uint8_t)(last >> (8 * lane));
    }
  }
  if (ok && lane < 8) {
    const uint32_t v = lane < 4 ? crc >> (8 * lane) : n >> (8 * (lane - 4));
    mem[kDefMemberHead + plen + lane] = (uint8_t)v;
  }
  if (lane == 0) clen[blockIdx.x] = ok ? (int32_t)total : -1;
}

namespace {

// coff[0..n] = prefix sums of the member sizes (a failed member counts 0).
__global__ __launch_bounds__(1024) void bgzf_compact_scan_kernel(const int32_t* __restrict__ clen, int32_t n,
                                                                 int64_t* __restrict__ coff) {
  __shared__ int64_t part[1024];
  const int t = (int)threadIdx.x;
  const int per = (n + 1023) / 1024, b0 = min(n, t * per), b1 = min(n, b0 + per);
  int64_t sum = 0;
  for (int k = b0; k < b1; ++k) sum += max(clen[k], 0);
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    int64_t run = 0;
    for (int k = 0; k < 1024; ++k) {
      const int64_t v = part[k];
      part[k] = run;
      run += v;
    }
    coff[n] = run;
  }
  __syncthreads();
  int64_t run = part[t];
  for (int k = b0; k < b1; ++k) {
    coff[k] = run;
    run += max(clen[k], 0);
  }
}

// Member k from its slot to out + coff[k]: bytes up to out's word boundary,
// then whole words assembled from two aligned slot words, then the tail.
__global__ __launch_bounds__(256) void bgzf_compact_copy_kernel(const uint8_t* __restrict__ slots,
                                                                const int64_t* __restrict__ coff,
                                                                uint8_t* __restrict__ out) {
  const int64_t k = blockIdx.x;
  const uint8_t* __restrict__ src = slots + k * kSlot;
  const uint32_t* __restrict__ src32 = reinterpret_cast<const uint32_t*>(src);
  uint8_t* dst = out + coff[k];
  const uint32_t len = (uint32_t)(coff[k + 1] - coff[k]);
  const uint32_t head = min(len, (uint32_t)((4 - ((uintptr_t)dst & 3)) & 3)), words = (len - head) >> 2;
  const uint32_t t = threadIdx.x;
  if (t < head) dst[t] = src[t];
  uint32_t* dst32 = reinterpret_cast<uint32_t*>(dst + head);
  const uint32_t sh = 8 * (head & 3);
  for (uint32_t i = t; i < words; i += 256) {
    const uint32_t q = (head + 4 * i) >> 2;  // q + 1 <= (len + 3) / 4 < the slot's words
    const uint32_t lo = src32[q], hi = src32[q + 1];
    dst32[i] = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
  }
  const uint32_t done = head + 4 * words;
  if (t < len - done) dst[done + t] = src[done + t];
}

}  // namespace

int launch_bgzf_deflate(const uint8_t* data, int64_t n_bytes, int32_t block_bytes, uint8_t* slots, int32_t* clen,
                        hipStream_t s) {
  if (n_bytes <= 0) return FCS_OK;
  const int64_t members = (n_bytes + block_bytes - 1) / block_bytes;
  hipLaunchKernelGGL(bgzf_deflate_kernel, dim3((unsigned)members), dim3(64), 0, s, data, n_bytes, block_bytes, slots,
                     clen);
  FCS_HIP_CHECK(hipGetLastError());
  return FCS_OK;
}

int launch_bgzf_compact(const uint8_t* slots, const int32_t* clen, int32_t n, int64_t* coff, uint8_t* out,
                        hipStream_t s) {
  if (n <= 0) return FCS_OK;
  hipLaunchKernelGGL(bgzf_compact_scan_kernel, dim3(1), dim3(1024), 0, s, clen, n, coff);
  FCS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(bgzf_compact_copy_kernel, dim3((unsigned)n), dim3(256), 0, s, slots, coff, out);
  FCS_HIP_CHECK(hipGetLastError());
  return FCS_OK;
}

}  // namespace fcs
