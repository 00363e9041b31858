// Raw DEFLATE encoding (RFC 1951) of one BGZF member's payload: the parts of
// the encoder that are serial and easy to get wrong, written once for the
// device and the host.  The device kernel (bgzf_deflate.hip) runs them on one
// wave per member with all of this state in LDS; the host unit test
// (tools/micro/deflate_test.cpp) runs the very same code under ASan / UBSan
// and inflates the result with zlib.  SURVEY.md §8 row f3: the other direction
// of bgzf_inflate.h (`fcs-genome` bgzips its VCF and writes BAM).
//
// What lives here:
// - the LZ77 token alphabet (length / distance symbols and their extra bits);
// - code-length construction from a histogram (Moffat / Katajainen in-place
//   minimum redundancy on the symbols sorted by (frequency, symbol)), limited
//   to 15 bits (7 for the code-length code) by moving codes down the tree
//   until the Kraft sum is exactly one, and canonical code assignment;
// - the dynamic block header: HLIT / HDIST / HCLEN trimming and the 16 / 17 /
//   18 run symbols;
// - the cost of the stored, fixed and dynamic forms and the choice between
//   them (the smallest; a member is never larger than its stored form);
// - a token's bits (Huffman codes are sent most significant bit first, so the
//   tables hold them bit-reversed: a token is one LSB-first bit string);
// - the 18-byte BGZF header.
// Finding the matches is the caller's business (lane-parallel on the device,
// the same scheme run serially in the host test).
//
// The policy `L` is bgzf_inflate.h's: `L::id()` / `L::n()` (the lanes that
// share a member: 1 on the host, 64 on the device) and `L::sync()`.  The
// symbol sort is split over the lanes; the rest is done by lane 0 between two
// syncs.  Every array indexed at run time lives in DefWork, never in a local
// array (LDS on the device: no scratch).
#pragma once

#include <cstddef>
#include <cstdint>

namespace fcs {

constexpr int kDefBlockMax = 0xff00;  // input bytes per member (htslib's BGZF_BLOCK_SIZE)
constexpr int kDefMinMatch = 3, kDefMaxMatch = 258, kDefWindow = 32768;
constexpr int kDefTooFar = 4096;  // a 3-byte match further back costs more than its literals (zlib's TOO_FAR)
constexpr int kDefHashBits = 13;  // the matcher's table of last positions
constexpr int kDefHashBytes = 4;  // bytes hashed per position
constexpr int kDefChunk = 64;     // positions matched at once (the wave's lanes)
constexpr int kDefLl = 288, kDefD = 32, kDefCl = 19;  // alphabet sizes as the fixed code counts them
constexpr int kDefNumLl = 286, kDefNumD = 30;         // symbols a block may use
constexpr int kDefEob = 256;
constexpr int kDefMemberHead = 18, kDefMemberTail = 8;

enum : int { kDefStored = 0, kDefFixed = 1, kDefDynamic = 2 };

struct DefWork {
  uint32_t freq[kDefLl + kDefD];  // literal / length histogram, then the distance one
  uint32_t cl_freq[kDefCl];
  uint16_t code[kDefLl + kDefD];  // bit-reversed codes
  uint16_t cl_code[kDefCl];
  uint8_t len[kDefLl + kDefD];  // code lengths
  uint8_t cl_len[kDefCl];
  // building a code
  uint32_t key[kDefLl];  // frequencies in sorted order, then the in-place tree, then depths
  uint16_t sym[kDefLl];  // symbols by (frequency, symbol)
  uint32_t cnt[17], next[17];
  // the dynamic header: the run-length coded code lengths
  uint8_t rle_sym[kDefNumLl + kDefNumD], rle_extra[kDefNumLl + kDefNumD];
  int32_t n_rle, nlit, ndist, ncl;
  // the plan
  int32_t form;                                   // kDefStored / kDefFixed / kDefDynamic
  uint32_t bits_fixed, bits_dynamic, bits_token;  // payload bits of the two coded forms; of the chosen one's tokens
};

__host__ __device__ __forceinline__ uint32_t def_hash(uint32_t v) {
  if (kDefHashBytes == 3) v &= 0xFFFFFFu;
  return (v * 2654435761u) >> (32 - kDefHashBits);
}

// 31 - clz for v >= 1
__host__ __device__ __forceinline__ int def_log2(uint32_t v) {
  int r = 0;
  if (v >> 16) r += 16, v >>= 16;
  if (v >> 8) r += 8, v >>= 8;
  if (v >> 4) r += 4, v >>= 4;
  if (v >> 2) r += 2, v >>= 2;
  return r + (int)(v >> 1);
}

// length 3..258 -> symbol 257..285, its extra bits
__host__ __device__ __forceinline__ void def_len_sym(int len, int& sym, int& nextra, uint32_t& extra) {
  const uint32_t l = (uint32_t)(len - 3);
  if (l < 8) { sym = 257 + (int)l, nextra = 0, extra = 0; return; }
  if (len == 258) { sym = 285, nextra = 0, extra = 0; return; }
  nextra = def_log2(l) - 2;
  sym = 257 + 4 * nextra + 4 + (int)((l >> nextra) & 3u);
  extra = l & ((1u << nextra) - 1);
}
// distance 1..32768 -> symbol 0..29, its extra bits
__host__ __device__ __forceinline__ void def_dist_sym(int dist, int& sym, int& nextra, uint32_t& extra) {
  const uint32_t d = (uint32_t)(dist - 1);
  if (d < 4) { sym = (int)d, nextra = 0, extra = 0; return; }
  nextra = def_log2(d) - 1;
  sym = 2 * nextra + 2 + (int)((d >> nextra) & 1u);
  extra = d & ((1u << nextra) - 1);
}
__host__ __device__ __forceinline__ int def_ll_extra(int sym) {  // extra bits of a literal / length symbol
  return sym < 265 || sym >= 285 ? 0 : (sym - 261) >> 2;
}
__host__ __device__ __forceinline__ int def_d_extra(int sym) { return sym < 4 ? 0 : (sym - 2) >> 1; }

__host__ __device__ __forceinline__ uint32_t def_reverse(uint32_t v, int n) {
  uint32_t r = 0;
  for (int k = 0; k < n; ++k) r |= ((v >> k) & 1u) << (n - 1 - k);
  return r;
}

// Code lengths (<= max_len, Kraft sum exactly 1) of the n symbols with the
// histogram freq into len.  No used symbol: all zero; one: that symbol gets
// length 1 (the caller decides whether the format takes a one-code tree).
template <class L>
__host__ __device__ inline void def_build_lengths(DefWork& w, const uint32_t* freq, int n, int max_len, uint8_t* len) {
  // rank of every used symbol in (frequency, symbol) order: split over the lanes
  for (int s = L::id(); s < n; s += L::n()) {
    len[s] = 0;
    const uint32_t f = freq[s];
    if (!f) continue;
    int rank = 0;
    for (int t = 0; t < n; ++t) {
      const uint32_t g = freq[t];
      rank += (int)(g != 0 && (g < f || (g == f && t < s)));
    }
    w.sym[rank] = (uint16_t)s;
    w.key[rank] = f;
  }
  L::sync();
  if (L::id() == 0) {
    int used = 0;
    for (int s = 0; s < n; ++s) used += (int)(freq[s] != 0);
    if (used == 1) len[w.sym[0]] = 1;
    if (used >= 2) {
      uint32_t* const A = w.key;
      // Moffat / Katajainen, "In-place calculation of minimum-redundancy codes"
      A[0] += A[1];
      int root = 0, leaf = 2;
      for (int nx = 1; nx < used - 1; ++nx) {
        if (leaf >= used || A[root] < A[leaf]) { A[nx] = A[root]; A[root++] = (uint32_t)nx; }
        else A[nx] = A[leaf++];
        if (leaf >= used || (root < nx && A[root] < A[leaf])) { A[nx] += A[root]; A[root++] = (uint32_t)nx; }
        else A[nx] += A[leaf++];
      }
      A[used - 2] = 0;
      for (int nx = used - 3; nx >= 0; --nx) A[nx] = A[A[nx]] + 1;
      int avbl = 1, inner = 0, depth = 0;
      root = used - 2;
      int nx = used - 1;
      while (avbl > 0) {
        while (root >= 0 && (int)A[root] == depth) { ++inner; --root; }
        while (avbl > inner) { A[nx--] = (uint32_t)depth; --avbl; }
        avbl = 2 * inner;
        ++depth;
        inner = 0;
      }
      // codes per length, the over-long ones folded into max_len; then codes
      // moved down until the Kraft sum is back to one
      for (int l = 0; l <= 16; ++l) w.cnt[l] = 0;
      for (int i = 0; i < used; ++i) w.cnt[A[i] < (uint32_t)max_len ? A[i] : (uint32_t)max_len]++;
      uint32_t total = 0;
      for (int l = max_len; l > 0; --l) total += w.cnt[l] << (max_len - l);
      while (total != (1u << max_len)) {
        w.cnt[max_len]--;
        for (int l = max_len - 1; l > 0; --l)
          if (w.cnt[l]) { w.cnt[l]--; w.cnt[l + 1] += 2; break; }
        --total;
      }
      // the shortest codes to the most frequent symbols
      int j = used;
      for (int l = 1; l <= max_len; ++l)
        for (uint32_t c = w.cnt[l]; c > 0; --c) len[w.sym[--j]] = (uint8_t)l;
    }
  }
  L::sync();
}

// Canonical codes of the lengths len[0, n), bit-reversed.
template <class L>
__host__ __device__ inline void def_assign_codes(DefWork& w, const uint8_t* len, int n, uint16_t* code) {
  if (L::id() == 0) {
    for (int l = 0; l <= 16; ++l) w.cnt[l] = 0;
    for (int s = 0; s < n; ++s) w.cnt[len[s]]++;
    w.cnt[0] = 0;
    uint32_t c = 0;
    for (int l = 1; l <= 15; ++l) {
      c = (c + w.cnt[l - 1]) << 1;
      w.next[l] = c;
    }
    for (int s = 0; s < n; ++s) {
      const int l = len[s];
      code[s] = l ? (uint16_t)def_reverse(w.next[l]++, l) : 0;
    }
  }
  L::sync();
}

__host__ __device__ __forceinline__ int def_cl_order(int i) {  // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
  return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - (i - 3) / 2 : 8 + (i - 4) / 2;
}

// The fixed code's lengths.
template <class L>
__host__ __device__ inline void def_fixed_lengths(DefWork& w) {
  for (int s = L::id(); s < kDefLl + kDefD; s += L::n())
    w.len[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
  L::sync();
}

// From the histograms (w.freq, the end-of-block symbol counted) of a block of
// n input bytes: the dynamic code, the run-length coded header, the cost of
// each form and the choice.  Leaves the chosen form's lengths and codes in
// w.len / w.code (nothing for stored).
template <class L>
__host__ __device__ inline void def_plan(DefWork& w, uint32_t n) {
  def_build_lengths<L>(w, w.freq, kDefNumLl, 15, w.len);
  def_build_lengths<L>(w, w.freq + kDefLl, kDefNumD, 15, w.len + kDefLl);
  if (L::id() == 0) {
    for (int s = kDefNumLl; s < kDefLl; ++s) w.len[s] = 0;
    for (int s = kDefNumD; s < kDefD; ++s) w.len[kDefLl + s] = 0;
    int nlit = kDefNumLl, ndist = kDefNumD;
    while (nlit > 257 && !w.len[nlit - 1]) --nlit;
    while (ndist > 1 && !w.len[kDefLl + ndist - 1]) --ndist;
    w.nlit = nlit;
    w.ndist = ndist;
    // the two length lists as one sequence, run-length coded
    const int total = nlit + ndist;
    int m = 0;
    for (int s = 0; s < kDefCl; ++s) w.cl_freq[s] = 0;
    for (int i = 0; i < total;) {
      const int v = i < nlit ? w.len[i] : w.len[kDefLl + i - nlit];
      int run = 1;
      while (i + run < total && (i + run < nlit ? w.len[i + run] : w.len[kDefLl + i + run - nlit]) == v) ++run;
      i += run;
      if (v == 0) {
        while (run >= 11) {
          const int r = run < 138 ? run : 138;
          w.rle_sym[m] = 18, w.rle_extra[m++] = (uint8_t)(r - 11), w.cl_freq[18]++;
          run -= r;
        }
        if (run >= 3) {
          w.rle_sym[m] = 17, w.rle_extra[m++] = (uint8_t)(run - 3), w.cl_freq[17]++;
          run = 0;
        }
      } else {
        w.rle_sym[m] = (uint8_t)v, w.rle_extra[m++] = 0, w.cl_freq[v]++;
        --run;
        while (run >= 3) {
          const int r = run < 6 ? run : 6;
          w.rle_sym[m] = 16, w.rle_extra[m++] = (uint8_t)(r - 3), w.cl_freq[16]++;
          run -= r;
        }
      }
      for (; run > 0; --run) w.rle_sym[m] = (uint8_t)v, w.rle_extra[m++] = 0, w.cl_freq[v]++;
    }
    w.n_rle = m;
    // a decoder takes no incomplete code-length code: at least two symbols
    int used = 0;
    for (int s = 0; s < kDefCl; ++s) used += (int)(w.cl_freq[s] != 0);
    for (int s = 0; used < 2 && s < kDefCl; ++s)
      if (!w.cl_freq[s]) w.cl_freq[s] = 1, ++used;  // (its one count is not sent: the cost below counts sent symbols)
  }
  L::sync();
  def_build_lengths<L>(w, w.cl_freq, kDefCl, 7, w.cl_len);
  def_assign_codes<L>(w, w.cl_len, kDefCl, w.cl_code);
  if (L::id() == 0) {
    int ncl = kDefCl;
    while (ncl > 4 && !w.cl_len[def_cl_order(ncl - 1)]) --ncl;
    w.ncl = ncl;
    uint32_t head = 3 + 5 + 5 + 4 + 3 * (uint32_t)ncl;
    for (int i = 0; i < w.n_rle; ++i) {
      const int s = w.rle_sym[i];
      head += (uint32_t)w.cl_len[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u);
    }
    uint32_t dyn = 0, fix = 0;
    for (int s = 0; s < kDefNumLl; ++s) {
      const uint32_t f = w.freq[s], x = (uint32_t)def_ll_extra(s);
      dyn += f * (w.len[s] + x);
      fix += f * ((s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u) + x);
    }
    for (int s = 0; s < kDefNumD; ++s) {
      const uint32_t f = w.freq[kDefLl + s], x = (uint32_t)def_d_extra(s);
      dyn += f * (w.len[kDefLl + s] + x);
      fix += f * (5u + x);
    }
    w.bits_dynamic = head + dyn;
    w.bits_fixed = 3 + fix;
    const uint32_t by_dyn = (w.bits_dynamic + 7) >> 3, by_fix = (w.bits_fixed + 7) >> 3, by_sto = n + 5;
    w.form = by_sto <= by_fix && by_sto <= by_dyn ? kDefStored : by_fix <= by_dyn ? kDefFixed : kDefDynamic;
    w.bits_token = w.form == kDefFixed ? fix : dyn;
  }
  L::sync();
  if (w.form == kDefFixed) def_fixed_lengths<L>(w);
  if (w.form != kDefStored) {
    def_assign_codes<L>(w, w.len, kDefLl, w.code);
    def_assign_codes<L>(w, w.len + kDefLl, kDefD, w.code + kDefLl);
  }
}

// Payload bytes of the chosen form.
__host__ __device__ __forceinline__ uint32_t def_payload_bytes(const DefWork& w, uint32_t n) {
  return w.form == kDefStored ? n + 5 : ((w.form == kDefFixed ? w.bits_fixed : w.bits_dynamic) + 7) >> 3;
}

// The block header of the chosen coded form through sink.put(value, bits)
// (bits <= 16, LSB first); one lane's work.
template <class Sink>
__host__ __device__ inline void def_put_header(const DefWork& w, Sink& sink) {
  sink.put(1u, 1);  // BFINAL: a member is one block
  sink.put((uint32_t)w.form, 2);
  if (w.form != kDefDynamic) return;
  sink.put((uint32_t)(w.nlit - 257), 5);
  sink.put((uint32_t)(w.ndist - 1), 5);
  sink.put((uint32_t)(w.ncl - 4), 4);
  for (int i = 0; i < w.ncl; ++i) sink.put(w.cl_len[def_cl_order(i)], 3);
  for (int i = 0; i < w.n_rle; ++i) {
    const int s = w.rle_sym[i];
    sink.put(w.cl_code[s], w.cl_len[s]);
    if (s >= 16) sink.put(w.rle_extra[i], s == 16 ? 2 : s == 17 ? 3 : 7);
  }
}

// One token as an LSB-first bit string (at most 15 + 5 + 15 + 13 = 48 bits):
// a literal (dist == 0, v the byte or kDefEob) or a match (v its length).
__host__ __device__ __forceinline__ void def_token_bits(const DefWork& w, int v, int dist, uint64_t& bits, int& nbits) {
  if (dist == 0) {
    bits = w.code[v];
    nbits = w.len[v];
    return;
  }
  int ls, lx, ds, dx;
  uint32_t le, de;
  def_len_sym(v, ls, lx, le);
  def_dist_sym(dist, ds, dx, de);
  uint64_t b = w.code[ls];
  int k = w.len[ls];
  b |= (uint64_t)le << k;
  k += lx;
  b |= (uint64_t)w.code[kDefLl + ds] << k;
  k += w.len[kDefLl + ds];
  b |= (uint64_t)de << k;
  k += dx;
  bits = b;
  nbits = k;
}

// The symbols a token counts towards (dsym < 0: none).
__host__ __device__ __forceinline__ void def_token_syms(int v, int dist, int& lsym, int& dsym) {
  if (dist == 0) {
    lsym = v, dsym = -1;
    return;
  }
  int x;
  uint32_t e;
  def_len_sym(v, lsym, x, e);
  def_dist_sym(dist, dsym, x, e);
}

// The first 16 of a member's 18 header bytes as four little-endian words (gzip
// magic, deflate, FEXTRA, no mtime, XFL 0, OS unknown, XLEN 6, 'B' 'C', SLEN
// 2); BSIZE (member bytes - 1) follows.
__host__ __device__ __forceinline__ uint32_t def_member_head_word(int i) {
  return i == 0 ? 0x04088b1fu : i == 1 ? 0u : i == 2 ? 0x0006ff00u : 0x00024342u;
}

}  // namespace fcs
