// The rules of indel realignment that the device kernels (indel.hip), the host
// oracle (host/indel.cpp) and the stand-alone program (tools/micro/ir_test.cpp)
// share, each stated once (DESIGN §2 [EXT] "RealignerTargetCreator and
// IndelRealigner, round 22"): the base codes, the score S of a read against a
// sequence at an offset, the order in which candidates are compared, and the
// candidate set of a (consensus, read) pair.
//
// The kernels do not compare codes one by one.  A read base is staged as the
// one-hot byte ir_hot(code) and a sequence base as the byte ir_mask(code), the
// set of read codes that differ from it; `ir_hot & ir_mask` is non-zero exactly
// when ir_differ holds, for four bases in one AND.  ir_test checks the two
// statements against each other for every pair of codes.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define IR_HD __host__ __device__ __forceinline__
#else
#define IR_HD inline
#endif

namespace fcs {

constexpr int kIrReadMax = 512;   // bases of a stripped read
constexpr int kIrSeqMax = 4096;   // bases of a window or a consensus
constexpr int kIrOverhang = 99;   // S per read base beyond the sequence's end
constexpr int kIrOrigMax = 1 << 30;
constexpr int kIrStatusField = 1, kIrStatusPairs = 2;

// 0 .. 3 for A C G T in either case, 4 for anything else.
IR_HD int ir_code(uint8_t b) {
  switch (b | 0x20) {
    case 'a': return 0;
    case 'c': return 1;
    case 'g': return 2;
    case 't': return 3;
  }
  return 4;
}

IR_HD bool ir_differ(int a, int b) { return a < 4 && b < 4 && a != b; }

// The kernels' encodings of a read code and of a sequence code.
IR_HD uint32_t ir_hot(int code) { return code < 4 ? 1u << code : 0u; }
IR_HD uint32_t ir_mask(int code) { return code < 4 ? 0xFu ^ (1u << code) : 0u; }

// S(r, s, o): rc, rq the read's L codes and qualities, s the sequence's len codes, o >= 0.
IR_HD uint32_t ir_score(const uint8_t* rc, const uint8_t* rq, int L, const uint8_t* s, int64_t len, int64_t o) {
  uint32_t sum = 0;
  for (int i = 0; i < L; ++i) {
    if (o + i >= len) sum += kIrOverhang;
    else if (ir_differ(rc[i], s[o + i])) sum += rq[i];
  }
  return sum;
}

// The argmin order: the smaller score, then the read's original offset, then the smaller offset.
// The smallest key of the candidates is best(c, r); offsets are below 2^31.
IR_HD uint64_t ir_key(uint32_t score, bool is_orig, int32_t o) {
  return ((uint64_t)score << 32) | (is_orig ? 0u : 0x80000000u) | (uint32_t)o;
}
IR_HD uint32_t ir_key_score(uint64_t key) { return (uint32_t)(key >> 32); }
IR_HD int32_t ir_key_offset(uint64_t key) { return (int32_t)(key & 0x7FFFFFFFu); }

// The candidate set: the original offset, and every o in [0, ir_offsets(len, L)).
IR_HD int64_t ir_offsets(int64_t len, int L) { return len >= L ? len - L + 1 : 0; }

// best(c, r) by the plain statement.
IR_HD uint64_t ir_best(const uint8_t* rc, const uint8_t* rq, int L, const uint8_t* s, int64_t len, int32_t orig) {
  uint64_t best = ir_key(ir_score(rc, rq, L, s, len, orig), true, orig);
  const int64_t n = ir_offsets(len, L);
  for (int64_t o = 0; o < n; ++o) {
    const uint64_t k = ir_key(ir_score(rc, rq, L, s, len, o), false, (int32_t)o);
    if (k < best) best = k;
  }
  return best;
}

}  // namespace fcs
