// PairHMM fp32 forward pass with COLUMN-BLOCKED lanes and continuous row
// streams (included by phmm_kernels.hip after phmm_stream.h).
//
// phmm3 (phmm_stream.h) gives each lane two read rows of a 32-row stripe and
// sweeps the haplotype columns over time, so every stripe pays a 31-step
// skew fill/drain and a ~700-VALU stripe setup (10.4 VALU per
// cell, of which the steady steps are 7.5).  Here the roles are transposed:
//   * lane l of a 16-lane segment OWNS the haplotype columns l*C + 1 ..
//     l*C + C (C per launch class, H <= 16 C - 1) and keeps their state in
//     registers: X~(r, c) (the diagonal hand-off M*mm' + I*gm' + D*gm' divided
//     by mm', see the cell below) and I(r + 1, c) of the row it finished last;
//   * each step the lane runs ONE read row across its C columns (row g = t - l
//     of the segment's row stream: one row of skew per lane), so a step is C
//     cells of straight-line code with no per-cell lane traffic: the only
//     cross-lane values are the lane below's X~(g - 1, l*C) and the deletion
//     chain E entering column l*C + 1 (two DPP row_shr:1 per value);
//   * the two halves of every packed register are two INDEPENDENT pairs
//     ("half-streams" A and B), so all six FP ops of a cell are v_pk_*_f32
//     on two cells, with no swaps;
//   * row parameters (7 per row and half) come from a 32-row LDS ring that the
//     segment's 16 lanes fill 8 rows ahead (one (row, half) item per lane every
//     8 steps): no per-stripe setup.
// Each half-stream runs K pairs back to back as one row stream per pair
// [rows 1..R, V, Z]: V sums the last row (as in phmm3: prior 1 on the
// haplotype's columns and on column H + 1, 0 past it, E = running sum), and
// Z resets every column to the row-0 boundary of the next pair (X~ = 1 with
// row 1's priors pre-multiplied by (2^120 / H) * gm_1, I = 0) through an E
// chain of ones started at lane 0.  The sum therefore leaves lane 15 as the
// E entering column 16 C + 1 of the V row: no column search.  There is no
// fill or drain inside a stream, only at its end (15 steps per stream).
// The cell is SIX fp32 operations, one fewer than phmm3's:
//     E  = fma(E(c - 1), yy, M(c - 1))      deletion chain, unit coefficient
//     M' = X~(r - 1, c) * prior(c + 1)      the next column's match
//     X~ = fma(E, b, fma(I, a, M))          hand-off, divided by mm'
//     I' = fma(M, mx, I * xx)
//   * along a row my and yy are constants, so D = my * E with E = yy * E + M:
//     a yy-weighted sum of the row's earlier M, bounded by the row's mass;
//   * X~ = X / mm' with a = gm' / mm' and b = gm' * my / mm' (mm', gm': the
//     row below's match-to-match and gap-to-match); the row below gets mm'
//     back in its priors, e1 * mm_own and e3 * mm_own (row 1 keeps (2^120 / H)
//     * gm_1: mm_1 never enters the recurrence).  Row R hands over M + I
//     (a = 1, b = 0), V hands over M (a = b = 0), Z gives E = X~ = 1 (yy = b =
//     1, a = 0, priors 0).
//   * A row below with mm' < 2^-4 (0 when both indel qualities are <= 3) is a
//     hazard: its item is built with a = b = 0, so only finite values enter
//     the stream (a Z row does not clear a NaN), and its pair is flagged in
//     `other`: the capture hands it to the one-row kernel like a haplotype
//     byte outside A/C/G/T/N.  With the bound a <= 16 and X~ < 2^125.
// The sums agree with the row-streamed kernel's to fp32 rounding (about 1e-7
// relative), no longer bitwise; the three kernels here stay bitwise equal to
// each other.
// Three kernels follow.  phmm4_kernel is the one described above, two packed
// half-streams per register; it stands alone and is kept as the bitwise
// reference of the other two (FCSHIP_COLS=packed).  phmm5_kernel and
// phmm6_kernel carry one pair stream per register and share one stream body,
// cols1_stream<C, Feed>: tables, code fetch, capture, ring stages, the 16-step
// block with the step arithmetic and the result write.  Each kernel adds only
// how pairs reach the streams:
//   * phmm5_kernel (FCSHIP_COLS=single): the batch loop over the workgroups,
//     the prefix-scan segment table of a batch, and Cols1Batch (pair k in lane
//     k, K pairs per stream, a fixed number of steps);
//   * phmm6_kernel (the one every class launches): the first dequeue and the
//     early exit, and Cols1Queue (the circular segment table filled from a
//     per-class queue by a persistent grid, streams that end when the class
//     is exhausted).  Each class is compiled and launched for its own number
//     of waves per SIMD, cols6_waves(C): 3 for every class, see there.
// The body holds little besides the 2 C floats of state across its pass loop
// (DESIGN §4.1j): the staged ring row waits as two packed dwords (PackedRow),
// and the segment table keeps pair, R, H, first row and read offset only; the
// haplotype offset and the first row's scale 2^120 / H are read again from
// the table's pair at the block tops that need them, once per pair.
// That the two compute the same bits per step is therefore structural: there
// is one step.  What the tests hold equal is the rest: the stream mechanics of
// phmm6 against phmm5 on the same batch (tests/test_pairhmm_queue_gpu.py), and
// the shared step against phmm4's independent one (there and in
// tests/test_pairhmm_single_gpu.py).
#pragma once

namespace fcs {

constexpr int kColsClasses = 8;
// The next pair's haplotype codes are converted at the first block start >= 16
// rows after a switch: <= 23 rows after it with phmm4's 8-step blocks, <= 31
// with phmm5's 16-step blocks, and the next pair starts R + 2 rows after it, so
// R >= 29 would do for both; 33 is the streamed kernels' common minimum.
constexpr int kColsMinR = 33;
// Columns per lane of launch class c (longest haplotypes first): H <= 16 C - 1.
__host__ __device__ constexpr int cols_C(int c) { return c == 0 ? 19 : 18 - c; }  // 19, 17, 16, .., 11
__host__ __device__ constexpr int cols_hmax(int c) { return 16 * cols_C(c) - 1; }
// The smallest class that holds H (-1: none).
__host__ __device__ inline int cols_class(int H) {
  for (int c = kColsClasses - 1; c >= 0; --c)
    if (H <= cols_hmax(c)) return c;
  return -1;
}
// LDS per wave: a 32-row ring per segment of six 16-byte chunks per row:
// {e1, e3}, {b, yy}, {a, -}, {mx, xx} as {A, B} pairs, the match tables
// {Tlo A, Tlo B, Thi A, Thi B} and the Z flags {A, B, A, B} (floats).  The
// layout is chunk-major, then segment, then slot (16 B entries): the 16 lanes
// of a segment read 16 consecutive slots of a chunk, 256 contiguous bytes
// (row-major records 256 B apart per slot put all 16 lanes on the same banks:
// 7.4 conflict cycles per LDS cycle; segment-minor entries, 64 B apart, 4.5).
constexpr int kColsRing = 32;
constexpr int kColsChunks = 6;
constexpr int kColsChunkBytes = kColsRing * 4 * 16;  // one chunk of every (slot, segment)
constexpr int kColsCapOff = kColsChunks * kColsChunkBytes;  // lane 15's E per step of a block
constexpr int kColsTabOff = kColsCapOff + 4 * 8 * 8;  // ph2pr | dmatch | dmis (3 x 128 floats) for the ring items
constexpr int kColsLds = kColsTabOff + 3 * 128 * 4;

// A constant materialised where it is used: left to the compiler, the
// constants of the code conversion and the item builder are hoisted out of
// every loop and held in VGPRs for the whole kernel.
__device__ __forceinline__ uint32_t vconst(uint32_t k) {
  uint32_t r;
  asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "i"(k));
  return r;
}

// One (row, half) item of the ring.
struct ColsItem {
  float e1, e3, b, yy, a, mx, xx;
  uint32_t tlo, thi;
  float z;
};

// A row below whose match-to-match is under this bound (both indel qualities
// <= 3 give exactly 0) cannot be divided out of the hand-off: its pair goes to
// the one-row kernel.  With it a <= 16, so X~ stays below 2^125 even for H = 1.
constexpr float kColsMinMm = 0.0625f;

// Roles: 0 = Z (reset row, also before and after the stream), 2 = row r < R,
// 3 = row R, 4 = V.  Match tables for v_perm on the column codes (A, C, G, T
// = 0..3 in Tlo, hap N = 4, column H + 1 = 5, past it = 6 in Thi): byte = 1
// on a match.
// oiq: the row's own insertion quality (rows >= 2 carry their own match-to-
// match in the priors: the row above handed X / mm over).  hazard: the row
// below's match-to-match is under kColsMinMm; the item then holds a = b = 0,
// so nothing but finite values enters the stream, and the caller flags the pair.
__device__ __forceinline__ ColsItem cols_item(const PhmmTables<float>& tab, const RawRow& raw, int oiq, int role,
                                              bool first, float ih, bool& hazard) {
  ColsItem c;
  hazard = false;
  if (role == 2 || role == 3) {
    const RowP<float> q = row_params<float, false>(tab, raw);
    const int oi = oiq & 127, od = raw.dq & 127;
    const int hi = oi > od ? oi : od, lo = oi > od ? od : oi;
    const float x0 = first ? ih * tab.dmatch[raw.gq & 127] : tab.mm[((hi * (hi + 1)) >> 1) + lo];
    const bool last = role == 3;
    hazard = !last && !(q.mm >= kColsMinMm);
    const float inv = (last || hazard) ? 0.f : 1.f / q.mm;
    c.e1 = q.e1 * x0;
    c.e3 = q.e3 * x0;
    c.b = q.my * inv;  // q.my = my * gm' (row_params)
    c.yy = q.yy;
    c.a = last ? 1.f : q.gm * inv;
    c.mx = last ? 0.f : q.mx;
    c.xx = last ? 0.f : q.xx;
    const int bc = base_code((unsigned char)raw.rb);
    c.tlo = bc < 4 ? 1u << (8 * bc) : bc == 4 ? vconst(0x01010101u) : 0u;
    c.thi = 0x00000001u;
    c.z = 0.f;
  } else if (role == 4) {  // V: prior 1 on codes 0..5, 0 past column H + 1; E = running sum of M, X~ = M
    c.e1 = 1.f;
    c.e3 = 0.f;
    c.yy = 1.f;
    c.a = c.b = c.mx = c.xx = 0.f;
    c.tlo = vconst(0x01010101u);
    c.thi = vconst(0x00000101u);
    c.z = 0.f;
  } else {  // Z: M = 0, E = 1 (from lane 0's boundary), X~ = E = 1, I = 0
    c.e1 = c.e3 = c.a = c.mx = c.xx = 0.f;
    c.b = c.yy = 1.f;
    c.tlo = c.thi = 0u;
    c.z = 1.f;
  }
  return c;
}

__device__ __forceinline__ void cols_put(unsigned char* smem, int slot, int seg, int h, const ColsItem& c) {
  float* const p = reinterpret_cast<float*>(smem + (seg * kColsRing + slot) * 16) + h;
  constexpr int F = kColsChunkBytes / 4;  // floats per chunk
  p[0] = c.e1;
  p[2] = c.e3;
  p[F] = c.b;
  p[F + 2] = c.yy;
  p[2 * F] = c.a;
  p[2 * F + 2] = 0.f;
  p[3 * F] = c.mx;
  p[3 * F + 2] = c.xx;
  uint32_t* const q = reinterpret_cast<uint32_t*>(p);
  q[4 * F] = c.tlo;
  q[4 * F + 2] = c.thi;
  q[5 * F] = __float_as_uint(c.z);
  q[5 * F + 2] = __float_as_uint(c.z);
}

// Column codes of one lane's block (hap indices i0 .. i0 + C - 1, i.e. columns
// i0 + 1 ..) from the aligned dwords raw[] starting `al` bytes before i0:
// A,C,G,T,N = 0..4, index H (column H + 1) = 5, past it = 6.  `other`: a byte
// of the haplotype outside A/C/G/T/N.
template <int NW>
__device__ __forceinline__ void cols_convert(const uint32_t (&raw)[NW + 1], int al, int i0, int H, uint32_t (&code)[NW],
                                             bool& other) {
#pragma unroll
  for (int d = 0; d < NW; ++d) {
    const uint32_t x = __builtin_amdgcn_alignbyte(raw[d + 1], raw[d], (uint32_t)al);
    const int rel = H - (i0 + 4 * d);  // byte of index H (column H + 1) when in [0, 4)
    const int nv = min(max(rel, 0), 4);  // valid haplotype bytes in this dword
    const uint32_t vmask = nv >= 4 ? 0xFFFFFFFFu : (1u << (8 * nv)) - 1u;
    // hap_codes4 (phmm_stream.h) with its table constants materialised here
    const uint32_t sel = (x >> 1) & vconst(0x07070707u);
    uint32_t c = __builtin_amdgcn_perm(vconst(0x04050505u), vconst(0x02030100u), sel);
    const uint32_t back = __builtin_amdgcn_perm(vconst(0x0000004Eu), vconst(0x54474341u), c);
    other |= ((back ^ x) & vmask) != 0u;
    c = (c & vmask) | (vconst(0x06060606u) & ~vmask);
    if (rel >= 0 && rel < 4) c = (c & ~(0xFFu << (8 * rel))) | (0x05u << (8 * rel));
    code[d] = c;
  }
}

// Aligned dwords covering a lane's C haplotype bytes (only those holding a
// byte of the haplotype are read: the buffer ends inside the last one).
template <int NW>
__device__ __forceinline__ void cols_load(const uint8_t* __restrict__ hb, int64_t ho, int H, int i0, uint32_t (&raw)[NW + 1],
                                          int& al) {
  const int64_t s = ho + i0;
  al = (int)(s & 3);
  const int64_t base = s - al;
  const uint32_t* const src = reinterpret_cast<const uint32_t*>(hb + base);
#pragma unroll
  for (int d = 0; d <= NW; ++d) raw[d] = (base + 4 * d < ho + H && H > 0) ? src[d] : 0u;
}

template <int C>
__global__ __launch_bounds__(64, 2) void phmm4_kernel(
    const PhmmDevBatch b, const int32_t* __restrict__ order, const int64_t* __restrict__ bounds, const int cls,
    const int K, const int tail_pairs, const PhmmTables<float> gtab, double* __restrict__ out,
    int32_t* __restrict__ rescue_list, unsigned long long* __restrict__ rescue_count, const float thr,
    const int use_rescue, int32_t* __restrict__ fb_list, unsigned long long* __restrict__ fb_count) {
  constexpr int NW = (C + 3) / 4;  // code dwords per half
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x;
  const int seg = lane >> 4;
  const int sl = lane & 15;
  const int sbase = lane & 48;
  const int th = sl >> 3, tk = sl & 7;  // this lane's entry of the segment table: half th, pair tk
  const int i0 = sl * C;                // first haplotype index of this lane's columns
  const int64_t cbeg = bounds[cls];
  const long long count = bounds[cls + 1] - cbeg;
  order += cbeg;
  // the ring items' small tables in LDS (matchToMatch stays in global
  // memory): their lookups wait on LDS instead of the L2 (+1%)
  PhmmTables<float> tab = gtab;
  {
    float* const t = reinterpret_cast<float*>(smem_raw + kColsTabOff);
    for (int i = lane; i < 128; i += 64) {
      t[i] = gtab.ph2pr[i];
      t[128 + i] = gtab.dmatch[i];
      t[256 + i] = gtab.dmis[i];
    }
    tab.ph2pr = t;
    tab.dmatch = t + 128;
    tab.dmis = t + 256;
  }
  // Batches: 8 half-streams per wave, K pairs each, except the range's last
  // tail_pairs (shortest haplotypes), one pair per half-stream.
  const long long tailn = count < (long long)tail_pairs ? count : (long long)tail_pairs;
  const long long headn = count - tailn;
  const long long per = 8LL * K;
  const long long nb_head = (headn + per - 1) / per;
  const long long nbatch = nb_head + (tailn + 7) / 8;

  for (long long w = blockIdx.x; w < nbatch; w += gridDim.x) {
    const bool head = w < nb_head;
    const int Kb = head ? K : 1;
    const long long bstart = head ? w * per : headn + (w - nb_head) * 8;
    const long long bend = head ? min(headn, bstart + per) : min(count, bstart + 8);
    // Segment table: lane (th, tk) holds pair tk of half-stream th (half-
    // streams 2 seg, 2 seg + 1 of the batch take every 8th pair).
    const long long idx = bstart + 2 * seg + th + 8LL * tk;
    const int pm = (tk < Kb && idx < bend) ? order[idx] : -1;
    int Rm = 0, Hm = 0;
    int64_t rom = 0, hom = 0;
    float Im = 0.f;
    if (pm >= 0) {
      const int ri = b.pair_read[pm], hi = b.pair_hap[pm];
      Rm = b.read_len[ri];
      Hm = b.hap_len[hi];
      rom = b.read_off[ri];
      hom = b.hap_off[hi];
      Im = tab.init_const / (float)Hm;
    }
    const int len = pm >= 0 ? Rm + 2 : 0;  // rows 1..R, V, Z
    int incl = len;
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) {
      const int v = __shfl_up(incl, d, 8);
      if (tk >= d) incl += v;
    }
    const int Gm = incl - len;  // first stream row of the pair
    const int totA = __builtin_amdgcn_ds_bpermute(4 * (sbase + 7), incl);
    const int totB = __builtin_amdgcn_ds_bpermute(4 * (sbase + 15), incl);
    const int nsteps = ((wave_max(max(totA, totB)) + 15) + 7) & ~7;
    // Table accessors (uniform control flow: every lane executes the shuffle).
    // sb is sbase laundered once per block (asm below), so the shuffle
    // addresses are computed where they are used instead of being hoisted out
    // of the loops as long-lived registers.
    int sb = sbase * 4;  // byte address of the segment's lane 0 for ds_bpermute
    auto bp = [&](int v, int h, int k) {
      return __builtin_amdgcn_ds_bpermute(sb + 4 * (8 * h + min(k, 7)), v);
    };
    auto tG = [&](int h, int k) { return bp(Gm, h, k); };
    auto tR = [&](int h, int k) { return bp(Rm, h, k); };
    auto tH = [&](int h, int k) { return bp(Hm, h, k); };
    auto tP = [&](int h, int k) { return bp(pm, h, k); };
    auto tI = [&](int h, int k) { return __int_as_float(bp(__float_as_int(Im), h, k)); };
    auto t64 = [&](int64_t v, int h, int k) {
      const int lo = bp((int)v, h, k), hi = bp((int)(v >> 32), h, k);
      return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
    };
    auto valid = [&](int h, int k) {  // the shuffle runs in every lane whatever k is
      const int pv = tP(h, k);
      return k < Kb && pv >= 0;
    };

    // Haplotype codes per half: cur (in use), nxt (the next pair of the
    // half-stream, taken by lane l at stream row swr[h], i.e. step swr + l),
    // nk[h] = the pair held in nxt.  other[h]: bit k = pair k of the half has
    // a haplotype byte outside A/C/G/T/N or a read row under kColsMinMm
    // (segment-uniform).
    uint32_t cur[2][NW], nxt[2][NW];
    int nk[2], swr[2];
    unsigned other[2] = {0u, 0u};
    auto fetch_codes = [&](int h, int k, uint32_t (&dst)[NW]) {  // uniform: every lane of the wave calls it
      const bool ok = valid(h, k);
      const int Hk = tH(h, k);
      const int H = ok ? Hk : 0;
      const int64_t ho = t64(hom, h, k);
      uint32_t raw[NW + 1];
      int al;
      cols_load<NW>(b.hb, ok ? ho : 0, H, i0, raw, al);
      bool oth = false;
      cols_convert<NW>(raw, al, i0, H, dst, oth);
      const unsigned long long bal = __ballot(oth && ok);
      if (((bal >> sbase) & 0xFFFFull) != 0ull) other[h] |= 1u << k;
    };
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int d = 0; d < NW; ++d) cur[h][d] = 0x06060606u;
      fetch_codes(h, 0, nxt[h]);
      nk[h] = 0;
      swr[h] = valid(h, 0) ? tG(h, 0) : 0x3FFFFFFF;
    }
    // Captures: lane 15 takes half h's sum at the V row of pair kc[h]
    // (stream row cap[h], pair index capp[h], fallback flag from other[h]).
    int kc[2] = {0, 0};
    int cap[2], capp[2];
    auto load_cap = [&](int h) {
      const bool ok = valid(h, kc[h]);
      const int v = tG(h, kc[h]) + tR(h, kc[h]);
      cap[h] = ok ? v : -0x3FFFFFFF;  // stream row of the V row
      capp[h] = tP(h, kc[h]);
    };
    load_cap(0);
    load_cap(1);

    // The ring's items (row g of half th per lane) in two stages one block
    // apart, so the read bytes' HBM latency is not paid inside a block:
    // stage A locates the row and issues its byte loads, stage B (eight steps
    // later) builds the item from them and writes it.
    int kp = 0;  // stage A's cursor: the pair of half th holding this lane's item row
    RawRow praw{-1, 0, 0, 0, 0, 0, 0};
    int prole = 0;  // role | first << 4 | the row's own insertion quality << 8
    float pih = 0.f;
    // the cursor pair's table entries, cached: the shuffles run only in the
    // blocks where some lane's cursor moves (about one block in 13 on C2)
    bool kok = false, nok = false;
    int kG = 0, kR = 0, nG = 0;
    float kI = 0.f;
    int64_t kro = 0;
    auto load_cursor = [&] {
      kok = valid(th, kp);
      kG = tG(th, kp);
      kR = tR(th, kp);
      kI = tI(th, kp);
      kro = t64(rom, th, kp);
      nok = valid(th, kp + 1);
      nG = tG(th, kp + 1);
    };
    load_cursor();
    auto stage_a = [&](int base) {
      const int g = base + tk;
      const bool adv = nok && g >= nG;  // pairs span >= 35 rows: at most one advance per 8 rows
      if (__ballot(adv) != 0ull) {
        if (adv) ++kp;
        load_cursor();
      }
      const bool ok = kok;
      const int G = kG, R = kR;
      pih = kI;
      const int64_t ro = kro;
      const int r = g - G;
      int role = 0;
      if (ok && r >= 0 && r < R) role = r == R - 1 ? 3 : 2;
      else if (ok && r == R) role = 4;
      prole = role | (r == 0 ? 16 : 0);
      praw = (role == 2 || role == 3) ? load_raw(b, R, ro, r) : RawRow{-1, 0, 0, 0, 0, 0, 0};
      if (role == 2 || role == 3) prole |= (int)b.iq[ro + r] << 8;
    };
    // kp is still the cursor stage A left for this item: a hazard row sets its
    // pair's bit of other[th] in every lane of the segment (rare: one branch).
    auto stage_b = [&](int base) {
      bool hz;
      cols_put(smem_raw, (base + tk) & (kColsRing - 1), seg, th,
               cols_item(tab, praw, prole >> 8, prole & 15, (prole & 16) != 0, pih, hz));
      if (__ballot(hz) != 0ull) {  // uniform
        unsigned m = hz ? 1u << (kp + 8 * th) : 0u;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) m |= (unsigned)__shfl_xor((int)m, d, 16);
        other[0] |= m & 0xFFu;
        other[1] |= m >> 8;
      }
    };
    {  // ring prologue: rows -16..-1 are Z (slots 16..31), rows 0..7 built, rows 8..15 requested
      bool hz;
      ColsItem z = cols_item(tab, RawRow{-1, 0, 0, 0, 0, 0, 0}, 0, 0, false, 0.f, hz);
      cols_put(smem_raw, 16 + tk, seg, th, z);
      cols_put(smem_raw, 24 + tk, seg, th, z);
      stage_a(0);
      stage_b(0);
      stage_a(8);
    }

    // Lane state: the columns' X~ and I after a Z row; the E chain and the
    // lane below's X~ as if it had run Z rows.
    pf2 Xn[C], In[C];
#pragma unroll
    for (int j = 0; j < C; ++j) {
      Xn[j] = pf2{1.f, 1.f};
      In[j] = pf2{0.f, 0.f};
    }
    pf2 dn = pf2{1.f, 1.f}, xo = pf2{1.f, 1.f}, xin = pf2{1.f, 1.f};
    const uint32_t segoff = (uint32_t)seg * (kColsRing * 16u) + lds_addr(smem_raw);

    for (int t0 = 0; t0 < nsteps; t0 += 8) {
      asm volatile("" : "+v"(sb));
      // Next pair's codes: once every lane took the pair in nxt (its row swr
      // was reached by lane 15 before this block), convert the one after it.
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const bool ev = swr[h] + 16 <= t0 && nk[h] + 1 < Kb;
        if (__ballot(ev) != 0ull) {  // uniform: fetch_codes shuffles
          uint32_t tmp[NW];
          fetch_codes(h, nk[h] + 1, tmp);
          const bool vn = valid(h, nk[h] + 1);
          const int gn = tG(h, nk[h] + 1);
          if (ev) {
#pragma unroll
            for (int d = 0; d < NW; ++d) nxt[h][d] = tmp[d];
            ++nk[h];
            swr[h] = vn ? gn : 0x3FFFFFFF;
          }
        }
        if (swr[h] + 16 <= t0 && nk[h] + 1 >= Kb) swr[h] = 0x3FFFFFFF;  // last pair taken
      }
      // The ring's rows t0 + 8 .. t0 + 15 (slots of rows t0 - 24 .. t0 - 17,
      // read last in the previous block), requested one block ago; then the
      // requests for rows t0 + 16 .. t0 + 23.
      stage_b(t0 + 8);
      stage_a(t0 + 16);
      // This block's captures (lane 15 at the V row of pair kc[h]) and switches.
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const bool adv = cap[h] >= 0 && cap[h] + 15 < t0;  // lane 15 passed the V row in an earlier block
        if (__ballot(adv) != 0ull) {
          if (adv) ++kc[h];
          load_cap(h);
        }
      }
      bool capo[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) capo[h] = (other[h] >> kc[h]) & 1u;
      const int g0 = t0 - sl;  // this lane's row at the block's first step
      const bool any_cap = __ballot(sl == 15 && ((unsigned)(cap[0] - g0) < 8u || (unsigned)(cap[1] - g0) < 8u)) != 0ull;
      // steps of this block at which some lane takes its next haplotype codes
      // (lane l of segment s switches half h at step swr - t0 + l): a uniform
      // 8-bit mask, tested per step by the scalar unit only
      unsigned swmask = 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int lo = __builtin_amdgcn_readlane(swr[h], 16 * q) - t0;  // steps lo .. lo + 15
          if (lo < 8 && lo + 15 >= 0) {
            const int a = max(lo, 0), bnd = min(lo + 15, 7);
            swmask |= ((2u << bnd) - 1u) & ~((1u << a) - 1u);
          }
        }
      const uint32_t xs = (uint32_t)(g0 & (kColsRing - 1)) * 16u;
      const uint32_t capa = lds_addr(smem_raw) + kColsCapOff + seg * 64;

      auto step = [&](auto S_) {
        constexpr int S = decltype(S_)::value;
        const int g = g0 + S;
        if (swmask & (1u << S)) {  // uniform
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const bool take = g == swr[h];
#pragma unroll
            for (int d = 0; d < NW; ++d) {  // the VOP3 select: the VOP2 form issues at ~1/5 rate
              uint32_t r;
              asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(cur[h][d]), "v"(nxt[h][d]), "s"(__ballot(take)));
              cur[h][d] = r;
            }
          }
        }
        // this row's records (the barrier keeps each step's LDS reads in their
        // step: hoisted ahead, eight steps' records would hold ~190 VGPRs)
        asm volatile("" ::: "memory");
        const uint32_t pa = ((xs + (uint32_t)(S * 16)) & (uint32_t)((kColsRing - 1) * 16)) + segoff;
        typedef float f4 __attribute__((ext_vector_type(4)));
        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
        auto ld4 = [&](int chunk) {
          return *reinterpret_cast<const __attribute__((address_space(3))) f4*>((uintptr_t)(pa + chunk * kColsChunkBytes));
        };
        const f4 r0 = ld4(0), r1 = ld4(1), r2 = ld4(2), r3 = ld4(3);
        const u4 cr = *reinterpret_cast<const __attribute__((address_space(3))) u4*>((uintptr_t)(pa + 4 * kColsChunkBytes));
        const pf2 z1 = *reinterpret_cast<const __attribute__((address_space(3))) pf2*>((uintptr_t)(pa + 5 * kColsChunkBytes));
        const pf2 z2 = *reinterpret_cast<const __attribute__((address_space(3))) pf2*>((uintptr_t)(pa + 5 * kColsChunkBytes + 8));
        const pf2 e1 = pf2{r0.x, r0.y}, e3 = pf2{r0.z, r0.w}, cb = pf2{r1.x, r1.y}, yy = pf2{r1.z, r1.w};
        const pf2 ca = pf2{r2.x, r2.y}, mx = pf2{r3.x, r3.y}, xx = pf2{r3.z, r3.w};
        // the lane below's E into column l*C + 1 (lane 0: 1 on Z rows, else
        // 0) and its X~(g, l*C) for the next row (lane 0: X~(g, 0) = 1 after a Z row)
        pf2 din, xnx;
        din.x = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(z1.x), __float_as_int(dn.x), kDppRowShr1, 0xF, 0xF, false));
        din.y = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(z1.y), __float_as_int(dn.y), kDppRowShr1, 0xF, 0xF, false));
        xnx.x = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(z2.x), __float_as_int(xo.x), kDppRowShr1, 0xF, 0xF, false));
        xnx.y = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(z2.y), __float_as_int(xo.y), kDppRowShr1, 0xF, 0xF, false));
        const pf2 xcur = xin;
        xin = xnx;
        uint32_t mA = 0, mB = 0;
        // prior(j) after `dep`: every per-column input is tied to the previous
        // column's E by an empty asm, so the columns run in order.  Left free,
        // the scheduler hoists all C columns' I * xx, priors and M products to
        // the top of the step (~6 extra VGPRs per column: 256 VGPRs and spills
        // at C = 16).
        auto prior = [&](int j, const pf2 dep) {
          if ((j & 3) == 0) {
            mA = __builtin_amdgcn_perm(cr.z, cr.x, cur[0][j >> 2]);
            mB = __builtin_amdgcn_perm(cr.w, cr.y, cur[1][j >> 2]);
          }
          int a, c;
          asm volatile("v_bfe_i32 %0, %2, %3, 1\n\tv_bfe_i32 %1, %4, %3, 1"
                       : "=&v"(a), "=&v"(c)
                       : "v"(mA), "i"(8 * (j & 3)), "v"(mB), "v"(dep));
          return pf2{sel_v((uint32_t)a, e1.x, e3.x), sel_v((uint32_t)c, e1.y, e3.y)};
        };
        pf2 Mn = xcur * prior(0, xcur);
        pf2 E = din, Mp = pf2{0.f, 0.f}, Ep = pf2{0.f, 0.f};
#pragma unroll
        for (int j = 0; j < C; ++j) {
          const pf2 M = Mn;
          if (j > 0) E = __builtin_elementwise_fma(Ep, yy, Mp);
          pf2 I = In[j], Xo = Xn[j];
          asm volatile("" : "+v"(I), "+v"(Xo) : "v"(E));
          if (j + 1 < C) Mn = Xo * prior(j + 1, E);
          pf2 xn = __builtin_elementwise_fma(E, cb, __builtin_elementwise_fma(I, ca, M));
          pf2 in = __builtin_elementwise_fma(M, mx, I * xx);
          asm volatile("" : "+v"(xn), "+v"(in));  // and its outputs leave it in order
          Xn[j] = xn;
          In[j] = in;
          Mp = M;
          Ep = E;
        }
        dn = __builtin_elementwise_fma(Ep, yy, Mp);
        xo = Xn[C - 1];
        // lane 15's E entering column 16 C + 1, kept per step in LDS (EXEC
        // narrowed to the lanes 15 inside the statement, no branch): at a V row
        // it is the half's sum, taken after the block
        uint64_t keep;
        const uint32_t cpa = capa + 0u;  // a local: asm operands of a generic lambda cannot name captured consts
        const pf2 dnv = dn;
        asm volatile(
            "s_mov_b64 %0, exec\n\t"
            "s_mov_b64 exec, %3\n\t"
            "ds_write_b64 %1, %2 offset:%4\n\t"
            "s_mov_b64 exec, %0"
            : "=&s"(keep)
            : "v"(cpa), "v"(dnv), "s"(kTopLanes), "i"(8 * S)
            : "memory");
      };
      [&]<int... S>(std::integer_sequence<int, S...>) {
        (step(std::integral_constant<int, S>{}), ...);
      }(std::make_integer_sequence<int, 8>{});
      if (any_cap) {
        // lane 15 at a V row: the E entering column 16 C + 1 is the half's sum
#pragma unroll
        for (int h = 0; h < 2; ++h)
          if (sl == 15 && (unsigned)(cap[h] - g0) < 8u) {
            const pf2 v = *reinterpret_cast<const pf2*>(smem_raw + kColsCapOff + seg * 64 + 8 * (cap[h] - g0));
            const float acc = h ? v.y : v.x;
            const int p = capp[h];
            if (capo[h]) {
              const unsigned long long k = atomicAdd(fb_count, 1ull);
              fb_list[k] = p;
              out[p] = __builtin_nan("");
            } else if (use_rescue && acc < thr) {
              const unsigned long long k = atomicAdd(rescue_count, 1ull);
              rescue_list[k] = p;
              out[p] = __builtin_nan("");
            } else {
              out[p] = (double)(log10f(acc) - tab.log10_init);
            }
          }
      }
    }
  }
}

// ---- phmm5 and phmm6: the same kernel with ONE pair stream per register
// (constants and ring layout here, the body and the two kernels below).
// phmm4 is pinned at 2 waves per SIMD by its registers (195 .. 249 VGPRs) and
// a packed f32 op issues in the time of its two scalar halves, so packing buys
// no issue rate and costs the occupancy.  Here a segment carries one stream:
// the per-lane state is 2 C floats, every v_pk_* is the scalar op on the same
// operands in the same order (bitwise the same results), all 16 lanes of the
// segment table hold pairs (K <= 16), and a block is 16 steps (one ring item
// per lane and block) run as two passes over the 8-step unrolled body.
// LDS per wave: a 48-row ring per segment (rows t0 - 15 .. t0 + 31 live at
// once) of five 8-byte chunks per row: {e1, e3}, {b, yy}, {a, -}, {mx, xx},
// {Tlo, Thi} with the Z flag in Thi's byte 3 (no column code selects it: codes
// end at 6); `a` is read alone (ds_read_b32, 8 bytes apart per lane: 0.29
// bank-conflict cycles per LDS cycle, where the 8-byte reads have none;
// reading the whole chunk, or moving the Z flag into it, spilled in phmm5 at
// C = 19: DESIGN §4.1i); chunk-major, then segment, then slot, so a segment's 16 lanes
// read 128 contiguous bytes (up to the wrap).  7,680 B ring + 256 B capture +
// 1,536 B tables = 9,472 B: 16 waves fit the CU's 160 KB.
constexpr int kCols1Ring = 48;
constexpr int kCols1Chunks = 5;
constexpr int kCols1ChunkBytes = kCols1Ring * 4 * 8;
constexpr int kCols1CapOff = kCols1Chunks * kCols1ChunkBytes;  // lane 15's E per step of a block (4 x 16 floats)
constexpr int kCols1TabOff = kCols1CapOff + 4 * 16 * 4;
constexpr int kCols1Lds = kCols1TabOff + 3 * 128 * 4;
constexpr int kCols1MaxK = 16;  // pairs per stream: one per lane of the segment table
// Waves per SIMD phmm5 is compiled for: what its registers allow without
// scratch (tools/kernel_resources.py: 127 VGPRs at C = 11 .. 163 at C = 19 with
// the staged row packed, DESIGN §4.1j, so every class takes 3; phmm6 has its
// own table, cols6_waves below).
__host__ __device__ constexpr int cols1_waves(int C) { return 3; }
static_assert(kCols1Lds <= 10240, "16 waves per CU");

typedef uint32_t pu2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void cols1_put(unsigned char* smem, int slot, int seg, const ColsItem& c) {
  unsigned char* const p = smem + (seg * kCols1Ring + slot) * 8;
  *reinterpret_cast<pf2*>(p) = pf2{c.e1, c.e3};
  *reinterpret_cast<pf2*>(p + kCols1ChunkBytes) = pf2{c.b, c.yy};
  *reinterpret_cast<pf2*>(p + 2 * kCols1ChunkBytes) = pf2{c.a, 0.f};
  *reinterpret_cast<pf2*>(p + 3 * kCols1ChunkBytes) = pf2{c.mx, c.xx};
  *reinterpret_cast<pu2*>(p + 4 * kCols1ChunkBytes) = pu2{c.tlo, c.thi | (c.z != 0.f ? 0x01000000u : 0u)};
}

// ---- The single-stream body, shared by phmm5_kernel and phmm6_kernel (DESIGN
// §4.1h).  cols1_stream<C, Feed> (below) runs a wave's four streams: the
// segment-table accessors, the code fetch, the capture, the ring's two stages
// and prologue, the 16-step block with the step arithmetic, and the result
// write exist once.  What a kernel adds is its Feed, the way pairs reach the
// streams: which lane of the segment table holds pair k (slot), whether pair
// k is there (valid, in cols1_stream), when the next pair's codes may be
// converted, and when the streams end.
constexpr int kNever = 0x3FFFFFFF;  // a stream row that never comes

// A staged row as it waits between stage A and the next block's stage B: the
// seven bytes of a RawRow and the row's own insertion quality in two dwords
// (own = rb | bq << 8 | dq << 16 | gq << 24, below = niq | ndq << 8 | ngq << 16 |
// own iq << 24) instead of eight registers held across the pass loop.  Every
// consumer masks the qualities with 127 and reads rb as an unsigned char, so
// the unpacked row builds the same item bit for bit.  A row that is no read
// row (role 0 or 4) is never unpacked into row_params: its words are 0.
struct PackedRow {
  uint32_t own, below;
};
__device__ __forceinline__ PackedRow cols1_pack(const RawRow& r, int oiq) {
  return PackedRow{(uint32_t)(r.rb & 255) | (uint32_t)(r.bq & 255) << 8 | (uint32_t)(r.dq & 255) << 16 |
                       (uint32_t)r.gq << 24,
                   (uint32_t)(r.niq & 255) | (uint32_t)(r.ndq & 255) << 8 | (uint32_t)(r.ngq & 255) << 16 |
                       (uint32_t)oiq << 24};
}
__device__ __forceinline__ RawRow cols1_unpack(const PackedRow& w) {
  return RawRow{(int)(w.own & 255u),         (int)((w.own >> 8) & 255u),    (int)((w.own >> 16) & 255u), (int)(w.own >> 24),
                (int)(w.below & 255u),       (int)((w.below >> 8) & 255u),  (int)((w.below >> 16) & 255u)};
}
__device__ __forceinline__ int cols1_own_iq(const PackedRow& w) { return (int)(w.below >> 24); }

// One entry of a segment table: lane sl of a segment holds the pair of slot
// sl of that segment's stream, G = the pair's first stream row.
struct Cols1Seg {
  int pm, Rm, Hm, Gm;
  int64_t rom;
};

// The match tables copied to LDS for the ring items (every lane of the wave calls it).
__device__ __forceinline__ PhmmTables<float> cols1_tables(const PhmmTables<float>& gtab) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  PhmmTables<float> tab = gtab;
  float* const t = reinterpret_cast<float*>(smem_raw + kCols1TabOff);
  for (int i = threadIdx.x; i < 128; i += 64) {
    t[i] = gtab.ph2pr[i];
    t[128 + i] = gtab.dmatch[i];
    t[256 + i] = gtab.dmis[i];
  }
  tab.ph2pr = t;
  tab.dmatch = t + 128;
  tab.dmis = t + 256;
  return tab;
}

// phmm5's feed: a batch.  The table is filled before the streams start: pair k
// of a stream in lane k, Kb pairs at most (k past them reads lane 15, which
// `valid` rejects), and the streams end after nsteps steps.
struct Cols1Batch {
  static constexpr bool kQueue = false;
  int Kb, nsteps;
  static __device__ __forceinline__ int slot(int k) { return min(k, 15); }
  static __device__ __forceinline__ int bit(int k) { return k; }
  __device__ __forceinline__ bool more(int t0) const { return t0 < nsteps; }
  __device__ __forceinline__ bool done(int) const { return false; }
};

// ---- phmm6's feed: CONTINUOUS streams fed from a per-class queue (DESIGN
// §4.1g).  A class launch is one round of the chip (CUs x 4 SIMDs x
// cols6_waves(C) waves, each a workgroup), and a wave's four streams run until the class is
// exhausted: no batches, so no drain, no ring prologue and no segment-table
// scan between pairs, no one-pair tail, and no workgroups that find nothing.
//   * The class's pairs order[bounds[cls] .. bounds[cls + 1]) are handed out
//     in that order (longest haplotypes first) by a returning device-scope
//     atomicAdd on the class's head word.  Lane 0 asks for one pair for every
//     stream of the wave that is within kCols6Ahead rows of its end, at a
//     block top, and the answer is read at the next block top: its latency
//     never stands in front of a step.  The head words are zeroed with the
//     rescue and fallback counts.
//   * The segment table is circular: pair number n of a stream lives in lane
//     n mod 16 of the segment.  A stream holds at most 8 pairs that lane 15
//     has not captured yet (in practice 2), so the slot that pair n takes was
//     left by pair n - 16 long before: all three cursors (kp, nk, kc) are past it.
//   * A new pair starts at stream row G = max(end of the previous pair, first
//     row stage A has not located yet), so the order of arrival never matters
//     for correctness: a pair that comes late is preceded by Z rows.  In the
//     steady state G is the previous pair's G + R + 2.
//   * kColsMinR: consecutive pairs still start >= R + 2 >= 35 rows apart, so
//     stage A advances at most once per 16 rows, and between the block top
//     where lane 15 has taken pair n's codes (<= G(n) + 31) and pair n + 1's
//     first row there is a block top at which pair n + 1 is in the table
//     (it arrives >= 32 rows before its G) and its codes are converted.
//   * When the queue is empty a stream runs out its pairs and feeds Z rows;
//     the wave ends at the block top after its last capture.
// The streams run in cols1_stream; this is its feed.
constexpr int kCols6Lds = kCols1Lds;
// Waves per SIMD of class C's launch: the kernel is compiled for that bound and
// the grid is CUs x 4 x cols6_waves(C) one-wave workgroups.  C <= 17 fit a
// fourth wave (<= 128 VGPRs, no scratch, under bound 4; C = 19 is 5 dwords
// short), but the fourth wave bought nothing measurable on C2 (DESIGN §4.1j:
// `C <= 14 ? 4 : 3` and `C <= 17 ? 4 : 3` ran within +-0.4% of this table; at
// 3 waves the step already issues at the rate §4.1e measured for 8), so every
// class stays at 3.
__host__ __device__ constexpr int cols6_waves(int C) { return 3; }
constexpr int kCols6Ahead = 48;  // rows located ahead of stage A below which a stream asks for its next pair
constexpr bool cols6_lds_fits(int C) { return cols6_waves(C) >= 4 ? kCols6Lds <= 10240 : kCols6Lds <= 13653; }
static_assert(cols6_lds_fits(11) && cols6_lds_fits(12) && cols6_lds_fits(13) && cols6_lds_fits(14) &&
                  cols6_lds_fits(15) && cols6_lds_fits(16) && cols6_lds_fits(17) && cols6_lds_fits(19),
              "16 waves per CU share 163,840 B at 4 per SIMD, 12 at 3");

struct Cols1Queue {
  static constexpr bool kQueue = true;
  const int32_t* order;  // the class's pairs
  long long count;
  unsigned long long* qhead;
  // pend = the streams with a request in flight (wave-uniform), qv = lane 0's
  // answer: the first position of the class handed to this request (its low
  // 32 bits: a class has fewer than 2^31 pairs and every stream overshoots
  // the end at most once).
  unsigned pend;
  uint32_t qv;
  // Stream state (the same in every lane of a segment): nq = pairs taken so
  // far (pair numbers 0 .. nq - 1 are in the table or done), gend = the stream
  // row after the last taken pair's Z row, closed = the queue had no pair left
  // for this stream.
  int nq = 0, gend = 0;
  bool closed = false;
  static __device__ __forceinline__ int slot(int k) { return k & 15; }
  static __device__ __forceinline__ int bit(int k) { return k & 15; }
  __device__ __forceinline__ bool more(int) const { return true; }
  // every stream closed and its last pair captured: the wave is done
  __device__ __forceinline__ bool done(int kc) const { return __ballot(!closed || kc < nq) == 0ull; }
  // The answer to the request in flight (uniform: every lane calls it): the
  // streams of `pend`, in stream order, take positions qv, qv + 1, ..; a
  // position past the class closes the stream.  The pair starts at row
  // max(gend, gmin), gmin = the first row stage A has not located, in slot
  // nq mod 16 of the table, whose `other` bit it clears.
  __device__ __forceinline__ void complete(int gmin, const PhmmDevBatch& b, Cols1Seg& tb, unsigned& other) {
    const int seg = threadIdx.x >> 4, sl = threadIdx.x & 15;
    const long long base = (long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)qv);
    const bool mine = (pend >> seg) & 1u;
    const long long idx = base + __popc(pend & ((1u << seg) - 1u));
    const bool got = mine && idx < count;
    if (mine && !got) closed = true;
    if (got) {
      const int p = order[idx];
      const int ri = b.pair_read[p], hi = b.pair_hap[p];
      const int R = b.read_len[ri], H = b.hap_len[hi];
      const int G = max(gend, gmin);
      if (sl == (nq & 15)) {
        tb.pm = p;
        tb.Rm = R;
        tb.Hm = H;
        tb.rom = b.read_off[ri];
        tb.Gm = G;
      }
      other &= ~(1u << (nq & 15));
      gend = G + R + 2;  // rows 1..R, V, Z
      ++nq;
    }
    pend = 0u;
  }
  // One request, at a block top, for every stream that has fewer than
  // kCols6Ahead located rows left ahead of stage A (kc: the capture cursor).
  __device__ __forceinline__ void request(int t0, int kc) {
    const bool need = !closed && gend < t0 + 32 + kCols6Ahead && nq - kc < 8;
    const unsigned long long bal = __ballot(need && (threadIdx.x & 15) == 0);
    if (bal != 0ull) {  // uniform
      pend = (unsigned)((bal & 1ull) | ((bal >> 15) & 2ull) | ((bal >> 30) & 4ull) | ((bal >> 45) & 8ull));
      qv = 0u;
      if (threadIdx.x == 0) qv = (uint32_t)atomicAdd(qhead, (unsigned long long)__popc(pend));
    }
  }
};

// The streams of one wave: tb = this lane's entry of its segment's table (a
// batch's, or empty for a queue, which fills it), tab = cols1_tables().
template <int C, class Feed>
__device__ __forceinline__ void cols1_stream(const PhmmDevBatch& b, const PhmmTables<float>& tab, Cols1Seg tb,
                                             Feed feed, double* __restrict__ out,
                                             int32_t* __restrict__ rescue_list,
                                             unsigned long long* __restrict__ rescue_count, const float thr,
                                             const int use_rescue, int32_t* __restrict__ fb_list,
                                             unsigned long long* __restrict__ fb_count) {
  constexpr int NW = (C + 3) / 4;  // code dwords
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x;
  const int seg = lane >> 4;
  const int sl = lane & 15;  // lane of the segment, and its slot of the segment table
  const int sbase = lane & 48;
  const int i0 = sl * C;  // first haplotype index of this lane's columns
  int sb = sbase * 4;  // laundered once per block, as in phmm4
  auto bp = [&](int v, int k) { return __builtin_amdgcn_ds_bpermute(sb + 4 * Feed::slot(k), v); };
  auto tG = [&](int k) { return bp(tb.Gm, k); };
  auto tR = [&](int k) { return bp(tb.Rm, k); };
  auto tH = [&](int k) { return bp(tb.Hm, k); };
  auto tP = [&](int k) { return bp(tb.pm, k); };
  auto t64 = [&](int64_t v, int k) {
    const int lo = bp((int)v, k), hi = bp((int)(v >> 32), k);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
  };
  auto valid = [&](int k) {
    if constexpr (Feed::kQueue) {
      return k >= 0 && k < feed.nq;
    } else {  // the shuffle runs in every lane whatever k is
      const int pv = tP(k);
      return k < feed.Kb && pv >= 0;
    }
  };

  // Haplotype codes: cur (in use), nxt (the stream's next pair, taken by lane
  // l at stream row swr, i.e. step swr + l; kNever: every lane has taken it),
  // nk = the pair held in nxt.  other: bit Feed::bit(k) = pair k has a
  // haplotype byte outside A/C/G/T/N, or a read row under kColsMinMm (stage B).
  uint32_t cur[NW], nxt[NW];
  int nk = -1, swr = kNever;
  unsigned other = 0u;
  auto fetch_codes = [&](int k, uint32_t (&dst)[NW]) {  // uniform: every lane of the wave calls it
    const bool ok = valid(k);
    const int Hk = tH(k);
    const int H = ok ? Hk : 0;
    // the haplotype's offset is not held in the table: it is read again from
    // the pair here, once per pair and stream
    const int pk = tP(k);
    const int64_t ho = ok ? b.hap_off[b.pair_hap[pk]] : 0;
    uint32_t raw[NW + 1];
    int al;
    cols_load<NW>(b.hb, ho, H, i0, raw, al);
    bool oth = false;
    cols_convert<NW>(raw, al, i0, H, dst, oth);
    const unsigned long long bal = __ballot(oth && ok);
    if (((bal >> sbase) & 0xFFFFull) != 0ull) other |= 1u << Feed::bit(k);
  };
#pragma unroll
  for (int d = 0; d < NW; ++d) cur[d] = nxt[d] = 0x06060606u;
  // Capture: lane 15 takes the sum at the V row of pair kc.
  int kc = 0, cap, capp;
  auto load_cap = [&] {
    const bool ok = valid(kc);
    const int v = tG(kc) + tR(kc);
    cap = ok ? v : -kNever;  // stream row of the V row
    capp = tP(kc);
  };

  // The ring's items (row base + sl per lane) in two stages one block apart.
  int kp = 0;  // stage A's cursor: the pair holding this lane's item row
  PackedRow praw{0u, 0u};  // the row's bytes and its own insertion quality (cols1_pack)
  int prole = 0;  // role | first << 4
  bool kok = false, nok = false;
  int kG = 0, kR = 0, nG = 0;
  int64_t kro = 0;
  auto load_cursor = [&] {
    kok = valid(kp);
    kG = tG(kp);
    kR = tR(kp);
    kro = t64(tb.rom, kp);
    nok = valid(kp + 1);
    nG = tG(kp + 1);
  };
  auto stage_a = [&](int base) {
    const int g = base + sl;
    const bool adv = nok && g >= nG;  // pairs start >= 35 rows apart: at most one advance per 16 rows
    if (__ballot(adv) != 0ull) {
      if (adv) ++kp;
      load_cursor();
    }
    const int r = g - kG;
    int role = 0;
    if (kok && r >= 0 && r < kR) role = r == kR - 1 ? 3 : 2;
    else if (kok && r == kR) role = 4;
    prole = role | (r == 0 ? 16 : 0);
    praw = (role == 2 || role == 3) ? cols1_pack(load_raw(b, kR, kro, r), b.iq[kro + r]) : PackedRow{0u, 0u};
  };
  // kp is still the cursor stage A left for this item.  A pair's first row
  // takes its scale 2^120 / H from the table here, once per pair and stream,
  // so no lane holds it across the pass loop; a hazard row sets its pair's bit
  // of `other` in every lane of the segment (rare: one branch each).
  auto stage_b = [&](int base) {  // base >= 0
    bool hz;
    const bool first = (prole & 16) != 0;
    float ih = 0.f;
    if (__ballot(first) != 0ull) ih = tab.init_const / (float)tH(kp);  // uniform: tH shuffles
    cols1_put(smem_raw, (int)((unsigned)(base + sl) % (unsigned)kCols1Ring), seg,
              cols_item(tab, cols1_unpack(praw), cols1_own_iq(praw), prole & 15, first, ih, hz));
    if (__ballot(hz) != 0ull) {  // uniform
      unsigned m = hz ? 1u << Feed::bit(kp) : 0u;
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) m |= (unsigned)__shfl_xor((int)m, d, 16);
      other |= m;
    }
  };
  // The streams' first pairs start at row 0: a queue's come with the answer
  // to the wave's first request, a batch's are in the table and their codes
  // are converted here.
  if constexpr (Feed::kQueue) {
    feed.complete(0, b, tb, other);
  } else {
    fetch_codes(0, nxt);
    nk = 0;
    swr = valid(0) ? tG(0) : kNever;
  }
  load_cursor();
  load_cap();
  {  // ring prologue: rows -16..-1 are Z (slots 32..47), rows 0..15 built, rows 16..31 requested
    bool hz;
    cols1_put(smem_raw, 32 + sl, seg, cols_item(tab, RawRow{-1, 0, 0, 0, 0, 0, 0}, 0, 0, false, 0.f, hz));
    stage_a(0);
    stage_b(0);
    stage_a(16);
  }

  float Xn[C], In[C];
#pragma unroll
  for (int j = 0; j < C; ++j) {
    Xn[j] = 1.f;
    In[j] = 0.f;
  }
  float dn = 1.f, xo = 1.f, xin = 1.f;
  const uint32_t segoff = (uint32_t)seg * (kCols1Ring * 8u) + lds_addr(smem_raw);

  for (int t0 = 0; feed.more(t0); t0 += 16) {
    asm volatile("" : "+v"(sb));
    // The queue.  The pairs asked for one block ago start at the first row
    // stage A has not located (t0 + 32) or after the stream's last pair; then
    // the next request.
    if constexpr (Feed::kQueue) {
      if (feed.pend != 0u) {  // uniform
        feed.complete(t0 + 32, b, tb, other);
        load_cursor();
        load_cap();
      }
      feed.request(t0, kc);
    }
    // Next pair's codes: once every lane took the pair in nxt (lane 15 reached
    // row swr before this block), convert the one after it: a batch's at once
    // (the block starts at most 31 rows after swr and the next pair at swr +
    // R + 2 >= swr + 35), a queue's as soon as it is in the table.
    {
      bool ev;
      if constexpr (Feed::kQueue) {
        if (swr != kNever && swr + 16 <= t0) swr = kNever;
        ev = swr == kNever && nk + 1 < feed.nq;
      } else {
        ev = swr + 16 <= t0 && nk + 1 < feed.Kb;
      }
      if (__ballot(ev) != 0ull) {  // uniform: fetch_codes shuffles
        uint32_t tmp[NW];
        fetch_codes(nk + 1, tmp);
        const bool vn = valid(nk + 1);
        const int gn = tG(nk + 1);
        if (ev) {
#pragma unroll
          for (int d = 0; d < NW; ++d) nxt[d] = tmp[d];
          ++nk;
          swr = vn ? gn : kNever;
        }
      }
      if constexpr (!Feed::kQueue)
        if (swr + 16 <= t0 && nk + 1 >= feed.Kb) swr = kNever;  // last pair taken
    }
    // The ring's rows t0 + 16 .. t0 + 31 (slots of rows t0 - 32 .. t0 - 17,
    // read last in the previous block), requested one block ago; then the
    // requests for rows t0 + 32 .. t0 + 47.
    stage_b(t0 + 16);
    stage_a(t0 + 32);
    {
      const bool adv = cap >= 0 && cap + 15 < t0;  // lane 15 passed the V row in an earlier block
      if (__ballot(adv) != 0ull) {
        if (adv) ++kc;
        load_cap();
      }
    }
    if (feed.done(kc)) break;
    const bool capo = (other >> Feed::bit(kc)) & 1u;
    const int gb = t0 - sl;  // this lane's row at the block's first step
    const bool any_cap = __ballot(sl == 15 && (unsigned)(cap - gb) < 16u) != 0ull;
    // steps of this block at which some lane takes its next haplotype codes
    // (lane l of segment q switches at step swr - t0 + l): a uniform 16-bit mask
    unsigned swmask = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int lo = __builtin_amdgcn_readlane(swr, 16 * q) - t0;  // steps lo .. lo + 15
      if (lo < 16 && lo + 15 >= 0) {
        const int a = max(lo, 0), bnd = min(lo + 15, 15);
        swmask |= ((2u << bnd) - 1u) & ~((1u << a) - 1u);
      }
    }
    uint32_t xs = ((uint32_t)(gb + kCols1Ring) % (uint32_t)kCols1Ring) * 8u;  // gb >= -15
    uint32_t capa = lds_addr(smem_raw) + kCols1CapOff + seg * 64;
    int g0 = gb;

#pragma nounroll
    for (int pass = 0; pass < 2; ++pass) {
      auto step = [&](auto S_) {
        constexpr int S = decltype(S_)::value;
        const int g = g0 + S;
        if (swmask & (1u << S)) {  // uniform
          const bool take = g == swr;
#pragma unroll
          for (int d = 0; d < NW; ++d) {
            uint32_t r;
            asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(cur[d]), "v"(nxt[d]), "s"(__ballot(take)));
            cur[d] = r;
          }
        }
        asm volatile("" ::: "memory");
        const uint32_t a0 = xs + (uint32_t)(S * 8);  // < 2 * 48 * 8: one subtraction wraps
        const uint32_t pa = min(a0, a0 - (uint32_t)(kCols1Ring * 8)) + segoff;
        auto ld2 = [&](int chunk) {
          return *reinterpret_cast<const __attribute__((address_space(3))) pf2*>((uintptr_t)(pa + chunk * kCols1ChunkBytes));
        };
        const pf2 r0 = ld2(0), r1 = ld2(1), r3 = ld2(3);
        const float ca = *reinterpret_cast<const __attribute__((address_space(3))) float*>((uintptr_t)(pa + 2 * kCols1ChunkBytes));
        const pu2 cr = *reinterpret_cast<const __attribute__((address_space(3))) pu2*>((uintptr_t)(pa + 4 * kCols1ChunkBytes));
        const float e1 = r0.x, e3 = r0.y, cb = r1.x, yy = r1.y, mx = r3.x, xx = r3.y;
        const float z = (float)(cr.y >> 24);  // v_cvt_f32_ubyte3: 1 on Z rows
        // the lane below's E into column l*C + 1 (lane 0: 1 on Z rows, else
        // 0) and its X~(g, l*C) for the next row (lane 0: X~(g, 0) = 1 after a Z row)
        const float din = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(z), __float_as_int(dn), kDppRowShr1, 0xF, 0xF, false));
        const float xnx = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(z), __float_as_int(xo), kDppRowShr1, 0xF, 0xF, false));
        const float xcur = xin;
        xin = xnx;
        uint32_t mA = 0;
        auto prior = [&](int j, const float dep) {  // tied to the previous column's E, as in phmm4
          if ((j & 3) == 0) mA = __builtin_amdgcn_perm(cr.y, cr.x, cur[j >> 2]);
          int a;
          asm volatile("v_bfe_i32 %0, %1, %2, 1" : "=v"(a) : "v"(mA), "i"(8 * (j & 3)), "v"(dep));
          return sel_v((uint32_t)a, e1, e3);
        };
        float Mn = xcur * prior(0, xcur);
        float E = din, Mp = 0.f, Ep = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) {
          const float M = Mn;
          if (j > 0) E = __builtin_fmaf(Ep, yy, Mp);
          float I = In[j], Xo = Xn[j];
          asm volatile("" : "+v"(I), "+v"(Xo) : "v"(E));
          if (j + 1 < C) Mn = Xo * prior(j + 1, E);
          float xn = __builtin_fmaf(E, cb, __builtin_fmaf(I, ca, M));
          float in = __builtin_fmaf(M, mx, I * xx);
          asm volatile("" : "+v"(xn), "+v"(in));
          Xn[j] = xn;
          In[j] = in;
          Mp = M;
          Ep = E;
        }
        dn = __builtin_fmaf(Ep, yy, Mp);
        xo = Xn[C - 1];
        // lane 15's E entering column 16 C + 1, kept per step in LDS: at a V
        // row it is the stream's sum, taken after the block
        uint64_t keep;
        const uint32_t cpa = capa + 0u;
        const float dnv = dn;
        asm volatile(
            "s_mov_b64 %0, exec\n\t"
            "s_mov_b64 exec, %3\n\t"
            "ds_write_b32 %1, %2 offset:%4\n\t"
            "s_mov_b64 exec, %0"
            : "=&s"(keep)
            : "v"(cpa), "v"(dnv), "s"(kTopLanes), "i"(4 * S)
            : "memory");
      };
      [&]<int... S>(std::integer_sequence<int, S...>) {
        (step(std::integral_constant<int, S>{}), ...);
      }(std::make_integer_sequence<int, 8>{});
      g0 += 8;
      swmask >>= 8;
      capa += 32;
      xs += 64;
      xs = min(xs, xs - (uint32_t)(kCols1Ring * 8));
    }
    if (any_cap) {
      // lane 15 at a V row: the E entering column 16 C + 1 is the stream's sum
      if (sl == 15 && (unsigned)(cap - gb) < 16u) {
        const float acc = *reinterpret_cast<const float*>(smem_raw + kCols1CapOff + seg * 64 + 4 * (cap - gb));
        const int p = capp;
        if (capo) {
          const unsigned long long k = atomicAdd(fb_count, 1ull);
          fb_list[k] = p;
          out[p] = __builtin_nan("");
        } else if (use_rescue && acc < thr) {
          const unsigned long long k = atomicAdd(rescue_count, 1ull);
          rescue_list[k] = p;
          out[p] = __builtin_nan("");
        } else {
          out[p] = (double)(log10f(acc) - tab.log10_init);
        }
      }
    }
  }
}

// phmm5: batches.  A workgroup runs batch after batch: 4 streams per wave, K
// pairs each, except the range's last tail_pairs (shortest haplotypes), one
// pair per stream.  Every batch fills its segment tables and pays the ring
// prologue and the 15-step drain.
template <int C>
__global__ __launch_bounds__(64, cols1_waves(C)) void phmm5_kernel(
    const PhmmDevBatch b, const int32_t* __restrict__ order, const int64_t* __restrict__ bounds, const int cls,
    const int K, const int tail_pairs, const PhmmTables<float> gtab, double* __restrict__ out,
    int32_t* __restrict__ rescue_list, unsigned long long* __restrict__ rescue_count, const float thr,
    const int use_rescue, int32_t* __restrict__ fb_list, unsigned long long* __restrict__ fb_count) {
  const int lane = threadIdx.x;
  const int seg = lane >> 4;
  const int sl = lane & 15;
  const int sbase = lane & 48;
  const int64_t cbeg = bounds[cls];
  const long long count = bounds[cls + 1] - cbeg;
  order += cbeg;
  const PhmmTables<float> tab = cols1_tables(gtab);
  const long long tailn = count < (long long)tail_pairs ? count : (long long)tail_pairs;
  const long long headn = count - tailn;
  const long long per = 4LL * K;
  const long long nb_head = (headn + per - 1) / per;
  const long long nbatch = nb_head + (tailn + 3) / 4;

  for (long long w = blockIdx.x; w < nbatch; w += gridDim.x) {
    const bool head = w < nb_head;
    const int Kb = head ? K : 1;
    const long long bstart = head ? w * per : headn + (w - nb_head) * 4;
    const long long bend = head ? min(headn, bstart + per) : min(count, bstart + 4);
    // Segment table: lane sl holds pair sl of the segment's stream (stream seg
    // of the batch takes every 4th pair).
    const long long idx = bstart + seg + 4LL * sl;
    Cols1Seg tb{(sl < Kb && idx < bend) ? order[idx] : -1, 0, 0, 0, 0};
    if (tb.pm >= 0) {
      const int ri = b.pair_read[tb.pm], hi = b.pair_hap[tb.pm];
      tb.Rm = b.read_len[ri];
      tb.Hm = b.hap_len[hi];
      tb.rom = b.read_off[ri];
    }
    const int len = tb.pm >= 0 ? tb.Rm + 2 : 0;  // rows 1..R, V, Z
    int incl = len;
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
      const int v = __shfl_up(incl, d, 16);
      if (sl >= d) incl += v;
    }
    tb.Gm = incl - len;  // first stream row of the pair
    const int tot = __builtin_amdgcn_ds_bpermute(4 * (sbase + 15), incl);
    const int nsteps = ((wave_max(tot) + 15) + 15) & ~15;
    cols1_stream<C>(b, tab, tb, Cols1Batch{Kb, nsteps}, out, rescue_list, rescue_count, thr, use_rescue, fb_list,
                    fb_count);
  }
}

// phmm6: one persistent wave per workgroup, its streams fed by Cols1Queue.
template <int C>
__global__ __launch_bounds__(64, cols6_waves(C)) void phmm6_kernel(
    const PhmmDevBatch b, const int32_t* __restrict__ order, const int64_t* __restrict__ bounds, const int cls,
    const PhmmTables<float> gtab, double* __restrict__ out, int32_t* __restrict__ rescue_list,
    unsigned long long* __restrict__ rescue_count, const float thr, const int use_rescue,
    int32_t* __restrict__ fb_list, unsigned long long* __restrict__ fb_count,
    unsigned long long* __restrict__ qhead) {
  const int64_t cbeg = bounds[cls];
  const long long count = bounds[cls + 1] - cbeg;
  // The wave's first dequeue: one pair per stream.
  uint32_t qv = 0u;
  if (threadIdx.x == 0) qv = (uint32_t)atomicAdd(qhead, 4ull);
  // a wave that finds its class exhausted leaves before it touches LDS
  if ((long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)qv) >= count) return;
  const PhmmTables<float> tab = cols1_tables(gtab);
  // The segment table starts empty: lane sl will hold the stream's pair number n with n mod 16 = sl.
  cols1_stream<C>(b, tab, Cols1Seg{-1, 0, 0, 0, 0}, Cols1Queue{order + cbeg, count, qhead, 0xFu, qv}, out,
                  rescue_list, rescue_count, thr, use_rescue, fb_list, fb_count);
}

}  // namespace fcs
