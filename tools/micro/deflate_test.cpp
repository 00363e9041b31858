// Host check of csrc/bgzf_deflate.h (the device kernel's code construction,
// dynamic header, form choice and token packing) against zlib's inflate.  The
// matcher here is the device's scheme run serially (bgzf_deflate.hip: 64
// positions at a time look their 4-byte hash up in a table of last positions
// that holds the chunks before them, then enter themselves; a greedy parse
// picks the tokens), so the payload sizes it prints are the kernel's.
//   g++ -O1 -fsanitize=address,undefined -Ifalcon-genome_amd/csrc \
//       tools/micro/deflate_test.cpp -o /tmp/deflate_test -lz
//   deflate_test [iterations]              built-in payloads, random sizes
//   deflate_test OUT IN BLOCK_BYTES ...    each IN cut into blocks; OUT gets,
//                                          per block, a little-endian u32
//                                          payload size and the payload
// Every payload must inflate (zlib, raw) to its block; no code is longer than
// 15 bits (7 for the code-length code); every code the block sends is
// complete, or the one-code distance tree DEFLATE allows; the bytes written
// are the bytes the plan counted; no block is larger than its stored form.
#define __host__
#define __device__
#define __forceinline__ inline
#include "bgzf_deflate.h"

#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace fcs;

struct HostLanes {
  static int id() { return 0; }
  static constexpr int n() { return 1; }
  static void sync() {}
};

struct Token {
  int v, dist;
};

static std::vector<Token> find_tokens(const uint8_t* in, uint32_t n) {
  std::vector<Token> out;
  std::vector<uint32_t> table(1u << kDefHashBits, 0);
  auto hash_at = [&](uint32_t p) {
    uint32_t v = 0;
    for (int k = 0; k < kDefHashBytes; ++k) v |= (uint32_t)in[p + k] << (8 * k);
    return def_hash(v);
  };
  uint32_t next = 0;
  for (uint32_t base = 0; base < n; base += kDefChunk) {
    int len[kDefChunk] = {0}, dist[kDefChunk] = {0};
    for (uint32_t l = 0; l < (uint32_t)kDefChunk; ++l) {
      const uint32_t p = base + l;
      if (p + kDefHashBytes > n || p < next) continue;
      // two candidates: the nearest earlier position of this chunk with the
      // same hash, and the table's (the last one of the chunks before)
      const uint32_t h = hash_at(p), most = std::min<uint32_t>(kDefMaxMatch, n - p);
      uint32_t cand[2] = {0, table[h]};
      for (uint32_t j = l; j-- > 0;)
        if (hash_at(base + j) == h) {
          cand[0] = base + j + 1;
          break;
        }
      for (int k = 0; k < 2; ++k) {
        if (!cand[k]) continue;
        const uint32_t c = cand[k] - 1, d = p - c;
        if (d > (uint32_t)kDefWindow) continue;
        uint32_t m = 0;
        while (m < most && in[c + m] == in[p + m]) ++m;
        if (m >= (uint32_t)kDefMinMatch && !(m == (uint32_t)kDefMinMatch && d > (uint32_t)kDefTooFar) && (int)m > len[l])
          len[l] = (int)m, dist[l] = (int)d;
      }
    }
    for (uint32_t l = 0; l < (uint32_t)kDefChunk; ++l) {
      const uint32_t p = base + l;
      if (p + kDefHashBytes > n) continue;
      uint32_t& t = table[hash_at(p)];
      t = std::max(t, p + 1);
    }
    uint32_t cur = std::max(next, base) - base;
    while (cur < (uint32_t)kDefChunk && base + cur < n) {
      if (len[cur]) {
        out.push_back({len[cur], dist[cur]});
        cur += (uint32_t)len[cur];
      } else {
        out.push_back({in[base + cur], 0});
        ++cur;
      }
    }
    next = base + cur;
  }
  return out;
}

struct ByteSink {
  std::vector<uint8_t>& out;
  uint64_t buf = 0, total = 0;
  int cnt = 0;
  void put64(uint64_t v, int n) {  // n <= 48
    buf |= v << cnt;
    cnt += n;
    total += (uint64_t)n;
    while (cnt >= 8) out.push_back((uint8_t)buf), buf >>= 8, cnt -= 8;
  }
  void put(uint32_t v, int n) { put64(v, n); }
  void finish() {
    if (cnt > 0) out.push_back((uint8_t)buf), buf = 0, cnt = 0;
  }
};

static int g_problems = 0;
static void problem(const char* what, long a = 0, long b = 0) {
  if (++g_problems < 10) std::printf("PROBLEM: %s (%ld, %ld)\n", what, a, b);
}

// Kraft sum of len[0, n) against 2^max_len; `single_ok`: one code of length 1
static void check_code(const uint8_t* len, int n, int max_len, bool single_ok, const char* what) {
  uint64_t sum = 0;
  int used = 0;
  for (int s = 0; s < n; ++s) {
    if (len[s] > max_len) problem(what, s, len[s]);
    if (len[s]) sum += 1ull << (max_len - len[s]), ++used;
  }
  if (used == 0 && single_ok) return;
  if (used == 1 && single_ok && sum == (1ull << (max_len - 1))) return;
  if (sum != (1ull << max_len)) problem(what, (long)sum, used);
}

static void encode_block(const uint8_t* in, uint32_t n, std::vector<uint8_t>& payload, DefWork& w) {
  payload.clear();
  const std::vector<Token> tok = find_tokens(in, n);
  std::memset(w.freq, 0, sizeof w.freq);
  uint64_t covered = 0;
  for (const Token& t : tok) {
    int ls, ds;
    def_token_syms(t.v, t.dist, ls, ds);
    w.freq[ls]++;
    if (ds >= 0) w.freq[kDefLl + ds]++;
    covered += t.dist ? (uint64_t)t.v : 1;
    if (t.dist && (t.v < kDefMinMatch || t.v > kDefMaxMatch || t.dist > kDefWindow)) problem("token range", t.v, t.dist);
  }
  if (covered != n) problem("parse does not cover the block", (long)covered, n);
  w.freq[kDefEob] = 1;
  def_plan<HostLanes>(w, n);
  if (w.form == kDefDynamic) {
    check_code(w.len, kDefLl, 15, false, "literal/length code");
    check_code(w.len + kDefLl, kDefD, 15, true, "distance code");
    check_code(w.cl_len, kDefCl, 7, false, "code-length code");
  }
  if (w.form == kDefStored) {
    payload.push_back(1);
    payload.push_back((uint8_t)n), payload.push_back((uint8_t)(n >> 8));
    payload.push_back((uint8_t)~n), payload.push_back((uint8_t)(~n >> 8));
    payload.insert(payload.end(), in, in + n);
  } else {
    ByteSink sink{payload};
    def_put_header(w, sink);
    const uint64_t head = sink.total;
    uint64_t bits;
    int nb;
    for (const Token& t : tok) {
      def_token_bits(w, t.v, t.dist, bits, nb);
      sink.put64(bits, nb);
    }
    def_token_bits(w, kDefEob, 0, bits, nb);
    sink.put64(bits, nb);
    sink.finish();
    if (sink.total - head != w.bits_token) problem("token bits differ from the plan", (long)(sink.total - head), w.bits_token);
    if (sink.total != (w.form == kDefFixed ? w.bits_fixed : w.bits_dynamic)) problem("bits differ from the plan", (long)sink.total, w.form);
  }
  if (payload.size() != def_payload_bytes(w, n)) problem("payload bytes differ from the plan", (long)payload.size(), n);
  if (payload.size() > (size_t)n + 5) problem("larger than stored", (long)payload.size(), n);
  // zlib reads it back
  std::vector<uint8_t> back(n + 16);
  z_stream zs{};
  inflateInit2(&zs, -15);
  zs.next_in = payload.data();
  zs.avail_in = (uInt)payload.size();
  zs.next_out = back.data();
  zs.avail_out = (uInt)back.size();
  const int rc = inflate(&zs, Z_FINISH);
  if (rc != Z_STREAM_END || zs.total_out != n || zs.avail_in != 0 || (n && std::memcmp(back.data(), in, n) != 0))
    problem("zlib does not give the block back", rc, (long)zs.total_out);
  inflateEnd(&zs);
}

static std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> d;
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::printf("cannot read %s\n", path);
    std::exit(2);
  }
  uint8_t buf[65536];
  size_t k;
  while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + k);
  std::fclose(f);
  return d;
}

int main(int argc, char** argv) {
  DefWork* w = new DefWork;
  std::vector<uint8_t> payload;
  int blocks = 0;
  if (argc >= 4) {
    FILE* out = std::fopen(argv[1], "wb");
    if (!out) return 2;
    for (int a = 2; a + 1 < argc; a += 2) {
      const std::vector<uint8_t> d = read_file(argv[a]);
      const size_t bb = (size_t)std::atoi(argv[a + 1]);
      if (bb < 1 || bb > (size_t)kDefBlockMax) return 2;
      for (size_t at = 0; at < d.size(); at += bb, ++blocks) {
        const uint32_t n = (uint32_t)std::min(bb, d.size() - at);
        encode_block(d.data() + at, n, payload, *w);
        const uint32_t sz = (uint32_t)payload.size();
        const uint8_t le[4] = {(uint8_t)sz, (uint8_t)(sz >> 8), (uint8_t)(sz >> 16), (uint8_t)(sz >> 24)};
        std::fwrite(le, 1, 4, out);
        std::fwrite(payload.data(), 1, payload.size(), out);
      }
    }
    std::fclose(out);
  } else {
    const int iters = argc > 1 ? std::atoi(argv[1]) : 300;
    std::mt19937 rng(11);
    const char* line = "chr1\t100\t.\tA\t<NON_REF>\t.\t.\tEND=105\tGT:DP\t0/0:30\n";
    const size_t line_len = std::strlen(line);
    for (int it = 0; it < iters; ++it, ++blocks) {
      size_t n = 1 + rng() % kDefBlockMax;
      if (it % 4 == 0) n = 1 + rng() % 600;
      std::vector<uint8_t> d(n);
      const int kind = it % 6;
      const int skew = 1 + (int)(rng() % 40);
      for (size_t i = 0; i < n; ++i) {
        if (kind == 0) d[i] = (uint8_t)rng();
        else if (kind == 1) d[i] = (uint8_t)"ACGT\t0123456789\n"[rng() % 16];
        else if (kind == 2) d[i] = (i % 100 < 60) ? (uint8_t)line[i % line_len] : (uint8_t)(rng() % 32 + 33);
        else if (kind == 3) d[i] = (rng() % 10 == 0) ? (uint8_t)rng() : 'A';
        else if (kind == 4) d[i] = i < 8 ? (uint8_t)rng() : d[i - 1 - rng() % 8];
        else {  // a steep histogram: deep unconstrained trees
          int s = 0;
          while (s < 40 && rng() % (unsigned)(skew % 3 + 2) == 0) ++s;
          d[i] = (uint8_t)(s * 5 + 1);
        }
      }
      encode_block(d.data(), (uint32_t)n, payload, *w);
    }
  }
  delete w;
  std::printf("deflate: %d problems in %d blocks\n", g_problems, blocks);
  return g_problems ? 1 : 0;
}
