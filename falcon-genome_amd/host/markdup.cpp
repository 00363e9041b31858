// The rules of duplicate marking on a flat batch (markdup.h): the oracle of
// the device path and the host path.  Nothing here touches BAM files or the
// device library, so tools/micro/markdup_test.cpp links this file alone.
#include "markdup.h"

#include <algorithm>
#include <tuple>

#include "common.h"

namespace fcsg {

namespace {

bool examined(uint16_t flag) { return (flag & (kUnmapped | kSecondary | kSupplementary)) == 0; }

void check_batch(const fcsdup_batch& b) {
  if (b.n < 0) throw invalidParam("markdup: negative record count");
  for (int k = 0; k < 2; ++k) {
    const int64_t* off = k ? b.qual_off : b.cigar_off;
    const int64_t total = k ? b.n_qual : b.n_cigar;
    if (b.n > 0 && off[0] < 0) throw invalidParam("markdup: offsets start below zero");
    for (int64_t r = 0; r < b.n; ++r)
      if (off[r + 1] < off[r]) throw invalidParam("markdup: offsets out of order at record " + std::to_string(r));
    if (b.n > 0 && off[b.n] > total) throw invalidParam("markdup: offsets beyond the data");
  }
  for (int64_t r = 0; r < b.n; ++r) {
    const int32_t m = b.mate[r];
    if (m < -1 || m >= b.n || m == r || (m >= 0 && b.mate[m] != r))
      throw invalidParam("markdup: mate of record " + std::to_string(r) + " is out of range or not its mate in turn");
  }
}

struct End {
  int32_t ref;
  int64_t u5;
  int strand;
};

}  // namespace

void markdup_host_ends(const fcsdup_batch& b, std::vector<int64_t>& u5, std::vector<uint32_t>& score) {
  u5.assign((size_t)b.n, 0);
  score.assign((size_t)b.n, 0);
  for (int64_t r = 0; r < b.n; ++r) {
    const uint32_t* c = b.cigar + b.cigar_off[r];
    const int64_t nc = b.cigar_off[r + 1] - b.cigar_off[r];
    if (b.flag[r] & kReverse) {
      int64_t reflen = 0, trail = 0;
      int64_t last = nc;  // one past the last operation that is not a clip
      while (last > 0 && (cigar_op(c[last - 1]) == kS || cigar_op(c[last - 1]) == kH)) --last;
      for (int64_t k = 0; k < last; ++k) {
        const CigarOp op = cigar_op(c[k]);
        if (op == kM || op == kD || op == kN || op == kEq || op == kX) reflen += cigar_len(c[k]);
      }
      if (last > 0)  // a CIGAR of clips only has leading clips, no trailing ones
        for (int64_t k = last; k < nc; ++k) trail += cigar_len(c[k]);
      u5[r] = (int64_t)b.pos[r] + reflen - 1 + trail;
    } else {
      int64_t lead = 0;
      for (int64_t k = 0; k < nc && (cigar_op(c[k]) == kS || cigar_op(c[k]) == kH); ++k) lead += cigar_len(c[k]);
      u5[r] = (int64_t)b.pos[r] - lead;
    }
    uint32_t s = 0;
    for (int64_t i = b.qual_off[r]; i < b.qual_off[r + 1]; ++i)
      if (b.qual[i] >= 15) s += b.qual[i];
    score[r] = s;
  }
}

MarkdupStats mark_duplicates_host(const fcsdup_batch& b, uint8_t* dup) {
  check_batch(b);
  MarkdupStats st;
  const size_t n = (size_t)b.n;
  std::vector<int64_t> u5;
  std::vector<uint32_t> score;
  markdup_host_ends(b, u5, score);
  std::vector<char> ex(n), paired(n);
  for (size_t r = 0; r < n; ++r) ex[r] = examined(b.flag[r]), dup[r] = 0;
  for (size_t r = 0; r < n; ++r) {
    const int32_t m = b.mate[r];
    paired[r] = ex[r] && (b.flag[r] & kPaired) && !(b.flag[r] & kMateUnmapped) && m >= 0 && ex[m];
    st.examined += ex[r];
    st.fragments += ex[r] && !paired[r];
  }
  auto end_of = [&](size_t r) { return End{b.ref_id[r], u5[r], (b.flag[r] & kReverse) ? 1 : 0}; };
  // pairs: (lib; lesser end; greater end), then the greatest score, then the smallest index
  typedef std::tuple<int32_t, int32_t, int64_t, int, int32_t, int64_t, int> PairKey;
  struct PairItem {
    PairKey key;
    uint64_t score;
    size_t index, other;
  };
  std::vector<PairItem> pairs;
  for (size_t r = 0; r < n; ++r) {
    if (!paired[r] || (size_t)b.mate[r] < r || !paired[(size_t)b.mate[r]]) continue;
    const size_t m = (size_t)b.mate[r];
    const End a = end_of(r), c = end_of(m);
    const bool first = std::make_tuple(a.ref, a.u5, a.strand, r) < std::make_tuple(c.ref, c.u5, c.strand, m);
    const End &lo = first ? a : c, &hi = first ? c : a;
    pairs.push_back({PairKey(b.lib[first ? r : m], lo.ref, lo.u5, lo.strand, hi.ref, hi.u5, hi.strand),
                     (uint64_t)score[r] + score[m], r, m});
  }
  st.pairs = (int64_t)pairs.size();
  std::sort(pairs.begin(), pairs.end(), [](const PairItem& x, const PairItem& y) {
    if (x.key != y.key) return x.key < y.key;
    if (x.score != y.score) return x.score > y.score;
    return x.index < y.index;
  });
  for (size_t i = 1; i < pairs.size(); ++i)
    if (pairs[i].key == pairs[i - 1].key) dup[pairs[i].index] = dup[pairs[i].other] = 1;
  // fragments: every examined record grouped by E = (lib, ref, u5, strand)
  typedef std::tuple<int32_t, int32_t, int64_t, int> EndKey;
  std::vector<size_t> order;
  for (size_t r = 0; r < n; ++r)
    if (ex[r]) order.push_back(r);
  auto key_of = [&](size_t r) { return EndKey(b.lib[r], b.ref_id[r], u5[r], (b.flag[r] & kReverse) ? 1 : 0); };
  std::sort(order.begin(), order.end(), [&](size_t x, size_t y) {
    const EndKey kx = key_of(x), ky = key_of(y);
    if (kx != ky) return kx < ky;
    if (score[x] != score[y]) return score[x] > score[y];
    return x < y;
  });
  for (size_t i = 0; i < order.size();) {
    size_t j = i;
    bool any_paired = false;
    while (j < order.size() && key_of(order[j]) == key_of(order[i])) any_paired |= paired[order[j++]] != 0;
    bool kept = false;  // the first fragment in (score, index) order stays when the group has no paired record
    for (size_t k = i; k < j; ++k) {
      const size_t r = order[k];
      if (paired[r]) continue;
      if (any_paired || kept) dup[r] = 1;
      kept = true;
    }
    i = j;
  }
  for (size_t r = 0; r < n; ++r) st.duplicates += dup[r];
  return st;
}

}  // namespace fcsg
