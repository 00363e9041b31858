"""Inputs at the shapes the record kernels really run at:
past the first trip of every block- and grid-stride loop, past the first pass of
every single-block scan, and at chr1-sized coordinates.

- CAPS: the launch caps as the .hip sources state them (PINNED: where and how
  each is read), and SHAPES: every scale shape, derived from CAPS.
  tests/test_scale_cpu.py fails when a source no longer says what CAPS says.
  The FMD seeding kernels' caps and shapes are here too; their
  inputs are tests/fmd_scale_cases.py.
- Sparse-wide inputs: a few thousand mixed-CIGAR records of the existing
  generators in bands around the tile boundaries of a very long window; the
  Python restatements (depth_cases, ug_cases) are their reference.
- Many-record inputs: flat numpy arrays (never per-record dicts) of records of
  1 to 3 aligned bases at distinct ascending positions, and a vectorised
  reference per feature, written from DESIGN §2's rules on np.add.at / bincount
  / cumsum / lexsort in int64.  No reference here calls the library.
"""
import os
import re

import numpy as np

import bqsr_cases as B
import depth_cases as D
import markdup_cases as M
import ug_cases as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "falcon-genome_amd", "csrc")

# ------------------------------------------------------------------ the caps and the shapes
CAPS = dict(ug_max_blocks=2048, ug_block=256, dp_max_blocks=4096, dp_tile=4 * 256, bq_max_blocks=2048, bq_min_slice=32,
            md_max_blocks=256 * 8, md_ends_blocks=256 * 32, bq_replica_bytes=64 << 20, bq_replica_max=16,
            fmd_max_units=32768, fmd_block=256, fmd_locate_max_blocks=256 * 8, seed_row=16, seed_order_block=64,
            seed_block=256, seed_scan_block=1024, seed_order_max_blocks=256 * 64, seed_expand_max_blocks=256 * 8,
            seed_locate_max_blocks=256 * 8)

# name: (source, pattern with one group, the group's text, the shapes to look at again)
PINNED = dict(
    ug_max_blocks=("ug.hip", r"constexpr int kUgMaxBlocks = ([^;]+);", "2048", "ug_window, ug_records"),
    ug_block=("ug.hip", r"constexpr int kUgBlock = ([^;]+);", "256", "ug_window, ug_records, ug_pass"),
    dp_max_blocks=("depth.hip", r"constexpr int kDpMaxBlocks = ([^;]+);", "4096", "dp_window, dp_pieces"),
    dp_tile=("depth.hip", r"constexpr int kDpTile = ([^;]+);", "4 * kDpBlock", "dp_window"),
    dp_block=("depth.hip", r"constexpr int kDpBlock = ([^;]+);", "256", "dp_window"),
    dp_stats_grid=("depth.hip", r"dp_stats_kernel, dim3\(\(unsigned\)std::clamp<int64_t>\(n_pieces, 1, ([^)]+)\)\)",
                   "8 * kDpMaxBlocks", "dp_pieces"),
    bq_max_blocks=("bqsr.hip", r"constexpr int kBqMaxBlocks = ([^;]+);", "2048", "bq_apply, bq_count, bq_check, bq_rg"),
    bq_min_slice=("bqsr.hip", r"constexpr int kBqMinSlice = ([^;]+);", "32", "bq_count"),
    bq_block=("bqsr.hip", r"constexpr int kBqBlock = ([^;]+);", "256", "bq_apply, bq_check"),
    md_max_blocks=("markdup.hip", r"constexpr int kMdMaxBlocks = ([^;]+);", "256 * 8", "md_all"),
    md_block=("markdup.hip", r"constexpr int kMdBlock = ([^;]+);", "256", "md_all, md_ends"),
    md_row=("markdup.hip", r"constexpr int kMdRow = ([^;]+);", "16", "md_ends"),
    md_ends_blocks=("markdup.hip", r"md_ends_kernel, dim3\(\(int\)std::min<int64_t>\(\(n \+ kRows - 1\) / kRows, ([^)]+)\)\)",
                    "256 * 32", "md_ends"),
    bq_replica_bytes=("bqsr.hip", r"\(\(size_t\)(64 << 20)\) / one\)", "64 << 20", "bq_rg"),
    bq_replica_max=("bqsr.hip", r"/ one\), 1, (\d+)\);", "16", "bq_rg"),
    fmd_max_units=("fmd_seed.hip", r"constexpr int kFmdMaxUnits = ([^;]+);", "32768", "fmd_units, fmd_reads"),
    fmd_block=("fmd_seed.hip", r"constexpr int kFmdBlock = ([^;]+);", "256", "fmd_locate, fmd_rows"),
    fmd_locate_max_blocks=("fmd_seed.hip", r"constexpr int kFmdLocateMaxBlocks = ([^;]+);", "256 * 8", "fmd_locate, fmd_rows"),
    seed_row=("fmd_seeds.hip", r"constexpr int kSeedRow = ([^;]+);", "16", "fmd_expand, fmd_order, fmd_reads"),
    seed_order_block=("fmd_seeds.hip", r"constexpr int kSeedOrderBlock = ([^;]+);", "64", "fmd_order, fmd_reads"),
    seed_block=("fmd_seeds.hip", r"constexpr int kSeedBlock = ([^;]+);", "256", "fmd_expand, fmd_seed_locate"),
    seed_scan_block=("fmd_seeds.hip", r"constexpr int kSeedScanBlock = ([^;]+);", "1024", "fmd_scan_per, fmd_scan_empty"),
    seed_order_max_blocks=("fmd_seeds.hip", r"constexpr int kSeedOrderMaxBlocks = ([^;]+);", "256 * 64", "fmd_order, fmd_reads"),
    seed_expand_max_blocks=("fmd_seeds.hip", r"constexpr int kSeedExpandMaxBlocks = ([^;]+);", "256 * 8", "fmd_expand"),
    seed_locate_max_blocks=("fmd_seeds.hip", r"constexpr int kSeedLocateMaxBlocks = ([^;]+);", "256 * 8", "fmd_seed_locate"),
)


def read_pinned():
    """{name: the text the source holds now, or None}."""
    out = {}
    for name, (source, pattern, _, _) in PINNED.items():
        m = re.search(pattern, open(os.path.join(CSRC, source)).read())
        out[name] = m.group(1) if m else None
    return out


def bq_replicas(n_rg):
    """bqsr.hip's bq_replicas: 64 MiB of replicas at most, 16 at most."""
    one = max(n_rg, 1) * B.NQ * (B.NCTX + B.NCYC) * 8
    return min(max(CAPS["bq_replica_bytes"] // one, 1), CAPS["bq_replica_max"])


def _shapes():
    c = CAPS
    ub, dt = c["ug_block"], c["dp_tile"]
    s = dict(
        ug_window=c["ug_max_blocks"] * ub + ub + 37,            # 2,050 tiles: block 0 takes a second tile, the last is partial
        ug_records=c["ug_max_blocks"] * ub + ub + 5,            # ug_span / ug_scan take a second grid trip
        ug_pass=ub * ub,                                        # records (or loci) per pass of a single-block scan
        ug_many_window=3 * ub * ub,
        dp_window=c["dp_max_blocks"] * dt + dt + 37,            # 4,098 tiles
        dp_records=150000, dp_many_window=300000,
        dp_pieces=8 * c["dp_max_blocks"] + 300, dp_pieces_len=2400000,
        md_ends=c["md_ends_blocks"] * 16 + 16 * 3 + 5,          # 16 records per block of md_ends_kernel
        md_all=c["md_max_blocks"] * 256 + 256 + 5,
        bq_apply=c["bq_max_blocks"] * 4 + 4 * 3 + 1,            # a wave per record, 4 waves per block
        bq_count=c["bq_max_blocks"] * c["bq_min_slice"] + c["bq_max_blocks"] + 7,
        bq_check=c["bq_max_blocks"] * 256 + 256 + 5,
        bq_rg=(6, 90),
        # FMD seeding: reads or rows one launch of each kernel covers in its first trip
        fmd_units=c["fmd_max_units"],                                                  # fmd_collect_kernel: a read per quad
        fmd_expand=c["seed_expand_max_blocks"] * (c["seed_block"] // c["seed_row"]),   # fmd_seed_expand_kernel
        fmd_order=c["seed_order_max_blocks"] * (c["seed_order_block"] // c["seed_row"]),   # fmd_seed_order_kernel
        fmd_locate=c["fmd_locate_max_blocks"] * c["fmd_block"],                        # fmd_locate_kernel
        fmd_seed_locate=c["seed_locate_max_blocks"] * c["seed_block"],                 # fmd_seed_locate_kernel
    )
    s["fmd_reads"] = max(s["fmd_order"], 2 * s["fmd_units"], 2 * s["fmd_expand"]) + 1 + 3   # past every per-read cap
    s["fmd_rows"] = s["fmd_locate"] + 257
    s["fmd_scan_per"] = -(-s["fmd_reads"] // c["seed_scan_block"])                     # reads per lane of the scan
    s["fmd_scan_empty"] = c["seed_scan_block"] - -(-s["fmd_reads"] // s["fmd_scan_per"])   # trailing lanes without a read
    s["ug_tiles"] = -(-s["ug_window"] // ub)
    s["dp_tiles"] = -(-s["dp_window"] // dt)
    s["bq_count_slice"] = -(-s["bq_count"] // c["bq_max_blocks"])
    return s


SHAPES = _shapes()
FILTER = D.FILTER
HIGH_CONTIG = 2 ** 31 - 1
HIGH_WINDOW = 1024 + 37


# ------------------------------------------------------------------ flat batches of short records
class Flat:
    """A batch of M-only records (optionally a leading and a trailing S) of 1 to 3 aligned bases as flat arrays.
    skips {record: k}: that record is 1M kN 1M instead."""

    def __init__(self, n, span, seed, skips=None, n_rg=3, n_lib=3):
        rng = np.random.default_rng(seed)
        self.n = n
        self.pos = np.sort(rng.choice(span, n, replace=False)).astype(np.int64)
        self.ref_id = np.zeros(n, np.int32)
        self.flag = rng.choice(np.array([0, 0, 0, 0, 0, 0, 0x10, 0x10, 0x41, 0x91, 0x800, 0x400, 0x100, 0x200, 0x4], np.uint16), n)
        self.mapq = rng.choice(np.array([0, 16, 17, 20, 29, 30, 60, 60, 60, 60, 255], np.uint8), n)
        self.m = rng.integers(1, 4, n).astype(np.int64)
        self.lead = rng.choice(np.array([0, 0, 0, 0, 1, 2], np.int64), n)
        self.trail = rng.choice(np.array([0, 0, 0, 0, 1], np.int64), n)
        self.skip = np.zeros(n, np.int64)
        for r, k in (skips or {}).items():
            self.skip[r], self.m[r], self.lead[r], self.trail[r] = k, 2, 0, 0
            self.flag[r], self.mapq[r] = 0, 60
        self.rg = rng.integers(0, n_rg, n).astype(np.int32)
        self.lib = rng.integers(0, n_lib, n).astype(np.int32)
        self.n_bases = self.lead + self.m + self.trail
        self.base_off = np.concatenate([[0], np.cumsum(self.n_bases)]).astype(np.int64)
        total = int(self.base_off[-1])
        self.absent = (rng.random(n) < 0.03).astype(np.uint8)
        self.qual = rng.choice(np.array([2, 10, 16, 17, 18, 25, 30, 30, 37, 40, 41], np.uint8), total)
        self.qual[np.repeat(self.absent, self.n_bases) != 0] = 0xFF
        self.bases = rng.choice(np.frombuffer(b"AAACCCGGGTTTNacgt", np.uint8), total)
        # the CIGAR words: up to three per record
        sk = self.skip > 0
        w = np.zeros((n, 3), np.uint32)
        w[:, 0] = np.where(sk, (1 << 4) | 0, (self.lead << 4) | 4)
        w[:, 1] = np.where(sk, (self.skip << 4) | 3, (self.m << 4) | 0)
        w[:, 2] = np.where(sk, (1 << 4) | 0, (self.trail << 4) | 4)
        keep = np.stack([sk | (self.lead > 0), np.ones(n, bool), sk | (self.trail > 0)], axis=1)
        self.cigar = w[keep]
        self.cigar_off = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)

    def ref_len(self):
        return self.m + self.skip

    def aligned(self):
        """Per aligned base: (record, reference position, index of its byte in bases / qual)."""
        rec = np.repeat(np.arange(self.n), self.m)
        j = np.arange(len(rec)) - np.repeat(np.cumsum(self.m) - self.m, self.m)
        locus = self.pos[rec] + j + np.where(j >= 1, self.skip[rec], 0)
        return rec, locus, self.base_off[rec] + self.lead[rec] + j

    def dp(self):
        return (self.flag, self.ref_id, self.pos, self.mapq, self.cigar, self.cigar_off, self.qual, self.base_off, self.absent)

    def ug(self):
        return (self.flag, self.ref_id, self.pos, self.mapq, self.cigar, self.cigar_off, self.bases, self.qual, self.base_off,
                self.absent)

    def records(self, lo, hi, kind):
        """Records [lo, hi) as the dicts of depth_cases ('dp') or ug_cases ('ug')."""
        out = []
        for r in range(lo, hi):
            words = self.cigar[self.cigar_off[r]:self.cigar_off[r + 1]]
            cigar = "".join(f"{int(x) >> 4}{D.OPS[int(x) & 15]}" for x in words)
            b0, b1 = int(self.base_off[r]), int(self.base_off[r + 1])
            qual = None if self.absent[r] else [int(q) for q in self.qual[b0:b1]]
            d = dict(flag=int(self.flag[r]), ref=int(self.ref_id[r]), pos=int(self.pos[r]), mapq=int(self.mapq[r]), cigar=cigar,
                     qual=qual, n_bases=b1 - b0)
            if kind == "ug":
                d["seq"] = self.bases[b0:b1].tobytes().decode()
            out.append(d)
        return out


# ------------------------------------------------------------------ depth: the vectorised reference
def depth_np(f, window, contig_len, prm):
    """DESIGN §2 "Depth of coverage" on a Flat batch: +1 / -1 at the ends of every counted base in a difference array."""
    ref, start, length = window
    ok = (f.ref_id == ref) & ((f.flag & FILTER) == 0) & (f.mapq.astype(np.int64) >= prm["min_mapq"]) & (
        f.mapq.astype(np.int64) <= prm["max_mapq"])
    rec, locus, byte = f.aligned()
    q = np.where(f.absent[rec] != 0, 0, f.qual[byte].astype(np.int64))
    take = ok[rec] & (q >= prm["min_baseq"]) & (q <= prm["max_baseq"]) & (locus >= max(start, 0)) & (
        locus < min(start + length, contig_len))
    diff = np.zeros(length + 1, np.int64)
    np.add.at(diff, locus[take] - start, 1)
    np.add.at(diff, locus[take] - start + 1, -1)
    return np.cumsum(diff)[:length].astype(np.uint32)


def bitmap_np(part):
    """depth_cases.bitmap, vectorised: bit i & 63 of word i >> 6, and one word to spare."""
    words = (len(part) + 63) // 64 + 1
    bits = np.zeros(words * 64, np.uint8)
    bits[:len(part)] = np.asarray(part, np.uint8)
    return np.packbits(bits, bitorder="little").view(np.uint64)


def quantile_np(hist, k):
    n = int(hist.sum())
    if n == 0:
        return 1
    return max(int(np.argmax(4 * np.cumsum(hist.astype(np.int64)) >= k * n)), 1)


def stats_np(d, part, pieces, n_long=0):
    """depth_cases.stats, a numpy pass per piece."""
    d, part = np.asarray(d, np.int64), np.asarray(part, bool)
    hist, long_hist, out = np.zeros(D.BINS, np.uint64), np.zeros((n_long, D.BINS), np.uint64), []
    for s, e, li in pieces:
        vals = d[s:e][part[s:e]]
        h = np.bincount(np.minimum(vals, D.BINS - 1), minlength=D.BINS).astype(np.uint64)
        hist += h
        row = dict(total=int(vals.sum()), loci=len(vals), above=int((vals >= D.ABOVE).sum()), q1=0, median=0, q3=0)
        if li >= 0:
            long_hist[li] += h
        else:
            row.update(q1=quantile_np(h, 1), median=quantile_np(h, 2), q3=quantile_np(h, 3))
        out.append(row)
    return hist, long_hist, out


def summaries(rows):
    return [{k: int(s[k]) for k in ("total", "loci", "above", "q1", "median", "q3")} for s in rows]


# ------------------------------------------------------------------ depth: the inputs
DP_PRM = D.params(1, 254, 2, 40, True)


def band_records(generator, bands, n, seed, **kw):
    """n records of generator over one contig of 1,200 loci per band, moved to [centre - 600, centre + 600) of contig 0."""
    refs = kw.pop("refs", None) or ["A" * 1200] * len(bands)
    out = []
    for r in generator(refs, seed=seed, n=n, **kw):
        out.append(dict(r, ref=0, pos=bands[r["ref"]] - 600 + r["pos"]))
    return out


def depth_sparse():
    """dict(records, window, contig_len, boundaries (window-relative), want): 3,000 mixed-CIGAR records around the tile
    boundaries 255|256, 4,095|4,096, 4,096|4,097 (the last, partial tile) and both window ends of a 4,195,365-locus
    window with an odd start."""
    W, T = SHAPES["dp_window"], CAPS["dp_tile"]
    start = 10001
    contig_len = start + W + 2000
    bounds = [256 * T, CAPS["dp_max_blocks"] * T, (CAPS["dp_max_blocks"] + 1) * T]
    centres = [start + 300] + [start + b for b in bounds] + [start + W]
    records = band_records(D.random_batch, centres, 3000, 31)
    edge = start + CAPS["dp_max_blocks"] * T
    # a deletion that straddles 4,095|4,096, a run of counted bases across it, and starts without ends before 255|256
    records += [D.rec(0, 0, edge - 25, "20M10D20M", 30, mapq=60), D.rec(0, 0, edge - 50, "100M", 30, mapq=60),
                D.rec(0, 0, start + bounds[0] - 3, "6M", 30, mapq=60)]
    window = (0, start, W)
    want, beyond = D.depth(records, window, contig_len, DP_PRM)
    assert not beyond
    return dict(records=records, window=window, contig_len=contig_len, bounds=bounds, want=want)


def depth_sparse_pieces(W):
    """Pieces across 255|256 and 4,095|4,096 tiles, short ones on each boundary, and one long interval over the whole
    window (long row 0) in pieces of 65,536."""
    T = CAPS["dp_tile"]
    pieces = []
    for b in (256 * T, CAPS["dp_max_blocks"] * T):
        pieces += [(b - 300, b + 300, -1), (b - 1, b + 1, -1), (b - 64, b, -1), (b, b + 65, -1), (b - 64000, b + 1000, 1)]
    pieces += [(W - 37, W, -1), (0, 1, -1)]
    pieces += [(s, min(s + D.PIECE_MAX, W), 0) for s in range(0, W, D.PIECE_MAX)]
    return pieces


def depth_sparse_part(W):
    part = np.ones(W, bool)
    b = CAPS["dp_max_blocks"] * CAPS["dp_tile"]
    part[b - 20:b + 7] = False            # a run of reference N across 4,095|4,096
    part[256 * CAPS["dp_tile"] + 100:256 * CAPS["dp_tile"] + 130] = False
    return part


def depth_many():
    f = Flat(SHAPES["dp_records"], SHAPES["dp_many_window"] - 3, 41)
    return f, (0, 0, SHAPES["dp_many_window"]), SHAPES["dp_many_window"]


def depth_pieces():
    """(depth, part, pieces, n_long): 33,068 pieces of 1 to 70 loci over 2,400,000 loci of depths 0 to 520, every
    seventh piece on one of 3 long rows, stretches without participating loci."""
    rng = np.random.default_rng(51)
    n, L = SHAPES["dp_pieces"], SHAPES["dp_pieces_len"]
    depth = rng.integers(0, 40, L).astype(np.uint32)
    hot = rng.integers(0, L - 400, 300)
    for h in hot:
        depth[h:h + 400] = rng.integers(0, 521, 400)
    part = rng.random(L) < 0.9
    lengths = rng.integers(1, 71, n)
    starts = np.sort(rng.choice(L - 71, n, replace=False))
    for k in range(0, n, 97):              # pieces without a participating locus
        part[starts[k]:starts[k] + lengths[k]] = False
    for k in range(1, n, 11):              # low depths: the quantiles 1 to 3 all occur
        depth[starts[k]:starts[k] + lengths[k]] = rng.integers(0, 5, lengths[k])
    pieces = [(int(s), int(s + k), (i // 7) % 3 if i % 7 == 0 else -1) for i, (s, k) in enumerate(zip(starts, lengths))]
    return depth, part, pieces, 3


def depth_high():
    """Records near 2^31 - 1: one ends at the contig's end, a deletion crosses each window's start, one runs to the
    contig's end; `past` lies a base beyond the contig.  Two windows of 1,061 loci: one ends at the contig's end, one
    has an odd start."""
    C, n = HIGH_CONTIG, HIGH_WINDOW
    s0 = C - n
    records = [D.rec(0, 0, s0 - 12, "8M10D6M", 30), D.rec(0, 0, s0 - 11, "8M10D6M", 30), D.rec(0, 0, s0 - 1, "3M", 30),
               D.rec(0x10, 0, s0 + 250, "30M2I30M5D10M", 30), D.rec(0, 0, s0 + 255, "2S300M", 35),
               D.rec(0, 0, s0 + 700, "20M200N5M", 30), D.rec(0, 0, C - 40, "10M30D", 30), D.rec(0, 0, C - 10, "10M", 30)]
    past = D.rec(0, 0, C - 9, "10M", 30)
    return dict(records=records, past=past, contig_len=C, windows=[(0, s0, n), (0, s0 - 1, n)])


# ------------------------------------------------------------------ ug: the vectorised reference
TAB = U.table()
_CODE = np.full(256, 4, np.int64)
for _k, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _k


def sites_np(f, window, refseq, site_dtype, min_baseq=17):
    """DESIGN §2 "UnifiedGenotyper, SNP model" on a Flat batch without deletions: rows of site_dtype (fcship.UG_SITE).
    refseq: the contig as uint8."""
    ref, start, length = window
    clen = len(refseq)
    mine = f.ref_id == ref
    assert (np.diff(f.pos[mine]) >= 0).all()
    ok = mine & ((f.flag & FILTER) == 0) & (f.mapq != 255)
    rec, locus, byte = f.aligned()
    mq = f.mapq[rec].astype(np.int64)
    qe = np.minimum(np.minimum(np.where(f.absent[rec] != 0, 0, f.qual[byte].astype(np.int64)), mq), U.MAXQ)
    x = _CODE[f.bases[byte]]
    take = ok[rec] & (x < 4) & (qe >= min_baseq) & (locus >= max(start, 0)) & (locus < min(start + length, clen))
    cell, x, qe, mq = (locus[take] - start), x[take], qe[take], mq[take]
    tab = np.array(TAB, np.int64)
    n, qsum = np.zeros((length, 4), np.int64), np.zeros((length, 4), np.int64)
    sums = np.zeros((3, length, 4), np.int64)
    mq2 = np.zeros(length, np.int64)
    np.add.at(n, (cell, x), 1)
    np.add.at(qsum, (cell, x), qe)
    np.add.at(mq2, cell, mq * mq)
    for k in range(3):
        np.add.at(sums[k], (cell, x), tab[qe, k])
    rc = _CODE[refseq[start:start + length]]
    letters = np.arange(4)[None, :]
    non_ref = letters != rc[:, None]
    site = (rc < 4) & ((n > 0) & non_ref).any(axis=1)
    at = np.nonzero(site)[0]
    n, qsum, sums, rc, non_ref = n[at], qsum[at], sums[:, at], rc[at], non_ref[at]
    alt = np.argmax(np.where(non_ref, qsum, -1), axis=1)           # the largest qsum, the smaller letter on a tie
    A, Bs, Cs = sums
    rows = np.arange(len(at))
    is_alt = letters == alt[:, None]
    out = np.zeros(len(at), site_dtype)
    out["offset"], out["ref"], out["alt"], out["n"], out["qsum"], out["mq2"] = at, rc, alt, n, qsum, mq2[at]
    out["gl"][:, 0] = A[rows, rc] + np.where(non_ref, Cs, 0).sum(axis=1)
    out["gl"][:, 1] = Bs[rows, rc] + Bs[rows, alt] + np.where(non_ref & ~is_alt, Cs, 0).sum(axis=1)
    out["gl"][:, 2] = A[rows, alt] + np.where(~is_alt, Cs, 0).sum(axis=1)
    return out


def site_rows(sites, site_dtype):
    """ug_cases' site dicts as rows of site_dtype."""
    out = np.zeros(len(sites), site_dtype)
    for k, s in enumerate(sites):
        out[k] = (s["offset"], s["ref"], s["alt"], 0, s["n"], s["qsum"], s["n_del"], 0, s["mq2"], s["gl"])
    return out


# ------------------------------------------------------------------ ug: the inputs
def ug_sparse(start):
    """dict(records, refseq, window, want): 3,000 mixed-CIGAR records from two planted haplotypes in bands at the window's
    start, around tiles 255|256, and from tile 2,046 to beyond the window's end, of a window of 524,581 loci at `start`;
    the contig outside the bands is ACGT repeating, with a run of N across 255|256."""
    W, T = SHAPES["ug_window"], CAPS["ug_block"]
    last = CAPS["ug_max_blocks"] * T
    centres = [start + 600, start + 256 * T, start + last - 700, start + last + 500]
    band_refs = U.random_world(seed=61)[0][:4800]
    band_refs = [band_refs[k:k + 1200].upper() for k in range(0, 4800, 1200)]
    clen = start + W + 1400
    seq = np.frombuffer(b"ACGT" * (clen // 4 + 1), np.uint8)[:clen].copy()
    for c, s in zip(centres, band_refs):
        seq[c - 600:c + 600] = np.frombuffer(s.encode(), np.uint8)
    cut = start + 256 * T
    seq[cut - 6:cut + 9] = ord("N")
    refseq = seq.tobytes().decode()
    moved = [refseq[c - 600:c + 600] for c in centres]
    records = band_records(U.random_batch, centres, 3000, 62, refs=moved, mismatch=0.15)

    def unlike(pos, cigar, mapq=60):
        return U.rec(0, 0, pos, cigar, "".join(U.other(ch) for ch in U.read_of(refseq, pos, cigar)), 30, mapq)

    t0 = start + last                      # the first locus of tile 2,048
    records += [unlike(t0 - 2, "4M"), unlike(t0, "1M"), unlike(t0 + T - 3, "6M"), unlike(t0 + T - 1, "1M"),
                unlike(t0 + 100, "4M4D4M"), unlike(t0 - 3, "2M3D2M"), unlike(start + W - 2, "4M")]
    records.sort(key=lambda r: r["pos"])
    window = (0, start, W)
    want, beyond = U.sites(records, window, refseq, TAB)
    assert not beyond
    return dict(records=records, refseq=refseq, window=window, want=want)


def ug_many(interleaved=False):
    """dict(flat, refs (uint8 per contig), windows): 524,549 records of 1 to 3 bases at distinct ascending positions of a
    contig of 900,000 loci; the window of 196,608 loci starts at an odd locus inside it.  Five records skip 3,000 loci
    (1M 3000N 1M), so the running maximum of the ends stays above the ends of the records that follow; two of them lie
    102 records before a pass boundary of the one-block scan over record tiles, inside the window, and both of their
    bases differ from the reference.  interleaved:
    every third record lies on contig 1."""
    n, clen, W = SHAPES["ug_records"], 900000, SHAPES["ug_many_window"]
    start = 300001
    probe = Flat(n, clen - 3010, 71)
    first = int(np.searchsorted(probe.pos, start - 1500))
    inside = int(np.searchsorted(probe.pos, start + 100000))
    skips = {first - first % 3: 3000, inside - inside % 3: 3000, 900: 3000}
    skips.update({k * SHAPES["ug_pass"] - 102 - (k * SHAPES["ug_pass"] - 102) % 3: 3000 for k in (3, 4)})   # across a scan pass
    f = Flat(n, clen - 3010, 71, skips=skips)
    rng = np.random.default_rng(72)
    refs = [rng.choice(np.frombuffer(b"ACGT", np.uint8), clen) for _ in range(2)]
    refs[0][start + 5000:start + 5040] = ord("N")
    refs[0][start + 9000:start + 9300] |= 0x20   # lower case
    for r in skips:                              # both bases of a skipping record differ from the reference
        b0 = int(f.base_off[r])
        for j, p in enumerate((int(f.pos[r]), int(f.pos[r]) + 3001)):
            refs[0][p] &= 0xDF
            if refs[0][p] == ord("N"):
                refs[0][p] = ord("A")
            f.bases[b0 + j] = ord(U.other(chr(refs[0][p])))
            f.qual[b0 + j] = 30
        f.absent[r] = 0
    if interleaved:
        f.ref_id = np.where(np.arange(n) % 3 == 2, 1, 0).astype(np.int32)
    return dict(flat=f, refs=refs, windows=[(c, start, W) for c in ((0, 1) if interleaved else (0,))], contig_len=clen)


def ug_end(f, window_ref):
    """ug_span_kernel's end[r]: pos + reference length of a counted record of the window's contig, else None (as -1)."""
    ok = (f.ref_id == window_ref) & ((f.flag & FILTER) == 0) & (f.mapq != 255)
    return np.where(ok, f.pos + f.ref_len(), -1)


def ug_swaps():
    """Pairs of record indices whose positions are swapped for the order tests: across the first and the third pass
    boundary of the one-block scan over record tiles, and inside a tile."""
    p = SHAPES["ug_pass"]
    return [(p - 1, p), (3 * p - 1, 3 * p), (1000, 1001)]


class SeqView:
    """A read-only contig of `length` letters: ACGT repeating, with `inside` (a str) at `at`."""

    def __init__(self, length, at, inside):
        self.length, self.at, self.inside = length, at, inside

    def __len__(self):
        return self.length

    def __getitem__(self, k):
        if isinstance(k, slice):
            return "".join(self[i] for i in range(*k.indices(self.length)))
        if k < 0:
            k += self.length
        if self.at <= k < self.at + len(self.inside):
            return self.inside[k - self.at]
        return "ACGT"[k % 4]


def ug_high():
    """depth_high's coordinates with letters: dict(records, past, refseq (a SeqView of 2^31 - 1 letters), windows)."""
    C, n = HIGH_CONTIG, HIGH_WINDOW
    s0 = C - n
    rng = np.random.default_rng(81)
    inside = rng.choice(np.frombuffer(b"ACGTACGTACGTNa", np.uint8), n + 40).tobytes().decode()
    inside = inside[:36] + "ACGTACGT" + inside[44:-12] + "ACGTACGTACGT"      # plain letters at both ends of the windows
    refseq = SeqView(C, s0 - 40, inside)

    def read(pos, cigar, every=3, mapq=60, flag=0):
        seq = list(U.read_of(refseq, pos, cigar))
        for i in range(0, len(seq), every):
            seq[i] = U.other(seq[i], 1 + i % 3)
        return U.rec(flag, 0, pos, cigar, "".join(seq), 30, mapq)

    records = [read(s0 - 12, "8M10D6M"), read(s0 - 11, "8M10D6M"), read(s0 - 1, "3M", 1), read(s0 + 250, "30M2I30M5D10M", flag=0x10),
               read(s0 + 255, "2S300M", 7), read(s0 + 700, "20M200N5M"), read(C - 40, "10M30D"), read(C - 10, "10M", 1)]
    past = read(C - 9, "10M", 2)
    return dict(records=records, past=past, refseq=refseq, windows=[(0, s0, n), (0, s0 - 1, n)])


# ------------------------------------------------------------------ markdup: flat batches and the vectorised reference
class FlatDup:
    """n records (fragments, pairs, and some secondary / supplementary / unmapped ones) as fcsdup_batch's arrays, in a
    random order, so that a pair's reads and a duplicate set's members lie anywhere in the batch.  About 45 % of the
    templates repeat another's (library, contig, unclipped 5' ends, strands) in sets of 2 to 5; a record is 1 to 3
    aligned bases, with up to 2 clipped bases at its 5' end that leave its unclipped 5' position where it was."""

    def __init__(self, n, seed, n_lib=3, n_ref=3):
        rng = np.random.default_rng(seed)
        # the classes of coordinates, and the templates that share each
        sizes = rng.choice(np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 3, 4, 5]), n)
        is_pair = rng.random(n) < 0.7
        per = np.where(is_pair, 2, 1) * sizes
        classes = int(np.searchsorted(np.cumsum(per), n * 0.95))
        sizes, is_pair = sizes[:classes], is_pair[:classes]
        cls = np.repeat(np.arange(classes), sizes)                    # a template's class
        c_lib, c_ref = rng.integers(0, n_lib, classes), rng.integers(0, n_ref, classes)
        c_u1 = rng.integers(10, 1 << 28, classes)
        c_u2 = c_u1 + rng.integers(50, 300, classes)
        c_rev = rng.random(classes) < 0.5
        t_pair = is_pair[cls]
        # the reads: a template's first, then the second reads of the pairs
        first, second = np.arange(len(cls)), np.nonzero(t_pair)[0]
        tmpl = np.concatenate([first, second])
        is_second = np.concatenate([np.zeros(len(first), bool), np.ones(len(second), bool)])
        k = len(tmpl)
        extra = n - k                                                 # unexamined records at examined ones' coordinates
        assert extra > n // 50
        src = rng.integers(0, k, extra)
        tmpl, is_second = np.concatenate([tmpl, tmpl[src]]), np.concatenate([is_second, is_second[src]])
        c = cls[tmpl]
        rev = np.where(is_second, ~c_rev[c], c_rev[c])
        u5 = np.where(is_second, c_u2[c], c_u1[c]).astype(np.int64)
        paired = t_pair[tmpl]
        flag = np.where(paired, 0x1 | np.where(is_second, 0x80, 0x40) | np.where(rev, 0x10, 0x20), np.where(rev, 0x10, 0)).astype(np.uint16)
        flag[k:] = (flag[k:] & 0x10) | rng.choice(np.array([0x100, 0x800, 0x4, 0x100 | 0x400], np.uint16), extra)
        m = rng.integers(1, 4, n).astype(np.int64)
        clip = rng.choice(np.array([0, 0, 0, 0, 1, 2], np.int64), n)
        hard = rng.random(n) < 0.3
        pos = np.where(rev, u5 - m + 1 - clip, u5 + clip)
        # a random order of the batch; mates by their new indices
        slot = rng.permutation(n)
        mate = np.full(n, -1, np.int64)
        read1 = np.full(len(cls), -1, np.int64)
        read1[first] = first
        mate[len(first):k] = read1[second]
        mate[second] = len(first) + np.arange(len(second))
        lone = np.nonzero(paired[:k] & (rng.random(k) < 0.01))[0]     # pairs whose reads name no mate: two fragments
        mate[mate[lone]] = -1
        mate[lone] = -1
        inv = np.empty(n, np.int64)
        inv[slot] = np.arange(n)                                      # inv[new index] = old index
        new_of = slot
        self.n, self.n_lib, self.n_ref = n, n_lib, n_ref
        self.flag, self.ref_id, self.pos = flag[inv], c_ref[c][inv].astype(np.int32), pos[inv].astype(np.int32)
        self.lib = c_lib[c][inv].astype(np.int32)
        old_mate = mate[inv]
        self.mate = np.where(old_mate >= 0, new_of[np.maximum(old_mate, 0)], -1).astype(np.int32)
        self.m, self.clip, self.hard, self.rev = m[inv], clip[inv], hard[inv], rev[inv]
        sk = self.clip > 0
        w = np.zeros((n, 3), np.uint32)
        cw = (self.clip << 4) | np.where(self.hard, 5, 4)
        w[:, 0], w[:, 1], w[:, 2] = cw, (self.m << 4) | 0, cw
        keep = np.stack([sk & ~self.rev, np.ones(n, bool), sk & self.rev], axis=1)
        self.cigar = w[keep]
        self.cigar_off = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
        self.n_qual = self.m + np.where(self.hard, 0, self.clip)
        self.qual_off = np.concatenate([[0], np.cumsum(self.n_qual)]).astype(np.int64)
        self.qual = rng.choice(np.array([2, 14, 15, 20, 30, 40], np.uint8), int(self.qual_off[-1]))

    def arrays(self):
        return (self.flag, self.ref_id, self.pos, self.mate, self.lib, self.cigar, self.cigar_off, self.qual, self.qual_off)

    def records(self):
        out = []
        for r in range(self.n):
            words = self.cigar[self.cigar_off[r]:self.cigar_off[r + 1]]
            cigar = "".join(f"{int(x) >> 4}{M.OPS[int(x) & 15]}" for x in words)
            out.append(dict(flag=int(self.flag[r]), ref=int(self.ref_id[r]), pos=int(self.pos[r]), cigar=cigar,
                            qual=self.qual[self.qual_off[r]:self.qual_off[r + 1]].tobytes(), mate=int(self.mate[r]),
                            lib=int(self.lib[r])))
        return out


def markdup_np(f):
    """DESIGN §2 "Mark duplicates" on a FlatDup batch: (dup[n] uint8, stats)."""
    n = f.n
    idx = np.arange(n)
    flag = f.flag.astype(np.int64)
    examined = (flag & (M.UNMAPPED | M.SECONDARY | M.SUPPLEMENTARY)) == 0
    rev = (flag & M.REVERSE) != 0
    # the unclipped 5' position: the leading clips of a forward read, the trailing ones of a reverse read
    u5 = np.where(rev, f.pos.astype(np.int64) + f.m - 1 + f.clip, f.pos.astype(np.int64) - f.clip)
    q = f.qual.astype(np.int64)
    score = np.bincount(np.repeat(idx, f.n_qual), weights=np.where(q >= 15, q, 0), minlength=n).astype(np.int64)
    mate = f.mate.astype(np.int64)
    has = mate >= 0
    m0 = np.maximum(mate, 0)
    paired = examined & ((flag & M.PAIRED) != 0) & ((flag & M.MATE_UNMAPPED) == 0) & has & examined[m0]
    dup = np.zeros(n, np.uint8)
    # pairs: the record with the lower index stands for the pair
    lead = paired & (mate > idx) & paired[m0] & (f.mate[m0] == idx)
    i = idx[lead]
    j = mate[lead]
    ei = np.stack([f.ref_id[i], u5[i], rev[i], i], axis=1).astype(np.int64)
    ej = np.stack([f.ref_id[j], u5[j], rev[j], j], axis=1).astype(np.int64)
    less = np.zeros(len(i), bool)
    tie = np.ones(len(i), bool)
    for col in range(4):
        less |= tie & (ei[:, col] < ej[:, col])
        tie &= ei[:, col] == ej[:, col]
    lo, hi = np.where(less[:, None], ei, ej), np.where(less[:, None], ej, ei)
    lib = f.lib[lo[:, 3]].astype(np.int64)
    total = score[i] + score[j]
    order = np.lexsort((i, -total, hi[:, 2], hi[:, 1], hi[:, 0], lo[:, 2], lo[:, 1], lo[:, 0], lib))
    key = np.stack([lib, lo[:, 0], lo[:, 1], lo[:, 2], hi[:, 0], hi[:, 1], hi[:, 2]], axis=1)[order]
    first = np.ones(len(order), bool)
    first[1:] = (key[1:] != key[:-1]).any(axis=1)
    lost = order[~first]
    dup[i[lost]] = 1
    dup[j[lost]] = 1
    # fragments: per (library, contig, unclipped 5' position, strand) of the examined records
    e = idx[examined]
    order = np.lexsort((e, -score[e], paired[e], rev[e], u5[e], f.ref_id[e], f.lib[e]))
    s = e[order]
    key = np.stack([f.lib[s], f.ref_id[s], u5[s], rev[s]], axis=1).astype(np.int64)
    first = np.ones(len(s), bool)
    first[1:] = (key[1:] != key[:-1]).any(axis=1)
    gid = np.cumsum(first) - 1
    any_paired = np.bincount(gid, weights=paired[s], minlength=gid[-1] + 1) > 0
    flagged = ~paired[s] & (any_paired[gid] | ~first)      # the unpaired come first in a group, the best of them first
    dup[s[flagged]] = 1
    stats = dict(examined=int(examined.sum()), pairs=int(lead.sum()), fragments=int((examined & ~paired).sum()),
                 duplicates=int(dup.sum()))
    return dup, stats


def markdup_sets(f, dup):
    """The index spans (lowest, highest member) of the fragment groups that hold a marked record."""
    flag = f.flag.astype(np.int64)
    rev = (flag & M.REVERSE) != 0
    u5 = np.where(rev, f.pos.astype(np.int64) + f.m - 1 + f.clip, f.pos.astype(np.int64) - f.clip)
    e = np.nonzero((flag & (M.UNMAPPED | M.SECONDARY | M.SUPPLEMENTARY)) == 0)[0]
    order = np.lexsort((e, rev[e], u5[e], f.ref_id[e], f.lib[e]))
    s = e[order]
    key = np.stack([f.lib[s], f.ref_id[s], u5[s], rev[s]], axis=1).astype(np.int64)
    first = np.ones(len(s), bool)
    first[1:] = (key[1:] != key[:-1]).any(axis=1)
    starts = np.nonzero(first)[0]
    lo, hi = np.minimum.reduceat(s, starts), np.maximum.reduceat(s, starts)
    marked = np.add.reduceat(dup[s].astype(np.int64), starts) > 0
    return lo[marked], hi[marked]


# ------------------------------------------------------------------ markdup: the high bits of the keys
MD_MAX_REFS, MD_MAX_LIBS = (1 << 21) - 1, (1 << 11) - 1


def _md_read(flag, lib, ref, u5, rev, q):
    """One base at the unclipped 5' position u5: hard clips carry a u5 that its position cannot."""
    if rev:
        pos, cigar = max(u5, 0), "1M"
        assert u5 >= 0
    elif u5 < 0:
        left, pos, ops = -u5, 0, []
        while left:
            k = min(left, (1 << 28) - 1)
            ops.append(f"{k}H")
            left -= k
        cigar = "".join(ops) + "1M"
    else:
        pos, cigar = u5, "1M"
    return M.rec(flag | (M.REVERSE if rev else 0), ref, pos, cigar, q, lib=lib)


def markdup_high_bits():
    """64 templates (fragments and pairs) whose keys are equal or differ in exactly one field, in the top bits of the 11-bit
    library, the 21-bit contig and the 31-bit u5 fields: the records, with mates as batch indices."""
    libs, refs = [0, 1, 1 + (1 << 10), 2046], [0, 1, 1 + (1 << 20), MD_MAX_REFS - 2]
    u5s = [-((1 << 30) - 1), -1, 0, 5, 5 + (1 << 29), (1 << 30) - 1]
    out, templates = [], 0

    def frag(lib, ref, u5, rev, q):
        nonlocal templates
        out.append(_md_read(0, lib, ref, u5, rev, q))
        templates += 1

    def pair(lib, a, b, q):
        """a, b: (ref, u5, rev) of read 1 and read 2."""
        nonlocal templates
        i = len(out)
        r1 = _md_read(M.PAIRED | M.READ1 | (M.MATE_REVERSE if b[2] else 0), lib, *a, q)
        r2 = _md_read(M.PAIRED | M.READ2 | (M.MATE_REVERSE if a[2] else 0), lib, *b, q)
        out.extend(M.pair(i, r1, r2))
        templates += 1

    # fragments: a base key twice, and twice each key that differs from it in one field's top bit, low bit or strand
    for lib, ref, u5, rev in ((1, 1, 5, False), (1 + (1 << 10), 1, 5, False), (1, 1 + (1 << 20), 1, False), (1, 1 + (1 << 20), 5, False),
                              (1, 1, 5 + (1 << 29), False), (1, 1, 5, True), (0, 1, 5, False), (1, 0, 5, False), (1, 1, 0, False),
                              (2046, MD_MAX_REFS - 2, (1 << 30) - 1, True), (2046, MD_MAX_REFS - 2, -((1 << 30) - 1), False),
                              (0, 0, -((1 << 30) - 1), False), (0, 0, -1, False), (1, 1, -1, False), (2046, 0, 0, False)):
        frag(lib, ref, u5, rev, 20)
        frag(lib, ref, u5, rev, 30)
    # pairs: the lesser end first in the key, the greater end second
    lo, hi = (1, 7, False), (1, 700, True)
    for lib, a, b in ((1, lo, hi), (1, lo, (1 + (1 << 20), 700, True)),        # the greater end's contig top bit
                      (1, (1, 7 + (1 << 29), False), (1, 5 + (1 << 29) + 700, True)),
                      (1, (1, 7 + (1 << 29), False), (1, 5 + (1 << 29) + 700 + (1 << 28), True)),
                      (1 + (1 << 10), lo, hi), (2046, lo, hi),                 # the library alone
                      (1, (0, 9, False), (MD_MAX_REFS - 2, (1 << 30) - 1, True)),
                      (1, (0, -((1 << 30) - 1), False), (MD_MAX_REFS - 2, (1 << 30) - 1, True)),
                      (1, (1, 40, False), (2, 900, True)), (1, (1, 40 + (1 << 29), False), (2, 900, True))):   # the lesser end's u5 top bit
        pair(lib, a, b, 20)
        pair(lib, b, a, 30)                                                    # read 2 is the lesser end: the same key
    eq = ((1 + (1 << 20), 11 + (1 << 29), False), (MD_MAX_REFS - 2, (1 << 30) - 1, True))
    for q in (20, 30, 30, 25):      # equal in all 117 bits: the scores decide, then the lower index
        pair(1 + (1 << 10), *eq, q)
    while templates < 64:
        frag(libs[templates % 4], refs[templates % 4], u5s[templates % 6], u5s[templates % 6] >= 0 and templates % 2 == 1, 20 + templates % 3)
    return out


def markdup_appended(base, tail):
    """tail's records behind base's, their mates moved along."""
    return base + [dict(r, mate=r["mate"] + len(base) if r["mate"] >= 0 else -1) for r in tail]


# ------------------------------------------------------------------ bqsr
def bq_world():
    return B.random_world()


def bq_tables(n_rg, seed=91):
    """base, dctx, dcyc in multiples of 1 / 8: base near q, the deltas within 3 of it."""
    rng = np.random.default_rng(seed)
    base = np.arange(B.NQ, dtype=np.float64)[None, :] + rng.integers(-24, 25, (n_rg, B.NQ)) / 8.0
    dctx = rng.integers(-24, 25, (n_rg, B.NQ, B.NCTX)) / 8.0
    dcyc = rng.integers(-24, 25, (n_rg, B.NQ, B.NCYC)) / 8.0
    return base, dctx, dcyc


def bq_count_case(refs, known, n, n_rg, seed, lengths):
    """(records in the generator's order, the same grouped by read group as the commands flatten them, ctx, cyc)."""
    records = B.random_batch(seed=seed, n=n, n_rg=n_rg, refs=refs, lengths=lengths)
    ctx, cyc = B.new_tables(n_rg)
    B.count(records, refs, known, n_rg, ctx, cyc)
    return records, sorted(records, key=lambda r: r["rg"]), ctx, cyc


def bq_check_batch(n_rg=3):
    """bq_arrays of 524,549 one-base records; record 524,300 names read group n_rg."""
    n = SHAPES["bq_check"]
    rng = np.random.default_rng(95)
    rg = rng.integers(0, n_rg, n).astype(np.int32)
    rg[CAPS["bq_max_blocks"] * 256 + 12] = n_rg
    off = np.arange(n + 1, dtype=np.int64)
    return (np.zeros(n, np.uint16), np.zeros(n, np.int32), rng.integers(0, 5000, n).astype(np.int32), np.full(n, 60, np.uint8), rg,
            np.full(n, (1 << 4) | 0, np.uint32), off, rng.choice(np.frombuffer(b"ACGT", np.uint8), n), np.full(n, 30, np.uint8), off,
            np.zeros(n, np.uint8))
