"""PairHMM batches larger than a launch's workgroup cap — a plain helper module.

Every forward and rescue launch of csrc/phmm_kernels.hip caps its grid; past
the cap a workgroup takes a second item of the class and must set up its LDS
rings, boundary columns, hap buffers and segment tables again.  The batches
here repeat a small set of unique (read, haplotype) pairs often enough that a
class exceeds its cap: the oracle runs on the unique pairs only and its answer
is tiled (`Case.tile`).

The caps are read from the source (`cap`), and the batch arithmetic of the
kernels (`stream_batches`, `launch_class`) is restated ONLY to assert that a
second trip happens and which pairs it holds; what is correct is decided by
the oracle alone.  The builders are pure functions of their arguments (fixed
seeds), so tests/test_grid_cases_cpu.py checks every coverage condition without
a GPU.
"""
from __future__ import annotations

import dataclasses
import functools
import os
import re

import numpy as np

import fcship
import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "falcon-genome_amd", "csrc")
ACGT = np.frombuffer(b"ACGT", np.uint8)


# ------------------------------------------------------------------ read from the source
@functools.lru_cache(maxsize=None)
def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def cap(file, name):
    """The value of `constexpr <int type> name = <int or a << b>;` in csrc/file."""
    m = re.search(r"constexpr (?:long long|int) %s = ([^;]+);" % re.escape(name), source(file))
    assert m, f"{name} not found in {file}"
    expr = m.group(1).strip()
    if "<<" in expr:
        a, b = expr.split("<<")
        return int(a) << int(b)
    return int(expr)


def stream_class_hmax():
    """phmm_stream.h stream_class_hmax(0..3)."""
    m = re.search(r"stream_class_hmax\(int c\) \{\s*return c == 0 \? (\d+) : c == 1 \? (\d+) : c == 2 \? (\d+) : (\d+);",
                  source("phmm_stream.h"))
    assert m, "stream_class_hmax changed its form"
    return [int(v) for v in m.groups()]


def cols_hmax():
    """phmm_cols.h cols_hmax(0..kColsLaunch-1), widest class first."""
    m = re.search(r"cols_C\(int c\) \{ return c == 0 \? (\d+) : (\d+) - c; \}", source("phmm_cols.h"))
    assert m, "cols_C changed its form"
    assert re.search(r"cols_hmax\(int c\) \{ return 16 \* cols_C\(c\) - 1; \}", source("phmm_cols.h"))
    c0, base = int(m.group(1)), int(m.group(2))
    n = cap("fcship_internal.h", "kColsLaunch")
    return [16 * (c0 if c == 0 else base - c) - 1 for c in range(n)]


def launch_class(R, H):
    """phmm_kernels.hip launch_phmm_forward: ('long', j), ('cols', c) or
    ('grouped', None) for a pair of read length R and haplotype length H."""
    if R < cap("phmm_stream.h", "kStreamMinR") or R > 0xFFFF:
        return ("grouped", None)
    sh, ch = stream_class_hmax(), cols_hmax()
    if H > sh[3]:
        return ("grouped", None)
    if H > sh[2]:
        return ("long", 0)
    if H > ch[0]:
        return ("long", 1)
    c = max(k for k in range(len(ch)) if H <= ch[k])
    return ("cols", c)


def stream_batches(count, K, tail, width):
    """(nb_head, nbatch) of phmm3_kernel / phmm5_kernel (width 4) and
    phmm4_kernel (width 8): K pairs per stream over the head, one per stream
    over the class's last `tail` pairs."""
    tailn = min(count, tail)
    headn = count - tailn
    per = width * K
    nb_head = -(-headn // per)
    return nb_head, nb_head + -(-tailn // width)


def phmm3_tail(j):
    """launch_phmm_forward: tail = 2 * 4 * 1024 * stream_class_waves(sc), one
    wave per SIMD for the longest class, two for H <= 472."""
    return 2 * 4 * 1024 * (1 if j == 0 else 2)


PHMM5_FORCED_TAIL = 4  # launch_phmm_forward: `cols1_forced_k() ? 4 : ...`
PHMM4_TAIL = 1024 * 3 * 8


def second_trip_pairs(count, K, tail, width, grid_cap):
    """How many of the class's last (shortest-haplotype) pairs lie in batches
    past the first grid trip."""
    nb_head, nbatch = stream_batches(count, K, tail, width)
    if nbatch <= grid_cap:
        return 0
    tailn = min(count, tail)
    if grid_cap >= nb_head:
        return count - (count - tailn) - (grid_cap - nb_head) * width
    return count - grid_cap * width * K


# ------------------------------------------------------------------ sequences
def rand_read(rng, R, n_frac=0.0):
    b = rng.choice(ACGT, R)
    if n_frac:
        b[rng.random(R) < n_frac] = ord("N")
    return [b, rng.integers(0, 60, R).astype(np.uint8), rng.integers(10, 60, R).astype(np.uint8),
            rng.integers(10, 60, R).astype(np.uint8), rng.integers(5, 40, R).astype(np.uint8)]


def mutated(rng, hap, R, sub=0.02):
    """R bases of `hap` from a random start, a few substituted; bytes of the
    haplotype outside ACGT are replaced so that the read stays ACGT."""
    start = int(rng.integers(0, max(1, len(hap) - R + 1)))
    r = np.array(hap[start:start + R], np.uint8)
    if r.size < R:
        r = np.concatenate([r, rng.choice(ACGT, R - r.size)])
    m = (rng.random(R) < sub) | ~np.isin(r, ACGT)
    r[m] = rng.choice(ACGT, int(m.sum()))
    return r


def high_quality(rd):
    """Base quality 40, gap open 60: an unrelated read underflows the fp32 pass."""
    rd[1][:] = 40
    rd[2][:] = rd[3][:] = 60
    return rd


def odd_bytes(h, step):
    """IUPAC and lower-case bytes: the haplotype takes the byte-compare path."""
    h = h.copy()
    h[::step] = np.resize(np.frombuffer(b"RYacgtMK", np.uint8), h[::step].size)
    return h


# ------------------------------------------------------------------ cases
@dataclasses.dataclass(eq=False)
class Case:
    """reads, haps and the unique pairs [(read, hap)]; sel[i] is the unique
    pair that pair i of the large batch repeats.  kind[u] of a unique pair: a
    set of 'odd_r', 'even_r', 'min_r', 'read_n', 'hap_n', 'unrelated',
    'odd_hap'."""
    reads: list
    haps: list
    unique: list
    kinds: list
    sel: np.ndarray

    def unique_pairs(self):
        return fcship.make_pairs(self.reads, self.haps, pairs=self.unique)

    def pairs(self):
        pu = self.unique_pairs()
        return dataclasses.replace(pu, pair_read=np.ascontiguousarray(pu.pair_read[self.sel]),
                                   pair_hap=np.ascontiguousarray(pu.pair_hap[self.sel]))

    @functools.cached_property
    def oracle(self):
        """(log10, used_d) of the unique pairs."""
        return oracle_lib.phmm_batch(self.unique_pairs())

    def tile(self, per_unique):
        return np.asarray(per_unique)[self.sel]

    def hap_len(self):
        hl = np.array([len(h) for h in self.haps])
        return hl[np.array([h for _, h in self.unique])]

    def read_len(self):
        rl = np.array([len(r[0]) for r in self.reads])
        return rl[np.array([r for r, _ in self.unique])]


STREAM_R = [33, 34, 40, 47, 48, 55, 63, 64, 65, 72, 79, 80]


def _related_pairs(rng, case_reads, unique, kinds, haps, h, rs, extra=()):
    for R in rs:
        rd = rand_read(rng, R)
        rd[0] = mutated(rng, haps[h], R)
        k = {"odd_r" if R & 1 else "even_r", *extra}
        if R == 33:
            k.add("min_r")
        unique.append((len(case_reads), h))
        kinds.append(k)
        case_reads.append(tuple(rd))


def _special_pairs(rng, case_reads, unique, kinds, haps, h, extra=()):
    """A read with N bases and an unrelated high-quality read on haplotype h."""
    rd = rand_read(rng, 58)
    rd[0] = mutated(rng, haps[h], 58)
    rd[0][[3, 30, 57]] = ord("N")
    unique.append((len(case_reads), h))
    kinds.append({"read_n", "even_r", *extra})
    case_reads.append(tuple(rd))
    for R in (45, 60):
        rd = high_quality(rand_read(rng, R))
        unique.append((len(case_reads), h))
        kinds.append({"unrelated", "odd_r" if R & 1 else "even_r", *extra})
        case_reads.append(tuple(rd))


@functools.lru_cache(maxsize=None)
def stream_case(hlo, hhi, n_pairs, seed):
    """n_pairs pairs of one launch class, H in [hlo, hhi] and R in 33..80.
    A quarter of them share the shortest length hlo, the class's last in the
    longest-first schedule: three haplotypes (plain, with N, with bytes outside
    ACGTN), each under reads of every length of STREAM_R, a read with N and two
    unrelated high-quality reads.  The rest spread over seven longer
    haplotypes."""
    rng = np.random.default_rng(seed)
    haps = [rng.choice(ACGT, hlo) for _ in range(3)]
    haps[1][5::37] = ord("N")
    haps[2] = odd_bytes(haps[2], 9)
    for H in np.linspace(hlo + 1, hhi, 7).astype(int):
        haps.append(rng.choice(ACGT, int(H)))
    haps[5][7::41] = ord("N")
    reads, unique, kinds = [], [], []
    for h in range(len(haps)):
        extra = {1: ("hap_n",), 2: ("odd_hap",), 5: ("hap_n",)}.get(h, ())
        _related_pairs(rng, reads, unique, kinds, haps, h, STREAM_R, extra)
        if h < 4:
            _special_pairs(rng, reads, unique, kinds, haps, h, extra)
    short = np.array([u for u, (_, h) in enumerate(unique) if h < 3], np.int32)
    rest = np.array([u for u, (_, h) in enumerate(unique) if h >= 3], np.int32)
    idx = np.arange(n_pairs)
    is_short = idx % 4 == 3
    sel = np.empty(n_pairs, np.int32)
    sel[is_short] = short[np.arange(int(is_short.sum())) % short.size]
    sel[~is_short] = rest[np.arange(int((~is_short).sum())) % rest.size]
    return Case(reads, haps, unique, kinds, sel)


def stream_counts():
    """Pair counts of the streamed cases from the parsed cap: K = 1 makes the
    batches past 4 x cap a ragged second trip (1203 pairs); K = 2 and the packed
    column kernel (8 pairs per batch at K = 1) need cap + 64 head batches."""
    g = cap("phmm_kernels.hip", "kStreamGridCap")
    return {"k1": 4 * g + 1200 + 3, "k2": 8 * (g + 64) + phmm3_tail(1) + 8 * 300 + 5,
            "packed": 8 * (g + 64) + PHMM4_TAIL + 8 * 300 + 5}


LONG1 = (320, 460)   # inside (303, 472], launch class ('long', 1)
LONG0 = (480, 700)   # inside (472, 3700], launch class ('long', 0)
COLS = (192, 207)    # column class C = 13


def phmm3_case(which):
    """'k1' / 'k2': launch class ('long', 1) for FCSHIP_STREAM_K = 1 / 2;
    'k1_long0': launch class ('long', 0) for K = 1."""
    n = stream_counts()
    if which == "k1":
        return stream_case(*LONG1, n["k1"], 3301)
    if which == "k2":
        return stream_case(*LONG1, n["k2"], 3302)
    assert which == "k1_long0"
    return stream_case(*LONG0, n["k1"], 3303)


def cols_case():
    """One column class, enough pairs for phmm4's eight-pair batches at K = 1
    (phmm5's four-pair batches then make more than two trips)."""
    return stream_case(*COLS, stream_counts()["packed"], 3304)


@functools.lru_cache(maxsize=None)
def fallback_case():
    """More haplotypes with bytes outside ACGTN than the fallback pass's
    groups take in one trip (4 pairs each), plus a ragged remainder, mixed one
    to one with clean pairs; H in two column classes and one long class; some
    handed-back pairs are unrelated high-quality reads (fallback, then rescue)."""
    g = cap("phmm_kernels.hip", "kFallbackGroups")
    n_odd = 4 * g + 4 * 37 + 3
    rng = np.random.default_rng(3305)
    haps = []
    for H in (180, 250, 350):
        haps.append(rng.choice(ACGT, H))
        haps.append(odd_bytes(rng.choice(ACGT, H), 7 + len(haps)))
    haps[0][11::29] = ord("N")
    reads, unique, kinds = [], [], []
    for h in range(len(haps)):
        extra = ("odd_hap",) if h & 1 else ()
        _related_pairs(rng, reads, unique, kinds, haps, h, STREAM_R, extra)
        _special_pairs(rng, reads, unique, kinds, haps, h, extra)
    odd = np.array([u for u, k in enumerate(kinds) if "odd_hap" in k], np.int32)
    clean = np.array([u for u, k in enumerate(kinds) if "odd_hap" not in k], np.int32)
    n = 2 * n_odd + 1
    sel = np.empty(n, np.int32)
    sel[1::2] = odd[np.arange(n_odd) % odd.size]
    sel[0::2] = clean[np.arange(n_odd + 1) % clean.size]
    return Case(reads, haps, unique, kinds, sel)


RESCUE_R = (1, 2, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 70)
RESCUE_H = (1, 7, 16, 40, 64, 65, 80)


@functools.lru_cache(maxsize=None)
def rescue_case():
    """Tiny pairs (R 1..70 on both sides of 64, H 1..80 and a haplotype with a
    byte outside ACGTN), more of them than the 64-lane rescue's waves: with
    the threshold above every fp32 sum each one is rescued, one per wave."""
    g = cap("phmm_kernels.hip", "kRescueWaves")
    rng = np.random.default_rng(3306)
    reads = [tuple(rand_read(rng, R)) for R in RESCUE_R]
    haps = [rng.choice(ACGT, H) for H in RESCUE_H] + [np.frombuffer(b"ACGTNACGRT", np.uint8)]
    unique = [(r, h) for r in range(len(reads)) for h in range(len(haps))]
    kinds = [set() for _ in unique]
    return Case(reads, haps, unique, kinds, (np.arange(g + 77) % len(unique)).astype(np.int32))


def rescue_reference(case):
    """GKL's rescue value per unique pair: log10 of the oracle's fp64 forward
    sum minus log10(2^1020)."""
    with np.errstate(divide="ignore"):
        return np.array([np.log10(oracle_lib.phmm_prob_d(case.reads[r], case.haps[h])) - np.log10(2.0 ** 1020)
                         for r, h in case.unique])
