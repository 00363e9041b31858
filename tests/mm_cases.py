"""The Python restatement of DESIGN §2 [EXT] "minimizer seeding and chaining"
(sketch, anchors, the chaining recurrence, backtrack), written from that text
and not from the C++, and the case builders that test_chain_cpu.py and
test_chain_gpu.py share.  Integers only."""
import ctypes as C

import numpy as np

K, W = 21, 11
MAX_GAP, BW, MIN_CNT, MIN_SCORE = 100, 50, 2, 20
LOOKBACK = 64


# ------------------------------------------------------------------ sketch
def codes(seq):
    return np.array([{"A": 0, "C": 1, "G": 2, "T": 3}.get(c, 4) for c in seq.upper()], np.uint8)


def revcomp(seq):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(c, "N") for c in reversed(seq.upper()))


def hash64(key, mask):
    key = (~key + (key << 21)) & mask
    key = key ^ key >> 24
    key = ((key + (key << 3)) + (key << 8)) & mask
    key = key ^ key >> 14
    key = ((key + (key << 2)) + (key << 4)) & mask
    key = key ^ key >> 28
    key = (key + (key << 31)) & mask
    return key


def kmers(seq, k):
    """Per position i (the k-mer's last base): None when the k bases ending at i hold a non-ACGT base (or i < k - 1),
    'skip' for a k-mer equal to its reverse complement, else (hash, strand)."""
    c = codes(seq)
    mask = (1 << (2 * k)) - 1
    out = [None] * len(c)
    for i in range(k - 1, len(c)):
        win = c[i - k + 1:i + 1]
        if (win > 3).any():
            continue
        fwd = rc = 0
        for b in win:
            fwd = fwd << 2 | int(b)
        for b in win[::-1]:
            rc = rc << 2 | (3 - int(b))
        out[i] = "skip" if fwd == rc else (hash64(min(fwd, rc), mask), 0 if fwd < rc else 1)
    return out


def sketch(seq, k=K, w=W):
    """[(hash, pos, strand)] in ascending pos: every k-mer that has the smallest hash of some window of w consecutive
    positions that all hold a k-mer (skipped ones never win); equal minima of a window are all selected; each once."""
    km = kmers(seq, k)
    chosen = set()
    for e in range(w - 1, len(km)):
        win = range(e - w + 1, e + 1)
        if any(km[i] is None for i in win):
            continue
        vals = [km[i][0] for i in win if km[i] != "skip"]
        if not vals:
            continue
        m = min(vals)
        chosen.update(i for i in win if km[i] != "skip" and km[i][0] == m)
    return [(km[i][0], i, km[i][1]) for i in sorted(chosen)]


def index(contigs, k=K, w=W):
    """{hash: [(contig, pos, strand)]} in (contig, pos) order."""
    idx = {}
    for c, seq in enumerate(contigs):
        for h, pos, s in sketch(seq, k, w):
            idx.setdefault(h, []).append((c, pos, s))
    return idx


def anchors(idx, read, k=K, w=W, max_occ=500):
    """(t[], q[], (rep bases, L)) of a read: sorted by (t, q)."""
    L = len(read)
    out, rep = [], set()
    for h, pos, s in sketch(read, k, w):
        occ = idx.get(h, [])
        if len(occ) > max_occ:
            rep.update(range(pos - k + 1, pos + 1))
            continue
        for c, r, sr in occ:
            rev = int(s != sr)
            out.append((((c * 2 + rev) << 32) | r, L - pos + k - 2 if rev else pos))
    out.sort()
    return [a[0] for a in out], [a[1] for a in out], (len(rep), L)


# ------------------------------------------------------------------ chaining
def ilog2(v):
    return v.bit_length() - 1


def chain(t, q, max_gap=MAX_GAP, bw=BW, span=K):
    """(f[], p[]) of one read's sorted anchors."""
    n = len(t)
    f, p = [span] * n, [-1] * n
    for i in range(n):
        best, from_ = span, -1
        for j in range(max(0, i - LOOKBACK), i):
            dr, dq = t[i] - t[j], q[i] - q[j]
            if dr == 0 or dr > max_gap or dq <= 0 or dq > max_gap:
                continue
            dd = abs(dr - dq)
            if dd > bw:
                continue
            sc = f[j] + min(min(dq, dr), span) - ((dd * span) // 100 + ((ilog2(dd) >> 1) if dd else 0))
            if sc > span and sc >= best:  # the largest score, among equals the largest j; strictly above span
                best, from_ = sc, j
        f[i], p[i] = best, from_
    return f, p


def chain_batch(t, q, off, **kw):
    f, p = np.full(len(t), -7, np.int32), np.full(len(t), -7, np.int32)
    for r in range(len(off) - 1):
        a, b = int(off[r]), int(off[r + 1])
        fr, pr = chain([int(x) for x in t[a:b]], [int(x) for x in q[a:b]], **kw)
        f[a:b], p[a:b] = fr, pr
    return f, p


def backtrack(f, p, min_cnt=MIN_CNT, min_score=MIN_SCORE):
    """[(score, [anchors ascending])]: heads by descending f, among equal f the larger index first; follow p until -1
    or a used anchor; every anchor walked is used from then on, whether the chain is kept or not."""
    n = len(f)
    used = [False] * n
    out = []
    for h in sorted(range(n), key=lambda i: (-f[i], -i)):
        if used[h]:
            continue
        walk, i = [], h
        while i >= 0 and not used[i]:
            walk.append(i)
            used[i] = True
            i = p[i]
        score = f[h] - (f[i] if i >= 0 else 0)
        if len(walk) >= min_cnt and score >= min_score:
            out.append((score, walk[::-1]))
    return out


# ------------------------------------------------------------------ case builders
def flat(reads):
    """reads: [(t[], q[])] -> (t int64, q int32, off int64)."""
    t = np.array([x for r in reads for x in r[0]], np.int64)
    q = np.array([x for r in reads for x in r[1]], np.int32)
    off = np.cumsum([0] + [len(r[0]) for r in reads]).astype(np.int64)
    return t, q, off


def colinear_read(n, rng, t0=1000, span=K):
    """n sorted anchors along one diagonal with small random steps and occasional small indels, so that most chain."""
    t, q, tt, qq = [], [], t0, span - 1
    for _ in range(n):
        t.append(tt), q.append(qq)
        step = int(rng.integers(1, 30))
        tt, qq = tt + step + int(rng.choice([0, 0, 0, 1, 2, 5])), qq + step
    return t, q


def random_read(n, rng, contigs=2):
    """n anchors at random places of a few (contig, strand) groups: few chain; sorted by (t, q)."""
    a = sorted((((int(rng.integers(0, contigs * 2)) << 32) | int(rng.integers(0, 400))), int(rng.integers(0, 150))) for _ in range(n))
    return [x[0] for x in a], [x[1] for x in a]


def random_dna(n, rng):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def host_hooks(lib):
    """Types of libfcsgenome's fcsg_mm_* hooks."""
    lib.fcsg_mm_sketch.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.fcsg_mm_anchors.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_int, C.c_void_p]
    lib.fcsg_mm_chain.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.fcsg_mm_backtrack.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return lib


def host_sketch(H, seq, k=K, w=W):
    c = codes(seq)
    cap = len(c) + 1
    h, pos, st = np.zeros(cap, np.uint64), np.zeros(cap, np.int32), np.zeros(cap, np.uint8)
    n = H.check(H.lib.fcsg_mm_sketch(c.ctypes.data, len(c), k, w, h.ctypes.data, pos.ctypes.data, st.ctypes.data, cap))
    return [(int(h[i]), int(pos[i]), int(st[i])) for i in range(n)]


def host_anchors(H, contigs, read, k=K, w=W, max_occ=500, cap=1 << 16):
    ref = np.concatenate([codes(s) for s in contigs])
    off = np.cumsum([0] + [len(s) for s in contigs]).astype(np.int64)
    rd = codes(read)
    t, q, frac = np.zeros(cap, np.int64), np.zeros(cap, np.int32), C.c_double(-1)
    n = H.check(H.lib.fcsg_mm_anchors(ref.ctypes.data, off.ctypes.data, len(contigs), rd.ctypes.data, len(rd), k, w, max_occ,
                                      t.ctypes.data, q.ctypes.data, cap, C.addressof(frac)))
    return t[:n].copy(), q[:n].copy(), frac.value


def host_chain_entry(H, threads=2):
    """An `entry` for fcship.mm_chain that runs mm_chain_host."""
    return lambda b, f, p: H.check(H.lib.fcsg_mm_chain(b, threads, f, p))


def host_backtrack(H, f, p, min_cnt=MIN_CNT, min_score=MIN_SCORE):
    f, p = np.ascontiguousarray(f, np.int32), np.ascontiguousarray(p, np.int32)
    n = len(f)
    score, coff, anc = np.zeros(n + 1, np.int32), np.zeros(n + 2, np.int32), np.zeros(n + 1, np.int32)
    nc = H.check(H.lib.fcsg_mm_backtrack(f.ctypes.data, p.ctypes.data, n, min_cnt, min_score, score.ctypes.data, coff.ctypes.data,
                                         anc.ctypes.data, n + 1))
    return [(int(score[c]), [int(x) for x in anc[coff[c]:coff[c + 1]]]) for c in range(nc)]
