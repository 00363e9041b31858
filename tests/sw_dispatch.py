"""Banded-SW kernel selection restated in Python, and the task builders of
tests/test_bsw_dispatch_gpu.py — a plain helper module.

The three Smith-Waterman entry points pick a kernel per task, per wave or per
launch from arithmetic on the scoring matrix, gap costs, lengths, band and h0.
The restatements below mirror those predicates and are used ONLY to assert
coverage: that a builder's batch holds tasks on each side of each edge, or a
wave of a given kind.  What is correct is decided by the oracle alone
(oracle_lib), never by this module.  If a kernel change moves an edge the
parity tests still hold; only the coverage assertions (and the restatement
here) need updating.

The builders are pure functions of their arguments (fixed seeds), so
tests/test_sw_dispatch_cpu.py checks every coverage condition without a GPU.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

KSW_XBYTE, KSW_XSTOP, KSW_XSUBO, KSW_XSTART = 0x10000, 0x20000, 0x40000, 0x80000
X_RESCUE = KSW_XSUBO | KSW_XSTART | 19  # mem_matesw's xtra without the width bit


# ------------------------------------------------------------------ matrices
def mat_abn(a, b, n):
    """5 x 5 matrix: match a, mismatch b, N row and column n (values as given)."""
    m = np.full((5, 5), n, np.int8)
    for i in range(4):
        for j in range(4):
            m[i, j] = a if i == j else b
    return m.ravel()


DEFAULT_MAT = mat_abn(1, -4, -1)


def asym_mat(seed=7):
    """An asymmetric random matrix, entries in [-12, 6], positive diagonal."""
    rng = np.random.default_rng(seed)
    m = rng.integers(-12, 0, 25).astype(np.int8)
    m[[0, 6, 12, 18]] = rng.integers(1, 7, 4)
    m[rng.integers(0, 25, 3)] = rng.integers(0, 7, 3)  # a few non-negative off-diagonal entries
    m[[0, 6, 12, 18]] = np.maximum(m[[0, 6, 12, 18]], 1)
    return m


ALIGN_MATS = {
    "default": mat_abn(1, -4, -1),
    "2_8_2": mat_abn(2, -8, -2),
    "3_5_1": mat_abn(3, -5, -1),
    "5_16_1": mat_abn(5, -16, -1),
    "15_16_3": mat_abn(15, -16, -3),
    "1_1_0": mat_abn(1, -1, 0),
    "asym": asym_mat(),
}


# ------------------------------------------------------------------ restated predicates
def to_params(mat, o_del=6, e_del=1, o_ins=6, e_ins=1, end_bonus=5, zdrop=100):
    """csrc/bsw_api.cpp to_params: the derived fields."""
    m = [int(v) for v in np.asarray(mat).ravel()]
    assert len(m) == 25
    p = SimpleNamespace(mat=m, o_del=o_del, e_del=e_del, o_ins=o_ins, e_ins=e_ins, end_bonus=end_bonus, zdrop=zdrop)
    p.max_mat = max(0, max(m))
    p.lane_ok = all(-16 <= v <= 15 for v in m)
    q4 = [m[t * 5 + c] for t in range(5) for c in range(4)]  # target rows A..N, query columns A..T
    p.pair_bias = -min(0, min(q4))
    p.pair_cg = max(0, max(q4)) + p.pair_bias + 1
    p.pair_ok = p.pair_cg <= 128 and e_del <= 16 and e_ins <= 16
    return p


PAIR_BUCKET0, WIDE_BUCKET = 10, 15  # csrc/fcship_internal.h kBswPairBucket0, kBswWideBucket


def query_acgt(q, p):
    """csrc/bsw_lane.hip bsw_keys_kernel: the `acgt` argument of bsw_bucket."""
    return bool(p.pair_ok and len(q) < 152 and all(int(c) < 4 for c in q))


def bound_of(qlen, h0, p):
    return h0 + qlen * p.max_mat


def bsw_bucket(qlen, tlen, h0, acgt, p):
    """csrc/bsw_lane.hip bsw_bucket."""
    bound = bound_of(qlen, h0, p)
    need = qlen + 1
    if p.pair_ok and acgt and h0 > 0 and need <= 152 and tlen < 1024 and bound + p.pair_cg - 1 <= 255:
        return PAIR_BUCKET0 + (0 if need <= 32 else 1 if need <= 64 else 2 if need <= 96 else 3 if need <= 128 else 4)
    if not p.lane_ok or h0 <= 0 or bound >= 32000:
        return WIDE_BUCKET
    if need <= 16:
        return 0
    if need <= 32:
        return 1
    if need <= 48:
        return 2
    if need <= 64:
        return 3
    c = 4 if need <= 96 else 5 if need <= 128 else 6 if need <= 152 else -1
    if c < 0:
        return WIDE_BUCKET
    if bound < 256:
        return c + 3
    return WIDE_BUCKET if c == 6 else c


def extend_buckets(items, p):
    return [bsw_bucket(len(q), len(t), h0, query_acgt(q, p), p) for q, t, h0, _ in items]


GLANE_MAX_NB = 65  # csrc/bsw_kernels.hip kGLaneMaxNB


def glane_ok(qlen, tlen, w, mat_ok):
    """csrc/bsw_kernels.hip glane_ok."""
    nb = 2 * w + 1
    return bool(mat_ok and w >= 2 and nb <= GLANE_MAX_NB and qlen >= nb and tlen >= 3 and
                4 * ((nb + 7) >> 3) * tlen + 3 <= nb * tlen)


def glane_span(qlen, tlen, p):
    return (qlen + tlen + 2) * (max(p.e_del, p.e_ins) + 16) + p.o_del + p.o_ins


def glane_u16_ok(qlen, tlen, p):
    """csrc/bsw_kernels.hip glane_u16_ok."""
    return glane_span(qlen, tlen, p) <= 8000


def global_waves(items, p):
    """csrc/bsw_kernels.hip bsw_global_lane_kernel: per 64-task wave, the
    number of lane-path tasks, of wave-path tasks, the NB class of the launch
    that runs the wave's lane tasks (17 / 33 / 65, None without any), the NB
    classes its lane tasks would have alone, and the row form (u16)."""
    out = []
    for s in range(0, len(items), 64):
        ws = items[s:s + 64]
        ok = [glane_ok(len(q), len(t), w, p.lane_ok) for q, t, _, w in ws]
        nbs = [2 * w + 1 for (q, t, _, w), o in zip(ws, ok) if o]
        cls = lambda nb: 17 if nb <= 17 else 33 if nb <= 33 else 65
        u16 = all(glane_u16_ok(len(q), len(t), p) for (q, t, _, w), o in zip(ws, ok) if o)
        out.append(SimpleNamespace(lane=sum(ok), wave=len(ws) - sum(ok), nb=cls(max(nbs)) if nbs else None,
                                   classes={cls(nb) for nb in nbs}, u16=u16 if nbs else None,
                                   over=sum(1 for (q, t, _, w), o in zip(ws, ok)
                                            if o and not glane_u16_ok(len(q), len(t), p))))
    return out


ALIGN_SEG_Q = 160  # csrc/bsw_align.hip kAlignSegQ


def align_packed_big(mmax, e_ins):
    """csrc/bsw_align.hip align_packed_big."""
    return mmax + 2 + 159 * e_ins


def align_i16_mmax(max_mat):
    """csrc/bsw_align.hip align_i16_mmax."""
    return ALIGN_SEG_Q * max(max_mat, 0)


def align_packed_ok(mmax, blocks, o_ins, e_ins):
    """csrc/bsw_align.hip align_packed_ok."""
    return (o_ins >= 0 and 0 <= e_ins <= 200 and mmax <= 8192 and
            blocks * align_packed_big(mmax, e_ins) + o_ins + 1 < 32768)


def align_shift(mat):
    """The u8 bias, csrc/bsw_align.hip bsw_align_kernel / launch_bsw_align (bwa's ksw_qinit)."""
    mn = min(127, min(int(v) for v in np.asarray(mat).ravel()))
    return (256 - (mn & 0xFF)) & 0xFF


def align_supported(mat):
    """csrc/bsw_align.hip launch_bsw_align: mx + shift <= 255."""
    return max(int(v) for v in np.asarray(mat).ravel()) + align_shift(mat) <= 255


def align_plan(qlens, tlens, xtras, p):
    """csrc/bsw_align.hip launch_bsw_align and the per-wave split of
    bsw_align_kernel.  kernel[k]: 'pk' (packed 16-lane), 'w16' (32-bit
    16-lane) or 'w64' (64-lane); waves: for each group of four consecutive
    tasks, 'u8' / 'i16' / 'mixed' by the widths of its 16-lane tasks (None
    when it holds none), and whether the per-wave vote sends it to the packed
    launch."""
    n = len(qlens)
    mt = max(max(tlens, default=0), 1)
    per_group = 4 * ((mt + 1) // 2) + mt
    seg = 4 * per_group + 16 <= 160 * 1024
    seg_q = ALIGN_SEG_Q if seg else -1
    packed = seg and align_packed_ok(255, 16, p.o_ins, p.e_ins)
    packed16 = packed and align_packed_ok(align_i16_mmax(p.max_mat), 8, p.o_ins, p.e_ins)
    all_u8 = all(x & KSW_XBYTE for x in xtras)
    pk = 0 if (not packed or packed16) else 1  # the packed launch's pk; the 32-bit launch gets 2 when pk == 1
    second_launch = seg and not (packed and (all_u8 or packed16))
    kernel, waves = [None] * n, []
    for s in range(0, n, 4):
        ks = range(s, min(s + 4, n))
        m16 = [k for k in ks if qlens[k] <= seg_q]
        u8w = all(xtras[k] & KSW_XBYTE for k in m16)  # the __ballot: no 16-lane task of the wave is i16
        kinds = {bool(xtras[k] & KSW_XBYTE) for k in m16}
        waves.append(SimpleNamespace(kind=None if not m16 else "u8" if kinds == {True} else "i16" if kinds == {False}
                                     else "mixed", packed_launch=bool(m16) and packed and (pk == 0 or u8w),
                                     partial=len(ks) < 4))
        for k in ks:
            if qlens[k] > seg_q:
                kernel[k] = "w64"
            elif packed and (pk == 0 or u8w):
                kernel[k] = "pk"
            else:
                assert second_launch
                kernel[k] = "w16"
    return SimpleNamespace(seg=seg, packed=packed, packed16=packed16, pk=pk, all_u8=all_u8,
                           second_launch=second_launch, kernel=kernel, waves=waves)


# ------------------------------------------------------------------ task packing
def pack(items):
    """items [(q, t, h0, w)] as the arrays oracle_lib's batch calls read (the
    layout of fcship.make_tasks)."""
    ql = np.array([len(x[0]) for x in items], np.int32)
    tl = np.array([len(x[1]) for x in items], np.int32)
    qo = np.concatenate([[0], np.cumsum(ql[:-1], dtype=np.int64)]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum(tl[:-1], dtype=np.int64)]).astype(np.int64)
    qb = np.concatenate([np.asarray(x[0], np.uint8) for x in items])
    tb = np.concatenate([np.asarray(x[1], np.uint8) for x in items])
    return SimpleNamespace(qbuf=qb, qoff=qo, qlen=ql, tbuf=tb, toff=to, tlen=tl, n=len(items),
                           h0=np.array([x[2] for x in items], np.int32), w=np.array([x[3] for x in items], np.int32))


# ------------------------------------------------------------------ sequence generators
def related_pair(rng, qlen, tlen, sub=0.03, indel=0.01, n_frac=0.0):
    t = rng.integers(0, 4, tlen).astype(np.uint8)
    q = []
    i = 0
    while len(q) < qlen:
        u = rng.random()
        if u < indel / 2:
            q.append(int(rng.integers(0, 4)))
            continue
        if u < indel:
            i += 1
            continue
        b = int(t[i % tlen]) if tlen else int(rng.integers(0, 4))
        if rng.random() < sub:
            b = (b + 1 + int(rng.integers(0, 3))) & 3
        q.append(b)
        i += 1
    q = np.array(q[:qlen], np.uint8)
    if n_frac:
        q[rng.random(qlen) < n_frac] = 4
        t[rng.random(tlen) < n_frac] = 4
    return q, t


def align_items(seed, n, qmin=20, qmax=200, tmin=40, tmax=700, related=0.7, mut=0.04, copy=0.5):
    """Mate-rescue-shaped ksw_align2 tasks: a query that is (mostly) a mutated
    piece of its target window, sometimes twice (score2), sometimes unrelated."""
    rng = np.random.default_rng(seed)
    items = []
    for k in range(n):
        ql = int(rng.integers(qmin, qmax + 1))
        tl = int(rng.integers(tmin, tmax + 1))
        t = rng.integers(0, 4, tl).astype(np.uint8)
        if rng.random() < related and tl > 8:
            a = int(rng.integers(0, max(1, tl - ql // 2)))
            q, _ = related_pair(rng, ql, ql, sub=0.03, indel=0.01)
            piece = t[a:a + ql]
            q = piece.copy() if rng.random() < copy else q
            if len(q) > 4:
                for j in range(len(q)):
                    if rng.random() < mut:
                        q[j] = (q[j] + 1) % 4
            if rng.random() < 0.3 and tl > 2 * len(q) + 10:  # a second, weaker copy far away
                b = int(rng.integers(0, tl - len(q)))
                t[b:b + len(q)] = q
                t[b + len(q) // 2] = (t[b + len(q) // 2] + 1) % 4
        else:
            q = rng.integers(0, 4, ql).astype(np.uint8)
        if rng.random() < 0.05:
            q[int(rng.integers(0, len(q)))] = 4  # N
        items.append((np.asarray(q, np.uint8), t, 0, 0))
    return items


# ------------------------------------------------------------------ ksw_align2 builders
def align_matrix_runs(name):
    """About 200 mate-rescue-shaped tasks for one matrix of ALIGN_MATS and the
    four xtra runs: XBYTE on all, on none, mixed per task (XSUBO|XSTART|19),
    and XSTOP|40 with mixed widths."""
    seed = 700 + sorted(ALIGN_MATS).index(name)
    items = align_items(seed, 200, related=0.9, mut=0.01, copy=0.9)
    n = len(items)
    mixed = np.array([X_RESCUE | (KSW_XBYTE if k % 3 else 0) for k in range(n)], np.int32)
    stop = np.array([KSW_XSTOP | 40 | (KSW_XBYTE if k % 2 else 0) for k in range(n)], np.int32)
    runs = {"u8": np.full(n, X_RESCUE | KSW_XBYTE, np.int32), "i16": np.full(n, X_RESCUE, np.int32),
            "mixed": mixed, "stop": stop}
    return items, runs


def _embed(rng, q, tlen, at):
    t = rng.integers(0, 4, tlen).astype(np.uint8)
    t[at:at + len(q)] = q  # the whole query matches, so the flanks cannot add to the score
    return t


def exact_query(rng, L, mism=(), ns=()):
    """A query of L bases and a 3 L / 2 + 40 base target holding its exact copy,
    but for the query positions `mism` (mismatches) and `ns` (query N)."""
    q = rng.integers(0, 4, L).astype(np.uint8)
    t = _embed(rng, q, L + L // 2 + 40, 20)
    q = q.copy()
    for x in mism:
        q[x] = (q[x] + 1) % 4
    for x in ns:
        q[x] = 4
    return q, t


def align_saturation_cases():
    """u8 saturation (gmax + shift >= 255 -> score 255) in each u8 code path,
    with exact-match scores just below, at and above 255 - shift.  Each case:
    (name, path, mat, gaps, items, xtra, expected best local score per task)."""
    rng = np.random.default_rng(811)
    x8 = X_RESCUE | KSW_XBYTE
    cases = []
    # 64-lane kernel: default matrix (shift 4), exact matches of 250 (score 250 stays), 251, 252 ... 300 bases
    items, want = [], []
    for L in [249, 250, 251, 252, 253, 260, 275, 300] * 2:
        q, t = exact_query(rng, L)
        items.append((q, t, 0, 0))
        want.append(L)
    cases.append(("w64_default", "w64", DEFAULT_MAT, (6, 1, 6, 1), items, x8, want))
    # 16-lane kernels, a = 2 (shift 8, even scores: 246 stays, 248 saturates), qlen 125..160 and the edge 122..125
    m2 = mat_abn(2, -8, -2)
    items, want = [], []
    for L in [122, 123, 124, 125, 126, 130, 140, 150, 159, 160] * 2:
        q, t = exact_query(rng, L)
        items.append((q, t, 0, 0))
        want.append(2 * L)
    cases.append(("pk_a2", "pk", m2, (6, 1, 6, 1), items, x8, want))
    cases.append(("w16_a2_eins12", "w16", m2, (6, 1, 6, 12), items, x8, want))
    # a = 3, b = -5, N = -1 (shift 5): best scores 249, 250, 251 exactly: 83 matches; 85 matches around one
    # mismatch; 84 matches around one N
    m3 = mat_abn(3, -5, -1)
    items, want = [], []
    for rep in range(3):
        for L, mism, ns, sc in ((83, (), (), 249), (86, (40,), (), 250), (85, (), (41,), 251), (82, (), (), 246),
                                (84, (), (), 252), (120, (), (), 360)):
            q, t = exact_query(rng, L, mism, ns)
            items.append((q, t, 0, 0))
            want.append(sc)
    cases.append(("pk_a3", "pk", m3, (6, 1, 6, 1), items, x8, want))
    cases.append(("w16_a3_eins12", "w16", m3, (6, 1, 6, 12), items, x8, want))
    return cases


def align_i16_saturation_case():
    """Without XBYTE bwa's scores are 16-bit with saturating adds: exact
    matches of 200 .. 600 bases at match 127 and 100 put the best score below,
    next to and at 32767 (the 64-lane kernels; 160 bases x 127 stays far below
    it in the 16-lane ones).  Returns (mat, items, expected best score)."""
    rng = np.random.default_rng(812)
    out = []
    for a, b in ((127, -128), (100, -60)):
        items, want = [], []
        for L in (200, 241, 257, 258, 259, 300, 327, 328, 400, 600):
            for mism in ((), (L // 3,)):
                q, t = exact_query(rng, L, mism)
                items.append((q, t, 0, 0))
                # (a mismatch this heavy is bridged by an insertion next to a deletion: -(6 + 1) - (6 + 1))
                want.append(min(32767, a * (L - len(mism)) + max(b, -14) * len(mism)))
        out.append((mat_abn(a, b, -1), items, want))
    return out


# (max_mat, e_ins) just inside / outside packed16 (8 (160 max_mat + 2 + 159 e_ins) + o_ins + 1 < 32768)
PACKED16_EDGES = [(24, 1, True), (25, 1, False), (14, 11, True), (15, 11, False)]


def align_wave_split_case(max_mat, e_ins):
    """A batch whose groups of four tasks are all-u8, all-i16 and mixed (also a
    u8 group next to a long i16 task of the 64-lane launch), the last group
    partial; matrix (max_mat, -30, -5), gaps (6, 1, 6, e_ins)."""
    mat = mat_abn(max_mat, -30, -5)
    base = align_items(900 + max_mat + e_ins, 123, qmin=20, qmax=160, tmin=40, tmax=400, related=0.8)
    lng = align_items(950 + max_mat, 8, qmin=161, qmax=200, tmin=100, tmax=400, related=0.9)
    rng = np.random.default_rng(960 + max_mat)
    for k in range(0, len(base), 5):  # exact copies of 150 .. 160 bases: the largest 16-bit values of the 16-lane tasks
        q, t = exact_query(rng, 150 + (k // 5) % 11)
        base[k] = (q, t, 0, 0)
    patterns = ["uuuu", "iiii", "uiui", "uuui", "iuuu", "uuuI", "iiuu", "IuuU"]  # I / U: a 64-lane task
    items, xt = [], []
    b = l = 0
    g = 0
    while b < len(base):
        for c in patterns[g % len(patterns)]:
            if b >= len(base):
                break
            if c in "IU":
                items.append(lng[l % len(lng)])
                l += 1
            else:
                items.append(base[b])
                b += 1
            xt.append(X_RESCUE | (KSW_XBYTE if c in "uU" else 0))
        g += 1
    while len(items) % 4 != 3:  # a last partial group
        items.pop()
        xt.pop()
    return mat, (6, 1, 6, e_ins), items, np.array(xt, np.int32)


def align_gap_edge_case(gaps):
    """e_ins 11 / 12 with matrix (3, -5, -1), widths mixed per task."""
    items = align_items(990 + gaps[3], 160, qmax=200)
    xt = np.array([X_RESCUE | (KSW_XBYTE if k % 3 else 0) for k in range(len(items))], np.int32)
    return mat_abn(3, -5, -1), gaps, items, xt


ALIGN_GAP_EDGES = [(6, 1, 6, 11), (6, 1, 6, 12), (1, 3, 0, 11), (5, 1, 2, 12)]


# ------------------------------------------------------------------ ksw_global2 builders
GLOBAL_U16_MATS = {"1_16_16": mat_abn(1, -16, -16), "15_16_16": mat_abn(15, -16, -16)}
GLOBAL_U16_GAPS = [(6, 1, 6, 1), (30, 12, 30, 12), (4, 2, 9, 5)]


def u16_edge_total(p):
    """The largest qlen + tlen with span <= 8000 (by evaluating glane_span)."""
    s = 0
    while glane_span(s + 1, 0, p) <= 8000:
        s += 1
    return s


def global_contents(rng, qlen, tlen, kind):
    if kind == "same":  # identical but for the length difference: the highest scores
        t = rng.integers(0, 4, max(qlen, tlen)).astype(np.uint8)
        return t[:qlen].copy(), t[:tlen].copy()
    if kind == "homo":  # A against C: every cell a mismatch, the lowest scores
        return np.zeros(qlen, np.uint8), np.ones(tlen, np.uint8)
    return related_pair(rng, qlen, tlen, sub=0.05, indel=0.03, n_frac=0.01)


def global_u16_batches(mat_name, gaps):
    """Tasks at the u16 row form's edge: `inside` (span the largest value <=
    8000), `outside` (the smallest > 8000), and `one_over` (64-task waves of
    inside tasks holding a single outside one), w = 16 and w = 4."""
    p = to_params(GLOBAL_U16_MATS[mat_name], *gaps)
    tot = u16_edge_total(p)
    rng = np.random.default_rng(1200 + tot)
    out = {"inside": [], "outside": []}
    for side, total in (("inside", tot), ("outside", tot + 1)):
        for w in (16, 4):
            for kind in ("same", "homo", "related"):
                for d in (0, 1, -2, 3):  # qlen - tlen (+ the total's parity)
                    qlen = (total + d + 1) // 2
                    tlen = total - qlen
                    q, t = global_contents(rng, qlen, tlen, kind)
                    out[side].append((q, t, 1, w))
    one = []
    for wv in range(2):
        blk = [out["inside"][(k * 5 + wv) % len(out["inside"])] for k in range(64)]
        blk[(23, 63)[wv]] = out["outside"][wv * 7]
        one += blk
    out["one_over"] = one + out["inside"][:10]
    return p, out


GRID_W = [0, 1, 2, 8, 9, 16, 17, 32, 33]


def global_grid_items(seed=1300, reps=2):
    """glane_ok / NB-class edges: every (w, qlen, tlen) cell of the grid, in a
    fixed shuffled order so that 64-task waves mix lane-path and wave-path
    tasks and NB classes."""
    rng = np.random.default_rng(seed)
    items = []
    for w in GRID_W:
        nb = 2 * w + 1
        for qlen in sorted({max(1, nb - 1), nb, nb + 1}):
            for tlen in sorted({1, 2, 3, max(1, qlen - 3), qlen, qlen + 3}):
                for r in range(reps):
                    q, t = related_pair(rng, qlen, tlen, sub=0.05, indel=0.03 if r else 0.0,
                                        n_frac=0.02 if r else 0.0)
                    items.append((q, t, 1, w))
    order = np.random.default_rng(seed + 1).permutation(len(items))
    return [items[k] for k in order]


GLOBAL_LANE_OK_MATS = {"15_16_16": mat_abn(15, -16, -16), "16_16_16": mat_abn(16, -16, -16),
                       "15_17_16": mat_abn(15, -17, -16), "1_16_17": mat_abn(1, -16, -17)}


# ------------------------------------------------------------------ ksw_extend2 builders
EXT_GRID_MATS = {"default": mat_abn(1, -4, -1), "2_8_2": mat_abn(2, -8, -2), "4_6_1": mat_abn(4, -6, -1)}
EXT_GRID_QLEN = [15, 16, 31, 32, 47, 48, 63, 64, 95, 96, 127, 128, 151, 152]


def _ext_pair(rng, qlen, tlen, junk, with_n, exact=False):
    q, t = related_pair(rng, qlen, max(tlen, 0), sub=0.02, indel=0.01)
    if exact:  # the query is the target's prefix: the score reaches h0 + qlen max_mat, the bound itself
        n = min(qlen, tlen)
        q[:n] = t[:n]
    if junk and tlen > 4:  # related prefix, then junk: z-drop and trims
        cut = int(rng.integers(tlen // 3, tlen))
        t[cut:] = rng.integers(0, 4, tlen - cut)
    if with_n:
        q[int(rng.integers(0, qlen))] = 4
    return q, t


def extend_grid_items(mat_name, seed=1400):
    """Column class x score form: for each class-edge qlen, h0 putting `bound`
    (h0 + qlen max_mat) at 255 and 256 and, where positive, bound + pair_cg - 1
    at 255 and 256 (h0 <= 0 is replaced by h0 = 1 + (qlen % 7)); tlen = qlen +
    {-10, 0, 60}; w in {5, 100}; related / junk-tail / exact-prefix contents
    (the last reach the bound); a query N in every third task of the first
    two."""
    p = to_params(EXT_GRID_MATS[mat_name])
    rng = np.random.default_rng(seed + len(mat_name))
    items = []
    k = 0
    for qlen in EXT_GRID_QLEN:
        h0s = [255 - qlen * p.max_mat, 256 - qlen * p.max_mat, 256 - p.pair_cg - qlen * p.max_mat,
               257 - p.pair_cg - qlen * p.max_mat]
        for h0 in h0s:
            if h0 <= 0:
                h0 = 1 + qlen % 7
            for dt in (-10, 0, 60):
                for w in (5, 100):
                    for kind in ("related", "junk", "exact"):
                        # the N tasks rotate through the grid: k % 3 alone would tie N to the contents
                        q, t = _ext_pair(rng, qlen, qlen + dt, kind == "junk", exact=kind == "exact",
                                         with_n=kind != "exact" and (k + k // 12) % 3 == 0)
                        items.append((q, t, h0, w))
                        k += 1
    return p, items


def _pair_shaped(seed, n, qmax=151, h0max=60, wlo=1, whi=60):
    rng = np.random.default_rng(seed)
    items = []
    for k in range(n):
        qlen = int(rng.integers(1, qmax + 1))
        tlen = max(0, qlen + int(rng.integers(-30, 110)))
        q, t = related_pair(rng, qlen, tlen, sub=0.02 + 0.05 * (k % 3 == 0), indel=0.01 + 0.03 * (k % 5 == 0))
        if k % 4 == 1 and tlen:
            cut = int(rng.integers(0, max(1, min(qlen, tlen))))
            t[cut:] = rng.integers(0, 4, tlen - cut)
        if k % 6 == 5:
            q[int(rng.integers(0, qlen))] = 4
        items.append((q, t, int(rng.integers(1, h0max + 1)), int(rng.integers(wlo, whi + 1))))
    return items


def extend_edge_cases():
    """The remaining bsw_bucket / to_params edges, each as runs on either side:
    {name: [(label, mat, params_kw, items)]}."""
    D = DEFAULT_MAT
    cases = {}
    # bound 31999 / 32000 (16-bit lane kernels vs the wave kernel): large h0
    rng = np.random.default_rng(1500)
    for label, bnd in (("31999", 31999), ("32000", 32000)):
        items = []
        for qlen in [10, 15, 31, 40, 63, 64, 95, 100, 127] * 3:
            q, t = _ext_pair(rng, qlen, qlen + int(rng.integers(-5, 60)), junk=len(items) % 2 == 1, with_n=False)
            items.append((q, t, bnd - qlen, 100 if len(items) % 3 else 7))
        cases.setdefault("bound_32000", []).append((label, D, {}, items))
    # tlen 1023 / 1024 inside the pair envelope
    rng = np.random.default_rng(1501)
    for label, tlen in (("1023", 1023), ("1024", 1024)):
        items = []
        for qlen in [8, 31, 32, 64, 100, 128, 151] * 3:
            q, t = related_pair(rng, qlen, tlen, sub=0.02, indel=0.01)
            items.append((q, t, int(rng.integers(20, 90)), 100 if len(items) % 2 else 9))
        cases.setdefault("tlen_1024", []).append((label, D, {}, items))
    # pair_ok: e_del, e_ins 16 / 17
    ps = _pair_shaped(1502, 240)
    cases["e_del_17"] = [("16", D, dict(e_del=16), ps), ("17", D, dict(e_del=17), ps)]
    cases["e_ins_17"] = [("16", D, dict(e_ins=16), ps), ("17", D, dict(e_ins=17), ps)]
    # pair_cg 128 / 129: min -100, max 27 / 28; queries of <= 4 bases still fit 255
    rng = np.random.default_rng(1503)
    items = []
    for k in range(240):
        qlen = 1 + k % 4
        tlen = int(rng.integers(0, 14))
        t = rng.integers(0, 4, tlen).astype(np.uint8)
        q = (t[:qlen].copy() if tlen >= qlen and k % 3 else rng.integers(0, 4, qlen).astype(np.uint8))
        if k % 8 == 7 and tlen:
            t[int(rng.integers(0, tlen))] = 4
        edge = 256 - 128 - qlen * 27  # bound + pair_cg - 1 <= 255 at max 27
        h0 = max(1, edge + int(rng.integers(-3, 3)))
        items.append((q, t, h0, int(rng.integers(1, 20))))
    cases["pair_cg_129"] = [("128", mat_abn(27, -100, -1), {}, items), ("129", mat_abn(28, -100, -1), {}, items)]
    # lane_ok: matrix entries -16 / -17 and 15 / 16 (the pair path is tested first: tiny tasks still pair)
    mix = _pair_shaped(1504, 260, qmax=140, h0max=90, wlo=3, whi=100)
    cases["mat_min_17"] = [("-16", mat_abn(15, -16, -3), {}, mix), ("-17", mat_abn(15, -17, -3), {}, mix)]
    cases["mat_max_16"] = [("15", mat_abn(15, -16, -3), {}, mix), ("16", mat_abn(16, -16, -3), {}, mix)]
    return cases
