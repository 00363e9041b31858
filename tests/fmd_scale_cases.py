"""The FMD seeding kernels past their first grid trip: the inputs
of test_fmd_scale_cpu.py and test_fmd_scale_gpu.py.  Every size comes from
scale_cases.CAPS, which test_scale_cpu.py pins to the .hip sources.

- ref(): fmd_seed_cases' plain and low-complexity contigs and one contig with
  a planted repeat (COPIES copies of a 48-base unit between unique spacers).
- batch_a(): 65,540 reads as numpy code arrays: past fmd_seed_order_kernel's
  cap, the third trip of fmd_collect_kernel and fmd_seed_expand_kernel, 65
  reads per lane of fmd_seed_scan_kernel with 15 empty lanes.  The bulk is
  random; the planted reads (planted_reads()) put deep and shallow interval stacks in
  one quad, empty reads on the seams, a multi-tile read in the order kernel's
  second round and reads the device hands back in later trips.
- batch_b(): 524,545 BWT rows for fcs_fmd_locate, the wrapped tail with a row
  below 0, a row past the index and a row many LF steps from a sample.
- host() / host_flat() / flat(): the host index's answer (fcsg_fmd_seeds mode
  0) for array batches, and fcs_fmd_seed's expected output computed from it.
"""
import ctypes as C
import functools

import numpy as np

import fmd_seed_cases as S
import fmd_seeds_cases as F
import host_lib as H
import scale_cases as SC

SH = SC.SHAPES
U, E, O = SH["fmd_units"], SH["fmd_expand"], SH["fmd_order"]
N_READS = SH["fmd_reads"]
STRIDES = (U, E, O)
UNIT, COPIES = 48, 24   # 24 > split_width 10: no re-seeding inside the unit, and 24 rows for every SMEM inside it
SA_INTV = 8
MIN1 = S.PARAM_SETS[1]   # min_len 1
SMALL_MEMS = 16          # the max_mems at which the planted reads go back to the host
MAX_READ = 151

_CODE = np.full(256, 4, np.uint8)
for _k, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _k


def encode(s):
    return _CODE[np.frombuffer(s.encode(), np.uint8)]


def decode(codes):
    return np.frombuffer(b"ACGTN", np.uint8)[np.minimum(codes, 4)].tobytes().decode()


# ------------------------------------------------------------------ the reference
@functools.lru_cache(maxsize=None)
def planted():
    """(contig, starts of the copies of the unit)."""
    rng = np.random.default_rng(2101)
    r = lambda n: "".join(rng.choice(list("ACGT"), n))  # noqa: E731
    unit = r(UNIT)
    parts, starts, at = [], [], 0
    for _ in range(COPIES):
        sp = r(int(rng.integers(40, 81)))
        parts += [sp, unit]
        starts.append(at + len(sp))
        at += len(sp) + UNIT
    parts.append(r(int(rng.integers(40, 81))))
    return "".join(parts), np.array(starts, np.int64)


@functools.lru_cache(maxsize=None)
def ref():
    """Six contigs: plain_ref's three, low_ref's two, the planted repeat."""
    return tuple(S.plain_ref()) + tuple(S.low_ref()) + (planted()[0],)


PLANTED_CONTIG = 5


# ------------------------------------------------------------------ batch A
def _bulk(rng, n):
    """n reads of 19 to 40 bases as a padded (n, 40) code matrix and their lengths: about half from inside the planted
    unit, the others from anywhere in the plain contigs and the planted one; 0 to 2 substitutions; every fourth
    reverse-complemented."""
    contigs = ref()
    text = np.concatenate([encode(c) for c in contigs])
    base = np.concatenate([[0], np.cumsum([len(c) for c in contigs])])
    length = rng.integers(19, 41, n)
    inside = rng.random(n) < 0.5
    starts = planted()[1]
    p_in = base[PLANTED_CONTIG] + starts[rng.integers(0, COPIES, n)] + (rng.random(n) * (UNIT - length + 1)).astype(np.int64)
    pick = np.array([0, 1, 2, PLANTED_CONTIG])[rng.integers(0, 4, n)]
    clen = np.array([len(c) for c in contigs])[pick]
    p_out = base[pick] + (rng.random(n) * (clen - length + 1)).astype(np.int64)
    p = np.where(inside, p_in, p_out)
    j = np.arange(40)[None, :]
    live = j < length[:, None]
    m = text[np.minimum(p[:, None] + j, len(text) - 1)]
    n_sub = rng.integers(0, 3, n)
    rows = np.arange(n)
    for k in range(2):
        at = (rng.random(n) * length).astype(np.int64)
        hit = (n_sub > k) & (m[rows, at] < 4)
        m[rows[hit], at[hit]] = (m[rows[hit], at[hit]] + rng.integers(1, 4, n)[hit]) % 4
    rc = rows % 4 == 1
    back = np.where(live, length[:, None] - 1 - j, 0)
    flipped = np.take_along_axis(m, back, axis=1)
    flipped = np.where(flipped < 4, 3 - flipped, flipped)
    m = np.where(rc[:, None], flipped, m)
    return np.where(live, m, 255).astype(np.uint8), length.astype(np.int64)


def _multi_tile_read():
    """151 random bases: at min_len 1 every few bases start another short SMEM."""
    return "".join(np.random.default_rng(2103).choice(list("ACGT"), MAX_READ))


@functools.lru_cache(maxsize=None)
def planted_reads():
    """{index: (kind, read)}: the reads placed by index.  kind: 'deep' (interval stacks as deep as the repeat), 'shallow'
    (its partner in the quad, one collect trip apart), 'empty' (no SMEM), 'tile' (more than 64 SMEMs at min_len 1),
    'over' (more than SMALL_MEMS SMEMs at bwa's parameters)."""
    plain = S.plain_ref()
    poly_a, acg = "A" * 150, "ACG" * 50
    out = {}
    k = 0
    for deep in (poly_a, acg):
        for r, deep_first in ((5, True), (1002, False), (20001, True), (31999, False)):
            r += 64 * k          # another block for the second deep read
            mer = plain[k % 3][700 + r % 900:730 + r % 900]
            a, b = (("deep", deep), ("shallow", mer)) if deep_first else (("shallow", mer), ("deep", deep))
            out[r], out[r + U] = a, b
        k += 1
    # the last read of a trip and the first of the next have no output; the order kernel's second round keeps ordinary
    # reads at O and O + 2 beside the multi-tile read, and the batch's last read (O + 3) is empty
    for at, q in ((U - 1, ""), (U, "N" * 40), (E - 1, ""), (E, "N" * 40), (O - 2, "N" * 33), (O - 1, ""), (N_READS - 1, "N" * 21)):
        out[at] = ("empty", q)
    out[O + 1] = ("tile", _multi_tile_read())
    # a little longer than the 120-base ACG tandem: some 25 SMEMs, between SMALL_MEMS and one tile of the order kernel
    out[U + 77] = ("over", "ACG" * 43)
    out[U + 4099] = ("over", "CGA" * 43)
    out[O + 2] = ("over", "CGT" * 43)
    return out


def kinds(kind):
    return sorted(r for r, (k, _) in planted_reads().items() if k == kind)


@functools.lru_cache(maxsize=None)
def batch_a():
    """(codes uint8, q_off int64 [n], q_len int32 [n]) of the 65,540 reads."""
    rng = np.random.default_rng(2102)
    m, length = _bulk(rng, N_READS)
    wide = np.full((N_READS, MAX_READ), 255, np.uint8)
    wide[:, :40] = m
    for r, (_, q) in planted_reads().items():
        wide[r] = 255
        wide[r, :len(q)] = encode(q)
        length[r] = len(q)
    # no period: two reads inside the unit, one stride apart, can come out equal; the later one gets another first base
    for _ in range(4):
        for T in sorted(set(STRIDES)):
            same = np.nonzero((wide[:-T] == wide[T:]).all(axis=1))[0] + T
            same = np.array([r for r in same if r not in planted_reads()], np.int64)
            wide[same, 0] = (wide[same, 0] + 1) % 4
    codes = wide[np.arange(MAX_READ)[None, :] < length[:, None]]
    q_off = np.cumsum(length) - length
    for a in (codes, q_off, length):
        a.setflags(write=False)
    return codes, q_off.astype(np.int64), length.astype(np.int32)


def padded(batch):
    """(n, longest) codes, 255 beyond each read's end."""
    codes, q_off, q_len = batch
    j = np.arange(int(q_len.max()))[None, :]
    live = j < q_len[:, None]
    return np.where(live, codes[np.minimum(q_off[:, None] + j, len(codes) - 1)], 255).astype(np.uint8)


def sub_batch(batch, idx):
    """The reads idx of a batch, as a batch."""
    codes, q_off, q_len = batch
    idx = np.asarray(idx, np.int64)
    length = q_len[idx].astype(np.int64)
    off = np.cumsum(length) - length
    take = np.repeat(q_off[idx] - off, length) + np.arange(int(length.sum()))
    return codes[take], off, q_len[idx].copy()


def strings(batch, idx):
    codes, q_off, q_len = batch
    return [decode(codes[q_off[r]:q_off[r] + q_len[r]]) for r in idx]


# ------------------------------------------------------------------ the host oracle on array batches
def _ref_arrays(contigs):
    return np.concatenate([encode(c) for c in contigs]), np.array([len(c) for c in contigs], np.int64)


def seeds_np(contigs, batch, mode, params=S.BWA, max_occ=500, sa_intv=1, max_mems=S.MAX_MEMS_DEFAULT, max_steps=0,
             mem_cap=1 << 21, loc_cap=1 << 21):
    """F.seeds for a batch given as arrays, its result left flat: (mems int64 (m, 5) {qb, qe, s, k, l}, mem_off,
    loc int64 (rows, 3) {contig, off, rev}, loc_off, stats)."""
    refc, cl = _ref_arrays(contigs)
    codes, q_off, q_len = (np.ascontiguousarray(a) for a in batch)
    n = len(q_len)
    qoff = np.concatenate([q_off, [len(codes)]]).astype(np.int64)
    mems, loc = np.zeros((mem_cap, 5), np.int64), np.zeros((loc_cap, 3), np.int64)
    mem_off, loc_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    n_mems, n_loc = np.zeros(n, np.int32), np.zeros(n, np.int32)
    stats = np.full(3, -1, np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    min_len, split_len, split_width, max_mem_intv = params
    H.check(H.lib.fcsg_fmd_seeds(vp(refc), vp(cl), len(contigs), vp(codes), vp(qoff), vp(q_len.astype(np.int32)), n, min_len,
                                 min(split_len, 2**31 - 1), split_width, max_mem_intv, max_occ, sa_intv, b"", int(mode),
                                 max_mems, int(max_steps), C.c_int64(0), C.c_int64(0), vp(mems), vp(mem_off), vp(n_mems),
                                 C.c_int64(mem_cap), vp(loc), vp(loc_off), vp(n_loc), C.c_int64(loc_cap), vp(stats)))
    assert np.array_equal(np.diff(mem_off), n_mems) and np.array_equal(np.diff(loc_off), n_loc)
    return mems[:mem_off[-1]].copy(), mem_off, loc[:loc_off[-1]].copy(), loc_off, [int(x) for x in stats]


@functools.lru_cache(maxsize=None)
def host(params=S.BWA):
    """The host index's answer for all of batch A.  At min_len 1 one occurrence per SMEM is located (the positions of
    that run come from flat(), which test_fmd_scale_cpu.py checks against the host's at bwa's parameters)."""
    return seeds_np(ref(), batch_a(), F.HOST, params, max_occ=500 if params == S.BWA else 1)


@functools.lru_cache(maxsize=None)
def index(sa_intv):
    return S.index_arrays(ref(), sa_intv)


def sa_full():
    return index(1)[3].astype(np.int64)


def flat(mems5, mem_off, sa1, max_occ=500, dropped=()):
    """fcs_fmd_seed's output for reads whose host SMEMs are mems5[mem_off[r]:mem_off[r + 1]]: (mems of FMD_MEM, mem_off,
    pos, row_off), the positions read from the full suffix array at the rows bwa samples.  dropped: reads the device
    hands back, whose ranges are empty."""
    import fcship
    counts = np.diff(mem_off)
    if len(dropped):
        keep_read = np.ones(len(counts), bool)
        keep_read[np.asarray(dropped, np.int64)] = False
        mems5 = mems5[np.repeat(keep_read, counts)]
        counts = np.where(keep_read, counts, 0)
    mems = np.zeros(len(mems5), fcship.FMD_MEM)
    for j, f in enumerate(("qb", "qe", "s", "k", "l")):
        mems[f] = mems5[:, j]
    s, k = mems5[:, 2], mems5[:, 3]
    kept = np.minimum(s, max_occ)
    step = np.where(s > max_occ, s // max_occ, 1)
    first = np.cumsum(kept) - kept
    rows = np.repeat(k, kept) + (np.arange(int(kept.sum())) - np.repeat(first, kept)) * np.repeat(step, kept)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    row_off = np.concatenate([[0], np.cumsum(kept)])[off].astype(np.int64)
    return mems, off, sa1[rows], row_off


def text_map(pos, length, contigs):
    """host/gpu_seed.cpp TextMap::locate: (contig, off, rev) of text positions of matches of `length` bases."""
    cstart = 1 + np.concatenate([[0], np.cumsum([len(c) + 1 for c in contigs])])
    flen = int(cstart[-1])
    rev = pos >= flen
    p = np.where(rev, 2 * flen - pos - length, pos)
    contig = np.searchsorted(cstart[:-1], p, side="right") - 1
    return np.stack([contig, p - cstart[contig], rev.astype(np.int64)], axis=1)


# ------------------------------------------------------------------ batch B
@functools.lru_cache(maxsize=None)
def batch_b():
    """dict(rows, pos, status, far): 524,545 rows of the sampled index, rows[i] = (i * 7919) % n_rows; in the wrapped
    tail one row is -1, one is n_rows and one (`far`, at index `far_at`) lies FAR_STEPS or more LF steps from a stored
    row.  pos / status are what fcs_fmd_locate answers at max_steps FAR_STEPS - 1."""
    occ, Carr, n_rows, sa8, rows8, ssa8, flen = index(SA_INTV)
    sa1 = sa_full()
    L, n = SH["fmd_locate"], SH["fmd_rows"]
    rows = (np.arange(n, dtype=np.int64) * 7919) % n_rows
    # a row's walk visits text positions SA[row], SA[row] - 1, ..: its steps to a stored row (sampled or special)
    stored = np.zeros(n_rows, bool)
    stored[::SA_INTV] = True
    stored[rows8] = True
    text_of = np.empty(n_rows, np.int64)
    text_of[sa1] = np.arange(n_rows)
    steps = np.full(n_rows, -1, np.int64)
    for d in range(64 * SA_INTV):
        p = sa1 - d
        hit = (steps < 0) & (p >= 0) & stored[text_of[np.maximum(p, 0)]]
        steps[hit] = d
    assert (steps >= 0).all()
    far = int(np.argmax(steps))
    rows[L + 11], rows[L + 130], rows[L + 255] = -1, n_rows, far
    ok = (rows >= 0) & (rows < n_rows)
    inside = np.where(ok, rows, 0)
    import fcship
    cap = FAR_STEPS - 1
    status = np.where(~ok, fcship.FCS_FMD_BAD_ROW, np.where(steps[inside] > cap, fcship.FCS_FMD_STEP_CAP, fcship.FCS_FMD_LOCATED))
    return dict(rows=rows, pos=sa1[inside], status=status.astype(np.int32), far=far, far_at=L + 255, steps=steps, n_rows=n_rows,
                bad_at=(L + 11, L + 130))


FAR_STEPS = 2   # batch_b()'s far row needs at least this many LF steps (the CPU test asserts it)
