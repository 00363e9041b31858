"""References, read batches and the test hook shared by the FMD-index seeding
tests: the host check of csrc/fmd_smem.h
(tools/micro/fmd_smem_test.cpp, test_fmd_seed_cpu.py) and the GPU kernels
(test_fmd_seed_gpu.py) see the same reads.  The oracle is the host index
(FmdIndex::collect / locate), which test_fmindex.py pins to a brute-force
definition."""
import ctypes as C
import functools

import numpy as np

import host_lib as H
from test_fmindex import make_ref, revcomp

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
LENGTHS = (1, 2, 18, 19, 20, 63, 64, 65, 151, 251)
# (min_len, split_len, split_width, max_mem_intv): bwa's, then one knob moved at a time
BWA = (19, 28, 10, 20)
PARAM_SETS = (BWA, (1, 28, 10, 20), (19, 10**9, 10, 20), (19, 28, 10, 0))
MAX_MEMS_DEFAULT = 128  # FCS_FMD_MAX_MEMS_DEFAULT


@functools.lru_cache(maxsize=None)
def plain_ref():
    return tuple(make_ref(np.random.default_rng(41)))


def mutate(rng, q, n_sub):
    q = list(q)
    for j in rng.choice(len(q), min(n_sub, len(q)), replace=False):
        q[j] = "ACGT"[(("ACGT".index(q[j]) if q[j] in "ACGT" else 0) + 1) % 4]
    return "".join(q)


@functools.lru_cache(maxsize=None)
def plain_batch(n_random=270):
    """The special reads first (so every prefix of the batch has some), then
    n_random reads of the lengths in LENGTHS drawn from the contigs with 0-5
    substitutions, every fourth reverse-complemented."""
    rng = np.random.default_rng(42)
    contigs = plain_ref()
    mid = contigs[1][700:801]
    special = [
        mid[:50] + "N" + mid[51:],                 # an N in the middle
        "N" + mid[1:],                             # at index 0
        mid[:-1] + "N",                            # at the last index
        "N" * 40,                                  # all N
        contigs[0][5950:] + "N" + contigs[1][:60],  # what the text holds across a contig separator
        contigs[0][5900:] + contigs[1][:80],       # a read spanning the separator
        contigs[2][1000:1251],                     # matches end to end (the i == len push)
        contigs[1][:80],                           # starts at a contig start: its row ends on a special row
        revcomp(contigs[2][-90:]),                 # ends at a contig end, reverse strand
        "".join(rng.choice(list("ACGT"), 151)),    # random: no long match
        contigs[1][480:560],                       # the cross-contig repeat: two occurrences
        revcomp(contigs[2][90:170]),               # the reverse-strand repeat
    ]
    reads = []
    for k in range(n_random):
        n = LENGTHS[k % len(LENGTHS)]
        c = contigs[(k // len(LENGTHS)) % 3]
        p = int(rng.integers(0, len(c) - n))
        q = mutate(rng, c[p:p + n], int(rng.integers(0, 6)))
        reads.append(revcomp(q) if k % 4 == 1 else q)
    # ten random reads follow the first six specials, so that the 15 / 16 / 17 prefixes mix both
    return tuple(special[:6] + reads[:10] + special[6:] + reads[10:])


@functools.lru_cache(maxsize=None)
def low_ref():
    rng = np.random.default_rng(43)
    r = lambda n: "".join(rng.choice(list("ACGT"), n))
    return (r(800) + "A" * 100 + r(700), r(500) + "ACG" * 40 + r(600))


@functools.lru_cache(maxsize=None)
def low_batch():
    c = low_ref()
    return ("A" * 150, "T" * 150, c[0][740:991], c[0][850:1001], revcomp(c[0][760:960]), c[1][450:701],
            c[1][560:711], "ACG" * 50, revcomp("ACG" * 50))


def write_tool_input(path, contigs, reads):
    """The file form tools/micro/fmd_smem_test.cpp reads."""
    with open(path, "w") as f:
        for c in contigs:
            f.write(">" + c + "\n")
        for q in reads:
            f.write(q + "\n")


H.lib.fcsg_fmd_seed_batch.restype = C.c_int


def seed_batch(contigs, reads, gpu, params=BWA, max_occ=500, sa_intv=1, index_path="", max_mems=MAX_MEMS_DEFAULT,
               mem_cap=1 << 17, loc_cap=1 << 20):
    """fcsg_fmd_seed_batch: ([per read int64 (n, 5) {qb, qe, s, k, l}], [per read
    int64 (m, 3) {contig, off, rev}], fallback reads)."""
    ref = np.array([CODE.get(b, 4) for b in "".join(contigs)], np.uint8)
    cl = np.array([len(c) for c in contigs], np.int64)
    q = np.array([CODE.get(b, 4) for b in "".join(reads)], np.uint8)
    qlen = np.array([len(r) for r in reads], np.int32)
    qoff = np.concatenate([[0], np.cumsum(qlen, dtype=np.int64)]).astype(np.int64)
    n = len(reads)
    mems, loc = np.zeros((mem_cap, 5), np.int64), np.zeros((loc_cap, 3), np.int64)
    mem_off, loc_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    n_mems, n_loc = np.zeros(n, np.int32), np.zeros(n, np.int32)
    fallback = C.c_int64(-1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    min_len, split_len, split_width, max_mem_intv = params
    H.check(H.lib.fcsg_fmd_seed_batch(vp(ref), vp(cl), len(contigs), vp(q), vp(qoff), vp(qlen), n, min_len,
                                      min(split_len, 2**31 - 1), split_width, max_mem_intv, max_occ, sa_intv,
                                      str(index_path).encode(), int(gpu), max_mems, vp(mems), vp(mem_off), vp(n_mems),
                                      C.c_int64(mem_cap), vp(loc), vp(loc_off), vp(n_loc), C.c_int64(loc_cap),
                                      C.byref(fallback)))
    return ([mems[mem_off[r]:mem_off[r + 1]].copy() for r in range(n)],
            [loc[loc_off[r]:loc_off[r + 1]].copy() for r in range(n)], fallback.value)


def index_arrays(contigs, sa_intv):
    """(occ, C[6], n_rows, sa, special_rows, special_sa, flen) of the FMD-index of
    the contigs: the arguments of fcship.fmd_index_create."""
    ref = np.array([CODE.get(b, 4) for b in "".join(contigs)], np.uint8)
    cl = np.array([len(c) for c in contigs], np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    sizes = np.zeros(5, np.int64)
    H.check(H.lib.fcsg_fmd_index_arrays(vp(ref), vp(cl), len(contigs), sa_intv, vp(sizes), None, None, None, None, None))
    occ, Carr, sa = np.zeros(sizes[0], np.uint64), np.zeros(6, np.int64), np.zeros(sizes[2], np.uint64)
    rows, ssa = np.zeros(sizes[3], np.int64), np.zeros(sizes[3], np.int64)
    H.check(H.lib.fcsg_fmd_index_arrays(vp(ref), vp(cl), len(contigs), sa_intv, vp(sizes), vp(occ), vp(Carr), vp(sa),
                                        vp(rows), vp(ssa)))
    return occ, Carr, int(sizes[1]), sa, rows, ssa, int(sizes[4])


def soa(reads):
    """(codes, q_off, q_len) of a batch: fcs_fmd_collect's input."""
    q = np.array([CODE.get(b, 4) for b in "".join(reads)], np.uint8)
    qlen = np.array([len(r) for r in reads], np.int32)
    return q, (np.cumsum(qlen, dtype=np.int64) - qlen).astype(np.int64), qlen


def assert_same(got, want):
    """Every integer of two seed_batch results (the fallback count apart)."""
    assert len(got[0]) == len(want[0])
    for r, (a, b) in enumerate(zip(got[0], want[0])):
        assert np.array_equal(a, b), ("SMEMs of read", r, a[:4], b[:4])
    for r, (a, b) in enumerate(zip(got[1], want[1])):
        assert np.array_equal(a, b), ("positions of read", r, a[:4], b[:4])
