"""The test hook of the fused seeding call (fcsg_fmd_seeds, host/capi.cpp),
shared by test_fmd_seeds_cpu.py and test_fmd_seeds_gpu.py; the references and
batches are fmd_seed_cases.py's."""
import ctypes as C

import numpy as np

import fmd_seed_cases as S
import host_lib as H

HOST, TWO_CALL, FUSED = 0, 1, 2

H.lib.fcsg_fmd_seeds.restype = C.c_int


def seeds(contigs, reads, mode, params=S.BWA, max_occ=500, sa_intv=1, index_path="", max_mems=S.MAX_MEMS_DEFAULT,
          max_steps=0, start_mem_cap=0, start_row_cap=0, mem_cap=1 << 17, loc_cap=1 << 20):
    """fcsg_fmd_seeds: ([per read int64 (n, 5) {qb, qe, s, k, l}], [per read int64
    (m, 3) {contig, off, rev}], fallback reads, [host reads, host rows, retries]):
    S.seed_batch's result (S.assert_same compares the first two) and the stats."""
    ref = np.array([S.CODE.get(b, 4) for b in "".join(contigs)], np.uint8)
    cl = np.array([len(c) for c in contigs], np.int64)
    q = np.array([S.CODE.get(b, 4) for b in "".join(reads)], np.uint8)
    qlen = np.array([len(r) for r in reads], np.int32)
    qoff = np.concatenate([[0], np.cumsum(qlen, dtype=np.int64)]).astype(np.int64)
    n = len(reads)
    mems, loc = np.zeros((mem_cap, 5), np.int64), np.zeros((loc_cap, 3), np.int64)
    mem_off, loc_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    n_mems, n_loc = np.zeros(n, np.int32), np.zeros(n, np.int32)
    stats = np.full(3, -1, np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    min_len, split_len, split_width, max_mem_intv = params
    H.check(H.lib.fcsg_fmd_seeds(vp(ref), vp(cl), len(contigs), vp(q), vp(qoff), vp(qlen), n, min_len,
                                 min(split_len, 2**31 - 1), split_width, max_mem_intv, max_occ, sa_intv,
                                 str(index_path).encode(), int(mode), max_mems, int(max_steps),
                                 C.c_int64(start_mem_cap), C.c_int64(start_row_cap), vp(mems), vp(mem_off), vp(n_mems),
                                 C.c_int64(mem_cap), vp(loc), vp(loc_off), vp(n_loc), C.c_int64(loc_cap), vp(stats)))
    return ([mems[mem_off[r]:mem_off[r + 1]].copy() for r in range(n)],
            [loc[loc_off[r]:loc_off[r + 1]].copy() for r in range(n)], int(stats[0]), [int(x) for x in stats])
