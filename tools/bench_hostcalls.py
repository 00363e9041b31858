"""Times the synchronous host-pointer calls of libfcship.so (the library FCSHIP_LIB names) and
prints one JSON line: per leg the median and the spread of REPS calls after WARM, in ms."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (one HIP runtime per process, before the binding)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "falcon-genome_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import fcship  # noqa: E402
import fmd_seed_cases as S  # noqa: E402

WARM, REPS = 2, 9
out = {"lib": os.environ.get("FCSHIP_LIB", "head")}


def timed(name, f):
    for _ in range(WARM):
        f()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    out[name] = {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


fcship.check(fcship.lib.fcs_device_warmup(0, 0))

p = fcship.synth_phmm(1234, 200_000, R=101, hmin=150, hmax=300)
pb, po, pout = p.to_struct(), fcship.phmm_opts(), np.zeros(p.n_pairs, np.float64)
timed("phmm_compute_pairs_200k", lambda: fcship.check(fcship.lib.fcs_phmm_compute_pairs(
    C.byref(pb), pout.ctypes.data_as(fcship.f64p), C.byref(po))))

t = fcship.synth_bsw(1234, 100_000, read_len=151, ref_len=10_000_000, w=100)
tb, params = t.to_struct(), fcship.bsw_params()
res, cells = np.zeros((t.n, 6), np.int32), np.zeros(t.n, np.int64)
timed(f"bsw_extend_batch_{t.n}", lambda: fcship.check(fcship.lib.fcs_bsw_extend_batch(
    C.byref(tb), C.byref(params), res.ctypes.data_as(fcship.i32p), cells.ctypes.data_as(fcship.i64p), 0)))

g = fcship.synth_bsw(1235, 20_000, read_len=151, ref_len=10_000_000, w=100, mode=1, fixed_q=151, fixed_t=251)
n = g.n
tasks = (fcship.BswTask * n)()
bq, bt = g.qbuf.ctypes.data, g.tbuf.ctypes.data
for k in range(n):
    tasks[k] = fcship.BswTask(int(g.qlen[k]), int(g.tlen[k]), 1, int(g.w[k]), C.cast(bq + int(g.qoff[k]), fcship.u8p),
                              C.cast(bt + int(g.toff[k]), fcship.u8p))
cap = (g.qlen + g.tlen + 2).astype(np.int32)
off = np.concatenate([[0], np.cumsum(cap[:-1], dtype=np.int64)]).astype(np.int64)
arena, scores, ncig = np.zeros(int(cap.sum()), np.uint32), np.zeros(n, np.int32), np.zeros(n, np.int32)
timed(f"bsw_global_cigar_{n}", lambda: fcship.check(fcship.lib.fcs_bsw_global(
    tasks, n, C.byref(params), scores.ctypes.data_as(fcship.i32p), arena.ctypes.data_as(fcship.u32p),
    off.ctypes.data_as(fcship.i64p), cap.ctypes.data_as(fcship.i32p), ncig.ctypes.data_as(fcship.i32p), 0)))
xt, kout = np.full(n, fcship.KSW_XSTART | fcship.KSW_XBYTE, np.int32), np.zeros((n, 7), np.int32)
timed(f"bsw_align_{n}", lambda: fcship.check(fcship.lib.fcs_bsw_align(
    tasks, n, C.byref(params), xt.ctypes.data_as(fcship.i32p), kout.ctypes.data, 0)))

contigs, reads = S.plain_ref(), S.plain_batch()
occ, Carr, n_rows, sa, rows, ssa, flen = S.index_arrays(contigs, 8)
h = fcship.fmd_index_create(occ, Carr, n_rows, sa, 8, rows, ssa, flen)
batch = S.soa([reads[i % len(reads)] for i in range(2300)])
mems, pos = np.zeros(1 << 18, fcship.FMD_MEM), np.zeros(1 << 20, np.int64)


def seed():
    assert fcship.fmd_seed(h, *batch, mem_cap=len(mems), row_cap=len(pos), mems=mems, pos=pos)[5] == fcship.FCS_OK


timed("fmd_seed_2300", seed)
fcship.fmd_index_destroy(h)

rng = np.random.default_rng(7)
data = rng.integers(0, 4, 16 << 20).astype(np.uint8)  # 2 bits of entropy a byte: compresses like base codes
bound = fcship.lib.fcs_bgzf_deflate_bound(len(data), fcship.FCS_BGZF_BLOCK_MAX, 1)
comp, coff = np.zeros(bound, np.uint8), np.zeros(bound // 65536 + 1, np.int64)
got, nm = C.c_int64(), C.c_int32()
timed("bgzf_deflate_16MiB", lambda: fcship.check(fcship.lib.fcs_bgzf_deflate(
    data.ctypes.data, len(data), fcship.FCS_BGZF_BLOCK_MAX, 1, comp.ctypes.data, bound, C.byref(got), coff.ctypes.data,
    C.byref(nm), 0)))
back, used, nb = np.zeros(len(data), np.uint8), C.c_int64(), C.c_int64()
timed("bgzf_inflate_16MiB", lambda: fcship.check(fcship.lib.fcs_bgzf_inflate(
    comp.ctypes.data, got.value, back.ctypes.data, len(back), C.byref(used), C.byref(nb), 0)))
assert nb.value == len(data) and np.array_equal(back, data)
out["checks"] = {"phmm_sum": float(pout.sum()), "extend_sum": int(res.sum()), "global_sum": int(scores.sum()),
                 "align_sum": int(kout.sum()), "deflate_bytes": got.value}
print(json.dumps(out))
