#!/usr/bin/env python3
"""FMD-index seeding rates on the GPU against the host threads it would
replace.  A tool, not a test.

The reads are the 2x151 synthetic pairs `fcs-genome synth` draws over the
bench's align reference (--mbp, 30x), the first --reads of them; the index is
built in memory at each --sa-intv.  Legs, each a child process of its own
under `timeout`, alternated --rounds times on the same box:
  gpu   fcs_fmd_collect_dev between two device events (the kernel alone,
        inputs resident, --kernel-reps launches per window), fcs_fmd_collect from and to host buffers (the
        synchronous call with its copies and the final sort); then the same
        two figures for fcs_fmd_locate over the rows the aligner samples;
        then the fused pipeline on the same reads: fcs_fmd_seed_dev between
        two events (collect, order, scan, expand, locate; inputs resident) and
        the synchronous fcs_fmd_seed, beside the two-call sum (collect call +
        row build + locate call) and the bytes each path copies back per read;
  host  FmdIndex::collect and FmdIndex::locate on --threads threads
        (fcsg_fmd_host_rates: parallel_for over the reads, as align_batch).
Prints one JSON line per sa_intv: reads/s of collect and rows/s of locate
(median, min, max over the rounds), and the overflow reads at --max-mems.
Without a GPU the gpu leg fails; nothing falls back.

  tools/bench_seed.py --work /tmp/bs --mbp 4 --rounds 3
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "falcon-genome_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
BWA = (19, 28, 10, 20)
MAX_OCC = 500


def load(work, n_reads):
    """(contigs as code arrays, reads as code arrays) of the synthetic sample."""
    import numpy as np
    lut = np.full(256, 4, np.uint8)
    for b, c in CODE.items():
        lut[ord(b)] = c
    contigs, cur = [], []
    for ln in open(os.path.join(work, "in", "ref.fasta")):
        if ln.startswith(">"):
            if cur:
                contigs.append(lut[np.frombuffer("".join(cur).encode(), np.uint8)])
            cur = []
        else:
            cur.append(ln.strip().upper())
    contigs.append(lut[np.frombuffer("".join(cur).encode(), np.uint8)])
    reads = []
    for name in ("sample_1.fastq", "sample_2.fastq"):
        with open(os.path.join(work, "in", name)) as f:
            for i, ln in enumerate(f):
                if i % 4 == 1:
                    reads.append(lut[np.frombuffer(ln.strip().encode(), np.uint8)])
                    if len(reads) % (n_reads // 2) == 0:
                        break
    return contigs, reads[:n_reads]


def soa(reads):
    import numpy as np
    qlen = np.array([len(r) for r in reads], np.int32)
    return np.concatenate(reads), (np.cumsum(qlen, dtype=np.int64) - qlen).astype(np.int64), qlen


def leg_gpu(a):
    import ctypes as C
    import numpy as np
    import torch
    import fcship
    import host_lib as H
    contigs, reads = load(a.work, a.reads)
    ref, cl = np.concatenate(contigs), np.array([len(c) for c in contigs], np.int64)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    sizes = np.zeros(5, np.int64)
    H.check(H.lib.fcsg_fmd_index_arrays(vp(ref), vp(cl), len(cl), a.sa_intv, vp(sizes), None, None, None, None, None))
    occ, Carr, sa = np.zeros(sizes[0], np.uint64), np.zeros(6, np.int64), np.zeros(sizes[2], np.uint64)
    rows, ssa = np.zeros(sizes[3], np.int64), np.zeros(sizes[3], np.int64)
    H.check(H.lib.fcsg_fmd_index_arrays(vp(ref), vp(cl), len(cl), a.sa_intv, vp(sizes), vp(occ), vp(Carr), vp(sa),
                                        vp(rows), vp(ssa)))
    h = fcship.fmd_index_create(occ, Carr, int(sizes[1]), sa, a.sa_intv, rows, ssa, int(sizes[4]))
    codes, q_off, q_len = soa(reads)
    n, max_len = len(reads), int(q_len.max())
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    P = fcship.FmdParams(BWA[0], BWA[1], BWA[2], a.max_mems, BWA[3])

    def timed(fn, reps):
        """Seconds of one launch: `reps` launches between two events (a window of tens of milliseconds)."""
        fn()  # warm: code object, caches, arenas
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / 1e3 / reps
    with torch.cuda.stream(stream):
        d_codes, d_off, d_len = (torch.from_numpy(x).to(dev) for x in (codes, q_off, q_len))
        d_order = torch.from_numpy(np.argsort(-q_len, kind="stable").astype(np.int32)).to(dev)
        arena = torch.zeros(fcship.lib.fcs_fmd_collect_arena_bytes(n, max_len), dtype=torch.uint8, device=dev)
        d_mems = torch.zeros(n * a.max_mems * 32, dtype=torch.uint8, device=dev)
        d_nm, d_ov = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        collect_kernel_s = timed(lambda: fcship.check(fcship.lib.fcs_fmd_collect_dev(
            h, d_codes.data_ptr(), len(codes), d_off.data_ptr(), d_len.data_ptr(), d_order.data_ptr(), n, max_len,
            C.addressof(P), arena.data_ptr(), arena.numel(), d_mems.data_ptr(), d_nm.data_ptr(), d_ov.data_ptr(),
            C.c_void_p(stream.cuda_stream))), a.kernel_reps)
    fcship.fmd_collect(h, codes, q_off, q_len, *BWA[:3], BWA[3], a.max_mems)
    t0 = time.perf_counter()
    mems, n_mems, overflow = fcship.fmd_collect(h, codes, q_off, q_len, *BWA[:3], BWA[3], a.max_mems)
    collect_call_s = time.perf_counter() - t0
    # the rows seed_read samples from each SMEM
    t0 = time.perf_counter()
    used = np.arange(a.max_mems)[None, :] < n_mems[:, None]
    k, s = mems["k"][used], mems["s"][used]
    step = np.where(s > MAX_OCC, s // MAX_OCC, 1)
    kept = np.minimum(s, MAX_OCC)
    r = np.repeat(k, kept) + (np.arange(kept.sum()) - np.repeat(np.cumsum(kept) - kept, kept)) * np.repeat(step, kept)
    r = r.astype(np.int64)
    row_build_s = time.perf_counter() - t0
    with torch.cuda.stream(stream):
        d_rows = torch.from_numpy(r).to(dev)
        d_pos = torch.zeros(len(r), dtype=torch.int64, device=dev)
        d_st = torch.zeros(len(r), dtype=torch.int32, device=dev)
        locate_kernel_s = timed(lambda: fcship.check(fcship.lib.fcs_fmd_locate_dev(
            h, d_rows.data_ptr(), len(r), 0, d_pos.data_ptr(), d_st.data_ptr(), C.c_void_p(stream.cuda_stream))),
            10 * a.kernel_reps)
        capped = int((d_st != 0).sum().item())
    fcship.fmd_locate(h, r)
    t0 = time.perf_counter()
    fcship.fmd_locate(h, r)
    locate_call_s = time.perf_counter() - t0
    # the fused pipeline: the aligner's first capacities
    mem_cap, row_cap = max(16 * n, 4096), max(64 * n, 65536)
    SP = fcship.FmdSeedParams(P, MAX_OCC, 0)
    with torch.cuda.stream(stream):
        ws = torch.zeros(fcship.lib.fcs_fmd_seed_workspace_bytes(n, max_len, a.max_mems, row_cap), dtype=torch.uint8,
                         device=dev)
        f_mems = torch.zeros(mem_cap * 32, dtype=torch.uint8, device=dev)
        f_pos = torch.zeros(row_cap, dtype=torch.int64, device=dev)
        f_moff, f_roff = (torch.zeros(n + 1, dtype=torch.int64, device=dev) for _ in range(2))
        fused_kernel_s = timed(lambda: fcship.check(fcship.lib.fcs_fmd_seed_dev(
            h, d_codes.data_ptr(), len(codes), d_off.data_ptr(), d_len.data_ptr(), d_order.data_ptr(), n, max_len,
            C.addressof(SP), ws.data_ptr(), ws.numel(), f_mems.data_ptr(), mem_cap, f_moff.data_ptr(), f_pos.data_ptr(),
            row_cap, f_roff.data_ptr(), d_ov.data_ptr(), C.c_void_p(stream.cuda_stream))), a.kernel_reps)
        fused_totals = [int(f_moff[-1].item()), int(f_roff[-1].item())]
        fused_unlocated = int((f_pos[:fused_totals[1]] < 0).sum().item())
    seed_args = (h, codes, q_off, q_len, *BWA[:3], BWA[3], a.max_mems, MAX_OCC)
    fcship.fmd_seed(*seed_args)
    t0 = time.perf_counter()
    f = fcship.fmd_seed(*seed_args)
    fused_call_s = time.perf_counter() - t0
    assert f[5] == fcship.FCS_OK and fused_totals == [int(f[1][-1]), int(f[3][-1])] == [int(n_mems.sum()), len(r)]
    fcship.fmd_index_destroy(h)
    return {"fused_kernel_s": fused_kernel_s, "fused_call_s": fused_call_s, "row_build_s": row_build_s,
            "two_call_s": collect_call_s + row_build_s + locate_call_s,
            "two_kernels_s": collect_kernel_s + locate_kernel_s, "fused_unlocated_rows": fused_unlocated,
            "d2h_bytes_per_read": {"two_call": 8 + 32 * a.max_mems + 12 * len(r) / n,
                                   "fused": 20 + (32 * int(n_mems.sum()) + 8 * len(r)) / n},
            "reads": n, "smems": int(n_mems.sum()), "overflow_reads": int(overflow.sum()), "rows": len(r),
            "rows_past_step_cap": capped, "collect_kernel_s": collect_kernel_s, "collect_call_s": collect_call_s,
            "locate_kernel_s": locate_kernel_s, "locate_call_s": locate_call_s}


def leg_host(a):
    import ctypes as C
    import numpy as np
    import host_lib as H
    contigs, reads = load(a.work, a.reads)
    ref, cl = np.concatenate(contigs), np.array([len(c) for c in contigs], np.int64)
    codes, q_off, q_len = soa(reads)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    out, counts = np.zeros(2, np.float64), np.zeros(2, np.int64)
    H.check(H.lib.fcsg_fmd_host_rates(vp(ref), vp(cl), len(cl), vp(codes), vp(q_off), vp(q_len), len(reads), *BWA, MAX_OCC,
                                      a.sa_intv, a.threads, vp(out), vp(counts)))
    return {"reads": len(reads), "smems": int(counts[0]), "rows": int(counts[1]), "collect_s": float(out[0]),
            "locate_s": float(out[1]), "threads": a.threads}


def child(a, leg, sa_intv):
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--work", a.work,
           "--reads", str(a.reads), "--sa-intv", str(sa_intv), "--threads", str(a.threads), "--max-mems", str(a.max_mems), "--kernel-reps", str(a.kernel_reps)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"leg {leg} at sa_intv {sa_intv} ended with {r.returncode}:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--work", required=True, help="directory for the generated inputs")
    ap.add_argument("--mbp", type=float, default=4.0, help="genome of the synthetic sample (30x of 2x151 pairs)")
    ap.add_argument("--reads", type=int, default=200000, help="reads of the sample that are seeded")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sa-intvs", default="8,32")
    ap.add_argument("--sa-intv", type=int, default=8)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the host leg")
    ap.add_argument("--max-mems", type=int, default=32, help="device SMEM slots per read (the aligner's)")
    ap.add_argument("--kernel-reps", type=int, default=20, help="collect launches per timed window (locate: ten times as many)")
    ap.add_argument("--limit", type=int, default=300, help="seconds a leg may take")
    ap.add_argument("--leg", choices=("gpu", "host"))
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(leg_gpu(a) if a.leg == "gpu" else leg_host(a)))
        return 0
    os.makedirs(a.work, exist_ok=True)
    binary = os.path.join(ROOT, "falcon-genome_amd", "bin", "fcs-genome")
    r = subprocess.run(["timeout", "-k", "10", "600", binary, "synth", "-o", os.path.join(a.work, "in"), "-c",
                        f"chr1:{int(a.mbp * 1e6)}", "-x", "30", "--no-fastq", "--paired", "350", "--seed", "20261015"],
                       capture_output=True, text=True, cwd=a.work)
    if r.returncode != 0:
        raise SystemExit(f"synth ended with {r.returncode}:\n{r.stderr[-3000:]}")
    for intv in (int(x) for x in a.sa_intvs.split(",")):
        runs = {"gpu": [], "host": []}
        for _ in range(a.rounds):  # alternating, on one box
            runs["gpu"].append(child(a, "gpu", intv))
            runs["host"].append(child(a, "host", intv))
        g, h = runs["gpu"][0], runs["host"][0]

        def rate(leg, key, count):
            v = sorted(count / x[key] for x in runs[leg])
            return {"median": round(statistics.median(v)), "min": round(v[0]), "max": round(v[-1])}
        print(json.dumps({
            "sa_intv": intv, "reads": g["reads"], "smems": g["smems"], "host_smems": h["smems"], "rows": g["rows"],
            "host_rows": h["rows"], "max_mems": a.max_mems, "overflow_reads": g["overflow_reads"],
            "rows_past_step_cap": g["rows_past_step_cap"], "rounds": a.rounds,
            "collect_reads_per_s": {"gpu_kernel": rate("gpu", "collect_kernel_s", g["reads"]),
                                    "gpu_sync_call": rate("gpu", "collect_call_s", g["reads"]),
                                    f"host_{a.threads}t": rate("host", "collect_s", h["reads"])},
            "fused_reads_per_s": {"gpu_kernels": rate("gpu", "fused_kernel_s", g["reads"]),
                                  "collect_plus_locate_kernels": rate("gpu", "two_kernels_s", g["reads"]),
                                  "gpu_sync_call": rate("gpu", "fused_call_s", g["reads"]),
                                  "two_call_sum": rate("gpu", "two_call_s", g["reads"])},
            "d2h_bytes_per_read": {k: round(v, 1) for k, v in g["d2h_bytes_per_read"].items()},
            "fused_unlocated_rows": g["fused_unlocated_rows"],
            "locate_rows_per_s": {"gpu_kernel": rate("gpu", "locate_kernel_s", g["rows"]),
                                  "gpu_sync_call": rate("gpu", "locate_call_s", g["rows"]),
                                  f"host_{a.threads}t": rate("host", "locate_s", h["rows"])},
        }), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
