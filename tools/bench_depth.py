#!/usr/bin/env python3
"""Depth of coverage on the GPU against the host path it would replace
(DESIGN.md §4.11).  A tool, not a test.

Batches are synthesised (seeded): 151M reads sorted by position at --coverage
on one contig sized to hold them, qualities drawn from eight values, one window
over the whole contig.  Two sets of pieces: no -L (the contig as one long
interval in pieces of 65,536 loci) and an exome-like -L (intervals of 200 loci,
one every 2,000).

Per size, --rounds rounds of these legs, alternated on the same box:
  kernels  fcsdp_runs_dev, fcsdp_scan_dev and fcsdp_stats_dev (both piece
           sets), each between two device events, inputs resident
           (--kernel-reps launches per window);
  call     fcsdp_count and fcsdp_stats from and to host arrays;
  host     depth_count_host and depth_stats_host (fcsg_depth_*), on one thread
           and on --host-threads threads.
Prints one JSON line per size with the median, min and max of each leg in
milliseconds, and checks that the legs give the same depths and statistics.

--ab DIR runs `fcs-genome depth` on a synthetic BAM (--ab-mbp, --ab-cov),
depth.gpu off and on, alternated --rounds times for every window size of
--window-bp, once with the per-locus file and once with -b; it requires
byte-identical files and prints both walls.

  tools/bench_depth.py --rounds 3
  tools/bench_depth.py --ab /tmp/dpab --rounds 3
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "falcon-genome_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

READ = 151
SUFFIXES = ["", ".sample_summary", ".sample_statistics", ".sample_cumulative_coverage_counts",
            ".sample_cumulative_coverage_proportions", ".sample_interval_summary", ".sample_interval_statistics"]


def synth(n, seed, coverage):
    """(the arrays of an fcsdp_batch of n records, contig length)."""
    rng = np.random.default_rng(seed)
    length = max(int(n * READ / coverage), 2 * READ)
    pos = np.sort(rng.integers(0, length - READ, n)).astype(np.int32)
    qual = np.array([2, 11, 25, 30, 33, 37, 40, 40], np.uint8)[rng.integers(0, 8, n * READ)]
    flag = np.where(rng.random(n) < 0.5, 0x10, 0).astype(np.uint16)
    return (flag, np.zeros(n, np.int32), pos, np.full(n, 60, np.uint8), np.full(n, READ << 4, np.uint32),
            np.arange(n + 1, dtype=np.int64), qual, np.arange(n + 1, dtype=np.int64) * READ, np.zeros(n, np.uint8)), length


def summary(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def bench_sizes(a):
    import torch
    import fcship
    import host_lib as H
    L = H.lib
    L.fcsg_depth_count.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.fcsg_depth_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_void_p]
    dev = torch.device("cuda", a.device)
    views = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    prm = fcship.dp_params(min_baseq=10)
    for size in a.sizes:
        arrays, length = synth(size, a.seed, a.coverage)
        arrays = fcship.dp_arrays(*arrays)
        hb = fcship.dp_batch(arrays)
        w = fcship.DpWindow(0, 0, 0, length, length)
        n = len(arrays[0])
        bits = np.full((length + 63) // 64 + 1, ~np.uint64(0), np.uint64)
        sets = {"whole": np.array([(s, min(s + 65536, length), 0, 0) for s in range(0, length, 65536)], fcship.DP_PIECE),
                "exome": np.array([(s, s + 200, -1, 0) for s in range(0, length - 200, 2000)], fcship.DP_PIECE)}
        stream = torch.cuda.Stream(device=dev)

        def host_count(threads):
            d = np.zeros(length, np.uint32)
            t0 = time.perf_counter()
            H.check(L.fcsg_depth_count(C.addressof(hb), C.addressof(prm), C.addressof(w), threads, d.ctypes.data))
            return (time.perf_counter() - t0) * 1e3, d

        _, depth = host_count(a.host_threads)

        def host_stats(pc, threads):
            hist, lh, sm = np.zeros(501, np.uint64), np.zeros((1, 501), np.uint64), np.zeros(len(pc), fcship.DP_SUMMARY)
            t0 = time.perf_counter()
            H.check(L.fcsg_depth_stats(depth.ctypes.data, bits.ctypes.data, length, pc.ctypes.data, len(pc), 1, threads,
                                       hist.ctypes.data, lh.ctypes.data, sm.ctypes.data))
            return (time.perf_counter() - t0) * 1e3, (hist, lh, sm)

        want = {k: host_stats(pc, a.host_threads)[1] for k, pc in sets.items()}

        with torch.cuda.stream(stream):
            t = [torch.from_numpy(x.view(views.get(x.dtype, x.dtype))).to(dev) for x in arrays]
            p = [x.data_ptr() for x in t]
            db = fcship.DpBatch(n, p[0], p[1], p[2], p[3], p[4], p[5], len(arrays[4]), 0, p[6], p[7], len(arrays[6]), p[8])
            cells = torch.zeros(length + 1, dtype=torch.int32, device=dev)
            ddepth = torch.from_numpy(depth.view(np.int32)).to(dev)
            dbits = torch.from_numpy(bits.view(np.int64)).to(dev)
            dpc = {k: torch.from_numpy(pc.view(np.int32).copy()).to(dev) for k, pc in sets.items()}
            dsum = {k: torch.zeros(len(pc) * 8, dtype=torch.int32, device=dev) for k, pc in sets.items()}
            dhist = torch.zeros(501, dtype=torch.int64, device=dev)
            dlong = torch.zeros(501, dtype=torch.int64, device=dev)
            status = torch.zeros(2, dtype=torch.int32, device=dev)
            need = fcship.lib.fcsdp_workspace_bytes(length)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        sp = C.c_void_p(stream.cuda_stream)

        def timed(launch, reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                for _ in range(reps):
                    launch()
                e1.record(stream)
            stream.synchronize()
            return e0.elapsed_time(e1) / reps

        def runs_kernel():
            cells.zero_()
            return timed(lambda: fcship.check(fcship.lib.fcsdp_runs_dev(
                a.device, C.addressof(db), C.addressof(prm), C.addressof(w), cells.data_ptr(), status.data_ptr(), sp)),
                a.kernel_reps)

        def scan_kernel():   # after runs_kernel: kernel_reps batches' runs, scanned once
            ms = timed(lambda: fcship.check(fcship.lib.fcsdp_scan_dev(a.device, cells.data_ptr(), length, ws.data_ptr(), need,
                                                                      status.data_ptr(), sp)), 1)
            ok = (cells.cpu().numpy()[:length].view(np.uint32) == a.kernel_reps * depth).all() and int(status.cpu()[0]) == 0
            return ms, bool(ok)

        def stats_kernel(k):
            dhist.zero_(), dlong.zero_()
            ms = timed(lambda: fcship.check(fcship.lib.fcsdp_stats_dev(
                a.device, ddepth.data_ptr(), dbits.data_ptr(), length, dpc[k].data_ptr(), len(sets[k]), 1, dhist.data_ptr(),
                dlong.data_ptr(), dsum[k].data_ptr(), status[1:].data_ptr(), sp)), a.kernel_reps)
            hist, lh, sm = want[k]
            ok = ((dhist.cpu().numpy() == a.kernel_reps * hist.astype(np.int64)).all()
                  and (dlong.cpu().numpy() == a.kernel_reps * lh[0].astype(np.int64)).all()
                  and dsum[k].cpu().numpy().tobytes() == sm.tobytes() and int(status.cpu()[1]) == 0)
            return ms, bool(ok)

        def call_count():
            t0 = time.perf_counter()
            out = fcship.dp_count(arrays, (0, 0, length, length), prm, device=a.device)
            return (time.perf_counter() - t0) * 1e3, out

        def call_stats(k):
            pc = sets[k]
            hist, lh, sm = np.zeros(501, np.uint64), np.zeros((1, 501), np.uint64), np.zeros(len(pc), fcship.DP_SUMMARY)
            t0 = time.perf_counter()
            fcship.check(fcship.lib.fcsdp_stats(a.device, depth.ctypes.data, bits.ctypes.data, length, pc.ctypes.data, len(pc), 1,
                                                hist.ctypes.data, lh.ctypes.data, sm.ctypes.data))
            return (time.perf_counter() - t0) * 1e3, (hist, lh, sm)

        runs_kernel(), scan_kernel(), stats_kernel("whole"), call_count(), call_stats("whole")   # warm-up
        names = ["runs_kernel", "scan_kernel", "stats_kernel_whole", "stats_kernel_exome", "count_call", "stats_call_whole",
                 "stats_call_exome", "count_host1", "count_hostN", "stats_host1_whole", "stats_hostN_whole",
                 "stats_host1_exome", "stats_hostN_exome"]
        legs = {k: [] for k in names}
        same = True
        for _ in range(a.rounds):
            legs["runs_kernel"].append(runs_kernel())
            ms, ok = scan_kernel()
            legs["scan_kernel"].append(ms)
            same &= ok
            for k in sets:
                ms, ok = stats_kernel(k)
                legs["stats_kernel_" + k].append(ms)
                same &= ok
            ms, d = call_count()
            legs["count_call"].append(ms)
            same &= bool((d == depth).all())
            for k in sets:
                ms, (hist, lh, sm) = call_stats(k)
                legs["stats_call_" + k].append(ms)
                same &= bool((hist == want[k][0]).all() and (lh == want[k][1]).all() and sm.tobytes() == want[k][2].tobytes())
            ms, d = host_count(1)
            legs["count_host1"].append(ms)
            same &= bool((d == depth).all())
            legs["count_hostN"].append(host_count(a.host_threads)[0])
            for k, pc in sets.items():
                ms, (hist, lh, sm) = host_stats(pc, 1)
                legs[f"stats_host1_{k}"].append(ms)
                same &= bool((hist == want[k][0]).all() and sm.tobytes() == want[k][2].tobytes())
                legs[f"stats_hostN_{k}"].append(host_stats(pc, a.host_threads)[0])
        print(json.dumps(dict(records=n, loci=length, counted_bases=int(depth.sum()), pieces_whole=len(sets["whole"]),
                              pieces_exome=len(sets["exome"]), input_mb=round(sum(x.nbytes for x in arrays) / 1e6, 1),
                              **{k + "_ms": summary(v) for k, v in legs.items()}, host_threads=a.host_threads,
                              rounds=a.rounds, kernel_reps=a.kernel_reps, identical=bool(same))), flush=True)
        if not same:
            return 1
    return 0


def command_ab(a):
    work = a.ab
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(ROOT, "falcon-genome_amd", "bin", "fcs-genome")
    env = dict(os.environ, FCS_TEMP_DIR=work, FCS_LOG_DIR=os.path.join(work, "log"))

    def run(args, **kw):
        t0 = time.perf_counter()
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, cwd=work, timeout=900, env=dict(env, **kw))
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-3000:])
        return time.perf_counter() - t0, r.stderr

    d = os.path.join(work, "in")
    run(["synth", "-o", d, "-c", f"chr1:{int(a.ab_mbp * 1e6)}", "-x", a.ab_cov, "--seed", a.seed, "--no-fastq"])
    cmd = ["depth", "-f", "-r", os.path.join(d, "ref.fasta"), "-i", os.path.join(d, "sample.bam")]
    for omit in (["-b"], []):
        for window in a.window_bp:
            walls = {"false": [], "true": []}
            for rnd in range(a.rounds + 1):   # round 0 warms the page cache and is dropped
                line = ""
                for gpu in (("false", "true") if rnd % 2 else ("true", "false")):
                    dt, err = run(cmd + ["-o", os.path.join(work, gpu)] + omit, FCS_DEPTH_GPU=gpu, FCS_DEPTH_WINDOW_BP=str(window))
                    line = [ln for ln in err.split("\n") if ln.startswith("[fcs-genome depth]") and " records" in ln][0]
                    if ("(GPU)" in line) != (gpu == "true"):
                        raise RuntimeError("the wrong path ran: " + line)
                    if rnd:
                        walls[gpu].append(dt)
                same = all(open(os.path.join(work, "true" + e), "rb").read() == open(os.path.join(work, "false" + e), "rb").read()
                           for e in SUFFIXES if not (omit and e == ""))
                print(f"window {window} {'-b ' if omit else ''}round {rnd}: identical files {same}; {line}", flush=True)
                if not same:
                    return 1
            pairs = list(zip(walls["false"], walls["true"]))
            print(json.dumps(dict(ab_mbp=a.ab_mbp, coverage=a.ab_cov, window_bp=window, per_locus_file=not omit, rounds=a.rounds,
                                  wall_s_host=[round(x, 3) for x in walls["false"]],
                                  wall_s_gpu=[round(x, 3) for x in walls["true"]],
                                  gpu_below_host_in_every_pair=all(g < h for h, g in pairs))), flush=True)
    return 0


def main():
    ints = lambda s: [int(x) for x in s.split(",")]  # noqa: E731
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=ints, default=[200_000, 1_000_000, 2_000_000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--ab", metavar="DIR", default=None)
    ap.add_argument("--ab-mbp", type=float, default=4.0)
    ap.add_argument("--ab-cov", type=int, default=30)
    ap.add_argument("--window-bp", type=ints, default=[4 << 20, 16 << 20, 64 << 20])
    a = ap.parse_args()
    return command_ab(a) if a.ab else bench_sizes(a)


if __name__ == "__main__":
    sys.exit(main())
