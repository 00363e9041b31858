#!/usr/bin/env python3
"""Pileup SNP genotyping on the GPU against the host path it would replace
(DESIGN.md §4.12).  A tool, not a test.

Batches are synthesised (seeded): 151M reads sorted by position at --coverage
on one random contig sized to hold them, read letters copied from the contig
with a --mismatch rate of other letters, qualities drawn from eight values, one
window over the whole contig.

Per size, --rounds rounds of these legs, alternated on the same box:
  kernels  fcsug_sites_dev between two device events, inputs resident
           (--kernel-reps launches);
  call     fcsug_sites from and to host arrays;
  host     ug_sites_host (fcsg_ug_sites), on one thread and on --host-threads
           threads.
Prints one JSON line per size with the median, min and max of each leg in
milliseconds, and checks that the legs give the same sites.

--ab DIR runs `fcs-genome ug` on a synthetic BAM (--ab-mbp, --ab-cov), ug.gpu
off and on, alternated --rounds times after a dropped warm-up for every window
size of --window-bp; it requires byte-identical files and prints both walls.

  tools/bench_ug.py --rounds 3
  tools/bench_ug.py --ab /tmp/ugab --rounds 3
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


def synth(n, seed, coverage, mismatch):
    """(the arrays of an fcsug_batch of n records, the contig as ASCII bytes)."""
    rng = np.random.default_rng(seed)
    length = max(int(n * READ / coverage), 2 * READ)
    letters = np.frombuffer(b"ACGT", np.uint8)
    contig = letters[rng.integers(0, 4, length)]
    pos = np.sort(rng.integers(0, length - READ, n)).astype(np.int32)
    bases = contig[(pos[:, None].astype(np.int64) + np.arange(READ)[None, :]).ravel()].copy()
    swap = np.nonzero(rng.random(n * READ) < mismatch)[0]
    bases[swap] = letters[rng.integers(0, 4, len(swap))]
    qual = np.array([2, 11, 25, 30, 33, 37, 40, 40], np.uint8)[rng.integers(0, 8, n * READ)]
    flag = np.where(rng.random(n) < 0.5, 0x10, 0).astype(np.uint16)
    return (flag, np.zeros(n, np.int32), pos, np.full(n, 60, np.uint8), np.full(n, READ << 4, np.uint32),
            np.arange(n + 1, dtype=np.int64), bases, qual, np.arange(n + 1, dtype=np.int64) * READ, np.zeros(n, np.uint8)), contig


def summary(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def bench_sizes(a):
    import torch
    import fcship
    import host_lib as H
    L = H.lib
    L.fcsg_ug_sites.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                C.c_void_p]
    dev = torch.device("cuda", a.device)
    views = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    prm = fcship.UgParams(17)
    table = fcship.ug_table(1e-4)
    for size in a.sizes:
        arrays, contig = synth(size, a.seed, a.coverage, a.mismatch)
        arrays = fcship.ug_arrays(*arrays)
        length = len(contig)
        hb = fcship.ug_batch(arrays)
        w = fcship.UgWindow(0, 0, 0, length, length)
        n = len(arrays[0])
        stream = torch.cuda.Stream(device=dev)

        def host(threads):
            out, found = np.zeros(length, fcship.UG_SITE), C.c_int64(0)
            t0 = time.perf_counter()
            H.check(L.fcsg_ug_sites(C.addressof(hb), C.addressof(prm), C.addressof(w), contig.ctypes.data, table.ctypes.data,
                                    threads, out.ctypes.data, length, C.addressof(found)))
            return (time.perf_counter() - t0) * 1e3, out[:found.value]

        _, want = host(a.host_threads)

        with torch.cuda.stream(stream):
            t = [torch.from_numpy(x.view(views.get(x.dtype, x.dtype))).to(dev) for x in arrays]
            p = [x.data_ptr() for x in t]
            db = fcship.UgBatch(n, p[0], p[1], p[2], p[3], p[4], p[5], len(arrays[4]), p[6], p[7], p[8], len(arrays[7]), p[9])
            dref = torch.from_numpy(contig).to(dev)
            dtab = torch.from_numpy(table).to(dev)
            dsites = torch.zeros(80 * length, dtype=torch.uint8, device=dev)
            dn = torch.zeros(1, dtype=torch.int64, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            need = fcship.lib.fcsug_workspace_bytes(n, length)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        sp = C.c_void_p(stream.cuda_stream)

        def kernels():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                for _ in range(a.kernel_reps):
                    fcship.check(fcship.lib.fcsug_sites_dev(a.device, C.addressof(db), C.addressof(prm), C.addressof(w),
                                                            dref.data_ptr(), dtab.data_ptr(), dsites.data_ptr(), length,
                                                            dn.data_ptr(), ws.data_ptr(), need, status.data_ptr(), sp))
                e1.record(stream)
            stream.synchronize()
            found = int(dn.cpu()[0])
            ok = (found == len(want) and int(status.cpu()[0]) == 0
                  and dsites.cpu().numpy()[:80 * found].tobytes() == want.tobytes())
            return e0.elapsed_time(e1) / a.kernel_reps, bool(ok)

        def call():
            t0 = time.perf_counter()
            out = fcship.ug_sites(arrays, (0, 0, length, length), contig, table, device=a.device)
            return (time.perf_counter() - t0) * 1e3, out

        kernels(), call()   # warm-up
        legs = {k: [] for k in ("kernels", "call", "host1", "hostN")}
        same = True
        for _ in range(a.rounds):
            ms, ok = kernels()
            legs["kernels"].append(ms)
            same &= ok
            ms, out = call()
            legs["call"].append(ms)
            same &= out.tobytes() == want.tobytes()
            ms, out = host(1)
            legs["host1"].append(ms)
            same &= out.tobytes() == want.tobytes()
            legs["hostN"].append(host(a.host_threads)[0])
        counted = int(want["n"].sum())
        print(json.dumps(dict(records=n, loci=length, sites=len(want), counted_bases_at_sites=counted,
                              input_mb=round(sum(x.nbytes for x in arrays) / 1e6, 1),
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
    cmd = ["ug", "-f", "-r", os.path.join(d, "ref.fasta"), "-i", os.path.join(d, "sample.bam")]
    for window in a.window_bp:
        walls = {"false": [], "true": []}
        for rnd in range(a.rounds + 1):   # round 0 warms the page cache and is dropped
            line = ""
            for gpu in (("false", "true") if rnd % 2 else ("true", "false")):
                dt, err = run(cmd + ["-o", os.path.join(work, gpu + ".vcf")], FCS_UG_GPU=gpu, FCS_UG_WINDOW_BP=str(window))
                line = [ln for ln in err.split("\n") if ln.startswith("[fcs-genome ug]") and " records" in ln][0]
                if ("(GPU)" in line) != (gpu == "true"):
                    raise RuntimeError("the wrong path ran: " + line)
                if rnd:
                    walls[gpu].append(dt)
            same = all(open(os.path.join(work, "true.vcf" + e), "rb").read() == open(os.path.join(work, "false.vcf" + e), "rb").read()
                       for e in ("", ".gz", ".gz.tbi"))
            print(f"window {window} round {rnd}: identical files {same}; {line}", flush=True)
            if not same:
                return 1
        pairs = list(zip(walls["false"], walls["true"]))
        print(json.dumps(dict(ab_mbp=a.ab_mbp, coverage=a.ab_cov, window_bp=window, rounds=a.rounds,
                              wall_s_host=[round(x, 3) for x in walls["false"]],
                              wall_s_gpu=[round(x, 3) for x in walls["true"]],
                              gpu_below_host_in_every_pair=all(g < h for h, g in pairs))), flush=True)
    return 0


def main():
    ints = lambda s: [int(x) for x in s.split(",")]  # noqa: E731
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=ints, default=[200_000, 1_000_000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--mismatch", type=float, default=0.005)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--ab", metavar="DIR", default=None)
    ap.add_argument("--ab-mbp", type=float, default=12.0)
    ap.add_argument("--ab-cov", type=int, default=30)
    ap.add_argument("--window-bp", type=ints, default=[256 << 10, 1 << 20, 4 << 20])
    a = ap.parse_args()
    return command_ab(a) if a.ab else bench_sizes(a)


if __name__ == "__main__":
    sys.exit(main())
