#!/usr/bin/env python3
"""Base quality recalibration on the GPU against the host path it would
replace.  A tool, not a test.

Batches are synthesised (seeded): 151M reads of --read-groups read groups
(grouped, as the commands flatten them) on one contig of --mbp Mbp, --err-rate
of the bases changed, 3% of the positions known sites, qualities drawn from
eight values (so the table's cells are as hot as in real data), half of the
reads on the reverse strand, half second of pair.

Per size, --rounds rounds of these legs, alternated on the same box:
  kernels  fcsbq_count_dev and fcsbq_apply_dev, each between two device
           events, inputs resident (--kernel-reps launches per window), for
           every replica count of --replicas (FCS_BQ_REPLICAS);
  call     fcsbq_count and fcsbq_apply from and to host arrays;
  host     bqsr_count_host and bqsr_apply_host (fcsg_bqsr_*), on one thread
           and on --host-threads threads.
Prints one JSON line per size with the median, min and max of each leg in
milliseconds, and checks that the legs give the same tables and bytes.

--ab DIR runs `fcs-genome bqsr` on a synthetic BAM (--ab-mbp, --ab-cov) with
its truth.vcf as known sites, bqsr.gpu off and on, alternated --rounds times
for every chunk size of --chunk-records; it requires byte-identical BAMs and
reports and prints both walls.

  tools/bench_bqsr.py --rounds 3
  tools/bench_bqsr.py --ab /tmp/bqab --rounds 3
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


def synth(n, seed, mbp, err_rate, n_rg):
    """(the arrays of an fcsbq_batch of n records, reference bases, ref_off, known bitmap)."""
    rng = np.random.default_rng(seed)
    L = int(mbp * 1e6)
    ref = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)]
    bits = np.packbits(rng.random(((L + 63) // 64 + 1) * 64) < 0.03, bitorder="little").view(np.uint64)
    pos = rng.integers(0, L - READ, n).astype(np.int32)
    bases = ref[(pos[:, None] + np.arange(READ)[None, :]).ravel()].copy()
    wrong = rng.random(n * READ) < err_rate
    bases[wrong] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(wrong.sum()))]
    qual = np.array([2, 11, 25, 30, 33, 37, 40, 40], np.uint8)[rng.integers(0, 8, n * READ)]
    flag = (np.where(rng.random(n) < 0.5, 0x10, 0) | np.where(rng.random(n) < 0.5, 0x81, 0x41)).astype(np.uint16)
    rg = np.sort(rng.integers(0, n_rg, n)).astype(np.int32)
    return ((flag, np.zeros(n, np.int32), pos, np.full(n, 60, np.uint8), rg, np.full(n, READ << 4, np.uint32),
             np.arange(n + 1, dtype=np.int64), bases, qual, np.arange(n + 1, dtype=np.int64) * READ,
             np.zeros(n, np.uint8)), ref, np.array([0, L], np.int64), bits)


def summary(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def bench_sizes(a):
    import torch
    import bqsr_cases as B
    import fcship
    import host_lib as H
    L = H.lib
    L.fcsg_bqsr_count.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int,
                                  C.c_void_p, C.c_void_p]
    L.fcsg_bqsr_finalize.argtypes = [C.c_int32] + [C.c_void_p] * 5
    L.fcsg_bqsr_apply.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    dev = torch.device("cuda", a.device)
    n_rg = a.read_groups
    views = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}
    for size in a.sizes:
        arrays, ref, ref_off, bits = synth(size, a.seed, a.mbp, a.err_rate, n_rg)
        arrays = fcship.bq_arrays(*arrays)
        hb = fcship.bq_batch(arrays)
        n, nb = len(arrays[0]), len(arrays[7])
        stream = torch.cuda.Stream(device=dev)

        def host_count(threads):
            ctx, cyc = B.new_tables(n_rg)
            t0 = time.perf_counter()
            H.check(L.fcsg_bqsr_count(C.addressof(hb), ref.ctypes.data, ref_off.ctypes.data, 1, bits.ctypes.data, n_rg,
                                      threads, ctx.ctypes.data, cyc.ctypes.data))
            return (time.perf_counter() - t0) * 1e3, (ctx, cyc)

        _, (hctx, hcyc) = host_count(a.host_threads)
        tables = [np.zeros((n_rg, B.NQ)), np.zeros((n_rg, B.NQ, B.NCTX)), np.zeros((n_rg, B.NQ, B.NCYC))]
        H.check(L.fcsg_bqsr_finalize(n_rg, hctx.ctypes.data, hcyc.ctypes.data, *[t.ctypes.data for t in tables]))

        def host_apply(threads):
            out = np.zeros(nb + 1, np.uint8)
            t0 = time.perf_counter()
            H.check(L.fcsg_bqsr_apply(C.addressof(hb), n_rg, *[t.ctypes.data for t in tables], threads, out.ctypes.data))
            return (time.perf_counter() - t0) * 1e3, out[:nb]

        with fcship.bq_ref(ref, ref_off, bits, device=a.device) as handle:
            with torch.cuda.stream(stream):
                t = [torch.from_numpy(x.view(views.get(x.dtype, x.dtype))).to(dev) for x in arrays]
                p = [x.data_ptr() for x in t]
                db = fcship.BqBatch(n, p[0], p[1], p[2], p[3], p[4], p[5], p[6], len(arrays[5]), p[7], p[8], p[9], nb, p[10])
                dtab = [torch.from_numpy(x).to(dev) for x in tables]
                dctx = torch.zeros(hctx.shape, dtype=torch.int64, device=dev)
                dcyc = torch.zeros(hcyc.shape, dtype=torch.int64, device=dev)
                dout = torch.zeros(nb, dtype=torch.uint8, device=dev)
                status = torch.zeros(2, dtype=torch.int32, device=dev)

            def timed(launch):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(stream):
                    e0.record(stream)
                    for _ in range(a.kernel_reps):
                        launch()
                    e1.record(stream)
                stream.synchronize()
                return e0.elapsed_time(e1) / a.kernel_reps

            def count_kernels(replicas):
                os.environ["FCS_BQ_REPLICAS"] = str(replicas)
                need = fcship.lib.fcsbq_workspace_bytes(n_rg)
                ws = torch.empty(need, dtype=torch.uint8, device=dev)
                dctx.zero_(), dcyc.zero_()
                ms = timed(lambda: fcship.check(fcship.lib.fcsbq_count_dev(
                    handle.handle, C.addressof(db), n_rg, ws.data_ptr(), need, dctx.data_ptr(), dcyc.data_ptr(),
                    status.data_ptr(), C.c_void_p(stream.cuda_stream))))
                os.environ.pop("FCS_BQ_REPLICAS")
                ok = ((dctx.cpu().numpy() == a.kernel_reps * hctx).all() and (dcyc.cpu().numpy() == a.kernel_reps * hcyc).all()
                      and int(status.cpu()[0]) == 0)
                return ms, bool(ok)

            def apply_kernels():
                return timed(lambda: fcship.check(fcship.lib.fcsbq_apply_dev(
                    a.device, C.addressof(db), n_rg, dtab[0].data_ptr(), dtab[1].data_ptr(), dtab[2].data_ptr(),
                    dout.data_ptr(), status[1:].data_ptr(), C.c_void_p(stream.cuda_stream))))

            def call_count():
                t0 = time.perf_counter()
                out = fcship.bq_count(handle, arrays, n_rg)
                return (time.perf_counter() - t0) * 1e3, out

            def call_apply():
                t0 = time.perf_counter()
                out = fcship.bq_apply(arrays, *tables, device=a.device)
                return (time.perf_counter() - t0) * 1e3, out

            count_kernels(a.replicas[0]), apply_kernels(), call_count(), call_apply()   # warm-up
            legs = {k: [] for k in ("apply_kernels", "count_call", "apply_call", "count_host1", "apply_host1", "count_hostN",
                                    "apply_hostN")}
            reps = {r: [] for r in a.replicas}
            same = True
            for _ in range(a.rounds):
                for r in a.replicas:
                    ms, ok = count_kernels(r)
                    reps[r].append(ms)
                    same &= ok
                legs["apply_kernels"].append(apply_kernels())
                ms, (cctx, ccyc) = call_count()
                legs["count_call"].append(ms)
                ms, cout = call_apply()
                legs["apply_call"].append(ms)
                legs["count_host1"].append(host_count(1)[0])
                ms, hout = host_apply(1)
                legs["apply_host1"].append(ms)
                legs["count_hostN"].append(host_count(a.host_threads)[0])
                legs["apply_hostN"].append(host_apply(a.host_threads)[0])
                same &= bool((cctx == hctx).all() and (ccyc == hcyc).all() and cout.tobytes() == hout.tobytes()
                             and dout.cpu().numpy().tobytes() == hout.tobytes())
        print(json.dumps(dict(records=n, bases=nb, read_groups=n_rg, observations=int(hcyc[..., 0].sum()),
                              errors=int(hcyc[..., 1].sum()), input_mb=round(sum(x.nbytes for x in arrays) / 1e6, 1),
                              count_kernels_ms={f"R{r}": summary(v) for r, v in reps.items()},
                              **{k + "_ms": summary(v) for k, v in legs.items()}, host_threads=a.host_threads,
                              rounds=a.rounds, identical=bool(same))), flush=True)
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
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, cwd=work, timeout=900,
                           env=dict(env, **kw))
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-3000:])
        return time.perf_counter() - t0, r.stderr

    d = os.path.join(work, "in")
    run(["synth", "-o", d, "-c", f"chr1:{int(a.ab_mbp * 1e6)}", "-x", a.ab_cov, "--seed", a.seed, "--no-fastq"])
    cmd = ["bqsr", "-f", "-r", os.path.join(d, "ref.fasta"), "-i", os.path.join(d, "sample.bam"),
           "-K", os.path.join(d, "truth.vcf")]
    rc = 0
    for chunk in a.chunk_records:
        walls = {"false": [], "true": []}
        line = ""
        for rnd in range(a.rounds + 1):   # round 0 warms the page cache and is dropped
            for gpu in (("false", "true") if rnd % 2 else ("true", "false")):
                dt, err = run(cmd + ["-o", os.path.join(work, f"{gpu}.bam"), "-b", os.path.join(work, f"{gpu}.grp")],
                              FCS_BQSR_GPU=gpu, FCS_BQSR_CHUNK_RECORDS=str(chunk))
                line = [ln for ln in err.split("\n") if ln.startswith("[fcs-genome bqsr]") and " records" in ln][0]
                if ("(GPU)" in line) != (gpu == "true"):
                    raise RuntimeError("the wrong path ran: " + line)
                if rnd:
                    walls[gpu].append(dt)
            same = all(open(os.path.join(work, "true" + e), "rb").read() == open(os.path.join(work, "false" + e), "rb").read()
                       for e in (".bam", ".bam.bai", ".grp"))
            print(f"chunk {chunk} round {rnd}: identical BAM, index and report {same}; {line}", flush=True)
            if not same:
                return 1
        pairs = list(zip(walls["false"], walls["true"]))
        print(json.dumps(dict(ab_mbp=a.ab_mbp, coverage=a.ab_cov, chunk_records=chunk, rounds=a.rounds,
                              wall_s_host=[round(x, 3) for x in walls["false"]],
                              wall_s_gpu=[round(x, 3) for x in walls["true"]],
                              gpu_below_host_in_every_pair=all(g < h for h, g in pairs))), flush=True)
    return rc


def main():
    ints = lambda s: [int(x) for x in s.split(",")]  # noqa: E731
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=ints, default=[200_000, 1_000_000, 2_000_000])
    ap.add_argument("--replicas", type=ints, default=[1, 4, 8, 16])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--read-groups", type=int, default=2)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--mbp", type=float, default=4.0)
    ap.add_argument("--err-rate", type=float, default=0.01)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--ab", metavar="DIR", default=None)
    ap.add_argument("--ab-mbp", type=float, default=4.0)
    ap.add_argument("--ab-cov", type=int, default=30)
    ap.add_argument("--chunk-records", type=ints, default=[250_000, 1_000_000])
    a = ap.parse_args()
    return command_ab(a) if a.ab else bench_sizes(a)


if __name__ == "__main__":
    sys.exit(main())
