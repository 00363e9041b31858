#!/usr/bin/env python3
"""The callers' pileup on the GPU against the host walk it would replace
(DESIGN.md §4.15).  A tool, not a test.

A window of the C4 shape is synthesised (seeded, tools/bench_ug.py's batch):
151M reads sorted by position at --coverage on one random contig of about
--mbp Mbp, read letters copied from the contig with a --mismatch rate of other
letters, qualities drawn from eight values; one call over the whole contig, gl
wanted, as htc's GVCF mode asks.

--rounds rounds of these legs after a warm-up, alternated on the same box:
  kernels  fcspu_pile_dev between two device events, inputs resident
           (--kernel-reps launches);
  call     fcspu_pile from and to host arrays;
  host     the exported host statement (fcsg_pu_pile) on one thread, which is
           how a shard runs it.
Prints one JSON line with the median, min and max of each leg in milliseconds,
and checks that the legs give the same arrays, the doubles bit for bit.

--ab DIR runs `fcs-genome htc` (GVCF) on a synthetic BAM of --ab-mbp Mbp at 30x
with htc.gpu_pileup off and on, alternated --rounds times after a dropped
warm-up; with --parent DIR (a build of the parent commit: DIR/bin/fcs-genome)
the parent's binary takes part in every alternation as the baseline.  It
requires byte-identical files and prints every run's wall and the shard lines'
sums: pileup seconds, total seconds, and with the key on the chunks, the time
inside fcspu_pile and the runner's flatten time.

  tools/bench_pileup.py --rounds 5
  tools/bench_pileup.py --ab /tmp/puab --rounds 3
"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "falcon-genome_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from bench_ug import READ, summary, synth  # noqa: E402

KEYS = ("depth", "events", "gl", "sites", "snvs")


def bench_call(a):
    import torch
    import fcship
    import host_lib as H
    dev = torch.device("cuda", a.device)
    views = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    n = int(a.mbp * 1e6 * a.coverage / READ)
    arrays, contig = synth(n, a.seed, a.coverage, a.mismatch)
    arrays = fcship.ug_arrays(*arrays)
    length = len(contig)
    table = fcship.pu_table()
    window = (0, 0, length, length)

    def host_entry(batches, nb, prm, w, ref, events_in, out):
        H.check(H.lib.fcsg_pu_pile(C.c_void_p(batches), nb, C.c_void_p(prm), C.c_void_p(w), C.c_void_p(ref), C.c_void_p(events_in),
                                   C.c_void_p(out)))

    def timed(**kw):
        clock = {}   # the entry alone: not the fresh output arrays
        out = fcship.pu_pile([arrays], window, contig, table, min_bq=a.min_bq, frac=a.frac, clock=clock, **kw)
        return clock["seconds"] * 1e3, out

    def equal(x, y):
        return all(np.ascontiguousarray(x[k]).tobytes() == np.ascontiguousarray(y[k]).tobytes() for k in KEYS)

    _, want = timed(entry=host_entry)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        t = [torch.from_numpy(x.view(views.get(x.dtype, x.dtype))).to(dev) for x in arrays]
        p = [x.data_ptr() for x in t]
        db = (fcship.UgBatch * 1)(fcship.UgBatch(n, p[0], p[1], p[2], p[3], p[4], p[5], len(arrays[4]), p[6], p[7], p[8],
                                                len(arrays[7]), p[9]))
        dref, dtab = torch.from_numpy(contig).to(dev), torch.from_numpy(table).to(dev)
        o = dict(depth=torch.zeros(length, dtype=torch.int32, device=dev), events=torch.zeros(length, dtype=torch.int32, device=dev),
                 gl=torch.zeros(3 * length, dtype=torch.float64, device=dev), sites=torch.zeros(length, dtype=torch.int32, device=dev),
                 snvs=torch.zeros(12 * 4 * length, dtype=torch.uint8, device=dev), counts=torch.zeros(2, dtype=torch.int64, device=dev),
                 status=torch.zeros(1, dtype=torch.int32, device=dev))
        out = fcship.PuOut(o["depth"].data_ptr(), o["events"].data_ptr(), o["gl"].data_ptr(), o["sites"].data_ptr(), length,
                           o["counts"].data_ptr(), o["snvs"].data_ptr(), 4 * length, o["counts"].data_ptr() + 8)
        need = fcship.pu_workspace_bytes([n], length)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    w, prm = fcship.UgWindow(0, 0, 0, length, length), fcship.PuParams(a.min_bq, 1, a.frac)
    sp = C.c_void_p(stream.cuda_stream)

    def kernels():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            for _ in range(a.kernel_reps):
                fcship.check(fcship.lib.fcspu_pile_dev(a.device, C.addressof(db), 1, C.addressof(prm), C.addressof(w), dref.data_ptr(),
                                                       dtab.data_ptr(), 0, C.addressof(out), ws.data_ptr(), need,
                                                       o["status"].data_ptr(), sp))
            e1.record(stream)
        stream.synchronize()
        ns, nv = (int(x) for x in o["counts"].cpu())
        got = dict(depth=o["depth"].cpu().numpy(), events=o["events"].cpu().numpy(), gl=o["gl"].cpu().numpy(),
                   sites=o["sites"].cpu().numpy()[:ns], snvs=o["snvs"].cpu().numpy()[:12 * nv])
        return e0.elapsed_time(e1) / a.kernel_reps, int(o["status"].cpu()[0]) == 0 and equal(got, want)

    kernels(), timed(device=a.device)   # warm-up
    legs = {k: [] for k in ("kernels", "call", "host1")}
    same = True
    for _ in range(a.rounds):
        ms, ok = kernels()
        legs["kernels"].append(ms)
        same &= ok
        ms, got = timed(device=a.device)
        legs["call"].append(ms)
        same &= equal(got, want)
        ms, got = timed(entry=host_entry)
        legs["host1"].append(ms)
        same &= equal(got, want)
    print(json.dumps(dict(records=n, loci=length, coverage=a.coverage, aligned_bases=n * READ, sites=len(want["sites"]),
                          snvs=len(want["snvs"]), input_mb=round(sum(x.nbytes for x in arrays) / 1e6, 1),
                          output_mb=round(32 * length / 1e6, 1), **{k + "_ms": summary(v) for k, v in legs.items()},
                          rounds=a.rounds, kernel_reps=a.kernel_reps, identical=bool(same))), flush=True)
    return 0 if same else 1


SHARD = re.compile(r"\] shard \d+ gpu \d+: .*? calls, ([\d.]+) s \(PairHMM .*?, pileup ([\d.]+) s, regions ")
PILE = re.compile(r"\] shard \d+ pileup: (\d+) gpu chunks, (\d+) host chunks, device ([\d.]+) s, flatten ([\d.]+) s")


def command_ab(a):
    work = os.path.abspath(a.ab)
    os.makedirs(work, exist_ok=True)
    exes = {"off": os.path.join(ROOT, "falcon-genome_amd", "bin", "fcs-genome")}
    exes["on"] = exes["off"]
    if a.parent:
        exes["parent"] = os.path.join(os.path.abspath(a.parent), "bin", "fcs-genome")
    env = dict(os.environ, FCS_TEMP_DIR=work, FCS_LOG_DIR=os.path.join(work, "log"), FCS_GATK_NPROCS="16",
               FCS_GPU_DEVICES=str(a.device))

    def run(exe, args, **kw):
        shutil.rmtree(env["FCS_LOG_DIR"], ignore_errors=True)
        t0 = time.perf_counter()
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, cwd=work, timeout=1500, env=dict(env, **kw))
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-3000:])
        logs = r.stderr
        if os.path.isdir(env["FCS_LOG_DIR"]):
            for f in sorted(os.listdir(env["FCS_LOG_DIR"])):
                logs += open(os.path.join(env["FCS_LOG_DIR"], f), errors="replace").read()
        return dt, logs

    d = os.path.join(work, "in")
    if not os.path.exists(os.path.join(d, "sample.bam")):
        run(exes["off"], ["synth", "-o", d, "-c", f"chr1:{int(a.ab_mbp * 1e6)}", "-x", a.ab_cov, "--no-fastq", "--noisy-frac", "0.01",
                          "--seed", a.seed])
    cmd = ["htc", "-f", "-r", os.path.join(d, "ref.fasta"), "-i", os.path.join(d, "sample.bam")]
    res = {k: [] for k in exes}
    order = list(exes)
    for rnd in range(a.rounds + 1):   # round 0 warms the page cache and is dropped
        for leg in order[rnd % len(order):] + order[:rnd % len(order)]:
            kw = {} if leg == "parent" else {"FCS_HTC_GPU_PILEUP": "true" if leg == "on" else "false",
                                             "FCS_HTC_PILEUP_CHUNK_BP": str(a.chunk_bp)}
            dt, logs = run(exes[leg], cmd + ["-o", os.path.join(work, leg + ".g.vcf")], **kw)
            shards, piles = SHARD.findall(logs), PILE.findall(logs)
            row = dict(wall_s=round(dt, 3), shards=len(shards), shard_seconds=round(sum(float(s) for s, _ in shards), 3),
                       pileup_seconds=round(sum(float(p) for _, p in shards), 3))
            if leg == "on":
                row.update(gpu_chunks=sum(int(x[0]) for x in piles), host_chunks=sum(int(x[1]) for x in piles),
                           device_seconds=round(sum(float(x[2]) for x in piles), 3),
                           flatten_seconds=round(sum(float(x[3]) for x in piles), 3))
                if row["gpu_chunks"] == 0:
                    raise RuntimeError("the device path did not run")
            print(f"round {rnd} {leg}: {json.dumps(row)}", flush=True)
            if rnd:
                res[leg].append(row)
        same = all(open(os.path.join(work, k + ".g.vcf" + e), "rb").read() == open(os.path.join(work, "off.g.vcf" + e), "rb").read()
                   for k in exes for e in ("", ".gz", ".gz.tbi"))
        print(f"round {rnd}: identical files {same}", flush=True)
        if not same:
            return 1
    print(json.dumps(dict(ab_mbp=a.ab_mbp, coverage=a.ab_cov, chunk_bp=a.chunk_bp, rounds=a.rounds,
                          **{leg: {k: [r[k] for r in rows] for k in rows[0]} for leg, rows in res.items() if rows})), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=1.0)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--mismatch", type=float, default=0.005)
    ap.add_argument("--min-bq", type=int, default=10)
    ap.add_argument("--frac", type=float, default=0.15)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--ab", metavar="DIR", default=None)
    ap.add_argument("--parent", metavar="DIR", default=None)
    ap.add_argument("--ab-mbp", type=float, default=31.0)
    ap.add_argument("--ab-cov", type=int, default=30)
    ap.add_argument("--chunk-bp", type=int, default=1 << 20)
    a = ap.parse_args()
    return command_ab(a) if a.ab else bench_call(a)


if __name__ == "__main__":
    sys.exit(main())
