#!/usr/bin/env python3
"""Duplicate marking on the GPU against the host path it would replace
(DESIGN.md §4.9).  A tool, not a test.

Batches are synthesised (seeded): 2x151 pairs and --frag-rate fragments on
one contig of --mbp Mbp, --dup-rate of the templates repeating an earlier
template's coordinates, --clip-rate of the reads soft-clipped at their 5' end
(same unclipped position), qualities uniform in [2, 40].  Sizes: the bench's
align shape (about 800K records) and a few larger ones (--sizes).

Per size, --rounds rounds of three legs, alternated on the same box:
  kernels  fcsdup_mark_dev between two device events, inputs resident
           (--kernel-reps launches per window);
  call     fcsdup_mark from and to host arrays (checks, staging, one H2D and
           one D2H copy);
  host     mark_duplicates_host (fcsg_markdup), one thread.
Prints one JSON line per size with the median, min and max of each leg in
milliseconds, and checks that the three legs give the same bytes.

--align-ab DIR runs `fcs-genome align` on a synthetic 2x151 sample
(--align-mbp, 30x, every --align-repeat-th pair once more) with
markdup.in_align=true and markdup.gpu off and on, alternated --rounds times,
requires byte-identical BAMs and prints both walls and the report lines.

  tools/bench_markdup.py --rounds 3
  tools/bench_markdup.py --align-ab /tmp/mdab --rounds 3
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


def synth(n_records, seed, mbp, dup_rate, frag_rate, clip_rate, read_len=151):
    """The SoA arrays of an fcsdup_batch with about n_records records."""
    rng = np.random.default_rng(seed)
    T = int(n_records / (2 - frag_rate))
    frag = rng.random(T) < frag_rate
    L = int(mbp * 1e6)
    p1 = rng.integers(0, L - 1000, T)
    p2 = p1 + rng.integers(200, 500, T)
    rev1 = rng.random(T) < 0.5
    dup = rng.random(T) < dup_rate
    dup[0] = False
    orig = np.flatnonzero(~dup)
    src = np.arange(T)
    src[dup] = orig[rng.integers(0, len(orig), int(dup.sum()))]
    frag, p1, p2, rev1 = frag[src], p1[src], p2[src], rev1[src]
    count = np.where(frag, 1, 2)
    start = np.cumsum(count) - count
    n = int(count.sum())
    flag, pos, mate = np.zeros(n, np.uint16), np.zeros(n, np.int32), np.full(n, -1, np.int32)
    rev = np.zeros(n, bool)
    a, b = start, start[~frag] + 1
    pos[a], rev[a] = p1, rev1
    flag[a] = np.where(frag, 0, 0x1 | 0x40 | np.where(rev1, 0, 0x20)).astype(np.uint16)
    pos[b], rev[b] = p2[~frag], ~rev1[~frag]
    flag[b] = (0x1 | 0x80 | np.where(rev1[~frag], 0x20, 0)).astype(np.uint16)
    mate[start[~frag]], mate[b] = b, start[~frag]
    flag |= (rev * 0x10).astype(np.uint16)
    clip = np.where(rng.random(n) < clip_rate, rng.integers(1, 30, n), 0)
    pos = (pos + np.where(rev, 0, clip)).astype(np.int32)   # a forward read's clip leads, a reverse read's trails
    n_ops = np.where(clip > 0, 2, 1)
    coff = np.concatenate([[0], np.cumsum(n_ops)]).astype(np.int64)
    cigar = np.zeros(coff[-1], np.uint32)
    m_op = ((read_len - clip) << 4).astype(np.uint32)
    s_op = ((clip << 4) | 4).astype(np.uint32)
    first = coff[:-1]
    cigar[first] = np.where((clip > 0) & ~rev, s_op, m_op)
    two = clip > 0
    cigar[first[two] + 1] = np.where(rev[two], s_op[two], m_op[two])
    qoff = (np.arange(n + 1, dtype=np.int64) * read_len)
    qual = rng.integers(2, 41, n * read_len, dtype=np.uint8)
    return (flag, np.zeros(n, np.int32), pos, mate, np.zeros(n, np.int32), cigar, coff, qual, qoff)


def summary(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def bench_sizes(a):
    import torch
    import fcship
    import host_lib as H
    dev = torch.device("cuda", a.device)
    f = H.lib.fcsg_markdup
    f.argtypes = [C.c_int64] + [C.c_void_p] * 9 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    for size in a.sizes:
        arrays = fcship.dup_arrays(*synth(size, a.seed, a.mbp, a.dup_rate, a.frag_rate, a.clip_rate))
        n = len(arrays[0])
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            t = [torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x.view(np.int32) if x.dtype == np.uint32
                                  else x).to(dev) for x in arrays]
            need = fcship.lib.fcsdup_workspace_bytes(n)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            ddup = torch.zeros(n, dtype=torch.uint8, device=dev)
            dst = torch.zeros(4, dtype=torch.int64, device=dev)
            dstatus = torch.zeros(1, dtype=torch.int32, device=dev)
        b = fcship.DupBatch(n, *[x.data_ptr() for x in t[:7]], len(arrays[5]), t[7].data_ptr(), t[8].data_ptr(),
                            len(arrays[7]), 1, 1)

        def kernels():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                for _ in range(a.kernel_reps):
                    fcship.check(fcship.lib.fcsdup_mark_dev(a.device, C.addressof(b), ws.data_ptr(), need, ddup.data_ptr(),
                                                            dst.data_ptr(), dstatus.data_ptr(),
                                                            C.c_void_p(stream.cuda_stream)))
                e1.record(stream)
            stream.synchronize()
            return e0.elapsed_time(e1) / a.kernel_reps

        def call():
            t0 = time.perf_counter()
            out = fcship.dup_mark(arrays, 1, 1, device=a.device)
            return (time.perf_counter() - t0) * 1e3, out

        hdup, hst = np.zeros(n, np.uint8), np.zeros(4, np.int64)

        def host():
            t0 = time.perf_counter()
            H.check(f(n, *[x.ctypes.data for x in arrays], 1, 1, hdup.ctypes.data, hst.ctypes.data))
            return (time.perf_counter() - t0) * 1e3

        kernels(), call()   # warm-up: code objects, the session's arenas
        tk, tc, th = [], [], []
        for _ in range(a.rounds):
            tk.append(kernels())
            ms, (cdup, cst) = call()
            tc.append(ms)
            th.append(host())
        same = (cdup.tobytes() == hdup.tobytes() == ddup.cpu().numpy().tobytes() and int(dstatus.cpu()[0]) == 0)
        print(json.dumps(dict(records=n, pairs=int(cst["pairs"]), fragments=int(cst["fragments"]),
                              duplicates=int(cst["duplicates"]), dup_share=round(cst["duplicates"] / n, 3),
                              input_mb=round(sum(x.nbytes for x in arrays) / 1e6, 1), workspace_mb=round(need / 1e6, 1),
                              kernels_ms=summary(tk), call_ms=summary(tc), host_ms=summary(th), rounds=a.rounds,
                              identical=bool(same))), flush=True)
        if not same:
            return 1
    return 0


def align_ab(a):
    work = a.align_ab
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
    run(["synth", "-o", d, "-c", f"chr1:{int(a.align_mbp * 1e6)}", "-x", "30", "--paired", "350", "--seed", a.seed,
         "--no-fastq"])
    run(["index", "-r", os.path.join(d, "ref.fasta"), "--sa-intv", "32"])
    fq = []
    for k in (1, 2):   # every align_repeat-th pair once more under another name
        lines = open(os.path.join(d, f"sample_{k}.fastq")).read().split("\n")
        reads = [lines[i:i + 4] for i in range(0, len(lines) - 3, 4)]
        extra = [["@again_" + r[0][1:], r[1], r[2], r[3]] for r in reads[::a.align_repeat]]
        path = os.path.join(work, f"r{k}.fastq")
        open(path, "w").write("\n".join("\n".join(r) for r in reads + extra) + "\n")
        fq.append(path)
    cmd = ["align", "-f", "-r", os.path.join(d, "ref.fasta"), "-1", fq[0], "-2", fq[1], "-o"]
    walls, marks = {"false": [], "true": []}, {"false": [], "true": []}
    for rnd in range(a.rounds + 1):   # round 0 warms the page cache and is dropped
        for gpu in (("false", "true") if rnd % 2 else ("true", "false")):
            dt, err = run(cmd + [os.path.join(work, f"{gpu}.bam")], FCS_MARKDUP_IN_ALIGN="true", FCS_MARKDUP_GPU=gpu)
            line = [ln for ln in err.split("\n") if "mark duplicates:" in ln][0]
            if rnd:
                walls[gpu].append(dt)
                marks[gpu].append(float(line.split(" records flagged, ")[1].split(" s ")[0]))
        same = open(os.path.join(work, "true.bam"), "rb").read() == open(os.path.join(work, "false.bam"), "rb").read()
        print(f"round {rnd}: identical BAMs {same}; {line}", flush=True)
        if not same:
            return 1
    pairs = list(zip(walls["false"], walls["true"]))
    print(json.dumps(dict(align_mbp=a.align_mbp, rounds=a.rounds, wall_s_host=[round(x, 3) for x in walls["false"]],
                          wall_s_gpu=[round(x, 3) for x in walls["true"]],
                          mark_s_host=marks["false"], mark_s_gpu=marks["true"],
                          gpu_below_host_in_every_pair=all(g < h for h, g in pairs))), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[800_000, 2_000_000, 4_000_000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--mbp", type=float, default=4.0)
    ap.add_argument("--dup-rate", type=float, default=0.15)
    ap.add_argument("--frag-rate", type=float, default=0.05)
    ap.add_argument("--clip-rate", type=float, default=0.10)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--align-ab", metavar="DIR", default=None)
    ap.add_argument("--align-mbp", type=float, default=4.0)
    ap.add_argument("--align-repeat", type=int, default=10)
    a = ap.parse_args()
    return align_ab(a) if a.align_ab else bench_sizes(a)


if __name__ == "__main__":
    sys.exit(main())
