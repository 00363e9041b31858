#!/usr/bin/env python3
"""Indel realignment's scoring step on the GPU against the host path it would
replace.  A tool, not a test.

The batch is synthesised (seeded) at a shape a deep target of a 30x to 60x
genome has: --bins bins of about --reads alt reads x --cons consensuses, reads of
--read-len bases over windows of about --window bases; a bin's consensuses are
its window with one indel each, its reads come from them with a few errors.

--rounds rounds of these legs, alternated on the same box, after --warmup
rounds that are dropped:
  kernels  fcsir_score_dev between two device events, inputs and outputs
           resident (--kernel-reps launches);
  call     fcsir_score from and to host arrays;
  host     ir_score_host (fcsg_ir_score) on --host-threads threads.
Prints one JSON line with the median, min and max of each leg in milliseconds,
the batch's shape, its base comparisons (pairs x offsets x read length), the
comparisons per second of the kernels leg and that rate against the VALU's
lane-operation peak (--cus x 4 SIMDs x 16 lanes x --ghz), and checks that the
legs give the same scores and offsets.

  tools/bench_indel.py --bins 64 --rounds 3
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "falcon-genome_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def synth(a):
    """(the arrays of ir_score, base comparisons)."""
    rng = np.random.default_rng(a.seed)
    seq, seq_off, bin_seq, read, qual, read_off, bin_read, orig = [], [0], [0], [], [], [0], [0], []
    work = 0
    for _ in range(a.bins):
        W = int(rng.integers(a.window - 100, a.window + 101))
        ref = rng.integers(0, 4, W).astype(np.uint8)
        cons = []
        for _ in range(max(1, int(rng.integers(a.cons - 2, a.cons + 3)))):
            u, k = int(rng.integers(50, W - 50)), int(rng.integers(1, 12))
            cons.append(np.concatenate([ref[:u], rng.integers(0, 4, k).astype(np.uint8), ref[u:]]) if rng.random() < 0.5
                        else np.concatenate([ref[:u], ref[u + k:]]))
        n_reads = max(1, int(rng.integers(a.reads * 3 // 4, a.reads * 5 // 4 + 1)))
        for _ in range(n_reads):
            src = cons[int(rng.integers(0, len(cons)))]
            o = int(rng.integers(0, len(src) - a.read_len))
            r = src[o:o + a.read_len].copy()
            bad = rng.random(a.read_len) < 0.01
            r[bad] = rng.integers(0, 4, int(bad.sum()))
            read.append(r), qual.append(rng.integers(2, 42, a.read_len).astype(np.uint8)), read_off.append(read_off[-1] + a.read_len)
            orig.append(min(o + int(rng.integers(-3, 4)) % 7, W))
        for c in cons:
            seq.append(c), seq_off.append(seq_off[-1] + len(c))
            work += n_reads * (len(c) - a.read_len + 2) * a.read_len
        bin_seq.append(len(seq_off) - 1), bin_read.append(len(read_off) - 1)
    return (np.concatenate(seq), np.array(seq_off, np.int64), np.array(bin_seq, np.int64), np.concatenate(read), np.concatenate(qual),
            np.array(read_off, np.int64), np.array(bin_read, np.int64), np.array(orig, np.int32)), work


def summary(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--reads", type=int, default=200)
    ap.add_argument("--cons", type=int, default=8)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--window", type=int, default=900)
    ap.add_argument("--seed", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-reps", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--ghz", type=float, default=2.4)
    a = ap.parse_args()
    import torch
    import fcship
    import host_lib as H
    L = H.lib
    L.fcsg_ir_score.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    arrays, work = synth(a)
    b, keep = fcship.ir_batch(*arrays)
    pairs = fcship.ir_pairs(keep[2], keep[6])
    dev = torch.device("cuda", a.device)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        t = [torch.from_numpy(x.view(np.uint8)).to(dev) for x in keep]
        db = fcship.IrBatch(b.n_bins, b.n_seq, b.n_reads, b.n_seq_bytes, b.n_read_bytes, *(x.data_ptr() for x in t))
        d_best = torch.zeros(pairs, dtype=torch.int32, device=dev)
        d_off = torch.zeros(pairs, dtype=torch.int32, device=dev)
        tail = torch.zeros(2, dtype=torch.int64, device=dev)
        need = fcship.lib.fcsir_workspace_bytes(b.n_bins)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    best_call, off_call, n_call = np.zeros(pairs, np.uint32), np.zeros(pairs, np.int32), C.c_int64(0)
    best_host, off_host = np.zeros(pairs, np.uint32), np.zeros(pairs, np.int32)
    legs = {"kernels": [], "call": [], "host": []}
    for rnd in range(a.warmup + a.rounds):
        if rnd == a.warmup:
            legs = {"kernels": [], "call": [], "host": []}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            for _ in range(a.kernel_reps):
                fcship.check(fcship.lib.fcsir_score_dev(a.device, C.addressof(db), d_best.data_ptr(), d_off.data_ptr(), pairs, tail.data_ptr(),
                                                        ws.data_ptr(), need, tail.data_ptr() + 8, C.c_void_p(stream.cuda_stream)))
            e1.record(stream)
        stream.synchronize()
        legs["kernels"].append(e0.elapsed_time(e1) / a.kernel_reps)
        t0 = time.perf_counter()
        fcship.check(fcship.lib.fcsir_score(a.device, C.addressof(b), best_call.ctypes.data, off_call.ctypes.data, pairs, C.addressof(n_call)))
        legs["call"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        H.check(L.fcsg_ir_score(C.addressof(b), a.host_threads, best_host.ctypes.data, off_host.ctypes.data))
        legs["host"].append(1e3 * (time.perf_counter() - t0))
    tl = tail.cpu().numpy()
    same = int(tl[0]) == pairs and int(tl[1]) == 0 and n_call.value == pairs
    same &= bool(np.array_equal(best_host, best_call) and np.array_equal(off_host, off_call))
    same &= bool(np.array_equal(best_host, d_best.cpu().numpy().view(np.uint32)) and np.array_equal(off_host, d_off.cpu().numpy()))
    rate = work / (statistics.median(legs["kernels"]) / 1e3)
    peak = a.cus * 4 * 16 * a.ghz * 1e9
    print(json.dumps(dict(bins=a.bins, sequences=int(b.n_seq), reads=int(b.n_reads), pairs=pairs, read_len=a.read_len, window=a.window,
                          base_comparisons=work, identical=same, kernels_ms=summary(legs["kernels"]), call_ms=summary(legs["call"]),
                          host_ms=dict(summary(legs["host"]), threads=a.host_threads),
                          comparisons_per_s=float(f"{rate:.4g}"), valu_lane_ops_per_s=float(f"{peak:.4g}"),
                          comparisons_per_lane_op=round(rate / peak, 4))))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
