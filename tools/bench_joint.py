#!/usr/bin/env python3
"""Joint genotyping on the GPU against the host path it would replace
(DESIGN.md §4.13).  A tool, not a test.

The cohort is synthesised (seeded): --samples samples over --sites sites of one
contig, about 100 positions apart.  A sample has three records per site: at
the site a call record (a carrier, --carriers of the samples at random: het or
hom-alt PLs; one site in twenty has a second ALT) or a reference block, and two
more reference blocks up to the next site.

--rounds rounds of these legs, alternated on the same box, after --warmup
rounds that are dropped:
  kernels  fcsjg_genotype_dev between two device events, inputs and outputs
           resident (--kernel-reps launches);
  call     fcsjg_genotype from and to host arrays;
  host     joint_genotype_host (fcsg_jg_genotype) on --host-threads threads.
Prints one JSON line with the median, min and max of each leg in milliseconds
and the cohort's shape, and checks that the legs give the same outputs, array
for array (the record text is joint_emit's function of them on both paths).

  tools/bench_joint.py --samples 64 --sites 100000 --rounds 3
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


def synth(n, sites, seed, carriers):
    """(cohort arrays, pos, n_alt)."""
    rng = np.random.default_rng(seed)
    pos = (100 * np.arange(sites) + rng.integers(0, 40, sites)).astype(np.int64)
    n_alt = np.where(rng.random(sites) < 0.05, 2, 1).astype(np.uint8)
    nxt = np.r_[pos[1:], pos[-1] + 100]
    beg, end, kind, alt, dp, pl = [], [], [], [], [], []
    for _ in range(n):
        carrier = rng.random(sites) < carriers
        hom = rng.random(sites) < 0.3
        a = np.where(carrier, np.where(rng.random(sites) < 0.2, n_alt, 1), 0)
        b = np.stack([pos, pos + 1 + (nxt - pos - 1) // 3, pos + 1 + 2 * (nxt - pos - 1) // 3], 1)
        e = np.stack([np.where(carrier, pos + 1, b[:, 1]), b[:, 2], nxt], 1)
        k = np.stack([carrier.astype(np.uint8), np.zeros(sites, np.uint8), np.zeros(sites, np.uint8)], 1)
        gq = rng.integers(20, 100, (sites, 3))
        p = np.zeros((sites, 3, 6), np.int32)
        p[:, :, 1], p[:, :, 2] = gq, 10 * gq
        x, y = rng.integers(30, 400, sites), rng.integers(30, 400, sites)
        het = np.stack([x, 0 * x, y, x + 30, y + 20, x + y], 1)
        homv = np.stack([x + y, y // 4 + 3, 0 * x, x + y + 20, y // 4 + 30, x + y + 60], 1)
        p[carrier, 0] = np.where(hom[carrier, None], homv[carrier], het[carrier])
        beg.append(b.ravel()), end.append(e.ravel()), kind.append(k.ravel())
        alt.append(np.stack([a, 0 * a, 0 * a], 1).ravel()), dp.append(rng.integers(8, 60, 3 * sites)), pl.append(p.reshape(-1, 6))
    rec_off = 3 * sites * np.arange(n + 1)
    return ((rec_off.astype(np.int64), np.concatenate(beg).astype(np.int32), np.concatenate(end).astype(np.int32),
             np.concatenate(kind).astype(np.uint8), np.concatenate(alt).astype(np.uint8), np.concatenate(dp).astype(np.int32),
             np.concatenate(pl).astype(np.int32)), pos.astype(np.int32), n_alt)


def summary(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--sites", type=int, default=100000)
    ap.add_argument("--carriers", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-reps", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import torch
    import fcship
    import host_lib as H
    L = H.lib
    L.fcsg_jg_genotype.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    n, ns = a.samples, a.sites
    cohort, pos, n_alt = synth(n, ns, a.seed, a.carriers)
    tabs = fcship.jg_tables(1e-3, n)
    minq = 10 << 20
    max_pl = ns * n * 6                       # one or two kept ALTs per site
    dev = torch.device("cuda", a.device)
    stream = torch.cuda.Stream(device=dev)
    c, arrays = fcship.jg_cohort(*cohort)
    with torch.cuda.stream(stream):
        t = [torch.from_numpy(x).to(dev) for x in arrays]
        dc = fcship.JgCohort(n, 0, len(arrays[1]), *(x.data_ptr() for x in t))
        dpos, dalt = torch.from_numpy(pos).to(dev), torch.from_numpy(n_alt).to(dev)
        dtab = [torch.from_numpy(x).to(dev) for x in tabs]
        dst = fcship.JgSites(ns, dpos.data_ptr(), dalt.data_ptr())
        dm = fcship.JgModel(*(x.data_ptr() for x in dtab), minq)
        host_out = fcship.jg_out_arrays(ns, n, max_pl)
        douts = {k: torch.from_numpy(v).to(dev) for k, v in host_out.items()}
        do = fcship.JgOut(*(douts[name].data_ptr() for name, *_ in fcship.JG_OUT_FIELDS), douts["pl"].data_ptr(), max_pl,
                          douts["n_pl"].data_ptr())
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        need = fcship.lib.fcsjg_workspace_bytes(ns, n)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = fcship.JgSites(ns, pos.ctypes.data, n_alt.ctypes.data)
    m = fcship.JgModel(*(x.ctypes.data for x in tabs), minq)
    out_call, out_host = fcship.jg_out_arrays(ns, n, max_pl), fcship.jg_out_arrays(ns, n, max_pl)
    o_call, o_host = fcship.jg_out(out_call), fcship.jg_out(out_host)
    legs = {"kernels": [], "call": [], "host": []}
    for rnd in range(a.warmup + a.rounds):
        if rnd == a.warmup:
            legs = {"kernels": [], "call": [], "host": []}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            for _ in range(a.kernel_reps):
                fcship.check(fcship.lib.fcsjg_genotype_dev(a.device, C.addressof(dc), C.addressof(dst), C.addressof(dm), C.addressof(do),
                                                           ws.data_ptr(), need, status.data_ptr(), C.c_void_p(stream.cuda_stream)))
            e1.record(stream)
        stream.synchronize()
        legs["kernels"].append(e0.elapsed_time(e1) / a.kernel_reps)
        t0 = time.perf_counter()
        fcship.check(fcship.lib.fcsjg_genotype(a.device, C.addressof(c), C.addressof(st), C.addressof(m), C.addressof(o_call)))
        legs["call"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        H.check(L.fcsg_jg_genotype(C.addressof(c), C.addressof(st), C.addressof(m), a.host_threads, C.addressof(o_host)))
        legs["host"].append(1e3 * (time.perf_counter() - t0))
    assert int(status.cpu()[0]) == 0
    n_pl = int(out_host["n_pl"][0])
    same = True
    for name in out_host:
        cut = slice(0, n_pl) if name == "pl" else slice(None)
        same &= bool(np.array_equal(out_host[name][cut], out_call[name][cut]))
        same &= bool(np.array_equal(out_host[name][cut], douts[name].cpu().numpy()[cut]))
    print(json.dumps(dict(samples=n, sites=ns, records=int(len(arrays[1])), carriers=a.carriers,
                          written=int((out_host["pl_off"] >= 0).sum()), pls=n_pl, identical=same,
                          kernels_ms=summary(legs["kernels"]), call_ms=summary(legs["call"]),
                          host_ms=dict(summary(legs["host"]), threads=a.host_threads))))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
