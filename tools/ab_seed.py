#!/usr/bin/env python3
"""`fcs-genome align` with seeding on the host, on the GPU through two calls
per chunk, and through the fused call.  A tool, not a test.

The bench's align shape (2x151 pairs at 30x over --mbp of random genome, a
saved index at --sa-intv), the three settings alternated --rounds times on one
box:
  host    bwa.gpu_seed=false
  two     bwa.gpu_seed=true bwa.gpu_seed_fused=false
  fused   bwa.gpu_seed=true bwa.gpu_seed_fused=true
Per run: the wall, the seeding thread-seconds and their collect / locate /
chain split from the log.  The BAMs of a round must be byte-identical.  The
full log goes to --log, one JSON document (runs and medians) to --json.

  tools/ab_seed.py --work /tmp/ab_seed --log ab.log --json ab.json
"""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "falcon-genome_amd", "bin", "fcs-genome")
SETTINGS = {"host": {"FCS_BWA_GPU_SEED": "false"},
            "two": {"FCS_BWA_GPU_SEED": "true", "FCS_BWA_GPU_SEED_FUSED": "false"},
            "fused": {"FCS_BWA_GPU_SEED": "true", "FCS_BWA_GPU_SEED_FUSED": "true"}}


def run(log, limit, args, env=None):
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit), BIN, *map(str, args)], capture_output=True, text=True,
                       env={**os.environ, **(env or {})})
    wall = time.perf_counter() - t0
    log.write(f"$ {' '.join(map(str, args))}  {env or ''}  rc={p.returncode} wall={wall:.3f}\n{p.stderr}\n")
    log.flush()
    if p.returncode != 0:
        raise SystemExit(f"{args[0]} ended with {p.returncode}:\n{p.stderr[-3000:]}")
    return wall, p.stderr


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--work", required=True)
    ap.add_argument("--mbp", type=float, default=4.0)
    ap.add_argument("--sa-intv", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--limit", type=int, default=120, help="seconds one command may take")
    ap.add_argument("--log", required=True)
    ap.add_argument("--json", required=True)
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    d = os.path.join(a.work, "a")
    runs = {k: [] for k in SETTINGS}
    identical = True
    with open(a.log, "w") as log:
        run(log, a.limit, ["synth", "-o", d, "-c", f"chr1:{int(a.mbp * 1e6)}", "-x", "30", "--no-fastq", "--paired", "350",
                           "--seed", "20261015"])
        run(log, a.limit, ["index", "-r", os.path.join(d, "ref.fasta"), "--sa-intv", a.sa_intv])
        for _ in range(a.rounds):
            digests = set()
            for name, env in SETTINGS.items():
                out = os.path.join(a.work, f"aln_{name}.bam")
                wall, err = run(log, a.limit, ["align", "-f", "-r", os.path.join(d, "ref.fasta"), "-1",
                                               os.path.join(d, "sample_1.fastq"), "-2", os.path.join(d, "sample_2.fastq"),
                                               "-o", out], env)
                m = re.search(r"alignment thread-seconds ([\d.]+): seeding ([\d.]+)", err)
                row = {"wall_s": round(wall, 3), "thread_s": float(m.group(1)), "seeding_thread_s": float(m.group(2))}
                g = re.search(r"seeding thread-seconds: collect ([\d.e-]+), locate ([\d.e-]+), chain ([\d.e-]+)", err)
                if g:
                    row.update(collect_s=float(g.group(1)), locate_s=float(g.group(2)), chain_s=float(g.group(3)),
                               fused="fused" in re.search(r"GPU seeding .*", err).group(0))
                runs[name].append(row)
                digests.add(hashlib.sha256(open(out, "rb").read() + open(out + ".bai", "rb").read()).hexdigest())
            identical = identical and len(digests) == 1
        med = {k: {f: round(statistics.median(r[f] for r in v), 4) for f in v[0] if f != "fused"} for k, v in runs.items()}
        pairs = [f["seeding_thread_s"] < t["seeding_thread_s"] for f, t in zip(runs["fused"], runs["two"])]
        doc = {"mbp": a.mbp, "sa_intv": a.sa_intv, "rounds": a.rounds, "bam_identical": identical, "runs": runs,
               "median": med, "fused_below_two_call_in_every_pair": all(pairs)}
        log.write(json.dumps({k: doc[k] for k in ("bam_identical", "median", "fused_below_two_call_in_every_pair")}) + "\n")
    with open(a.json, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: doc[k] for k in ("bam_identical", "median", "fused_below_two_call_in_every_pair")}))
    return 0 if identical else 1


if __name__ == "__main__":
    sys.exit(main())
