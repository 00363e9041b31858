"""The world of the sorted-BAM stream tests (tests/test_bam_stream_cpu.py and
the `*_command_streams_a_part_directory_*` GPU tests): two contigs of 6,000
loci, 1,200 mapped records of 1 to 200 bases with mixed CIGARs (indels, skips,
soft and hard clips) drawn from two haplotypes with planted SNPs, and an
unmapped tail, in two read groups of one sample; written as one BAM or as a
directory of part BAMs.

A record is a dict of ug_cases.rec with a "name" (r<index in the world>) and an
"rg" (the RG:Z tag it carries).
"""
import functools
import os

import bqsr_cases as B
import host_lib as H
import ug_cases as U
from test_markdup_cpu import add_rg_tags

NAMES = ["ctgA", "ctgB"]
HEADER = "@RG\tID:a\tSM:NA12878\tPU:unitA\tLB:lib1\n@RG\tID:b\tSM:NA12878\tLB:lib1\n"
TAIL = 12            # unmapped records without a contig, after the mapped ones
WINDOW_BP = 1024
H.lib.fcsg_text_to_bam.argtypes = [H.C.c_char_p] * 4


@functools.lru_cache(maxsize=None)
def world():
    """(refs, records): the records sorted by contig and position, the unmapped tail last."""
    refs = B.random_world(seed=19, length=6000, n_contigs=2)[0]
    records = U.random_batch(refs, seed=23, n=1200)
    for k in range(TAIL):
        seq = "".join(U.LETTERS[(k + j * j) % 4] for j in range(100))
        records.append(dict(U.rec(0x4, -1, -1, "*", seq, None), n_bases=100, qual=[20 + (k + j) % 20 for j in range(100)]))
    for k, r in enumerate(records):
        r["name"], r["rg"] = f"r{k}", "ab"[k % 2]
    return refs, records


def key(r):
    """The sort key of a record: unmapped records without a contig come last."""
    return (r["ref"] if r["ref"] >= 0 else 1 << 31, r["pos"])


def place(r):
    """contig:position as the commands print it ("*" without a contig)."""
    return f"{NAMES[r['ref']] if r['ref'] >= 0 else '*'}:{r['pos'] + 1}"


def end(r):
    return r["pos"] + U.ref_len(r["cigar"])


def file_boundary(records):
    """k: the parts records[:k] and records[k:] meet between two records of one contig at different positions, the
    first of which reaches over a window edge that the second starts before: the windows on both sides of that edge
    take records from both files."""
    for k in range(len(records) // 4, len(records)):
        a, b = records[k - 1], records[k]
        edge = (a["pos"] // WINDOW_BP + 1) * WINDOW_BP
        if 0 <= a["ref"] == b["ref"] and a["pos"] < b["pos"] < edge < end(a) and not (a["flag"] | b["flag"]) & U.FILTER:
            return k
    raise AssertionError("no such boundary")


def same_position_boundary(records):
    """k: records[k - 1] and records[k] lie at one position."""
    for k in range(len(records) // 3, len(records)):
        if 0 <= records[k]["ref"] == records[k - 1]["ref"] and records[k]["pos"] == records[k - 1]["pos"]:
            return k
    raise AssertionError("no two records at one position")


def write_fasta(path, refs, names=NAMES):
    with open(path, "w") as f:
        for n, s in zip(names, refs):
            f.write(f">{n}\n" + "".join(s[k:k + 60] + "\n" for k in range(0, len(s), 60)))
    return path


def write_bam(path, records, header=HEADER):
    """The records in the order given, each with its RG:Z tag, under the header's @RG lines."""
    path = str(path)
    lines = [header]
    for r in records:
        qual = "*" if r["qual"] is None else "".join(chr(q + 33) for q in r["qual"])
        lines.append(f"{r['name']}\t{r['flag']}\t{r['ref']}\t{r['pos']}\t{r['mapq']}\t{r['cigar']}\t{r['seq'].upper()}\t{qual}\n")
    with open(path + ".txt", "w") as f:
        f.write("".join(lines))
    H.check(H.lib.fcsg_text_to_bam((path + ".txt").encode(), (path + ".plain").encode(), ",".join(NAMES).encode(), b"6000,6000"))
    add_rg_tags(path + ".plain", path, [r["rg"] for r in records])
    os.remove(path + ".txt"), os.remove(path + ".plain")
    return path


def write_parts(d, *parts, **kw):
    """A directory of part-00000k.bam, one per list of records."""
    os.makedirs(d, exist_ok=True)
    for k, records in enumerate(parts):
        write_bam(os.path.join(str(d), f"part-{k:06d}.bam"), records, **kw)
    return d


def part_directory(d):
    """(ref.fa, parts/, n) under d: the world's n records as two part BAMs that meet at file_boundary."""
    refs, records = world()
    k = file_boundary(records)
    return write_fasta(d / "ref.fa", refs), write_parts(d / "parts", records[:k], records[k:]), len(records)
