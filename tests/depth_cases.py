"""Depth of coverage (DESIGN §2 [EXT] "Depth of coverage", §4.11): the Python
restatement of the rules (counted records and bases, the window clip, the
501-bin histogram, the granular quantiles, the text of the seven files),
builders of batches, and the hand cases with their expected depths written out.

A record is a dict: flag, ref (contig index), pos (0-based), mapq, cigar (text),
qual (list of phred values, or None: absent), n_bases.  Base letters are not
part of a record: they do not matter.  A reference is a list of contig strings.
A window is (ref, start, len).
"""
import random
import re

import numpy as np

BINS, ABOVE, PIECE_MAX = 501, 15, 65536
UNMAPPED, REVERSE, SECONDARY, QCFAIL, DUPLICATE, SUPPLEMENTARY = 0x4, 0x10, 0x100, 0x200, 0x400, 0x800
FILTER = UNMAPPED | SECONDARY | QCFAIL | DUPLICATE
OPS = "MIDNSHP=X"


class Refused(ValueError):
    """What the host path throws and the ABI answers with FCS_ERR_INVALID."""


def parse_cigar(text):
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", text)]


def read_len(cigar):
    return sum(n for n, op in parse_cigar(cigar) if op in "MIS=X")


def ref_len(cigar):
    return sum(n for n, op in parse_cigar(cigar) if op in "MDN=X")


def rec(flag, ref, pos, cigar, qual=30, mapq=60):
    n = read_len(cigar)
    if isinstance(qual, int):
        qual = [qual] * n
    return dict(flag=flag, ref=ref, pos=pos, mapq=mapq, cigar=cigar, qual=None if qual is None else list(qual), n_bases=n)


def params(min_mapq=-1, max_mapq=2 ** 31 - 1, min_baseq=-1, max_baseq=127, include_deletions=False):
    return dict(min_mapq=min_mapq, max_mapq=max_mapq, min_baseq=min_baseq, max_baseq=max_baseq,
                include_deletions=include_deletions)


# ------------------------------------------------------------------ the rules
def counted(r, prm):
    return (r["ref"] >= 0 and bool(parse_cigar(r["cigar"])) and not r["flag"] & FILTER
            and prm["min_mapq"] <= r["mapq"] <= prm["max_mapq"])


def record_positions(r, prm):
    """The reference positions the record adds 1 to (before any clip), and whether it needs its base count checked."""
    out, p, i = [], r["pos"], 0
    for n, op in parse_cigar(r["cigar"]):
        if op in "M=X":
            for j in range(n):
                q = 0 if r["qual"] is None else r["qual"][i + j]
                if prm["min_baseq"] <= q <= prm["max_baseq"]:
                    out.append((p + j, True))
            p += n
            i += n
        elif op in "IS":
            i += n
        elif op == "D":
            if prm["include_deletions"]:
                out += [(p + j, False) for j in range(n)]
            p += n
        elif op == "N":
            p += n
    return out


def depth(records, window, contig_len, prm=None):
    """(depths of the window's loci, a counted base lay beyond the contig).  Refused on a CIGAR that does not cover its
    record's bases."""
    prm = prm or params()
    ref, start, length = window
    d = np.zeros(length, np.uint32)
    beyond = False
    for r in records:
        if r["ref"] != ref or not counted(r, prm):
            continue
        if read_len(r["cigar"]) != r["n_bases"] or (r["qual"] is not None and len(r["qual"]) != r["n_bases"]):
            raise Refused("the CIGAR does not cover the bases")
        p, aligned_beyond = r["pos"], False
        for n, op in parse_cigar(r["cigar"]):   # an aligned base beyond the contig, whatever its quality
            if op in "M=X" and n and (p < 0 or p + n > contig_len):
                aligned_beyond = True
            if op in "MDN=X":
                p += n
        beyond |= aligned_beyond
        for p, _ in record_positions(r, prm):
            if 0 <= p < contig_len and start <= p < start + length:
                d[p - start] += 1
    return d, beyond


def quantile(hist, k):
    """The reported granular quantile k / 4: max(bin, 1), and 1 without loci; the comparison in integers."""
    n = int(sum(int(v) for v in hist))
    if n == 0:
        return 1
    cum = 0
    for b in range(BINS):
        cum += int(hist[b])
        if 4 * cum >= k * n:
            return max(b, 1)
    raise AssertionError


def histogram(depths):
    h = np.zeros(BINS, np.uint64)
    for d in depths:
        h[min(int(d), BINS - 1)] += 1
    return h


def stats(d, part, pieces, n_long=0):
    """(hist, long_hist, [summary dict]) of pieces (start, end, long_index) over depths d and participation flags part."""
    hist = np.zeros(BINS, np.uint64)
    long_hist = np.zeros((n_long, BINS), np.uint64)
    out = []
    for s, e, li in pieces:
        vals = [int(d[i]) for i in range(s, e) if part[i]]
        h = histogram(vals)
        hist += h
        row = dict(total=sum(vals), loci=len(vals), above=sum(v >= ABOVE for v in vals), q1=0, median=0, q3=0)
        if li >= 0:
            long_hist[li] += h
        else:
            row.update(q1=quantile(h, 1), median=quantile(h, 2), q3=quantile(h, 3))
        out.append(row)
    return hist, long_hist, out


def bitmap(part):
    """One bit per locus, bit i & 63 of word i >> 6."""
    words = np.zeros((len(part) + 63) // 64 + 1, np.uint64)
    for i, p in enumerate(part):
        if p:
            words[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    return words


# ------------------------------------------------------------------ the text
def mean_text(total, n):
    return "%.2f" % (total / n) if n else "NaN"


def percent_text(above, n):
    return "%.1f" % (100.0 * above / n) if n else "NaN"


def merge_intervals(intervals):
    """(ref, start, end) half-open, sorted by contig index, overlapping and abutting ones merged."""
    out = []
    for ref, s, e in sorted(intervals):
        if out and out[-1][0] == ref and s <= out[-1][2]:
            out[-1][2] = max(out[-1][2], e)
        else:
            out.append([ref, s, e])
    return [tuple(i) for i in out]


STAT_HEADER = "Source_of_reads" + "".join(f"\tfrom_{k}_to_{k + 1})" for k in range(BINS - 1)) + "\tfrom_500_to_inf\n"
CUM_HEADER = "".join(f"\tgte_{k}" for k in range(BINS)) + "\n"


def files(sample, names, refs, intervals, depths, include_ref_n=False):
    """{suffix: text} of the seven files; depths[c] are contig c's depths, intervals are merged ones."""
    locus = [f"Locus\tTotal_Depth\tAverage_Depth_sample\tDepth_for_{sample}\n"]
    hist = np.zeros(BINS, np.uint64)
    total = 0
    rows = []
    for ref, s, e in intervals:
        seq = refs[ref]
        vals = []
        for p in range(s, e):
            if include_ref_n or seq[p] not in "Nn":
                d = int(depths[ref][p])
                vals.append(d)
                locus.append(f"{names[ref]}:{p + 1}\t{d}\t{d}.00\t{d}\n")
        h = histogram(vals)
        hist += h
        total += sum(vals)
        name = f"{names[ref]}:{s + 1}-{e}" if e - s > 1 else f"{names[ref]}:{s + 1}"
        rows.append((name, sum(vals), len(vals), sum(v >= ABOVE for v in vals), quantile(h, 1), quantile(h, 2), quantile(h, 3)))
    n = int(hist.sum())
    above = int(hist[ABOVE:].sum())
    cum = [int(hist[k:].sum()) for k in range(BINS)]
    out = {"": "".join(locus)}
    out[".sample_summary"] = (
        "sample_id\ttotal\tmean\tgranular_third_quartile\tgranular_median\tgranular_first_quartile\t%_bases_above_15\n"
        f"{sample}\t{total}\t{mean_text(total, n)}\t{quantile(hist, 3)}\t{quantile(hist, 2)}\t{quantile(hist, 1)}\t"
        f"{percent_text(above, n)}\nTotal\t{total}\t{mean_text(total, n)}\tN/A\tN/A\tN/A\n")
    out[".sample_statistics"] = STAT_HEADER + f"sample_{sample}" + "".join(f"\t{int(v)}" for v in hist) + "\n"
    out[".sample_cumulative_coverage_counts"] = CUM_HEADER + "NSamples_1" + "".join(f"\t{c}" for c in cum) + "\n"
    out[".sample_cumulative_coverage_proportions"] = CUM_HEADER + sample + "".join(
        "\t" + ("%.2f" % (c / cum[0]) if cum[0] else "NaN") for c in cum) + "\n"
    text = (f"Target\ttotal_coverage\taverage_coverage\t{sample}_total_cvg\t{sample}_mean_cvg\t{sample}_granular_Q1\t"
            f"{sample}_granular_median\t{sample}_granular_Q3\t{sample}_%_above_15\n")
    cells = [0] * BINS
    for name, t, k, a, q1, q2, q3 in rows:
        text += f"{name}\t{t}\t{mean_text(t, k)}\t{t}\t{mean_text(t, k)}\t{q1}\t{q2}\t{q3}\t{percent_text(a, k)}\n"
        cells[min(t // k, BINS - 1) if k else 0] += 1
    out[".sample_interval_summary"] = text
    out[".sample_interval_statistics"] = STAT_HEADER + "At_least_1_samples" + "".join(f"\t{c}" for c in cells) + "\n"
    return out


# ------------------------------------------------------------------ the flat batch
def flatten(records, first_offset=0):
    """(flag, ref_id, pos, mapq, cigar, cigar_off, qual, base_off, qual_absent): fcsdp_batch's arrays; the quality
    bytes start at first_offset (the bytes before them are 0xEE)."""
    cigar, cigar_off, qual, base_off = [], [0], [0xEE] * first_offset, [first_offset]
    for r in records:
        cigar += [(n << 4) | OPS.index(op) for n, op in parse_cigar(r["cigar"])]
        cigar_off.append(len(cigar))
        qual += [0xFF] * r["n_bases"] if r["qual"] is None else r["qual"]
        base_off.append(len(qual))
    return ([r["flag"] for r in records], [r["ref"] for r in records], [r["pos"] for r in records],
            [r["mapq"] for r in records], cigar, cigar_off, qual, base_off, [int(r["qual"] is None) for r in records])


# ------------------------------------------------------------------ the hand cases
LENS = [300, 40]   # the hand cases' contigs


def hand_cases():
    """[dict(name, records, prm, window, want: [(first position, one past the last, depth)], beyond)]; every locus of
    the window outside want has depth 0."""
    whole0, whole1, mid = (0, 0, 300), (1, 0, 40), (0, 100, 50)

    def case(name, records, want, window=whole0, prm=None, beyond=False):
        return dict(name=name, records=records, prm=prm or params(), window=window, want=want, beyond=beyond)

    on = params(include_deletions=True)
    return [
        case("op_m", [rec(0, 0, 10, "10M")], [(10, 20, 1)]),
        case("op_eq", [rec(0, 0, 10, "10=")], [(10, 20, 1)]),
        case("op_x", [rec(0, 0, 10, "10X")], [(10, 20, 1)]),
        case("op_i", [rec(0, 0, 10, "5I")], []),
        case("op_s", [rec(0, 0, 10, "5S")], []),
        case("op_h", [rec(0, 0, 10, "5H")], []),
        case("op_p", [rec(0, 0, 10, "5P")], []),
        case("op_n", [rec(0, 0, 10, "5N")], []),
        case("op_d", [rec(0, 0, 10, "5D")], []),
        case("op_d_with_deletions", [rec(0, 0, 10, "5D")], [(10, 15, 1)], prm=on),
        case("clips", [rec(0, 0, 10, "3H2S10M2S3H")], [(10, 20, 1)]),
        case("deletion_off", [rec(0, 0, 10, "10M2D10M")], [(10, 20, 1), (22, 32, 1)]),
        case("deletion_on", [rec(0, 0, 10, "10M2D10M")], [(10, 32, 1)], prm=on),
        case("skip", [rec(0, 0, 10, "5M100N5M")], [(10, 15, 1), (115, 120, 1)]),
        case("skip_with_deletions", [rec(0, 0, 10, "5M100N5M")], [(10, 15, 1), (115, 120, 1)], prm=on),
        case("insertion", [rec(0, 0, 10, "5M3I5M")], [(10, 20, 1)]),
        case("reverse", [rec(REVERSE, 0, 10, "10M")], [(10, 20, 1)]),
        case("flags", [rec(UNMAPPED, 0, 10, "10M"), rec(SECONDARY, 0, 30, "10M"), rec(QCFAIL, 0, 50, "10M"),
                       rec(DUPLICATE, 0, 70, "10M"), rec(SUPPLEMENTARY, 0, 90, "10M"), rec(0x1 | 0x2 | 0x20 | 0x40, 0, 95, "10M")],
             [(90, 95, 1), (95, 100, 2), (100, 105, 1)]),
        case("no_contig_and_no_cigar", [rec(0, -1, 10, "10M"), rec(0, 0, 10, "")], []),
        case("mapq_bounds", [rec(0, 0, 0, "10M", mapq=19), rec(0, 0, 20, "10M", mapq=20), rec(0, 0, 40, "10M", mapq=40),
                             rec(0, 0, 60, "10M", mapq=41)], [(20, 30, 1), (40, 50, 1)], prm=params(min_mapq=20, max_mapq=40)),
        case("mapq_255_counts_by_default", [rec(0, 0, 10, "10M", mapq=255), rec(0, 0, 10, "10M", mapq=0)], [(10, 20, 2)]),
        case("baseq_bounds", [rec(0, 0, 10, "6M", qual=[9, 10, 20, 30, 31, 10])], [(11, 14, 1), (15, 16, 1)],
             prm=params(min_baseq=10, max_baseq=30)),
        case("absent_qualities_min_0", [rec(0, 0, 10, "10M", qual=None)], [(10, 20, 1)], prm=params(min_baseq=0)),
        case("absent_qualities_min_1", [rec(0, 0, 10, "10M", qual=None)], [], prm=params(min_baseq=1)),
        # the batch carries no base letters: a read base N is a base like any other
        case("read_base_n", [rec(0, 0, 10, "4M", qual=[2, 2, 2, 2])], [(10, 14, 1)]),
        case("deletion_has_no_quality_test", [rec(0, 0, 10, "2M3D2M", qual=[5, 5, 5, 5])], [(12, 15, 1)],
             prm=params(min_baseq=10, include_deletions=True)),
        case("starts_before_window", [rec(0, 0, 90, "20M")], [(100, 110, 1)], window=mid),
        case("ends_after_window", [rec(0, 0, 140, "20M")], [(140, 150, 1)], window=mid),
        case("covers_window", [rec(0, 0, 80, "100M")], [(100, 150, 1)], window=mid),
        case("outside_window", [rec(0, 0, 80, "20M"), rec(0, 0, 150, "20M"), rec(0, 1, 10, "20M")], [], window=mid),
        case("deletion_across_window_start", [rec(0, 0, 90, "5M10D5M")], [(100, 105, 1), (105, 110, 1)], window=mid, prm=on),
        case("ends_at_contig_end", [rec(0, 1, 30, "10M")], [(30, 40, 1)], window=whole1),
        case("ends_one_past_contig_end", [rec(0, 1, 31, "10M")], [(31, 40, 1)], window=whole1, beyond=True),
        case("two_reads_overlap", [rec(0, 0, 10, "10M"), rec(REVERSE, 0, 15, "10M")], [(10, 15, 1), (15, 20, 2), (20, 25, 1)]),
    ]


def want_depths(case):
    ref, start, length = case["window"]
    d = np.zeros(length, np.uint32)
    for a, b, v in case["want"]:
        d[a - start:b - start] = v
    return d


def stats_hand():
    """(depths, participation, pieces, want hist as {bin: count}, want summary) written out by hand."""
    d = [0, 1, 1, 2, 3, 3, 3, 20, 600, 7]
    part = [1, 1, 1, 1, 1, 1, 1, 1, 0, 0]
    # n = 8: cumulative 1, 3, 4, 7, ..., 8 at bins 0, 1, 2, 3, 20: Q1 needs 4 cum >= 8 (bin 1), the median 16 (bin 2), Q3 24 (bin 3)
    return d, part, [(0, 10, -1)], {0: 1, 1: 2, 2: 1, 3: 3, 20: 1}, dict(total=33, loci=8, above=1, q1=1, median=2, q3=3)


# ------------------------------------------------------------------ generators
def random_world(seed=7):
    """Three contigs, about 20 kbp, with runs of N (one of them lower-case)."""
    rng = random.Random(seed)
    refs = []
    for length in (9000, 7000, 4096):
        s = [rng.choice("ACGT") for _ in range(length)]
        for _ in range(3):
            a = rng.randrange(0, length - 200)
            k = rng.randrange(1, 150)
            s[a:a + k] = ("n" if rng.random() < 0.3 else "N") * k
        refs.append("".join(s))
    return refs


def random_cigar(rng, n):
    """A CIGAR of n read bases with mixed ops."""
    ops = []
    if rng.random() < 0.1:
        ops.append((rng.randrange(1, 5), "H"))
    left = n
    if rng.random() < 0.2 and left > 1:
        k = rng.randrange(1, min(left, 20))
        ops.append((k, "S"))
        left -= k
    tail = 0
    if rng.random() < 0.2 and left > 1:
        tail = rng.randrange(1, min(left, 20))
        left -= tail
    first = True
    while left > 0:
        if not first:
            gap = rng.random()
            if gap < 0.3:
                ops.append((rng.randrange(1, 6), "D"))
            elif gap < 0.4:
                ops.append((rng.randrange(1, 300), "N"))
            elif gap < 0.5:
                ops.append((1, "P"))
            elif gap < 0.8 and left > 1:
                k = rng.randrange(1, min(left, 8))
                ops.append((k, "I"))
                left -= k
        k = left if rng.random() < 0.5 else rng.randrange(1, left + 1)
        op = rng.choice("MMMM=X")
        if ops and ops[-1][1] == op:
            op = "X" if op != "X" else "M"
        ops.append((k, op))
        left -= k
        first = False
    if tail:
        ops.append((tail, "S"))
    if rng.random() < 0.1:
        ops.append((rng.randrange(1, 5), "H"))
    return "".join(f"{k}{op}" for k, op in ops)


def random_batch(refs, seed=11, n=2000, sort=False):
    """About n records of 1-200 bases with mixed CIGARs, flags, MAPQs and qualities, inside their contigs."""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        L = rng.randrange(1, 201)
        cigar = random_cigar(rng, L)
        ref = rng.randrange(len(refs))
        span = ref_len(cigar)
        if span > len(refs[ref]):
            continue
        pos = rng.randrange(0, len(refs[ref]) - span + 1)
        flag = rng.choice([0, 0, 0, REVERSE, 0x1 | 0x40, 0x1 | 0x80 | REVERSE, SUPPLEMENTARY, DUPLICATE, SECONDARY, QCFAIL, UNMAPPED])
        qual = None if rng.random() < 0.03 else [rng.randrange(0, 42) for _ in range(L)]
        out.append(rec(flag, ref, pos, cigar, qual, mapq=rng.choice([0, 1, 20, 29, 30, 60, 255])))
    if sort:
        out.sort(key=lambda r: (r["ref"], r["pos"]))
    return out


def sweep_batch(refs, seed=3):
    """Records of 1 .. 200 bases one after the other, so that their quality bytes start at every 4-byte residue."""
    rng = random.Random(seed)
    out = []
    for L in range(1, 201):
        pos = rng.randrange(0, len(refs[0]) - L)
        out.append(rec(0, 0, pos, f"{L}M", [rng.randrange(0, 42) for _ in range(L)]))
    return out


def copies_batch():
    """600 copies of one 30-base read: 499 at 100, one at 110, one at 120 and 99 at 1000, so that the depths 499, 500
    and 501 are all reached (bins 499 and 500)."""
    return ([rec(0, 0, 100, "30M")] * 499 + [rec(0, 0, 110, "30M"), rec(0, 0, 120, "30M")] + [rec(0, 0, 1000, "30M")] * 99)
