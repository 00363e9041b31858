"""The pileup in front of htc's and mutect2's PairHMM: the Python
restatement of the rules over flat records (the per-base part, the per-op
events, the site predicate and the SNV list), the hand cases with their
expected arrays written out, and a random world.

Records, references and windows are ug_cases': a record is a dict (ref, pos,
cigar text, seq, qual list, ...), a window is (ref, start, len).  The doubles are
Python floats added in record order, which reproduces the host's sums bit for bit.
"""
import math

import numpy as np

import ug_cases as U
from depth_cases import parse_cigar

MAXQ = 93
MIN_BQ, FRAC = 10, 0.15
STATUS_FIELD, STATUS_REF, STATUS_ORDER, STATUS_SITES, STATUS_SNVS, STATUS_LETTER = 1, 2, 4, 8, 16, 32


# ------------------------------------------------------------------ the rules
def table_formulas():
    """T[94][3] from the documented formulas, in Python's libm."""
    out = []
    for q in range(MAXQ + 1):
        e = min(0.75, 10.0 ** (-q / 10.0))
        out.append([math.log10(1.0 - e), math.log10(0.5 * (1.0 - e) + 0.5 * e / 3.0), math.log10(e / 3.0)])
    return out


def nonref(b, r):
    return b != r and r != "N" and b != "N"


def pile(batches, window, refseq, tab, min_bq=MIN_BQ, frac=FRAC, want_gl=True, events_in=None):
    """fcspu_pile's results for one or two lists of records: dict(depth, events, gl, sites, snvs); snvs are
    (offset, alt letter, count).  refseq is the whole contig; tab a [94][3] of floats."""
    ref, start, length = window
    depth, events = np.zeros(length, np.int32), np.zeros(length, np.int32)
    gl = [[0.0, 0.0, 0.0] for _ in range(length)] if want_gl else None
    counts = {}
    sites = []
    for k, records in enumerate(batches):
        for r in records:
            if r["ref"] != ref:
                continue
            p, i = r["pos"], 0
            for n, op in parse_cigar(r["cigar"]):
                if op in "M=X":
                    for j in range(max(p, start) - p, min(p + n, start + length) - p):
                        bq = r["qual"][i + j]
                        if bq < min_bq:
                            continue
                        off = p + j - start
                        depth[off] += 1
                        b, rl = r["seq"][i + j], refseq[p + j]
                        alt = nonref(b, rl)
                        if alt:
                            events[off] += 1
                            counts[(off, b)] = counts.get((off, b), 0) + 1
                        if k == 0 and want_gl:
                            t, g = tab[min(bq, MAXQ)], gl[off]
                            g[0] += t[2 if alt else 0]
                            g[1] += t[1]
                            g[2] += t[0 if alt else 2]
                    p, i = p + n, i + n
                elif op in "IS":
                    i += n
                elif op == "D":
                    for q in range(max(p, start), min(p + n, start + length)):
                        depth[q - start] += 1
                    p += n
                elif op == "N":
                    p += n
        if k == 0:
            for off in range(length):
                ev = int(events[off]) + (0 if events_in is None else int(events_in[off]))
                if ev >= 2 and ev >= frac * max(1, int(depth[off])):
                    sites.append(off)
    snvs = [(off, b, c) for (off, b), c in sorted(counts.items(), key=lambda kv: (kv[0][0], ord(kv[0][1]))) if c >= 2]
    return dict(depth=depth, events=events, gl=np.array(gl, np.float64).reshape(length, 3) if want_gl else None,
                sites=sites, snvs=snvs)


def op_events(records, window, refseq):
    """The per-op part's events: 1 at the anchor of every insertion and deletion that is not the record's first
    reference-consuming step, with the anchor inside the window and, for a deletion, its end inside the contig."""
    ref, start, length = window
    out = np.zeros(length, np.int32)
    for r in records:
        if r["ref"] != ref:
            continue
        p = r["pos"]
        for n, op in parse_cigar(r["cigar"]):
            if op in "ID" and p > r["pos"] and start <= p - 1 < start + length and (op == "I" or p + n <= len(refseq)):
                out[p - 1 - start] += 1
            if op in "M=XDN":
                p += n
    return out


def cut(res, start, length):
    """A whole contig's results cut to the window [start, start + length) of it."""
    return dict(depth=res["depth"][start:start + length], events=res["events"][start:start + length],
                gl=None if res["gl"] is None else res["gl"][start:start + length],
                sites=[s - start for s in res["sites"] if start <= s < start + length],
                snvs=[(o - start, b, c) for o, b, c in res["snvs"] if start <= o < start + length])


def same(got, want, gl=True):
    """The entry's dict (numpy arrays, PU_SNV rows) equals the restatement's: every array, the doubles by their bits."""
    assert np.array_equal(np.asarray(got["depth"]), want["depth"]), "depth"
    assert np.array_equal(np.asarray(got["events"]), want["events"]), "events"
    if gl and want["gl"] is not None:
        a, b = np.ascontiguousarray(got["gl"], np.float64), np.ascontiguousarray(want["gl"], np.float64)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), "gl bits"
    assert [int(s) for s in got["sites"]] == list(want["sites"]), "sites"
    assert [(int(v["offset"]), chr(int(v["alt"])), int(v["count"])) for v in got["snvs"]] == list(want["snvs"]), "snvs"
    return True


# ------------------------------------------------------------------ records
def read(refs, pos, cigar, subs=None, qual=30, contig=0):
    """ug_cases.rec of the read the CIGAR copies from the contig, with subs {reference position: letter} of aligned bases."""
    seq = list(U.read_of(refs[contig], pos, cigar))
    p, i, at = pos, 0, {}
    for n, op in parse_cigar(cigar):
        if op in "M=X":
            for j in range(n):
                at[p + j] = i + j
            p, i = p + n, i + n
        elif op in "IS":
            i += n
        elif op in "DN":
            p += n
    for where, ch in (subs or {}).items():
        seq[at[where]] = ch
    return U.rec(0, contig, pos, cigar, "".join(seq), qual, 60)


def sparse(length, cells):
    out = np.zeros(length, np.int32)
    for off, v in cells.items():
        out[off] = v
    return out


def hand_cases():
    """[dict(name, batches, window, frac, ops, depth, events, sites, snvs)]: ops, depth and events are the expected
    arrays of the window as {offset: value} (every other locus 0): ops the per-op events of batch 0, depth and events
    fcspu_pile's; sites the expected offsets and snvs the expected (offset, alt, count)."""
    refs = U.hand_refs()
    whole0, whole1 = (0, 0, 1200), (1, 0, 40)

    def rd(pos, cigar, subs=None, qual=30, contig=0):
        return read(refs, pos, cigar, subs, qual, contig)

    def span(a, b, v=1):
        return {p: v for p in range(a, b)}

    def case(name, batches, depth, events=None, sites=(), snvs=(), ops=None, window=whole0, frac=FRAC):
        if batches and isinstance(batches[0], dict):
            batches = [batches]
        return dict(name=name, batches=batches, window=window, frac=frac, ops=ops or {}, depth=depth, events=events or {},
                    sites=list(sites), snvs=list(snvs))

    # locus p of contig 0 holds ACGT[p % 4]; N at 600 .. 609, lower case at 700 .. 719
    return [
        case("every_cigar_op", [rd(10, "2H3S4M2I1P4M3D2M20N4=1X3S", {47: "A"})],
             depth={**span(10, 23), **span(43, 48)}, events={47: 1}, ops={13: 1, 17: 1}),
        case("insertion_as_the_first_op_is_no_event", [rd(50, "2I6M")], depth=span(50, 56)),
        case("insertion_anchors_at_the_window_edges", [rd(96, "4M2I4M"), rd(146, "4M2I4M")],
             depth={**span(0, 4), **span(46, 50)}, ops={49: 1}, window=(0, 100, 50)),
        case("deletion_to_the_contig_end_and_one_past", [rd(30, "6M4D", contig=1), rd(31, "6M4D", contig=1)],
             depth={30: 1, **span(31, 40, 2)}, ops={35: 1}, window=whole1),
        case("deleted_span_under_low_quality_neighbours", [rd(200, "4M3D4M", qual=5)], depth=span(204, 207), ops={203: 1}),
        case("min_bq_minus_one_and_min_bq", [rd(300, "4M", {301: "T", 302: "T"}, qual=[30, 9, 10, 30])],
             depth={300: 1, 302: 1, 303: 1}, events={302: 1}),
        case("reference_n", [rd(596, "20M", {598: "A", 604: "C", 611: "A"})] * 2,
             depth=span(596, 616, 2), events={598: 2, 611: 2}, sites=[598, 611], snvs=[(598, "A", 2), (611, "A", 2)]),
        case("read_n", [rd(620, "4M", {621: "N"})] * 2, depth=span(620, 624, 2)),
        case("lower_case_reference_differs_from_every_read_letter", [rd(698, "4M")] * 2,
             depth=span(698, 702, 2), events={700: 2, 701: 2}, sites=[700, 701], snvs=[(700, "A", 2), (701, "C", 2)]),
        case("quality_94_and_above_takes_row_93", [rd(800, "4M", qual=[94, 120, 93, 30])], depth=span(800, 804)),
        case("one_alt_read_is_no_snv", [rd(900, "4M"), rd(900, "4M", {901: "A"}), rd(900, "4M")],
             depth=span(900, 904, 3), events={901: 1}),
        case("two_alt_reads", [rd(904, "4M", {905: "A"}), rd(904, "4M"), rd(904, "4M", {905: "A"})],
             depth=span(904, 908, 3), events={905: 2}, sites=[905], snvs=[(905, "A", 2)]),
        case("two_alt_letters_at_one_locus", [rd(910, "4M", {911: "G"}), rd(910, "4M", {911: "A"}), rd(910, "4M"),
                                              rd(910, "4M", {911: "A"}), rd(910, "4M", {911: "G"})],
             depth=span(910, 914, 5), events={911: 4}, sites=[911], snvs=[(911, "A", 2), (911, "G", 2)]),
        # frac 1 / 8 is exact in binary: 2 events of depth 16 meet it exactly, 2 of depth 17 fall just below
        case("events_equal_frac_times_depth_and_just_below",
             [rd(1000, "4M", {1001: "A"})] * 2 + [rd(1000, "4M")] * 14 + [rd(1010, "4M", {1011: "A"})] * 2 + [rd(1010, "4M")] * 15,
             depth={**span(1000, 1004, 16), **span(1010, 1014, 17)}, events={1001: 2, 1011: 2}, sites=[1001],
             snvs=[(1001, "A", 2), (1011, "A", 2)], frac=0.125),
        # batch 0 the tumor, batch 1 the normal: an SNV of 1 + 1 reads is listed; a locus active in the normal alone is no site
        case("tumor_plus_normal",
             [[rd(1100, "8M", {1101: "A", 1103: "A"}), rd(1100, "8M", {1103: "A"}), rd(1100, "8M")],
              [rd(1100, "8M", {1101: "A", 1105: "T"}), rd(1100, "8M", {1105: "T"}), rd(1100, "8M")]],
             depth=span(1100, 1108, 6), events={1101: 2, 1103: 2, 1105: 2}, sites=[1103],
             snvs=[(1101, "A", 2), (1103, "A", 2), (1105, "T", 2)]),
    ]


def want_of(case):
    """The case's expected arrays as the comparable part of pile's dict (no gl)."""
    length = case["window"][2]
    return dict(depth=sparse(length, case["depth"]), events=sparse(length, case["events"]), gl=None, sites=case["sites"],
                snvs=case["snvs"])


# ------------------------------------------------------------------ generators
def random_world(seed=7):
    """Three contigs of about 6,000 loci with runs of N and lower-case stretches."""
    return [s[:n] for s, n in zip(U.random_world(seed), (6000, 6100, 4096))]


def random_batch(refs, seed=11, n=1500):
    """About n records of ug_cases.random_batch's kind (indels, clips, skips, qualities 2 to 41, read N) as the callers'
    decoder hands them on: upper-case letters, qualities present, every record counted."""
    out = U.random_batch(refs, seed, n)
    for k, r in enumerate(out):
        r["flag"], r["seq"] = 0, r["seq"].upper()
        if r["qual"] is None:
            r["qual"] = [2 + (7 * k + i) % 40 for i in range(r["n_bases"])]
    return out


def reversed_ties(records):
    """The records with every run of equal (ref, pos) reversed: still sorted."""
    out, i = [], 0
    while i < len(records):
        j = i
        while j < len(records) and (records[j]["ref"], records[j]["pos"]) == (records[i]["ref"], records[i]["pos"]):
            j += 1
        out += records[i:j][::-1]
        i = j
    return out
