"""Base quality recalibration (DESIGN §2 [EXT], §4.10): the Python restatement
of the rules (count, finalise, apply, report), builders of batches, and the 14
hand cases with their expected tables and qualities written out.

A record is a dict: flag, ref (contig index), pos (0-based), mapq, rg (-1:
none), cigar (text), seq (ASCII), qual (list of phred values, or None: absent).
A reference is a list of contig strings; known sites are a set of (contig,
0-based position).  Tables: ctx[n_rg, 94, 16, 2] and cyc[n_rg, 94, 1000, 2] of
int64 (observations, errors).
"""
import math
import random
import re
import sys

import numpy as np

NQ, NCTX, NCYC, MAX_CYCLE, MAX_QE = 94, 16, 1000, 500, 60
PAIRED, UNMAPPED, REVERSE, READ2 = 0x1, 0x4, 0x10, 0x80
SECONDARY, QCFAIL, DUPLICATE, SUPPLEMENTARY = 0x100, 0x200, 0x400, 0x800
FILTER = UNMAPPED | SECONDARY | QCFAIL | DUPLICATE
DBL_MAX = sys.float_info.max
MAX_OBS = 2 ** 31 - 2
OPS = "MIDNSHP=X"


class Refused(ValueError):
    """What the host path throws and the ABI answers with FCS_ERR_INVALID."""


def parse_cigar(text):
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", text)]


def code(ch):
    return "ACGT".find(ch.upper()) if len(ch) == 1 and ch.upper() in "ACGT" else -1


def rec(flag, ref, pos, cigar, seq, qual, mapq=60, rg=0):
    if isinstance(qual, int):
        qual = [qual] * len(seq)
    return dict(flag=flag, ref=ref, pos=pos, mapq=mapq, rg=rg, cigar=cigar, seq=seq,
                qual=None if qual is None else list(qual))


# ------------------------------------------------------------------ the rules
def counted(r):
    return r["rg"] >= 0 and r["qual"] is not None and not r["flag"] & FILTER and r["mapq"] not in (0, 255)


def applied(r):
    return r["rg"] >= 0 and r["qual"] is not None


def sites(r):
    """Per read base: ('M', reference position), ('I', the aligned position before the insertion) or ('S', None)."""
    out, p = [], r["pos"]
    for n, op in parse_cigar(r["cigar"]):
        if op in "M=X":
            out += [("M", p + k) for k in range(n)]
            p += n
        elif op == "I":
            out += [("I", p - 1)] * n
        elif op == "S":
            out += [("S", None)] * n
        elif op in "DN":
            p += n
    return out


def clips(r):
    """Soft-clipped bases before the first and after the last of M / I / = / X."""
    lead = trail = 0
    seen = False
    for n, op in parse_cigar(r["cigar"]):
        if op == "S":
            if seen:
                trail += n
            else:
                lead += n
        elif op in "MI=X":
            seen, trail = True, 0
    return lead, trail


def covariates(seq, qual, reverse, second):
    """[(context key or -1, cycle key)] of every base of seq (the kept read, or the whole read in apply)."""
    k = len(seq)
    nl = 0
    while nl < k and qual[nl] <= 2:
        nl += 1
    nr = 0
    while nr < k and qual[k - 1 - nr] <= 2:
        nr += 1
    out = []
    for j in range(k):
        jp = j + 1 if reverse else j - 1
        cc = cp = -1
        if nl <= j < k - nr:
            cc = code(seq[j])
        if 0 <= jp < k and nl <= jp < k - nr:
            cp = code(seq[jp])
        if reverse:   # the reverse complement's bases
            cc = 3 - cc if cc >= 0 else -1
            cp = 3 - cp if cp >= 0 else -1
        cycle = k - j if reverse else j + 1
        out.append((4 * cp + cc if cc >= 0 and cp >= 0 else -1, 2 * (cycle - 1) + (1 if second else 0)))
    return out


def is_second(flag):
    return bool(flag & PAIRED) and bool(flag & READ2)


def new_tables(n_rg):
    return np.zeros((n_rg, NQ, NCTX, 2), np.int64), np.zeros((n_rg, NQ, NCYC, 2), np.int64)


def count(records, refs, known, n_rg, ctx, cyc):
    """Adds the batch's observations to ctx and cyc; Refused (and nothing added) on a record the rules refuse."""
    adds = []
    for r in records:
        if r["rg"] >= n_rg or r["rg"] < -1:
            raise Refused("rg")
        if not counted(r):
            continue
        L = len(r["seq"])
        st = sites(r)
        if len(st) != L or len(r["qual"]) != L or not 0 <= r["ref"] < len(refs):
            raise Refused("fields")
        lead, trail = clips(r)
        k = L - lead - trail
        if k > MAX_CYCLE:
            raise Refused("more than 500 kept bases")
        contig = refs[r["ref"]]
        cov = covariates(r["seq"][lead:L - trail], r["qual"][lead:L - trail], bool(r["flag"] & REVERSE),
                         is_second(r["flag"]))
        for j in range(k):
            i = lead + j
            kind, p = st[i]
            if kind == "M" and not 0 <= p < len(contig):
                raise Refused("an aligned base beyond its contig")
            q, c = r["qual"][i], code(r["seq"][i])
            if kind == "S" or c < 0 or q < 6 or q >= NQ:
                continue
            if 0 <= p < len(contig) and (r["ref"], p) in known:
                continue
            err = 1 if kind == "M" and code(contig[p]) != c else 0
            adds.append((r["rg"], q, cov[j][0], cov[j][1], err))
    for rg, q, ck, yk, err in adds:
        if ck >= 0:
            ctx[rg, q, ck] += (1, err)
        cyc[rg, q, yk] += (1, err)


def log10_prior(qe, prior):
    d = min(abs(int(qe - prior)), 40)
    v = 0.9 * math.exp(-(d * d) / 0.5)
    return math.log10(v) if v > 0 else -DBL_MAX


def emp_q(obs, err, prior):
    """GATK's RecalDatum empirical quality: the MAP over Qe = 0 .. 60, first maximum, capped at 93."""
    n, m = obs + 2, err + 1
    if n > MAX_OBS:
        m = math.floor(m * (MAX_OBS / n) + 0.5)
        n = MAX_OBS
    coeff = (math.lgamma(n + 1.0) - math.lgamma(m + 1.0) - math.lgamma(n - m + 1.0)) / math.log(10.0)
    best, best_v = 0, None
    for qe in range(MAX_QE + 1):
        p = math.pow(10.0, -qe / 10.0)
        lik = coeff + (m * (-qe / 10.0) if m else 0.0)
        if n - m:
            lik = lik + ((n - m) * math.log10(1.0 - p) if 1.0 - p > 0 else -math.inf)
        if not math.isfinite(lik):
            lik = -DBL_MAX
        v = log10_prior(float(qe), prior) + lik
        if best_v is None or v > best_v:
            best, best_v = qe, v
    return float(min(best, NQ - 1))


def finalize(ctx, cyc):
    """base[n_rg, 94], dctx[n_rg, 94, 16], dcyc[n_rg, 94, 1000] of float64."""
    n_rg = ctx.shape[0]
    base, dctx, dcyc = np.zeros((n_rg, NQ)), np.zeros((n_rg, NQ, NCTX)), np.zeros((n_rg, NQ, NCYC))
    for rg in range(n_rg):
        qt = cyc[rg].sum(axis=1)   # [94, 2]: every observation has a cycle
        obs, err = int(qt[:, 0].sum()), int(qt[:, 1].sum())
        if obs == 0:
            base[rg] = np.arange(NQ)
            continue
        exp_err = 0.0
        for q in range(NQ):
            exp_err += float(qt[q, 0]) * math.pow(10.0, -q / 10.0)
        eps = -10.0 * math.log10(exp_err / float(obs))
        prior_q = eps + (emp_q(obs, err, eps) - eps)
        for q in range(NQ):
            b = prior_q
            if qt[q, 0] > 0:
                b = prior_q + (emp_q(int(qt[q, 0]), int(qt[q, 1]), prior_q) - prior_q)
            base[rg, q] = b
            for tab, out in ((ctx, dctx), (cyc, dcyc)):
                for k in np.nonzero(tab[rg, q, :, 0])[0]:
                    out[rg, q, k] = emp_q(int(tab[rg, q, k, 0]), int(tab[rg, q, k, 1]), b) - b
    return base, dctx, dcyc


def new_quality(q, base, dc, dy):
    v = ((base + dc) + dy) + 0.5
    if not v >= 1.0:
        return 1
    return 93 if v > 93.0 else int(v)


def apply(records, base, dctx, dcyc):
    """The new qualities of every record (None where absent); Refused on an applied record beyond 500 bases."""
    for r in records:
        if applied(r) and (len(r["seq"]) > MAX_CYCLE or r["rg"] >= base.shape[0] or len(r["qual"]) != len(r["seq"])):
            raise Refused("more than 500 bases")
    out = []
    for r in records:
        if not applied(r):
            out.append(None if r["qual"] is None else list(r["qual"]))
            continue
        cov = covariates(r["seq"], r["qual"], bool(r["flag"] & REVERSE), is_second(r["flag"]))
        rg, new = r["rg"], []
        for q, (ck, yk) in zip(r["qual"], cov):
            if q < 6 or q >= NQ:
                new.append(q)
            else:
                new.append(new_quality(q, base[rg, q], dctx[rg, q, ck] if ck >= 0 else 0.0, dcyc[rg, q, yk]))
        out.append(new)
    return out


# ------------------------------------------------------------------ the report
ARGUMENTS = [("binary_tag_name", "null"),
             ("covariate", "ReadGroupCovariate,QualityScoreCovariate,ContextCovariate,CycleCovariate"),
             ("default_platform", "null"), ("deletions_default_quality", "45"), ("force_platform", "null"),
             ("indels_context_size", "3"), ("insertions_default_quality", "45"), ("low_quality_tail", "2"),
             ("maximum_cycle_value", "500"), ("mismatches_context_size", "2"), ("mismatches_default_quality", "-1"),
             ("no_standard_covs", "false"), ("quantizing_levels", "16"), ("recalibration_report", "null"),
             ("run_without_dbsnp", "false"), ("solid_nocall_strategy", "THROW_EXCEPTION"),
             ("solid_recal_mode", "SET_Q_ZERO")]


def _table(name, desc, cols, rows):
    """A GATKReport v1.1 table: strings flush left, numbers flush right, two spaces between columns."""
    cells = [[(f % v) for (_, f), v in zip(cols, row)] for row in rows]
    width = [max([len(c)] + [len(row[k]) for row in cells]) for k, (c, _) in enumerate(cols)]
    out = ["#:GATKTable:%d:%d:%s:;" % (len(cols), len(rows), ":".join(f for _, f in cols)),
           "#:GATKTable:%s:%s" % (name, desc)]

    def line(vals):
        return "  ".join(v.ljust(w) if f == "%s" else v.rjust(w) for v, w, (_, f) in zip(vals, width, cols)).rstrip()
    out.append(line([c for c, _ in cols]))
    out += [line(row) for row in cells]
    return "\n".join(out) + "\n\n"


def report(ctx, cyc, names):
    n_rg = ctx.shape[0]
    qt = cyc.sum(axis=2)   # [n_rg, 94, 2]
    text = "#:GATKReport.v1.1:5\n"
    text += _table("Arguments", "Recalibration argument collection values used in this run",
                   [("Argument", "%s"), ("Value", "%s")], ARGUMENTS)
    text += _table("Quantized", "Quality quantization map",
                   [("QualityScore", "%d"), ("Count", "%d"), ("QuantizedScore", "%d")],
                   [(q, int(qt[:, q, 0].sum()), q) for q in range(NQ)])
    t0, t1, t2 = [], [], []
    for rg in range(n_rg):
        obs, err = int(qt[rg, :, 0].sum()), int(qt[rg, :, 1].sum())
        if obs == 0:
            continue
        exp_err = 0.0
        for q in range(NQ):
            exp_err += float(qt[rg, q, 0]) * math.pow(10.0, -q / 10.0)
        eps = -10.0 * math.log10(exp_err / float(obs))
        t0.append((names[rg], "M", emp_q(obs, err, eps), eps, obs, float(err)))
        for q in range(NQ):
            if qt[rg, q, 0] > 0:
                t1.append((names[rg], q, "M", emp_q(int(qt[rg, q, 0]), int(qt[rg, q, 1]), float(q)), int(qt[rg, q, 0]),
                           float(qt[rg, q, 1])))
            for k in np.nonzero(ctx[rg, q, :, 0])[0]:
                o, e = int(ctx[rg, q, k, 0]), int(ctx[rg, q, k, 1])
                t2.append((names[rg], q, "ACGT"[k // 4] + "ACGT"[k % 4], "Context", "M", emp_q(o, e, float(q)), o, float(e)))
            for k in np.nonzero(cyc[rg, q, :, 0])[0]:
                o, e = int(cyc[rg, q, k, 0]), int(cyc[rg, q, k, 1])
                cycle = (k // 2 + 1) * (-1 if k % 2 else 1)
                t2.append((names[rg], q, str(cycle), "Cycle", "M", emp_q(o, e, float(q)), o, float(e)))
    text += _table("RecalTable0", "", [("ReadGroup", "%s"), ("EventType", "%s"), ("EmpiricalQuality", "%.4f"),
                                       ("EstimatedQReported", "%.4f"), ("Observations", "%d"), ("Errors", "%.2f")], t0)
    text += _table("RecalTable1", "", [("ReadGroup", "%s"), ("QualityScore", "%d"), ("EventType", "%s"),
                                       ("EmpiricalQuality", "%.4f"), ("Observations", "%d"), ("Errors", "%.2f")], t1)
    text += _table("RecalTable2", "", [("ReadGroup", "%s"), ("QualityScore", "%d"), ("CovariateValue", "%s"),
                                       ("CovariateName", "%s"), ("EventType", "%s"), ("EmpiricalQuality", "%.4f"),
                                       ("Observations", "%d"), ("Errors", "%.2f")], t2)
    return text


# ------------------------------------------------------------------ flat batches
def cigar_words(text):
    return [(n << 4) | OPS.index(op) for n, op in parse_cigar(text)]


def flatten(records, first_offset=0):
    """The arrays of an fcsbq_batch (fcship.bq_arrays' order); base_off starts at first_offset."""
    flag = np.array([r["flag"] for r in records], np.uint16)
    ref_id = np.array([r["ref"] for r in records], np.int32)
    pos = np.array([r["pos"] for r in records], np.int32)
    mapq = np.array([r["mapq"] for r in records], np.uint8)
    rg = np.array([r["rg"] for r in records], np.int32)
    cigar, cigar_off, base_off = [], [0], [first_offset]
    bases, qual = bytearray(b"N" * first_offset), bytearray(b"\xff" * first_offset)
    for r in records:
        cigar += cigar_words(r["cigar"])
        cigar_off.append(len(cigar))
        bases += r["seq"].encode()
        qual += bytes([0xFF] * len(r["seq"]) if r["qual"] is None else r["qual"])
        base_off.append(len(bases))
    absent = np.array([r["qual"] is None for r in records], np.uint8)
    return (flag, ref_id, pos, mapq, rg, np.array(cigar, np.uint32), np.array(cigar_off, np.int64),
            np.frombuffer(bytes(bases), np.uint8), np.frombuffer(bytes(qual), np.uint8), np.array(base_off, np.int64),
            absent)


def flat_reference(refs, known):
    """(bases, ref_off[n_ref + 1], known bitmap as uint64 words) of the reference handle."""
    off = np.zeros(len(refs) + 1, np.int64)
    for k, s in enumerate(refs):
        off[k + 1] = off[k] + len(s)
    bits = np.zeros((int(off[-1]) + 63) // 64 + 1, np.uint64)
    for c, p in known:
        g = int(off[c]) + p
        bits[g >> 6] |= np.uint64(1 << (g & 63))
    return np.frombuffer("".join(refs).encode(), np.uint8), off, bits


def known_from_vcf(vcf_records, names, refs):
    """VCF (CHROM, POS, REF) records -> the known set: positions POS-1 .. POS-1+len(REF)-1."""
    known = set()
    for chrom, pos, ref in vcf_records:
        if chrom in names:
            c = names.index(chrom)
            known |= {(c, p) for p in range(pos - 1, pos - 1 + len(ref)) if 0 <= p < len(refs[c])}
    return known


def unflatten_quals(records, out_qual, first_offset=0):
    out, o = [], first_offset
    for r in records:
        n = len(r["seq"])
        out.append(None if r["qual"] is None else list(out_qual[o:o + n]))
        o += n
    return out


# ------------------------------------------------------------------ the hand cases' world
def _ref0():
    s = list("ACGT" * 32)
    s[80:84] = "acgt"
    s[85] = "N"
    return "".join(s)


REFS = [_ref0(), "TTGCA" * 8, "ACGT" * 150]
NAMES = ["chr1", "chr2", "chr3"]
# case 6's known sites as VCF records (CHROM, POS 1-based, REF)
VCF = [("chr1", 21, "A"), ("chr1", 25, "ACG"), ("chr1", 31, "G"), ("chr1", 64, "T"), ("chr1", 65, "A"),
       ("chr2", 1, "T"), ("chr2", 40, "A"), ("chrUn", 5, "A")]
KNOWN = known_from_vcf(VCF, NAMES, REFS)

# case 14's table: base = q - 2 everywhere; the context AC (key 1) adds 1.25; cycle 1 (key 0) takes 3, cycle 2
# (key 2) adds 0.25; every other delta is 0.
def hand_table(n_rg=1):
    base = np.tile(np.arange(NQ, dtype=np.float64) - 2.0, (n_rg, 1))
    dctx, dcyc = np.zeros((n_rg, NQ, NCTX)), np.zeros((n_rg, NQ, NCYC))
    dctx[:, :, 1] = 1.25
    dcyc[:, :, 0] = -3.0
    dcyc[:, :, 2] = 0.25
    return base, dctx, dcyc


def _cells(q, ctx, cyc, rg=0):
    """{('ctx' | 'cyc', rg, q, key): (observations, errors)} from {key: (obs, err)} maps."""
    out = {("ctx", rg, q, k): v for k, v in ctx.items()}
    out.update({("cyc", rg, q, k): v for k, v in cyc.items()})
    return out


def hand_cases():
    """[dict(name, records, n_rg, want, refused, table, want_qual)]: `want` the non-zero cells after count;
    `refused`: records that count and apply refuse; `table`: 'hand' (hand_table) or 'final' (finalize of the
    counts), with `want_qual` what apply then gives."""
    C = []

    def case(name, records, want, n_rg=1, refused=None, table=None, want_qual=None):
        C.append(dict(name=name, records=records, n_rg=n_rg, want=want, refused=refused, table=table,
                      want_qual=want_qual))

    one = lambda keys: {k: (1, 0) for k in keys}  # noqa: E731
    # 1. forward 10M at 4: ref ACGTACGTAC, the read has G for T at index 3.  Contexts (prev, cur): AC CG GG GA AC CG
    #    GT TA AC = 1 6 10 8 1 6 11 12 1; the mismatch is the GG; cycles 1 .. 10 = keys 0, 2 .. 18, the mismatch 4.
    fwd = rec(0, 0, 4, "10M", "ACGGACGTAC", 30)
    ctx1 = {1: (3, 0), 6: (2, 0), 10: (1, 1), 8: (1, 0), 11: (1, 0), 12: (1, 0)}
    case("forward_one_mismatch", [fwd], _cells(30, ctx1, {**one(range(0, 20, 2)), 6: (1, 1)}))
    # 2. the same bases on the reverse strand: sequencing order is GTACGTCCGT, contexts GT TA AC CG GT TC CC CG GT =
    #    11 12 1 6 11 13 5 6 11; index 3 is cycle 7 (key 12) and the C after T (13).
    case("reverse_strand", [dict(fwd, flag=REVERSE)],
         _cells(30, {11: (3, 0), 12: (1, 0), 1: (1, 0), 6: (2, 0), 13: (1, 1), 5: (1, 0)},
                {**one(range(0, 20, 2)), 12: (1, 1)}))
    # 3. second of pair: cycles -1 .. -10 = keys 1, 3 .. 19, the mismatch -4 (key 7); contexts as in 1.
    case("second_of_pair", [dict(fwd, flag=PAIRED | READ2)], _cells(30, ctx1, {**one(range(1, 20, 2)), 7: (1, 1)}))
    # 4. 2S6M2S at 6: kept GTACGT = ref 6 .. 11; contexts GT TA AC CG GT; cycles 1 .. 6.  Apply with the hand table
    #    covers the clips: TTGTACGTAA at Q30 -> base 28; cycle 1 gives 28 - 3 + .5 -> 25, cycle 2 28.75 -> 28, the C
    #    after A (index 5) 28 + 1.25 + .5 -> 29, every other base 28.5 -> 28.
    case("soft_clips", [rec(0, 0, 6, "2S6M2S", "TTGTACGTAA", 30)],
         _cells(30, {11: (2, 0), 12: (1, 0), 1: (1, 0), 6: (1, 0)}, one(range(0, 12, 2))),
         table="hand", want_qual=[[25, 28, 28, 28, 28, 29, 28, 28, 28, 28]])
    # 5. 3M2I3M2D2M at 8: ACG | TT inserted | TAC with N for the A | 2 deleted | AC.  Index 6 (N) is skipped and
    #    index 7 has no context; contexts AC CG GT TT TT . . CA AC; cycles 1 .. 10 without 7; no error anywhere.
    case("insertion_deletion_n", [rec(0, 0, 8, "3M2I3M2D2M", "ACGTTTNCAC", 30)],
         _cells(30, {1: (2, 0), 6: (1, 0), 11: (1, 0), 15: (2, 0), 4: (1, 0)}, one([0, 2, 4, 6, 8, 10, 14, 16, 18])))
    # 6. known sites (VCF above): chr1 20; 24 25 26; 30 (the anchor of an insertion); 63 64; chr2 0 and 39.
    #    a 10M at 16 ACGTCCGTAC: the mismatch at 20 and the bases at 24 25 are hidden; contexts AC CG GT . CC CG GT.
    #    b 3M2I3M at 28 ACG TT TAC: 30 and both inserted bases hidden; contexts AC . . . TT TA AC.
    #    c 4M at 62 GTAC: 63 64 hidden; AC at index 3.   d chr2 3M at 0 TTG: 0 hidden, TT TG;  3M at 37 GCA: 39
    #    hidden, GC.  18 observations, no error.
    case("known_sites", [rec(0, 0, 16, "10M", "ACGTCCGTAC", 30), rec(0, 0, 28, "3M2I3M", "ACGTTTAC", 30),
                         rec(0, 0, 62, "4M", "GTAC", 30), rec(0, 1, 0, "3M", "TTG", 30), rec(0, 1, 37, "3M", "GCA", 30)],
         _cells(30, {1: (4, 0), 6: (2, 0), 11: (2, 0), 5: (1, 0), 15: (2, 0), 12: (1, 0), 14: (1, 0), 9: (1, 0)},
                {0: (4, 0), 2: (4, 0), 4: (2, 0), 6: (2, 0), 10: (2, 0), 12: (2, 0), 14: (2, 0)}))
    # 7. 8M at 40 ACNTACGT, index 4 at Q5: indexes 2 and 4 skipped, index 3 without context (after N), index 5
    #    keeps AC (a low quality inside the read is no N).
    q7 = [30, 30, 30, 30, 5, 30, 30, 30]
    case("n_and_low_quality", [rec(0, 0, 40, "8M", "ACNTACGT", q7)],
         _cells(30, {1: (2, 0), 6: (1, 0), 11: (1, 0)}, one([0, 2, 6, 10, 12, 14])))
    # 8. qualities 2 2 . . . . 2 1: the ends are N for the context, so index 2 has none; GT TA AC; cycles 3 .. 6.
    case("low_quality_ends", [rec(0, 0, 40, "8M", "ACGTACGT", [2, 2, 30, 30, 30, 30, 2, 1])],
         _cells(30, {11: (1, 0), 12: (1, 0), 1: (1, 0)}, one([4, 6, 8, 10])))
    # 9. eight records that are not counted and a supplementary one that is: AC CG GT, cycles 1 .. 4.
    f = lambda **kw: dict(rec(0, 0, 40, "4M", "ACGT", 30), **kw)  # noqa: E731
    case("filters", [f(flag=UNMAPPED), f(flag=SECONDARY), f(flag=QCFAIL), f(flag=DUPLICATE), f(mapq=0), f(mapq=255),
                     f(rg=-1), f(qual=None), f(flag=SUPPLEMENTARY)],
         _cells(30, one([1, 6, 11]), one([0, 2, 4, 6])))
    # 10. 8M at 80 over acgtANGT: the lower-case bases match, the reference N at 85 is an error of index 5 (AC, cycle 6).
    case("lower_case_and_n_reference", [rec(0, 0, 80, "8M", "ACGTACGT", 30)],
         _cells(30, {1: (2, 1), 6: (2, 0), 11: (2, 0), 12: (1, 0)}, {**one(range(0, 16, 2)), 10: (1, 1)}))
    # 11. 2H3=1X2P4M2H at 40: ACG | A against T | ACGT; contexts AC CG GA AA AC CG GT, the X base is the error.
    case("eq_x_h_p_ops", [rec(0, 0, 40, "2H3=1X2P4M2H", "ACGAACGT", 30)],
         _cells(30, {1: (2, 0), 6: (2, 0), 8: (1, 1), 0: (1, 0), 11: (1, 0)}, {**one(range(0, 16, 2)), 6: (1, 1)}))
    # 12. 500M on chr3 (ACGT x 150): 125 each of AC CG GT and 124 TA; cycles 1 .. 500 once each.  501M is refused.
    case("cycle_500_and_501", [rec(0, 2, 0, "500M", ("ACGT" * 125), 30)],
         _cells(30, {1: (125, 0), 6: (125, 0), 11: (125, 0), 12: (124, 0)}, one(range(0, 1000, 2))),
         refused=[rec(0, 2, 0, "501M", ("ACGT" * 126)[:501], 30)])
    # 13. read group 0 holds case 1's read (10 observations, 1 error, all Q30), read group 1 only a duplicate.
    #     Finalise: eps = 30; empQ_rg: n 12 m 2, log10 lik -4.19 at 30, -3.99 at 29, the prior costs 0.87 d^2, so 30
    #     and dR = 0; the Q30 datum has the same counts, dQ = 0; a covariate cell of one error in one (n 3 m 2) has
    #     lik -5.52 at 30, -5.32 at 29: 30 again.  So base[0][q] = 30 for every q and every delta is 0: read group 0's
    #     duplicate at Q20 becomes 30.5 -> 30, its Q30 read stays; read group 1 has no observation and keeps its 20s.
    case("two_read_groups",
         [fwd, rec(DUPLICATE, 0, 4, "10M", "ACGGACGTAC", 20), rec(DUPLICATE, 0, 4, "10M", "ACGGACGTAC", 20, rg=1)],
         _cells(30, ctx1, {**one(range(0, 20, 2)), 6: (1, 1)}), n_rg=2, table="final",
         want_qual=[[30] * 10, [30] * 10, [20] * 10])
    # 14. the hand table on ACACG with qualities 30 30 5 40 2: index 0 28 - 3 + .5 -> 25; index 1 (AC, cycle 2)
    #     28 + 1.25 + .25 + .5 -> 30; index 2 stays (Q5); index 3 (AC) 38 + 1.25 + .5 -> 39; index 4 stays (Q2).
    case("apply_hand_table", [rec(DUPLICATE, 0, 4, "5M", "ACACG", [30, 30, 5, 40, 2])], {}, table="hand",
         want_qual=[[25, 30, 5, 39, 2]])
    return C


def dense(want, n_rg):
    ctx, cyc = new_tables(n_rg)
    for (kind, rg, q, k), v in want.items():
        (ctx if kind == "ctx" else cyc)[rg, q, k] = v
    return ctx, cyc


def case_table(case, ctx, cyc):
    return hand_table(case["n_rg"]) if case["table"] == "hand" else finalize(ctx, cyc)


# ------------------------------------------------------------------ built batches
SWEEP_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 151)


def random_world(seed=7, length=6000, n_contigs=2):
    rnd = random.Random(seed)
    refs = []
    for _ in range(n_contigs):
        s = [rnd.choice("ACGT") for _ in range(length)]
        for _ in range(length // 200):
            p = rnd.randrange(length)
            s[p] = rnd.choice("Nacgt")
        refs.append("".join(s))
    known = {(c, p) for c in range(n_contigs) for p in range(length) if rnd.random() < 0.03}
    return refs, known


def random_read(rnd, refs, length, rg):
    c = rnd.randrange(len(refs))
    lead = rnd.choice((0, 0, 0, 3, 10)) if length > 12 else 0
    trail = rnd.choice((0, 0, 0, 2, 7)) if length - lead > 9 else 0
    body = length - lead - trail
    pos = rnd.randrange(20, len(refs[c]) - body - 30)
    ops, seq, p = [], [], pos
    if lead:
        ops.append((lead, "S"))
        seq += [rnd.choice("ACGT") for _ in range(lead)]
    left = body
    while left > 0:
        n = left if rnd.random() < 0.5 else rnd.randrange(1, left + 1)
        op = rnd.choice("MMMM=X")
        ops.append((n, op))
        for k in range(n):
            b = refs[c][p + k].upper()
            # errors gather at the read's first bases and after a T, so that cycle and context deltas arise
            rate = 0.5 if len(seq) < 4 else 0.3 if seq and seq[-1] == "T" else 0.02
            seq.append(rnd.choice("ACGTN") if rnd.random() < rate or b == "N" and rnd.random() < 0.5 else b)
        p += n
        left -= n
        if left > 1 and rnd.random() < 0.4:
            if rnd.random() < 0.5:
                m = rnd.randrange(1, min(4, left) + 1)
                ops.append((m, "I"))
                seq += [rnd.choice("ACGT") for _ in range(m)]
                left -= m
            else:
                d = rnd.randrange(1, 5)
                ops.append((d, rnd.choice("DN")))
                p += d
    if trail:
        ops.append((trail, "S"))
        seq += [rnd.choice("ACGT") for _ in range(trail)]
    if rnd.random() < 0.1:
        ops = [(5, "H")] + ops
    if ops[-1][1] in "DN":
        ops.pop()
    merged = []
    for n, op in ops:
        if merged and merged[-1][1] == op:
            merged[-1] = (merged[-1][0] + n, op)
        else:
            merged.append((n, op))
    qual = [rnd.choice((1, 2, 2, 5, 6, 11, 25, 25, 25, 37, 37, 40)) for _ in range(length)]
    if rnd.random() < 0.2:
        for k in range(rnd.randrange(0, min(4, length) + 1)):
            qual[k] = 2
            qual[length - 1 - k] = 2
    flag = rnd.choice((0, REVERSE, PAIRED | 0x40, PAIRED | READ2, PAIRED | READ2 | REVERSE, PAIRED | 0x40 | REVERSE))
    if rnd.random() < 0.08:
        flag |= rnd.choice((UNMAPPED, SECONDARY, QCFAIL, DUPLICATE, SUPPLEMENTARY))
    r = rec(flag, c, pos, "".join(f"{n}{op}" for n, op in merged), "".join(seq), qual,
            mapq=rnd.choice((0, 255, 20, 60, 60, 60, 60, 60)), rg=rg)
    if rnd.random() < 0.03:
        r["qual"] = None
    assert len(sites(r)) == length, r
    return r


def random_batch(seed=11, n=1200, n_rg=3, refs=None, lengths=(1, 2, 30, 76, 100, 151, 151, 151, 250)):
    rnd = random.Random(seed)
    return [random_read(rnd, refs, rnd.choice(lengths), rnd.randrange(-1, n_rg) if rnd.random() < 0.05
                        else rnd.randrange(n_rg)) for _ in range(n)]


def sweep_batch(refs, seed=3):
    """Every length of SWEEP_LENGTHS at every residue of base_off mod 4 (fillers without a read group between)."""
    rnd = random.Random(seed)
    records, off, seen = [], 0, set()
    for length in SWEEP_LENGTHS:
        for residue in range(4):
            pad = (residue - off) % 4
            if pad:
                records.append(rec(UNMAPPED, -1, -1, "", "N" * pad, 0, rg=-1))
                off += pad
            records.append(random_read(rnd, refs, length, rnd.randrange(3)))
            records[-1]["flag"] &= ~(UNMAPPED | SECONDARY | QCFAIL | DUPLICATE)
            records[-1]["mapq"] = 60
            seen.add((length, off % 4))
            off += length
    assert len(seen) == 4 * len(SWEEP_LENGTHS)
    return records


def one_hot_read(copies=20000):
    """One 151M read at one quality, many times: one hot cell per cycle."""
    seq = (REFS[2] * 2)[3:154]
    return [rec(0, 2, 3, "151M", seq, 33)] * copies
