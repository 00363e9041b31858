"""GenotypeGVCFs, round 20 (DESIGN §2 [EXT], §4.13): the rules restated in Python,
the hand cases with their expected lines, and the cohort builders.

Two levels.  The integer level is what fcsjg_genotype computes: genotype(cohort,
pos, n_alt, tables, min_qual) returns fcsjg_out's arrays.  It is numpy int64
throughout, vectorised over (site, ALT) items and allele counts, with one Python
loop over the samples, so that a cohort of a thousand samples or of a hundred
thousand sites takes seconds.  The text level is what the command does around
it: parse_gvcf, combine, emit and command_vcf.
"""
import math

import numpy as np

UNIT_BITS = 20
ONE = 1 << UNIT_BITS
PL_MAX = ONE - 1
ALTS_MAX = 6
S_ROWS = 1282
CUT = 80 << UNIT_BITS
BLOCK, CALL, NO_CALL = 0, 1, 255
GENOTYPES_MAX = 28
OUT_NAMES = ("q", "mle", "qual", "kept", "ac", "an", "dp", "pl_off", "src", "gt", "gq", "pl", "n_pl")


class Refused(Exception):
    pass


def rnd(x):
    """llround for the values met here (none is negative and at a half)."""
    return int(math.floor(x + 0.5))


# ------------------------------------------------------------------ the tables
def tables(het, n_samples):
    """S[1282], LG[4 n + 1], LP[2 n + 1] as int64 arrays."""
    S = np.array([rnd(10.0 * math.log10(1.0 + 10.0 ** (-i / 160.0)) * 1048576.0) for i in range(S_ROWS)], np.int64)
    LG = np.array([0] + [rnd(10.0 * math.log10(float(n)) * 1048576.0) for n in range(1, 4 * n_samples + 1)], np.int64)
    rest = 1.0
    for k in range(1, 2 * n_samples + 1):
        rest -= het / k
    if not rest > 0.0:
        raise Refused("no prior for k = 0")
    LP = np.array([rnd(10.0 * math.log10(rest) * 1048576.0)] +
                  [rnd(10.0 * math.log10(het / k) * 1048576.0) for k in range(1, 2 * n_samples + 1)], np.int64)
    return S, LG, LP


def min_qual(stand_call_conf=10.0):
    return rnd(stand_call_conf * 1048576.0)


def lse(a, b, S):
    """max + S[d >> 16], interpolated on the low 16 bits of d = max - min; the maximum alone from 80 PL on."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    hi = np.maximum(a, b)
    d = hi - np.minimum(a, b)
    i = np.minimum(d >> 16, S_ROWS - 2)
    f = d & 0xFFFF
    s0, s1 = S[i], S[i + 1]
    return np.where(d >= CUT, hi, hi + s0 - (((s0 - s1) * f) >> 16))


# ------------------------------------------------------------------ the integer level
def own(kind, alt, x):
    """The own allele of merged allele x for records of kind and merged ALT index alt (arrays)."""
    return np.where(x == 0, 0, np.where(kind == BLOCK, 1, np.where(x == alt, 1, 2)))


def pl_index(a, b):
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return hi * (hi + 1) // 2 + lo


def sources(rec_off, beg, end, kind, pos):
    """src[site, sample]: the last record with beg <= p, on equal beg the first; -1 for a no-call."""
    n = len(rec_off) - 1
    pos = np.asarray(pos, np.int64)
    src = np.full((len(pos), n), -1, np.int64)
    for s in range(n):
        lo, hi = int(rec_off[s]), int(rec_off[s + 1])
        b, e, k = beg[lo:hi].astype(np.int64), end[lo:hi].astype(np.int64), kind[lo:hi]
        if hi == lo:
            continue
        a = np.searchsorted(b, pos, "right")
        have = a > 0
        at = b[np.maximum(a - 1, 0)]
        c = np.searchsorted(b, at, "left")
        ok = have & (pos < e[c]) & ((k[c] == BLOCK) | (at == pos))
        src[:, s] = np.where(ok, lo + c, -1)
    return src


def collapse(kind, alt, n_alt, i, pl):
    """c[., 3] of ALT i for records (kind, alt, pl[., 6]) at sites of n_alt ALTs, the minimum subtracted."""
    big = np.int64(1) << 40
    oi = own(kind, alt, i)
    rows = np.arange(len(kind))
    c0 = np.full(len(kind), big)
    c1 = np.full(len(kind), big)
    for x in range(ALTS_MAX + 1):
        okx = (x <= n_alt) & (x != i)
        ox = own(kind, alt, np.full(len(kind), x))
        c1 = np.where(okx, np.minimum(c1, pl[rows, pl_index(ox, oi)]), c1)
        for y in range(x, ALTS_MAX + 1):
            oky = okx & (y <= n_alt) & (y != i)
            oy = own(kind, alt, np.full(len(kind), y))
            c0 = np.where(oky, np.minimum(c0, pl[rows, pl_index(ox, oy)]), c0)
    c2 = pl[rows, pl_index(oi, oi)]
    c = np.stack([c0, c1, c2], 1)
    return c - c.min(1, keepdims=True)


def exact_model(cc, called, S, LG, LP):
    """cc[item, sample, 3], called[item, sample] -> (q, mle, z) per item; z is the last row, for the tests."""
    items, n = called.shape
    K = 2 * n + 1
    k = np.arange(K, dtype=np.int64)[None, :]
    z = np.zeros((items, K), np.int64)
    j = np.zeros(items, np.int64)
    top = len(LG) - 1
    for s in range(n):
        on = called[:, s]
        if not on.any():
            continue
        j = j + on
        g = -(cc[:, s, :].astype(np.int64) << UNIT_BITS)
        m = 2 * j[:, None] - k
        z1 = np.concatenate([np.zeros((items, 1), np.int64), z[:, :-1]], 1)
        z2 = np.concatenate([np.zeros((items, 2), np.int64), z[:, :-2]], 1)
        lg = lambda v: LG[np.clip(v, 0, top)]  # noqa: E731
        p0 = m >= 2
        acc = np.where(p0, z + g[:, 0:1] + lg(m) + lg(m - 1), 0)
        have = p0
        p1 = (k >= 1) & (m >= 1)
        t = z1 + g[:, 1:2] + lg(2 * k) + lg(m)
        acc = np.where(p1, np.where(have, lse(acc, t, S), t), acc)
        have = have | p1
        p2 = (k >= 2) & (m >= 0)
        t = z2 + g[:, 2:3] + lg(k) + lg(k - 1)
        acc = np.where(p2, np.where(have, lse(acc, t, S), t), acc)
        new = acc - (lg(2 * j) + lg(2 * j - 1))[:, None]
        z = np.where(on[:, None] & (m >= 0), new, z)
    valid = k <= 2 * j[:, None]
    post = z + LP[np.minimum(k, len(LP) - 1)]
    acc = post[:, 0].copy()
    for kk in range(1, K):
        live = kk <= 2 * j
        if not live.any():
            break
        acc = np.where(live, lse(acc, post[:, kk], S), acc)
    q = acc - post[:, 0]
    mle = np.argmax(np.where(valid, post, np.iinfo(np.int64).min), 1)
    return q, mle.astype(np.int32), z


def kept_list(mask):
    return [0] + [i for i in range(1, ALTS_MAX + 1) if mask >> (i - 1) & 1]


def genotype(cohort, pos, n_alt, tabs, minq, max_pl=None):
    """fcsjg_out's arrays ({name: array}; pl cut to n_pl) of cohort = (rec_off, beg, end, kind, alt, dp, pl[., 6])."""
    rec_off, beg, end, kind, alt, dp, pl = (np.asarray(a) for a in cohort)
    pl = np.clip(pl.astype(np.int64).reshape(-1, 6), 0, PL_MAX)
    S, LG, LP = (np.asarray(t, np.int64) for t in tabs)
    n, ns = len(rec_off) - 1, len(pos)
    n_alt = np.asarray(n_alt, np.int64)
    src = sources(rec_off, beg, end, kind, pos)
    out = {"src": src.reshape(-1).copy()}
    q = np.zeros((ns, ALTS_MAX), np.int64)
    mle = np.zeros((ns, ALTS_MAX), np.int32)
    # the items: (site, ALT i) with i <= n_alt
    site_of, alt_of = np.nonzero(np.arange(1, ALTS_MAX + 1)[None, :] <= n_alt[:, None])
    if len(site_of):
        isrc = src[site_of]                                   # [item, sample]
        called = isrc >= 0
        r = np.maximum(isrc, 0).reshape(-1)
        cc = collapse(kind[r], alt[r].astype(np.int64), np.repeat(n_alt[site_of], n), np.repeat(alt_of + 1, n), pl[r])
        qi, mi, _ = exact_model(cc.reshape(len(site_of), n, 3), called, S, LG, LP)
        q[site_of, alt_of], mle[site_of, alt_of] = qi, mi
    keep = mle > 0
    kept = (keep * (1 << np.arange(ALTS_MAX))[None, :]).sum(1).astype(np.uint8)
    qual = (q * keep).sum(1)
    K = keep.sum(1)
    G = (K + 1) * (K + 2) // 2
    written = (kept != 0) & (qual >= minq)
    counts = np.where(written, n * G, 0)
    pl_off = np.where(written, np.cumsum(counts) - counts, -1)
    n_pl = int(counts.sum())
    if max_pl is not None and n_pl > max_pl:
        raise Refused(f"the sites written have {n_pl} PLs, max_pl is {max_pl}")
    gt = np.full((ns, n, 2), NO_CALL, np.uint8)
    gq = np.zeros((ns, n), np.uint8)
    ac = np.zeros((ns, ALTS_MAX), np.int32)
    an = np.zeros(ns, np.int32)
    dps = np.zeros(ns, np.int64)
    pls = np.zeros(n_pl, np.int32)
    for mask in np.unique(kept[written]):
        a = np.array(kept_list(int(mask)), np.int64)
        pairs = [(x, y) for y in range(len(a)) for x in range(y + 1)]
        sites = np.nonzero(written & (kept == mask))[0]
        s_src = src[sites]                                    # [site, sample]
        has = s_src >= 0
        r = np.maximum(s_src, 0)
        kd, al = kind[r], alt[r].astype(np.int64)
        vals = np.stack([pl[r, pl_index(own(kd, al, a[x]), own(kd, al, a[y]))] for x, y in pairs], 2)  # [site, sample, G]
        vals = vals - vals.min(2, keepdims=True)
        first = np.argmin(vals, 2)
        second = np.sort(vals, 2)[:, :, 1]
        call = has & (vals.max(2) > 0)
        ax = np.array([a[x] for x, _ in pairs], np.uint8)
        ay = np.array([a[y] for _, y in pairs], np.uint8)
        gt[sites, :, 0] = np.where(call, ax[first], NO_CALL)
        gt[sites, :, 1] = np.where(call, ay[first], NO_CALL)
        gq[sites] = np.where(call, np.minimum(second, 99), 0)
        an[sites] = 2 * call.sum(1)
        for i in a[1:]:
            ac[sites, i - 1] = ((ax[first] == i) & call).sum(1) + ((ay[first] == i) & call).sum(1)
        dps[sites] = np.where(has, dp[r].astype(np.int64), 0).sum(1)
        vals = np.where(has[:, :, None], vals, 0)
        for row, site in enumerate(sites):
            pls[pl_off[site]:pl_off[site] + n * len(pairs)] = vals[row].reshape(-1)
    out.update(q=q.reshape(-1), mle=mle.reshape(-1), qual=qual, kept=kept, ac=ac.reshape(-1), an=an, dp=dps, pl_off=pl_off,
               gt=gt.reshape(-1), gq=gq.reshape(-1), pl=pls, n_pl=np.array([n_pl], np.int64))
    return out


# ------------------------------------------------------------------ the text level
def parse_gvcf(text):
    """(sample, [(contig name, length)], {contig name: [record]}) of a GVCF; a record is a dict of beg, end, kind, dp,
    pl[6], ref, alt.  A sample's second and later call records at one POS are dropped."""
    contigs, sample, recs = [], None, {}
    last_call = None
    for ln in text.splitlines():
        if ln.startswith("##contig=<ID="):
            name, length = ln[len("##contig=<ID="):-1].split(",length=")
            contigs.append((name, int(length)))
        elif ln.startswith("#CHROM"):
            f = ln.split("\t")
            if len(f) != 10:
                raise Refused("samples")
            sample = f[9]
        elif ln.startswith("#"):
            continue
        else:
            f = ln.split("\t")
            if len(f) != 10:
                raise Refused("columns")
            chrom, pos, ref, alts = f[0], int(f[1]), f[3], f[4].split(",")
            if alts[-1] != "<NON_REF>" or len(alts) > 2:
                raise Refused("ALT")
            block = len(alts) == 1
            vals = dict(zip(f[8].split(":"), f[9].split(":")))
            if "PL" not in vals or len(vals["GT"].replace("|", "/").split("/")) != 2:
                raise Refused("PL or ploidy")
            pl = [min(int(v), PL_MAX) for v in vals["PL"].split(",")]
            if len(pl) != (3 if block else 6):
                raise Refused("PL count")
            end = pos - 1 + len(ref)
            if block:
                end = int([kv[4:] for kv in f[7].split(";") if kv.startswith("END=")][0])
            elif last_call == (chrom, pos):
                continue
            else:
                last_call = (chrom, pos)
            recs.setdefault(chrom, []).append(dict(beg=pos - 1, end=end, kind=BLOCK if block else CALL, dp=int(vals.get("DP", 0)),
                                                   pl=pl + [0] * (6 - len(pl)), ref=ref, alt=None if block else alts[0]))
    return sample, contigs, recs


def combine(samples, max_alt=ALTS_MAX):
    """samples: one record list per column.  (cohort arrays, pos, n_alt, REF per site, ALT texts per site)."""
    rec_off = np.cumsum([0] + [len(s) for s in samples])
    flat = [r for s in samples for r in s]
    alt = np.zeros(len(flat), np.uint8)
    by_pos = {}
    for s, recs in enumerate(samples):
        for k, r in enumerate(recs):
            if r["kind"] == CALL:
                by_pos.setdefault(r["beg"], []).append((s, int(rec_off[s]) + k, r))
    pos, n_alt, refs, alts = [], [], [], []
    for p in sorted(by_pos):
        group = by_pos[p]                                      # column order
        ref = max((r["ref"] for _, _, r in group), key=len)    # the first of the longest
        texts = [r["alt"] + ref[len(r["ref"]):] for _, _, r in group]
        distinct = []
        for t in texts:
            if t not in distinct:
                distinct.append(t)
        order = sorted(distinct, key=lambda t: -texts.count(t))  # stable: ties by first appearance
        keep = order[:max_alt]
        for (_, at, _), t in zip(group, texts):
            alt[at] = keep.index(t) + 1 if t in keep else 0
        pos.append(p), n_alt.append(len(keep)), refs.append(ref), alts.append(keep)
    cohort = (rec_off.astype(np.int64), np.array([r["beg"] for r in flat], np.int32), np.array([r["end"] for r in flat], np.int32),
              np.array([r["kind"] for r in flat], np.uint8), alt, np.array([r["dp"] for r in flat], np.int32),
              np.array([r["pl"] for r in flat], np.int32).reshape(-1, 6))
    return cohort, np.array(pos, np.int32), np.array(n_alt, np.uint8), refs, alts


def af_text(ac, an):
    return "1.00" if an > 0 and ac == an else "%.3f" % (ac / an if an > 0 else 0.0)


def emit(chrom, cohort, pos, refs, alts, o):
    """The records of the written sites."""
    n = len(cohort[0]) - 1
    dp = cohort[5]
    lines = []
    for k in range(len(pos)):
        off = int(o["pl_off"][k])
        if off < 0:
            continue
        a = kept_list(int(o["kept"][k]))
        G = len(a) * (len(a) + 1) // 2
        rank = {m: x for x, m in enumerate(a)}
        ac = [int(o["ac"][k * ALTS_MAX + i - 1]) for i in a[1:]]
        an = int(o["an"][k])
        info = (f"AC={','.join(map(str, ac))};AF={','.join(af_text(c, an) for c in ac)};AN={an};DP={int(o['dp'][k])}")
        cols = []
        for s in range(n):
            i = k * n + s
            if o["gt"][2 * i] == NO_CALL:
                cols.append("./.")
                continue
            pls = o["pl"][off + s * G:off + (s + 1) * G]
            cols.append(f"{rank[int(o['gt'][2 * i])]}/{rank[int(o['gt'][2 * i + 1])]}:{int(dp[o['src'][i]])}:{int(o['gq'][i])}:"
                        + ",".join(str(int(v)) for v in pls))
        lines.append("\t".join([chrom, str(int(pos[k]) + 1), ".", refs[k], ",".join(alts[k][i - 1] for i in a[1:]),
                                "%.2f" % (int(o["qual"][k]) / 1048576.0), ".", info, "GT:DP:GQ:PL"] + cols) + "\n")
    return "".join(lines)


HEADER_META = ('##INFO=<ID=AC,Number=A,Type=Integer,Description="Allele count in genotypes">\n'
               '##INFO=<ID=AF,Number=A,Type=Float,Description="Allele frequency">\n'
               '##INFO=<ID=AN,Number=1,Type=Integer,Description="Total number of alleles in called genotypes">\n'
               '##INFO=<ID=DP,Number=1,Type=Integer,Description="Sum of the samples\' DP">\n'
               '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
               '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Read depth of the sample\'s GVCF record">\n'
               '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality">\n'
               '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods">\n')


def header_text(samples, contigs):
    return ("##fileformat=VCFv4.2\n##source=fcs-genome joint (exact allele-frequency model)\n" + HEADER_META +
            "".join(f"##contig=<ID={n},length={ln}>\n" for n, ln in contigs) +
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples) + "\n")


def command_vcf(gvcf_texts, contigs, het=1e-3, conf=10.0, max_alt=ALTS_MAX, header=True):
    """The joint command's VCF for the GVCF texts (any order) on the reference's contigs."""
    parsed = sorted((parse_gvcf(t) for t in gvcf_texts), key=lambda p: p[0])
    names = [p[0] for p in parsed]
    tabs = tables(het, len(parsed))
    text = header_text(names, contigs) if header else ""
    for name, _ in contigs:
        cohort, pos, n_alt, refs, alts = combine([p[2].get(name, []) for p in parsed], max_alt)
        if len(pos):
            text += emit(name, cohort, pos, refs, alts, genotype(cohort, pos, n_alt, tabs, min_qual(conf)))
    return text


# ------------------------------------------------------------------ GVCF text
def block(pos, end, pl=(0, 30, 300), dp=20, ref="A", gq=None):
    """A <NON_REF> block line's fields after CHROM (1-based POS and END)."""
    gq = sorted(pl)[1] if gq is None else gq
    return (pos, f"{pos}\t.\t{ref}\t<NON_REF>\t.\t.\tEND={end}\tGT:DP:GQ:MIN_DP:PL\t0/0:{dp}:{min(gq, 99)}:{dp}:" + ",".join(map(str, pl)))


def call(pos, ref, alt, pl, dp=20, gt="0/1", ad=None):
    ad = ad or f"{dp // 2},{dp - dp // 2},0"
    gq = min(sorted(pl)[1], 99)
    return (pos, f"{pos}\t.\t{ref}\t{alt},<NON_REF>\t50.00\tPASS\tDP={dp}\tGT:AD:DP:GQ:PL\t{gt}:{ad}:{dp}:{gq}:" + ",".join(map(str, pl)))


def gvcf_text(sample, contigs, records):
    """records: {contig name: [block(...) or call(...)]} in file order."""
    head = "##fileformat=VCFv4.2\n##source=fcs-genome htc (GPU PairHMM)\n" + \
        "".join(f"##contig=<ID={n},length={ln}>\n" for n, ln in contigs) + \
        f"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t{sample}\n"
    return head + "".join(f"{name}\t{line}\n" for name, _ in contigs for _, line in records.get(name, []))


HET = (60, 0, 80, 90, 100, 200)      # own genotypes 0/0 0/1 1/1 0/2 1/2 2/2
HOM = (120, 30, 0, 130, 40, 210)
CONTIGS = [("ctgA", 1000), ("ctgB", 400)]


_S = "GT:DP:GQ:PL"
_HET3, _HOM3 = "20:60:60,0,80", "20:30:120,30,0"
# The record lines of the hand cases.  "one sample" by hand: c = (60, 0, 80), the row of one sample is z = g, so
# post = (-60.0065, -30, -113.01) PL with the priors of heterozygosity 0.001, mle = 1 and QUAL = lse - post[0] = 30.01.
EXPECTED = {
    "one sample": f"ctgA\t10\t.\tA\tG\t30.01\t.\tAC=1;AF=0.500;AN=2;DP=21\t{_S}\t0/1:21:60:60,0,80\n",
    "a site carried by one of three samples":
        f"ctgA\t20\t.\tC\tT\t75.28\t.\tAC=2;AF=0.333;AN=6;DP=56\t{_S}\t1/1:30:30:120,30,0\t0/0:15:45:0,45,450\t0/0:11:33:0,33,330\n",
    "a block ending at p - 1, at p and at p + 1":
        f"ctgA\t30\t.\tG\tA\t25.26\t.\tAC=1;AF=0.167;AN=6;DP=60\t{_S}\t0/1:{_HET3}\t./.\t0/0:20:30:0,30,300\t0/0:20:30:0,30,300\n",
    "a no-call from no coverage": f"ctgA\t40\t.\tT\tC\t30.01\t.\tAC=1;AF=0.500;AN=2;DP=20\t{_S}\t0/1:{_HET3}\t./.\t./.\n",
    "a no-call inside a deletion's span":
        f"ctgA\t50\t.\tGTAC\tG\t30.01\t.\tAC=1;AF=0.500;AN=2;DP=20\t{_S}\t./.\t0/1:{_HET3}\n"
        f"ctgA\t52\t.\tA\tT\t87.01\t.\tAC=2;AF=1.00;AN=2;DP=20\t{_S}\t1/1:{_HOM3}\t./.\n",
    "two ALTs at one POS":
        f"ctgA\t60\t.\tA\tT,C\t160.51\t.\tAC=3,1;AF=0.500,0.167;AN=6;DP=60\t{_S}\t0/2:20:60:60,90,200,0,100,80\t"
        "1/1:20:30:120,30,0,130,40,210\t0/1:20:60:60,0,80,90,100,200\n",
    "three ALTs at one POS":
        f"ctgA\t61\t.\tA\tC,T,G\t120.61\t.\tAC=1,2,1;AF=0.125,0.250,0.125;AN=8;DP=80\t{_S}\t0/1:20:60:60,0,80,90,100,200,90,100,200,200\t"
        "2/2:20:30:120,130,210,30,40,0,130,210,40,210\t0/3:20:60:60,90,200,90,200,200,0,100,100,80\t"
        "0/0:20:30:0,30,300,30,300,300,30,300,300,300\n",
    "a REF of differing length with ALT padding":
        f"ctgA\t70\t.\tATCC\tACC,GTCC,A\t125.79\t.\tAC=1,1,2;AF=0.167,0.167,0.333;AN=6;DP=60\t{_S}\t"
        "0/1:20:60:60,0,80,90,100,200,90,100,200,200\t0/2:20:60:60,90,200,0,100,80,90,200,100,200\t"
        "3/3:20:30:120,130,210,130,210,210,30,40,40,0\n",
    "a seventh ALT cut":
        "ctgA\t80\t.\tA\tAC,ACC,ACCC,ACCCC,ACCCCC,ACCCCCC\t177.73\t.\tAC=2,1,1,1,1,1;AF=0.125,0.062,0.062,0.062,0.062,0.062;AN=16;"
        f"DP=160\t{_S}\t"
        "0/1:20:60:60,0,80,90,100,200,90,100,200,200,90,100,200,200,200,90,100,200,200,200,200,90,100,200,200,200,200,200\t"
        "0/1:20:60:60,0,80,90,100,200,90,100,200,200,90,100,200,200,200,90,100,200,200,200,200,90,100,200,200,200,200,200\t"
        "0/2:20:60:60,90,200,0,100,80,90,200,100,200,90,200,100,200,200,90,200,100,200,200,200,90,200,100,200,200,200,200\t"
        "0/3:20:60:60,90,200,90,200,200,0,100,100,80,90,200,200,100,200,90,200,200,100,200,200,90,200,200,100,200,200,200\t"
        "0/4:20:60:60,90,200,90,200,200,90,200,200,200,0,100,100,100,80,90,200,200,200,100,200,90,200,200,200,100,200,200\t"
        "0/5:20:60:60,90,200,90,200,200,90,200,200,200,90,200,200,200,200,0,100,100,100,100,80,90,200,200,200,200,100,200\t"
        "0/6:20:60:60,90,200,90,200,200,90,200,200,200,90,200,200,200,200,90,200,200,200,200,200,0,100,100,100,100,100,80\t"
        "0/0:20:10:0,10,90,10,90,90,10,90,90,90,10,90,90,90,90,10,90,90,90,90,90,10,90,90,90,90,90,90\n",
    "an ALT dropped by mle = 0": f"ctgA\t90\t.\tA\tC\t82.25\t.\tAC=2;AF=0.500;AN=4;DP=40\t{_S}\t1/1:{_HOM3}\t0/0:20:3:0,3,40\n",
    "all samples hom-alt":
        f"ctgA\t100\t.\tG\tT\t440.99\t.\tAC=8;AF=1.00;AN=8;DP=46\t{_S}\t1/1:10:30:120,30,0\t1/1:11:30:120,30,0\t1/1:12:30:120,30,0\t"
        "1/1:13:30:120,30,0\n",
    "equal PLs": f"ctgA\t110\t.\tA\tC\t30.02\t.\tAC=1;AF=0.500;AN=2;DP=40\t{_S}\t0/1:{_HET3}\t./.\t./.\n",
    "ties in GT": f"ctgA\t120\t.\tA\tC\t50.36\t.\tAC=1;AF=0.250;AN=4;DP=40\t{_S}\t0/0:20:0:0,0,50\t0/1:20:0:80,0,0\n",
    "a PL at the clamp":
        f"ctgA\t130\t.\tA\tC\t1048542.00\t.\tAC=1;AF=0.250;AN=4;DP=40\t{_S}\t0/1:20:99:1048575,0,1048575\t0/0:20:99:0,1048575,1048575\n",
    "a site below the threshold": f"ctgA\t150\t.\tA\tG\t27.01\t.\tAC=1;AF=0.250;AN=4;DP=40\t{_S}\t0/1:{_HET3}\t0/0:20:30:0,30,300\n",
}


def hand_cases():
    """{name: (GVCF records per sample {sample: {contig: [...]}}, options, expected record lines)}.  Expected lines
    are written out; test_joint_cpu asserts that the restatement, the host path and the command all give them."""
    c = {}
    c["one sample"] = ({"s1": {"ctgA": [block(1, 9), call(10, "A", "G", HET, dp=21), block(11, 50)]}}, {}, None)
    three = {"s1": {"ctgA": [block(1, 19), call(20, "C", "T", HOM, dp=30, gt="1/1"), block(21, 60)]},
             "s2": {"ctgA": [block(1, 60, pl=(0, 45, 450), dp=15)]},
             "s3": {"ctgA": [block(1, 60, pl=(0, 33, 330), dp=11)]}}
    c["a site carried by one of three samples"] = (three, {}, None)
    c["a block ending at p - 1, at p and at p + 1"] = (
        {"s1": {"ctgA": [call(30, "G", "A", HET)]},
         "s2": {"ctgA": [block(1, 29)]}, "s3": {"ctgA": [block(1, 30)]}, "s4": {"ctgA": [block(1, 31)]}}, {}, None)
    c["a no-call from no coverage"] = ({"s1": {"ctgA": [call(40, "T", "C", HET)]}, "s2": {"ctgA": [block(50, 90)]},
                                        "s3": {"ctgB": [block(1, 100)]}}, {}, None)
    c["a no-call inside a deletion's span"] = (
        {"s1": {"ctgA": [call(52, "A", "T", HOM, gt="1/1")]},
         "s2": {"ctgA": [block(1, 49), call(50, "GTAC", "G", HET), block(54, 80)]}}, {}, None)
    c["two ALTs at one POS"] = ({"s1": {"ctgA": [call(60, "A", "C", HET)]}, "s2": {"ctgA": [call(60, "A", "T", HOM, gt="1/1")]},
                                 "s3": {"ctgA": [call(60, "A", "T", HET)]}}, {}, None)
    c["three ALTs at one POS"] = ({"s1": {"ctgA": [call(61, "A", "C", HET)]}, "s2": {"ctgA": [call(61, "A", "T", HOM, gt="1/1")]},
                                   "s3": {"ctgA": [call(61, "A", "G", HET)]}, "s4": {"ctgA": [block(1, 100)]}}, {}, None)
    c["a REF of differing length with ALT padding"] = (
        {"s1": {"ctgA": [call(70, "AT", "A", HET)]}, "s2": {"ctgA": [call(70, "A", "G", HET)]},
         "s3": {"ctgA": [call(70, "ATCC", "A", HOM, gt="1/1")]}}, {}, None)
    c["a seventh ALT cut"] = ({f"s{k}": {"ctgA": [call(80, "A", "A" + "C" * k, HET if k != 7 else HOM)]} for k in range(1, 8)}
                              | {"s0": {"ctgA": [call(80, "A", "AC", HET)]}}, {}, None)
    c["an ALT dropped by mle = 0"] = ({"s1": {"ctgA": [call(90, "A", "C", HOM, gt="1/1")]},
                                       "s2": {"ctgA": [call(90, "A", "T", (0, 3, 40, 3, 43, 40))]}}, {}, None)
    c["all samples hom-alt"] = ({f"s{k}": {"ctgA": [call(100, "G", "T", HOM, gt="1/1", dp=10 + k)]} for k in range(4)}, {}, None)
    c["equal PLs"] = ({"s1": {"ctgA": [call(110, "A", "C", HET)]}, "s2": {"ctgA": [block(100, 120, pl=(0, 0, 0), dp=0)]},
                       "s3": {"ctgA": [call(110, "A", "C", (7, 7, 7, 7, 7, 7))]}}, {}, None)
    c["ties in GT"] = ({"s1": {"ctgA": [call(120, "A", "C", (0, 0, 50, 60, 60, 90))]},
                        "s2": {"ctgA": [call(120, "A", "C", (80, 0, 0, 90, 90, 120))]}}, {"conf": 4.5}, None)
    c["a PL at the clamp"] = ({"s1": {"ctgA": [call(130, "A", "C", (2000000, 0, 1048575, 1048576, 3000000, 99999999))]},
                               "s2": {"ctgA": [block(1, 200, pl=(0, 1048575, 5000000))]}}, {}, None)
    c["a site below the threshold"] = ({"s1": {"ctgA": [call(140, "A", "C", (36, 0, 60, 40, 70, 90)), call(150, "A", "G", HET)]},
                                        "s2": {"ctgA": [block(1, 200)]}}, {}, None)
    assert set(c) == set(EXPECTED)
    return {name: (samples, opts, EXPECTED[name]) for name, (samples, opts, _) in c.items()}


def case_texts(case):
    samples, opts, want = case
    return [gvcf_text(name, CONTIGS, recs) for name, recs in samples.items()], opts, want


def case_arrays(case):
    """(cohort arrays, pos, n_alt) of a hand case's contig ctgA, and its options."""
    texts, opts, _ = case_texts(case)
    parsed = sorted((parse_gvcf(t) for t in texts), key=lambda p: p[0])
    cohort, pos, n_alt, _, _ = combine([p[2].get("ctgA", []) for p in parsed])
    return cohort, pos, n_alt, opts


def flat_prior_case():
    """Ties in mle need equal posts, which no PL gives under the priors: a flat LP and PLs (50, 0, 0) tie k = 1 and 2;
    PLs (0, 0, 0) tie all three.  (cohort arrays, pos, n_alt, tables)."""
    cohort = (np.array([0, 1, 2]), np.array([5, 9]), np.array([6, 10]), np.array([1, 1]), np.array([1, 1]), np.array([7, 8]),
              np.array([[50, 0, 0, 90, 90, 90], [0, 0, 0, 0, 0, 0]]))
    S, LG, _ = tables(1e-3, 2)
    return cohort, np.array([5, 9]), np.array([1, 1]), (S, LG, np.zeros(5, np.int64))


# ------------------------------------------------------------------ cohort builders (the integer level)
def random_cohort(seed, n_samples, n_sites, max_alt=3, span=None, base=0, no_call=0.25):
    """(cohort arrays, pos, n_alt): random records and sites over [base, base + span): blocks and calls with
    random ALT indices, equal begs, overlaps, gaps, ties and PLs at the clamp."""
    rng = np.random.default_rng(seed)
    span = span or max(4 * n_sites, 64)
    pos = base + np.sort(rng.choice(span, n_sites, replace=False)).astype(np.int64)
    n_alt = rng.integers(1, max_alt + 1, n_sites).astype(np.uint8)
    beg, end, kind, alt, dp, pl, rec_off = [], [], [], [], [], [], [0]
    for s in range(n_samples):
        # a record at most sites (so that sources exist), some off them
        at = pos[rng.random(n_sites) >= no_call] if n_sites else pos
        extra = base + rng.integers(0, span, max(n_sites // 4, 1))
        b = np.sort(np.concatenate([at, extra, at[: len(at) // 8]]))  # with equal begs
        m = len(b)
        k = (rng.random(m) < 0.6).astype(np.uint8)
        length = np.where(k == CALL, rng.integers(1, 4, m), rng.integers(1, 12, m))
        a = np.where(k == CALL, rng.integers(0, max_alt + 1, m), 0).astype(np.uint8)
        p = rng.integers(0, 400, (m, 6)).astype(np.int32)
        truth = rng.integers(0, 3, m)
        p[np.arange(m), np.where(k == CALL, truth, 0)] = 0
        p[rng.random((m, 6)) < 0.05] = 0
        p[rng.random((m, 6)) < 0.01] = PL_MAX
        flat = rng.random(m) < 0.03
        p[flat] = p[flat, :1]
        beg.append(b), end.append(np.minimum(b + length, 2**31 - 1)), kind.append(k), alt.append(a)
        dp.append(rng.integers(0, 60, m)), pl.append(p)
        rec_off.append(rec_off[-1] + m)
    cat = lambda v, t: np.concatenate(v).astype(t) if v else np.zeros(0, t)  # noqa: E731
    cohort = (np.array(rec_off, np.int64), cat(beg, np.int32), cat(end, np.int32), cat(kind, np.uint8), cat(alt, np.uint8),
              cat(dp, np.int32), np.concatenate(pl).astype(np.int32).reshape(-1, 6))
    return cohort, pos.astype(np.int32), n_alt


def random_gvcfs(seed, n_samples, contigs=CONTIGS, refs=None, sites_per_contig=40):
    """GVCF texts of n_samples samples in htc's dialect: blocks, gaps, calls that share positions and ALTs."""
    rng = np.random.default_rng(seed)
    letters = "ACGT"
    texts = []
    shared = {name: np.sort(rng.choice(np.arange(5, ln - 5), min(sites_per_contig, ln // 8), replace=False)) for name, ln in contigs}
    site_alts = {name: [[letters[(k + 1 + int(j)) % 4] for j in rng.permutation(3)] for k in range(len(p))] for name, p in shared.items()}
    for s in range(n_samples):
        recs = {}
        for name, ln in contigs:
            out, at = [], 1
            for k, p in enumerate(shared[name]):
                p = int(p)
                if p < at:
                    continue
                u = rng.random()
                if u < 0.15:          # no coverage up to the site
                    at = p + 1
                    continue
                if p > at and rng.random() < 0.9:   # a block up to p - 1 before a call, or over p
                    e = p - 1 if u < 0.6 else p + int(rng.integers(0, 3))
                    out.append(block(at, e, pl=(0, int(rng.integers(3, 90)), int(rng.integers(90, 900))),
                                     dp=int(rng.integers(1, 50)), ref=letters[p % 4]))
                    at = e + 1
                if u < 0.6:
                    ref = letters[k % 4] + ("" if rng.random() < 0.8 else "TG"[: int(rng.integers(1, 3))])
                    alt = site_alts[name][k][int(rng.integers(0, 3) if rng.random() < 0.3 else 0)]
                    if rng.random() < 0.1:
                        alt = alt + "AC"
                    pls = [int(v) for v in rng.integers(20, 500, 6)]
                    pls[int(rng.integers(1, 3))] = 0
                    if rng.random() < 0.2:
                        pls = [0, 2, 30, 5, 33, 60]
                    out.append(call(p, ref, alt, pls, dp=int(rng.integers(2, 60))))
                    at = p + len(ref)
            recs[name] = out
        texts.append(gvcf_text(f"smp{n_samples - s:03d}", contigs, recs))  # the column order is not the order given
    return texts
