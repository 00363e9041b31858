"""Pileup SNP genotyping (DESIGN §2 [EXT] "UnifiedGenotyper, SNP model", §4.12):
the Python restatement of the rules (the table, counted records and bases, the
window clip, a locus's integer sums, the site predicate, the genotype step and
the VCF text), builders of batches, and the hand cases with their expected
sites written out.

A record is a dict: flag, ref (contig index), pos (0-based), mapq, cigar (text),
seq (read letters), qual (list of phred values, or None: absent), n_bases.  A
reference is a list of contig strings.  A window is (ref, start, len).  A site
is a dict: offset, ref and alt (letter codes), n[4], qsum[4], n_del, mq2, gl[3].
"""
import math
import random

import depth_cases as D
from depth_cases import DUPLICATE, QCFAIL, REVERSE, SECONDARY, SUPPLEMENTARY, UNMAPPED, Refused, parse_cigar, read_len, ref_len

FILTER = UNMAPPED | SECONDARY | QCFAIL | DUPLICATE
LETTERS = "ACGT"
MAXQ = 93
TILE = 256
OPS = D.OPS
STATUS_FIELD, STATUS_REF, STATUS_ORDER, STATUS_SITES = 1, 2, 4, 8


def code(ch):
    return LETTERS.find(ch.upper()) if ch.upper() in LETTERS else 4


# ------------------------------------------------------------------ the rules
def table_reals(pcr_error=1e-4):
    """log10(p_c) * 2^32 for q = 0 .. 93, c = 0, 1, 2, in double, before rounding."""
    out = []
    for q in range(MAXQ + 1):
        e = 10.0 ** (-q / 10.0)
        same = (1.0 - pcr_error) * (1.0 - e) + pcr_error * e / 3.0
        diff = (1.0 - pcr_error) * e / 3.0 + (pcr_error / 3.0) * (1.0 - e) + 2.0 * (pcr_error / 3.0) * (e / 3.0)
        out.append([math.log10(p) * 4294967296.0 for p in (same, 0.5 * same + 0.5 * diff, diff)])
    return out


def table(pcr_error=1e-4):
    """T[94][3]: llround of table_reals (half away from zero)."""
    return [[int(math.copysign(math.floor(abs(x) + 0.5), x)) for x in row] for row in table_reals(pcr_error)]


def counted(r):
    return r["ref"] >= 0 and bool(parse_cigar(r["cigar"])) and not r["flag"] & FILTER and r["mapq"] != 255


def sites(records, window, refseq, tab, min_baseq=17):
    """(sites of the window, a counted record has an aligned base beyond the contig).  refseq is the whole contig.
    Refused on a CIGAR that does not cover its record's bases and on positions that decrease."""
    ref, start, length = window
    clen = len(refseq)
    cells = {}
    beyond = False
    last = None
    for r in records:
        if r["ref"] != ref:
            continue
        if last is not None and r["pos"] < last:
            raise Refused("positions decrease")
        last = r["pos"]
        if not counted(r):
            continue
        if read_len(r["cigar"]) != r["n_bases"] or len(r["seq"]) != r["n_bases"] or (
                r["qual"] is not None and len(r["qual"]) != r["n_bases"]):
            raise Refused("the CIGAR does not cover the bases")
        p, i = r["pos"], 0
        mq = r["mapq"]
        for n, op in parse_cigar(r["cigar"]):
            if op in "M=X":
                if n and (p < 0 or p + n > clen):
                    beyond = True
                for j in range(n):
                    x = code(r["seq"][i + j])
                    qe = min(0 if r["qual"] is None else r["qual"][i + j], mq, MAXQ)
                    if x < 4 and qe >= min_baseq and 0 <= p + j < clen and start <= p + j < start + length:
                        c = cells.setdefault(p + j - start, new_cell())
                        c["n"][x] += 1
                        c["qsum"][x] += qe
                        c["mq2"] += mq * mq
                        for k, name in enumerate("ABC"):
                            c[name][x] += tab[qe][k]
                p += n
                i += n
            elif op in "IS":
                i += n
            elif op == "D":
                if min(mq, MAXQ) >= min_baseq:
                    for j in range(n):
                        if 0 <= p + j < clen and start <= p + j < start + length:
                            cells.setdefault(p + j - start, new_cell())["n_del"] += 1
                p += n
            elif op == "N":
                p += n
    out = []
    for off in sorted(cells):
        c = cells[off]
        rc = code(refseq[start + off])
        if rc > 3 or not any(c["n"][x] for x in range(4) if x != rc):
            continue
        alt = max((x for x in range(4) if x != rc), key=lambda x: (c["qsum"][x], -x))
        A, B, Cc = c["A"], c["B"], c["C"]
        gl = [A[rc] + sum(Cc[x] for x in range(4) if x != rc),
              B[rc] + B[alt] + sum(Cc[x] for x in range(4) if x not in (rc, alt)),
              A[alt] + sum(Cc[x] for x in range(4) if x != alt)]
        out.append(dict(offset=off, ref=rc, alt=alt, n=list(c["n"]), qsum=list(c["qsum"]), n_del=c["n_del"], mq2=c["mq2"], gl=gl))
    return out, beyond


def new_cell():
    return dict(n=[0] * 4, qsum=[0] * 4, n_del=0, mq2=0, A=[0] * 4, B=[0] * 4, C=[0] * 4)


def log10_add(a, b):
    m = max(a, b)
    if m == -math.inf:
        return m
    return m + math.log10(10.0 ** (a - m) + 10.0 ** (b - m))


def genotype(s, heterozygosity=1e-3, stand_call_conf=10.0, max_deletion_fraction=0.05, margin=None):
    """The call of a site as dict(gt, qual, pl, gq, ad, dp, mq, ac, af), or None.  margin: assert that a QUAL that decides
    the call lies at least that far from stand_call_conf."""
    depth = sum(s["n"])
    if s["n_del"] > max_deletion_fraction * (depth + s["n_del"]):
        return None
    prior = [math.log10(1.0 - 1.5 * heterozygosity), math.log10(heterozygosity), math.log10(heterozygosity / 2.0)]
    post = [float(s["gl"][k]) * (1.0 / 4294967296.0) + prior[k] for k in range(3)]
    norm = -math.inf
    for k in range(3):
        norm = log10_add(norm, post[k])
    qual = min(-10.0 * (post[0] - norm), 9999.0)
    gt = max(range(3), key=lambda k: (s["gl"][k], -k))
    if gt == 0:
        return None
    if margin is not None:
        assert abs(qual - stand_call_conf) >= margin, (s, qual)
    if qual < stand_call_conf:
        return None
    pl = [(10 * (s["gl"][gt] - s["gl"][k]) + (1 << 31)) >> 32 for k in range(3)]
    return dict(gt=gt, qual=qual, pl=pl, gq=min(99, sorted(pl)[1]), ad=[s["n"][s["ref"]], s["n"][s["alt"]]], dp=depth,
                mq="%.2f" % math.sqrt(s["mq2"] / depth), ac=gt, af="0.500" if gt == 1 else "1.00")


def vcf_line(s, g, chrom, window_start):
    return (f"{chrom}\t{window_start + s['offset'] + 1}\t.\t{LETTERS[s['ref']]}\t{LETTERS[s['alt']]}\t{g['qual']:.2f}\tPASS\t"
            f"AC={g['ac']};AF={g['af']};AN=2;DP={g['dp']};MQ={g['mq']}\tGT:AD:DP:GQ:PL\t"
            f"{'0/1' if g['gt'] == 1 else '1/1'}:{g['ad'][0]},{g['ad'][1]}:{g['dp']}:{g['gq']}:{g['pl'][0]},{g['pl'][1]},{g['pl'][2]}\n")


def vcf_text(site_list, chrom, window_start=0, margin=None, **kw):
    """The record lines of the calls among site_list."""
    out = []
    for s in site_list:
        g = genotype(s, margin=margin, **kw)
        if g is not None:
            out.append(vcf_line(s, g, chrom, window_start))
    return "".join(out)


def vcf_header(sample, names, lengths):
    meta = ['##INFO=<ID=AC,Number=A,Type=Integer,Description="Allele count in genotypes">',
            '##INFO=<ID=AF,Number=A,Type=Float,Description="Allele frequency">',
            '##INFO=<ID=AN,Number=1,Type=Integer,Description="Total number of alleles in called genotypes">',
            '##INFO=<ID=DP,Number=1,Type=Integer,Description="Counted bases at the locus">',
            '##INFO=<ID=MQ,Number=1,Type=Float,Description="RMS mapping quality of the counted bases">',
            '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
            '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Counted bases of the ref and alt letters">',
            '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Counted bases">',
            '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality">',
            '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods">',
            '##FILTER=<ID=PASS,Description="All filters passed">']
    return ("##fileformat=VCFv4.2\n##source=fcs-genome ug (pileup SNP model)\n" + "".join(m + "\n" for m in meta) +
            "".join(f"##contig=<ID={n},length={k}>\n" for n, k in zip(names, lengths)) +
            f"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t{sample}\n")


def same_vcf(got, want, tol=0.011):
    """The two texts' record lines agree: every field exactly but QUAL, which agrees as a number within tol."""
    g, w = [ln.split("\t") for ln in got.splitlines()], [ln.split("\t") for ln in want.splitlines()]
    if len(g) != len(w):
        return False
    for a, b in zip(g, w):
        if a[:5] != b[:5] or a[6:] != b[6:] or abs(float(a[5]) - float(b[5])) > tol:
            return False
    return True


def command_vcf(refs, names, sample, records, intervals=None, margin=0.05, **kw):
    """The whole VCF the command writes for sorted records: intervals are merged (ref, start, end), default every contig."""
    tab = table(kw.pop("pcr_error", 1e-4))
    min_baseq = kw.pop("min_baseq", 17)
    body = []
    for c, seq in enumerate(refs):
        all_sites, _ = sites(records, (c, 0, len(seq)), seq, tab, min_baseq)
        spans = [(0, len(seq))] if intervals is None else [(s, e) for r, s, e in intervals if r == c]
        keep = [s for s in all_sites if any(a <= s["offset"] < b for a, b in spans)]
        body.append(vcf_text(keep, names[c], margin=margin, **kw))
    return vcf_header(sample, names, [len(s) for s in refs]) + "".join(body)


# ------------------------------------------------------------------ records and the flat batch
def other(ch, k=1):
    """A letter that differs from the reference letter ch (N counts as A)."""
    return LETTERS[(max(code(ch), 0) % 4 + k) % 4] if code(ch) < 4 else LETTERS[k % 4]


def read_of(refseq, pos, cigar, subs=None):
    """The read that the CIGAR copies from the reference (upper case; I and S bases are A; reference N is read as A),
    with subs {read index: letter}."""
    out, p = [], pos
    for n, op in parse_cigar(cigar):
        if op in "M=X":
            for j in range(n):
                ch = refseq[p + j].upper() if 0 <= p + j < len(refseq) else "A"
                out.append(ch if ch in LETTERS else "A")
            p += n
        elif op in "IS":
            out += ["A"] * n
        elif op in "DN":
            p += n
    for i, ch in (subs or {}).items():
        out[i] = ch
    return "".join(out)


def rec(flag, ref, pos, cigar, seq, qual=30, mapq=60):
    n = read_len(cigar)
    if isinstance(qual, int):
        qual = [qual] * n
    return dict(flag=flag, ref=ref, pos=pos, mapq=mapq, cigar=cigar, seq=seq, qual=None if qual is None else list(qual), n_bases=n)


def flatten(records, first_offset=0):
    """(flag, ref_id, pos, mapq, cigar, cigar_off, bases, qual, base_off, qual_absent): fcsug_batch's arrays; the base
    and quality bytes start at first_offset (the bytes before them are 0xEE)."""
    cigar, cigar_off, qual, bases, base_off = [], [0], [0xEE] * first_offset, [0xEE] * first_offset, [first_offset]
    for r in records:
        cigar += [(n << 4) | OPS.index(op) for n, op in parse_cigar(r["cigar"])]
        cigar_off.append(len(cigar))
        qual += [0xFF] * r["n_bases"] if r["qual"] is None else r["qual"]
        bases += list(r["seq"].encode())
        base_off.append(len(qual))
    return ([r["flag"] for r in records], [r["ref"] for r in records], [r["pos"] for r in records],
            [r["mapq"] for r in records], cigar, cigar_off, bases, qual, base_off, [int(r["qual"] is None) for r in records])


# ------------------------------------------------------------------ the hand cases
def hand_refs():
    """Contig 0: 1,200 loci of ACGT repeating (locus p holds ACGT[p % 4]) with N at 600 .. 609 and lower case at
    700 .. 719; contig 1: 40 loci of the same pattern."""
    s = [LETTERS[p % 4] for p in range(1200)]
    s[600:610] = "N" * 10
    s[700:720] = [ch.lower() for ch in s[700:720]]
    return ["".join(s), "".join(LETTERS[p % 4] for p in range(40))]


def hand_cases():
    """[dict(name, records, window, want, beyond)]: want is [(offset, ref letter, alt letter, n per letter, n_del)] of
    every site of the window, in order."""
    refs = hand_refs()
    R0, R1 = refs
    whole0, whole1 = (0, 0, 1200), (1, 0, 40)

    def read(pos, cigar, subs=None, qual=30, mapq=60, flag=0, contig=0):
        """subs: {reference position: letter} of aligned bases, turned into read indices."""
        seq = list(read_of(refs[contig], pos, cigar))
        p, i = pos, 0
        at = {}
        for n, op in parse_cigar(cigar):
            if op in "M=X":
                for j in range(n):
                    at[p + j] = i + j
                p, i = p + n, i + n
            elif op in "IS":
                i += n
            elif op in "DN":
                p += n
        quals = [qual] * len(seq) if isinstance(qual, int) else qual
        for where, ch in (subs or {}).items():
            seq[at[where]] = ch
        return rec(flag, contig, pos, cigar, "".join(seq), quals, mapq)

    def case(name, records, want, window=whole0, beyond=False):
        return dict(name=name, records=records, window=window, want=want, beyond=beyond)

    def n_of(**kw):
        return [kw.get(ch, 0) for ch in LETTERS]

    q16 = [30, 30, 16, 30]
    q17 = [30, 30, 17, 30]
    return [
        # p % 4: 0 A, 1 C, 2 G, 3 T
        case("match_only", [read(10, "10M")], []),
        case("one_mismatch", [read(10, "10M", {12: "C"})], [(12, "A", "C", n_of(C=1), 0)]),
        case("qe_16_and_17", [read(8, "4M", {10: "T"}, q16), read(18, "4M", {20: "G"}, q17)], [(20, "A", "G", n_of(G=1), 0)]),
        case("quality_capped_by_mapq", [read(8, "4M", {10: "T"}, 30, mapq=16), read(18, "4M", {20: "G"}, 40, mapq=20)],
             [(20, "A", "G", n_of(G=1), 0)]),
        case("mapq_255", [read(8, "4M", {10: "T"}, mapq=255)], []),
        case("mapq_0_deletions", [read(8, "4M2D4M", mapq=0), read(8, "4M2D4M"), read(10, "8M", {12: "C", 13: "G"})],
             [(12, "A", "C", n_of(C=1), 1), (13, "C", "G", n_of(G=1), 1)]),
        case("equal_qsum_smaller_letter_wins", [read(10, "4M", {12: "G"}), read(10, "4M", {12: "C"}), read(11, "4M", {13: "T"}),
                                               read(11, "4M", {13: "A"})],
             [(12, "A", "C", n_of(A=2, C=1, G=1), 0), (13, "C", "A", n_of(C=2, A=1, T=1), 0)]),
        case("larger_qsum_wins_over_count", [read(10, "4M", {12: "C"}, 17), read(10, "4M", {12: "C"}, 17), read(10, "4M", {12: "T"}, 40)],
             [(12, "A", "T", n_of(C=2, T=1), 0)]),
        case("reference_n", [read(596, "20M", {598: "A", 604: "C", 611: "A"})],
             [(598, "G", "A", n_of(A=1), 0), (611, "T", "A", n_of(A=1), 0)]),
        case("lower_case_reference", [read(698, "12M", {705: "G"}), read(698, "12M")], [(705, "C", "G", n_of(C=1, G=1), 0)]),
        case("read_n_and_lower_case_read", [read(10, "4M", {12: "N"}), read(10, "4M", {12: "c", 13: "N"}), read(10, "4M", {11: "t"})],
             [(12, "A", "C", n_of(C=1, A=1), 0)]),
        case("only_s_and_i", [rec(0, 0, 10, "3S2I", "CCCCC")], []),
        case("ops_i_s_h_p_n_add_nothing", [read(10, "2H3S4M2I1P4M20N4M3S", {12: "C", 40: "G"})],
             [(12, "A", "C", n_of(C=1), 0), (40, "A", "G", n_of(G=1), 0)]),
        case("eq_and_x", [read(10, "4=1X4=", {14: "T"})], [(14, "G", "T", n_of(T=1), 0)]),
        case("flags", [read(8, "8M", {10: "T"}, flag=UNMAPPED), read(9, "8M", {10: "T"}, flag=SECONDARY),
                       read(10, "8M", {10: "T"}, flag=QCFAIL), read(11, "8M", {12: "T"}, flag=DUPLICATE),
                       read(12, "8M", {14: "T"}, flag=SUPPLEMENTARY), read(13, "8M", {15: "A"}, flag=REVERSE | 0x1 | 0x40)],
             [(14, "G", "T", n_of(T=1, G=1), 0), (15, "T", "A", n_of(A=1, T=1), 0)]),
        case("d_at_a_tile_edge", [read(250, "4M4D4M"), read(252, "8M", {255: "A", 256: "C"})],
             [(255, "T", "A", n_of(A=1), 1), (256, "A", "C", n_of(C=1), 1)]),
        case("two_tiles", [read(200, "100M", {210: "A", 280: "C"})], [(210, "G", "A", n_of(A=1), 0), (280, "A", "C", n_of(C=1), 0)]),
        case("three_tiles_through_a_skip", [read(230, "50M560N50M", {240: "C", 850: "A"})],
             [(240, "A", "C", n_of(C=1), 0), (850, "G", "A", n_of(A=1), 0)]),
        case("window_clip", [read(90, "30M", {95: "A", 100: "C", 109: "G", 110: "A"})],
             [(0, "A", "C", n_of(C=1), 0), (9, "C", "G", n_of(G=1), 0)], window=(0, 100, 10)),
        case("other_contig_and_no_cigar", [rec(0, 0, 10, "", ""), read(10, "4M", {12: "C"}, contig=1)], []),
        case("ends_at_contig_end", [read(30, "10M", {39: "A"}, contig=1)], [(39, "T", "A", n_of(A=1), 0)], window=whole1),
        case("ends_one_past_contig_end", [read(31, "10M", {31: "A"}, contig=1)], [(31, "T", "A", n_of(A=1), 0)], window=whole1,
             beyond=True),
    ]


def want_sites(case):
    """The case's expected sites as the comparable part of the restatement's dicts."""
    return [dict(offset=o, ref=code(r), alt=code(a), n=n, n_del=d) for o, r, a, n, d in case["want"]]


def brief(site_list):
    return [dict(offset=int(s["offset"]), ref=int(s["ref"]), alt=int(s["alt"]), n=[int(v) for v in s["n"]], n_del=int(s["n_del"]))
            for s in site_list]


def full(site_list):
    """Every field of sites (restatement dicts or UG_SITE rows) as plain integers."""
    return [dict(offset=int(s["offset"]), ref=int(s["ref"]), alt=int(s["alt"]), n=[int(v) for v in s["n"]],
                 qsum=[int(v) for v in s["qsum"]], n_del=int(s["n_del"]), mq2=int(s["mq2"]), gl=[int(v) for v in s["gl"]])
            for s in site_list]


# ------------------------------------------------------------------ generators
def random_world(seed=7):
    """Three contigs of at most 9,000 loci with runs of N and lower-case stretches."""
    rng = random.Random(seed)
    refs = []
    for length in (9000, 7000, 4096):
        s = [rng.choice(LETTERS) for _ in range(length)]
        for _ in range(3):
            a, k = rng.randrange(0, length - 200), rng.randrange(1, 150)
            s[a:a + k] = ("n" if rng.random() < 0.3 else "N") * k
        for _ in range(3):
            a, k = rng.randrange(0, length - 400), rng.randrange(50, 300)
            s[a:a + k] = [ch.lower() for ch in s[a:a + k]]
        refs.append("".join(s))
    return refs


def planted(refs, seed):
    """Two haplotypes of the reference: 25 SNPs per contig, every third on both (a 1/1 call), the others on one."""
    rng = random.Random(seed + 1000)
    haps = [[list(s) for s in refs], [list(s) for s in refs]]
    for c, s in enumerate(refs):
        for k in range(25):
            p = rng.randrange(len(s))
            alt = other(s[p], 1 + rng.randrange(3))
            haps[0][c][p] = alt
            if k % 3 == 0:
                haps[1][c][p] = alt
    return [["".join(s) for s in h] for h in haps]


def random_batch(refs, seed=11, n=2000, mismatch=0.02):
    """About n records of 1-200 bases with mixed CIGARs (M, I, D, N, S, H, P, =, X), flags, MAPQ 0 to 60 and 255,
    qualities 2 to 41, absent qualities and N bases, inside their contigs, sorted by contig and position; the reads come
    from two haplotypes with planted SNPs."""
    rng = random.Random(seed)
    haps = planted(refs, seed)
    out = []
    while len(out) < n:
        L = rng.randrange(1, 201)
        cigar = D.random_cigar(rng, L)
        ref = rng.randrange(len(refs))
        span = ref_len(cigar)
        if span > len(refs[ref]):
            continue
        pos = rng.randrange(0, len(refs[ref]) - span + 1)
        flag = rng.choice([0, 0, 0, REVERSE, 0x1 | 0x40, 0x1 | 0x80 | REVERSE, SUPPLEMENTARY, DUPLICATE, SECONDARY, QCFAIL, UNMAPPED])
        qual = None if rng.random() < 0.03 else [rng.randrange(2, 42) for _ in range(L)]
        seq = list(read_of(haps[rng.randrange(2)][ref], pos, cigar))
        for i in range(L):
            u = rng.random()
            if u < mismatch:
                seq[i] = rng.choice(LETTERS)
            elif u < mismatch + 0.005:
                seq[i] = "N"
            elif u < mismatch + 0.01:
                seq[i] = seq[i].lower()
        out.append(rec(flag, ref, pos, cigar, "".join(seq), qual, mapq=rng.choice([0, 1, 16, 17, 20, 29, 30, 60, 60, 255])))
    out.sort(key=lambda r: (r["ref"], r["pos"]))
    return out


def sweep_batch(refs, seed=3):
    """Records of 1 .. 200 bases, sorted, so that their bytes start at every 4-byte residue; every fifth base differs."""
    rng = random.Random(seed)
    out = []
    for L in range(1, 201):
        pos = rng.randrange(0, len(refs[0]) - L)
        seq = list(read_of(refs[0], pos, f"{L}M"))
        for i in range(0, L, 5):
            seq[i] = other(seq[i], 1 + i % 3)
        out.append(rec(0, 0, pos, f"{L}M", "".join(seq), [rng.randrange(2, 42) for _ in range(L)]))
    out.sort(key=lambda r: r["pos"])
    return out
