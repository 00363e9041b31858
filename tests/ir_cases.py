"""Indel realignment restated in numpy / plain Python (DESIGN §2 [EXT]
"RealignerTargetCreator and IndelRealigner, round 22"): the base codes, S, the
argmin order and the candidate set, the targets, left alignment and clean(bin),
with hand cases and seeded random bins.  Nothing here calls the library; the
tests compare the library with this file.

A CIGAR is a list of (length, op letter).  A read is a dict: start (on the
contig), cigar (without clips), codes, quals, dup.  A known indel is (pos, k,
ins, codes): a deletion of [pos, pos + k) or an insertion before pos.
"""
import numpy as np

READ_MAX, SEQ_MAX, OVERHANG, ORIG_MAX, TARGET_MAX, PAD = 512, 4096, 99, 1 << 30, 500, 30
OPS = "MIDNSHP=X"


def code(b):
    return "ACGT".find(chr(b).upper()) if chr(b).upper() in "ACGT" else 4


def codes(text):
    return np.array([code(b) for b in text.encode()], np.uint8)


def differ(a, b):
    return a < 4 and b < 4 and a != b


def S(rc, rq, s, o):
    """S(r, s, o) base by base."""
    total = 0
    for i in range(len(rc)):
        if o + i >= len(s):
            total += OVERHANG
        elif differ(int(rc[i]), int(s[o + i])):
            total += int(rq[i])
    return total


def best(rc, rq, s, orig):
    """(score, offset) of best(c, r): the smallest S; among equals orig, then the smallest offset."""
    rc, rq, s = np.asarray(rc, np.int64), np.asarray(rq, np.int64), np.asarray(s, np.int64)
    L, n = len(rc), len(s)
    top = (S(rc, rq, s, orig), 0, orig)
    if n >= L:
        w = np.lib.stride_tricks.sliding_window_view(s, L)
        sc = (((w < 4) & (rc < 4) & (w != rc)) * rq).sum(1)
        o = int(np.argmin(sc))   # the first of the smallest
        top = min(top, (int(sc[o]), 1, o))
    return top[0], top[2]


def pack(cigar):
    return [(n << 4) | OPS.index(op) for n, op in cigar]


def unpack(words):
    return [(int(w) >> 4, OPS[int(w) & 15]) for w in words]


def text(cigar):
    return "".join(f"{n}{op}" for n, op in cigar)


# ------------------------------------------------------------------ targets
def cigar_events(pos, cigar):
    out, p = [], pos
    for n, op in cigar:
        if op == "I":
            out.append((max(p - 1, 0), p + 1))
        elif op == "D":
            out.append((max(p - 1, 0), p + n))
            p += n
        elif op in "M=XN":
            p += n
    return out


def merge_targets(events):
    """events: (ref, start, end); merged when they overlap or abut; longer than 500 dropped."""
    out = []
    for ref, s, e in sorted(events):
        if out and out[-1][0] == ref and s <= out[-1][2]:
            out[-1][2] = max(out[-1][2], e)
        else:
            out.append([ref, s, e])
    return [tuple(t) for t in out if t[2] - t[1] <= TARGET_MAX]


def target_text(chrom, start, end):
    return f"{chrom}:{start + 1}" + (f"-{end}" if end - start > 1 else "")


# ------------------------------------------------------------------ left alignment
def one_indel(cigar):
    """(a, k, ins) of aM kI bM / aM kD bM with = and X as M, else None."""
    runs = []
    for n, op in cigar:
        op = "M" if op in "M=X" else op
        if n == 0:
            continue
        if runs and runs[-1][1] == op == "M":
            runs[-1][0] += n
        else:
            runs.append([n, op])
    if len(runs) == 3 and runs[0][1] == "M" and runs[1][1] in "ID" and runs[2][1] == "M":
        return runs[0][0], runs[1][0], runs[1][1] == "I"
    return None


def left_align(ref, at, a, k, ins, bases=None):
    """The indel after ref[at + a - 1] moved left while a > 1 and the spelled sequence is the same: (a, bases)."""
    bases = None if bases is None else list(bases)
    while a > 1:
        p = at + a
        if ins:
            if ref[p - 1] != bases[-1]:
                break
            bases = [bases[-1]] + bases[:-1]
        elif ref[p - 1] != ref[p + k - 1]:
            break
        a -= 1
    return a, bases


# ------------------------------------------------------------------ clean(bin)
def columns(read, at, cigar):
    """[(read index, window column)] of the M bases, and the I + D lengths."""
    out, i, x, gaps = [], 0, at, 0
    for n, op in cigar:
        if op in "M=X":
            out += [(i + t, x + t) for t in range(n)]
            i, x = i + n, x + n
        elif op == "I":
            i, gaps = i + n, gaps + n
        elif op == "D":
            x, gaps = x + n, gaps + n
        elif op == "N":
            x += n
    return out, gaps


def along(read, at, cigar, ref):
    total = 0
    for i, x in columns(read, at, cigar)[0]:
        total += OVERHANG if x >= len(ref) else int(read["quals"][i]) if differ(int(read["codes"][i]), int(ref[x])) else 0
    return total


def consensus(ref, u, k, ins, bases):
    ref = list(ref)
    return ref[:u] + (list(bases) + ref[u:] if ins else ref[u + k:])


def restrict(lo, u, k, ins, o, L):
    """(start, cigar) of consensus columns [o, o + L), None without an M."""
    if not ins:
        start = lo + o if o < u else lo + o + k
        return (start, [(u - o, "M"), (k, "D"), (o + L - u, "M")]) if o < u < o + L else (start, [(L, "M")])
    kinds = ["I" if u <= col < u + k else "M" for col in range(o, o + L)]
    if "M" not in kinds:
        return None
    cigar = []
    for kind in kinds:
        if cigar and cigar[-1][1] == kind:
            cigar[-1][0] += 1
        else:
            cigar.append([1, kind])
    start = lo + o if o <= u else lo + u if o < u + k else lo + o - k
    return start, [tuple(c) for c in cigar]


def prepare(lo, ref, reads, known=(), max_reads=20000, max_cons=30):
    """(skip, cigars, alt, raw, aligner, total_raw, consensuses [(seq, u, k, ins)])."""
    W = len(ref)
    cigars = [list(r["cigar"]) for r in reads]
    if len(reads) > max_reads or W > SEQ_MAX:
        return True, cigars, [], [], [], 0, []
    alt, raw, aligner, total, proposed = [], [], [], 0, []
    for i, r in enumerate(reads):
        at = r["start"] - lo
        form = one_indel(r["cigar"])
        if form:
            a, k, ins = form
            m = sum(n for n, op in r["cigar"] if op in "M=X")
            bases = list(r["codes"][a:a + k]) if ins else None
            a2, bases = left_align(ref, at, a, k, ins, bases)
            if a2 != a:
                cigars[i] = [(a2, "M"), (k, "I" if ins else "D"), (m - a2, "M")]
        s = S(r["codes"], r["quals"], ref, at)
        if s == 0:
            continue
        alt.append(i), raw.append(s), aligner.append(along(r, at, cigars[i], ref))
        if not r["dup"]:
            total += s
        if form and (not ins or all(b < 4 for b in bases)):
            proposed.append((at + a2, k, ins, bases))
    cons, skip = [], False
    todo = []
    for pos, k, ins, bases in known:
        ev0, ev1 = pos - 1, pos if ins else pos + k
        if ev0 >= lo + 1 and ev1 <= lo + W - 1:
            a, b2 = left_align(ref, 0, pos - lo, k, ins, list(bases) if ins else None)
            todo.append((a, k, ins, b2))
    for u, k, ins, bases in todo + proposed:
        seq = consensus(ref, u, k, ins, bases)
        if len(cons) >= max_cons or any(c[0] == seq for c in cons):
            continue
        skip |= len(seq) > SEQ_MAX
        cons.append((seq, u, k, ins))
    return skip, cigars, alt, raw, aligner, total, cons


def clean(lo, ref, reads, known=(), max_reads=20000, max_cons=30, lod=50, scores=None):
    """The bin's updates [(read, start, cigar, nm)] and what led to them (a dict); scores(c, j) -> (best, off)
    stands in for the restatement's own best()."""
    skip, cigars, alt, raw, aligner, total, cons = prepare(lo, ref, reads, known, max_reads, max_cons)
    info = dict(skip=skip, cons=cons, alt=alt, raw=raw, aligner=aligner, total=total, pick=None, sums=[], refused=False, replaced=0, lod_failed=False)
    if skip or not cons or not alt:
        return [], info
    lists = []
    for c, (seq, u, k, ins) in enumerate(cons):
        total_c, listed = 0, []
        for j, i in enumerate(alt):
            r = reads[i]
            my, o = scores(c, j) if scores else best(r["codes"], r["quals"], np.array(seq), r["start"] - lo)
            if my > aligner[j] or my >= raw[j]:
                info["replaced"] += 1
                my = raw[j]
            else:
                listed.append((j, o))
            if not r["dup"]:
                total_c += my
        info["sums"].append(total_c), lists.append(listed)
    pick = info["sums"].index(min(info["sums"]))
    info["pick"] = pick
    if total - info["sums"][pick] < lod:
        info["lod_failed"] = True
        return [], info
    seq, u, k, ins = cons[pick]
    ups = {}
    for j, o in lists[pick]:
        r = reads[alt[j]]
        new = restrict(lo, u, k, ins, o, len(r["codes"]))
        if new is None or (new[0] == r["start"] and list(new[1]) == list(r["cigar"])):
            continue
        cols, gaps = columns(r, new[0] - lo, new[1])
        nm = gaps + sum(differ(int(r["codes"][i]), int(ref[x])) for i, x in cols if 0 <= x < len(ref))
        ups[j] = (alt[j], new[0], new[1], nm)
    W = len(ref)
    om, ot, cm, ct = (np.zeros(W, np.int64) for _ in range(4))
    for j, i in enumerate(alt):
        r = reads[i]
        if r["dup"] or any(op in "ID" for _, op in r["cigar"]):
            continue
        for (m, t, at, cig) in ((om, ot, r["start"] - lo, r["cigar"]),
                                (cm, ct, *((ups[j][1] - lo, ups[j][2]) if j in ups else (r["start"] - lo, r["cigar"])))):
            for bi, x in columns(r, at, cig)[0]:
                if 0 <= x < W:
                    t[x] += int(r["quals"][bi])
                    m[x] += int(r["quals"][bi]) if differ(int(r["codes"][bi]), int(ref[x])) else 0
    orig_cols = clean_cols = 0
    for x in range(W):
        if cm[x] == om[x]:
            continue
        if 100 * om[x] > 15 * ot[x]:
            orig_cols += 1
            clean_cols += 100 * cm[x] > 15 * ct[x]
        elif 100 * cm[x] > 15 * ct[x]:
            clean_cols += 1
    info["cols"] = (orig_cols, clean_cols)
    if not (orig_cols == 0 or clean_cols < orig_cols):
        info["refused"] = True
        return [], info
    return [ups[j] for j in sorted(ups)], info


# ------------------------------------------------------------------ batches for the scoring step
def flat(bins, seq_pad=0, read_pad=0):
    """bins: [(sequences, [(codes, quals, orig)])] -> the arrays of ir_score, the byte arrays beginning at the pads."""
    seq, seq_off, bin_seq = [np.zeros(seq_pad, np.uint8)], [seq_pad], [0]
    read, qual, read_off, bin_read, orig = [np.zeros(read_pad, np.uint8)], [np.zeros(read_pad, np.uint8)], [read_pad], [0], []
    for seqs, reads in bins:
        for s in seqs:
            seq.append(np.asarray(s, np.uint8)), seq_off.append(seq_off[-1] + len(s))
        for c, q, o in reads:
            read.append(np.asarray(c, np.uint8)), qual.append(np.asarray(q, np.uint8)), read_off.append(read_off[-1] + len(c))
            orig.append(o)
        bin_seq.append(len(seq_off) - 1), bin_read.append(len(read_off) - 1)
    return (np.concatenate(seq), np.array(seq_off, np.int64), np.array(bin_seq, np.int64), np.concatenate(read),
            np.concatenate(qual), np.array(read_off, np.int64), np.array(bin_read, np.int64), np.array(orig, np.int32))


def expected(bins):
    """(best, off) of every pair, bin by bin, consensus-major."""
    b, o = [], []
    for seqs, reads in bins:
        for s in seqs:
            for c, q, og in reads:
                sc, at = best(c, q, s, og)
                b.append(sc), o.append(at)
    return np.array(b, np.uint32), np.array(o, np.int32)


def random_bin(rng, n_seq, n_reads, len_lo, len_hi, L_lo, L_hi, n_frac=0.02):
    """Consensuses that differ by an indel from one window, reads drawn from them with errors."""
    W = int(rng.integers(len_lo, len_hi + 1))
    ref = rng.integers(0, 4, W).astype(np.uint8)
    ref[rng.random(W) < n_frac] = 4
    seqs = []
    for _ in range(n_seq):
        u, k = int(rng.integers(1, max(W - 1, 2))), int(rng.integers(1, 9))
        s = np.concatenate([ref[:u], rng.integers(0, 4, k).astype(np.uint8), ref[u:]]) if rng.random() < 0.5 else np.concatenate([ref[:u], ref[u + k:]])
        seqs.append(s[:SEQ_MAX] if len(s) else ref)
    reads = []
    for _ in range(n_reads):
        L = int(rng.integers(L_lo, L_hi + 1))
        src = seqs[int(rng.integers(0, len(seqs)))] if seqs else ref
        o = int(rng.integers(0, max(len(src) - L, 0) + 1))
        c = np.resize(src[o:o + L], L).copy() if len(src[o:o + L]) else rng.integers(0, 4, L).astype(np.uint8)
        bad = rng.random(L) < 0.05
        c[bad] = rng.integers(0, 5, int(bad.sum()))
        q = rng.integers(0, 94, L).astype(np.uint8)
        reads.append((c, q, int(rng.integers(0, W + 5))))
    return seqs, reads


def random_bins(seed, n_bins, **kw):
    rng = np.random.default_rng(seed)
    kw = dict(dict(len_lo=40, len_hi=260, L_lo=1, L_hi=90), **kw)
    return [random_bin(rng, int(rng.integers(0, 4)), int(rng.integers(0, 6)), **kw) for _ in range(n_bins)]


# ------------------------------------------------------------------ BAM files for the command
def aux_z(tag, s):
    return tag.encode() + b"Z" + s.encode() + b"\0"


def aux_i(tag, v):
    import struct
    return tag.encode() + b"i" + struct.pack("<i", v)


def rec(name, flag, ref, pos, mapq, cigar, seq, qual=30, nref=-1, npos=-1, tlen=0, aux=b""):
    return dict(name=name, flag=flag, ref=ref, pos=pos, mapq=mapq, cigar=cigar, seq=seq,
                qual=[qual] * len(seq) if isinstance(qual, int) else qual, nref=nref, npos=npos, tlen=tlen, aux=aux)


def parse(cigar_text):
    import re
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar_text)]


def encode_record(r):
    import struct
    from host_lib import reg2bin
    cig = parse(r["cigar"]) if r["cigar"] != "*" else []
    end = r["pos"] + max(sum(n for n, op in cig if op in "MDN=X"), 1)
    seq = r["seq"] if r["seq"] != "*" else ""
    nib = ["=ACMGRSVTWYHKDBN".index(c) for c in seq.upper()] + [0]
    packed = bytes((nib[i] << 4) | nib[i + 1] for i in range(0, len(seq), 2))
    qual = bytes([0xFF] * len(seq)) if r["qual"] is None else bytes(r["qual"])
    name = r["name"].encode() + b"\0"
    body = struct.pack("<iiBBHHHiiii", r["ref"], r["pos"], len(name), r["mapq"], reg2bin(r["pos"], end) if r["pos"] >= 0 else 4680,
                       len(cig), r["flag"], len(seq), r["nref"], r["npos"], r["tlen"])
    body += name + struct.pack(f"<{len(cig)}I", *pack(cig)) + packed + qual + r["aux"]
    return struct.pack("<i", len(body)) + body


def bgzf(data):
    import struct
    import zlib
    out = b""
    for k in list(range(0, len(data), 60000)) + [None]:
        piece = b"" if k is None else data[k:k + 60000]
        if k is not None and not piece:
            continue
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = c.compress(piece) + c.flush()
        out += (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp +
                struct.pack("<II", zlib.crc32(piece), len(piece)))
    return out


def write_bam(path, contigs, records, header="@HD\tVN:1.6\tSO:coordinate\n"):
    """contigs: [(name, length)]; the records in the order given."""
    import struct
    text = (header + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in contigs)).encode()
    raw = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(contigs))
    for n, ln in contigs:
        raw += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
    raw += b"".join(encode_record(r) for r in records)
    with open(path, "wb") as f:
        f.write(bgzf(raw))
    return path


def write_fasta(path, contigs):
    """contigs: [(name, sequence)]."""
    with open(path, "w") as f:
        for n, s in contigs:
            f.write(f">{n}\n" + "".join(s[k:k + 60] + "\n" for k in range(0, len(s), 60)))
    return path


def classic_case():
    """(reference, records, the names of the six that must move): a 400-base reference with a 6-base deletion at
    [200, 206); six 50-base reads spanning it as 20M6D30M; six that end 5 bases beyond it, aligned 50M with
    mismatching tails at q = 30; and records that no target touches."""
    rng = np.random.default_rng(22)
    ref = [int(x) for x in rng.integers(0, 4, 400)]
    for i in range(5):                     # the tails mismatch at every base
        if ref[206 + i] == ref[200 + i]:
            ref[206 + i] = (ref[206 + i] + 1) % 4
    if ref[199] == ref[205]:               # the deletion cannot move left
        ref[199] = (ref[199] + 1) % 4
    s = "".join("ACGT"[c] for c in ref)
    hap = s[:200] + s[206:]
    records = [rec("far0", 0, 0, 10, 40, "50M", s[10:60])]
    records += [rec(f"tail{k}", 0, 0, 155, 40, "50M", hap[155:205]) for k in range(6)]
    records += [rec(f"span{k}", 0, 0, 180, 40, "20M6D30M", hap[180:230]) for k in range(6)]
    records += [rec("far1", 16, 0, 300, 40, "50M", s[300:350]), rec("lost", 4, -1, -1, 0, "*", "ACGTACGTAC")]
    return s, records, [f"tail{k}" for k in range(6)]


def random_clean_bin(rng):
    """(lo, ref, reads, known): reads drawn from a haplotype with one planted indel, aligned with it, without it, or
    a few bases off; qualities 0 .. 60; a few duplicates, code-4 bases and = / X CIGARs."""
    W = int(rng.integers(90, 300))
    lo = int(rng.integers(0, 1000))
    ref = rng.integers(0, 4, W).astype(np.uint8)
    if rng.random() < 0.3:                                  # a homopolymer run for left alignment
        at = int(rng.integers(35, W - 50))
        ref[at:at + 8] = ref[at]
    ref[rng.random(W) < 0.01] = 4
    k, ins, a = int(rng.integers(1, 9)), bool(rng.random() < 0.5), int(rng.integers(35, W - 45))
    bases = [int(x) for x in rng.integers(0, 4, k)]
    hap = np.array(consensus(ref, a, k, ins, bases), np.uint8)
    reads = []
    for _ in range(int(rng.integers(0, 16))):
        L = int(rng.integers(1, 60))
        o = int(rng.integers(30, max(31, len(hap) - L - 30)))
        c = hap[o:o + L].copy()
        if len(c) < L:
            continue
        q = rng.integers(0, 61, L).astype(np.uint8)
        if rng.random() < 0.15:
            c[int(rng.integers(0, L))] = int(rng.integers(0, 5))
        spans = o + 1 < a and o + L > a + (k if ins else 0) + 1
        if spans and rng.random() < 0.5:
            m1 = a - o
            cigar = [(m1, "M"), (k, "I"), (L - m1 - k, "=")] if ins else [(m1, "M"), (k, "D"), (L - m1, "M")]
            start = lo + o
        else:
            start = lo + (o if o <= a else max(o - k, a) if ins else o + k) + int(rng.integers(-2, 3)) * int(rng.random() < 0.3)
            cigar = [(L, "M")] if rng.random() < 0.8 else [(L, "X")]
        if start < lo or start + L + k + 1 >= lo + W:
            continue
        reads.append(dict(start=start, cigar=cigar, codes=c, quals=q, dup=bool(rng.random() < 0.1)))
    reads.sort(key=lambda r: r["start"])
    known = [(lo + a, k, ins, bases if ins else [])] if rng.random() < 0.3 else []
    return lo, ref, reads, known
