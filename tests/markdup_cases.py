"""Duplicate marking: the rules restated in Python (from DESIGN §2's text, not
from the C++), and the batches the CPU and GPU tests share.

A record is a dict: flag, ref (ref_id), pos (0-based), cigar (text), qual
(bytes, b"" when quality is absent), mate (batch index of the primary record
of the template's other read, or -1), lib.  expected(records) answers which
records are to carry 0x400.
"""
import re

import numpy as np

PAIRED, PROPER, UNMAPPED, MATE_UNMAPPED, REVERSE, MATE_REVERSE, READ1, READ2 = 1, 2, 4, 8, 16, 32, 64, 128
SECONDARY, DUPLICATE, SUPPLEMENTARY = 0x100, 0x400, 0x800
R1_FWD = PAIRED | PROPER | MATE_REVERSE | READ1   # 99
R2_REV = PAIRED | PROPER | REVERSE | READ2        # 147
R1_REV = PAIRED | PROPER | REVERSE | READ1        # 83
R2_FWD = PAIRED | PROPER | MATE_REVERSE | READ2   # 163
OPS = "MIDNSHP=X"


def rec(flag, ref, pos, cigar, qual, mate=-1, lib=0):
    if isinstance(qual, int):   # one value for every base of the read
        qual = bytes([qual]) * query_len(cigar)
    return dict(flag=flag, ref=ref, pos=pos, cigar=cigar, qual=bytes(qual), mate=mate, lib=lib)


def parse_cigar(text):
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", text)]


def query_len(text):
    return sum(n for n, op in parse_cigar(text) if op in "MIS=X")


# ------------------------------------------------------------------ the rules
def examined(r):
    return not r["flag"] & (UNMAPPED | SECONDARY | SUPPLEMENTARY)


def u5(r):
    ops = parse_cigar(r["cigar"])
    if r["flag"] & REVERSE:
        trail = 0
        while ops and ops[-1][1] in "SH":
            trail += ops.pop()[0]
        if not ops:      # nothing but clips: they all lead
            trail = 0
        return r["pos"] + sum(n for n, op in ops if op in "MDN=X") - 1 + trail
    lead = 0
    for n, op in ops:
        if op not in "SH":
            break
        lead += n
    return r["pos"] - lead


def score(r):
    return sum(q for q in r["qual"] if q >= 15)


def strand(r):
    return 1 if r["flag"] & REVERSE else 0


def is_paired(records, i):
    r = records[i]
    return bool(examined(r) and r["flag"] & PAIRED and not r["flag"] & MATE_UNMAPPED and r["mate"] >= 0
                and examined(records[r["mate"]]))


def expected(records):
    """dup[i] for every record."""
    n = len(records)
    dup = [0] * n
    paired = [is_paired(records, i) for i in range(n)]
    groups = {}
    for i, r in enumerate(records):
        m = r["mate"]
        if not (paired[i] and m > i and paired[m] and records[m]["mate"] == i):
            continue
        ends = sorted([(r["ref"], u5(r), strand(r), i), (records[m]["ref"], u5(records[m]), strand(records[m]), m)])
        key = (records[ends[0][3]]["lib"],) + ends[0][:3] + ends[1][:3]
        groups.setdefault(key, []).append((-(score(r) + score(records[m])), i, m))
    for members in groups.values():
        for _, i, m in sorted(members)[1:]:
            dup[i] = dup[m] = 1
    groups = {}
    for i, r in enumerate(records):
        if examined(r):
            groups.setdefault((r["lib"], r["ref"], u5(r), strand(r)), []).append(i)
    for members in groups.values():
        frags = sorted((-score(records[i]), i) for i in members if not paired[i])
        if any(paired[i] for i in members):
            flagged = frags
        else:
            flagged = frags[1:]
        for _, i in flagged:
            dup[i] = 1
    return dup


def stats(records):
    paired = [is_paired(records, i) for i in range(len(records))]
    ex = [examined(r) for r in records]
    pairs = sum(1 for i, r in enumerate(records)
                if paired[i] and r["mate"] > i and paired[r["mate"]] and records[r["mate"]]["mate"] == i)
    return dict(examined=sum(ex), pairs=pairs, fragments=sum(e and not p for e, p in zip(ex, paired)),
                duplicates=sum(expected(records)))


# ------------------------------------------------------------------ flattening
def flatten(records):
    """The SoA arrays of fcsdup_batch: (flag, ref_id, pos, mate, lib, cigar, cigar_off, qual, qual_off)."""
    cig, coff, qual, qoff = [], [0], bytearray(), [0]
    for r in records:
        cig += [(n << 4) | OPS.index(op) for n, op in parse_cigar(r["cigar"])]
        coff.append(len(cig))
        qual += r["qual"]
        qoff.append(len(qual))
    return (np.array([r["flag"] for r in records], np.uint16), np.array([r["ref"] for r in records], np.int32),
            np.array([r["pos"] for r in records], np.int32), np.array([r["mate"] for r in records], np.int32),
            np.array([r["lib"] for r in records], np.int32), np.array(cig, np.uint32), np.array(coff, np.int64),
            np.frombuffer(bytes(qual), np.uint8).copy(), np.array(qoff, np.int64))


def n_ref_lib(records):
    return (max([r["ref"] for r in records] + [0]) + 1, max([r["lib"] for r in records] + [0]) + 1)


# ------------------------------------------------------------------ hand-traced cases
def pair(i, r1, r2):
    """Two records at batch indices i and i + 1 that are each other's mates."""
    r1["mate"], r2["mate"] = i + 1, i
    return [r1, r2]


def hand_cases():
    """[(name, records, the flags traced by hand)]"""
    c = []
    # read 1 forward at 100, read 2 reverse ending at 399: twice; the second has the better qualities
    c.append(("two identical pairs, different scores",
              pair(0, rec(R1_FWD, 0, 100, "100M", 20), rec(R2_REV, 0, 300, "100M", 20)) +
              pair(2, rec(R1_FWD, 0, 100, "100M", 30), rec(R2_REV, 0, 300, "100M", 30)),
              [1, 1, 0, 0]))
    c.append(("a score tie: the lower index stays",
              pair(0, rec(R1_FWD, 0, 100, "100M", 30), rec(R2_REV, 0, 300, "100M", 30)) +
              pair(2, rec(R1_FWD, 0, 100, "100M", 30), rec(R2_REV, 0, 300, "100M", 30)),
              [0, 0, 1, 1]))
    # u5 = 100 three ways: 100 - 0, 105 - 5, 110 - (3 + 7)
    c.append(("one u5 through different leading soft / hard clips",
              [rec(0, 0, 100, "100M", 30), rec(0, 0, 105, "5S95M", 25), rec(0, 0, 110, "3H7S90M", 20)],
              [0, 1, 1]))
    # reverse: 100 + 100 - 1 = 199 and 100 + 90 - 1 + (6 + 4) = 199
    c.append(("a reverse read with trailing S + H",
              [rec(REVERSE, 0, 100, "100M", 20), rec(REVERSE, 0, 100, "90M6S4H", 30)],
              [1, 0]))
    # reverse ends at 199: 100 + (50 + 10 + 40) - 1; 90 + (50 + 45 + 10 + 5) - 1; 100 + 100 - 1
    # scores 90 x 30 = 2700, 105 x 20 = 2100, 100 x 25 = 2500
    c.append(("I, D and N before the 3' end",
              [rec(REVERSE, 0, 100, "50M10D40M", 30), rec(REVERSE, 0, 90, "50M5I45M10N5M", 20),
               rec(REVERSE, 0, 100, "100M", 25)],
              [0, 1, 1]))
    # 100 x 14 counts nothing; 10 x 15 = 150
    c.append(("qualities below 15 are ignored",
              [rec(0, 0, 100, "100M", 14), rec(0, 0, 100, "100M", bytes([15] * 10 + [0] * 90))],
              [1, 0]))
    c.append(("absent quality scores 0",
              [rec(0, 0, 100, "100M", b""), rec(0, 0, 100, "100M", bytes([15] + [0] * 99)),
               rec(0, 1, 100, "100M", b""), rec(0, 1, 100, "100M", b"")],
              [1, 0, 0, 1]))
    c.append(("read 2 listed before read 1",
              pair(0, rec(R2_REV, 0, 300, "100M", 20), rec(R1_FWD, 0, 100, "100M", 20)) +
              pair(2, rec(R1_FWD, 0, 100, "100M", 30), rec(R2_REV, 0, 300, "100M", 30)),
              [1, 1, 0, 0]))
    c.append(("ends on two contigs",
              pair(0, rec(R1_FWD, 0, 100, "100M", 30), rec(R2_REV, 1, 50, "100M", 30)) +
              pair(2, rec(R1_FWD, 0, 100, "100M", 20), rec(R2_REV, 1, 50, "100M", 20)) +
              pair(4, rec(R1_FWD, 0, 100, "100M", 20), rec(R2_REV, 1, 60, "100M", 20)),
              [0, 0, 1, 1, 0, 0]))
    c.append(("two libraries at one position",
              pair(0, rec(R1_FWD, 0, 100, "100M", 30, lib=0), rec(R2_REV, 0, 300, "100M", 30, lib=0)) +
              pair(2, rec(R1_FWD, 0, 100, "100M", 20, lib=1), rec(R2_REV, 0, 300, "100M", 20, lib=1)) +
              [rec(0, 0, 700, "100M", 30, lib=0), rec(0, 0, 700, "100M", 20, lib=1)],
              [0, 0, 0, 0, 0, 0]))
    # both ends at (0, 100): forward 100, reverse 51 + 50 - 1; the second pair has read 1 as the reverse end
    c.append(("an equal-(ref, u5) pair with opposite strands",
              pair(0, rec(R1_FWD, 0, 100, "50M", 30), rec(R2_REV, 0, 51, "50M", 30)) +
              pair(2, rec(R1_REV, 0, 51, "50M", 20), rec(R2_FWD, 0, 100, "50M", 20)),
              [0, 0, 1, 1]))
    c.append(("a fragment at the E of a paired end",
              pair(0, rec(R1_FWD, 0, 100, "100M", 20), rec(R2_REV, 0, 300, "100M", 20)) +
              [rec(0, 0, 100, "100M", 40), rec(REVERSE, 0, 100, "100M", 40)],
              [0, 0, 1, 0]))
    c.append(("a fragment-only group",
              [rec(0, 0, 100, "100M", 20), rec(0, 0, 100, "100M", 30), rec(0, 0, 100, "100M", 30),
               rec(REVERSE, 0, 1, "100M", 30)],
              [1, 0, 1, 0]))
    # the unexamined records sit at the examined fragments' position and carry the better scores; read 1 whose
    # mate is unmapped is a fragment
    c.append(("unmapped, secondary and supplementary records untouched",
              [rec(0, 0, 100, "100M", 20), rec(UNMAPPED, 0, 100, "100M", 40), rec(SECONDARY, 0, 100, "100M", 40),
               rec(SUPPLEMENTARY | DUPLICATE, 0, 100, "100M", 40), rec(0, 0, 100, "100M", 30)] +
              pair(5, rec(PAIRED | MATE_UNMAPPED | READ1, 0, 100, "100M", 25),
                   rec(PAIRED | UNMAPPED | READ2, 0, 100, "100M", 25)),
              [1, 0, 0, 0, 0, 1, 0]))
    c.append(("an incoming 0x400 is cleared",
              [rec(DUPLICATE, 0, 100, "100M", 30), rec(DUPLICATE, 0, 100, "100M", 20), rec(DUPLICATE, 0, 500, "100M", 20)],
              [0, 1, 0]))
    # 2 - 10 = -8, 0 - 8 = -8, 5 - 13 = -8
    c.append(("a negative u5",
              [rec(0, 0, 2, "10S90M", 20), rec(0, 0, 0, "8S92M", 30), rec(0, 0, 5, "13H87M", 25),
               rec(0, 0, 0, "7S93M", 40)],
              [1, 0, 1, 0]))
    return c


# ------------------------------------------------------------------ built batches
def identical_pairs(k=300):
    """One group of k identical pairs; pair 137 has the best score."""
    out = []
    for i in range(k):
        q = 31 if i == 137 else 20 + i % 10
        out += pair(2 * i, rec(R1_FWD, 1, 1000, "151M", q), rec(R2_REV, 1, 1200, "151M", q))
    return out


def fragment_group(k=70):
    return [rec(REVERSE, 0, 40, "5S95M", 35 if i == 41 else 15 + i % 20) for i in range(k)]


QUAL_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 151)


def quality_offsets(seed=5):
    """Groups of three fragments whose scores differ by one in their first
    and last bytes, at every quality length and every byte offset mod 4:
    unmapped records with 1 to 3 bytes of 0xff push the offsets along."""
    rng = np.random.default_rng(seed)
    out, pos, at = [], 0, 0
    seen = set()
    for L in QUAL_LENGTHS:
        for shift in range(4):
            while at % 4 != shift:
                out.append(rec(UNMAPPED, -1, -1, "", b"\xff"))
                at += 1
            pos += 10
            base = rng.integers(15, 41, L).astype(np.uint8)
            if L >= 3:
                base[L // 2] = 14
            b, c = base.copy(), base.copy()
            if L:
                b[0] += 1
                c[0] += 1
                c[-1] += 1
            for q in (base, b, c):
                seen.add((L, at % 4))
                out.append(rec(0, 0, pos, f"{max(L, 1)}M", q.tobytes()))
                at += L
    assert seen >= {(L, s) for L in QUAL_LENGTHS if L for s in range(4)}
    return out


def random_batch(seed=20261020, templates=10500):
    """About 20,000 records on 3 contigs of 2,000 positions and 3 libraries:
    20% of the templates are fragments, 40% repeat an earlier template's
    coordinates, 10% of the reads are soft- or hard-clipped at their 5' end
    (same u5), 5% extra records are secondary, supplementary or unmapped."""
    rng = np.random.default_rng(seed)
    out, coords = [], []
    for _ in range(templates):
        if coords and rng.random() < 0.4:
            frag, lib, ref, p1, p2, rev1 = coords[rng.integers(len(coords))]
        else:
            frag, lib, ref = bool(rng.random() < 0.2), int(rng.integers(3)), int(rng.integers(3))
            p1, rev1 = int(rng.integers(0, 1700)), bool(rng.random() < 0.5)
            p2 = p1 + int(rng.integers(50, 300))
            coords.append((frag, lib, ref, p1, p2, rev1))

        def read(flag, pos, rev):
            L = 100
            cigar = "100M"
            if rng.random() < 0.1:
                k = int(rng.integers(1, 20))
                op = "SH"[int(rng.integers(2))]
                if rev:   # the clip trails: the leftmost position stays
                    cigar = f"{100 - k}M{k}{op}"
                else:     # the clip leads: the leftmost position moves in
                    cigar, pos = f"{k}{op}{100 - k}M", pos + k
                L = 100 - k if op == "H" else 100
            elif rng.random() < 0.05:
                cigar = "40M2I58M" if rng.random() < 0.5 else "40M3D57M3M"
            q = rng.integers(2, 41, L).astype(np.uint8).tobytes()
            return rec(flag | (REVERSE if rev else 0), ref, pos, cigar, q, lib=lib)

        if frag:
            out.append(read(0, p1, rev1))
        else:
            i = len(out)
            a = read(PAIRED | READ1 | (0 if rev1 else MATE_REVERSE), p1, rev1)
            b = read(PAIRED | READ2 | (MATE_REVERSE if rev1 else 0), p2, not rev1)
            if rng.random() < 0.5:
                out += pair(i, a, b)
            else:
                out += pair(i, b, a)
        if rng.random() < 0.09:
            flag = (SECONDARY, SUPPLEMENTARY, UNMAPPED)[int(rng.integers(3))]
            out.append(read(flag | int(rng.integers(2)) * DUPLICATE, p1, rev1))
    return out
