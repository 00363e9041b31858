"""The register diet of the queue-fed column kernel (phmm6, phmm_cols.h,
DESIGN §4.1j), made to fit four waves per SIMD: the staged row of the ring's
item builder waits packed in two dwords, a pair's haplotype offset and its
first row's scale are read again from the segment table's pair at the block
tops that need them, and a class is launched as CUs x 4 x cols6_waves(C)
workgroups (the measurement left every class at 3).

The packed kernel (phmm4, FCSHIP_COLS=packed) shares none of that: it keeps
its own staged row, table and batches, so bitwise agreement with it checks the
new state handling and not only its self-consistency.  FCSHIP_COLS and
FCSHIP_QUEUE_WAVES are read once per process, so each run of the library is a
child process with its own timeout; no test sets any other variable.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import fcship
from test_pairhmm_gpu import check_parity, mutate
from test_pairhmm_queue_gpu import CHILD, CHILD_PLAN, same_bits, save_batch

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
SPECIAL = np.array([0, 1, 3, 4, 127], np.uint8)


def run(code, path, p, cols, waves):
    """One child: cols = None is the default dispatch (phmm6 for every column
    class), waves = 0 the real grid."""
    src = save_batch(path, p)
    dst = path / f"{cols or 'default'}_{waves}.npz"
    env = dict(os.environ)
    for k in ("FCSHIP_COLS", "FCSHIP_QUEUE_WAVES", "FCSHIP_STREAM_K"):
        env.pop(k, None)
    if cols:
        env["FCSHIP_COLS"] = cols
    if waves:
        env["FCSHIP_QUEUE_WAVES"] = str(waves)
    r = subprocess.run([sys.executable, "-c", code, str(src), str(dst)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert "DONE" in r.stdout, r.stderr[-3000:]
    return np.load(dst)


def assert_same_runs(d, ref):
    for k in ("raw", "out"):
        assert same_bits(d[k], ref[k]), (k, np.flatnonzero(d[k].view(np.uint64) != ref[k].view(np.uint64))[:8])
    assert int(d["rescued"]) == int(ref["rescued"]), (int(d["rescued"]), int(ref["rescued"]))


def hazard_rows(iq, dq):
    """Rows 2..R whose match-to-match is under 2^-4 for certain: both indel
    qualities <= 3 give exactly 0."""
    return int(((iq[1:] <= 3) & (dq[1:] <= 3)).sum())


def packed_fields_batch():
    """200 reads x 6 haplotypes = 400 pairs in each of C = 11, 15 and 19 (H
    inside the class and at its upper edge: 175, 239, 303).  R = 33 + i mod 128
    puts rows R, V and Z on every residue of the 16-step block.  Every other
    read draws all four quality arrays and the GCP from 0..127; the rest keep
    moderate qualities (so their sums stay in fp32's range and are compared as
    such) with 0, 1, 3, 4 and 127 planted in every array, and every tenth of
    them a row with both indel qualities <= 3, a hazard row.  N in 3% of the
    read bases and 1% of the haplotypes'."""
    rng = np.random.default_rng(21104)
    haps = []
    for H in (160, 175, 230, 239, 290, 303):
        h = rng.choice(ACGT, H)
        h[rng.random(H) < 0.01] = ord("N")
        haps.append(h)
    reads, hazards = [], 0
    for i in range(200):
        R = 33 + i % 128
        b = mutate(rng, haps[i % 6], R)
        b[rng.random(R) < 0.03] = ord("N")
        if i % 2:
            bq, iq, dq, gq = (rng.integers(0, 128, R).astype(np.uint8) for _ in range(4))
        else:
            bq = rng.integers(2, 60, R).astype(np.uint8)
            iq = rng.integers(10, 60, R).astype(np.uint8)
            dq = rng.integers(10, 60, R).astype(np.uint8)
            gq = rng.integers(5, 40, R).astype(np.uint8)
            for a in (bq, iq, dq, gq):
                a[rng.choice(R, SPECIAL.size, replace=False)] = SPECIAL
            if i % 20 == 0:
                r = int(rng.integers(1, R))
                iq[r], dq[r] = 3, 1
        hazards += hazard_rows(iq, dq) > 0
        reads.append((b, bq, iq, dq, gq))
    allq = np.concatenate([np.concatenate(r[1:]) for r in reads])
    assert set(SPECIAL.tolist()) <= set(allq.tolist()) and allq.max() == 127
    assert hazards >= 10, hazards
    assert sorted({len(r[0]) % 16 for r in reads}) == list(range(16))
    return fcship.make_pairs(reads, haps)


def test_packed_row_fields(gpu, tmp_path):
    """The default dispatch with two waves per class (streams tens of pairs
    long: table slots and ring slots are reused) bitwise equal to the packed
    kernel with and without the rescue, the same rescue count, and inside the
    1e-5 bar of the oracle."""
    p = packed_fields_batch()
    assert p.n_pairs == 1200
    d = run(CHILD, tmp_path, p, None, 2)
    ref = run(CHILD, tmp_path, p, "packed", 0)
    assert_same_runs(d, ref)
    used_d = check_parity(p, d["out"], False)
    fb = np.isnan(d["raw"]).sum()
    print(f"pairs {p.n_pairs}, rescued {int(d['rescued'])}, oracle rescued {int(used_d.sum())}, NaN without rescue {fb}")
    assert not np.isnan(d["out"]).any()


def test_full_residency_grid(gpu, tmp_path):
    """One class (C = 12, H in 176..191), 3,000 pairs, the real grid of CUs x 4
    x cols6_waves(12) workgroups: most find the queue empty and leave.  Every
    output is written (no sentinel), none is NaN, all three forwards of the
    plan agree and equal the single-stream kernel's bit for bit."""
    rng = np.random.default_rng(21112)
    haps = [rng.choice(ACGT, 176 + i % 16) for i in range(30)]
    reads = []
    for i in range(100):
        R = int(rng.integers(33, 152))
        reads.append((mutate(rng, haps[i % 30], R), rng.integers(2, 60, R).astype(np.uint8),
                      rng.integers(10, 60, R).astype(np.uint8), rng.integers(10, 60, R).astype(np.uint8),
                      rng.integers(5, 40, R).astype(np.uint8)))
    p = fcship.make_pairs(reads, haps)
    assert p.n_pairs == 3000
    q = run(CHILD_PLAN, tmp_path, p, None, 0)
    s = run(CHILD_PLAN, tmp_path, p, "single", 0)
    res = q["res"]
    assert not (res == 12345.0).any(), np.argwhere(res == 12345.0)[:8]
    assert not np.isnan(res).any(), np.argwhere(np.isnan(res))[:8]
    assert same_bits(res[0], res[1]) and same_bits(res[0], res[2])
    assert same_bits(res[0], s["res"][0]), np.flatnonzero(res[0].view(np.uint64) != s["res"][0].view(np.uint64))[:8]
    assert np.array_equal(q["cnt"], s["cnt"]), (q["cnt"], s["cnt"])


@pytest.mark.parametrize("H0", [256, 288])
def test_rederived_offsets_differ_between_pairs(gpu, tmp_path, H0):
    """One class (C = 17 from H0 = 256, C = 19 from 288), one wave, eight
    pairs of eight different haplotype lengths and read lengths: each of the
    wave's four streams runs two pairs, so the haplotype offset and the scale
    2^120 / H that the body reads again from the table's pair differ between
    pair n and pair n + 1 of a stream.  Bitwise the packed kernel's."""
    rng = np.random.default_rng(21117 + H0)
    haps = [rng.choice(ACGT, H0 + 2 * i) for i in range(8)]
    reads = []
    for i in range(8):
        R = 40 + 13 * i
        reads.append((mutate(rng, haps[i], R), rng.integers(2, 60, R).astype(np.uint8),
                      rng.integers(10, 60, R).astype(np.uint8), rng.integers(10, 60, R).astype(np.uint8),
                      rng.integers(5, 40, R).astype(np.uint8)))
    p = fcship.make_pairs(reads, haps, pairs=[(i, i) for i in range(8)])
    d = run(CHILD, tmp_path, p, None, 1)
    ref = run(CHILD, tmp_path, p, "packed", 0)
    assert_same_runs(d, ref)
    assert not np.isnan(d["out"]).any()
    check_parity(p, d["out"], False)
