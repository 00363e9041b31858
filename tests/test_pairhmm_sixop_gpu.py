"""The six-op cell of the column kernels (phmm_cols.h): the
deletion chain runs with unit coefficient (E = D / my) and a row hands
X / mm' to the row below, whose priors carry mm'.  The division makes rows
whose match-to-match is under 2^-4 (exactly 0 when both indel qualities are
<= 3) a hazard: their pairs must reach the one-row kernel through the fallback
list, and nothing but finite values may enter a stream, because a Z row does
not clear a NaN and every later pair of the stream would be poisoned.

FCSHIP_COLS, FCSHIP_QUEUE_WAVES and FCSHIP_STREAM_K are read once per process,
so each run of the library is a child process.  Every batch runs under `queue`
(one wave per class: each of its four streams runs its pairs back to back),
`single` and `packed` (eight pairs per stream); the three must agree bitwise,
with and without the fp64 rescue.

Comparison with the oracle: with the rescue, check_parity's 1e-5 relative bar.
Without it, the same bar against the oracle's own fp32 forward sum wherever the
oracle accepted that sum (it is then >= GKL's 1e-28 threshold scaled by 2^120,
a normal float with full relative precision); below the threshold the fp32
sums of two operation orders may differ by any factor, so those pairs are only
required not to be NaN.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import fcship
import oracle_lib
from test_pairhmm_gpu import RTOL, check_parity, mutate
from test_pairhmm_single_gpu import CHILD

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
LOG10_INIT = np.float32(np.log10(np.float32(2.0 ** 120)))


def run(path, p, cols, tag=""):
    src = path / f"batch{tag}.npz"
    if not src.exists():
        np.savez(src, **{f: getattr(p, f) for f in p.__dataclass_fields__})
    dst = path / f"{cols}{tag}.npz"
    env = dict(os.environ, FCSHIP_COLS=cols)
    env.pop("FCSHIP_QUEUE_WAVES", None)
    env.pop("FCSHIP_STREAM_K", None)
    if cols == "queue":
        env["FCSHIP_QUEUE_WAVES"] = "1"
    else:
        env["FCSHIP_STREAM_K"] = "8"
    r = subprocess.run([sys.executable, "-c", CHILD, str(src), str(dst)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert "DONE" in r.stdout, r.stderr[-3000:]
    d = np.load(dst)
    return d["out"], d["raw"], int(d["rescued"])


def same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_three(path, p):
    """queue, single and packed bitwise equal (outputs with and without the
    rescue, rescue count); no NaN; parity with the oracle.  Returns the queue
    run's (out, raw)."""
    out, raw, n = run(path, p, "queue")
    for cols in ("single", "packed"):
        o, r, m = run(path, p, cols)
        assert same_bits(r, raw), (cols, np.flatnonzero(r.view(np.uint64) != raw.view(np.uint64))[:8])
        assert same_bits(o, out), (cols, np.flatnonzero(o.view(np.uint64) != out.view(np.uint64))[:8])
        assert m == n, (cols, m, n)
    assert not np.isnan(out).any(), np.flatnonzero(np.isnan(out))[:8]
    assert not np.isnan(raw).any(), np.flatnonzero(np.isnan(raw))[:8]
    ref, used_d, rawf = oracle_lib.phmm_batch(p, raw=True)
    ok = ~used_d
    exp = (np.log10(rawf[ok]) - LOG10_INIT).astype(np.float64)
    err = np.abs(raw[ok] - exp) / np.abs(exp)
    fin = np.isfinite(ref)
    print(f"pairs {p.n_pairs}, rescued {n}, fp32-accepted {ok.sum()}, max rel err with rescue "
          f"{np.max(np.abs(out[fin] - ref[fin]) / np.abs(ref[fin])):.3g}, without {err.max() if err.size else 0:.3g}")
    check_parity(p, out, False)
    assert (err <= RTOL).all(), (int((err > RTOL).sum()), raw[ok][err > RTOL][:5], exp[err > RTOL][:5])
    return out, raw


def read_for(rng, hap, R, iq, dq, gq, bq=None, n_frac=0.0, related=True):
    b = mutate(rng, hap, R) if related and len(hap) >= 4 else rng.choice(ACGT, R)
    if n_frac:
        b[rng.random(R) < n_frac] = ord("N")
    if bq is None:
        bq = rng.integers(0, 60, R)

    def arr(v):
        return (np.full(R, v) if np.isscalar(v) else np.asarray(v)).astype(np.uint8)
    return (b, arr(bq), arr(iq), arr(dq), arr(gq))


def test_full_quality_range(gpu, tmp_path):
    """Insertion, deletion and gap-continuation qualities drawn from 0..127 on
    every row (a hazard row in roughly one read in ten), N bases on both
    sides, R at the streamed kernels' minimum, beside it, at the ring's length
    and at 101, H from 1 through the class edges 175 | 176 to the last column
    haplotype 303."""
    rng = np.random.default_rng(61601)
    haps = []
    for H in (1, 2, 15, 16, 17, 150, 175, 176, 303):
        h = rng.choice(ACGT, H)
        h[rng.random(H) < 0.02] = ord("N")
        haps.append(h)
    reads = []
    for i in range(32):
        R = (33, 34, 48, 101)[i % 4]
        reads.append(read_for(rng, haps[5 + i % 4], R, rng.integers(0, 128, R), rng.integers(0, 128, R),
                              rng.integers(0, 128, R), n_frac=0.03, related=i % 3 != 0))
    p = fcship.make_pairs(reads, haps)
    assert p.n_pairs == 288
    check_three(tmp_path, p)


def test_hazard_rows(gpu, tmp_path):
    """One row of iq = dq in {0, 1, 3} (match-to-match exactly 0) at row 1 only
    (no hazard: mm of row 1 never enters the recurrence), at row 2, in the
    middle and at row R; the same places with (iq, dq) = (1, 7), the smallest
    nonzero match-to-match; gcp = 0 (gap-to-match 0) on one row, on every row
    and together with a hazard row."""
    rng = np.random.default_rng(61602)
    haps = [rng.choice(ACGT, H) for H in (40, 160, 290)]
    reads = []
    for R in (33, 101):
        rows = (0, 1, R // 2, R - 1)
        for q in (0, 1, 3, (1, 7)):
            for r in rows:
                iq, dq = np.full(R, 45), np.full(R, 45)
                iq[r], dq[r] = q if isinstance(q, tuple) else (q, q)
                if r == R // 2 and isinstance(q, tuple):
                    iq[r], dq[r] = dq[r], iq[r]  # (7, 1) too
                reads.append(read_for(rng, haps[len(reads) % 3], R, iq, dq, 10))
        for kind in range(3):
            iq, dq, gq = np.full(R, 45), np.full(R, 45), np.full(R, 10)
            if kind == 0:
                gq[R // 3] = 0
            else:
                gq[:] = 0
            if kind == 2:
                iq[R // 2] = dq[R // 2] = 0
            reads.append(read_for(rng, haps[kind], R, iq, dq, gq))
    p = fcship.make_pairs(reads, haps)
    assert p.n_pairs == 2 * 19 * 3
    check_three(tmp_path, p)


def test_hazard_pairs_do_not_poison_their_stream(gpu, tmp_path):
    """One class (H = 165), one wave, 60 reads, every fifth with a row whose
    match-to-match is 0: each of the wave's four streams runs hazard pairs
    between ordinary ones.  The ordinary pairs' outputs are bitwise those of
    the batch without the hazard pairs."""
    rng = np.random.default_rng(61603)
    hap = rng.choice(ACGT, 165)
    reads = []
    for i in range(60):
        R = int(rng.integers(33, 120))
        iq, dq = rng.integers(10, 60, R), rng.integers(10, 60, R)
        if i % 5 == 2:
            r = (1, R // 2, R - 1)[(i // 5) % 3]
            iq[r] = dq[r] = (0, 3)[(i // 5) % 2]
        reads.append(read_for(rng, hap, R, iq, dq, rng.integers(5, 40, R)))
    keep = [i for i in range(60) if i % 5 != 2]
    p = fcship.make_pairs(reads, [hap])
    q = fcship.make_pairs([reads[i] for i in keep], [hap])
    assert p.n_pairs == 60 and q.n_pairs == 48
    out, raw, _ = run(tmp_path, p, "queue")
    qout, qraw, _ = run(tmp_path, q, "queue", tag="_clean")
    assert not np.isnan(out).any() and not np.isnan(raw).any()
    assert same_bits(out[keep], qout) and same_bits(raw[keep], qraw)
    check_parity(p, out, False)


def test_headroom_short_haplotypes(gpu, tmp_path):
    """H = 1 and H = 2 (the largest row-0 value, 2^120 / H) against R = 33,
    matching high-quality reads whose rows have (iq, dq) = (1, 9): the
    match-to-match closest above the 2^-4 bound, so the hand-off X / mm' is as
    large as the kernel ever lets it get (a = gm'/mm' = 12.5 of the bound's
    16).  On row 2 only, on every row (with gcp = 1 from row 3 on, so that the
    31 or 32 insertions these pairs need do not underflow fp32 and the sum comes
    from the column kernel itself), and (1, 9) | (9, 1) alternating."""
    mm = 1.0 - (10 ** -0.1 + 10 ** -0.9)
    assert 2.0 ** -4 < mm < 0.09
    rng = np.random.default_rng(61604)
    haps = [np.frombuffer(b"A", np.uint8), np.frombuffer(b"AC", np.uint8)]
    reads = []
    for kind in range(3):
        for base in b"AC":
            R = 33
            iq, dq, gq = np.full(R, 45), np.full(R, 45), np.full(R, 40)
            if kind == 0:
                iq[1], dq[1] = 1, 9
            elif kind == 1:
                iq[:], dq[:] = 1, 9
                gq[2:] = 1  # cheap insertions: 31 or 32 of them stay inside fp32
            else:
                iq[::2], dq[::2] = 1, 9
                iq[1::2], dq[1::2] = 9, 1
            rd = list(read_for(rng, haps[1], R, iq, dq, gq, bq=60, related=False))
            rd[0][:] = base
            reads.append(tuple(rd))
    p = fcship.make_pairs(reads, haps)
    assert p.n_pairs == 12
    out, raw = check_three(tmp_path, p)
    assert np.isfinite(out).all()
