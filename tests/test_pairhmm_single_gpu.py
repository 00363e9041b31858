"""The single-stream column kernel (phmm5, phmm_cols.h) against the oracle and,
bitwise, against the packed column kernel (phmm4) on the same batch.

FCSHIP_COLS=single|packed forces either kernel for every column class and
FCSHIP_STREAM_K the pairs per stream; both are read once per process, so each
run of the library is a child process.  A rescued pair is one whose result
changes when the fp64 rescue is switched off.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import fcship
from test_pairhmm_gpu import check_parity, mutate, rand_read, random_batch

pytestmark = pytest.mark.gpu

CHILD = (
    "import sys; sys.path.insert(0, %r)\n"
    "import ctypes as C, numpy as np, fcship\n"
    "d = np.load(sys.argv[1])\n"
    "p = fcship.PhmmPairs(**{f: d[f] for f in d.files})\n"
    "out = fcship.phmm_compute_pairs(p)\n"
    "n = C.c_int64()\n"
    "fcship.lib.fcs_phmm_last_rescued(C.byref(n))\n"
    "raw = fcship.phmm_compute_pairs(p, rescue=False)\n"
    "np.savez(sys.argv[2], out=out, raw=raw, rescued=np.int64(n.value))\n"
    "print('DONE')\n"
) % os.path.dirname(os.path.abspath(fcship.__file__))


def run_child(tmp_path, p, cols, k):
    src = tmp_path / "batch.npz"
    if not src.exists():
        np.savez(src, **{f: getattr(p, f) for f in p.__dataclass_fields__})
    dst = tmp_path / f"{cols}_{k}.npz"
    env = dict(os.environ, FCSHIP_COLS=cols, FCSHIP_STREAM_K=str(k))
    r = subprocess.run([sys.executable, "-c", CHILD, str(src), str(dst)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert "DONE" in r.stdout, r.stderr[-3000:]
    d = np.load(dst)
    return d["out"], d["raw"], int(d["rescued"])


def same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_single_against_packed(tmp_path, p, k):
    """The single-stream kernel within the parity bar of the oracle, bitwise
    equal to the packed kernel (NaN patterns included, with and without the
    rescue) and with the same set of rescued pairs.  Returns (out, rescued mask)."""
    out, raw, n = run_child(tmp_path, p, "single", k)
    check_parity(p, out, False)
    pout, praw, pn = run_child(tmp_path, p, "packed", k)
    assert same_bits(raw, praw), np.flatnonzero(raw.view(np.uint64) != praw.view(np.uint64))[:8]
    assert same_bits(out, pout), np.flatnonzero(out.view(np.uint64) != pout.view(np.uint64))[:8]
    resc, presc = out.view(np.uint64) != raw.view(np.uint64), pout.view(np.uint64) != praw.view(np.uint64)
    assert np.array_equal(resc, presc) and n == pn
    return out, resc


def edge_batch():
    rng = np.random.default_rng(7005)
    hl = [150, 175, 176, 191, 192, 207, 208, 223, 224, 239, 240, 255, 256, 271, 272, 303, 304]
    haps = []
    for H in hl:
        h = rng.choice(np.frombuffer(b"ACGT", np.uint8), H)
        h[rng.random(H) < 0.01] = ord("N")
        haps.append(h)
    haps[5] = haps[5].copy()
    haps[5][::11] = ord("Y")  # bytes outside ACGTN: handed back to the byte-compare kernel
    reads = []
    for i in range(140):
        R = (33, 34, 60, 101, 151, 160)[i % 6]
        rd = list(rand_read(rng, R, n_frac=0.01))
        if i % 7:
            rd[0] = mutate(rng, haps[i % len(haps)], R)
        else:  # unrelated, Q40, gap 60: underflows the fp32 pass
            rd[1][:] = 40
            rd[2][:] = rd[3][:] = 60
        reads.append(tuple(rd))
    return fcship.make_pairs(reads, haps)


@pytest.mark.parametrize("k", [1, 9, 16])
def test_single_class_edges(gpu, tmp_path, k):
    """Haplotype lengths at and beside every class edge (H = 16 C - 1 is the
    class's last, 304 goes to the row-streamed kernel), reads from the minimum
    R = 33 up, N bases, rescues inside streams and a haplotype handed back.
    K = 9 and 16 use lanes 8..15 of the segment table."""
    p = edge_batch()
    _, resc = check_single_against_packed(tmp_path, p, k)
    assert resc.sum() > 0, "the fp64 rescue must run on some streamed pairs"


def test_single_ring_wrap(gpu, tmp_path):
    """R takes every value 33 .. 81, so (R + 2) mod 48 takes every residue and
    pair boundaries, V and Z rows land on every slot of the 48-row ring."""
    rng = np.random.default_rng(4801)
    haps = [rng.choice(np.frombuffer(b"ACGT", np.uint8), H) for H in (160, 250, 300)]
    reads = []
    for i in range(267):
        R = 33 + i % 49
        rd = list(rand_read(rng, R, n_frac=0.01))
        rd[0] = mutate(rng, haps[i % 3], R)
        reads.append(tuple(rd))
    p = fcship.make_pairs(reads, haps)
    assert p.n_pairs == 801
    check_single_against_packed(tmp_path, p, 16)


def test_single_ragged_ends(gpu, tmp_path):
    """Per-class pair counts 1, 3, 4 K - 1 and 4 K + 1 (K = 5): a partly filled
    wave, an empty stream beside full ones, a stream one pair short, and a
    one-pair-per-stream tail batch after a full one."""
    k = 5
    rng = np.random.default_rng(505)
    reads, haps, pairs = [], [], []
    for H, n in ((300, 1), (270, 3), (230, 4 * k - 1), (170, 4 * k + 1)):  # classes C = 19, 17, 15, 11
        haps.append(rng.choice(np.frombuffer(b"ACGT", np.uint8), H))
        for _ in range(n):
            R = int(rng.integers(33, 152))
            rd = list(rand_read(rng, R))
            rd[0] = mutate(rng, haps[-1], R)
            pairs.append((len(reads), len(haps) - 1))
            reads.append(tuple(rd))
    p = fcship.make_pairs(reads, haps, pairs=pairs)
    assert p.n_pairs == 8 * k + 4
    out, _ = check_single_against_packed(tmp_path, p, k)
    assert not np.isnan(out).any()
