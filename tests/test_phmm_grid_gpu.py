"""PairHMM launches past their first grid trip.

Each launch of csrc/phmm_kernels.hip caps its grid (kStreamGridCap,
kOneGridCap, kFallbackGroups, kRescueWaves); a workgroup that takes a second
batch, group or pair must set up its LDS rings, boundary columns, hap buffers
and segment tables again.  The batches of tests/phmm_grid_cases.py repeat a
few hundred unique pairs past each cap (the counts are asserted here against
the caps parsed from the source, and in tests/test_grid_cases_cpu.py); the
oracle runs on the unique pairs and its answer is tiled.  Bars: the
project's, as test_pairhmm_gpu.check_parity applies them.

FCSHIP_STREAM_K and FCSHIP_COLS are read once per process, so the forced runs
are child processes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import fcship
import phmm_grid_cases as P
from test_pairhmm_gpu import compare_parity

pytestmark = pytest.mark.gpu

CHILD = (
    "import sys; sys.path.insert(0, %r)\n"
    "import numpy as np, fcship\n"
    "d = np.load(sys.argv[1])\n"
    "p = fcship.PhmmPairs(**{f: d[f] for f in d.files})\n"
    "np.save(sys.argv[2], fcship.phmm_compute_pairs(p))\n"
    "print('DONE')\n"
) % os.path.dirname(os.path.abspath(fcship.__file__))


def run_child(tmp_path, p, **env_set):
    src, dst = tmp_path / "batch.npz", tmp_path / "out.npy"
    np.savez(src, **{f: getattr(p, f) for f in p.__dataclass_fields__})
    env = dict(os.environ)
    for k in ("FCSHIP_STREAM_K", "FCSHIP_COLS", "FCSHIP_QUEUE_WAVES"):
        env.pop(k, None)
    env.update(env_set)
    r = subprocess.run([sys.executable, "-c", CHILD, str(src), str(dst)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert "DONE" in r.stdout, r.stderr[-3000:]
    return np.load(dst)


def check_tiled(case, out, exact):
    ref, used_d = case.oracle
    compare_parity(out, case.tile(ref), case.tile(used_d), exact)


def shortest_is_rescued(case):
    hl = case.hap_len()
    return bool(case.oracle[1][hl == hl.min()].any())


@pytest.mark.parametrize("which,K", [("k1", 1), ("k2", 2), ("k1_long0", 1)])
def test_streamed_kernel_more_batches_than_grid_slots(gpu, tmp_path, which, K):
    """phmm3_kernel, `for w = blockIdx.x; w < nbatch; w += gridDim.x`: more
    batches than kStreamGridCap workgroups.  K = 1: the batches past the cap
    are one-pair-per-segment tail batches and the last is ragged; K = 2: K-pair
    head batches past the cap as well.  Those batches hold the class's
    shortest haplotypes: odd and even R, R = 33, N on both sides, rescued pairs
    and a haplotype handed back to the byte-compare kernel."""
    case = P.phmm3_case(which)
    g = P.cap("phmm_kernels.hip", "kStreamGridCap")
    n = case.sel.size
    assert n > g * 4 * K
    nb_head, nbatch = P.stream_batches(n, K, P.phmm3_tail(0 if which == "k1_long0" else 1), 4)
    assert nbatch > g and (K == 1 or nb_head > g + 64)
    assert shortest_is_rescued(case)
    out = run_child(tmp_path, case.pairs(), FCSHIP_STREAM_K=str(K))
    check_tiled(case, out, False)


def test_one_row_kernel_more_groups_than_grid_slots(gpu):
    """exact=True sends the long class through launch_one<float, true, false>:
    more four-pair groups than kOneGridCap workgroups."""
    case = P.phmm3_case("k1")
    assert (case.sel.size + 3) // 4 > P.cap("phmm_kernels.hip", "kOneGridCap")
    out = fcship.phmm_compute_pairs(case.pairs(), exact=True)
    check_tiled(case, out, True)


@pytest.mark.parametrize("cols", ["single", "packed"])
def test_column_kernels_more_batches_than_grid_slots(gpu, tmp_path, cols):
    """phmm5_kernel (four one-pair streams per batch at K = 1, forced tail 4)
    and phmm4_kernel (eight half-streams): one column class with more batches
    than kStreamGridCap."""
    case = P.cols_case()
    g = P.cap("phmm_kernels.hip", "kStreamGridCap")
    width, tail = (4, P.PHMM5_FORCED_TAIL) if cols == "single" else (8, P.PHMM4_TAIL)
    assert case.sel.size > g * width
    assert P.stream_batches(case.sel.size, 1, tail, width)[1] > g + 64
    assert shortest_is_rescued(case)
    out = run_child(tmp_path, case.pairs(), FCSHIP_STREAM_K="1", FCSHIP_COLS=cols)
    check_tiled(case, out, False)


def test_fallback_pass_more_groups_than_grid_slots(gpu):
    """The pass over the pairs that the streamed, column and queue kernels hand
    back (haplotypes with IUPAC or lower-case bytes): more than 4 x
    kFallbackGroups of them and a ragged last group, between as many clean
    pairs; the unrelated high-quality ones underflow there and are rescued.
    Default kernels."""
    case = P.fallback_case()
    odd = np.array(["odd_hap" in k for k in case.kinds])
    assert int(odd[case.sel].sum()) > 4 * P.cap("phmm_kernels.hip", "kFallbackGroups")
    assert (case.oracle[1] & odd).any()
    out = fcship.phmm_compute_pairs(case.pairs())
    check_tiled(case, out, False)


@pytest.mark.parametrize("exact", [True, False])
def test_rescue_pass_more_pairs_than_waves(gpu, exact):
    """Threshold 1e37 rescues every pair (as test_rescue_every_pair): more
    pairs than the 64-lane rescue's kRescueWaves one-pair waves, against the
    oracle's fp64 forward sum."""
    case = P.rescue_case()
    assert case.sel.size > P.cap("phmm_kernels.hip", "kRescueWaves")
    out = fcship.phmm_compute_pairs(case.pairs(), exact=exact, threshold=1e37)
    ref = case.tile(P.rescue_reference(case))
    assert not np.isnan(out).any(), np.flatnonzero(np.isnan(out))[:5]
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(out), fin), np.flatnonzero(np.isfinite(out) != fin)[:5]
    assert np.array_equal(out[~fin], ref[~fin])
    np.testing.assert_allclose(out[fin], ref[fin], rtol=1e-12 if exact else 1e-9, atol=1e-12)
