"""Banded-SW batches larger than a launch's workgroup cap — a plain helper
module, the twin of phmm_grid_cases.py.

bsw_extend_kernel (the wave-per-task "wide bucket") and bsw_global_kernel (one
64-task probe per wave and trip) stride over their work past a capped grid.
The batches here repeat a few hundred unique tasks: the oracle runs on the
unique tasks only and its answer is tiled with `sel`.  The caps are read from
the source; sw_dispatch's restated predicates count the tasks that reach each
kernel.  Pure functions of fixed seeds: tests/test_grid_cases_cpu.py checks
the counts without a GPU.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import sw_dispatch as D
from phmm_grid_cases import cap

EXTEND_Q_SHORT = [1, 17, 62, 63, 64, 65, 100, 127, 128, 129, 140, 152, 160, 191, 192, 193, 254, 255]
EXTEND_Q_LONG = [256, 257, 300, 319, 320, 321, 447, 448, 449, 510, 511, 512, 600]


@functools.lru_cache(maxsize=None)
def extend_wide_case(long_queries):
    """Tasks of the wide bucket only, with the default matrix: queries of 152
    bases and more, shorter ones whose score bound h0 + qlen reaches 32000,
    and the 129..151-base class with a bound past 255.  qlen on both sides of
    every 64-column slot edge; `long_queries` adds qlen > 255, which selects the
    kernel's 16-slot instantiation for the whole batch.  Returns the unique
    items, sel (cap + 200 + a few tasks) and the parameters."""
    p = D.to_params(D.DEFAULT_MAT)
    rng = np.random.default_rng(3401 + long_queries)
    items = []
    for qlen in EXTEND_Q_SHORT + (EXTEND_Q_LONG if long_queries else []):
        for v in range(4):
            tlen = max(1, qlen + int(rng.integers(-10, 60)))
            q, t = D.related_pair(rng, qlen, tlen, sub=0.03, indel=0.02, n_frac=0.01 if v == 3 else 0.0)
            if v == 1 and tlen > 4:  # related prefix, then junk: z-drop and band trimming
                cut = int(rng.integers(tlen // 3, tlen))
                t[cut:] = rng.integers(0, 4, tlen - cut)
            if qlen >= 152:
                h0 = int(rng.integers(1, 80))
            elif 129 <= qlen + 1 <= 152 and v & 1:
                h0 = 256 - qlen + int(rng.integers(0, 40))
            else:
                h0 = 32000 - qlen + int(rng.integers(0, 50))
            items.append((q, t, h0, (5, 100, 30, 100)[v]))
    n = cap("bsw_kernels.hip", "kExtendWideGrid") + 200 + 13
    sel = (np.arange(n) % len(items)).astype(np.int32)
    return SimpleNamespace(items=items, sel=sel, params=p)


GLOBAL_W = [0, 1, 2, 3, 4, 8, 16, 50]


@functools.lru_cache(maxsize=None)
def global_case():
    """333 tiny tasks (qlen, tlen 4..40) whose bands put about half on the
    lane path and half on the wave kernel, repeated past 64 x cap tasks: 40 more
    probes and a ragged one of 17.  333 is odd, so every probe mixes both kinds
    at shifting lanes."""
    p = D.to_params(D.DEFAULT_MAT)
    rng = np.random.default_rng(3402)
    items = []
    for k in range(333):
        qlen = int(rng.integers(4, 41))
        tlen = int(np.clip(qlen + rng.integers(-4, 5), 4, 40))
        q, t = D.related_pair(rng, qlen, tlen, sub=0.05, indel=0.03, n_frac=0.02 if k % 5 == 0 else 0.0)
        items.append((q, t, 1, GLOBAL_W[k % len(GLOBAL_W)]))
    n = 64 * cap("bsw_kernels.hip", "kGlobalGrid") + 64 * 40 + 17
    sel = (np.arange(n) % len(items)).astype(np.int32)
    lane = np.array([D.glane_ok(len(q), len(t), w, p.lane_ok) for q, t, _, w in items])
    return SimpleNamespace(items=items, sel=sel, params=p, lane=lane)


def probe_mix(case):
    """Per 64-task probe of the large batch: (lane-path tasks, wave tasks)."""
    lane = case.lane[case.sel]
    pad = (-lane.size) % 64
    a = np.concatenate([lane, np.zeros(pad, bool)]).reshape(-1, 64)
    size = np.full(a.shape[0], 64)
    size[-1] -= pad
    nl = a.sum(axis=1)
    return nl, size - nl


# The ksw_align2 batches run under a lowered grid cap (FCSHIP_ALIGN_GRID):
# test_ksw_align2_batch_bit_exact's two, test_ksw_align2_long_windows[2000]'s,
# and one of test_ksw_align2_gap_costs (e_ins = 12 is past the packed kernel's
# range, so the 32-bit 16-lane launch takes its tasks).
ALIGN_FORCED_GRID = 8
ALIGN_BATCHES = {
    "u8": dict(seed=31, n=400, kw=dict(qmax=240), xbyte="all", gaps=(6, 1, 6, 1)),
    "i16": dict(seed=32, n=400, kw=dict(qmax=400), xbyte="none", gaps=(6, 1, 6, 1)),
    "long_windows": dict(seed=44 + 2000, n=24, kw=dict(qmin=60, qmax=200, tmin=1000, tmax=2000), xbyte="all",
                         gaps=(6, 1, 6, 1)),
    "e_ins_12": dict(seed=90 + 12, n=160, kw=dict(qmax=160), xbyte="mixed", gaps=(5, 1, 2, 12)),
}


@functools.lru_cache(maxsize=None)
def align_batch(name):
    b = ALIGN_BATCHES[name]
    items = D.align_items(b["seed"], b["n"], **b["kw"])
    base = D.X_RESCUE
    if b["xbyte"] == "all":
        xs = np.full(len(items), base | D.KSW_XBYTE, np.int32)
    elif b["xbyte"] == "none":
        xs = np.full(len(items), base, np.int32)
    else:
        xs = np.array([base | (D.KSW_XBYTE if k % 3 else 0) for k in range(len(items))], np.int32)
    p = D.to_params(D.DEFAULT_MAT, *b["gaps"])
    plan = D.align_plan([len(i[0]) for i in items], [len(i[1]) for i in items], xs, p)
    return SimpleNamespace(items=items, xtra=xs, gaps=b["gaps"], plan=plan)


def align_trips(case, grid_cap):
    """Trips of the task loop per launch that runs ({'pk', 'w16', 'w64'}):
    the 16-lane launches take four tasks per workgroup and trip, the 64-lane
    launch one; every launch loops over the whole batch."""
    n = len(case.items)
    out = {}
    for k in set(case.plan.kernel):
        groups = n if k == "w64" else (n + 3) // 4
        out[k] = -(-groups // min(groups, grid_cap))
    return out
