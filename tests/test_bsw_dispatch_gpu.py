"""GPU parity at the banded-SW kernel-selection edges.

ksw_extend2, ksw_global2 and ksw_align2 each choose among several kernels by
predicates on the scoring matrix, gap costs, lengths, band and h0; a narrow
kernel (packed u8 / 16-bit / biased u16) is exact only inside its envelope.
The batches here (tests/sw_dispatch.py, coverage asserted on the CPU by
tests/test_sw_dispatch_cpu.py and again here) put tasks on each side of each
predicate's edge.  Bar: bit-exact against the oracle — the six ksw_extend2
integers and the cell count, ksw_global2's score and CIGAR (and the
score-only run), all seven kswr_t fields of ksw_align2.  No tolerances, no
filtered tasks.
"""
import numpy as np
import pytest

import fcship
import oracle_lib
import sw_dispatch as D

pytestmark = pytest.mark.gpu


def assert_extend_equal(items, mat, kw=None, what=""):
    kw = kw or {}
    m = np.asarray(mat, np.int8)
    tasks = fcship.make_tasks(items)
    res, cells = fcship.bsw_extend_batch(tasks, fcship.bsw_params(mat=m, **kw))
    ref, rcells = oracle_lib.ksw_extend2_batch(tasks, m, **kw)
    bad = np.flatnonzero((res != ref).any(axis=1) | (cells != rcells))
    if bad.size:
        k = int(bad[0])
        raise AssertionError(f"{what}: {bad.size}/{tasks.n} tasks differ; task {k} qlen={tasks.qlen[k]} "
                             f"tlen={tasks.tlen[k]} h0={tasks.h0[k]} w={tasks.w[k]} mat={m.tolist()} kw={kw}: "
                             f"gpu={res[k]}/{cells[k]} ref={ref[k]}/{rcells[k]}")
    return tasks.n


def assert_global_equal(items, mat, gaps=(6, 1, 6, 1), what=""):
    m = np.asarray(mat, np.int8)
    kw = dict(zip(("o_del", "e_del", "o_ins", "e_ins"), gaps))
    t = fcship.make_tasks(items)
    params = fcship.bsw_params(mat=m, **kw)
    scores, cigars = fcship.bsw_global(t, params)
    for k in range(t.n):
        q, tg, _, w = t.task(k)
        rs, rc = oracle_lib.ksw_global2(q, tg, w, m, **kw)
        where = f"{what}: task {k} qlen={len(q)} tlen={len(tg)} w={w} mat={m.tolist()} gaps={gaps}"
        assert scores[k] == rs, f"{where}: score {scores[k]} != {rs}"
        assert np.array_equal(cigars[k], rc), f"{where}: {fcship.cigar_str(cigars[k])} != {fcship.cigar_str(rc)}"
    s2, _ = fcship.bsw_global(t, params, with_cigar=False)
    assert np.array_equal(s2, scores), what
    return t.n


def assert_align_equal(items, mat, xtra, gaps=(6, 1, 6, 1), what=""):
    m = np.asarray(mat, np.int8)
    t = fcship.make_tasks(items)
    xs = np.ascontiguousarray(np.broadcast_to(np.asarray(xtra, np.int32), (t.n,)))
    got = fcship.bsw_align(t, xs, fcship.bsw_params(mat=m, **dict(zip(("o_del", "e_del", "o_ins", "e_ins"), gaps))))
    refs = []
    for k in range(t.n):
        q, tg, _, _ = t.task(k)
        ref = oracle_lib.ksw_align2(q, tg, m, int(xs[k]), *gaps)
        assert tuple(int(v) for v in got[k]) == ref, (
            f"{what}: task {k} qlen={len(q)} tlen={len(tg)} xtra={int(xs[k]):#x} mat={m.tolist()} gaps={gaps}: "
            f"gpu={tuple(int(v) for v in got[k])} ref={ref}")
        refs.append(ref)
    return refs


def _plan(items, xtra, mat, gaps=(6, 1, 6, 1)):
    xs = np.broadcast_to(np.asarray(xtra, np.int32), (len(items),))
    return D.align_plan([len(i[0]) for i in items], [len(i[1]) for i in items], xs, D.to_params(mat, *gaps))


# ------------------------------------------------------------------ ksw_align2
@pytest.mark.parametrize("name", sorted(D.ALIGN_MATS))
def test_align_matrices(gpu, name):
    """Seven matrices x (XBYTE on all / none / mixed per task, XSUBO | XSTART |
    19; XSTOP | 40): 4 x 200 tasks each.  With match >= 2 a good share of the
    XBYTE tasks saturate (score 255, tail skipped) and, but for match 15, a
    good share do not."""
    mat = D.ALIGN_MATS[name]
    items, runs = D.align_matrix_runs(name)
    for run, xs in runs.items():
        refs = assert_align_equal(items, mat, xs, what=f"{name}/{run}")
        if run == "u8" and name in ("2_8_2", "3_5_1", "5_16_1", "15_16_3"):
            sat = sum(r[0] == 255 for r in refs)
            assert sat >= len(items) // 5 and (name == "15_16_3" or len(items) - sat >= len(items) // 5), sat


def test_align_u8_saturation_in_each_path(gpu):
    """gmax + shift >= 255 -> score 255 in the 64-lane kernel, the packed
    16-lane kernel and the 32-bit 16-lane kernel (e_ins = 12), with exact-match
    scores next to 255 - shift on both sides; 92 tasks, each with and without
    XBYTE."""
    seen = set()
    for name, path, mat, gaps, items, x, want in D.align_saturation_cases():
        assert set(_plan(items, x, mat, gaps).kernel) == {path}
        refs = assert_align_equal(items, mat, x, gaps, what=name)
        shift = D.align_shift(mat)
        assert [r[0] for r in refs] == [255 if w + shift >= 255 else w for w in want]
        assert 255 in [r[0] for r in refs] and any(r[0] != 255 for r in refs)
        # the same tasks without XBYTE: the 16-bit run of the same kernels
        assert_align_equal(items, mat, x & ~D.KSW_XBYTE, gaps, what=name + "/i16")
        seen.add(path)
    assert seen == {"w64", "pk", "w16"}


def test_align_i16_score_saturation(gpu):
    """bwa's 16-bit scores saturate at 32767 (saturating adds, no early exit):
    exact matches of 200 .. 600 bases at match 127 and 100, best scores below,
    next to and at 32767, in both 64-lane kernels; 2 x 20 tasks."""
    for mat, items, want in D.align_i16_saturation_case():
        refs = assert_align_equal(items, mat, D.X_RESCUE, what=f"match {int(mat[0])}")
        assert [r[0] for r in refs] == want and 32767 in want
        assert_align_equal(items, mat, D.KSW_XSTART, what=f"match {int(mat[0])}, no XSUBO")


@pytest.mark.parametrize("max_mat,e_ins,inside", D.PACKED16_EDGES)
def test_align_packed_wave_split(gpu, max_mat, e_ins, inside):
    """(max_mat, e_ins) just inside / outside packed16: outside it the packed
    kernel takes the waves whose 16-lane tasks are all u8 (pk = 1) and the
    32-bit kernel the others (pk = 2); the batch holds all-u8, all-i16 and
    mixed groups of four and a partial last group.  Then every task u8 (no
    second launch) and none.  3 x 135 tasks."""
    mat, gaps, items, xt = D.align_wave_split_case(max_mat, e_ins)
    plan = _plan(items, xt, mat, gaps)
    assert plan.packed and plan.packed16 == inside and len(items) % 4 == 3
    assert {"u8", "i16", "mixed"} <= {w.kind for w in plan.waves}
    if not inside:
        assert plan.pk == 1 and {"pk", "w16", "w64"} == set(plan.kernel)
        assert not _plan(items, xt | D.KSW_XBYTE, mat, gaps).second_launch
    assert_align_equal(items, mat, xt, gaps, what="split")
    assert_align_equal(items, mat, xt | D.KSW_XBYTE, gaps, what="all u8")
    assert_align_equal(items, mat, xt & ~D.KSW_XBYTE, gaps, what="all i16")


@pytest.mark.parametrize("gaps", D.ALIGN_GAP_EDGES)
def test_align_gap_edges_matrix_3_5_1(gpu, gaps):
    """e_ins 11 (packed kernel) / 12 (32-bit kernel) with matrix (3, -5, -1),
    widths mixed per task; 160 tasks."""
    mat, gaps, items, xt = D.align_gap_edge_case(gaps)
    assert _plan(items, xt, mat, gaps).packed == (gaps[3] <= 11)
    assert_align_equal(items, mat, xt, gaps, what=str(gaps))


def test_align_matrix_support_edge(gpu):
    """mx + shift <= 255 is the profile's limit.  max 127 / min -128 sits on
    it (shift 128) and must be exact; a matrix without a non-positive entry is
    past it and must raise, not return numbers."""
    items = D.align_items(1001, 60, qmax=200, tmax=300, related=0.9, copy=0.9)
    mat = D.mat_abn(127, -128, -1)
    assert D.align_supported(mat) and int(mat.max()) + D.align_shift(mat) == 255
    xt = np.array([D.X_RESCUE | (D.KSW_XBYTE if k % 2 else 0) for k in range(len(items))], np.int32)
    assert_align_equal(items, mat, xt, what="127/-128")
    for bad in (D.mat_abn(3, 1, 1), np.full(25, 127, np.int8)):
        assert not D.align_supported(bad)
        out_before = None
        with pytest.raises(fcship.FcsError, match="a scoring matrix without a negative entry is unsupported") as e:
            out_before = fcship.bsw_align(fcship.make_tasks(items[:8]), D.X_RESCUE | D.KSW_XBYTE,
                                          fcship.bsw_params(mat=bad))
        assert e.value.code == fcship.FCS_ERR_UNSUPPORTED and out_before is None


# ------------------------------------------------------------------ ksw_global2
@pytest.mark.parametrize("gaps", D.GLOBAL_U16_GAPS)
@pytest.mark.parametrize("mat_name", sorted(D.GLOBAL_U16_MATS))
def test_global_u16_form_edge(gpu, mat_name, gaps):
    """span (glane_u16_ok) at the largest value <= 8000 and the smallest above
    it, matrices with -16 entries, w = 16 and 4, identical / all-mismatch /
    related contents; and 64-task waves of in-span tasks holding one over-span
    task (the wave vote sends them to the 32-bit rows).  24 + 24 + 138 tasks."""
    p, b = D.global_u16_batches(mat_name, gaps)
    assert all(w.u16 for w in D.global_waves(b["inside"], p))
    assert not any(w.u16 for w in D.global_waves(b["outside"], p))
    assert [w.over for w in D.global_waves(b["one_over"], p)] == [1, 1, 0]
    mat = D.GLOBAL_U16_MATS[mat_name]
    for side in ("inside", "outside", "one_over"):
        assert_global_equal(b[side], mat, gaps, what=side)


@pytest.mark.parametrize("mat_name", ["default", "1_16_16"])
def test_global_lane_path_grid(gpu, mat_name):
    """glane_ok and the NB classes: w in {0, 1, 2, 8, 9, 16, 17, 32, 33} x qlen
    in {nb - 1, nb, nb + 1} x tlen in {1, 2, 3, qlen - 3, qlen, qlen + 3}, the
    64-task waves mixing lane-path and wave-path tasks and NB classes; 288
    tasks."""
    items = D.global_grid_items()
    mat = D.DEFAULT_MAT if mat_name == "default" else D.GLOBAL_U16_MATS[mat_name]
    waves = D.global_waves(items, D.to_params(mat))
    assert all(w.lane and w.wave for w in waves) and any(len(w.classes) >= 2 for w in waves)
    assert_global_equal(items, mat, what=mat_name)


@pytest.mark.parametrize("mat_name", sorted(D.GLOBAL_LANE_OK_MATS))
def test_global_lane_ok_matrix_edge(gpu, mat_name):
    """Matrix entries -16 / 15 keep the lane path; -17 or 16 send every task
    to the wave kernel.  The grid's tasks (144) either way."""
    items = D.global_grid_items(reps=1)
    mat = D.GLOBAL_LANE_OK_MATS[mat_name]
    p = D.to_params(mat)
    assert p.lane_ok == (mat_name == "15_16_16")
    assert (sum(w.lane for w in D.global_waves(items, p)) > 0) == p.lane_ok
    assert_global_equal(items, mat, what=mat_name)


# ------------------------------------------------------------------ ksw_extend2
@pytest.mark.parametrize("mat_name", sorted(D.EXT_GRID_MATS))
def test_extend_class_and_form_grid(gpu, mat_name):
    """Column classes (qlen + 1 at 16 / 32 / 48 / 64 / 96 / 128 / 152, each
    side) x score forms (bound 255 / 256, pair envelope 255 / 256), three
    matrices, related / junk-tail / exact-prefix contents (the last reach the
    bound itself), query N in a third of the first two; 1,008 tasks per run."""
    p, items = D.extend_grid_items(mat_name)
    bk = set(D.extend_buckets(items, p))
    if mat_name == "default":
        assert bk == set(range(16)) - {6}  # bucket 6 is never selected (those tasks take the wave kernel)
    assert D.WIDE_BUCKET in bk and any(D.PAIR_BUCKET0 <= b < D.WIDE_BUCKET for b in bk) and any(b < 4 for b in bk)
    mat = D.EXT_GRID_MATS[mat_name]
    assert_extend_equal(items, mat, what=mat_name)
    if mat_name == "default":
        assert_extend_equal(items, mat, dict(zdrop=0), what="zdrop 0")
        assert_extend_equal(items, mat, dict(end_bonus=0), what="end_bonus 0")
        assert_extend_equal(items, mat, dict(o_del=4, e_del=2, o_ins=7, e_ins=1, zdrop=30), what="asymmetric gaps")


@pytest.mark.parametrize("edge", ["bound_32000", "tlen_1024", "e_del_17", "e_ins_17", "pair_cg_129", "mat_min_17",
                                  "mat_max_16"])
def test_extend_predicate_edges(gpu, edge):
    """bound 31999 / 32000, tlen 1023 / 1024 in the pair envelope, e_del and
    e_ins 16 / 17, pair_cg 128 / 129, matrix entries -16 / -17 and 15 / 16:
    the same tasks (or the same shapes) on either side of each edge."""
    sides = set()
    for label, mat, kw, items in D.extend_edge_cases()[edge]:
        sides.add(frozenset(D.extend_buckets(items, D.to_params(mat, **kw))))
        assert_extend_equal(items, mat, kw, what=f"{edge}/{label}")
    assert len(sides) == 2  # the two runs take different sets of kernels
