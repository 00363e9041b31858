"""Coverage of tests/test_bsw_dispatch_gpu.py's batches, checked without a GPU.

The task builders of sw_dispatch are pure functions; here the restated
selection predicates (sw_dispatch, mirroring csrc/) classify their tasks and
each side of each kernel-selection edge must hold at least one task, each
kind of wave must exist, and each u8 path must hold saturating tasks (by the
oracle).  The restatements decide coverage only, never correctness.
"""
import numpy as np
import pytest

import oracle_lib
import sw_dispatch as D


def test_packed16_edges_by_evaluation():
    """The (max_mat, e_ins) pairs straddle packed16 while packed holds; e_ins
    12 leaves the packed kernel altogether."""
    for mm, e, inside in D.PACKED16_EDGES:
        assert D.align_packed_ok(255, 16, 6, e)
        assert D.align_packed_ok(D.align_i16_mmax(mm), 8, 6, e) == inside, (mm, e)
    assert D.align_packed_ok(255, 16, 6, 11) and not D.align_packed_ok(255, 16, 6, 12)
    assert D.align_packed_ok(D.align_i16_mmax(1), 8, 6, 11)  # default matrix: packed16 whenever packed


def test_align_shift_and_support():
    assert [D.align_shift(D.ALIGN_MATS[k]) for k in ("default", "2_8_2", "3_5_1", "5_16_1", "15_16_3", "1_1_0")] == \
        [4, 8, 5, 16, 16, 1]
    assert all(D.align_supported(m) for m in D.ALIGN_MATS.values())
    assert D.align_supported(D.mat_abn(127, -128, -1))  # mx + shift == 255: the last supported matrix
    assert not D.align_supported(D.mat_abn(3, 1, 1)) and not D.align_supported(np.full(25, 127, np.int8))
    a = D.ALIGN_MATS["asym"].reshape(5, 5)
    assert (np.diag(a)[:4] > 0).all() and a.min() >= -12 and a.max() <= 6 and not np.array_equal(a, a.T)


@pytest.mark.parametrize("name", sorted(D.ALIGN_MATS))
def test_align_matrix_runs_cover_kernels_and_saturation(name):
    mat = D.ALIGN_MATS[name]
    items, runs = D.align_matrix_runs(name)
    assert len(items) == 200
    ql, tl = [len(x[0]) for x in items], [len(x[1]) for x in items]
    assert min(ql) >= 10 and max(ql) <= 200 and min(tl) >= 40 and max(tl) <= 700
    p = D.to_params(mat)
    plan = D.align_plan(ql, tl, runs["mixed"], p)
    assert plan.seg and plan.packed and plan.packed16  # these matrices: one packed launch + the 64-lane launch
    assert {"pk", "w64"} <= set(plan.kernel)
    assert D.align_plan(ql, tl, runs["u8"], p).all_u8 and not plan.all_u8
    sat = sum(oracle_lib.ksw_align2(q, t, mat, int(runs["u8"][0]))[0] == 255 for q, t, _, _ in items)
    if int(mat.reshape(5, 5)[0, 0]) >= 2 and name != "asym":
        assert sat >= len(items) // 5, sat
        if name == "15_16_3":  # with gaps 6/1 against match 15 even unrelated sequences pass 255 - 16
            assert sat >= len(items) * 9 // 10
        else:
            assert len(items) - sat >= len(items) // 5, sat
    if name in ("default", "1_1_0"):
        assert sat == 0  # match 1: 200 bases cannot reach 255


def test_align_saturation_cases_cover_each_u8_path():
    seen = set()
    for name, path, mat, gaps, items, x, want in D.align_saturation_cases():
        p = D.to_params(mat, *gaps)
        ql, tl = [len(i[0]) for i in items], [len(i[1]) for i in items]
        plan = D.align_plan(ql, tl, [x] * len(items), p)
        assert set(plan.kernel) == {path}, (name, set(plan.kernel))
        shift = D.align_shift(mat)
        scores = [oracle_lib.ksw_align2(q, t, mat, x, *gaps)[0] for q, t, _, _ in items]
        for s, w in zip(scores, want):  # the builder's exact-match arithmetic
            assert s == (255 if w + shift >= 255 else w), (name, s, w)
        assert any(w + shift >= 255 for w in want) and any(w + shift < 255 for w in want), name
        edge = {w - (255 - shift) for w in want}
        assert (edge & {-2, -1}) and (edge & {0, 1}), (name, sorted(edge))  # next to the edge on both sides
        if name.endswith("a3") or name.startswith("w64") or "a3_" in name:
            assert {-1, 0, 1} <= edge, (name, sorted(edge))
        seen.add(path)
    assert seen == {"w64", "pk", "w16"}


def test_align_i16_saturation_case_straddles_32767():
    for mat, items, want in D.align_i16_saturation_case():
        assert D.align_supported(mat)
        plan = D.align_plan([len(i[0]) for i in items], [len(i[1]) for i in items], [D.X_RESCUE] * len(items),
                            D.to_params(mat))
        assert set(plan.kernel) == {"w64"}
        scores = [oracle_lib.ksw_align2(q, t, mat, D.X_RESCUE)[0] for q, t, _, _ in items]
        assert scores == want  # the builder's arithmetic, capped at 32767
        a = int(mat[0])
        assert 32767 in want and any(32767 - a < w < 32767 for w in want) and min(want) < 30000
        assert any(len(i[0]) + 15 <= 256 for i in items) and any(len(i[0]) + 15 > 256 for i in items)  # both slot counts


@pytest.mark.parametrize("max_mat,e_ins,inside", D.PACKED16_EDGES)
def test_align_wave_split_case_holds_every_wave_kind(max_mat, e_ins, inside):
    mat, gaps, items, xt = D.align_wave_split_case(max_mat, e_ins)
    assert D.align_supported(mat) and mat.min() < 0 and len(items) % 4 == 3
    p = D.to_params(mat, *gaps)
    ql, tl = [len(i[0]) for i in items], [len(i[1]) for i in items]
    plan = D.align_plan(ql, tl, xt, p)
    assert plan.packed and plan.packed16 == inside
    kinds = {w.kind for w in plan.waves}
    assert {"u8", "i16", "mixed"} <= kinds
    assert plan.waves[-1].partial
    assert "w64" in plan.kernel
    if inside:
        assert plan.pk == 0 and not plan.second_launch and "w16" not in plan.kernel
    else:
        assert plan.pk == 1 and plan.second_launch
        for kind in ("u8",):  # pk = 1: the packed launch's waves
            assert any(w.kind == kind and w.packed_launch for w in plan.waves)
        for kind in ("i16", "mixed"):  # pk = 2: the 32-bit launch's waves
            assert any(w.kind == kind and not w.packed_launch for w in plan.waves)
        assert {"pk", "w16", "w64"} == set(plan.kernel)
        # a u8 group next to a long i16 task (the 64-lane launch's) still votes u8
        assert any(w.kind == "u8" and w.packed_launch and
                   any(not (xt[k] & D.KSW_XBYTE) for k in range(4 * i, min(4 * i + 4, len(items))))
                   for i, w in enumerate(plan.waves))
        allu8 = D.align_plan(ql, tl, xt | D.KSW_XBYTE, p)
        assert allu8.all_u8 and not allu8.second_launch and "w16" not in allu8.kernel


@pytest.mark.parametrize("gaps", D.ALIGN_GAP_EDGES)
def test_align_gap_edge_case_selects_by_e_ins(gaps):
    mat, gaps, items, xt = D.align_gap_edge_case(gaps)
    plan = D.align_plan([len(i[0]) for i in items], [len(i[1]) for i in items], xt, D.to_params(mat, *gaps))
    assert plan.packed == (gaps[3] <= 11)
    assert set(plan.kernel) == ({"pk", "w64"} if gaps[3] <= 11 else {"w16", "w64"})


@pytest.mark.parametrize("gaps", D.GLOBAL_U16_GAPS)
@pytest.mark.parametrize("mat_name", sorted(D.GLOBAL_U16_MATS))
def test_global_u16_batches_sit_on_the_edge(mat_name, gaps):
    p, b = D.global_u16_batches(mat_name, gaps)
    assert p.lane_ok
    tot = D.u16_edge_total(p)
    if gaps == (6, 1, 6, 1):
        assert tot == 467
    for q, t, _, w in b["inside"]:
        assert len(q) + len(t) == tot and D.glane_span(len(q), len(t), p) <= 8000 < D.glane_span(len(q) + 1, len(t), p)
        assert D.glane_ok(len(q), len(t), w, True)
    for q, t, _, w in b["outside"]:
        assert len(q) + len(t) == tot + 1 and D.glane_span(len(q), len(t), p) > 8000
        assert D.glane_ok(len(q), len(t), w, True)
    assert {w for _, _, _, w in b["inside"]} == {16, 4} == {w for _, _, _, w in b["outside"]}
    assert all(w.u16 for w in D.global_waves(b["inside"], p))
    assert not any(w.u16 for w in D.global_waves(b["outside"], p))
    one = D.global_waves(b["one_over"], p)
    assert [w.over for w in one[:2]] == [1, 1] and not one[0].u16 and not one[1].u16 and one[0].lane == 64
    assert one[2].u16  # the batch's last wave: in-span tasks only


def test_global_grid_covers_glane_ok_edges():
    items = D.global_grid_items()
    p = D.to_params(D.DEFAULT_MAT)
    ok = {}
    for q, t, _, w in items:
        ok.setdefault((w, len(q) - (2 * w + 1), min(len(t), 4)), set()).add(D.glane_ok(len(q), len(t), w, True))
    assert {w for w, _, _ in ok} == set(D.GRID_W)
    for w in D.GRID_W:
        lane = 2 <= w <= 32
        assert ok[(w, 0, 3)] == {lane} and ok[(w, 1, 3)] == {lane}, w  # w 1/2, nb 65/67
        assert ok[(w, 0, 2)] == {False} and ok[(w, 0, 1)] == {False}  # tlen 2/3
        if w >= 1:
            assert ok[(w, -1, 3)] == {False}  # qlen nb - 1 / nb
    waves = D.global_waves(items, p)
    assert len(waves) >= 4
    assert all(w.lane and w.wave for w in waves)  # every wave mixes the two paths
    assert sum(len(w.classes) >= 2 for w in waves) >= 3  # and NB classes
    assert {w.nb for w in waves} <= {17, 33, 65} and 65 in {w.nb for w in waves}
    assert set().union(*[w.classes for w in waves]) == {17, 33, 65}
    for name, mat in D.GLOBAL_LANE_OK_MATS.items():
        pp = D.to_params(mat)
        assert pp.lane_ok == (name == "15_16_16"), name
        lanes = sum(w.lane for w in D.global_waves(items, pp))
        assert (lanes > 0) == pp.lane_ok


def test_extend_grid_covers_every_bucket_and_form():
    seen = set()
    for name in D.EXT_GRID_MATS:
        p, items = D.extend_grid_items(name)
        assert p.lane_ok and p.pair_ok
        bk = D.extend_buckets(items, p)
        seen |= set(bk)
        per_q = {}
        for (q, t, h0, w), b in zip(items, bk):
            per_q.setdefault(len(q), []).append((D.bound_of(len(q), h0, p), 4 in q, b))
        for qlen, rows in per_q.items():
            assert {len(t) - len(q) for q, t, _, _ in items if len(q) == qlen} == {-10, 0, 60}
            assert any(n for _, n, _ in rows) and any(not n for _, n, _ in rows)
            if 256 - qlen * p.max_mat > 1:  # both sides of bound 255 / 256 where h0 can reach them
                assert {255, 256} <= {bd for bd, _, _ in rows}, (name, qlen)
            if 257 - p.pair_cg - qlen * p.max_mat > 1 and qlen <= 151:  # and of the pair envelope
                assert {255, 256} <= {bd + p.pair_cg - 1 for bd, _, _ in rows}, (name, qlen)
                assert any(b >= D.PAIR_BUCKET0 and b < D.WIDE_BUCKET for _, _, b in rows)
        if name == "default":  # pair_cg 6: every class on both sides of both score edges
            # (bucket 6, 152 16-bit columns, is never selected: bsw_bucket sends those tasks to the wave kernel)
            assert set(bk) == set(range(16)) - {6}, sorted(set(bk))
            want = {15: {0, 10}, 16: {1, 10}, 31: {1, 10}, 32: {2, 11}, 47: {2, 11}, 48: {3, 11}, 63: {3, 11},
                    64: {4, 7, 12}, 95: {4, 7, 12}, 96: {5, 8, 13}, 127: {5, 8, 13}, 128: {15, 9, 14},
                    151: {15, 9, 14}, 152: {15}}
            for qlen, rows in per_q.items():
                assert {b for _, _, b in rows} == want[qlen], (qlen, {b for _, _, b in rows})
    assert seen == set(range(16)) - {6}
    assert {D.to_params(m).pair_cg for m in D.EXT_GRID_MATS.values()} == {6, 11}
    assert {D.to_params(m).max_mat for m in D.EXT_GRID_MATS.values()} == {1, 2, 4}


def test_extend_grid_scores_reach_the_bound_in_each_form():
    """The exact-prefix tasks score h0 + qlen max_mat, the bound itself (by the
    oracle): 255 in each byte bucket, 256 in the 16-bit buckets beside them,
    and bound + pair_cg - 1 = 255 in every pair bucket."""
    p, items = D.extend_grid_items("default")
    ref, _ = oracle_lib.ksw_extend2_batch(D.pack(items), D.EXT_GRID_MATS["default"])
    hit = set()
    for (q, t, h0, w), r, b in zip(items, ref, D.extend_buckets(items, p)):
        if int(r[0]) == D.bound_of(len(q), h0, p):
            hit.add((int(r[0]), b))
            hit.add(("pair", int(r[0]) + p.pair_cg - 1, b))
    assert {(255, b) for b in (0, 1, 2, 3, 7, 8, 9)} <= hit
    assert {(256, b) for b in (0, 1, 2, 3, 4, 5, D.WIDE_BUCKET)} <= hit
    assert {("pair", 255, b) for b in range(D.PAIR_BUCKET0, D.WIDE_BUCKET)} <= hit
    assert {("pair", 256, b) for b in (0, 1, 2, 3, 7, 8, 9)} <= hit


def test_extend_edge_cases_flip_the_predicates():
    cases = D.extend_edge_cases()

    def buckets(run):
        label, mat, kw, items = run
        p = D.to_params(mat, **kw)
        return p, D.extend_buckets(items, p)

    (pa, a), (pb, b) = map(buckets, cases["bound_32000"])
    assert D.WIDE_BUCKET not in a and set(a) >= {0, 1, 2, 3, 4, 5} and set(b) == {D.WIDE_BUCKET}
    for (lab, mat, kw, items), bnd in zip(cases["bound_32000"], (31999, 32000)):
        assert all(D.bound_of(len(q), h0, pa) == bnd for q, _, h0, _ in items)
    (pa, a), (pb, b) = map(buckets, cases["tlen_1024"])
    assert all(x >= D.PAIR_BUCKET0 and x < D.WIDE_BUCKET for x in a) and len(set(a)) == 5
    assert all(x < D.PAIR_BUCKET0 for x in b)
    for key in ("e_del_17", "e_ins_17"):
        (pa, a), (pb, b) = map(buckets, cases[key])
        assert pa.pair_ok and not pb.pair_ok
        assert sum(x >= D.PAIR_BUCKET0 and x < D.WIDE_BUCKET for x in a) > 100
        assert all(x < D.PAIR_BUCKET0 for x in b)
    (pa, a), (pb, b) = map(buckets, cases["pair_cg_129"])
    assert (pa.pair_cg, pb.pair_cg) == (128, 129) and pa.pair_ok and not pb.pair_ok and not pa.lane_ok
    assert set(a) == {D.PAIR_BUCKET0, D.WIDE_BUCKET} and set(b) == {D.WIDE_BUCKET}
    assert min(a.count(D.PAIR_BUCKET0), a.count(D.WIDE_BUCKET)) >= 40  # both sides of bound + 127 <= 255
    for key in ("mat_min_17", "mat_max_16"):
        (pa, a), (pb, b) = map(buckets, cases[key])
        assert pa.lane_ok and not pb.lane_ok and pb.pair_ok
        assert any(x < D.PAIR_BUCKET0 for x in a) and any(x >= D.PAIR_BUCKET0 and x < D.WIDE_BUCKET for x in a)
        # outside [-16, 15] the pair path is still tested first: tiny tasks pair, the rest go wide
        assert set(b) <= set(range(D.PAIR_BUCKET0, D.WIDE_BUCKET + 1))
        assert D.WIDE_BUCKET in b and any(x < D.WIDE_BUCKET for x in b)
