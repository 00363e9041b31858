"""The scale inputs (tests/scale_cases.py) before any GPU is involved: every
vectorised reference equals the existing Python restatement on a 3,000-record
slice and the host oracle at the full size, the sparse-wide inputs through the
host oracles equal the restatements at the full window, every input meets the
conditions that keep its GPU test from passing vacuously, and the launch caps
the shapes are derived from are still what the .hip sources say."""
import ctypes as C

import numpy as np
import pytest

import bqsr_cases as B
import depth_cases as D
import fcship
import host_lib as H
import markdup_cases as M
import scale_cases as S
import ug_cases as U

L = H.lib
L.fcsg_depth_count.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
L.fcsg_depth_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_void_p,
                               C.c_void_p, C.c_void_p]
L.fcsg_ug_sites.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
L.fcsg_markdup.argtypes = [C.c_int64] + [C.c_void_p] * 9 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
L.fcsg_bqsr_count.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int, C.c_void_p,
                              C.c_void_p]
L.fcsg_bqsr_apply.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
SH, CAPS = S.SHAPES, S.CAPS
THREADS = 8


# ------------------------------------------------------------------ the caps
def test_the_launch_caps_are_what_the_shapes_were_derived_from():
    now = S.read_pinned()
    for name, (source, _, want, shapes) in S.PINNED.items():
        assert now[name] == want, (f"csrc/{source} no longer says {name} = {want} (found {now[name]!r}): update CAPS and look at "
                                   f"the shapes {shapes} in tests/scale_cases.py, so that they still cross the new cap")
    assert SH["ug_window"] == 524581 and SH["ug_tiles"] == 2050 and SH["ug_records"] == 524549 and SH["ug_pass"] == 65536
    assert SH["dp_window"] == 4195365 and SH["dp_tiles"] == 4098 and SH["dp_pieces"] == 33068
    assert SH["md_ends"] == 131125 and SH["md_all"] == 524549
    assert SH["bq_apply"] == 8205 and SH["bq_count"] == 67591 and SH["bq_count_slice"] == 34 and SH["bq_check"] == 524549
    assert [S.bq_replicas(k) for k in (1, 5, 6, 87, 88, 90)] == [16, 16, 14, 1, 1, 1]
    # a read group's cells: the fold kernel strides from six read groups on
    cells = B.NQ * (B.NCTX + B.NCYC)
    assert 5 * cells <= CAPS["bq_max_blocks"] * 256 < 6 * cells


# ------------------------------------------------------------------ depth
def host_depth(arrays, window, contig_len, prm, threads=THREADS):
    arrays = fcship.dp_arrays(*arrays)
    b = fcship.dp_batch(arrays)
    ref, start, length = window
    w = fcship.DpWindow(ref, 0, start, length, contig_len)
    p = fcship.dp_params(**prm)
    depth = np.zeros(length, np.uint32)
    H.check(L.fcsg_depth_count(C.addressof(b), C.addressof(p), C.addressof(w), threads, depth.ctypes.data))
    return depth


def host_stats(d, part, pieces, n_long, threads=THREADS):
    d, bits = np.ascontiguousarray(d, np.uint32), S.bitmap_np(part)
    pc = np.array([(s, e, li, 0) for s, e, li in pieces], fcship.DP_PIECE)
    hist, long_hist = np.zeros(D.BINS, np.uint64), np.zeros((max(n_long, 1), D.BINS), np.uint64)
    summary = np.zeros(len(pc), fcship.DP_SUMMARY)
    H.check(L.fcsg_depth_stats(d.ctypes.data, bits.ctypes.data, len(d), pc.ctypes.data, len(pc), n_long, threads,
                               hist.ctypes.data, long_hist.ctypes.data, summary.ctypes.data))
    return hist, long_hist[:n_long], S.summaries(summary)


def test_depth_reference_equals_the_restatement_and_the_host_path():
    f, window, clen = S.depth_many()
    want = S.depth_np(f, window, clen, S.DP_PRM)
    k = 3000
    span = int(f.pos[k - 1]) + 4
    head = D.depth(f.records(0, k, "dp"), (0, 0, span), clen, S.DP_PRM)[0]
    assert (head[:int(f.pos[k])] == want[:int(f.pos[k])]).all() and head.sum() > 1000
    part = D.depth(f.records(0, k, "dp"), (0, 100, 777), clen, D.params())[0]          # a clipped window, other parameters
    assert (part == S.depth_np(f, (0, 100, 777), clen, D.params())).all()
    assert (host_depth(f.dp(), window, clen, S.DP_PRM) == want).all()
    # distinct records, and enough of every kind
    assert f.n == SH["dp_records"] and (np.diff(f.pos) > 0).all() and want.max() >= 3 and (want == 0).sum() > 10000
    assert set(f.m) == {1, 2, 3} and (f.lead > 0).sum() > 1000 and (f.trail > 0).sum() > 1000 and f.absent.sum() > 100


def test_depth_statistics_reference_equals_the_restatement_and_the_host_path():
    depth, part, pieces, n_long = S.depth_pieces()
    assert S.bitmap_np(part[:5000]).tolist() == D.bitmap(part[:5000]).tolist()
    few = pieces[:400]
    a, b = S.stats_np(depth, part, few, n_long), D.stats(depth, part, few, n_long)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2]
    hist, long_hist, rows = S.stats_np(depth, part, pieces, n_long)
    h, lh, sm = host_stats(depth, part, pieces, n_long)
    assert (h == hist).all() and (lh == long_hist).all() and sm == rows
    # the conditions: more pieces than the kernel's grid, every quantile value, empty pieces, every long row in use
    assert len(pieces) == SH["dp_pieces"] > 8 * CAPS["dp_max_blocks"] and len(depth) == SH["dp_pieces_len"]
    assert {len(range(s, e)) for s, e, _ in pieces} == set(range(1, 71)) and depth.max() == 520
    short = [r for r, (_, _, li) in zip(rows, pieces) if li < 0]
    for k in ("q1", "median", "q3"):
        assert {1, 2, 3} <= {r[k] for r in short}
    assert sum(r["loci"] == 0 for r in rows) >= 100 and (long_hist.sum(axis=1) > 0).all() and hist[500] > 0


@pytest.fixture(scope="module")
def dp_sparse():
    return S.depth_sparse()


def test_depth_sparse_wide_through_the_host_path_and_its_conditions(dp_sparse):
    c = dp_sparse
    want, (_, start, W) = c["want"], c["window"]
    assert W == SH["dp_window"] and start % 2 == 1
    got = host_depth(D.flatten(c["records"]), c["window"], c["contig_len"], S.DP_PRM)
    assert (got == want).all()
    T = CAPS["dp_tile"]
    for b in c["bounds"] + [W - 37]:
        assert want[b - 1] > 0 and want[b] > 0, b          # both sides of the boundary
    # the scan's offset entering a tile is the depth of the locus before it
    assert want[256 * T - 1] > 0 and want[CAPS["dp_max_blocks"] * T - 1] > 0
    assert want[0] > 0 and want[W - 1] > 0 and want[:600].sum() > 1000 and want[W - 37:].sum() > 100
    edge = CAPS["dp_max_blocks"] * T
    off = D.depth(c["records"], c["window"], c["contig_len"], dict(S.DP_PRM, include_deletions=False))[0]
    assert (want[edge - 5:edge + 5] > off[edge - 5:edge + 5]).all()      # the deletion across 4,095|4,096 counts
    part, pieces = S.depth_sparse_part(W), S.depth_sparse_pieces(W)
    hist, long_hist, rows = S.stats_np(want, part, pieces, 2)
    h, lh, sm = host_stats(want, part, pieces, 2)
    assert (h == hist).all() and (lh == long_hist).all() and sm == rows
    short = D.stats(want, part, pieces[:4], 2)
    assert short[2] == rows[:4] and rows[0]["total"] > 0
    assert int(long_hist[0].sum()) == int(part.sum()) and long_hist[0][1:].sum() > 1000


def test_depth_high_coordinates_through_the_host_path():
    c = S.depth_high()
    on = D.params(include_deletions=True)
    for window in c["windows"]:
        want, beyond = D.depth(c["records"], window, c["contig_len"], on)
        assert not beyond and (host_depth(D.flatten(c["records"]), window, c["contig_len"], on) == want).all()
        assert want[-1] > 0 and want[0] > 0 and want.sum() > 400
        assert D.depth(c["records"] + [c["past"]], window, c["contig_len"], on)[1]
        with pytest.raises(RuntimeError, match="beyond its contig"):
            host_depth(D.flatten(c["records"] + [c["past"]]), window, c["contig_len"], on)
    assert c["windows"][0][1] + S.HIGH_WINDOW == c["contig_len"] == 2 ** 31 - 1 and c["windows"][1][1] % 2 == 1
    assert c["windows"][0][1] % 256 and c["windows"][1][1] % 256


# ------------------------------------------------------------------ ug
def host_sites(arrays, window, contig_len, ref_window, threads=THREADS):
    arrays = fcship.ug_arrays(*arrays)
    b = fcship.ug_batch(arrays)
    ref, start, length = window
    w = fcship.UgWindow(ref, 0, start, length, contig_len)
    p = fcship.UgParams(17)
    seq = np.ascontiguousarray(ref_window, np.uint8)
    assert len(seq) == length
    tab = np.array(S.TAB, np.int64)
    sites = np.zeros(length, fcship.UG_SITE)
    n = C.c_int64(-1)
    H.check(L.fcsg_ug_sites(C.addressof(b), C.addressof(p), C.addressof(w), seq.ctypes.data, tab.ctypes.data, threads,
                            sites.ctypes.data, length, C.addressof(n)))
    return sites[:n.value]


def test_ug_reference_equals_the_restatement_and_the_host_path():
    c = S.ug_many()
    f, (window,), clen = c["flat"], c["windows"], c["contig_len"]
    _, start, W = window
    want = S.sites_np(f, window, c["refs"][0], fcship.UG_SITE)
    lo = int(np.searchsorted(f.pos, start - 3100))
    small = (0, int(f.pos[lo]) + 3200, 4000)
    hi = int(np.searchsorted(f.pos, small[1] + small[2]))
    assert hi - lo >= 3000 and (f.skip[lo:hi] > 0).any()
    refstr = c["refs"][0].tobytes().decode()
    head = U.sites(f.records(lo, hi, "ug"), small, refstr, S.TAB)[0]
    assert len(head) > 500 and (S.site_rows(head, fcship.UG_SITE) == S.sites_np(f, small, c["refs"][0], fcship.UG_SITE)).all()
    got = host_sites(f.ug(), window, clen, c["refs"][0][start:start + W])
    assert len(got) == len(want) and (got == want).all()
    # the conditions
    assert f.n == SH["ug_records"] and W == SH["ug_many_window"] and start % 2 == 1 and (np.diff(f.pos) > 0).all()
    assert len(want) >= 50000
    end = S.ug_end(f, 0)
    tiles = np.array([end[k:k + 256].max() for k in range(0, f.n, 256)])
    assert len(tiles) == 2050 and (np.diff(tiles) > 0).sum() >= 2000
    running = np.maximum.accumulate(end)
    below = (end >= 0) & (end < running)
    in_window = (f.pos >= start) & (f.pos < start + W)
    assert (below & in_window).sum() > 500 and len(np.unique(tiles)) > 2000
    assert {int(x) for x in want["ref"]} == {0, 1, 2, 3} and (want["n"].sum(axis=1) >= 2).sum() > 1000
    # a maximum carried into the scan's passes 4 and 5 decides which records a tile walks: the far base of the record
    # that skips across the pass boundary is a site, in a tile that starts beyond the boundary's record
    offsets = set(want["offset"].tolist())
    for k in (3, 4):
        b = k * SH["ug_pass"]
        r = int(np.nonzero(f.skip[b - 110:b] > 0)[0][0]) + b - 110
        far = int(f.pos[r]) + 3001
        assert start <= f.pos[r] and far - start in offsets and running[b - 1] == end[r] > end[b + 1024]
        assert (far - start) // 256 * 256 + start > f.pos[b + 256]


def test_ug_interleaved_contigs_through_the_host_path():
    c = S.ug_many(interleaved=True)
    f = c["flat"]
    for window in c["windows"]:
        ref, start, W = window
        want = S.sites_np(f, window, c["refs"][ref], fcship.UG_SITE)
        got = host_sites(f.ug(), window, c["contig_len"], c["refs"][ref][start:start + W])
        assert len(want) > 20000 and len(got) == len(want) and (got == want).all()
    assert (f.ref_id == 1).sum() == f.n // 3


@pytest.mark.parametrize("start", [0, 1001])
def test_ug_sparse_wide_through_the_host_path_and_its_conditions(start):
    c = S.ug_sparse(start)
    want, (_, _, W) = c["want"], c["window"]
    assert W == SH["ug_window"]
    seq = np.frombuffer(c["refseq"][start:start + W].encode(), np.uint8)
    got = host_sites(U.flatten(c["records"]), c["window"], len(c["refseq"]), seq)
    assert (got == S.site_rows(want, fcship.UG_SITE)).all() and len(got) == len(want)
    tile = np.array([s["offset"] for s in want]) // 256
    for lo, hi in ((0, 256), (256, 512), (2047, 2048), (2048, 2049), (2049, 2050)):
        assert ((tile >= lo) & (tile < hi)).sum() >= 20, (lo, hi)
    offsets = {s["offset"] for s in want}
    assert 2048 * 256 in offsets and 2049 * 256 - 1 in offsets and W - 1 in offsets
    assert any(s["n_del"] > 0 for s in want if s["offset"] // 256 == 2048)
    assert "N" in c["refseq"][start + 65530:start + 65540] and not any(65530 <= o < 65545 for o in offsets)


def test_ug_high_coordinates_through_the_host_path():
    c = S.ug_high()
    refseq = c["refseq"]
    for window in c["windows"]:
        _, start, n = window
        want, beyond = U.sites(c["records"], window, refseq, S.TAB)
        seq = np.frombuffer(refseq[start:start + n].encode(), np.uint8)
        got = host_sites(U.flatten(c["records"]), window, len(refseq), seq)
        assert not beyond and (got == S.site_rows(want, fcship.UG_SITE)).all() and len(got) == len(want) > 60
        assert any(s["n_del"] for s in want) and want[-1]["offset"] >= n - 3 and want[0]["offset"] <= 2
        with pytest.raises(RuntimeError, match="beyond its contig"):
            host_sites(U.flatten(sorted(c["records"] + [c["past"]], key=lambda r: r["pos"])), window, len(refseq), seq)


# ------------------------------------------------------------------ markdup
def host_mark(arrays, n_ref, n_lib):
    arrays = fcship.dup_arrays(*arrays)
    n = len(arrays[0])
    dup, st = np.full(max(n, 1), 0xEE, np.uint8), np.zeros(4, np.int64)
    H.check(L.fcsg_markdup(n, *[a.ctypes.data for a in arrays], n_ref, n_lib, dup.ctypes.data, st.ctypes.data))
    return dup[:n], dict(zip(("examined", "pairs", "fragments", "duplicates"), map(int, st)))


def test_markdup_reference_equals_the_restatement_and_the_host_path():
    small = S.FlatDup(3000, 101)
    dup, st = S.markdup_np(small)
    records = small.records()
    assert list(dup) == M.expected(records) and st == M.stats(records) and 0.2 < dup.mean() < 0.5
    assert [a.tolist() for a in M.flatten(records)] == [np.asarray(a).tolist() for a in small.arrays()]
    for n, seed in ((SH["md_ends"], 102), (SH["md_all"], 103)):
        f = S.FlatDup(n, seed)
        dup, st = S.markdup_np(f)
        got, got_st = host_mark(f.arrays(), f.n_ref, f.n_lib)
        assert (got == dup).all() and got_st == st
        # the conditions
        assert f.n == n and 0.25 <= dup.mean() <= 0.45, dup.mean()
        assert st["pairs"] > n // 5 and st["fragments"] > n // 10 and st["examined"] < n - n // 50
        lo, hi = S.markdup_sets(f, dup)
        for edge in (CAPS["md_ends_blocks"] * 16, CAPS["md_max_blocks"] * 256):
            if edge < n:
                assert ((lo < edge) & (hi >= edge)).sum() >= 10, edge
        far = f.mate[f.mate >= 0].astype(np.int64) - np.nonzero(f.mate >= 0)[0]
        assert (np.abs(far) > n // 2).sum() > n // 20                   # mates lie anywhere in the batch


def test_markdup_high_bits_through_the_host_path():
    records = S.markdup_high_bits()
    want = M.expected(records)
    got, st = host_mark(M.flatten(records), S.MD_MAX_REFS, S.MD_MAX_LIBS)
    assert list(got) == want and st == M.stats(records)
    templates = sum(1 for i, r in enumerate(records) if r["mate"] < 0 or r["mate"] > i)
    assert templates == 64 and S.MD_MAX_REFS == fcship.FCSDUP_MAX_REFS and S.MD_MAX_LIBS == fcship.FCSDUP_MAX_LIBS
    assert {r["lib"] for r in records} >= {0, 1, 1 + (1 << 10), 2046}
    assert {r["ref"] for r in records} >= {0, 1, 1 + (1 << 20), S.MD_MAX_REFS - 2}
    assert {M.u5(r) for r in records} >= {-((1 << 30) - 1), -1, 0, 5, 5 + (1 << 29), (1 << 30) - 1}
    # keys that differ in one field keep their templates apart: of the first 15 fragment keys and the first 10 pair
    # keys the better-scored copy stays and the other is marked
    assert want[:30] == [1, 0] * 15
    assert want[30:70] == [1, 1, 0, 0] * 10
    assert want[70:78] == [1, 1, 0, 0, 1, 1, 1, 1]      # equal in all 117 bits: the best score, then the lower index
    # dropping any top bit would merge two of these sets
    def dropped(r, field, bit):
        return dict(r, **{field: r[field] & ~(1 << bit)})
    assert M.expected([dropped(r, "lib", 10) for r in records]) != want
    assert M.expected([dropped(r, "ref", 20) for r in records]) != want
    both = S.markdup_appended(M.random_batch(), records)
    got, st = host_mark(M.flatten(both), S.MD_MAX_REFS, S.MD_MAX_LIBS)
    assert list(got) == M.expected(both) and st == M.stats(both)


# ------------------------------------------------------------------ bqsr
def host_count(records, refs, known, n_rg, threads=THREADS):
    arrays = fcship.bq_arrays(*B.flatten(records))
    b = fcship.bq_batch(arrays)
    bases, off, bits = B.flat_reference(refs, known)
    ctx, cyc = B.new_tables(n_rg)
    H.check(L.fcsg_bqsr_count(C.addressof(b), bases.ctypes.data, off.ctypes.data, len(refs), bits.ctypes.data, n_rg,
                              threads, ctx.ctypes.data, cyc.ctypes.data))
    return ctx, cyc


@pytest.fixture(scope="module")
def bq_world():
    return S.bq_world()


@pytest.mark.parametrize("n_rg", SH["bq_rg"])
def test_bqsr_six_and_ninety_read_groups_through_the_host_path(bq_world, n_rg):
    refs, known = bq_world
    records, grouped, ctx, cyc = S.bq_count_case(refs, known, 1200, n_rg, 115, B.random_batch.__defaults__[-1])
    for batch in (records, grouped):
        got = host_count(batch, refs, known, n_rg)
        assert (got[0] == ctx).all() and (got[1] == cyc).all()
    assert (ctx[..., 0].sum(axis=(1, 2)) > 0).all() and (cyc[..., 0].sum(axis=(1, 2)) > 0).all()      # every read group
    assert S.bq_replicas(n_rg) == {6: 14, 90: 1}[n_rg] and [r["rg"] for r in records] != [r["rg"] for r in grouped]


def test_bqsr_count_of_67591_short_records_through_the_host_path(bq_world):
    refs, known = bq_world
    records, grouped, ctx, cyc = S.bq_count_case(refs, known, SH["bq_count"], 3, 112, (1, 2, 3))
    for batch in (records, grouped):
        got = host_count(batch, refs, known, 3)
        assert (got[0] == ctx).all() and (got[1] == cyc).all()
    assert len(records) == SH["bq_count"] and SH["bq_count_slice"] == 34 and cyc[..., 0].sum() > 20000 and ctx[..., 0].sum() > 5000
    assert cyc[..., 1].sum() > 1000 and {len(r["seq"]) for r in records} == {1, 2, 3}


def test_bqsr_apply_of_8205_records_through_the_host_path(bq_world):
    refs, known = bq_world
    records = B.random_batch(seed=113, n=SH["bq_apply"], n_rg=6, refs=refs, lengths=(1, 2, 30))
    tables = S.bq_tables(6)
    want = B.apply(records, *tables)
    arrays = fcship.bq_arrays(*B.flatten(records, 3))
    b = fcship.bq_batch(arrays)
    out = np.full(len(arrays[7]) + 5, 0xEE, np.uint8)
    H.check(L.fcsg_bqsr_apply(C.addressof(b), 6, tables[0].ctypes.data, tables[1].ctypes.data, tables[2].ctypes.data, THREADS,
                              out.ctypes.data))
    assert B.unflatten_quals(records, out, 3) == want and (out[:3] == 0xEE).all() and (out[-5:] == 0xEE).all()
    # the conditions
    old = arrays[8][3:]
    assert (out[3:-5] != old).mean() >= 0.30 and sum(1 for r in records if not B.applied(r)) >= 100
    assert sum(r["rg"] < 0 for r in records) > 10 and sum(r["qual"] is None for r in records) > 50


def test_bqsr_check_batch_names_one_read_group_too_many():
    arrays = S.bq_check_batch(3)
    assert len(arrays[0]) == SH["bq_check"] > CAPS["bq_max_blocks"] * 256
    assert np.nonzero(arrays[4] >= 3)[0].tolist() == [524300]
