"""The batches of tests/test_phmm_grid_gpu.py and tests/test_bsw_grid_gpu.py,
checked without a GPU: each one exceeds the workgroup cap parsed from the
source by the margin its test relies on, the pairs of a second trip have the
properties the tests are after, and the oracle is finite where they expect it.
"""
import numpy as np
import pytest

import bsw_grid_cases as B
import phmm_grid_cases as P
import sw_dispatch as D


def test_caps_are_named_and_parsed():
    assert P.cap("phmm_kernels.hip", "kStreamGridCap") == 65536
    assert P.cap("phmm_kernels.hip", "kOneGridCap") == 65536
    assert P.cap("phmm_kernels.hip", "kFallbackGroups") == 2048
    assert P.cap("phmm_kernels.hip", "kRescueWaves") == 4096
    assert P.cap("phmm_kernels.hip", "kRescueGroups") == 2048
    assert P.cap("bsw_kernels.hip", "kExtendWideGrid") == 2048
    assert P.cap("bsw_kernels.hip", "kGlobalGrid") == 2048
    assert P.cap("bsw_align.hip", "kAlignGridCap") == 1 << 20
    # each name is what its launch uses
    src = P.source("phmm_kernels.hip")
    assert src.count(", 1), kStreamGridCap);") == 3
    assert "if (grid > kOneGridCap) grid = kOneGridCap;" in src
    assert "std::min<long long>(groups, kFallbackGroups)" in src
    assert "std::min<long long>(max_count, kRescueWaves)" in src
    bsw = P.source("bsw_kernels.hip")
    assert "if (grid > kExtendWideGrid) grid = kExtendWideGrid;" in bsw
    assert "if (grid > kGlobalGrid) grid = kGlobalGrid;" in bsw
    al = P.source("bsw_align.hip")
    assert 'std::getenv("FCSHIP_ALIGN_GRID")' in al and al.count("align_grid_cap())") == 2


def test_class_edges_as_restated():
    assert P.stream_class_hmax() == [224, 300, 472, 3700]
    assert P.cols_hmax() == [303, 271, 255, 239, 223, 207, 191, 175]
    assert P.launch_class(33, 304) == ("long", 1) and P.launch_class(33, 303) == ("cols", 0)
    assert P.launch_class(33, 472) == ("long", 1) and P.launch_class(33, 473) == ("long", 0)
    assert P.launch_class(32, 400) == ("grouped", None)
    assert P.launch_class(40, 192) == P.launch_class(40, 207) == ("cols", 5)
    assert P.launch_class(40, 191) == ("cols", 6) and P.launch_class(40, 100) == ("cols", 7)


def one_class(case):
    cls = {P.launch_class(int(r), int(h)) for r, h in zip(case.read_len(), case.hap_len())}
    assert len(cls) == 1, cls
    return cls.pop()


def shortest_kinds(case):
    """Kinds of the unique pairs at the class's shortest haplotype length that
    the large batch repeats, and how many of its pairs have that length."""
    hl = case.hap_len()
    at = np.flatnonzero(hl == hl.min())
    used = np.intersect1d(at, np.unique(case.sel))
    return used, [case.kinds[u] for u in used], int(np.isin(case.sel, at).sum())


STREAM = [("k1", 1, ("long", 1)), ("k2", 2, ("long", 1)), ("k1_long0", 1, ("long", 0))]


@pytest.mark.parametrize("which,K,cls", STREAM)
def test_phmm3_batches_take_a_second_trip(which, K, cls):
    case = P.phmm3_case(which)
    g = P.cap("phmm_kernels.hip", "kStreamGridCap")
    n = case.sel.size
    assert one_class(case) == cls
    assert n > g * 4 * K
    nb_head, nbatch = P.stream_batches(n, K, P.phmm3_tail(cls[1]), 4)
    assert nbatch > g + 300
    if K > 1:
        assert nb_head > g + 64  # second trips in K-pair head batches too
    else:
        assert n % 4 == 3  # a ragged last batch
        assert n > 4 * P.cap("phmm_kernels.hip", "kOneGridCap")  # launch_one's groups with exact
    late = P.second_trip_pairs(n, K, P.phmm3_tail(cls[1]), 4, g)
    used, kinds, n_short = shortest_kinds(case)
    assert n_short >= late + 4096, (n_short, late)  # the second trip holds the shortest length only
    have = set().union(*kinds)
    assert {"odd_r", "even_r", "min_r", "read_n", "hap_n", "unrelated", "odd_hap"} <= have
    ref, used_d = case.oracle
    assert np.isfinite(ref).all()
    assert any(used_d[u] and "unrelated" in case.kinds[u] for u in used), "a rescue from a second-trip batch"
    assert not used_d[[u for u in used if "unrelated" not in case.kinds[u]]].any()
    assert (~used_d).sum() > 0.9 * used_d.size  # the fp32 result is what most pairs report


def test_column_batches_take_a_second_trip():
    case = P.cols_case()
    g = P.cap("phmm_kernels.hip", "kStreamGridCap")
    n = case.sel.size
    assert one_class(case) == ("cols", 5)
    assert n > 8 * g > 4 * g
    assert P.stream_batches(n, 1, P.PHMM5_FORCED_TAIL, 4)[1] > 2 * g
    nb_head, nbatch = P.stream_batches(n, 1, P.PHMM4_TAIL, 8)
    assert nb_head > g + 64 and nbatch > g + 300
    late = P.second_trip_pairs(n, 1, P.PHMM4_TAIL, 8, g)
    used, kinds, n_short = shortest_kinds(case)
    assert n_short >= late + 4096
    assert {"odd_r", "even_r", "min_r", "read_n", "hap_n", "unrelated", "odd_hap"} <= set().union(*kinds)
    ref, used_d = case.oracle
    assert np.isfinite(ref).all()
    assert any(used_d[u] and "unrelated" in case.kinds[u] for u in used)


def test_fallback_batch_exceeds_its_groups():
    case = P.fallback_case()
    g = P.cap("phmm_kernels.hip", "kFallbackGroups")
    odd = np.array(["odd_hap" in k for k in case.kinds])
    n_odd = int(odd[case.sel].sum())
    assert n_odd > 4 * g + 100 and n_odd % 4 == 3
    assert abs(case.sel.size - 2 * n_odd) <= 1  # about as many clean pairs
    # every odd haplotype really holds a byte outside ACGTN, no clean one does
    for (r, h), k in zip(case.unique, case.kinds):
        assert ("odd_hap" in k) == bool((~np.isin(case.haps[h], np.frombuffer(b"ACGTN", np.uint8))).any())
    cls = {P.launch_class(int(r), int(h)) for r, h in zip(case.read_len()[odd], case.hap_len()[odd])}
    assert cls == {("cols", 6), ("cols", 2), ("long", 1)}
    assert case.read_len().min() >= 33
    ref, used_d = case.oracle
    assert np.isfinite(ref).all()
    assert (used_d & odd).sum() > 0, "a handed-back pair that the fallback underflows"
    assert np.array_equal(used_d, np.array(["unrelated" in k for k in case.kinds]))
    assert np.unique(case.sel).size == len(case.unique)


def test_rescue_batch_exceeds_its_waves():
    case = P.rescue_case()
    g = P.cap("phmm_kernels.hip", "kRescueWaves")
    assert case.sel.size == g + 77
    assert np.unique(case.sel).size == len(case.unique)
    rl, hl = case.read_len(), case.hap_len()
    assert rl.min() == 1 and rl.max() == 70 and {63, 64, 65} <= set(rl.tolist())
    assert hl.min() == 1 and hl.max() == 80
    ref = P.rescue_reference(case)
    assert np.isfinite(ref).all()


@pytest.mark.parametrize("long_queries", [False, True])
def test_extend_wide_batches_exceed_the_cap(long_queries):
    case = B.extend_wide_case(long_queries)
    g = P.cap("bsw_kernels.hip", "kExtendWideGrid")
    bk = np.array(D.extend_buckets(case.items, case.params))
    assert (bk == D.WIDE_BUCKET).all()
    assert (bk[case.sel] == D.WIDE_BUCKET).sum() > g + 200
    assert np.unique(case.sel).size == len(case.items)
    ql = np.array([len(i[0]) for i in case.items])
    assert (ql.max() > 255) == long_queries  # bsw_extend_kernel<16> or <4>
    assert {62, 63, 64, 127, 128, 191, 192, 254, 255} <= set(ql.tolist())
    if long_queries:
        assert {256, 319, 320, 447, 448, 510, 511, 512} <= set(ql.tolist())
    h0 = np.array([i[2] for i in case.items])
    assert (h0 > 0).all() and ((h0 + ql >= 32000) & (ql < 128)).any() and ((h0 < 300) & (ql < 152)).any()


def test_global_batch_exceeds_the_cap_with_mixed_probes():
    case = B.global_case()
    g = P.cap("bsw_kernels.hip", "kGlobalGrid")
    n = case.sel.size
    assert n > 64 * g + 64 * 40 and n % 64 == 17
    lanes, waves = B.probe_mix(case)
    assert lanes.size == g + 41
    assert (lanes[g:] > 0).all() and (waves[g:] > 0).all(), "every second-trip probe holds both kinds"
    assert 0.3 < case.lane.mean() < 0.7
    ql = np.array([len(i[0]) for i in case.items])
    tl = np.array([len(i[1]) for i in case.items])
    assert ql.min() >= 4 and ql.max() <= 40 and tl.min() >= 4 and tl.max() <= 40


@pytest.mark.parametrize("name", sorted(B.ALIGN_BATCHES))
def test_align_batches_stride_under_the_forced_cap(name):
    case = B.align_batch(name)
    assert B.ALIGN_FORCED_GRID < P.cap("bsw_align.hip", "kAlignGridCap")
    trips = B.align_trips(case, B.ALIGN_FORCED_GRID)
    want = {"u8": {"pk", "w64"}, "i16": {"pk", "w64"}, "long_windows": {"w64"}, "e_ins_12": {"w16"}}[name]
    assert want <= set(trips), trips
    assert all(trips[k] >= 3 for k in want), trips
    if name == "e_ins_12":
        assert not case.plan.packed and case.plan.second_launch
    ql = max(len(i[0]) for i in case.items)
    assert (ql + 15 <= 256) == (name != "i16")  # both 64-lane instantiations
