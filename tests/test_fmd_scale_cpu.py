"""The inputs of test_fmd_scale_gpu.py (fmd_scale_cases.py), pinned without a GPU:

- the shapes follow from the launch caps test_scale_cpu.py pins to csrc/fmd_seed.hip and csrc/fmd_seeds.hip;
- the conditions under which batch A and batch B make every FMD kernel take a later trip, on the host index's
  answer alone, and batch A's lack of a period;
- the host index's answer equals the host build of the kernels' per-read code (tools/micro/fmd_smem_test.cpp and
  fmd_expand_test.cpp, with ASan and UBSan) on every planted read and 2,000 others;
- the vectorised expectation of fcs_fmd_seed's output equals the host's answer read by read, positions included.
"""
import numpy as np
import pytest

import fcship
import fmd_scale_cases as A
import fmd_seed_cases as S
import fmd_seeds_cases as F
import scale_cases as SC
from test_fmd_seed_cpu import figures as smem_figures, run, smem_exe  # noqa: F401  (smem_exe is a fixture)
from test_fmd_seeds_cpu import clean, expand_exe, figures as expand_figures  # noqa: F401

SH, CAPS = SC.SHAPES, SC.CAPS
U, E, O, N = A.U, A.E, A.O, A.N_READS


def counts(params=S.BWA):
    return np.diff(A.host(params)[1])


def test_the_shapes_cross_every_cap():
    assert (U, E, O) == (32768, 32768, 65536) and N == 65540 == O + 4
    assert N > O and N > 2 * U and N > 2 * E                      # order's second trip, collect's and expand's third
    assert SH["fmd_locate"] == SH["fmd_seed_locate"] == 524288 and SH["fmd_rows"] == 524545
    assert SH["fmd_scan_per"] == 65 and SH["fmd_scan_empty"] == 15   # lanes 1,009 to 1,023 of the scan sum nothing
    assert SH["fmd_scan_per"] * (CAPS["seed_scan_block"] - SH["fmd_scan_empty"]) >= N
    codes, q_off, q_len = A.batch_a()
    assert len(q_len) == N and int(q_len.max()) == A.MAX_READ and len(codes) == int(q_len.sum())
    assert np.array_equal(q_off, np.cumsum(q_len, dtype=np.int64) - q_len)


def test_batch_a_has_no_period():
    """Read r + T differs from read r in bases or length for every stride T of a kernel, the placed empty pairs apart:
    a slot that kept the read of the trip before would not pass for the next."""
    m = A.padded(A.batch_a())
    empty = set(A.kinds("empty"))
    for T in sorted(set(A.STRIDES)):
        same = np.nonzero((m[:-T] == m[T:]).all(axis=1))[0]
        assert all(int(r) in empty and int(r) + T in empty for r in same), (T, same[:8])
    # reads with and without SMEMs alternate irregularly: neither kind is rare
    assert 0.1 < np.mean(counts() == 0) < 0.9


def test_conditions_on_the_host_answer():
    mems, mem_off, loc, loc_off, stats = A.host()
    c, c1 = counts(), counts(A.MIN1)
    assert stats == [0, 0, 0]
    # fmd_seed_locate_kernel strides: more rows than one launch's lanes, and they fit the capacities the tests pass
    assert loc_off[-1] > SH["fmd_seed_locate"], loc_off[-1]
    assert mem_off[-1] <= 16 * N and loc_off[-1] <= 64 * N          # the aligner's first capacities: no repeat
    # the reads the device hands back: at the default max_mems the deep reads, at SMALL_MEMS those and the planted ones
    deep, over = A.kinds("deep"), A.kinds("over")
    assert list(np.nonzero(c > S.MAX_MEMS_DEFAULT)[0]) == deep == list(np.nonzero(c1 > S.MAX_MEMS_DEFAULT)[0])
    assert list(np.nonzero(c > A.SMALL_MEMS)[0]) == sorted(deep + over)
    assert all(A.SMALL_MEMS < c[r] <= S.MAX_MEMS_DEFAULT for r in over)
    assert sum(r > U for r in over) == 3 and sum(r > O for r in over) == 1 and max(c) <= 4096
    # a deep and a shallow read share a quad of the collect grid, in both orders, one trip apart
    pairs = [(r, r + U) for r in deep + A.kinds("shallow") if r + U in A.planted_reads()]
    first = {A.planted_reads()[a][0] for a, _ in pairs}
    assert len(pairs) == 8 and first == {"deep", "shallow"}
    assert all({A.planted_reads()[a][0], A.planted_reads()[b][0]} == {"deep", "shallow"} for a, b in pairs)
    assert all(c[r] > 0 for r in A.kinds("shallow"))
    # the multi-tile read, in the order kernel's second round, between one-tile reads; the first round's are one-tile
    (tile,) = A.kinds("tile")
    assert tile == O + 1 and 64 < c1[tile] <= S.MAX_MEMS_DEFAULT
    assert 0 < c1[O] <= 64 and 0 < c1[O + 2] <= 64 and c1[O + 3] == 0
    assert (c1[:O][c1[:O] <= S.MAX_MEMS_DEFAULT] <= 64).all() and all(0 < c1[r] <= 64 for r in range(4))
    # the seams: the last read of a trip and the first of the next have no SMEM, under either parameter set
    empty = A.kinds("empty")
    assert {U - 1, U, E - 1, E, O - 1, N - 1} <= set(empty)
    assert all(c[r] == 0 and c1[r] == 0 for r in empty)
    q_len = A.batch_a()[2]
    assert {int(q_len[r]) == 0 for r in empty} == {True, False}     # zero-length and all-N reads


def test_array_hook_is_the_string_hook():
    """seeds_np on a slice of the arrays equals F.seeds on the same reads as strings."""
    idx = sorted(set(A.planted_reads()) | set(range(0, N, 331)))
    got = A.seeds_np(A.ref(), A.sub_batch(A.batch_a(), idx), F.HOST)
    want = F.seeds(A.ref(), A.strings(A.batch_a(), idx), F.HOST, mem_cap=1 << 18, loc_cap=1 << 20)
    assert np.array_equal(got[0], np.concatenate(want[0])) and np.array_equal(got[2], np.concatenate(want[1]))
    assert list(np.diff(got[1])) == [len(m) for m in want[0]] and list(np.diff(got[3])) == [len(x) for x in want[1]]
    # and the whole batch's answer restricted to the slice is the slice's answer: reads are independent on the host
    mems, mem_off = A.host()[:2]
    assert np.array_equal(got[0], np.concatenate([mems[mem_off[r]:mem_off[r + 1]] for r in idx]))


@pytest.fixture(scope="module")
def the_slice(tmp_path_factory):
    """Every planted read and 2,000 of the others, as the micro tools' input file."""
    idx = sorted(set(A.planted_reads()) | set(range(7, N, N // 2000)))
    path = tmp_path_factory.mktemp("fmdscale") / "slice.txt"
    S.write_tool_input(path, A.ref(), A.strings(A.batch_a(), idx))
    return idx, path


def slice_total(idx, params):
    return int(counts(params)[idx].sum())


def test_host_answer_is_the_shared_collect_code(smem_exe, the_slice):  # noqa: F811
    """tools/micro/fmd_smem_test.cpp: fmd_smem.h's collect and LF walk, built for the host, against FmdIndex on the
    slice; the SMEM totals it prints are the hook's."""
    idx, path = the_slice
    assert len(idx) >= 2000 + len(A.planted_reads()) - 30
    r = run(smem_exe, path)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    rows = smem_figures(r.stdout)
    for params in (S.BWA, A.MIN1):
        row = rows[(1, params[0], params[1], params[3])]
        assert row["reads"] == len(idx) and row["smems"] == slice_total(idx, params), (params, row)
    assert rows[(1, 19, 28, 20)]["max_depth"] == 100 and rows[(1, 19, 28, 20)]["max_smems"] == 2700
    assert all(rows[(intv, 19, 28, 20)]["located"] > 0 for intv in (4, 7, 32))


def test_host_answer_is_the_shared_expand_code(expand_exe, the_slice):  # noqa: F811
    """tools/micro/fmd_expand_test.cpp: fmd_expand.h's ranks, row counts and sampled rows against std::stable_sort and
    bwa's sampling loop on the slice; the SMEM and row totals it prints are the hook's."""
    idx, path = the_slice
    r = run(expand_exe, path, 500)
    clean(r)
    row = expand_figures(r.stdout)[(500, 19, 28, 20)]
    loc_off = A.host()[3]
    assert row["reads"] == len(idx) and row["smems"] == slice_total(idx, S.BWA)
    assert row["rows"] == int(np.diff(loc_off)[idx].sum())


def test_flat_expectation_is_the_host_answer():
    """flat(): mems, mem_off, row_off and the positions read through the full suffix array, mapped to (contig, offset,
    strand) as the aligner maps them, equal the host's lists for the whole batch."""
    mems5, mem_off, loc, loc_off, _ = A.host()
    mems, off, pos, row_off = A.flat(mems5, mem_off, A.sa_full())
    assert np.array_equal(off, mem_off) and np.array_equal(row_off, loc_off) and len(pos) == len(loc)
    for j, f in enumerate(("qb", "qe", "s", "k", "l")):
        assert np.array_equal(mems[f], mems5[:, j])
    kept = np.minimum(mems5[:, 2], 500)
    length = np.repeat(mems5[:, 1] - mems5[:, 0], kept)
    assert np.array_equal(A.text_map(pos, length, A.ref()), loc)
    # dropped reads leave empty ranges and move the later offsets
    deep = A.kinds("deep")
    d = A.flat(mems5, mem_off, A.sa_full(), dropped=deep)
    c = np.diff(mem_off)
    assert d[1][-1] == mem_off[-1] - c[deep].sum() and all(d[1][r] == d[1][r + 1] and d[3][r] == d[3][r + 1] for r in deep)
    keep = np.ones(N, bool)
    keep[deep] = False
    assert np.array_equal(d[0], mems[np.repeat(keep, c)]) and np.array_equal(np.diff(d[3])[keep], np.diff(loc_off)[keep])


def test_batch_b():
    """rows[i] = i * 7919 mod n_rows never repeats one trip later; the three planted rows are in the wrapped tail; the
    expected positions are the full suffix array's and the statuses those test_locate_step_cap_and_bad_rows pins."""
    b = A.batch_b()
    rows, L = b["rows"], SH["fmd_locate"]
    assert len(rows) == SH["fmd_rows"] == L + 257
    assert (rows[:257] != rows[L:]).all() and (rows[:L] >= 0).all() and (rows[:L] < b["n_rows"]).all()
    assert np.gcd(7919, b["n_rows"]) == 1 and b["n_rows"] > 257
    assert rows[b["bad_at"][0]] == -1 and rows[b["bad_at"][1]] == b["n_rows"] and min(b["bad_at"]) >= L
    assert b["far_at"] >= L and rows[b["far_at"]] == b["far"] and b["steps"][b["far"]] >= A.FAR_STEPS
    st = b["status"]
    assert [st[i] for i in b["bad_at"]] == [fcship.FCS_FMD_BAD_ROW] * 2 and st[b["far_at"]] == fcship.FCS_FMD_STEP_CAP
    assert (st == fcship.FCS_FMD_BAD_ROW).sum() == 2 and 0 < (st == fcship.FCS_FMD_LOCATED).sum() < len(st)
    ok = st == fcship.FCS_FMD_LOCATED
    assert np.array_equal(b["pos"][ok], A.sa_full()[rows[ok]])
    # a stored row is sampled or special: 0 steps; no walk is longer than 32 * sa_intv, the default cap
    assert b["steps"].max() < 32 * A.SA_INTV and (b["steps"][::A.SA_INTV] == 0).all()
