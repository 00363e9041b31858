"""Depth of coverage (DESIGN §2 [EXT], §4.11): what needs no GPU.

- The hand cases, each with its expected depths written out, against the Python
  restatement (tests/depth_cases.py) and the host path (host/depth.cpp through
  fcsg_depth_*), at windows of 4,096 loci and of the whole contig on the
  random batches.
- csrc/dp_runs.h, the text the kernels run, compiled for the host with ASan and
  UBSan as a stand-alone program (tools/micro/depth_test.cpp), gives the depths
  and summaries of host/depth.cpp.
- The depth command with the CPU mock of libfcship (the host path) writes the
  restatement's bytes.
- fcsdp_* is declared in include/fcsdp.h and exported, beside an unchanged
  fcship.h surface; bad arguments are refused before any device is looked for.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import depth_cases as D
import fcship
import host_lib as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = D.hand_cases()
L = H.lib
L.fcsg_depth_count.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
L.fcsg_depth_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_void_p,
                               C.c_void_p, C.c_void_p]
L.fcsg_text_to_bam.argtypes = [C.c_char_p] * 4
SUFFIXES = ["", ".sample_summary", ".sample_statistics", ".sample_cumulative_coverage_counts",
            ".sample_cumulative_coverage_proportions", ".sample_interval_summary", ".sample_interval_statistics"]


def host_depth(records, window, contig_len, prm=None, threads=1, first_offset=0, depth=None):
    arrays = fcship.dp_arrays(*D.flatten(records, first_offset))
    b = fcship.dp_batch(arrays)
    ref, start, length = window
    w = fcship.DpWindow(ref, 0, start, length, contig_len)
    p = fcship.dp_params(**(prm or D.params()))
    depth = np.zeros(length, np.uint32) if depth is None else depth
    H.check(L.fcsg_depth_count(C.addressof(b), C.addressof(p), C.addressof(w), threads, depth.ctypes.data))
    return depth


def host_stats(d, part, pieces, n_long=0, threads=1):
    d = np.ascontiguousarray(d, np.uint32)
    bits = D.bitmap(part)
    pc = np.array([(s, e, li, 0) for s, e, li in pieces], fcship.DP_PIECE)
    hist, long_hist = np.zeros(D.BINS, np.uint64), np.zeros((max(n_long, 1), D.BINS), np.uint64)
    summary = np.zeros(len(pc), fcship.DP_SUMMARY)
    H.check(L.fcsg_depth_stats(d.ctypes.data, bits.ctypes.data, len(d), pc.ctypes.data, len(pc), n_long, threads,
                               hist.ctypes.data, long_hist.ctypes.data, summary.ctypes.data))
    return hist, long_hist[:n_long], summary


def same_summaries(got, want):
    return [{k: int(g[k]) for k in ("total", "loci", "above", "q1", "median", "q3")} for g in got] == want


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_case(case):
    want = D.want_depths(case)
    clen = D.LENS[case["window"][0]]
    d, beyond = D.depth(case["records"], case["window"], clen, case["prm"])
    assert (d == want).all() and beyond == case["beyond"]
    if case["beyond"]:   # the host path refuses the record and adds nothing
        got = np.full(len(want), 7, np.uint32)
        with pytest.raises(RuntimeError, match="record 0 has an aligned base beyond its contig"):
            host_depth(case["records"], case["window"], clen, case["prm"], depth=got)
        assert (got == 7).all()
    else:
        assert (host_depth(case["records"], case["window"], clen, case["prm"]) == want).all()


def test_the_list_of_hand_cases_is_the_issue_s():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names) == 34
    for must in ("op_m", "op_eq", "op_x", "op_i", "op_d", "op_n", "op_s", "op_h", "op_p", "clips", "deletion_off", "deletion_on",
                 "skip", "insertion", "reverse", "flags", "mapq_bounds", "baseq_bounds", "absent_qualities_min_0",
                 "absent_qualities_min_1", "read_base_n", "starts_before_window", "ends_after_window", "covers_window",
                 "ends_at_contig_end", "ends_one_past_contig_end"):
        assert must in names
    flags = next(c for c in CASES if c["name"] == "flags")["records"]
    assert [r["flag"] for r in flags[:5]] == [0x4, 0x100, 0x200, 0x400, 0x800]


@pytest.fixture(scope="module")
def world():
    return D.random_world()


@pytest.fixture(scope="module")
def built(world):
    """[(records, params, first quality offset, the restatement's depths per contig)] of the built batches."""
    out = []
    for records, prm, first in ((D.random_batch(world), D.params(), 0),
                                (D.random_batch(world, seed=12, n=600), D.params(20, 60, 10, 40, True), 1),
                                (D.sweep_batch(world), D.params(min_baseq=5), 3), (D.copies_batch(), D.params(), 0)):
        out.append((records, prm, first, [D.depth(records, (c, 0, len(s)), len(s), prm)[0] for c, s in enumerate(world)]))
    return out


def test_host_path_equals_the_restatement_on_built_batches(world, built):
    for records, prm, first, want in built:
        assert sum(int(w.sum()) for w in want) > 5000
        for c, seq in enumerate(world):
            n = len(seq)
            assert (host_depth(records, (c, 0, n), n, prm, first_offset=first) == want[c]).all()
            for start in range(0, n, 4096):   # records straddle the windows and are clipped to each
                length = min(4096, n - start)
                got = host_depth(records, (c, start, length), n, prm, first_offset=first)
                assert (got == want[c][start:start + length]).all()
                assert (D.depth(records, (c, start, length), n, prm)[0] == got).all()
    records, prm, _, want = built[0]
    n = len(world[0])
    d = host_depth(records * 3, (0, 0, n), n, prm, threads=4)   # slices on several threads sum to the same depths
    assert (d == 3 * want[0]).all()
    host_depth(records, (0, 0, n), n, prm, depth=d)             # two calls add up
    assert (d == 4 * want[0]).all()
    top = built[3][3][0]
    assert {499, 500, 501} <= set(int(v) for v in top) and int(D.histogram(top)[500]) == 20 and int(D.histogram(top)[499]) == 10


def test_host_statistics_equal_the_restatement(world, built):
    d, part, pieces, want_hist, want = D.stats_hand()
    for fn in (D.stats, host_stats):
        hist, _, summary = fn(d, part, pieces)
        assert {k: int(v) for k, v in enumerate(hist) if v} == want_hist
        assert same_summaries(summary, [want]) if fn is host_stats else summary == [want]
    depth = built[3][3][0].copy()
    depth[2000:6000] = built[0][3][0][2000:6000]
    part = [ch not in "Nn" for ch in world[0]]
    assert not all(part)
    pieces, s = [], 0
    for n, li in zip([1, 63, 64, 65, 255, 256, 257, 1000, 3000, 0, 2000], [-1, -1, -1, -1, -1, -1, -1, 0, 0, -1, 1]):
        pieces.append((s, s + n, li))
        s += n
    hist, long_hist, summary = D.stats(depth, part, pieces, 2)
    for threads in (1, 3):
        h, lh, sm = host_stats(depth, part, pieces, 2, threads)
        assert (h == hist).all() and (lh == long_hist).all() and same_summaries(sm, summary)
    assert long_hist.sum() > 0 and hist[500] > 0 and any(row["above"] for row in summary)
    assert D.quantile(np.zeros(D.BINS, np.uint64), 2) == 1 and summary[9] == dict(total=0, loci=0, above=0, q1=1, median=1, q3=1)
    with pytest.raises(RuntimeError, match="piece 0"):
        host_stats(depth, part, [(0, 65537, -1)])


def test_host_path_refuses_bad_batches():
    d = np.full(40, 7, np.uint32)
    r = D.rec(0, 1, 5, "10M")
    r["n_bases"] = 9
    r["qual"] = r["qual"][:9]
    with pytest.raises(RuntimeError, match="CIGAR of record 1 does not cover"):
        host_depth([D.rec(0, 1, 0, "4M"), r], (1, 0, 40), 40, depth=d)
    with pytest.raises(RuntimeError, match="beyond its contig"):
        host_depth([D.rec(0, 1, -1, "4M")], (1, 0, 40), 40, depth=d)
    assert (d == 7).all()
    with pytest.raises(D.Refused):
        D.depth([r], (1, 0, 40), 40)


# ------------------------------------------------------------------ dp_runs.h on the host, under sanitizers
@pytest.fixture(scope="module")
def runs_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("dpr") / "depth_test"
    pkg = os.path.join(ROOT, "falcon-genome_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(pkg, "csrc"), "-I" + os.path.join(pkg, "host"),
                    os.path.join(ROOT, "tools", "micro", "depth_test.cpp"), os.path.join(pkg, "host", "depth.cpp"),
                    "-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("seed,records", [(1, 3000), (2, 300), (3, 0), (4, 1)])
def test_shared_runs_host_build_equals_the_host_rules(runs_exe, seed, records):
    r = subprocess.run([str(runs_exe), str(seed), str(records)], capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "MISMATCH" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    if records >= 300:
        fig = dict(zip(r.stdout.split()[0::2], r.stdout.split()[1::2]))
        assert int(fig["counted_bases"]) > int(fig["run_ends"]) > 0 and int(fig["loci"]) > 0


# ------------------------------------------------------------------ the ABI
def last_error():
    return fcship.lib.fcs_last_error().decode()


def test_symbols_declared_and_exported_beside_an_unchanged_fcship_h():
    names = ["fcsdp_count", "fcsdp_runs_dev", "fcsdp_scan_dev", "fcsdp_stats", "fcsdp_stats_dev", "fcsdp_workspace_bytes"]
    assert fcship.dp_header_symbols() == names
    nm = subprocess.run(["nm", "-D", "--defined-only", fcship.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("fcsdp_")}
    assert exported == set(names)
    assert fcship.lib.fcs_abi_symbol_count() == len(fcship.header_symbols()) == 61
    assert not [s for s in fcship.header_symbols() if "dp" in s.split("_")]
    assert C.sizeof(fcship.DpBatch) == 13 * 8 and C.sizeof(fcship.DpWindow) == 32 and C.sizeof(fcship.DpParams) == 20
    assert fcship.DP_PIECE.itemsize == 16 and fcship.DP_SUMMARY.itemsize == 32
    mock = subprocess.run(["nm", "-D", "--defined-only", f"{ROOT}/tests/cpu_mock/build/libfcship.so"],
                          capture_output=True, text=True).stdout
    assert "fcs_phmm" in mock and "fcsdp_" not in mock


def test_arguments_are_checked_before_the_device():
    records = [D.rec(0, 0, 10 * k, "10M") for k in range(4)]
    arrays = fcship.dp_arrays(*D.flatten(records))
    depth = np.full(300, 7, np.uint32)
    prm = fcship.dp_params()

    def swapped(k, values):
        a = list(arrays)
        a[k] = np.ascontiguousarray(values, arrays[k].dtype)
        return tuple(a)

    def count(a=arrays, window=(0, 0, 300, 300), p=prm, **kw):
        b = fcship.dp_batch(a, **kw)
        w = fcship.DpWindow(window[0], 0, *window[1:])
        return fcship.lib.fcsdp_count(99, C.addressof(b), C.addressof(p), C.addressof(w), depth.ctypes.data), last_error()

    for kw, what in ((dict(n=-1), "negative record count"),
                     (dict(a=swapped(7, [0, 10, 9, 30, 40])), "base offsets out of order at record 1"),
                     (dict(a=swapped(5, [0, 1, 2, 1, 4])), "CIGAR offsets out of order at record 2"),
                     (dict(n_bases=39), "base offsets end at 40, beyond the 39 given"),
                     (dict(window=(0, 0, 301, 300)), "lies outside its contig of 300 bases"),
                     (dict(window=(-1, 0, 300, 300)), "window ref_id -1"),
                     (dict(window=(0, 0, (1 << 30) + 1, 1 << 31)), "loci (at most 1073741824)"),
                     (dict(p=fcship.dp_params(min_mapq=5, max_mapq=4)), "a lower bound above its upper bound"),
                     (dict(a=swapped(2, [0, 10, 295, 30])), "record 2 has an aligned base beyond its contig"),
                     (dict(a=swapped(4, [10 << 4, 10 << 4, 9 << 4, 10 << 4])), "the CIGAR of record 2 does not cover its bases")):
        rc, err = count(**kw)
        assert rc == fcship.FCS_ERR_INVALID and "[E::fcsdp_count]" in err and what in err, (kw, err)
        assert (depth == 7).all(), kw
    b = fcship.dp_batch(arrays)
    w = fcship.DpWindow(0, 0, 0, 300, 300)
    assert fcship.lib.fcsdp_count(0, None, C.addressof(prm), C.addressof(w), depth.ctypes.data) == fcship.FCS_ERR_INVALID
    assert "null batch" in last_error()
    assert fcship.lib.fcsdp_count(0, C.addressof(b), None, C.addressof(w), depth.ctypes.data) == fcship.FCS_ERR_INVALID
    assert "null parameters" in last_error()
    # a good batch on a device that is not there: the device error comes after every check
    rc, err = count()
    assert rc in (fcship.FCS_ERR_INVALID, fcship.FCS_ERR_DEVICE) and "[E::fcsdp_count]" not in err and (depth == 7).all()
    # an empty batch and an empty window need no device
    e = fcship.dp_batch(fcship.dp_arrays([], [], [], [], [], [0], [], [0], []))
    assert fcship.lib.fcsdp_count(99, C.addressof(e), C.addressof(prm), C.addressof(w), depth.ctypes.data) == 0
    w0 = fcship.DpWindow(0, 0, 10, 0, 300)
    assert fcship.lib.fcsdp_count(99, C.addressof(b), C.addressof(prm), C.addressof(w0), None) == 0
    # the statistics
    d, bits = np.zeros(100, np.uint32), D.bitmap([1] * 100)
    hist, summary = np.full(D.BINS, 7, np.uint64), np.zeros(2, fcship.DP_SUMMARY)

    def stats(pieces, n_long=0, length=100):
        pc = np.array(pieces, fcship.DP_PIECE)
        return fcship.lib.fcsdp_stats(99, d.ctypes.data, bits.ctypes.data, length, pc.ctypes.data, len(pc), n_long,
                                      hist.ctypes.data, hist.ctypes.data, summary.ctypes.data), last_error()

    for args, what in ((dict(pieces=[(0, 50, -1, 0), (50, 101, -1, 0)]), "piece 1 [50, 101) is outside the window of 100 loci"),
                       (dict(pieces=[(10, 5, -1, 0)]), "piece 0 [10, 5)"),
                       (dict(pieces=[(0, 50, 0, 0)]), "long_index 0 of piece 0 is outside [-1, 0)"),
                       (dict(pieces=[(0, 50, -2, 0)], n_long=1), "long_index -2"),
                       (dict(pieces=[(0, 50, -1, 0)], length=-1), "a window of -1 loci")):
        rc, err = stats(**args)
        assert rc == fcship.FCS_ERR_INVALID and "[E::fcsdp_stats]" in err and what in err, (args, err)
        assert (hist == 7).all() and not summary["loci"].any()
    assert stats([])[0] == 0                                         # no piece needs no device
    rc, err = stats([(0, 50, -1, 0)])
    assert rc in (fcship.FCS_ERR_INVALID, fcship.FCS_ERR_DEVICE) and "[E::fcsdp_stats]" not in err and (hist == 7).all()
    assert fcship.lib.fcsdp_workspace_bytes(-1) == fcship.FCS_ERR_INVALID and "[E::fcsdp_workspace_bytes]" in last_error()
    assert 0 < fcship.lib.fcsdp_workspace_bytes(1) <= fcship.lib.fcsdp_workspace_bytes(1 << 24) <= 1 << 20
    one = np.zeros(64, np.uint8).ctypes.data   # stands for device memory: never dereferenced
    assert fcship.lib.fcsdp_scan_dev(0, one, 5000, one, 16, one, None) == fcship.FCS_ERR_INVALID
    assert "[E::fcsdp_scan_dev]" in last_error() and "the workspace holds 16 bytes" in last_error()
    assert fcship.lib.fcsdp_runs_dev(0, C.addressof(b), C.addressof(prm), C.addressof(w), one, None, None) == fcship.FCS_ERR_INVALID
    assert "[E::fcsdp_runs_dev]" in last_error()
    assert fcship.lib.fcsdp_stats_dev(0, one, one, 100, one, 1, 0, one, None, one, None, None) == fcship.FCS_ERR_INVALID
    assert "[E::fcsdp_stats_dev]" in last_error()


# ------------------------------------------------------------------ the command, on the host path
@pytest.fixture(scope="module")
def mock_env():
    subprocess.run(["make", "-C", f"{ROOT}/tests/cpu_mock"], check=True, capture_output=True)
    return {"LD_LIBRARY_PATH": f"{ROOT}/tests/cpu_mock/build", "FCS_GPU_DEVICES": "0", "FCS_DEPTH_GPU": "false"}


NAMES = ["ctgA", "ctgB", "ctgC"]


def write_world(d, refs, records, header="@RG\tID:a\tSM:NA12878\n@RG\tID:b\tSM:NA12878\tPL:x\n", name="in"):
    """ref.fa and <name>.bam of the records (in the order given) under d."""
    os.makedirs(d, exist_ok=True)
    with open(d / "ref.fa", "w") as f:
        for n, s in zip(NAMES, refs):
            f.write(f">{n}\n" + "".join(s[k:k + 60] + "\n" for k in range(0, len(s), 60)))
    lines = [header]
    for k, r in enumerate(records):
        qual = "*" if r["qual"] is None else "".join(chr(q + 33) for q in r["qual"])
        lines.append(f"r{k}\t{r['flag']}\t{r['ref']}\t{r['pos']}\t{r['mapq']}\t{r['cigar']}\t{'A' * r['n_bases']}\t{qual}\n")
    (d / f"{name}.txt").write_text("".join(lines))
    H.check(L.fcsg_text_to_bam(str(d / f"{name}.txt").encode(), str(d / f"{name}.bam").encode(), ",".join(NAMES).encode(),
                               ",".join(str(len(s)) for s in refs).encode()))
    return d / "ref.fa", d / f"{name}.bam"


@pytest.fixture(scope="module")
def custom(world, tmp_path_factory):
    """A sorted BAM of the random batch over the random world (runs of N, mixed CIGARs), and its depths per contig."""
    d = tmp_path_factory.mktemp("dpc")
    records = D.random_batch(world, seed=21, n=1500, sort=True)
    ref, bam = write_world(d, world, records)
    depths = [D.depth(records, (c, 0, len(s)), len(s))[0] for c, s in enumerate(world)]
    return d, ref, bam, records, depths


def run_depth(out, ref, bam, *extra, env=None, cwd=None):
    return H.run_cli("depth", "-r", ref, "-i", bam, "-o", out, *extra, env=env, cwd=cwd)


def check_files(out, want, omitted=()):
    for suffix in SUFFIXES:
        path = str(out) + suffix
        if suffix in omitted:
            assert not os.path.exists(path), suffix
        else:
            got = open(path).read()
            assert got == want[suffix], (suffix, got[:300], want[suffix][:300])


def test_command_on_a_synth_bam_writes_the_restatement_s_bytes(mock_env, tmp_path):
    d = tmp_path / "s"
    p = H.run_cli("synth", "-o", d, "-c", "chr1:30000,chr2:12000", "-x", "4", "--seed", "13", "--no-fastq")
    assert p.returncode == 0, p.stderr[-2000:]
    p = run_depth(tmp_path / "cov", d / "ref.fasta", d / "sample.bam", "--sample-id", "x", env=mock_env, cwd=tmp_path)
    assert p.returncode == 0 and "(host)" in p.stderr and "entry point" not in p.stderr, p.stderr[-2000:]
    names, lens, recs = H.read_bam(d / "sample.bam")
    records = [D.rec(r["flag"], r["ref_id"], r["pos"], "".join(r["cigar"]),
                     None if r["qual"][:1] == b"\xff" or not r["qual"] else list(r["qual"]), mapq=r["mapq"]) for r in recs]
    refs = ["N" * 0 + s for s in read_fasta(d / "ref.fasta")[1]]
    depths = [D.depth(records, (c, 0, n), n)[0] for c, n in enumerate(lens)]
    assert len(records) > 500 and sum(int(x.sum()) for x in depths) > 100000
    want = D.files("sample", names, refs, [(c, 0, n) for c, n in enumerate(lens)], depths)
    check_files(tmp_path / "cov", want)
    assert f"{len(records)} records, 2 intervals, 2 windows, 42000 loci" in p.stderr
    # the output exists: refused without -f, overwritten with it
    assert run_depth(tmp_path / "cov", d / "ref.fasta", d / "sample.bam", env=mock_env).returncode == 1
    os.remove(tmp_path / "cov")
    p = run_depth(tmp_path / "cov", d / "ref.fasta", d / "sample.bam", env=mock_env)
    assert p.returncode == 1 and "cov.sample_summary exists (use -f)" in p.stderr
    assert run_depth(tmp_path / "cov", d / "ref.fasta", d / "sample.bam", "-f", env=mock_env).returncode == 0
    check_files(tmp_path / "cov", want)
    # missing files and arguments, help, usage
    assert run_depth(tmp_path / "x", d / "none.fasta", d / "sample.bam", env=mock_env).returncode == 3
    assert run_depth(tmp_path / "x", d / "ref.fasta", d / "none.bam", env=mock_env).returncode == 3
    assert run_depth(tmp_path / "x", d / "ref.fasta", d / "sample.bam", "-L", d / "none.bed", env=mock_env).returncode == 3
    p = H.run_cli("depth", "-r", d / "ref.fasta", "-o", tmp_path / "x", env=mock_env)
    assert p.returncode == 1 and "--input is required" in p.stderr
    p = run_depth(tmp_path / "x", d / "ref.fasta", d / "sample.bam", "-L", "", env=mock_env)
    assert p.returncode == 1 and "cannot be empty" in p.stderr
    h = H.run_cli("depth", "--help", env=mock_env)
    assert h.returncode == 0
    for opt in ("--omitBaseOutput", "--omitIntervals", "--omitSampleSummary", "--intervalList", "--geneList", "--sample-id"):
        assert opt in h.stderr
    assert "depth" in H.run_cli(env=mock_env).stdout
    assert not os.path.exists(tmp_path / "x")


def read_fasta(path):
    names, seqs = [], []
    for ln in open(path).read().split("\n"):
        if ln.startswith(">"):
            names.append(ln[1:].split()[0])
            seqs.append([])
        elif ln:
            seqs[-1].append(ln)
    return names, ["".join(s) for s in seqs]


def test_command_on_mixed_cigars_and_reference_n(custom, world, mock_env, tmp_path):
    d, ref, bam, records, depths = custom
    whole = [(c, 0, len(s)) for c, s in enumerate(world)]
    want = D.files("NA12878", NAMES, world, whole, depths)
    assert want[""].count("\n") - 1 == sum(ch not in "Nn" for s in world for ch in s) < sum(len(s) for s in world)
    p = run_depth(tmp_path / "all", ref, bam, env=mock_env, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    check_files(tmp_path / "all", want)
    # small windows and small chunks stream to the same bytes
    env = {**mock_env, "FCS_DEPTH_WINDOW_BP": "4096", "FCS_DEPTH_CHUNK_RECORDS": "500"}
    p = run_depth(tmp_path / "small", ref, bam, env=env, cwd=tmp_path)
    assert p.returncode == 0 and "3 intervals, 6 windows" in p.stderr, p.stderr[-2000:]
    check_files(tmp_path / "small", want)
    # -b, -v and -s each drop their files and nothing else
    for flag, gone in (("-b", [""]), ("-v", [".sample_interval_summary", ".sample_interval_statistics"]),
                       ("-s", [".sample_summary", ".sample_statistics"]), ("--omitBaseOutput", [""])):
        out = tmp_path / ("o" + flag.strip("-"))
        assert run_depth(out, ref, bam, flag, env=mock_env, cwd=tmp_path).returncode == 0
        check_files(out, want, omitted=gone)
    # the other parameters reach the rules
    env = {**mock_env, "FCS_DEPTH_MIN_MAPQ": "20", "FCS_DEPTH_MAX_MAPQ": "60", "FCS_DEPTH_MIN_BASEQ": "10",
           "FCS_DEPTH_MAX_BASEQ": "40", "FCS_DEPTH_INCLUDE_DELETIONS": "true", "FCS_DEPTH_INCLUDE_REF_N": "true"}
    prm = D.params(20, 60, 10, 40, True)
    other = [D.depth(records, (c, 0, len(s)), len(s), prm)[0] for c, s in enumerate(world)]
    assert run_depth(tmp_path / "prm", ref, bam, env=env, cwd=tmp_path).returncode == 0
    check_files(tmp_path / "prm", D.files("NA12878", NAMES, world, whole, other, include_ref_n=True))
    # the mock lacks the entry points: one line, and the host path's bytes
    p = run_depth(tmp_path / "gpu", ref, bam, env={**mock_env, "FCS_DEPTH_GPU": "true", "FCS_DEPTH_CHUNK_RECORDS": "400"}, cwd=tmp_path)
    assert p.returncode == 0 and "(host)" in p.stderr and p.stderr.count("has no fcsdp_count entry point") == 1
    check_files(tmp_path / "gpu", want)


def n_run(seq):
    """(start, end) of the first run of N / n."""
    a = min(i for i, ch in enumerate(seq) if ch in "Nn")
    b = a
    while seq[b] in "Nn":
        b += 1
    return a, b


def test_intervals_overlapping_abutting_one_locus_and_only_n(custom, world, mock_env, tmp_path):
    d, ref, bam, records, depths = custom
    a, b = n_run(world[1])
    bed = [("ctgC", 100, 300), ("ctgA", 4000, 4200), ("ctgA", 50, 120), ("ctgA", 100, 180), ("ctgA", 180, 250),
           ("ctgA", 4090, 4100), ("ctgA", 777, 778), ("ctgB", a, b), ("ctgB", 0, 5000)]
    (tmp_path / "l.bed").write_text("track name=x\n" + "".join(f"{c}\t{s}\t{e}\n" for c, s, e in bed))
    merged = D.merge_intervals([(NAMES.index(c), s, e) for c, s, e in bed])
    assert merged == [(0, 50, 250), (0, 777, 778), (0, 4000, 4200), (1, 0, 5000), (2, 100, 300)]
    want = D.files("NA12878", NAMES, world, merged, depths)
    assert "ctgA:778\t" in want[".sample_interval_summary"] and "ctgA:51-250\t" in want[".sample_interval_summary"]
    for env in (mock_env, {**mock_env, "FCS_DEPTH_WINDOW_BP": "4096", "FCS_DEPTH_CHUNK_RECORDS": "300"}):
        out = tmp_path / f"l{len(env)}"
        p = run_depth(out, ref, bam, "-L", tmp_path / "l.bed", env=env, cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-2000:]
        check_files(out, want)
    # an interval list, with an interval of only N: no locus, NaN, cell 0
    (tmp_path / "n.list").write_text(f"ctgB:{a + 1}-{b}\nctgA:11-20\n")
    only_n = [(0, 10, 20), (1, a, b)]
    want = D.files("NA12878", NAMES, world, only_n, depths)
    row = want[".sample_interval_summary"].split("\n")[2].split("\t")
    assert row[0] == f"ctgB:{a + 1}-{b}" and row[1:] == ["0", "NaN", "0", "NaN", "1", "1", "1", "NaN"]
    p = run_depth(tmp_path / "n", ref, bam, "-L", tmp_path / "n.list", env=mock_env, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    check_files(tmp_path / "n", want)
    (tmp_path / "bad.bed").write_text("ctgZ\t1\t5\n")
    p = run_depth(tmp_path / "z", ref, bam, "-L", tmp_path / "bad.bed", env=mock_env)
    assert p.returncode == 1 and "contig ctgZ" in p.stderr


def test_refusals_gene_list_two_samples_unsorted_and_a_missing_contig(custom, world, mock_env, tmp_path):
    d, ref, bam, records, depths = custom
    (tmp_path / "g.list").write_text("GENE1\n")
    p = run_depth(tmp_path / "g", ref, bam, "-g", tmp_path / "g.list", env=mock_env)
    assert p.returncode == 1 and "Invalid parameter" in p.stderr and "gene summaries are not built" in p.stderr
    few = records[:50]
    _, two = write_world(tmp_path / "w", world, few, header="@RG\tID:a\tSM:one\n@RG\tID:b\tSM:two\n", name="two")
    p = run_depth(tmp_path / "t", ref, two, env=mock_env)
    assert p.returncode == 1 and "Invalid parameter" in p.stderr and "2 samples (one, two)" in p.stderr
    _, none = write_world(tmp_path / "w", world, few, header="@RG\tID:a\n", name="none")
    p = run_depth(tmp_path / "t", ref, none, env=mock_env)
    assert p.returncode == 1 and "names no sample" in p.stderr
    later = next(k for k in range(21, 50) if few[k]["pos"] > few[20]["pos"])
    swapped = few[:20] + [few[later]] + few[20:later]
    _, unsorted = write_world(tmp_path / "w", world, swapped, name="unsorted")
    p = run_depth(tmp_path / "t", ref, unsorted, env=mock_env)
    where = f"record r21 at {NAMES[few[20]['ref']]}:{few[20]['pos'] + 1}"
    assert p.returncode == 1 and "not coordinate-sorted" in p.stderr and where in p.stderr, p.stderr[-1000:]
    short = tmp_path / "short.fa"
    short.write_text("".join(f">{n}\n{s}\n" for n, s in zip(NAMES[:2], world)))
    p = run_depth(tmp_path / "t", short, bam, env=mock_env)
    assert p.returncode == 1 and "contig ctgC of the BAM header is not in" in p.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("t.")]
    # a directory of part BAMs in name order is one sorted stream
    parts = tmp_path / "parts"
    k = len(records) // 2
    write_world(parts, world, records[:k], name="part-000000")
    write_world(parts, world, records[k:], name="part-000001")
    for f in ("ref.fa", "part-000000.txt", "part-000001.txt"):
        os.remove(parts / f)
    p = run_depth(tmp_path / "dir", ref, parts, env=mock_env, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    check_files(tmp_path / "dir", D.files("NA12878", NAMES, world, [(c, 0, len(s)) for c, s in enumerate(world)], depths))
