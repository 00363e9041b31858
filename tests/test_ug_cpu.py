"""Pileup SNP genotyping (DESIGN §2 [EXT], §4.12): what needs no GPU.

- The table: fcsug_table and the host's ug_table equal the Python restatement
  (tests/ug_cases.py) and the exactly rounded values (mpmath), none of which
  lies near a half-integer.
- The hand cases, each with its expected sites written out, and the random
  batches against the restatement and the host path (host/ug.cpp through
  fcsg_ug_*), on 1 and on 16 threads, at windows of 4,096 loci and of the whole
  contig.
- csrc/ug_pile.h, the text the kernels run, compiled for the host with ASan and
  UBSan as a stand-alone program (tools/micro/ug_test.cpp), gives the sites of
  host/ug.cpp.
- The ug command with the CPU mock of libfcship (the host path) writes the
  restatement's VCF.
- fcsug_* is declared in include/fcsug.h and exported, beside an unchanged
  fcship.h surface; bad arguments are refused before any device is looked for.
"""
import ctypes as C
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import fcship
import host_lib as H
import ug_cases as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = U.hand_cases()
REFS = U.hand_refs()
TAB = U.table()
L = H.lib
L.fcsg_ug_table.argtypes = [C.c_double, C.c_void_p]
L.fcsg_ug_sites.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
L.fcsg_ug_vcf_text.argtypes = [C.c_void_p, C.c_int64, C.c_char_p, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_char_p, C.c_int]
L.fcsg_ug_vcf_header.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_char_p, C.c_int]
L.fcsg_text_to_bam.argtypes = [C.c_char_p] * 4
NAMES = ["ctgA", "ctgB", "ctgC"]


def host_sites(records, window, refseq, min_baseq=17, threads=1, first_offset=0, max_sites=None, table=None):
    arrays = fcship.ug_arrays(*U.flatten(records, first_offset))
    b = fcship.ug_batch(arrays)
    ref, start, length = window
    w = fcship.UgWindow(ref, 0, start, length, len(refseq))
    p = fcship.UgParams(min_baseq)
    seq = np.frombuffer(refseq[start:start + length].encode(), np.uint8)
    tab = np.ascontiguousarray(TAB if table is None else table, np.int64)
    max_sites = length if max_sites is None else max_sites
    sites = np.zeros(max(max_sites, 1), fcship.UG_SITE)
    n = C.c_int64(-1)
    H.check(L.fcsg_ug_sites(C.addressof(b), C.addressof(p), C.addressof(w), seq.ctypes.data, tab.ctypes.data, threads,
                            sites.ctypes.data, max_sites, C.addressof(n)))
    return sites[:n.value]


def host_vcf_text(sites, chrom, window_start=0, het=1e-3, conf=10.0, maxdel=0.05):
    sites = np.ascontiguousarray(sites)
    buf = C.create_string_buffer(1 << 20)
    n = L.fcsg_ug_vcf_text(sites.ctypes.data, len(sites), chrom.encode(), window_start, het, conf, maxdel, buf, len(buf))
    assert n >= 0
    return buf.value.decode()


# ------------------------------------------------------------------ the table
def test_table_equals_the_restatement_and_the_exactly_rounded_values():
    mpmath = pytest.importorskip("mpmath")
    got = fcship.ug_table(1e-4)
    assert got.shape == (94, 3) and got.dtype == np.int64 and got.tolist() == TAB
    host = np.zeros((94, 3), np.int64)
    H.check(L.fcsg_ug_table(1e-4, host.ctypes.data))
    assert host.tolist() == TAB
    mpmath.mp.dps = 60
    eps, third = mpmath.mpf(1e-4), mpmath.mpf(1) / 3   # the double nearest 1e-4, as the code holds it
    nearest_half = 1.0
    for q in range(94):
        e = mpmath.mpf(10) ** (-mpmath.mpf(q) / 10)
        same = (1 - eps) * (1 - e) + eps * e * third
        diff = (1 - eps) * e * third + eps * third * (1 - e) + 2 * (eps * third) * (e * third)
        for c, p in enumerate((same, (same + diff) / 2, diff)):
            x = mpmath.log10(p) * 2 ** 32
            assert int(mpmath.nint(x)) == TAB[q][c], (q, c)
            nearest_half = min(nearest_half, float(abs(abs(x - mpmath.floor(x)) - mpmath.mpf(1) / 2)))
    print(f"closest exact value to a half-integer: {nearest_half:.4f} units")
    assert nearest_half > 1e-3
    assert TAB[30][0] > TAB[30][1] > TAB[30][2] and TAB[93][0] > TAB[0][0] and all(v < 0 for row in TAB for v in row)
    assert fcship.ug_table(1e-3).tolist() == U.table(1e-3) != TAB
    for bad in (0.0, 1.0, -1e-4, float("nan")):
        assert fcship.lib.fcsug_table(bad, got.ctypes.data) == fcship.FCS_ERR_INVALID
        assert "[E::fcsug_table]" in fcship.lib.fcs_last_error().decode()
    assert got.tolist() == TAB


# ------------------------------------------------------------------ the host oracle
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_case(case):
    refseq = REFS[case["window"][0]]
    want, beyond = U.sites(case["records"], case["window"], refseq, TAB)
    assert U.brief(want) == U.want_sites(case) and beyond == case["beyond"]
    if case["beyond"]:   # the host path refuses the record
        with pytest.raises(RuntimeError, match="record 0 has an aligned base beyond its contig"):
            host_sites(case["records"], case["window"], refseq)
    else:
        for threads in (1, 16):
            assert U.full(host_sites(case["records"], case["window"], refseq, threads=threads)) == U.full(want)


def test_the_list_of_hand_cases_is_the_issue_s_and_one_site_by_hand():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    for must in ("qe_16_and_17", "quality_capped_by_mapq", "mapq_255", "mapq_0_deletions", "equal_qsum_smaller_letter_wins",
                 "reference_n", "lower_case_reference", "read_n_and_lower_case_read", "only_s_and_i", "d_at_a_tile_edge",
                 "ends_one_past_contig_end", "two_tiles", "three_tiles_through_a_skip", "flags"):
        assert must in names
    flags = next(c for c in CASES if c["name"] == "flags")["records"]
    assert [r["flag"] for r in flags[:5]] == [0x4, 0x100, 0x200, 0x400, 0x800]
    # one base C of quality 30 and MAPQ 60 on a reference A: gl = T[30][2], T[30][1], T[30][0]
    s, _ = U.sites(next(c for c in CASES if c["name"] == "one_mismatch")["records"], (0, 0, 1200), REFS[0], TAB)
    assert U.full(s) == [dict(offset=12, ref=0, alt=1, n=[0, 1, 0, 0], qsum=[0, 30, 0, 0], n_del=0, mq2=3600,
                              gl=[TAB[30][2], TAB[30][1], TAB[30][0]])]
    # two matching A and one C: ref/ref = 2 T[30][0] + T[30][2], ref/alt = 3 T[30][1], alt/alt = T[30][0] + 2 T[30][2]
    three = [U.rec(0, 0, 12, "1M", "A"), U.rec(0, 0, 12, "1M", "A"), U.rec(0, 0, 12, "1M", "C")]
    s, _ = U.sites(three, (0, 0, 1200), REFS[0], TAB)
    assert s[0]["gl"] == [2 * TAB[30][0] + TAB[30][2], 3 * TAB[30][1], TAB[30][0] + 2 * TAB[30][2]]
    # the genotype step by hand: 20 alt bases of quality 30 are a 1/1 call with PL 0 for alt/alt
    hom = [U.rec(0, 0, 12, "1M", "C")] * 20
    s, _ = U.sites(hom, (0, 0, 1200), REFS[0], TAB)
    g = U.genotype(s[0])
    assert g["gt"] == 2 and g["pl"][2] == 0 and g["pl"][0] > g["pl"][1] > 0 and g["ad"] == [0, 20] and g["dp"] == 20
    assert g["mq"] == "60.00" and g["af"] == "1.00" and g["gq"] == min(99, g["pl"][1])
    assert g["pl"][1] == (10 * 20 * (TAB[30][0] - TAB[30][1]) + (1 << 31)) >> 32
    line = U.vcf_line(s[0], g, "ctgA", 0).split("\t")
    assert line[:5] == ["ctgA", "13", ".", "A", "C"] and line[8] == "GT:AD:DP:GQ:PL" and line[9].startswith("1/1:0,20:20:")
    assert line[7] == "AC=2;AF=1.00;AN=2;DP=20;MQ=60.00"
    # too many deletions drop the site: 2 of 21 reads is above 0.05
    dels = [U.rec(0, 0, 11, "1M2D1M", "TG")] * 2
    s, _ = U.sites(dels + hom, (0, 0, 1200), REFS[0], TAB)
    assert s[0]["n_del"] == 2 and U.genotype(s[0]) is None and U.genotype(s[0], max_deletion_fraction=0.1) is not None


@pytest.fixture(scope="module")
def world():
    return U.random_world()


@pytest.fixture(scope="module")
def built(world):
    """[(records, min_baseq, first base offset, the restatement's sites per contig)] of the built batches."""
    out = []
    for records, min_baseq, first in ((U.random_batch(world), 17, 0), (U.random_batch(world, seed=12, n=600), 0, 1),
                                      (U.sweep_batch(world), 5, 3)):
        out.append((records, min_baseq, first, [U.sites(records, (c, 0, len(s)), s, TAB, min_baseq)[0] for c, s in enumerate(world)]))
    return out


def test_host_path_equals_the_restatement_on_built_batches(world, built):
    for records, min_baseq, first, want in built:
        assert sum(len(w) for w in want) > 100
        for c, seq in enumerate(world):
            n = len(seq)
            for threads in (1, 16):
                got = host_sites(records, (c, 0, n), seq, min_baseq, threads, first)
                assert U.full(got) == U.full(want[c])
            for start in range(0, n, 4096):   # records straddle the windows and are clipped to each
                length = min(4096, n - start)
                got = U.full(host_sites(records, (c, start, length), seq, min_baseq, 16, first))
                assert got == U.full([dict(s, offset=s["offset"] - start) for s in want[c] if start <= s["offset"] < start + length])
                assert got == U.full(U.sites(records, (c, start, length), seq, TAB, min_baseq)[0])
    records, _, _, want = built[0]
    text = "".join(U.vcf_text(want[c], NAMES[c], margin=0.05) for c in range(3))
    assert text.count("\t0/1:") > 3 and text.count("\t1/1:") > 3
    # the shared genotype step writes the restatement's lines; a window start moves POS
    for c in range(3):
        got = host_vcf_text(host_sites(records, (c, 0, len(world[c])), world[c]), NAMES[c])
        assert U.same_vcf(got, U.vcf_text(want[c], NAMES[c])) and got.count("\n") == U.vcf_text(want[c], NAMES[c]).count("\n")
    buf, lens = C.create_string_buffer(1 << 16), np.array([len(s) for s in world], np.int64)
    assert L.fcsg_ug_vcf_header(b"NA12878", "\n".join(NAMES).encode(), lens.ctypes.data, buf, len(buf)) > 0
    assert buf.value.decode() == U.vcf_header("NA12878", NAMES, lens.tolist())
    moved = host_vcf_text(host_sites(records, (0, 4096, 4096), world[0]), "x", 4096, conf=0.0)
    assert U.same_vcf(moved, U.vcf_text([dict(s, offset=s["offset"] - 4096) for s in want[0] if 4096 <= s["offset"] < 8192], "x",
                                        4096, stand_call_conf=0.0))
    assert moved.count("\n") > text.count("\n") / 3


def test_host_path_refuses_bad_batches(world):
    r = U.rec(0, 1, 5, "10M", "A" * 10)
    r["n_bases"], r["qual"], r["seq"] = 9, r["qual"][:9], r["seq"][:9]
    with pytest.raises(RuntimeError, match="CIGAR of record 1 does not cover"):
        host_sites([U.rec(0, 1, 0, "4M", "ACGT"), r], (1, 0, 40), REFS[1])
    with pytest.raises(RuntimeError, match="beyond its contig"):
        host_sites([U.rec(0, 1, -1, "4M", "ACGT")], (1, 0, 40), REFS[1])
    with pytest.raises(RuntimeError, match="record 2 at position 3 follows record 0 at 4: positions decrease"):
        host_sites([U.rec(0, 1, 4, "4M", "ACGT"), U.rec(0, 0, 1, "4M", "ACGT"), U.rec(0x4, 1, 3, "4M", "ACGT")], (1, 0, 40), REFS[1])
    with pytest.raises(RuntimeError, match="max_sites is 0"):
        host_sites([U.rec(0, 1, 4, "4M", "CCCC")], (1, 0, 40), REFS[1], max_sites=0)
    with pytest.raises(U.Refused):
        U.sites([r], (1, 0, 40), REFS[1], TAB)
    with pytest.raises(U.Refused):
        U.sites([U.rec(0, 1, 4, "4M", "ACGT"), U.rec(0x4, 1, 3, "4M", "ACGT")], (1, 0, 40), REFS[1], TAB)


# ------------------------------------------------------------------ ug_pile.h on the host, under sanitizers
@pytest.fixture(scope="module")
def pile_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("ugp") / "ug_test"
    pkg = os.path.join(ROOT, "falcon-genome_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(pkg, "csrc"), "-I" + os.path.join(pkg, "host"),
                    os.path.join(ROOT, "tools", "micro", "ug_test.cpp"), os.path.join(pkg, "host", "ug.cpp"),
                    "-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("seed,records", [(1, 3000), (2, 300), (3, 0), (4, 1)])
def test_shared_pile_host_build_equals_the_host_rules(pile_exe, seed, records):
    r = subprocess.run([str(pile_exe), str(seed), str(records)], capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "MISMATCH" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    if records >= 300:
        fig = dict(zip(r.stdout.split()[0::2], r.stdout.split()[1::2]))
        assert int(fig["counted_bases"]) > int(fig["sites"]) > int(fig["calls"]) > 0


# ------------------------------------------------------------------ the ABI
def last_error():
    return fcship.lib.fcs_last_error().decode()


def test_symbols_declared_and_exported_beside_an_unchanged_fcship_h():
    names = ["fcsug_sites", "fcsug_sites_dev", "fcsug_table", "fcsug_workspace_bytes"]
    assert fcship.ug_header_symbols() == names
    nm = subprocess.run(["nm", "-D", "--defined-only", fcship.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("fcsug_")}
    assert exported == set(names)
    assert fcship.lib.fcs_abi_symbol_count() == len(fcship.header_symbols()) == 61
    assert not [s for s in fcship.header_symbols() if "ug" in s.split("_")]
    assert C.sizeof(fcship.UgBatch) == 13 * 8 and C.sizeof(fcship.UgWindow) == 32 and C.sizeof(fcship.UgParams) == 4
    assert fcship.UG_SITE.itemsize == 80 and fcship.UG_SITE.fields["mq2"][1] == 48 and fcship.UG_SITE.fields["gl"][1] == 56
    header = open(fcship.UG_HEADER_PATH).read()
    assert f"#define FCSUG_TILE {fcship.FCSUG_TILE}" in header and fcship.FCSUG_TILE >= 256
    assert fcship.FCSUG_TILE & (fcship.FCSUG_TILE - 1) == 0 and U.TILE == fcship.FCSUG_TILE
    assert f"#define FCSUG_WINDOW_MAX {fcship.FCSUG_WINDOW_MAX}" in header and fcship.FCSUG_WINDOW_MAX == 16777216
    for name, bit in (("FIELD", 1), ("REF", 2), ("ORDER", 4), ("SITES", 8)):
        assert f"#define FCSUG_STATUS_{name} {bit}" in header and getattr(fcship, "FCSUG_STATUS_" + name) == bit
    mock = subprocess.run(["nm", "-D", "--defined-only", f"{ROOT}/tests/cpu_mock/build/libfcship.so"],
                          capture_output=True, text=True).stdout
    assert "fcs_phmm" in mock and "fcsug_" not in mock


def test_arguments_are_checked_before_the_device():
    seq = REFS[0][:300]
    records = [U.rec(0, 0, 10 * k, "10M", U.read_of(seq, 10 * k, "10M", {3: U.other(seq[10 * k + 3])})) for k in range(4)]
    arrays = fcship.ug_arrays(*U.flatten(records))
    sites = np.zeros(300, fcship.UG_SITE)
    sites["offset"] = 7
    n = C.c_int64(-7)
    prm = fcship.UgParams(17)
    ref = np.frombuffer(seq.encode(), np.uint8)
    tab = np.ascontiguousarray(TAB, np.int64)

    def swapped(k, values):
        a = list(arrays)
        a[k] = np.ascontiguousarray(values, arrays[k].dtype)
        return tuple(a)

    def call(a=arrays, window=(0, 0, 300, 300), max_sites=300, device=99, **kw):
        b = fcship.ug_batch(a, **kw)
        w = fcship.UgWindow(window[0], 0, *window[1:])
        return fcship.lib.fcsug_sites(device, C.addressof(b), C.addressof(prm), C.addressof(w), ref.ctypes.data, tab.ctypes.data,
                                      sites.ctypes.data, max_sites, C.addressof(n)), last_error()

    for kw, what in ((dict(n=-1), "negative record count"),
                     (dict(a=swapped(8, [0, 10, 9, 30, 40])), "base offsets out of order at record 1"),
                     (dict(a=swapped(5, [0, 1, 2, 1, 4])), "CIGAR offsets out of order at record 2"),
                     (dict(n_bases=39), "base offsets end at 40, beyond the 39 given"),
                     (dict(window=(0, 0, 301, 300)), "lies outside its contig of 300 bases"),
                     (dict(window=(-1, 0, 300, 300)), "window ref_id -1"),
                     (dict(window=(0, 0, (1 << 24) + 1, 1 << 31)), "loci (at most 16777216)"),
                     (dict(max_sites=-1), "max_sites -1"),
                     (dict(a=swapped(2, [0, 10, 295, 30])), "record 2 has an aligned base beyond its contig"),
                     (dict(a=swapped(2, [0, 10, 9, 30])), "record 2 at position 9 follows record 1 at 10: positions decrease"),
                     (dict(a=swapped(4, [10 << 4, 10 << 4, 9 << 4, 10 << 4])), "the CIGAR of record 2 does not cover its bases")):
        rc, err = call(**kw)
        assert rc == fcship.FCS_ERR_INVALID and "[E::fcsug_sites]" in err and what in err, (kw, err)
        assert (sites["offset"] == 7).all() and n.value == -7, kw
    b = fcship.ug_batch(arrays)
    w = fcship.UgWindow(0, 0, 0, 300, 300)
    args = (ref.ctypes.data, tab.ctypes.data, sites.ctypes.data, 300, C.addressof(n))
    assert fcship.lib.fcsug_sites(0, None, C.addressof(prm), C.addressof(w), *args) == fcship.FCS_ERR_INVALID
    assert "null batch" in last_error()
    assert fcship.lib.fcsug_sites(0, C.addressof(b), None, C.addressof(w), *args) == fcship.FCS_ERR_INVALID
    assert "null parameters" in last_error()
    assert fcship.lib.fcsug_sites(0, C.addressof(b), C.addressof(prm), C.addressof(w), ref.ctypes.data, None, sites.ctypes.data,
                                  300, C.addressof(n)) == fcship.FCS_ERR_INVALID
    assert "null reference, table, sites or count" in last_error()
    # a good batch on a device that is not there: the device error comes after every check
    rc, err = call()
    assert rc in (fcship.FCS_ERR_INVALID, fcship.FCS_ERR_DEVICE) and "[E::fcsug_sites]" not in err
    assert (sites["offset"] == 7).all() and n.value == -7
    # an empty batch and an empty window need no device
    e = fcship.ug_batch(fcship.ug_arrays([], [], [], [], [], [0], [], [], [0], []))
    assert fcship.lib.fcsug_sites(99, C.addressof(e), C.addressof(prm), C.addressof(w), *args) == 0 and n.value == 0
    n.value = -7
    w0 = fcship.UgWindow(0, 0, 10, 0, 300)
    assert fcship.lib.fcsug_sites(99, C.addressof(b), C.addressof(prm), C.addressof(w0), None, tab.ctypes.data, None, 0,
                                  C.addressof(n)) == 0 and n.value == 0
    assert fcship.lib.fcsug_workspace_bytes(-1, 10) == fcship.FCS_ERR_INVALID and "[E::fcsug_workspace_bytes]" in last_error()
    assert fcship.lib.fcsug_workspace_bytes(10, (1 << 24) + 1) == fcship.FCS_ERR_INVALID
    assert 0 < fcship.lib.fcsug_workspace_bytes(0, 1) <= fcship.lib.fcsug_workspace_bytes(1 << 20, 1 << 24) <= 1 << 25
    one = np.zeros(64, np.uint8).ctypes.data   # stands for device memory: never dereferenced
    assert fcship.lib.fcsug_sites_dev(0, C.addressof(b), C.addressof(prm), C.addressof(w), one, one, one, 300, one, one, 16, one,
                                      None) == fcship.FCS_ERR_INVALID
    assert "[E::fcsug_sites_dev]" in last_error() and "the workspace holds 16 bytes" in last_error()
    assert fcship.lib.fcsug_sites_dev(0, C.addressof(b), C.addressof(prm), C.addressof(w), one, one, one, 300, one, one, 1 << 20,
                                      None, None) == fcship.FCS_ERR_INVALID
    assert "null reference, table, sites, count, workspace or status" in last_error()
    assert fcship.lib.fcsug_sites_dev(0, C.addressof(b), C.addressof(prm), C.addressof(w), one, one, one, -1, one, one, 1 << 20,
                                      one, None) == fcship.FCS_ERR_INVALID
    assert "max_sites -1" in last_error()


# ------------------------------------------------------------------ the command, on the host path
@pytest.fixture(scope="module")
def mock_env():
    subprocess.run(["make", "-C", f"{ROOT}/tests/cpu_mock"], check=True, capture_output=True)
    return {"LD_LIBRARY_PATH": f"{ROOT}/tests/cpu_mock/build", "FCS_GPU_DEVICES": "0", "FCS_UG_GPU": "false"}


def write_world(d, refs, records, header="@RG\tID:a\tSM:NA12878\n@RG\tID:b\tSM:NA12878\tPL:x\n", name="in"):
    """ref.fa and <name>.bam of the records (in the order given) under d."""
    os.makedirs(d, exist_ok=True)
    with open(d / "ref.fa", "w") as f:
        for n, s in zip(NAMES, refs):
            f.write(f">{n}\n" + "".join(s[k:k + 60] + "\n" for k in range(0, len(s), 60)))
    lines = [header]
    for k, r in enumerate(records):
        qual = "*" if r["qual"] is None else "".join(chr(q + 33) for q in r["qual"])
        lines.append(f"r{k}\t{r['flag']}\t{r['ref']}\t{r['pos']}\t{r['mapq']}\t{r['cigar']}\t{r['seq'].upper()}\t{qual}\n")
    (d / f"{name}.txt").write_text("".join(lines))
    H.check(L.fcsg_text_to_bam(str(d / f"{name}.txt").encode(), str(d / f"{name}.bam").encode(), ",".join(NAMES).encode(),
                               ",".join(str(len(s)) for s in refs).encode()))
    return d / "ref.fa", d / f"{name}.bam"


@pytest.fixture(scope="module")
def custom(world, tmp_path_factory):
    """A sorted BAM of the random batch over the random world (runs of N, lower case, mixed CIGARs), and its VCF."""
    d = tmp_path_factory.mktemp("ugc")
    records = U.random_batch(world, seed=21, n=3000)
    ref, bam = write_world(d, world, records)
    return d, ref, bam, records, U.command_vcf(world, NAMES, "NA12878", records)


def n_calls(text):
    return sum(1 for ln in text.splitlines() if not ln.startswith("#"))


def run_ug(out, ref, bam, *extra, env=None, cwd=None):
    return H.run_cli("ug", "-r", ref, "-i", bam, "-o", out, *extra, env=env, cwd=cwd)


def check_vcf(out, want):
    """out, out.gz and out.gz.tbi: the restatement's header and records, the bgzipped copy and an index of its contigs."""
    got = open(out).read()
    head = "".join(ln + "\n" for ln in got.splitlines() if ln.startswith("#"))
    whead = "".join(ln + "\n" for ln in want.splitlines() if ln.startswith("#"))
    assert head == whead, (head[-400:], whead[-400:])
    assert U.same_vcf(got[len(head):], want[len(whead):]), (got[len(head):][:600], want[len(whead):][:600])
    assert gzip.decompress(open(str(out) + ".gz", "rb").read()).decode() == got
    names, refs = H.parse_index(gzip.decompress(open(str(out) + ".gz.tbi", "rb").read()), b"TBI\x01")
    called = []
    for ln in got[len(head):].splitlines():
        if ln.split("\t")[0] not in called:
            called.append(ln.split("\t")[0])
    assert names == called


def read_fasta(path):
    names, seqs = [], []
    for ln in open(path).read().split("\n"):
        if ln.startswith(">"):
            names.append(ln[1:].split()[0])
            seqs.append([])
        elif ln:
            seqs[-1].append(ln)
    return names, ["".join(s) for s in seqs]


def test_command_on_a_synth_bam_writes_the_restatement_s_vcf(mock_env, tmp_path):
    d = tmp_path / "s"
    p = H.run_cli("synth", "-o", d, "-c", "chr1:30000,chr2:12000", "-x", "12", "--seed", "13", "--no-fastq")
    assert p.returncode == 0, p.stderr[-2000:]
    p = run_ug(tmp_path / "out.vcf", d / "ref.fasta", d / "sample.bam", "--sample-id", "x", "-O", "--foo 1", env=mock_env, cwd=tmp_path)
    assert p.returncode == 0 and "(host)" in p.stderr and "entry point" not in p.stderr, p.stderr[-2000:]
    assert p.stderr.count("--extra-options --foo 1: ignored") == 1
    names, lens, recs = H.read_bam(d / "sample.bam")
    records = [U.rec(r["flag"], r["ref_id"], r["pos"], "".join(r["cigar"]), r["seq"],
                     None if r["qual"][:1] == b"\xff" or not r["qual"] else list(r["qual"]), mapq=r["mapq"]) for r in recs]
    refs = read_fasta(d / "ref.fasta")[1]
    want = U.command_vcf(refs, names, "sample", records)
    calls = n_calls(want)
    assert len(records) > 1500 and calls >= 1
    check_vcf(tmp_path / "out.vcf", want)
    assert f"{len(records)} records, 2 intervals, 2 windows" in p.stderr and f" {calls} calls" in p.stderr
    # the alias; the output exists: refused without -f, overwritten with it
    assert H.run_cli("unifiedgeno", "-r", d / "ref.fasta", "-i", d / "sample.bam", "-o", tmp_path / "alias.vcf",
                     env=mock_env).returncode == 0
    assert open(tmp_path / "alias.vcf").read() == open(tmp_path / "out.vcf").read()
    assert run_ug(tmp_path / "out.vcf", d / "ref.fasta", d / "sample.bam", env=mock_env).returncode == 1
    os.remove(tmp_path / "out.vcf")
    p = run_ug(tmp_path / "out.vcf", d / "ref.fasta", d / "sample.bam", env=mock_env)
    assert p.returncode == 1 and "out.vcf.gz exists (use -f)" in p.stderr
    assert run_ug(tmp_path / "out.vcf", d / "ref.fasta", d / "sample.bam", "-f", env=mock_env).returncode == 0
    check_vcf(tmp_path / "out.vcf", want)
    # missing files and arguments, help, usage
    assert run_ug(tmp_path / "x", d / "none.fasta", d / "sample.bam", env=mock_env).returncode == 3
    assert run_ug(tmp_path / "x", d / "ref.fasta", d / "none.bam", env=mock_env).returncode == 3
    assert run_ug(tmp_path / "x", d / "ref.fasta", d / "sample.bam", "-L", d / "none.bed", env=mock_env).returncode == 3
    p = H.run_cli("ug", "-r", d / "ref.fasta", "-o", tmp_path / "x", env=mock_env)
    assert p.returncode == 1 and "--input is required" in p.stderr
    h = H.run_cli("ug", "--help", env=mock_env)
    assert h.returncode == 0
    for opt in ("--intervalList", "--sample-id", "--skip-concat", "--extra-options"):
        assert opt in h.stderr
    assert "  ug  " in H.run_cli(env=mock_env).stdout
    conf = H.run_cli("conf", env=mock_env)
    conf = conf.stdout + conf.stderr
    for key, value in (("ug.gpu", "false"), ("ug.chunk_records", "1000000"), ("ug.window_bp", "1048576"), ("ug.min_baseq", "17"),
                       ("ug.stand_call_conf", "10"), ("ug.heterozygosity", "0.001"), ("ug.pcr_error", "0.0001"),
                       ("ug.max_deletion_fraction", "0.05")):
        assert f"{key} = {value} " in conf, key
    assert not os.path.exists(tmp_path / "x")


def test_command_on_mixed_cigars_lower_case_and_reference_n(custom, world, mock_env, tmp_path):
    d, ref, bam, records, want = custom
    assert want.count("\t0/1:") > 5 and want.count("\t1/1:") > 5
    p = run_ug(tmp_path / "all.vcf", ref, bam, env=mock_env, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    check_vcf(tmp_path / "all.vcf", want)
    # small windows and small chunks stream to the same bytes
    env = {**mock_env, "FCS_UG_WINDOW_BP": "4096", "FCS_UG_CHUNK_RECORDS": "500"}
    p = run_ug(tmp_path / "small.vcf", ref, bam, env=env, cwd=tmp_path)
    assert p.returncode == 0 and "3 intervals, 6 windows" in p.stderr, p.stderr[-2000:]
    assert open(tmp_path / "small.vcf").read() == open(tmp_path / "all.vcf").read()
    env = {**mock_env, "FCS_UG_WINDOW_BP": "1000", "FCS_UG_CHUNK_RECORDS": "7"}
    assert run_ug(tmp_path / "tiny.vcf", ref, bam, env=env, cwd=tmp_path).returncode == 0
    assert open(tmp_path / "tiny.vcf").read() == open(tmp_path / "all.vcf").read()
    # the other parameters reach the rules
    env = {**mock_env, "FCS_UG_MIN_BASEQ": "25", "FCS_UG_STAND_CALL_CONF": "30", "FCS_UG_HETEROZYGOSITY": "0.01",
           "FCS_UG_PCR_ERROR": "0.001", "FCS_UG_MAX_DELETION_FRACTION": "0.5"}
    other = U.command_vcf(world, NAMES, "NA12878", records, min_baseq=25, stand_call_conf=30.0, heterozygosity=0.01,
                          pcr_error=1e-3, max_deletion_fraction=0.5)
    assert other != want
    assert run_ug(tmp_path / "prm.vcf", ref, bam, env=env, cwd=tmp_path).returncode == 0
    check_vcf(tmp_path / "prm.vcf", other)
    # the mock lacks the entry points: one line, and the host path's bytes
    p = run_ug(tmp_path / "gpu.vcf", ref, bam, env={**mock_env, "FCS_UG_GPU": "true", "FCS_UG_WINDOW_BP": "2000"}, cwd=tmp_path)
    assert p.returncode == 0 and "(host)" in p.stderr and p.stderr.count("has no fcsug_sites entry point") == 1
    assert open(tmp_path / "gpu.vcf").read() == open(tmp_path / "all.vcf").read()


def test_intervals_overlapping_abutting_and_one_locus(custom, world, mock_env, tmp_path):
    d, ref, bam, records, want = custom
    calls = [ln.split("\t") for ln in want.splitlines() if not ln.startswith("#")]
    first_a = next(int(c[1]) for c in calls if c[0] == "ctgA")          # 1-based POS of a call: a one-locus interval
    bed = [("ctgC", 100, 3000), ("ctgA", 4000, 4200), ("ctgA", 50, 120), ("ctgA", 100, 180), ("ctgA", 180, 2500),
           ("ctgA", first_a - 1, first_a), ("ctgB", 0, 5000), ("ctgA", 8000, 8001)]
    (tmp_path / "l.bed").write_text("track name=x\n" + "".join(f"{c}\t{s}\t{e}\n" for c, s, e in bed))
    merged = U.D.merge_intervals([(NAMES.index(c), s, e) for c, s, e in bed])
    assert (0, 50, 2500) in merged
    inside = U.command_vcf(world, NAMES, "NA12878", records, intervals=merged)
    n_in = n_calls(inside)
    assert 0 < n_in < len(calls) and f"ctgA\t{first_a}\t" in inside
    for env in (mock_env, {**mock_env, "FCS_UG_WINDOW_BP": "4096", "FCS_UG_CHUNK_RECORDS": "300"}):
        out = tmp_path / f"l{len(env)}.vcf"
        p = run_ug(out, ref, bam, "-L", tmp_path / "l.bed", env=env, cwd=tmp_path)
        assert p.returncode == 0 and f" {n_in} calls" in p.stderr, p.stderr[-2000:]
        check_vcf(out, inside)
    (tmp_path / "one.list").write_text(f"ctgA:{first_a}-{first_a}\n")
    one = U.command_vcf(world, NAMES, "NA12878", records, intervals=[(0, first_a - 1, first_a)])
    assert n_calls(one) == 1
    assert run_ug(tmp_path / "one.vcf", ref, bam, "-L", tmp_path / "one.list", env=mock_env, cwd=tmp_path).returncode == 0
    check_vcf(tmp_path / "one.vcf", one)
    (tmp_path / "bad.bed").write_text("ctgZ\t1\t5\n")
    p = run_ug(tmp_path / "z.vcf", ref, bam, "-L", tmp_path / "bad.bed", env=mock_env)
    assert p.returncode == 1 and "contig ctgZ" in p.stderr


def test_refusals_skip_concat_two_samples_unsorted_and_a_missing_contig(custom, world, mock_env, tmp_path):
    d, ref, bam, records, want = custom
    p = run_ug(tmp_path / "g.vcf", ref, bam, "-s", env=mock_env)
    assert p.returncode == 1 and "Invalid parameter" in p.stderr and "one run is one stream" in p.stderr
    few = records[:50]
    _, two = write_world(tmp_path / "w", world, few, header="@RG\tID:a\tSM:one\n@RG\tID:b\tSM:two\n", name="two")
    p = run_ug(tmp_path / "t.vcf", ref, two, env=mock_env)
    assert p.returncode == 1 and "Invalid parameter" in p.stderr and "2 samples (one, two); ug takes one" in p.stderr
    _, none = write_world(tmp_path / "w", world, few, header="@RG\tID:a\n", name="none")
    p = run_ug(tmp_path / "t.vcf", ref, none, env=mock_env)
    assert p.returncode == 1 and "names no sample" in p.stderr
    later = next(k for k in range(21, 50) if few[k]["pos"] > few[20]["pos"])
    swapped = few[:20] + [few[later]] + few[20:later]
    _, unsorted = write_world(tmp_path / "w", world, swapped, name="unsorted")
    p = run_ug(tmp_path / "t.vcf", ref, unsorted, env=mock_env)
    where = f"record r21 at {NAMES[few[20]['ref']]}:{few[20]['pos'] + 1}"
    assert p.returncode == 1 and "not coordinate-sorted" in p.stderr and where in p.stderr, p.stderr[-1000:]
    short = tmp_path / "short.fa"
    short.write_text("".join(f">{n}\n{s}\n" for n, s in zip(NAMES[:2], world)))
    p = run_ug(tmp_path / "t.vcf", short, bam, env=mock_env)
    assert p.returncode == 1 and "contig ctgC of the BAM header is not in" in p.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("t.")]
    # a directory of part BAMs in name order is one sorted stream
    parts = tmp_path / "parts"
    k = len(records) // 2
    write_world(parts, world, records[:k], name="part-000000")
    write_world(parts, world, records[k:], name="part-000001")
    for f in ("ref.fa", "part-000000.txt", "part-000001.txt"):
        os.remove(parts / f)
    p = run_ug(tmp_path / "dir.vcf", ref, parts, env=mock_env, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    check_vcf(tmp_path / "dir.vcf", want)
