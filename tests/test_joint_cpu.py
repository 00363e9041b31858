"""Joint genotyping (DESIGN §2 [EXT] "GenotypeGVCFs, round 20", §4.13): what needs no GPU.

- The tables: fcsjg_tables and the host's joint_tables equal the Python
  restatement (tests/jg_cases.py) and the exactly rounded values (mpmath); the
  log-sum table's error e is measured, and QUAL stays within n (4 e + 2) + 1
  units of a 40-digit evaluation of the recurrence.
- The hand cases, each with its expected lines written out, through the
  restatement and the command; random cohorts against the host path
  (host/joint.cpp through fcsg_jg_*) on 1 and on 16 threads.
- csrc/jg_model.h and host/joint.cpp compiled with ASan and UBSan as a
  stand-alone program (tools/micro/jg_test.cpp), which also runs the model in
  the kernel's lane layout.
- The joint command with the CPU mock of libfcship (the host path): its VCF is
  the restatement's byte for byte, every refusal names file and line, and
  synth -> htc -> joint for three samples round-trips.
- fcsjg_* is declared in include/fcsjg.h and exported, beside an unchanged
  fcship.h surface; bad arguments are refused before any device is looked for.
"""
import ctypes as C
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fcship
import host_lib as H
import jg_cases as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = H.lib
L.fcsg_jg_tables.argtypes = [C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
L.fcsg_jg_genotype.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
L.fcsg_bgzip_tabix.argtypes = [C.c_char_p, C.c_char_p]
CASES = J.hand_cases()
NAMES = ("q", "mle", "qual", "kept", "ac", "an", "dp", "pl_off", "src", "gt", "gq", "pl", "n_pl")


def host_tables(het, conf, n):
    S, LG, LP = np.zeros(J.S_ROWS, np.int32), np.zeros(4 * n + 1, np.int32), np.zeros(2 * n + 1, np.int32)
    q = C.c_int64(-1)
    H.check(L.fcsg_jg_tables(het, conf, n, S.ctypes.data, LG.ctypes.data, LP.ctypes.data, C.addressof(q)))
    return (S, LG, LP), q.value


def host_genotype(cohort, pos, n_alt, tabs, minq, threads=1, max_pl=None):
    return fcship.jg_genotype(cohort, pos, n_alt, tabs, minq, max_pl=max_pl,
                              entry=lambda c, s, m, o: H.check(L.fcsg_jg_genotype(c, s, m, threads, o)))


def same(got, want, what=""):
    for name in NAMES:
        assert np.array_equal(np.asarray(got[name]).reshape(-1), np.asarray(want[name]).reshape(-1)), (what, name)


# ------------------------------------------------------------------ the tables and the fixed point
@pytest.fixture(scope="module")
def mp():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 40
    return mpmath


def exact_s(mp, d_units):
    """10 log10(1 + 10^(-d / 10)) in units, d in units."""
    d = mp.mpf(int(d_units)) / J.ONE
    return 10 * mp.log10(1 + mp.power(10, -d / 10)) * J.ONE


@pytest.fixture(scope="module")
def table_error(mp):
    """e: the largest error of lse's table term over 20,000 random differences, the cut included."""
    S = J.tables(1e-3, 1)[0]
    rng = np.random.default_rng(20)
    d = np.concatenate([rng.integers(0, J.CUT, 19000), rng.integers(J.CUT, 2 * J.CUT, 1000), [0, J.CUT - 1, J.CUT]])
    got = J.lse(d, np.zeros_like(d), S) - d
    e = max(abs(float(exact_s(mp, x) - int(g))) for x, g in zip(d, got))
    drop = float(exact_s(mp, J.CUT))
    print(f"S table error e = {e:.2f} units over {len(d)} differences; drop at the cut {drop:.3f} unit")
    return e


def test_tables_equal_the_restatement_and_the_exactly_rounded_values(mp, table_error):
    for het, conf, n in ((1e-3, 10.0, 1), (1e-3, 10.0, 3), (0.01, 30.0, 200), (1e-3, 0.0, 1024)):
        want = J.tables(het, n)
        (hS, hLG, hLP), hq = host_tables(het, conf, n)
        dev = fcship.jg_tables(het, n)
        for a, b, c in zip(want, (hS, hLG, hLP), dev):
            assert np.array_equal(a, b) and np.array_equal(a, c) and b.dtype == np.int32
        assert hq == J.min_qual(conf) == round(conf * J.ONE)
    S, LG, LP = J.tables(1e-3, 1024)
    assert len(S) == 1282 and S.nbytes // 2 <= 5 * 1024 + 8 and len(LG) == 4097 and len(LP) == 2049
    assert list(S) == [int(mp.nint(exact_s(mp, i << 16))) for i in range(J.S_ROWS)]
    assert list(LG[1:]) == [int(mp.nint(10 * mp.log10(n) * J.ONE)) for n in range(1, 4097)]
    h = mp.mpf(1e-3)
    rest = 1 - sum(h / k for k in range(1, 2049))
    assert list(LP) == [int(mp.nint(10 * mp.log10(rest) * J.ONE))] + [int(mp.nint(10 * mp.log10(h / k) * J.ONE)) for k in range(1, 2049)]
    assert (np.diff(S) <= 0).all() and S[0] == round(10 * np.log10(2) * J.ONE) and S[1280] == 0 and S[1281] == 0
    assert table_error > 0.5          # measured, not a constant: the bound below is built from it
    assert fcship.lib.fcsjg_tables(1.0, 3, hS.ctypes.data, hLG.ctypes.data, hLP.ctypes.data) == fcship.FCS_ERR_INVALID
    assert fcship.lib.fcsjg_tables(1e-3, 1025, hS.ctypes.data, hLG.ctypes.data, hLP.ctypes.data) == fcship.FCS_ERR_INVALID
    assert fcship.lib.fcsjg_tables(0.2, 1024, hS.ctypes.data, hLG.ctypes.data, hLP.ctypes.data) == fcship.FCS_ERR_INVALID
    assert "leaves no prior for k = 0" in fcship.lib.fcs_last_error().decode()


def exact_qual(mp, cc, het):
    """The recurrence in 40-digit arithmetic: 10 log10(sum_k z_n[k] p_k / (z_n[0] p_0)) in units."""
    n = len(cc)
    z = [mp.mpf(1)]
    for j in range(1, n + 1):
        g = [mp.power(10, -mp.mpf(int(c)) / 10) for c in cc[j - 1]]
        old = z + [mp.mpf(0), mp.mpf(0)]
        z = []
        for k in range(2 * j + 1):
            v = (2 * j - k) * (2 * j - k - 1) * old[k] * g[0] if k <= 2 * j - 2 else mp.mpf(0)
            if k >= 1:
                v += 2 * k * (2 * j - k) * old[k - 1] * g[1]
            if k >= 2:
                v += k * (k - 1) * old[k - 2] * g[2]
            z.append(v / (2 * j * (2 * j - 1)))
    h = mp.mpf(het)
    p = [1 - sum(h / k for k in range(1, 2 * n + 1))] + [h / k for k in range(1, 2 * n + 1)]
    return 10 * mp.log10(sum(a * b for a, b in zip(z, p)) / (z[0] * p[0])) * J.ONE


@pytest.mark.parametrize("n", [1, 2, 3, 32, 33, 65, 200])
def test_qual_is_within_the_derived_bound_of_the_exact_recurrence(mp, table_error, n):
    """lse is 1-Lipschitz in the sup norm; a row adds two table errors and four half-unit LG roundings, the final sum
    2 n e at most, the priors 1: |QUAL - exact| <= n (4 e + 2) + 1 units."""
    rng = np.random.default_rng(100 + n)
    cc = rng.integers(0, 120, (1, n, 3))
    cc[0, rng.random(n) < 0.7, 0] = 0                    # most samples are reference
    cc[0, 0] = (60, 0, 80)                               # one carrier at least
    cc = cc - cc.min(2, keepdims=True)
    S, LG, LP = J.tables(1e-3, n)
    q, mle, _ = J.exact_model(cc, np.ones((1, n), bool), S, LG, LP)
    want = exact_qual(mp, cc[0], 1e-3)
    err, bound = abs(float(want - int(q[0]))), n * (4 * table_error + 2) + 1
    print(f"n = {n}: QUAL {int(q[0])} units, exact {float(want):.1f}, error {err:.1f} units, bound {bound:.0f}")
    assert err <= bound and int(q[0]) > 0


# ------------------------------------------------------------------ the hand cases
@pytest.mark.parametrize("name", list(CASES))
def test_hand_case(name):
    texts, opts, want = J.case_texts(CASES[name])
    got = J.command_vcf(texts, J.CONTIGS, conf=opts.get("conf", 10.0), header=False)
    assert got == want and want.count("\n") >= 1, (got, want)


def test_the_hand_cases_are_the_issue_s_and_none_is_vacuous():
    assert list(CASES) == ["one sample", "a site carried by one of three samples", "a block ending at p - 1, at p and at p + 1",
                           "a no-call from no coverage", "a no-call inside a deletion's span", "two ALTs at one POS",
                           "three ALTs at one POS", "a REF of differing length with ALT padding", "a seventh ALT cut",
                           "an ALT dropped by mle = 0", "all samples hom-alt", "equal PLs", "ties in GT", "a PL at the clamp",
                           "a site below the threshold"]
    col = lambda name, k=0: CASES[name][2].splitlines()[k].split("\t")  # noqa: E731
    assert len(col("one sample")) == 10
    assert [c.split(":")[0] for c in col("a site carried by one of three samples")[9:]] == ["1/1", "0/0", "0/0"]
    assert [c.split(":")[0] for c in col("a block ending at p - 1, at p and at p + 1")[9:]] == ["0/1", "./.", "0/0", "0/0"]
    assert col("a no-call from no coverage")[9:] == ["0/1:20:60:60,0,80", "./.", "./."]
    assert col("a no-call inside a deletion's span", 1)[1] == "52" and col("a no-call inside a deletion's span", 1)[10] == "./."
    assert col("two ALTs at one POS")[4] == "T,C" and col("three ALTs at one POS")[4] == "C,T,G"   # by samples, then by column
    assert col("a REF of differing length with ALT padding")[3:5] == ["ATCC", "ACC,GTCC,A"]
    assert col("a seventh ALT cut")[4].count(",") == 5 and col("a seventh ALT cut")[-1].startswith("0/0:20:10:0,10,90")
    assert col("an ALT dropped by mle = 0")[4] == "C" and col("an ALT dropped by mle = 0")[10] == "0/0:20:3:0,3,40"
    assert "AC=8;AF=1.00;AN=8" in col("all samples hom-alt")[7]
    assert col("equal PLs")[10:] == ["./.", "./."] and "DP=40" in col("equal PLs")[7]
    assert [c.split(":")[0] for c in col("ties in GT")[9:]] == ["0/0", "0/1"] and ":0:0,0,50" in col("ties in GT")[9]
    assert "1048575,0,1048575" in col("a PL at the clamp")[9]
    assert CASES["a site below the threshold"][2].count("\n") == 1 and col("a site below the threshold")[1] == "150"
    # the site that is not written was a site: its QUAL lies below the threshold, its ALT has mle > 0
    texts, _, _ = J.case_texts(CASES["a site below the threshold"])
    parsed = sorted((J.parse_gvcf(t) for t in texts), key=lambda p: p[0])
    cohort, pos, n_alt, _, _ = J.combine([p[2]["ctgA"] for p in parsed])
    o = J.genotype(cohort, pos, n_alt, J.tables(1e-3, 2), J.min_qual())
    assert list(pos) == [139, 149] and o["kept"][0] == 1 and 0 < o["qual"][0] < J.min_qual() and o["pl_off"][0] == -1


def test_ties_in_mle_go_to_the_smaller_k():
    cohort, pos, n_alt, tabs = J.flat_prior_case()
    o = J.genotype(cohort, pos, n_alt, tabs, 0)
    assert list(o["mle"][[0, 6]]) == [1, 0] and list(o["kept"]) == [1, 0] and list(o["pl_off"]) == [0, -1]
    for threads in (1, 16):
        same(host_genotype(cohort, pos, n_alt, tabs, 0, threads), o)


# ------------------------------------------------------------------ the host path
@pytest.mark.parametrize("seed,n,sites,max_alt", [(1, 1, 40, 1), (2, 3, 300, 3), (3, 33, 30, 6), (4, 65, 12, 2), (5, 130, 6, 3)])
def test_host_path_equals_the_restatement_on_1_and_16_threads(seed, n, sites, max_alt):
    cohort, pos, n_alt = J.random_cohort(seed, n, sites, max_alt)
    tabs = J.tables(1e-3, n)
    want = J.genotype(cohort, pos, n_alt, tabs, J.min_qual())
    written = int((want["pl_off"] >= 0).sum())
    assert (want["src"] >= 0).sum() > len(pos) * n // 2 and written > 0 and (want["gt"] == 255).any()
    assert sites < 100 or (written < len(pos) and (want["kept"] == 0).any() and (want["mle"] > 1).any())
    for threads in (1, 16):
        same(host_genotype(cohort, pos, n_alt, tabs, J.min_qual(), threads), want, (seed, threads))
    # capacity: exactly enough, and one too few
    need = int(want["n_pl"][0])
    same(host_genotype(cohort, pos, n_alt, tabs, J.min_qual(), 1, max_pl=need), want)
    with pytest.raises(RuntimeError, match=f"have {need} PLs, max_pl is {need - 1}"):
        host_genotype(cohort, pos, n_alt, tabs, J.min_qual(), 1, max_pl=need - 1)


# ------------------------------------------------------------------ jg_model.h and joint.cpp under sanitizers
@pytest.fixture(scope="module")
def jg_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("jg") / "jg_test"
    pkg = os.path.join(ROOT, "falcon-genome_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"), "-I" + os.path.join(pkg, "host"),
                    os.path.join(ROOT, "tools", "micro", "jg_test.cpp"), os.path.join(pkg, "host", "joint.cpp"), "-o", str(exe)],
                   check=True)
    return exe


@pytest.mark.parametrize("seed,n,sites", [(1, 1, 50), (2, 3, 300), (3, 32, 40), (4, 65, 20), (5, 130, 8), (6, 544, 2), (7, 4, 0)])
def test_shared_model_host_build_in_the_kernel_s_lane_layout(jg_exe, seed, n, sites):
    r = subprocess.run([str(jg_exe), str(seed), str(n), str(sites)], capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "MISMATCH" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    fig = dict(zip(r.stdout.split()[0::2], r.stdout.split()[1::2]))
    if sites:
        assert int(fig["sources"]) > 0 and int(fig["written"]) > 0 and int(fig["pls"]) >= 3 * n
        assert int(fig["passes"]) == next(p for p in (1, 2, 3, 5, 9, 17, 33) if 2 * n + 1 <= 64 * p)


# ------------------------------------------------------------------ the ABI
def last_error():
    return fcship.lib.fcs_last_error().decode()


def test_symbols_declared_and_exported_beside_an_unchanged_fcship_h():
    names = ["fcsjg_genotype", "fcsjg_genotype_dev", "fcsjg_tables", "fcsjg_workspace_bytes"]
    assert fcship.jg_header_symbols() == names
    nm = subprocess.run(["nm", "-D", "--defined-only", fcship.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("fcsjg_")}
    assert exported == set(names)
    assert fcship.lib.fcs_abi_symbol_count() == len(fcship.header_symbols()) == 61
    assert not [s for s in fcship.header_symbols() if "jg" in s.split("_")]
    assert (C.sizeof(fcship.JgCohort), C.sizeof(fcship.JgSites), C.sizeof(fcship.JgModel), C.sizeof(fcship.JgOut)) == (72, 24, 32, 112)
    header = open(fcship.JG_HEADER_PATH).read()
    for name in ("SAMPLES_MAX", "ALTS_MAX", "PL_MAX", "UNIT_BITS", "S_ROWS", "GENOTYPES_MAX", "KIND_BLOCK", "KIND_CALL", "NO_CALL",
                 "STATUS_FIELD", "STATUS_PL"):
        assert re.search(rf"#define FCSJG_{name} {getattr(fcship, 'FCSJG_' + name)}\b", header), name
    assert 1024 <= fcship.FCSJG_SAMPLES_MAX <= 4096 and fcship.FCSJG_PL_MAX == J.PL_MAX == 2**20 - 1
    mock = subprocess.run(["nm", "-D", "--defined-only", f"{ROOT}/tests/cpu_mock/build/libfcship.so"],
                          capture_output=True, text=True).stdout
    assert "fcs_phmm" in mock and "fcsjg_" not in mock


def test_arguments_are_checked_before_the_device():
    cohort, pos, n_alt = J.random_cohort(9, 3, 20, 3)
    tabs = J.tables(1e-3, 3)

    def call(cohort=cohort, pos=pos, n_alt=n_alt, device=99, **kw):
        try:
            fcship.jg_genotype(cohort, pos, n_alt, tabs, J.min_qual(), device=device, **kw)
        except fcship.FcsError as e:
            return e.code, str(e)
        return 0, ""

    def swapped(k, f):
        a = [np.array(x) for x in cohort]
        f(a[k])
        return tuple(a)

    def set_at(i, v):
        def f(a):
            a.reshape(-1)[i] = v
        return f

    r0 = int(cohort[0][1])   # the first record of sample 1
    for kw, what in ((dict(n_samples=0), "a cohort of 0 samples (1 to 1024)"),
                     (dict(n_samples=1025), "a cohort of 1025 samples"),
                     (dict(n_records=-1), "negative record count"),
                     (dict(max_pl=-1), "max_pl -1"),
                     (dict(cohort=swapped(0, set_at(1, int(cohort[0][2]) + 1))), "record offsets out of order at record 1"),
                     (dict(n_records=len(cohort[1]) - 1), "record offsets end at"),
                     (dict(cohort=swapped(1, set_at(r0 + 1, -5))), "record 1 of sample 1 spans -5"),
                     (dict(cohort=swapped(2, set_at(r0, int(cohort[1][r0])))), "record 0 of sample 1 spans"),
                     (dict(cohort=swapped(1, set_at(r0 + 2, int(cohort[1][r0 + 1]) - 1))), "positions decrease"),
                     (dict(cohort=swapped(3, set_at(2, 2))), "record 2 of sample 0 has kind 2"),
                     (dict(cohort=swapped(4, set_at(2, 7))), "record 2 of sample 0 has ALT index 7"),
                     (dict(cohort=swapped(5, set_at(0, -1))), "record 0 of sample 0 has DP -1"),
                     (dict(cohort=swapped(6, set_at(1, 1 << 20))), "record 0 of sample 0 has a PL of 1048576 (0 to 1048575)"),
                     (dict(cohort=swapped(6, set_at(6, -1))), "record 1 of sample 0 has a PL of -1"),
                     (dict(pos=np.r_[pos[:3], pos[2], pos[4:]]), "site 3 at position"),
                     (dict(n_alt=np.r_[n_alt[:5], 0, n_alt[6:]]), "site 5 has 0 ALTs (1 to 6)"),
                     (dict(n_alt=np.r_[n_alt[:5], 7, n_alt[6:]]), "site 5 has 7 ALTs")):
        rc, err = call(**kw)
        assert rc == fcship.FCS_ERR_INVALID and "[E::fcsjg_genotype]" in err and what in err, (kw.keys(), err)
    # nothing is written on a refusal
    arrays = fcship.jg_out_arrays(len(pos), 3, 100, fill=7)
    c, keep = fcship.jg_cohort(*cohort)
    p32, a8 = pos.astype(np.int32), np.r_[n_alt[:5], 9, n_alt[6:]].astype(np.uint8)
    S, LG, LP = (np.ascontiguousarray(t, np.int32) for t in tabs)
    st, m, o = fcship.JgSites(len(pos), p32.ctypes.data, a8.ctypes.data), fcship.JgModel(S.ctypes.data, LG.ctypes.data, LP.ctypes.data, 0), fcship.jg_out(arrays)
    addr = [C.addressof(x) for x in (c, st, m, o)]
    assert fcship.lib.fcsjg_genotype(0, *addr) == fcship.FCS_ERR_INVALID and all((v == 7).all() for v in arrays.values())
    for k, what in enumerate(("null cohort", "null sites", "null model", "null outputs")):
        assert fcship.lib.fcsjg_genotype(0, *(None if i == k else a for i, a in enumerate(addr))) == fcship.FCS_ERR_INVALID
        assert what in last_error()
    # a good cohort on a device that is not there: the device error comes after every check
    rc, err = call()
    assert rc in (fcship.FCS_ERR_INVALID, fcship.FCS_ERR_DEVICE) and "[E::fcsjg_genotype]" not in err
    # an empty site list needs no device
    out = fcship.jg_genotype(cohort, pos[:0], n_alt[:0], tabs, 0, device=99)
    assert out["n_pl"][0] == 0 and len(out["pl"]) == 0
    assert fcship.lib.fcsjg_workspace_bytes(-1, 3) == fcship.FCS_ERR_INVALID and "[E::fcsjg_workspace_bytes]" in last_error()
    assert fcship.lib.fcsjg_workspace_bytes(10, 1025) == fcship.FCS_ERR_INVALID
    assert 0 < fcship.lib.fcsjg_workspace_bytes(0, 1) <= fcship.lib.fcsjg_workspace_bytes(1 << 20, 1024) <= 1 << 24
    a8[5] = 1
    one = np.zeros(64, np.uint8).ctypes.data   # stands for device memory: never dereferenced
    assert fcship.lib.fcsjg_genotype_dev(0, *addr, one, 16, one, None) == fcship.FCS_ERR_INVALID
    assert "[E::fcsjg_genotype_dev]" in last_error() and "the workspace holds 16 bytes" in last_error()
    assert fcship.lib.fcsjg_genotype_dev(0, *addr, one, 1 << 20, None, None) == fcship.FCS_ERR_INVALID
    assert "null workspace or status" in last_error()


# ------------------------------------------------------------------ the command, on the host path
@pytest.fixture(scope="module")
def mock_env():
    subprocess.run(["make", "-C", f"{ROOT}/tests/cpu_mock"], check=True, capture_output=True)
    return {"LD_LIBRARY_PATH": f"{ROOT}/tests/cpu_mock/build", "FCS_GPU_DEVICES": "0", "FCS_JOINT_GPU": "false"}


def write_ref(d, contigs=J.CONTIGS):
    os.makedirs(d, exist_ok=True)
    with open(d / "ref.fa", "w") as f:
        for k, (name, ln) in enumerate(contigs):
            seq = (("ACGT"[k % 4] * 7 + "GATTACA") * (ln // 14 + 1))[:ln]
            f.write(f">{name}\n" + "".join(seq[i:i + 60] + "\n" for i in range(0, ln, 60)))
    return d / "ref.fa"


def write_inputs(d, texts, gz=()):
    """The texts as f<k>.g.vcf (or, for k in gz, bgzipped as f<k>.gvcf.gz) under d/in."""
    os.makedirs(d / "in", exist_ok=True)
    for k, t in enumerate(texts):
        (d / "in" / f"f{k}.g.vcf").write_text(t)
        if k in gz:
            H.check(L.fcsg_bgzip_tabix(str(d / "in" / f"f{k}.g.vcf").encode(), str(d / "in" / f"f{k}.gvcf.gz").encode()))
            os.remove(d / "in" / f"f{k}.g.vcf")
            os.remove(d / "in" / f"f{k}.gvcf.gz.tbi")
    return d / "in"


def run_joint(out, ref, indir, *extra, env=None, cwd=None):
    return H.run_cli("joint", "-r", ref, "-i", indir, "-o", out, *extra, env=env, cwd=cwd)


def test_command_writes_the_hand_cases_expected_lines(mock_env, tmp_path):
    ref = write_ref(tmp_path)
    for k, (name, case) in enumerate(CASES.items()):
        texts, opts, want = J.case_texts(case)
        d = tmp_path / f"c{k}"
        env = dict(mock_env, **({"FCS_JOINT_STAND_CALL_CONF": str(opts["conf"])} if "conf" in opts else {}))
        p = run_joint(d / "out.vcf", ref, write_inputs(d, texts), env=env)
        assert p.returncode == 0 and "(host)" in p.stderr, (name, p.stderr[-2000:])
        got = open(d / "out.vcf").read()
        assert got == J.header_text(sorted(case[0]), J.CONTIGS) + want, name
        assert ("5 PLs clamped" if name == "a PL at the clamp" else "0 PLs clamped") in p.stderr, name
        assert ("1 ALTs cut" if name == "a seventh ALT cut" else "0 ALTs cut") in p.stderr, name


def test_command_on_random_gvcfs_writes_the_restatement_s_vcf(mock_env, tmp_path):
    ref = write_ref(tmp_path)
    texts = J.random_gvcfs(31, 5)
    want = J.command_vcf(texts, J.CONTIGS)
    body = [ln for ln in want.splitlines() if not ln.startswith("#")]
    assert len(body) > 20 and sum("./." in ln for ln in body) > 3 and sum("," in ln.split("\t")[4] for ln in body) > 2
    assert {ln.split("\t")[0] for ln in body} == {"ctgA", "ctgB"} and any(len(ln.split("\t")[3]) > 1 for ln in body)
    indir = write_inputs(tmp_path, texts, gz=(1, 3))
    (indir / "notes.txt").write_text("not a GVCF\n")
    p = run_joint(tmp_path / "out.vcf", ref, indir, "--sample-id", "x", "--database_name", "db", env=mock_env, cwd=tmp_path)
    assert p.returncode == 0 and "(host)" in p.stderr and "entry point" not in p.stderr, p.stderr[-2000:]
    assert "--database_name db: ignored" in p.stderr and f"5 samples, " in p.stderr and f" {len(body)} written" in p.stderr
    got = open(tmp_path / "out.vcf").read()
    assert got == want
    assert gzip.decompress(open(tmp_path / "out.vcf.gz", "rb").read()).decode() == got
    names, _ = H.parse_index(gzip.decompress(open(tmp_path / "out.vcf.gz.tbi", "rb").read()), b"TBI\x01")
    assert names == ["ctgA", "ctgB"]
    # chunks of 7 sites and of one: the same bytes
    for chunk in ("7", "1"):
        p = run_joint(tmp_path / f"c{chunk}.vcf", ref, indir, env=dict(mock_env, FCS_JOINT_CHUNK_SITES=chunk))
        assert p.returncode == 0 and open(tmp_path / f"c{chunk}.vcf").read() == want, p.stderr[-2000:]
    # joint.max_alt and the threshold are the restatement's
    p = run_joint(tmp_path / "m.vcf", ref, indir, env=dict(mock_env, FCS_JOINT_MAX_ALT="1", FCS_JOINT_STAND_CALL_CONF="40.5",
                                                            FCS_JOINT_HETEROZYGOSITY="0.01"))
    assert p.returncode == 0 and open(tmp_path / "m.vcf").read() == J.command_vcf(texts, J.CONTIGS, het=0.01, conf=40.5, max_alt=1)
    assert " ALTs cut" in p.stderr and ", 0 ALTs cut" not in p.stderr
    # the output exists: refused without -f, overwritten with it
    assert run_joint(tmp_path / "out.vcf", ref, indir, env=mock_env).returncode == 1
    os.remove(tmp_path / "out.vcf")
    p = run_joint(tmp_path / "out.vcf", ref, indir, env=mock_env)
    assert p.returncode == 1 and "out.vcf.gz exists (use -f)" in p.stderr
    assert run_joint(tmp_path / "out.vcf", ref, indir, "-f", env=mock_env).returncode == 0
    assert open(tmp_path / "out.vcf").read() == want
    # options refused, missing files and arguments, help, usage, configuration
    for opt, what in (("--combine-only", "no combined GVCF is written"), ("-g", "no combined GVCF is read")):
        p = run_joint(tmp_path / "x", ref, indir, opt, env=mock_env)
        assert p.returncode == 1 and what in p.stderr
    assert run_joint(tmp_path / "x", tmp_path / "none.fa", indir, env=mock_env).returncode == 3
    assert run_joint(tmp_path / "x", ref, tmp_path / "none", env=mock_env).returncode == 3
    assert run_joint(tmp_path / "x", ref, ref, env=mock_env).returncode == 3
    os.makedirs(tmp_path / "empty")
    p = run_joint(tmp_path / "x", ref, tmp_path / "empty", env=mock_env)
    assert p.returncode == 1 and "holds no *.gvcf.gz" in p.stderr
    p = H.run_cli("joint", "-r", ref, "-o", tmp_path / "x", env=mock_env)
    assert p.returncode == 1 and "--input-dir is required" in p.stderr
    h = H.run_cli("joint", "--help", env=mock_env)
    assert h.returncode == 0
    for opt in ("--input-dir", "--sample-id", "--database_name", "--combine-only", "--skip-combine"):
        assert opt in h.stderr
    assert "  joint  " in H.run_cli(env=mock_env).stdout
    conf = H.run_cli("conf", env=mock_env)
    conf = conf.stdout + conf.stderr
    for key, value in (("joint.gpu", "false"), ("joint.stand_call_conf", "10"), ("joint.heterozygosity", "0.001"), ("joint.max_alt", "6"),
                       ("joint.chunk_sites", "0")):
        assert f"{key} = {value} " in conf, key
    assert not os.path.exists(tmp_path / "x")


def test_every_refusal_names_file_and_line(mock_env, tmp_path):
    ref = write_ref(tmp_path)
    good = {"s1": {"ctgA": [J.block(1, 9), J.call(10, "A", "G", J.HET), J.block(11, 50)], "ctgB": [J.block(1, 20)]}}
    base = J.gvcf_text("s1", J.CONTIGS, good["s1"]).splitlines()
    first = next(k for k, ln in enumerate(base) if not ln.startswith("#"))   # 0-based index of the first record: line first + 1

    def edited(k, f):
        lines = list(base)
        lines[k] = f(lines[k])
        return "\n".join(x for x in lines if x is not None) + "\n"

    def swap(lines_fn):
        return "\n".join(lines_fn(list(base))) + "\n"

    cases = [
        (edited(first + 1, lambda ln: ln.replace("G,<NON_REF>", "G")), first + 2, "does not end in <NON_REF>"),
        (edited(first + 1, lambda ln: ln.replace("G,<NON_REF>", "G,T,<NON_REF>")), first + 2, "more than one allele beside <NON_REF>"),
        (edited(first + 1, lambda ln: ln.replace("G,<NON_REF>", "<DEL>,<NON_REF>")), first + 2, "a symbolic or missing allele"),
        (edited(first + 1, lambda ln: ln.replace("0/1:", "0/1/1:")), first + 2, "ploidy is not 2"),
        (edited(first + 1, lambda ln: ln.replace("0/1:", "1:")), first + 2, "ploidy is not 2"),
        (edited(first + 1, lambda ln: ln.replace(":PL\t", ":XX\t")), first + 2, "no PL"),
        (edited(first + 1, lambda ln: ln.replace("60,0,80,90,100,200", ".")), first + 2, "no PL"),
        (edited(first + 1, lambda ln: ln.replace("60,0,80,90,100,200", "60,0,80")), first + 2, "3 PLs, a call has 6"),
        (edited(first + 1, lambda ln: ln.replace("60,0,80,90,100,200", "60,0,-1,90,100,200")), first + 2, "PL -1"),
        (edited(first, lambda ln: ln.replace("0,30,300", "0,30,300,4,5,6")), first + 1, "6 PLs, a block has 3"),
        (edited(first, lambda ln: ln.replace("END=9", "DP=3")), first + 1, "a <NON_REF> block without END="),
        (edited(first + 2, lambda ln: ln.replace("END=50", "END=10")), first + 3, "END=10 at POS 11"),
        (edited(first + 2, lambda ln: ln.replace("\t11\t", "\t9\t")), first + 3, "POS 9 follows 10: unsorted positions"),
        (edited(first + 2, lambda ln: ln.replace("\t11\t", "\t1001\t")), first + 3, "POS 1001"),
        (edited(first + 2, lambda ln: ln + "\textra"), first + 3, "11 columns, not 10"),
        (edited(first + 2, lambda ln: ln.replace("ctgA", "ctgX")), first + 3, "contig ctgX is not in the reference"),
        (swap(lambda ls: ls[:first] + ls[first + 3:] + ls[first:first + 3]), first + 2, "contig ctgA follows ctgB: unsorted contigs"),
        (edited(first - 1, lambda ln: ln + "\ts2"), first, "the #CHROM line names 2 samples, not one"),
        (edited(first - 2, lambda ln: ln.replace("length=400", "length=401")), first - 1, "contig ctgB of 401 bases is not contig 2 of the reference"),
        (swap(lambda ls: ls[:first - 2] + ls[first - 1:]), first - 1, "the header has 1 ##contig lines, the reference 2 contigs"),
    ]
    for k, (text, line, what) in enumerate(cases):
        d = tmp_path / f"r{k}"
        indir = write_inputs(d, [J.gvcf_text("s0", J.CONTIGS, good["s1"]), text])
        p = run_joint(d / "out.vcf", ref, indir, env=mock_env)
        assert p.returncode == 4 and f"[E::joint] {indir}/f1.g.vcf:{line}: " in p.stderr and what in p.stderr, (what, p.stderr[-600:])
        assert not os.path.exists(d / "out.vcf") and not os.path.exists(d / "out.vcf.gz")
    # two files of one sample
    d = tmp_path / "dup"
    indir = write_inputs(d, [J.gvcf_text("s1", J.CONTIGS, good["s1"])] * 2)
    p = run_joint(d / "out.vcf", ref, indir, env=mock_env)
    assert p.returncode == 4 and "both hold sample s1" in p.stderr and "f0.g.vcf" in p.stderr and "f1.g.vcf" in p.stderr
    # what is counted, not refused: a second call record at one POS, PLs above the clamp
    twice = edited(first + 1, lambda ln: ln + "\n" + ln.replace("\tG,<NON_REF>", "\tT,<NON_REF>").replace("60,0,80", "0,70,5000000"))
    d = tmp_path / "twice"
    p = run_joint(d / "out.vcf", ref, write_inputs(d, [twice]), env=mock_env)
    assert p.returncode == 0 and "0 PLs clamped, 1 calls ignored" in p.stderr, p.stderr[-600:]
    assert open(d / "out.vcf").read() == J.command_vcf([twice], J.CONTIGS) and "\tG\t" in open(d / "out.vcf").read()


def test_round_trip_synth_htc_joint_for_three_samples(mock_env, tmp_path):
    d = tmp_path / "s"
    p = H.run_cli("synth", "-o", d, "-c", "chr1:24000,chr2:9000", "-x", "14", "--seed", "17", "--no-fastq", "--tumor",
                  "--tumor-coverage", "10")
    assert p.returncode == 0, p.stderr[-2000:]
    p = H.run_cli("synth", "-o", tmp_path / "t", "-c", "chr1:24000,chr2:9000", "-x", "14", "--seed", "17", "--no-fastq",
                  "--max-reads", "2200")
    assert p.returncode == 0, p.stderr[-2000:]
    env = dict(mock_env, FCS_MOCK_PHMM="gkl", FCS_LOG_DIR=str(tmp_path / "log"))
    os.makedirs(tmp_path / "in")
    texts = []
    for name, bam in (("one", d / "sample.bam"), ("two", d / "tumor.bam"), ("three", tmp_path / "t" / "sample.bam")):
        p = H.run_cli("htc", "-f", "-r", d / "ref.fasta", "-i", bam, "-o", tmp_path / f"{name}.g.vcf", env=env, cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-3000:]
        text = gzip.decompress(open(tmp_path / f"{name}.g.vcf.gz", "rb").read()).decode()
        head, _, body = text.partition("#CHROM")
        line, _, rest = body.partition("\n")
        text = head + "#CHROM" + "\t".join(line.split("\t")[:9] + [name]) + "\n" + rest   # the three BAMs name one sample
        texts.append(text)
        (tmp_path / "in" / f"{name}.g.vcf").write_text(text)
    p = run_joint(tmp_path / "out.vcf", d / "ref.fasta", tmp_path / "in", env=mock_env, cwd=tmp_path)
    assert p.returncode == 0 and "3 samples" in p.stderr, p.stderr[-2000:]
    got = open(tmp_path / "out.vcf").read()
    contigs = [("chr1", 24000), ("chr2", 9000)]
    assert got == J.command_vcf(texts, contigs)
    parsed = sorted((J.parse_gvcf(t) for t in texts), key=lambda q: q[0])
    assert [q[0] for q in parsed] == ["one", "three", "two"]
    calls = {}   # (contig, 0-based pos) -> {column: (ref, alt)}
    for col, (_, _, recs) in enumerate(parsed):
        for chrom, rs in recs.items():
            for r in rs:
                if r["kind"] == J.CALL:
                    calls.setdefault((chrom, r["beg"]), {})[col] = (r["ref"], r["alt"])
    body = [ln.split("\t") for ln in got.splitlines() if not ln.startswith("#")]
    assert len(body) >= 5 and len(calls) >= len(body)
    shared = 0
    for f in body:
        at = calls[(f[0], int(f[1]) - 1)]
        ref = max((r for r, _ in at.values()), key=len)
        named = {col: a + ref[len(r):] for col, (r, a) in at.items()}
        assert f[3] == ref and set(f[4].split(",")) <= set(named.values())
        for col, sample in enumerate(f[9:]):
            gt = sample.split(":")[0]
            carried = {f[4].split(",")[int(x) - 1] for x in gt.split("/") if x not in (".", "0")}
            if col in named:   # a carrier with a call record here named the ALT in it
                assert carried <= {named[col]}, (f[:5], col, sample)
            elif carried:      # one without is under a block, whose <NON_REF> stands for every ALT
                assert any(r["kind"] == J.BLOCK and r["beg"] < int(f[1]) <= r["end"] for r in parsed[col][2][f[0]]), (f[:5], col)
        shared += sum(col in named and s.split(":")[0] not in ("./.", "0/0") for col, s in enumerate(f[9:])) >= 2
    assert shared >= 2   # the samples share variants: sites carried by several
