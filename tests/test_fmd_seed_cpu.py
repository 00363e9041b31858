"""FMD-index seeding checks that need no GPU.

- The per-read logic the kernels run (falcon-genome_amd/csrc/fmd_smem.h: occ4,
  the extension, bwt_smem1, mem_collect_intv's rounds, the LF walk), compiled
  for the host with ASan and UBSan (tools/micro/fmd_smem_test.cpp), equals
  FmdIndex::collect / locate on every SMEM field and position: on the tool's
  own references and on the batches the GPU test uses, whose largest SMEM
  count stays under the default max_mems.
- The new entry points are declared, exported and counted, refuse bad
  arguments before they look for a device, and answer FCS_ERR_DEVICE without
  one.
- `fcs-genome align` with bwa.gpu_seed=true against the CPU mock of libfcship
  (which has no fcs_fmd_* entry points) falls back to host seeding, says so
  once, and writes the BAM of a run with the key off.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fcship
import fmd_seed_cases as S
import host_lib as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fcs_fmd_index_create", "fcs_fmd_index_destroy", "fcs_fmd_collect", "fcs_fmd_collect_arena_bytes",
         "fcs_fmd_collect_dev", "fcs_fmd_locate", "fcs_fmd_locate_dev"]


@pytest.fixture(scope="module")
def smem_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("fmd") / "fmd_smem_test"
    pkg = os.path.join(ROOT, "falcon-genome_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(pkg, "csrc"), "-I" + os.path.join(pkg, "host"),
                    os.path.join(ROOT, "tools", "micro", "fmd_smem_test.cpp"), os.path.join(pkg, "host", "fmindex.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def run(exe, *args):
    return subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True,
                          env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})


def figures(out):
    """{(sa_intv, min_len, split_len, max_mem_intv): {name: value}} of the tool's lines."""
    rows = {}
    for m in re.finditer(r"sa_intv (\d+) min_len (\d+) split_len (\d+) max_mem_intv (\d+): (.*)", out):
        f = m.group(5).split()
        rows[tuple(int(m.group(k)) for k in range(1, 5))] = {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}
    return rows


def test_shared_logic_host_build_equals_the_index(smem_exe):
    r = run(smem_exe)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "MISMATCH" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    low = figures(r.stdout.split("low-complexity", 1)[1])
    # the poly-A read over the 100-base homopolymer fills a stack to the homopolymer's length
    assert low[(1, 19, 28, 20)]["max_depth"] == 100


def test_gpu_test_batches_on_the_host_build(smem_exe, tmp_path):
    """The GPU test's plain batch through the host build: equal to the index at
    every parameter set, and no read has more SMEMs than the default max_mems
    (so the GPU test's fallback count of 0 cannot hide a kernel's failure)."""
    f = tmp_path / "plain.txt"
    S.write_tool_input(f, S.plain_ref(), S.plain_batch())
    r = run(smem_exe, f)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    rows = figures(r.stdout)
    print(r.stdout)
    for min_len, split_len, _, max_mem_intv in S.PARAM_SETS:
        row = rows[(1, min_len, split_len, max_mem_intv)]
        assert row["reads"] == len(S.plain_batch())
        assert 0 < row["max_smems"] <= S.MAX_MEMS_DEFAULT, row
    assert all(rows[(intv,) + (19, 28, 20)]["located"] > 0 for intv in (4, 7, 32))
    f = tmp_path / "low.txt"
    S.write_tool_input(f, S.low_ref(), S.low_batch())
    r = run(smem_exe, f)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert figures(r.stdout)[(1, 19, 28, 20)]["max_depth"] == 100


def test_seed_batch_hook_on_the_host_index():
    """fcsg_fmd_seed_batch(gpu=0) is FmdIndex::collect / locate: the SMEMs and
    positions fcsg_fmd_smems returns read by read."""
    from test_fmindex import smems
    contigs, reads = S.plain_ref(), S.plain_batch()[:40]
    mems, loc, fallback = S.seed_batch(contigs, reads, 0, S.BWA, max_occ=10**6, sa_intv=4)
    assert fallback == 0
    for q, m, l in zip(reads, mems, loc):
        want, wloc = smems(list(contigs), q, *S.BWA, loc_cap=max(len(l), 1))
        assert [tuple(int(x) for x in row[:3]) for row in m] == want
        assert np.array_equal(l, wloc[:len(l)])


def test_symbols_declared_exported_and_counted():
    syms = fcship.header_symbols()
    assert all(n in syms for n in NAMES)
    assert all(hasattr(fcship.lib, n) for n in NAMES)
    assert fcship.lib.fcs_abi_symbol_count() == len(syms)
    assert f"#define FCS_FMD_MAX_MEMS_DEFAULT {S.MAX_MEMS_DEFAULT}" in open(fcship.HEADER_PATH).read()
    assert fcship.FCS_FMD_MAX_MEMS_DEFAULT == S.MAX_MEMS_DEFAULT
    assert fcship.FMD_MEM.itemsize == 32 and C.sizeof(fcship.FmdParams) == 24


def tiny_index():
    """Arrays with the layout fcs_fmd_index_create checks (their content is never read without a device)."""
    n_rows = 100
    occ = np.zeros(8 * ((n_rows + 63) // 64 + 1), np.uint64)
    Carr = np.array([0, 1, 30, 50, 70, 99], np.int64)
    sa = np.zeros((n_rows + 3) // 4, np.uint64)
    rows = np.array([3, 9], np.int64)
    return occ, Carr, n_rows, sa, rows, np.array([5, 6], np.int64)


def last_error():
    return fcship.lib.fcs_last_error().decode()


def test_arguments_are_checked_before_the_device():
    lib = fcship.lib
    occ, Carr, n_rows, sa, rows, ssa = tiny_index()
    h = C.c_void_p()

    def create(**kw):
        a = dict(occ=occ.ctypes.data, n_occ=len(occ), C=Carr.ctypes.data, n_rows=n_rows, sa=sa.ctypes.data,
                 n_sa=len(sa), intv=4, rows=rows.ctypes.data, ssa=ssa.ctypes.data, ns=2, flen=49, h=C.byref(h))
        a.update(kw)
        return lib.fcs_fmd_index_create(0, a["occ"], a["n_occ"], a["C"], a["n_rows"], a["sa"], a["n_sa"], a["intv"],
                                        a["rows"], a["ssa"], a["ns"], a["flen"], a["h"])
    bad_rows = np.array([9, 3], np.int64)
    bad_C = np.array([0, 40, 30, 50, 70, 99], np.int64)
    for kw in (dict(occ=None), dict(C=None), dict(n_rows=0), dict(intv=0), dict(n_occ=len(occ) - 8), dict(n_sa=3),
               dict(sa=None), dict(rows=None), dict(ns=-1), dict(flen=-1), dict(h=None),
               dict(rows=bad_rows.ctypes.data), dict(C=bad_C.ctypes.data)):
        assert create(**kw) == fcship.FCS_ERR_INVALID, kw
        assert "[E::fcs_fmd_index_create]" in last_error(), kw
    assert lib.fcs_fmd_index_destroy(None) == fcship.FCS_OK
    # never a handle of this library: refused, not followed
    fake = (C.c_char * 256)()
    assert lib.fcs_fmd_index_destroy(C.addressof(fake)) == fcship.FCS_ERR_INVALID
    assert "[E::fcs_fmd_index_destroy]" in last_error()

    codes = np.zeros(100, np.uint8)
    q_off, q_len = np.array([0, 50], np.int64), np.array([50, 50], np.int32)
    mems = np.zeros((2, 4), fcship.FMD_MEM)
    nm, ov = np.zeros(2, np.int32), np.zeros(2, np.int32)

    def collect(handle=None, n_bytes=100, off=q_off, qlen=q_len, n=2, P=fcship.FmdParams(19, 28, 10, 4, 20)):
        return lib.fcs_fmd_collect(handle, codes.ctypes.data, n_bytes, off.ctypes.data, qlen.ctypes.data, n,
                                   C.addressof(P) if P is not None else None, mems.ctypes.data, nm.ctypes.data,
                                   ov.ctypes.data)
    for kw, what in ((dict(), "null index handle"),
                     (dict(handle=C.addressof(fake)), "not a live one"),
                     (dict(n=-1), "bad arguments"),
                     (dict(n_bytes=-1), "bad arguments"),
                     (dict(P=None), "null params"),
                     (dict(qlen=np.array([50, -1], np.int32)), "negative length"),
                     (dict(off=np.array([0, 51], np.int64)), "leaves the 100 code bytes"),
                     (dict(off=np.array([-1, 50], np.int64)), "leaves the 100 code bytes"),
                     (dict(P=fcship.FmdParams(19, 28, 10, 0, 20)), "max_mems 0 < 1"),
                     (dict(P=fcship.FmdParams(-1, 28, 10, 4, 20)), "negative min_len")):
        assert collect(**kw) == fcship.FCS_ERR_INVALID, kw
        assert "[E::fcs_fmd_collect]" in last_error() and what in last_error(), (kw, last_error())
    P = fcship.FmdParams(19, 28, 10, 0, 20)
    assert lib.fcs_fmd_collect_dev(None, None, 0, None, None, None, 0, 151, C.addressof(P), None, 0, None, None, None,
                                   None) == fcship.FCS_ERR_INVALID
    assert "[E::fcs_fmd_collect_dev]" in last_error() and "max_mems 0 < 1" in last_error()
    P = fcship.FmdParams(19, 28, 10, 4, 20)
    one = np.zeros(64, np.uint8).ctypes.data  # never dereferenced: the arena is too small
    assert lib.fcs_fmd_collect_dev(None, one, 10, one, one, None, 1, 151, C.addressof(P), one, 64, one, one, one,
                                   None) == fcship.FCS_ERR_INVALID
    assert "the arena holds 64 bytes" in last_error()
    assert lib.fcs_fmd_collect_arena_bytes(-1, 151) == fcship.FCS_ERR_INVALID
    assert lib.fcs_fmd_collect_arena_bytes(1, 151) == 64 * 2 * 152 * 32            # one block of 64 quads
    assert lib.fcs_fmd_collect_arena_bytes(10**6, 151) == 32768 * 2 * 152 * 32     # the bounded grid
    r = np.zeros(4, np.int64)
    for f, name in ((lib.fcs_fmd_locate, "fcs_fmd_locate"), (lib.fcs_fmd_locate_dev, "fcs_fmd_locate_dev")):
        extra = (None,) if name.endswith("_dev") else ()
        assert f(None, r.ctypes.data, 4, 0, r.ctypes.data, r.ctypes.data, *extra) == fcship.FCS_ERR_INVALID
        assert f"[E::{name}]" in last_error() and "null index handle" in last_error()
        assert f(None, r.ctypes.data, -1, 0, r.ctypes.data, r.ctypes.data, *extra) == fcship.FCS_ERR_INVALID
        assert f(None, None, 4, 0, r.ctypes.data, r.ctypes.data, *extra) == fcship.FCS_ERR_INVALID
        assert "bad arguments" in last_error()


NO_DEVICE = """
import ctypes as C, sys
import numpy as np
lib = C.CDLL(sys.argv[1])
lib.fcs_last_error.restype = C.c_char_p
n_rows = 100
occ = np.zeros(8 * ((n_rows + 63) // 64 + 1), np.uint64)
Carr = np.array([0, 1, 30, 50, 70, 99], np.int64)
sa = np.zeros((n_rows + 3) // 4, np.uint64)
rows, ssa = np.array([3, 9], np.int64), np.array([5, 6], np.int64)
h = C.c_void_p()
vp = lambda a: C.c_void_p(a.ctypes.data)
rc = lib.fcs_fmd_index_create(0, vp(occ), C.c_int64(len(occ)), vp(Carr), C.c_int64(n_rows), vp(sa), C.c_int64(len(sa)), 4,
                              vp(rows), vp(ssa), C.c_int64(2), C.c_int64(49), C.byref(h))
print(lib.fcs_device_count(), rc, h.value, lib.fcs_last_error().decode())
"""


def test_without_a_device_the_index_cannot_be_made():
    """A process that sees no device (its own, so that the devices of a GPU
    box can be hidden from it): well-formed arguments get FCS_ERR_DEVICE and
    no handle."""
    import sys
    env = {**os.environ, "ROCR_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": ""}
    r = subprocess.run([sys.executable, "-c", NO_DEVICE, fcship.LIB_PATH], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    count, rc, handle, msg = r.stdout.strip().split(" ", 3)
    assert (int(count), int(rc), handle) == (0, fcship.FCS_ERR_DEVICE, "None"), r.stdout
    assert "no HIP device" in msg


def test_mock_align_with_the_key_on_seeds_on_the_host(tmp_path):
    """`fcs-genome align` against the CPU mock of libfcship, which has no
    fcs_fmd_* entry points: with bwa.gpu_seed=true the aligner finds none at
    run time, says so once and seeds on the host; the BAM and its index are
    those of a run with the key off."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpu_mock")], check=True, capture_output=True)
    mock = os.path.join(ROOT, "tests", "cpu_mock", "build")
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(mock, "libfcship.so")], capture_output=True, text=True)
    assert "fcs_bsw_extend" in nm.stdout and "fcs_fmd_" not in nm.stdout
    d = tmp_path / "pe"
    env = {"LD_LIBRARY_PATH": mock, "FCS_GPU_DEVICES": "0", "FCS_BWA_CHUNK_SIZE": "400"}
    p = H.run_cli("synth", "-o", d, "-c", "chr1:60000,chr2:30000", "-x", "3", "--paired", "350", "--seed", "5", env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    out = {}
    for key in ("true", "false"):
        o = tmp_path / f"{key}.bam"
        p = H.run_cli("align", "-r", d / "ref.fasta", "-1", d / "sample_1.fastq", "-2", d / "sample_2.fastq", "-o", o,
                      env={**env, "FCS_BWA_GPU_SEED": key}, cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-3000:]
        said = p.stderr.count("bwa.gpu_seed: the loaded libfcship has no fcs_fmd_* entry points")
        assert said == (1 if key == "true" else 0), p.stderr[-3000:]
        assert "GPU seeding (bwa.gpu_seed)" not in p.stderr
        assert re.search(r"alignment thread-seconds [\d.]+: seeding [\d.]+, extension [\d.]+, pairing [\d.]+", p.stderr)
        out[key] = (open(o, "rb").read(), open(str(o) + ".bai", "rb").read())
    assert len(out["true"][0]) > 10000 and out["true"] == out["false"]
