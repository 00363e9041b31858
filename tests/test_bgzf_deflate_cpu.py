"""BGZF deflate checks that need no GPU (the writing side).

- The device encoder's serial parts (falcon-genome_amd/csrc/bgzf_deflate.h:
  code lengths and their limit, canonical codes, the dynamic header, the
  choice of form, token packing), compiled for the host with ASan and UBSan
  (tools/micro/deflate_test.cpp, whose matcher is the kernel's scheme run
  serially): every shape of bgzf_deflate_cases inflates with zlib to its
  input, no code exceeds its length limit, every code sent is complete, and
  the size conditions of the GPU test hold for the same token streams.
- The new entry points are declared, exported and counted, and refuse bad
  arguments before they look for a device.
"""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bgzf_deflate_cases as D
import fcship

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def deflate_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("deflate") / "deflate_test"
    src = os.path.join(ROOT, "tools", "micro", "deflate_test.cpp")
    subprocess.run(["g++", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "falcon-genome_amd", "csrc"), src, "-o", str(exe), "-lz"], check=True)
    return exe


def run(exe, *args):
    return subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True,
                          env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})


def test_shared_encoder_host_build_random_blocks(deflate_exe):
    r = run(deflate_exe, 150)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "deflate: 0 problems in 150 blocks" in r.stdout


def test_shared_encoder_host_build_every_shape(deflate_exe, tmp_path):
    cases = D.cases()
    args = []
    for k, (_, data, bb) in enumerate(cases):
        f = tmp_path / f"in{k}.bin"
        f.write_bytes(data)
        args += [f, bb]
    out = tmp_path / "out.bin"
    r = run(deflate_exe, out, *args)
    want = sum(len(D.blocks(d, bb)) for _, d, bb in cases)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"deflate: 0 problems in {want} blocks" in r.stdout
    blob = out.read_bytes()
    at = 0
    for label, data, bb in cases:
        for block in D.blocks(data, bb):
            n, = struct.unpack_from("<I", blob, at)
            D.check_payload(label, blob[at + 4:at + 4 + n], block)
            at += 4 + n
    assert at == len(blob)


def test_deflate_symbols_declared_exported_and_counted():
    names = ["fcs_bgzf_deflate_bound", "fcs_bgzf_deflate", "fcs_bgzf_deflate_try", "fcs_bgzf_deflate_dev"]
    syms = fcship.header_symbols()
    assert all(n in syms for n in names)
    assert all(hasattr(fcship.lib, n) for n in names)
    assert fcship.lib.fcs_abi_symbol_count() == len(syms)
    assert "#define FCS_BGZF_BLOCK_MAX 0xff00" in open(fcship.HEADER_PATH).read()
    assert fcship.FCS_BGZF_BLOCK_MAX == 0xff00


def test_deflate_bound_and_arguments_without_a_device():
    bound = fcship.lib.fcs_bgzf_deflate_bound
    assert bound(0, 0xff00, 0) == 0 and bound(0, 0xff00, 1) == 28
    assert bound(1, 0xff00, 0) == 65536 and bound(0xff00 + 1, 0xff00, 1) == 2 * 65536 + 28
    assert bound(10, 1, 0) == 10 * 65536
    for n, bb in ((-1, 64), (5, 0), (5, 0xff01)):
        assert bound(n, bb, 0) == fcship.FCS_ERR_INVALID
        assert b"[E::fcs_bgzf_deflate_bound]" in fcship.lib.fcs_last_error()
    data = np.frombuffer(b"abc" * 100, np.uint8).copy()
    out = np.zeros(65536 + 28, np.uint8)
    got, n = C.c_int64(), C.c_int32()
    for f in (fcship.lib.fcs_bgzf_deflate, fcship.lib.fcs_bgzf_deflate_try):
        for nb, bb in ((-1, 64), (300, 0), (300, 0xff01)):
            rc = f(data.ctypes.data, nb, bb, 0, out.ctypes.data, len(out), C.byref(got), None, C.byref(n), 0)
            assert rc == fcship.FCS_ERR_INVALID and b"[E::fcs_bgzf_deflate]" in fcship.lib.fcs_last_error()
    assert fcship.lib.fcs_bgzf_deflate_dev(None, 300, 0, None, None, 0, None) == fcship.FCS_ERR_INVALID
    assert b"[E::fcs_bgzf_deflate_dev]" in fcship.lib.fcs_last_error()
    # no input: no member, only the EOF member when asked for (no device needed)
    assert fcship.bgzf_deflate(b"")[0] == b""
    blob, coff = fcship.bgzf_deflate(b"", eof=True)
    assert blob.hex() == "1f8b08040000000000ff0600424302001b0003000000000000000000" and list(coff) == [0]


def test_mock_htc_with_the_key_on_falls_back_to_the_host_codec(tmp_path):
    """`fcs-genome htc` against the CPU mock of libfcship, which has no deflate
    entry points: with gpu.bgzf_deflate=true the writer finds none at run time
    and stays on the host codec; the VCF.gz and its index are those of a run
    with the key off."""
    import gzip
    import host_lib as H
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpu_mock")], check=True, capture_output=True)
    mock = os.path.join(ROOT, "tests", "cpu_mock", "build")
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(mock, "libfcship.so")], capture_output=True, text=True)
    assert "fcs_bgzf_inflate_try" in nm.stdout and "fcs_bgzf_deflate" not in nm.stdout
    d = tmp_path / "in"
    p = H.run_cli("synth", "-o", d, "-c", "chrA:120000", "-x", "10", "--no-fastq", "--seed", "9")
    assert p.returncode == 0, p.stderr[-2000:]
    out = {}
    for key in ("true", "false"):
        o = tmp_path / f"{key}.g.vcf"
        e = {"LD_LIBRARY_PATH": mock, "FCS_GPU_DEVICES": "0", "FCS_MOCK_PHMM": "gkl", "FCS_BGZF_TRACE": "1",
             "FCS_LOG_DIR": str(tmp_path / f"log_{key}"), "FCS_GPU_BGZF_DEFLATE": key}
        p = H.run_cli("htc", "-f", "-r", d / "ref.fasta", "-i", d / "sample.bam", "-o", o, env=e, cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-3000:]
        assert "[bgzf_writer]" not in p.stderr  # no writer entered device mode
        out[key] = ((tmp_path / f"{key}.g.vcf.gz").read_bytes(), (tmp_path / f"{key}.g.vcf.gz.tbi").read_bytes())
    text = gzip.decompress(out["true"][0])
    assert len(text) > 100000 and text == gzip.decompress(out["false"][0]) == (tmp_path / "true.g.vcf").read_bytes()
    strip = lambda t: b"".join(ln for ln in t.splitlines(True) if not ln.startswith(b"##"))  # noqa: E731
    assert strip(text) == strip(gzip.decompress(out["false"][0]))
    assert out["true"][1] == out["false"][1]
    assert "gpu.bgzf_deflate" in open(os.path.join(ROOT, "falcon-genome_amd", "host", "config.cpp")).read()
