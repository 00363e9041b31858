"""GPU: BGZF member compression (fcs_bgzf_deflate / _try / _dev, SURVEY.md §8
row f3, the writing side) over the shapes of bgzf_deflate_cases: every member
is walked by fcs_bgzf_index, inflated by zlib and by the library's own GPU
inflate kernel, checked for CRC-32, ISIZE, BSIZE and its size limits, and is
the same bytes whatever batch it is compressed in."""
import ctypes as C
import threading

import numpy as np
import pytest

import bgzf_cases
import bgzf_deflate_cases as D
import fcship

pytestmark = pytest.mark.gpu


def members(blob: bytes, coff):
    return [blob[coff[k]:coff[k + 1]] for k in range(len(coff) - 1)]


@pytest.fixture(scope="module")
def alone(gpu):
    """{block bytes: its member compressed in a call of its own}, filled on demand."""
    memo = {}

    def get(block: bytes) -> bytes:
        if block not in memo:
            memo[block] = fcship.bgzf_deflate(block, len(block), device=gpu)[0]
        return memo[block]
    return get


@pytest.mark.parametrize("bb", D.BLOCK_BYTES)
def test_every_length_one_by_one(gpu, bb):
    for label, data, cbb in D.cases():
        if cbb != bb:
            continue
        blob, coff = fcship.bgzf_deflate(data, bb, device=gpu)
        want = D.blocks(data, bb)
        assert len(coff) == len(want) + 1 and coff[0] == 0 and coff[-1] == len(blob), label
        icoff, iuoff, used = fcship.bgzf_index(blob)
        assert used == len(blob) and list(icoff) == list(coff), label
        assert list(np.diff(iuoff)) == [len(b) for b in want], label
        for m, block in zip(members(blob, coff), want):
            D.check_member(label, m, block)
        # the library's own inflate kernel reads the new kernel's output
        assert fcship.bgzf_inflate(blob, device=gpu)[0] == data, label
        # the same bytes again, and with the EOF member behind them
        again, coff2 = fcship.bgzf_deflate(data, bb, eof=True, device=gpu)
        assert again == blob + bgzf_cases.EOF_MEMBER and list(coff2) == list(coff), label


@pytest.mark.parametrize("bb", D.BLOCK_BYTES)
def test_concatenated_batch_equals_members_alone(gpu, alone, bb):
    """All the cases of one block size as one call: every member is the member
    its block gives alone (its bytes depend on the block's bytes only)."""
    data = b"".join(d for _, d, cbb in D.cases() if cbb == bb)
    if bb == 1:
        data = data[:300]
    blob, coff = fcship.bgzf_deflate(data, bb, device=gpu)
    want = D.blocks(data, bb)
    got = members(blob, coff)
    assert len(got) == len(want)
    for k, (m, block) in enumerate(zip(got, want)):
        assert m == alone(block), (bb, k)
    assert fcship.bgzf_inflate(blob, device=gpu)[0] == data
    assert fcship.bgzf_deflate(data, bb, device=gpu)[0] == blob


def test_bad_arguments(gpu):
    data = np.frombuffer(D.text(5000), np.uint8).copy()
    out = np.full(65536 + 28, 0xAA, np.uint8)
    got, n = C.c_int64(), C.c_int32()
    f = fcship.lib.fcs_bgzf_deflate
    for nb, bb, cap in ((5000, 0, len(out)), (5000, 0xff01, len(out)), (-1, 4096, len(out)), (5000, 4096, 100)):
        rc = f(data.ctypes.data, nb, bb, 0, out.ctypes.data, cap, C.byref(got), None, C.byref(n), gpu)
        assert rc == fcship.FCS_ERR_INVALID and b"[E::fcs_bgzf_deflate]" in fcship.lib.fcs_last_error(), (nb, bb, cap)
        assert (out == 0xAA).all()
    # the EOF member counts towards the capacity
    blob, _ = fcship.bgzf_deflate(data, 4096, device=gpu)
    rc = f(data.ctypes.data, 5000, 4096, 1, out.ctypes.data, len(blob) + 27, C.byref(got), None, C.byref(n), gpu)
    assert rc == fcship.FCS_ERR_INVALID and (out == 0xAA).all()
    rc = f(data.ctypes.data, 5000, 4096, 1, out.ctypes.data, len(blob) + 28, C.byref(got), None, C.byref(n), gpu)
    assert rc == fcship.FCS_OK and n.value == 2 and out[:got.value].tobytes() == blob + bgzf_cases.EOF_MEMBER


def test_dev_entry_point_on_a_caller_stream(gpu):
    import torch
    data = b"".join(d for _, d in D.kinds())
    bb = 4096
    blob, coff = fcship.bgzf_deflate(data, bb, device=gpu)
    want = members(blob, coff)
    dev = torch.device("cuda", gpu)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        d = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
        slots = torch.zeros(len(want) * 65536, dtype=torch.uint8, device=dev)
        clen = torch.full((len(want),), -7, dtype=torch.int32, device=dev)
        fcship.check(fcship.lib.fcs_bgzf_deflate_dev(d.data_ptr(), len(data), bb, slots.data_ptr(), clen.data_ptr(), gpu,
                                                     C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    sizes = clen.cpu().numpy()
    s = slots.cpu().numpy()
    assert list(sizes) == [len(m) for m in want]
    for k, m in enumerate(want):
        assert s[k * 65536:k * 65536 + len(m)].tobytes() == m, k


def test_try_answers_busy_without_a_warm_session(gpu):
    """A call no warm session's arenas hold: FCS_BGZF_BUSY, nothing written;
    after the warm-up the same entry point compresses."""
    big = np.zeros(200 << 20, np.uint8)
    cap = fcship.lib.fcs_bgzf_deflate_bound(len(big), 0xff00, 0)
    out = np.zeros(cap, np.uint8)
    got, n = C.c_int64(-5), C.c_int32(-5)
    f = fcship.lib.fcs_bgzf_deflate_try
    rc = f(big.ctypes.data, len(big), 0xff00, 0, out.ctypes.data, cap, C.byref(got), None, C.byref(n), gpu)
    assert rc == fcship.FCS_BGZF_BUSY and got.value == 0 and n.value == 0
    assert not out[:1 << 20].any()
    data = np.frombuffer(D.text(3 * 0xff00 + 7), np.uint8).copy()
    fcship.check(fcship.lib.fcs_bgzf_warmup(gpu, 1, 8 << 20))
    rc = f(data.ctypes.data, len(data), 0xff00, 0, out.ctypes.data, cap, C.byref(got), None, C.byref(n), gpu)
    assert rc == fcship.FCS_OK and n.value == 4
    assert out[:got.value].tobytes() == fcship.bgzf_deflate(data, device=gpu)[0]


def test_concurrent_deflate_calls(gpu):
    """Four host threads compress different buffers at once, several calls
    each: every call gives what the buffer gives alone."""
    bufs = [b"".join(bgzf_cases.payload(np.random.default_rng(500 + 10 * k + j), kind, 40000 + 977 * k)
                     for j, kind in enumerate(D.KINDS)) for k in range(4)]
    want = [fcship.bgzf_deflate(b, device=gpu)[0] for b in bufs]
    errors = []

    def worker(k):
        try:
            for _ in range(6):
                got, _ = fcship.bgzf_deflate(np.frombuffer(bufs[k], np.uint8).copy(), device=gpu)
                if got != want[k]:
                    errors.append(f"thread {k}: output differs from the call alone")
        except Exception as e:  # noqa: BLE001 (reported below, with the thread)
            errors.append(f"thread {k}: {e}")
    th = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[:4]
    for b, w in zip(bufs, want):
        assert fcship.bgzf_inflate(w, device=gpu)[0] == b


# ------------------------------------------------------------------ end to end
HOST_ENV = {"FCS_GATK_NCONTIGS": "6", "FCS_GATK_NPROCS": "3", "FCS_GPU_DEVICES": "0", "FCS_BGZF_TRACE": "1"}


def reg2bins(beg, end):
    """SAM spec §5.3: the bins a [beg, end) region may overlap."""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


def tabix_query(gz, chrom, beg, end):
    """The records of gz overlapping chrom:[beg, end) (0-based), found through
    gz.tbi: candidate chunks by bin, lines read from their virtual offsets."""
    import bisect
    import gzip
    import host_lib as H
    names, refs = H.parse_index(gzip.decompress(open(str(gz) + ".tbi", "rb").read()), b"TBI\x01")
    bins, _ = refs[names.index(chrom)]
    lines = {v: ln for v, ln in H.bgzf_text_with_voffsets(gz)}
    voffs = sorted(lines)
    out = []
    for b in reg2bins(beg, end):
        for c0, c1 in bins.get(b, []):
            for v in voffs[bisect.bisect_left(voffs, c0):bisect.bisect_left(voffs, c1)]:
                f = lines[v].split("\t")
                if f[0] != chrom or lines[v].startswith("#"):
                    continue
                pos = int(f[1]) - 1
                e = pos + len(f[3])
                for kv in f[7].split(";"):
                    if kv.startswith("END="):
                        e = int(kv[4:])
                if pos < end and e > beg:
                    out.append((v, lines[v]))
    return [ln for _, ln in sorted(set(out))]


def device_batches(stderr: str):
    import re
    return [(int(a), int(b)) for a, b in re.findall(r"\[bgzf_writer\] device \d+: (\d+) batches on the GPU, (\d+) on", stderr)]


def test_htc_writes_the_same_vcf_gz_through_the_device(gpu, tmp_path):
    """`fcs-genome htc` with gpu.bgzf_deflate on and off: the same text in the
    .vcf.gz, both ending in the EOF member, blocks cut at the same places, and
    each file's own .tbi answering a region query with the same records."""
    import gzip
    import host_lib as H
    d = tmp_path / "in"
    p = H.run_cli("synth", "-o", d, "-c", "chr20:250000,chr21:100000", "-x", "30", "--seed", "11", "--no-fastq")
    assert p.returncode == 0, p.stderr
    gz = {}
    for key in ("true", "false"):
        out = tmp_path / f"{key}.g.vcf"
        p = H.run_cli("htc", "-r", d / "ref.fasta", "-i", d / "sample.bam", "-o", out,
                      env=dict(HOST_ENV, FCS_GPU_BGZF_DEFLATE=key), cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-3000:]
        gz[key] = tmp_path / f"{key}.g.vcf.gz"
        got = device_batches(p.stderr)
        if key == "true":
            assert got and got[0][0] >= 1, p.stderr[-2000:]  # the tail's blocks went through the kernel
        else:
            assert not got
    raw = {k: v.read_bytes() for k, v in gz.items()}
    assert raw["true"].endswith(bgzf_cases.EOF_MEMBER) and raw["false"].endswith(bgzf_cases.EOF_MEMBER)
    assert raw["true"] != raw["false"]
    text = gzip.decompress(raw["true"])
    assert text == gzip.decompress(raw["false"]) == (tmp_path / "true.g.vcf").read_bytes()
    assert [b[2] for b in H.bgzf_blocks(gz["true"])] == [b[2] for b in H.bgzf_blocks(gz["false"])]
    assert fcship.bgzf_inflate(raw["true"], device=gpu)[0] == text
    for chrom, beg, end in (("chr20", 100000, 140000), ("chr21", 0, 20000), ("chr20", 249000, 250000)):
        a = tabix_query(gz["true"], chrom, beg, end)
        assert a and a == tabix_query(gz["false"], chrom, beg, end), (chrom, beg, end)


def test_align_writes_the_same_bam_through_the_device(gpu, tmp_path):
    import gzip
    import host_lib as H
    d = tmp_path / "in"
    p = H.run_cli("synth", "-o", d, "-c", "chr1:120000", "-x", "8", "--seed", "23")
    assert p.returncode == 0, p.stderr
    bam = {}
    for key in ("true", "false"):
        out = tmp_path / f"{key}.bam"
        p = H.run_cli("align", "-r", d / "ref.fasta", "-1", d / "sample.fastq", "-o", out,
                      env=dict(HOST_ENV, FCS_GPU_BGZF_DEFLATE=key), cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-3000:]
        bam[key] = out.read_bytes()
        got = device_batches(p.stderr)
        assert (got and got[0][0] >= 1) if key == "true" else not got, p.stderr[-2000:]
    assert bam["true"].endswith(bgzf_cases.EOF_MEMBER)
    assert bam["true"] != bam["false"]
    assert gzip.decompress(bam["true"]) == gzip.decompress(bam["false"])
    assert (tmp_path / "true.bam.bai").exists()
