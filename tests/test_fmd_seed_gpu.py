"""FMD-index seeding on the GPU:
fmd_collect_kernel and fmd_locate_kernel (falcon-genome_amd/csrc/fmd_seed.hip)
against the host index.  fcsg_fmd_seed_batch(gpu=1), the aligner's device path
(host/gpu_seed.cpp over fcs_fmd_collect / fcs_fmd_locate), must return every
integer fcsg_fmd_seed_batch(gpu=0) (FmdIndex::collect / locate, pinned to a
brute-force definition by test_fmindex.py) returns: the sorted SMEMs {qb, qe,
s, k, l} and the located {contig, offset, strand} of the sampled occurrences.
The batches are those of fmd_seed_cases.py, which test_fmd_seed_cpu.py runs
through the host build of the same per-read code."""
import re
import threading

import numpy as np
import pytest

import fcship
import fmd_seed_cases as S
import host_lib as H

pytestmark = pytest.mark.gpu

ENV = {"FCS_GPU_DEVICES": "0"}


@pytest.fixture(scope="module")
def host_plain():
    """The host's answer for the plain batch at each parameter set, computed once."""
    return {P: S.seed_batch(S.plain_ref(), S.plain_batch(), 0, P) for P in S.PARAM_SETS}


def prefix(result, n):
    return result[0][:n], result[1][:n], result[2]


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, len(S.plain_batch())])
def test_plain_batch_sizes(gpu, host_plain, n):
    """1, 15, 16, 17 reads (a wave holds 16 quads), 63, 64, 65 (a block holds
    64) and the whole batch (several blocks), bwa's parameters: equal, and no
    read left to the host at the default max_mems."""
    got = S.seed_batch(S.plain_ref(), S.plain_batch()[:n], 1, S.BWA)
    S.assert_same(got, prefix(host_plain[S.BWA], n))
    assert got[2] == 0


@pytest.mark.parametrize("P", S.PARAM_SETS[1:], ids=["min_len1", "no_reseed", "no_third_round"])
def test_plain_batch_parameters(gpu, host_plain, P):
    """min_len 1 (every SMEM is kept: up to 114 per read), split_len 10^9 (no
    second round), max_mem_intv 0 (no third round)."""
    got = S.seed_batch(S.plain_ref(), S.plain_batch(), 1, P)
    S.assert_same(got, host_plain[P])
    assert got[2] == 0


def test_low_complexity_stacks(gpu):
    """A 100-base homopolymer and a 120-base ACG tandem: interval stacks 100
    deep and runs of equal-size intervals.  With room for the 2,700 SMEMs the
    re-seeding of the poly-A read gives, no read goes back to the host, so no
    read was dropped for stack depth; at the default max_mems the reads with
    more than 128 SMEMs (the two homopolymer and the two tandem reads), and
    only they, are the host's."""
    want = S.seed_batch(S.low_ref(), S.low_batch(), 0)
    counts = [len(m) for m in want[0]]
    assert max(counts) > 2000
    got = S.seed_batch(S.low_ref(), S.low_batch(), 1, max_mems=4096)
    S.assert_same(got, want)
    assert got[2] == 0
    got = S.seed_batch(S.low_ref(), S.low_batch(), 1)
    S.assert_same(got, want)
    assert got[2] == sum(c > S.MAX_MEMS_DEFAULT for c in counts)


def test_forced_overflow_goes_to_the_host(gpu, host_plain):
    want = host_plain[S.BWA]
    got = S.seed_batch(S.plain_ref(), S.plain_batch(), 1, S.BWA, max_mems=2)
    S.assert_same(got, want)
    over = sum(len(m) > 2 for m in want[0])
    assert 0 < over < len(want[0]) and got[2] == over


@pytest.mark.parametrize("sa_intv,saved", [(1, False), (4, True), (7, False), (32, True)])
def test_locate_sampled_suffix_array(gpu, tmp_path, sa_intv, saved):
    """sa_intv 1 (the wrapper reads the suffix array on the host), 4 and 32
    from a saved and mapped index, 7 built in memory; min_len 5 gives SMEMs
    with tens of occurrences, and max_occ 3 samples those with more (s >
    max_occ: rows k, k + step, ..).  The batch has reads that start at a contig
    start (their rows walk to a special row)."""
    path = tmp_path / "x.fcsidx" if saved else ""
    P = (5, 28, 10, 20)
    reads = S.plain_batch()[:120]
    want = S.seed_batch(S.plain_ref(), reads, 0, P, max_occ=3, sa_intv=1)
    assert any((m[:, 2] > 3).any() for m in want[0] if len(m))
    got = S.seed_batch(S.plain_ref(), reads, 1, P, max_occ=3, sa_intv=sa_intv, index_path=path)
    S.assert_same(got, want)
    assert got[2] == 0
    want = S.seed_batch(S.plain_ref(), reads, 0, S.BWA, sa_intv=1)
    got = S.seed_batch(S.plain_ref(), reads, 1, S.BWA, sa_intv=sa_intv, index_path=path)
    S.assert_same(got, want)


def test_locate_step_cap_and_bad_rows(gpu):
    """fcs_fmd_locate directly: every row of the index at sa_intv 32 against the
    full suffix array; with max_steps 3 the rows more than 3 LF steps from a
    stored row are flagged FCS_FMD_STEP_CAP (and only they), rows outside the
    index FCS_FMD_BAD_ROW."""
    contigs = S.plain_ref()
    occ, Carr, n_rows, sa1, rows1, ssa1, flen = S.index_arrays(contigs, 1)
    occ32, C32, n32, sa32, rows32, ssa32, _ = S.index_arrays(contigs, 32)
    assert n32 == n_rows and np.array_equal(occ, occ32)
    h = fcship.fmd_index_create(occ32, C32, n32, sa32, 32, rows32, ssa32, flen)
    try:
        rows = np.arange(n_rows, dtype=np.int64)
        pos, status = fcship.fmd_locate(h, rows)
        assert (status == fcship.FCS_FMD_LOCATED).all() and np.array_equal(pos, sa1.astype(np.int64))
        pos3, st3 = fcship.fmd_locate(h, rows, max_steps=3)
        ok = st3 == fcship.FCS_FMD_LOCATED
        assert np.array_equal(pos3[ok], sa1.astype(np.int64)[ok])
        assert set(st3[~ok]) == {fcship.FCS_FMD_STEP_CAP} and 0 < (~ok).sum() < n_rows
        # located are exactly the rows whose walk (text positions SA[row], SA[row] - 1, ..) meets a stored row within 3 steps
        stored = np.zeros(n_rows, bool)
        stored[::32] = True
        stored[rows32] = True
        sa = sa1.astype(np.int64)
        text_of = np.empty(n_rows, np.int64)
        text_of[sa] = rows
        near = np.zeros(n_rows, bool)
        for d in range(4):
            p = sa - d
            near |= (p >= 0) & stored[text_of[np.maximum(p, 0)]]
        assert np.array_equal(ok, near)
        _, bad = fcship.fmd_locate(h, np.array([-1, n_rows, 1 << 40], np.int64))
        assert list(bad) == [fcship.FCS_FMD_BAD_ROW] * 3
    finally:
        fcship.fmd_index_destroy(h)
    with pytest.raises(fcship.FcsError) as e:   # the handle is gone: refused, not followed
        fcship.fmd_locate(h, np.zeros(1, np.int64))
    assert e.value.code == fcship.FCS_ERR_INVALID


def test_four_threads_share_one_index(gpu, host_plain):
    """Four host threads, each with its own chunk and its own output buffers,
    on one device and one index handle (the aligner's bwa.gpu_slots threads):
    fcs_fmd_collect and fcs_fmd_locate through the ctypes binding, each
    chunk's result equal to the serial call's and to the host's SMEMs."""
    contigs, reads = S.plain_ref(), S.plain_batch()
    occ, Carr, n_rows, sa, rows, ssa, flen = S.index_arrays(contigs, 8)
    h = fcship.fmd_index_create(occ, Carr, n_rows, sa, 8, rows, ssa, flen)
    try:
        chunks = [reads[k::4] for k in range(4)]

        def work(chunk):
            mems, n_mems, overflow = fcship.fmd_collect(h, *S.soa(chunk))
            k = np.concatenate([mems[r, :n_mems[r]]["k"] for r in range(len(chunk))] + [np.zeros(0, np.int64)])
            pos, status = fcship.fmd_locate(h, k)
            return mems, n_mems, overflow, pos, status
        serial = [work(c) for c in chunks]
        for k, c in enumerate(chunks):   # the serial result is the host's
            want = host_plain[S.BWA][0][k::4]
            mems, n_mems, overflow = serial[k][:3]
            assert not overflow.any()
            for r in range(len(c)):
                m = mems[r, :n_mems[r]]
                assert np.array_equal(np.stack([m["qb"], m["qe"], m["s"], m["k"], m["l"]], 1).reshape(-1, 5), want[r])
        out, errors = [None] * 4, []

        def run(k):
            try:
                for _ in range(3):
                    out[k] = work(chunks[k])
            except Exception as e:  # noqa: BLE001
                errors.append(e)
        threads = [threading.Thread(target=run, args=(k,)) for k in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for k in range(4):
            for a, b in zip(out[k], serial[k]):
                assert np.array_equal(a, b)
    finally:
        fcship.fmd_index_destroy(h)


def align(tmp_path, name, key, ref, *fastqs):
    out = tmp_path / f"{name}_{key}.bam"
    args = ["align", "-r", ref, "-1", fastqs[0]] + (["-2", fastqs[1]] if len(fastqs) > 1 else []) + ["-o", out]
    p = H.run_cli(*args, env={**ENV, "FCS_BWA_GPU_SEED": key, "FCS_BWA_CHUNK_SIZE": "3000"}, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stderr, open(out, "rb").read(), open(str(out) + ".bai", "rb").read()


def test_align_is_byte_identical_with_the_key_on(gpu, tmp_path):
    """`fcs-genome align`, single reads on an index built in memory (full
    suffix array) and paired reads on a saved index with sa_intv 8 (device
    locate), several chunks each: the BAM and BAI with bwa.gpu_seed=true are
    those with the key off, and the log shows the device path with its
    fallback count."""
    d = tmp_path / "se"
    p = H.run_cli("synth", "-o", d, "-c", "chr20:150000,chr21:60000", "-x", "6", "--seed", "11", env=ENV, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    d2 = tmp_path / "pe"
    p = H.run_cli("synth", "-o", d2, "-c", "chr1:150000", "-x", "6", "--paired", "350", "--seed", "77", env=ENV,
                  cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    p = H.run_cli("index", "-r", d2 / "ref.fasta", "--sa-intv", "8", env=ENV, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    for name, ref, fq in (("se", d / "ref.fasta", [d / "sample.fastq"]),
                          ("pe", d2 / "ref.fasta", [d2 / "sample_1.fastq", d2 / "sample_2.fastq"])):
        log_on, bam_on, bai_on = align(tmp_path, name, "true", ref, *fq)
        log_off, bam_off, bai_off = align(tmp_path, name, "false", ref, *fq)
        assert len(bam_on) > 100000 and bam_on == bam_off and bai_on == bai_off, name
        m = re.search(r"GPU seeding \(bwa.gpu_seed\): (\d+) reads through the device, (\d+) of them collected on the "
                      r"host .*, (\d+) rows located on the host; seeding thread-seconds: collect ([\d.e-]+), locate "
                      r"([\d.e-]+), chain ([\d.e-]+)", log_on)
        assert m, log_on[-3000:]
        reads = int(re.search(r"(\d+) reads, ", log_on).group(1))
        assert int(m.group(1)) == reads and int(m.group(2)) <= reads // 100
        assert ("sa_intv 8" in log_on) == (name == "pe")
        assert "GPU seeding" not in log_off
        for log in (log_on, log_off):   # the line the benchmark parses is as it was
            assert re.search(r"alignment thread-seconds [\d.]+: seeding [\d.]+, extension [\d.]+, pairing [\d.]+, "
                             r"records [\d.]+", log)
