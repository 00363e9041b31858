"""Minimizer seeding and chaining on the host (falcon-genome_amd/host/minimizer.h,
DESIGN §2 [EXT] "minimizer seeding and chaining"): the sketch, the anchors, the
recurrence's host statement and the backtrack against the restatement of
tests/mm_cases.py; the shared rules under the sanitizers (tools/micro/mm_test.cpp,
its own program: nothing loaded into Python is sanitized); and `fcs-genome align`
with bwa.seeder=minimizer on the CPU mock.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import align_cases as A
import fcship
import host_lib as H
import mm_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M.host_hooks(H.lib)


# ------------------------------------------------------------------ sketch
HAND = [
    "ACGTTGCATGCCGATAGCTAGCTAGGATCGATCGGCTAGCATCGACTAGCATCAGCATCGACTACGACTAGCA",
    "ACGT" * 30,                      # a repeat: equal minima in every window
    "A" * 80,                         # one k-mer everywhere
    "ACGTTGCATGCCGATAGCTAGCTAGGATCGATCGGNCTAGCATCGACTAGCATCAGCATCGACTACGACTAGCAGGATTTACGA",
    "ACG",                            # shorter than k
    "",
]


@pytest.mark.parametrize("k,w", [(21, 11), (15, 10), (6, 4), (4, 3), (5, 1)])
def test_sketch_equals_the_restatement(k, w):
    rng = np.random.default_rng(100 * k + w)
    seqs = HAND + [M.random_dna(int(n), rng) for n in rng.integers(40, 400, 6)]
    seqs += ["".join(rng.choice(list("AT"), 120)), "".join(rng.choice(list("ACGTN"), 200, p=[.24, .24, .24, .24, .04]))]
    total = 0
    for s in seqs:
        got, want = M.host_sketch(H, s, k, w), M.sketch(s, k, w)
        assert got == want, (s, got[:5], want[:5])
        total += len(got)
    assert total > 50


def test_every_window_of_w_kmers_holds_a_minimizer():
    rng = np.random.default_rng(5)
    s = M.random_dna(600, rng)
    pos = [p for _, p, _ in M.host_sketch(H, s)]
    assert pos == sorted(set(pos))
    for e in range(M.K - 1 + M.W - 1, len(s)):
        assert any(e - M.W + 1 <= p <= e for p in pos), e


def test_reverse_complement_selects_mirrored_positions():
    rng = np.random.default_rng(6)
    for n in (200, 333):
        s = M.random_dna(n, rng)
        fw, rv = M.host_sketch(H, s), M.host_sketch(H, M.revcomp(s))
        # a k-mer whose last base is i is, on the other strand, the one whose last base is n - 1 - (i - k + 1)
        mirrored = sorted((h, n - 1 - (p - M.K + 1), 1 - st) for h, p, st in rv)
        assert sorted(fw) == mirrored


def test_non_acgt_base_restarts_the_kmer():
    rng = np.random.default_rng(7)
    a, b = M.random_dna(120, rng), M.random_dna(90, rng)
    got = M.host_sketch(H, a + "N" + b)
    left, right = M.host_sketch(H, a), M.host_sketch(H, b)
    assert got == left + [(h, p + len(a) + 1, st) for h, p, st in right]
    # no k-mer over the N, and none selected by a window that reaches over it
    assert not any(len(a) <= p < len(a) + M.K for _, p, _ in got)
    # too little on one side for a window: nothing from it
    assert M.host_sketch(H, a + "N" + b[:M.K + M.W - 2]) == left


def test_palindromic_kmer_is_skipped():
    # k = 4: ACGT, AATT, GATC ... are their own reverse complements
    s = "ACGTACGTAATTGGCCGATCTTAAGCGC" * 3
    km = M.kmers(s, 4)
    pal = {i for i, v in enumerate(km) if v == "skip"}
    assert len(pal) > 10
    got = M.host_sketch(H, s, 4, 3)
    assert got == M.sketch(s, 4, 3) and got
    assert not pal & {p for _, p, _ in got}
    # nothing but palindromes: no minimizer at all
    assert M.host_sketch(H, "GC" * 20, 4, 3) == [] and M.host_sketch(H, "AT" * 20, 4, 2) == []


# ------------------------------------------------------------------ anchors
def test_anchors_equal_the_restatement_and_match_exactly():
    rng = np.random.default_rng(8)
    contigs = [M.random_dna(3000, rng), M.random_dna(1500, rng)]
    contigs[1] = contigs[1][:500] + contigs[0][700:1300] + contigs[1][1100:]   # a repeat across contigs
    idx = M.index(contigs)
    seen_rev = seen_rep = 0
    for r in range(12):
        c = r % 2 if r < 8 else 0
        at = int(rng.integers(0, len(contigs[c]) - 160)) if r < 8 else 800 + 10 * r   # the last four inside the repeat
        read = contigs[c][at:at + 150]
        if r % 3 == 0:
            read = M.revcomp(read)
        max_occ = 1 if r >= 8 else 500
        t, q, frac = M.host_anchors(H, contigs, read, max_occ=max_occ)
        wt, wq, (rep, L) = M.anchors(idx, read, max_occ=max_occ)
        assert list(t) == wt and list(q) == wq
        assert frac == pytest.approx(rep / L, abs=1e-12)
        seen_rep += rep > 0
        for ti, qi in zip(wt, wq):
            rev, pos, cg = (ti >> 32) & 1, ti & 0xFFFFFFFF, ti >> 33
            o = M.revcomp(read) if rev else read
            assert o[qi - M.K + 1:qi + 1] == contigs[cg][pos - M.K + 1:pos + 1]
            seen_rev += rev
    assert seen_rev > 0 and seen_rep > 0


# ------------------------------------------------------------------ recurrence and backtrack
def both_chain(reads, **kw):
    t, q, off = M.flat(reads)
    got = fcship.mm_chain((t, q, off), entry=M.host_chain_entry(H), **kw)
    want = M.chain_batch(t, q, off, **{k: v for k, v in kw.items() if k in ("max_gap", "bw", "span")})
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return got, off


def test_chain_host_and_backtrack_equal_the_restatement():
    rng = np.random.default_rng(9)
    reads = [M.colinear_read(int(n), rng) for n in (0, 1, 2, 63, 64, 65, 128, 129, 200)]
    reads += [M.random_read(int(n), rng) for n in (5, 40, 150, 300)]
    (f, p), off = both_chain(reads)
    assert (p >= 0).sum() > 500
    kept = 0
    for r in range(len(reads)):
        fr, pr = f[off[r]:off[r + 1]], p[off[r]:off[r + 1]]
        for mc, ms in ((2, 20), (1, 0), (3, 40)):
            got = M.host_backtrack(H, fr, pr, mc, ms)
            assert got == M.backtrack([int(x) for x in fr], [int(x) for x in pr], mc, ms)
            kept += len(got)
    assert kept > 20
    both_chain(reads, max_gap=40, bw=3, span=15)


def test_chain_host_refuses_what_the_rules_refuse():
    t, q, off = M.flat([([10, 30, 20], [1, 3, 2])])
    with pytest.raises(RuntimeError, match="not sorted"):
        fcship.mm_chain((t, q, off), entry=M.host_chain_entry(H))
    with pytest.raises(RuntimeError, match="bad offsets"):
        fcship.mm_chain((np.array([10, 20]), np.array([1, 2]), np.array([0, 3])), entry=M.host_chain_entry(H))
    with pytest.raises(RuntimeError, match="predecessor"):
        M.host_backtrack(H, [21, 30], [-1, 1])


# ------------------------------------------------------------------ mm_rules.h and minimizer.cpp under sanitizers
@pytest.fixture(scope="module")
def mm_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("mm") / "mm_test"
    pkg = os.path.join(ROOT, "falcon-genome_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"), "-I" + os.path.join(pkg, "host"),
                    os.path.join(ROOT, "tools", "micro", "mm_test.cpp"), os.path.join(pkg, "host", "minimizer.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def test_shared_rules_and_the_kernel_s_protocol_in_a_host_build(mm_exe):
    r = subprocess.run([str(mm_exe), "1", "150"], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "MISMATCH" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    fig = dict(zip(r.stdout.split()[0::2], r.stdout.split()[1::2]))
    assert int(fig["minimizers"]) > 1000 and int(fig["anchors"]) > 3000 and int(fig["chained"]) > 2000 and int(fig["chains"]) > 150


def test_abi_symbols_and_constants():
    assert fcship.mm_header_functions() == ["fcsmm_chain", "fcsmm_chain_dev", "fcsmm_workspace_bytes"]
    hdr = open(fcship.MM_HEADER_PATH).read()
    for name in ("LOOKBACK", "SPAN_MAX", "GAP_MAX", "READ_ANCHORS", "STATUS_FIELD", "STATUS_ORDER"):
        assert int(re.search(rf"#define FCSMM_{name} (\d+)", hdr).group(1)) == getattr(fcship, "FCSMM_" + name)
    assert M.LOOKBACK == fcship.FCSMM_LOOKBACK


# ------------------------------------------------------------------ align with bwa.seeder=minimizer on the CPU mock
@pytest.fixture(scope="module")
def mock_env():
    subprocess.run(["make", "-C", f"{ROOT}/tests/cpu_mock"], check=True, capture_output=True)
    return {"LD_LIBRARY_PATH": f"{ROOT}/tests/cpu_mock/build", "FCS_GPU_DEVICES": "0"}


@pytest.fixture(scope="module")
def pe(tmp_path_factory, mock_env):
    """The inputs of test_align_host_cpu.py's paired-end case."""
    d = tmp_path_factory.mktemp("mm_pe") / "pe"
    p = H.run_cli("synth", "-o", d, "-c", "chr1:150000", "-x", "6", "--paired", "350", "--seed", "77")
    assert p.returncode == 0, p.stderr[-2000:]
    return d, A.damage_mates(d / "sample_2.fastq")


def test_paired_end_with_the_minimizer_seeder(mock_env, pe, tmp_path):
    d, damaged = pe
    out = tmp_path / "pe.bam"
    p = H.run_cli("align", "-r", d / "ref.fasta", "-1", d / "sample_1.fastq", "-2", d / "sample_2.fastq", "-o", out,
                  "--chains-out", tmp_path / "chains.txt", env=dict(mock_env, FCS_BWA_SEEDER="minimizer"), cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    A.check_pairs(p.stderr, out, d / "pairs_truth.tsv", damaged)
    assert re.search(r"minimizer seeding \(bwa\.seeder\): \d+ anchors, \d+ chains kept, chaining \S+ s \(host\)", p.stderr)
    assert "minimizer index" in p.stderr and "FMD index" not in p.stderr   # the FMD-index is neither built nor loaded
    # --chains-out: every read in input order, mates together; f and p are the restatement's for its anchors
    txt = open(tmp_path / "chains.txt").read().split("\n")
    heads = [ln for ln in txt if ln.startswith("read ")]
    n_pairs = sum(1 for _ in open(d / "sample_1.fastq")) // 4
    assert [h.split()[1] for h in heads] == [f"{i}/{m}" for i in range(n_pairs) for m in (1, 2)]
    k = txt.index(heads[0])
    n = int(heads[0].split()[3])
    f, pp = [int(x) for x in txt[k + 1].split()[1:]], [int(x) for x in txt[k + 2].split()[1:]]
    assert len(f) == len(pp) == n > 2 and txt[k + 3].startswith("chain ")
    ref = "".join(ln.strip() for ln in open(d / "ref.fasta") if not ln.startswith(">"))
    read = open(d / "sample_1.fastq").read().split("\n")[1]
    wt, wq, _ = M.anchors(M.index([ref]), read)
    assert (f, pp) == M.chain(wt, wq)
    chains = M.backtrack(f, pp)
    assert txt[k + 3].split() == ["chain", str(chains[0][0]), str(len(chains[0][1]))] + [str(a) for a in chains[0][1]]


def test_single_end_whole_and_split_reads_with_the_minimizer_seeder(mock_env, tmp_path):
    d = tmp_path / "ref"
    p = H.run_cli("synth", "-o", d, "-c", "chr20:150000,chr21:60000", "-x", "1", "--seed", "11", "--no-fastq")
    assert p.returncode == 0, p.stderr[-2000:]
    fq = tmp_path / "split.fastq"
    truth = A.split_reads_fastq(d / "ref.fasta", fq, n_split=120, n_whole=60, seed=3)
    out = tmp_path / "split.bam"
    p = H.run_cli("align", "-r", d / "ref.fasta", "-1", fq, "-o", out, env=dict(mock_env, FCS_BWA_SEEDER="minimizer"), cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    # whole reads: the same module's position check; split reads: only that the run reports its supplementary count
    whole = {name: t for name, t in truth.items() if len(t) != 4}
    assert len(whole) == 60
    good, bad = A.check_split_reads(out, whole)
    assert not bad, bad[:5]
    n_supp = int(re.search(r"(\d+) supplementary", p.stderr).group(1))
    print(f"supplementary records with the minimizer seeder: {n_supp} of 120 split reads")


def test_default_seeder_writes_the_bytes_of_smem(mock_env, pe, tmp_path):
    d, _ = pe
    outs = []
    for name, env in (("default", mock_env), ("smem", dict(mock_env, FCS_BWA_SEEDER="smem"))):
        out = tmp_path / f"{name}.bam"
        p = H.run_cli("align", "-r", d / "ref.fasta", "-1", d / "sample_1.fastq", "-2", d / "sample_2.fastq", "-o", out, env=env, cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-3000:]
        assert "FMD index" in p.stderr and "minimizer" not in p.stderr
        outs.append(out)
    assert open(outs[0], "rb").read() == open(outs[1], "rb").read()
    assert open(str(outs[0]) + ".bai", "rb").read() == open(str(outs[1]) + ".bai", "rb").read()
    p = H.run_cli("align", "-r", d / "ref.fasta", "-1", d / "sample_1.fastq", "-o", tmp_path / "x.bam", env=dict(mock_env, FCS_BWA_SEEDER="kmer"),
                  cwd=tmp_path)
    assert p.returncode != 0 and "smem or minimizer" in p.stderr
    p = H.run_cli("align", "-r", d / "ref.fasta", "-1", d / "sample_1.fastq", "-o", tmp_path / "y.bam", "--chains-out", tmp_path / "c.txt",
                  env=mock_env, cwd=tmp_path)
    assert p.returncode != 0 and "--chains-out needs the minimizer seeder" in p.stderr
