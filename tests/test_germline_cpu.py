"""`fcs-genome germline` on the CPU mock (tests/cpu_mock, its PairHMM by the
reference's CPU path): FASTQ to VCF in one run writes what `align` with
bwa.seeder=minimizer followed by `htc` writes; -v and -L reach the htc half; a
sample sheet yields one output per sample; the argument errors.
"""
import os
import subprocess

import pytest

import host_lib as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mock_env(tmp_path_factory):
    subprocess.run(["make", "-C", f"{ROOT}/tests/cpu_mock"], check=True, capture_output=True)
    return {"LD_LIBRARY_PATH": f"{ROOT}/tests/cpu_mock/build", "FCS_GPU_DEVICES": "0", "FCS_MOCK_PHMM": "gkl", "FCS_HOST_THREADS": "4",
            "FCS_LOG_DIR": str(tmp_path_factory.mktemp("log"))}


@pytest.fixture(scope="module")
def sample(tmp_path_factory, mock_env):
    d = tmp_path_factory.mktemp("germline") / "syn"
    p = H.run_cli("synth", "-o", d, "-c", "chr1:150000", "-x", "6", "--paired", "350", "--seed", "41")
    assert p.returncode == 0, p.stderr[-2000:]
    return d


def fastq(d):
    return ["-1", d / "sample_1.fastq", "-2", d / "sample_2.fastq"]


def body(path):
    return [ln for ln in open(path).read().split("\n") if ln and not ln.startswith("#")]


@pytest.fixture(scope="module")
def two_step(sample, mock_env, tmp_path_factory):
    """align with bwa.seeder=minimizer, then htc -v on its BAM."""
    o = tmp_path_factory.mktemp("two_step")
    p = H.run_cli("align", "-r", sample / "ref.fasta", *fastq(sample), "-o", o / "a.bam", env=dict(mock_env, FCS_BWA_SEEDER="minimizer"), cwd=o)
    assert p.returncode == 0, p.stderr[-3000:]
    p = H.run_cli("htc", "-r", sample / "ref.fasta", "-i", o / "a.bam", "-o", o / "h.vcf", "-v", env=mock_env, cwd=o)
    assert p.returncode == 0, p.stderr[-3000:]
    return o


def test_germline_writes_what_align_then_htc_write(sample, mock_env, two_step, tmp_path):
    out = tmp_path / "g.vcf"
    p = H.run_cli("germline", "-r", sample / "ref.fasta", *fastq(sample), "-o", out, "-b", "-v", env=mock_env, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    for ext in (".vcf", ".vcf.gz", ".vcf.gz.tbi", ".bam", ".bam.bai"):
        assert os.path.getsize(str(tmp_path / "g") + ext) > 0, ext
    assert open(out, "rb").read() == open(two_step / "h.vcf", "rb").read()
    assert open(tmp_path / "g.bam", "rb").read() == open(two_step / "a.bam", "rb").read()
    assert len(body(out)) > 50
    assert "minimizer seeding (bwa.seeder)" in p.stderr and "(host)" in p.stderr
    # an existing output without -f; with -f it is written again
    p = H.run_cli("germline", "-r", sample / "ref.fasta", *fastq(sample), "-o", out, "-b", "-v", env=mock_env, cwd=tmp_path)
    assert p.returncode == 1 and "exists (use -f)" in p.stderr
    p = H.run_cli("germline", "-f", "-r", sample / "ref.fasta", *fastq(sample), "-o", out, "-v", env=mock_env, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    assert open(out, "rb").read() == open(two_step / "h.vcf", "rb").read()


def test_without_produce_bam_no_bam_is_left_and_the_default_is_a_gvcf(sample, mock_env, tmp_path):
    out = tmp_path / "g.g.vcf"
    p = H.run_cli("germline", "-r", sample / "ref.fasta", *fastq(sample), "-o", out, "--gatk4", env=mock_env, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".bam") or f.endswith(".bai")]
    lines = body(out)
    assert any("<NON_REF>" in ln for ln in lines) and os.path.getsize(str(out) + ".gz.tbi") > 0


def test_produce_vcf_and_interval_list_reach_the_htc_half(sample, mock_env, two_step, tmp_path):
    intv = tmp_path / "part.list"
    intv.write_text("chr1:20001-60000\n")
    out = tmp_path / "g.vcf"
    p = H.run_cli("germline", "-r", sample / "ref.fasta", *fastq(sample), "-o", out, "-v", "-L", intv, env=mock_env, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = body(out)
    assert lines and not any("<NON_REF>" in ln for ln in lines)
    pos = [int(ln.split("\t")[1]) for ln in lines]
    assert min(pos) >= 20001 and max(pos) <= 60000
    whole = [ln for ln in body(two_step / "h.vcf") if 20001 <= int(ln.split("\t")[1]) <= 60000]
    assert 10 < len(lines) <= len(whole) + 2
    # the smem seeder through germline.seeder: the FMD-index path
    p = H.run_cli("germline", "-f", "-r", sample / "ref.fasta", *fastq(sample), "-o", out, "-v", "-L", intv,
                  env=dict(mock_env, FCS_GERMLINE_SEEDER="smem"), cwd=tmp_path)
    assert p.returncode == 0 and "FMD index" in p.stderr and "minimizer seeding" not in p.stderr, p.stderr[-3000:]


def test_sample_sheet_yields_one_output_per_sample(sample, mock_env, tmp_path):
    # sample A has two read groups (the two halves of the pairs), sample B one
    def halves(name):
        lines = open(sample / name).read().split("\n")
        n = (len(lines) // 4) // 2 * 4
        return lines[:n], lines[n:]
    a1, b1 = halves("sample_1.fastq")
    a2, b2 = halves("sample_2.fastq")
    for name, lines in (("a_1", a1), ("a_2", a2), ("b_1", b1), ("b_2", b2)):
        (tmp_path / f"{name}.fastq").write_text("\n".join(ln for ln in lines if ln) + "\n")
    sheet = tmp_path / "sheet.csv"
    sheet.write_text("#sample_id,fastq1,fastq2,rg,platform_id,library_id\n"
                     f"A,{tmp_path}/a_1.fastq,{tmp_path}/a_2.fastq,rgA1,illumina,libA\n"
                     f"A,{tmp_path}/b_1.fastq,{tmp_path}/b_2.fastq,rgA2,illumina,libA\n"
                     f"B,{tmp_path}/a_1.fastq,{tmp_path}/a_2.fastq,rgB,illumina,libB\n")
    out = tmp_path / "out"
    p = H.run_cli("germline", "-r", sample / "ref.fasta", "-F", sheet, "-o", out, "-b", "-v", env=mock_env, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    for s in ("A", "B"):
        for ext in (".vcf", ".vcf.gz", ".vcf.gz.tbi", ".bam", ".bam.bai"):
            assert os.path.getsize(out / (s + ext)) > 0, (s, ext)
    _, _, recs = H.read_bam(out / "A.bam")
    rgs = {H.parse_aux(r["aux"]).get("RG") for r in recs}
    assert rgs == {"rgA1", "rgA2"}
    assert len(body(out / "A.vcf")) > len(body(out / "B.vcf")) > 5


def test_argument_errors(sample, mock_env, tmp_path):
    ref = sample / "ref.fasta"
    p = H.run_cli("germline", "-r", ref, "-F", tmp_path, *fastq(sample), "-o", tmp_path / "x.vcf", env=mock_env, cwd=tmp_path)
    assert p.returncode == 1 and "cannot be specified at the same time" in p.stderr
    p = H.run_cli("germline", "-r", ref, "-o", tmp_path / "x.vcf", env=mock_env, cwd=tmp_path)
    assert p.returncode == 1 and "needs to be specified" in p.stderr
    p = H.run_cli("germline", "-r", ref, "-1", sample / "sample_1.fastq", "-o", tmp_path / "x.vcf", env=mock_env, cwd=tmp_path)
    assert p.returncode == 1 and "needs to be specified" in p.stderr
    (tmp_path / "there.vcf").write_text("x")
    p = H.run_cli("germline", "-r", ref, *fastq(sample), "-o", tmp_path / "there.vcf", env=mock_env, cwd=tmp_path)
    assert p.returncode == 1 and "exists (use -f)" in p.stderr and (tmp_path / "there.vcf").read_text() == "x"
    p = H.run_cli("germline", "-r", ref, *fastq(sample), "-o", tmp_path / "y.vcf", env=dict(mock_env, FCS_GERMLINE_SEEDER="bwt"), cwd=tmp_path)
    assert p.returncode == 1 and "smem or minimizer" in p.stderr
    assert H.run_cli("germline", "--help", cwd=tmp_path).returncode == 0
    assert "germline" in H.run_cli("--help", cwd=tmp_path).stdout
