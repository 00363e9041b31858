"""What the host runners of markdup, baserecal / printreads / bqsr, depth and
ug share (host/bam_stream.h): the part-BAM rule, the record stream over file
boundaries and its order check, the windows, the contigs, the @RG lines and the
handlers' checks, pinned through the fcs-genome binary on the host path (the
CPU mock of libfcship), and through tools/micro/bam_stream_test.cpp.  No GPU.

- One world (tests/bam_stream_cases.py) as a single BAM, as a directory of two
  parts and as a directory whose part boundary lies between two records at one
  position: every output file of depth, ug, baserecal and bqsr is the same
  bytes for every chunk size around the file boundary, at windows of 1,024
  loci.
- The order check: across a file boundary, after an unmapped record, and past
  ug's last window; baserecal does not check.
- Every refusal of the six commands with its exit status and its line on
  stderr, and which of two faults is reported.
- The @RG rules: PU names a read group, else its ID; a line without an ID is
  no read group but its SM counts; read groups that share an LB are one
  library.
"""
import os
import re
import shutil
import subprocess

import pytest

import bam_stream_cases as S
import host_lib as H
import markdup_cases as M
from test_markdup_cpu import add_rg_tags, sam_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERROR = "[fcs-genome] ERROR: "
INVALID = ERROR + "Failed to parse arguments: invalid option Invalid parameter: "
MISSING = ERROR + "Cannot find "
DEPTH_SUFFIXES = ["", ".sample_summary", ".sample_statistics", ".sample_cumulative_coverage_counts",
                  ".sample_cumulative_coverage_proportions", ".sample_interval_summary", ".sample_interval_statistics"]
UG_SUFFIXES = ["", ".gz", ".gz.tbi"]
# command: (the output option's file name, the suffixes of the files it writes, the chunk key, a figure of the stats line)
STREAMING = {"depth": ("cov", DEPTH_SUFFIXES, "FCS_DEPTH_CHUNK_RECORDS", r"total depth (\d+),"),
             "ug": ("out.vcf", UG_SUFFIXES, "FCS_UG_CHUNK_RECORDS", r" (\d+) calls,"),
             "baserecal": ("out.grp", [""], "FCS_BQSR_CHUNK_RECORDS", r" (\d+) counted,"),
             "bqsr": ("out.bam", ["", ".grp"], "FCS_BQSR_CHUNK_RECORDS", r" (\d+) recalibrated,")}


@pytest.fixture(scope="module")
def env():
    subprocess.run(["make", "-C", f"{ROOT}/tests/cpu_mock"], check=True, capture_output=True)
    return {"LD_LIBRARY_PATH": f"{ROOT}/tests/cpu_mock/build", "FCS_GPU_DEVICES": "0", "FCS_MARKDUP_GPU": "false",
            "FCS_BQSR_GPU": "false", "FCS_DEPTH_GPU": "false", "FCS_UG_GPU": "false",
            "FCS_DEPTH_WINDOW_BP": str(S.WINDOW_BP), "FCS_UG_WINDOW_BP": str(S.WINDOW_BP)}


class World:
    pass


@pytest.fixture(scope="module")
def w(tmp_path_factory):
    """The world's files: ref.fa, one.bam, parts/ (k and n - k records) and same/ (the boundary inside one position)."""
    w = World()
    w.d = tmp_path_factory.mktemp("bst")
    w.refs, w.records = S.world()
    w.n, w.k, w.k2 = len(w.records), S.file_boundary(w.records), S.same_position_boundary(w.records)
    w.ref = S.write_fasta(w.d / "ref.fa", w.refs)
    w.one = S.write_bam(w.d / "one.bam", w.records)
    w.parts = S.write_parts(w.d / "parts", w.records[:w.k], w.records[w.k:])
    w.same = S.write_parts(w.d / "same", w.records[:w.k2], w.records[w.k2:])
    return w


def run(cmd, ref, bam, out, *extra, env=None, cwd=None):
    args = ["-r", ref, "-i", bam, "-o", out, *extra]
    if cmd == "bqsr":
        args += ["-b", str(out) + ".grp"]
    return H.run_cli(cmd, *args, env=env, cwd=cwd)


def last_line(p):
    return p.stderr.rstrip("\n").split("\n")[-1]


# ------------------------------------------------------------------ chunk, file and window boundaries
def test_the_world_is_the_issue_s(w):
    recs, n, k, k2 = w.records, w.n, w.k, w.k2
    mapped = [r for r in recs if r["ref"] >= 0]
    assert [len(s) for s in w.refs] == [6000, 6000] and len(mapped) == 1200 and n == 1200 + S.TAIL > 2 * 7
    assert 90 < sum(r["n_bases"] for r in mapped) / len(mapped) < 110
    for op in "IDS":
        assert sum(op in r["cigar"] for r in mapped) > 50
    assert recs == sorted(recs, key=S.key) and all(r["ref"] == -1 and r["flag"] & 0x4 for r in recs[1200:])
    assert {r["rg"] for r in recs} == {"a", "b"} and S.HEADER.count("SM:NA12878") == S.HEADER.count("@RG") == 2
    assert 7 < k - 1 and k + 1 < n and k != k2
    # the file boundary: the record before it reaches over a window edge that the record after it starts before
    a, b = recs[k - 1], recs[k]
    edge = (a["pos"] // S.WINDOW_BP + 1) * S.WINDOW_BP
    assert a["ref"] == b["ref"] and a["pos"] < b["pos"] < edge < S.end(a)
    assert recs[k2 - 1]["ref"] == recs[k2]["ref"] and recs[k2 - 1]["pos"] == recs[k2]["pos"]
    # every window of both contigs holds the start of a record, and every inner window edge lies inside one
    for c in (0, 1):
        on = [r for r in mapped if r["ref"] == c]
        assert {r["pos"] // S.WINDOW_BP for r in on} == set(range(6))
        for e in range(S.WINDOW_BP, 6000, S.WINDOW_BP):
            assert any(r["pos"] < e < S.end(r) for r in on)


@pytest.mark.parametrize("cmd", list(STREAMING))
def test_every_chunk_size_and_part_layout_writes_the_same_bytes(cmd, w, env, tmp_path):
    name, suffixes, chunk_key, figure = STREAMING[cmd]
    want = None
    for tag, bam in (("one", w.one), ("parts", w.parts), ("same", w.same)):
        for chunk in (None, 1, 7, w.k - 1, w.k, w.k + 1, w.n):
            out = tmp_path / f"{tag}{chunk}" / name
            os.makedirs(out.parent)
            p = run(cmd, w.ref, bam, out, env={**env, **({} if chunk is None else {chunk_key: str(chunk)})}, cwd=tmp_path)
            assert p.returncode == 0 and "(host)" in p.stderr, (tag, chunk, p.stderr[-2000:])
            assert f" {w.n} records, " in last_line(p), (tag, chunk, last_line(p))
            assert int(re.search(figure, last_line(p)).group(1)) > 0
            if cmd in ("depth", "ug"):
                assert " 2 intervals, 12 windows, " in last_line(p)
            assert sorted(os.listdir(out.parent)) == sorted(name + s for s in suffixes)
            got = [(out.parent / (name + s)).read_bytes() for s in suffixes]
            want = want or got
            assert got == want, (tag, chunk, [a == b for a, b in zip(got, want)])
            shutil.rmtree(out.parent)


# ------------------------------------------------------------------ the order check
def unsorted_line(r, after):
    return f"{INVALID}the input is not coordinate-sorted: record {r['name']} at {S.place(r)} follows one at {S.place(after)}"


def test_a_part_that_starts_before_its_predecessor_s_end(w, env, tmp_path):
    recs, k = w.records, w.k   # records k - 1 and k lie at different positions of one contig: they change places
    d = S.write_parts(tmp_path / "swapped", recs[:k - 1] + [recs[k]], [recs[k - 1]] + recs[k + 1:])
    for cmd in ("depth", "ug"):
        for chunk in (None, 7):
            e = {**env, **({} if chunk is None else {STREAMING[cmd][2]: str(chunk)})}
            p = run(cmd, w.ref, d, tmp_path / STREAMING[cmd][0], env=e, cwd=tmp_path)
            assert p.returncode == 1 and last_line(p) == unsorted_line(recs[k - 1], recs[k]), p.stderr[-2000:]
    assert not [f for f in os.listdir(tmp_path) if os.path.isfile(tmp_path / f)]   # a refused run leaves no file
    p = run("baserecal", w.ref, d, tmp_path / "out.grp", env=env, cwd=tmp_path)
    assert p.returncode == 0 and f" {w.n} records, " in last_line(p), p.stderr[-2000:]


def test_a_mapped_record_after_an_unmapped_one(w, env, tmp_path):
    recs = w.records
    bam = S.write_bam(tmp_path / "tail.bam", recs[:40] + [recs[-1], recs[40]])
    for cmd in ("depth", "ug"):
        p = run(cmd, w.ref, bam, tmp_path / STREAMING[cmd][0], env=env, cwd=tmp_path)
        assert p.returncode == 1, p.stderr[-2000:]
        assert last_line(p) == f"{INVALID}the input is not coordinate-sorted: record r40 at {S.place(recs[40])} follows one at *:0"
    # an unmapped record that carries a contig and a position sorts there
    placed = dict(recs[-1], ref=recs[40]["ref"], pos=recs[40]["pos"])
    bam = S.write_bam(tmp_path / "placed.bam", recs[:40] + [placed, recs[40]])
    assert run("depth", w.ref, bam, tmp_path / "cov", env=env, cwd=tmp_path).returncode == 0


def test_a_violation_past_ug_s_last_window(w, env, tmp_path):
    recs = w.records
    j = next(k for k in range(1000, 1200) if recs[k]["ref"] == 1 and recs[k - 1]["pos"] < recs[k]["pos"])
    bam = S.write_bam(tmp_path / "late.bam", recs[:j - 1] + [recs[j], recs[j - 1]] + recs[j + 1:])
    (tmp_path / "a.bed").write_text("ctgA\t0\t6000\n")
    for chunk in ("100", "100000"):
        p = run("ug", w.ref, bam, tmp_path / "out.vcf", "-L", tmp_path / "a.bed", env={**env, "FCS_UG_CHUNK_RECORDS": chunk},
                cwd=tmp_path)
        assert p.returncode == 1 and last_line(p) == unsorted_line(recs[j - 1], recs[j]), p.stderr[-2000:]
        assert not os.path.exists(tmp_path / "out.vcf") and not os.path.exists(tmp_path / "out.vcf.gz")
    # the same interval list over the sorted input is a run like any other
    p = run("ug", w.ref, w.one, tmp_path / "out.vcf", "-L", tmp_path / "a.bed", env=env, cwd=tmp_path)
    assert p.returncode == 0 and f" {w.n} records, 1 intervals, 6 windows, " in last_line(p), p.stderr[-2000:]


# ------------------------------------------------------------------ refusals and their order
@pytest.fixture(scope="module")
def bad(w, tmp_path_factory):
    """Inputs that are refused, or accepted by the commands that do not look: b.<name> are paths."""
    b = World()
    d = b.d = tmp_path_factory.mktemp("bad")
    few = w.records[:60] + w.records[-2:]
    b.none = str(d / "none")
    b.empty_dir = str(d / "empty")
    os.makedirs(b.empty_dir)
    b.few = S.write_bam(d / "few.bam", few)
    b.no_sm = S.write_bam(d / "no_sm.bam", few, header="@RG\tID:a\n@RG\tID:b\tSM:\n")
    b.two_sm = S.write_bam(d / "two_sm.bam", few, header="@RG\tID:a\tSM:one\n@RG\tID:b\tSM:two\n")
    b.ref_one = S.write_fasta(d / "one_contig.fa", w.refs[:1])
    b.ref_long = S.write_fasta(d / "long.fa", [w.refs[0], w.refs[1] + "ACGTACGTAC"])
    b.gene_list = str(d / "genes.list")
    open(b.gene_list, "w").write("GENE1\n")
    b.beyond = str(d / "beyond.list")
    open(b.beyond, "w").write("ctgA:10-20\nctgA:7000-7100\n")
    b.empty = str(d / "empty.list")
    open(b.empty, "w").write("ctgA:10-20\nctgB:301-300\n")
    b.sites = str(d / "sites.vcf")
    open(b.sites, "w").write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\nctgA\t100\t.\tA\tC\t.\t.\t.\n")
    return b


def good(cmd, w, b, out):
    """The command's options over good inputs, as {option: value}."""
    o = {"-r": w.ref, "-i": b.few, "-o": out}
    if cmd == "markdup":
        del o["-r"]
    if cmd == "printreads":
        o["-b"] = b.report
    return o


def cli(cmd, options, env, cwd):
    args = []
    for k, v in options.items():
        if v is not None:
            args += [k] if v is True else [k, v]
    return H.run_cli(cmd, *args, env=env, cwd=cwd)


COMMANDS = ["markdup", "baserecal", "printreads", "bqsr", "depth", "ug"]
REQUIRED = {"-r": "--ref", "-i": "--input", "-o": "--output", "-b": "--bqsr"}


@pytest.fixture(scope="module")
def report(w, bad, env):
    """A report of baserecal over the good input, for printreads."""
    bad.report = str(bad.d / "few.grp")
    p = H.run_cli("baserecal", "-r", w.ref, "-i", bad.few, "-o", bad.report, env=env, cwd=bad.d)
    assert p.returncode == 0, p.stderr[-2000:]
    return bad.report


@pytest.mark.parametrize("cmd", COMMANDS)
def test_refusals(cmd, w, bad, report, env, tmp_path):
    b, out = bad, str(tmp_path / "o")
    base = good(cmd, w, b, out)
    outputs = {"depth": [out + s for s in DEPTH_SUFFIXES], "ug": [out + s for s in UG_SUFFIXES]}.get(cmd, [out])
    takes_l, has_ref, streams = cmd != "markdup", cmd != "markdup", cmd in ("depth", "ug")
    counts = cmd in ("baserecal", "bqsr")

    def refused(options, rc, line):
        p = cli(cmd, options, env, tmp_path)
        assert (p.returncode, last_line(p)) == (rc, line), (options, p.returncode, p.stderr[-2000:])
        assert not [f for f in outputs if os.path.exists(f)], options

    def accepted(options):
        p = cli(cmd, options, env, tmp_path)
        assert p.returncode == 0 and last_line(p).endswith(" s (host)"), (options, p.stderr[-2000:])
        for f in os.listdir(tmp_path):
            os.remove(tmp_path / f)

    accepted(base)
    # a missing required option
    for opt in base:
        refused({**base, opt: None}, 1, f"{INVALID}{REQUIRED[opt]} is required")
    # files that are not there
    if has_ref:
        refused({**base, "-r": b.none}, 3, MISSING + b.none)
        refused({**base, "-r": b.empty_dir}, 3, MISSING + b.empty_dir)
    refused({**base, "-i": b.none}, 3, MISSING + b.none)
    refused({**base, "-i": b.empty_dir}, 3, MISSING + b.empty_dir + ("" if cmd == "markdup" else "/*.bam"))
    if takes_l:
        refused({**base, "-L": b.none}, 3, MISSING + b.none)
        refused({**base, "-L": ""}, 1, ERROR + "Failed to parse arguments: option Path of intervalList is empty cannot be empty")
    if counts:
        refused({**base, "-K": b.none}, 3, MISSING + b.none)
    if cmd == "printreads":
        refused({**base, "-b": b.none}, 3, MISSING + b.none)
    # every output file, one at a time
    for f in outputs + ([out + ".grp"] if cmd == "bqsr" else []):
        open(f, "w").write("kept")
        options = {**base, **({"-b": out + ".grp"} if cmd == "bqsr" else {})}
        p = cli(cmd, options, env, tmp_path)
        assert (p.returncode, last_line(p)) == (1, f"{INVALID}output {f} exists (use -f)"), p.stderr[-2000:]
        assert open(f).read() == "kept" and [x for x in sorted(os.listdir(tmp_path))] == [os.path.basename(f)]
        os.remove(f)
    # the header's samples
    if streams:
        refused({**base, "-i": b.no_sm}, 1, INVALID + "the BAM header names no sample (no @RG line with SM)")
        refused({**base, "-i": b.two_sm}, 1, f"{INVALID}the BAM header names 2 samples (one, two); {cmd} takes one")
    elif cmd != "printreads":   # (printreads needs the report's read groups)
        accepted({**base, "-i": b.no_sm})
        accepted({**base, "-i": b.two_sm})
    # the contigs of the header against the FASTA
    if streams or counts:
        refused({**base, "-r": b.ref_one}, 1, f"{INVALID}contig ctgB of the BAM header is not in {b.ref_one}")
    if streams:
        refused({**base, "-r": b.ref_long}, 1,
                f"{INVALID}contig ctgB has 6000 bases in the BAM header and 6010 in {b.ref_long}")
    elif has_ref:
        accepted({**base, "-r": b.ref_long})
    if cmd == "printreads":   # it reads no reference base
        accepted({**base, "-r": b.ref_one})
    # options that are refused, and intervals that hold nothing
    if cmd == "depth":
        refused({**base, "-g": b.gene_list}, 1, INVALID + "--geneList: gene summaries are not built")
        refused({**base, "--geneList": b.none}, 1, INVALID + "--geneList: gene summaries are not built")
    if cmd == "ug":
        refused({**base, "--skip-concat": True}, 1,
                INVALID + "--skip-concat: one run is one stream and writes one VCF, there are no parts to keep")
    if streams:
        refused({**base, "-L": b.beyond}, 1, f"{INVALID}interval ctgA:7000-7100 of {b.beyond} is empty or beyond its contig")
        refused({**base, "-L": b.empty}, 1, f"{INVALID}interval ctgB:301-300 of {b.empty} is empty or beyond its contig")
    elif takes_l:
        accepted({**base, "-L": b.beyond})
        accepted({**base, "-L": b.empty})
    # two faults at once: the one that is reported
    open(out, "w").write("kept")

    def refused_kept(options, rc, line):
        check_kept(cmd, options, rc, line, env, tmp_path)

    refused_kept({**base, "-i": b.none}, 3, MISSING + b.none)                       # a missing input, an existing output
    if has_ref:
        refused_kept({**base, "-r": b.none, "-i": b.none}, 3, MISSING + b.none)     # the reference before the input
        refused_kept({**base, "-i": b.empty_dir}, 1, f"{INVALID}output {out} exists (use -f)")   # the output before the part BAMs
        refused_kept({**base, "-L": b.none}, 3, MISSING + b.none)                   # -L before the output
    if counts:
        refused_kept({**base, "-K": b.none}, 3, MISSING + b.none)                   # known sites before the output
        refused_kept({**base, "-L": b.none + ".bed", "-K": b.none}, 3, MISSING + b.none + ".bed")   # -L before known sites
    if cmd == "printreads":
        refused_kept({**base, "-b": b.none}, 3, MISSING + b.none)                   # the report before the output
    if cmd == "bqsr":
        open(out + ".grp", "w").write("kept")
        refused_kept({**base, "-b": out + ".grp"}, 1, f"{INVALID}output {out} exists (use -f)")   # the BAM before the report
        os.remove(out + ".grp")
    if cmd == "depth":
        refused_kept({**base, "-g": b.gene_list, "-r": b.none}, 1, INVALID + "--geneList: gene summaries are not built")
    if cmd == "ug":
        refused_kept({**base, "--skip-concat": True, "-r": b.none}, 1,
                     INVALID + "--skip-concat: one run is one stream and writes one VCF, there are no parts to keep")
    os.remove(out)
    if streams:   # inside the run: the sample, then the contigs, then the intervals, then the records' order
        refused({**base, "-i": b.two_sm, "-r": b.ref_one}, 1, f"{INVALID}the BAM header names 2 samples (one, two); {cmd} takes one")
        refused({**base, "-r": b.ref_one, "-L": b.beyond}, 1, f"{INVALID}contig ctgB of the BAM header is not in {b.ref_one}")
        recs = w.records
        j = next(j for j in range(8) if S.key(recs[j]) < S.key(recs[j + 1]))
        swapped = S.write_bam(tmp_path / "swapped.bam", recs[:j] + [recs[j + 1], recs[j]] + recs[j + 2:9])
        refused({**base, "-i": swapped, "-L": b.beyond}, 1,
                f"{INVALID}interval ctgA:7000-7100 of {b.beyond} is empty or beyond its contig")
        refused({**base, "-i": swapped}, 1, unsorted_line(recs[j], recs[j + 1]))


def check_kept(cmd, options, rc, line, env, cwd):
    """The refusal, with the files that were there before it untouched."""
    before = {f: open(cwd / f).read() for f in os.listdir(cwd) if os.path.isfile(cwd / f)}
    p = cli(cmd, options, env, cwd)
    assert (p.returncode, last_line(p)) == (rc, line), (options, p.returncode, p.stderr[-2000:])
    assert {f: open(cwd / f).read() for f in os.listdir(cwd) if os.path.isfile(cwd / f)} == before


# ------------------------------------------------------------------ the @RG rules
RG_HEADER = ("@RG\tID:a\tPU:unitA\tSM:s1\tLB:lib1\n"     # a PU
             "@RG\tID:b\tSM:s1\tLB:lib1\n"               # no PU, the same SM and the same LB
             "@RG\tID:\tPU:ghost\tSM:s1\tLB:lib2\n")     # an empty ID


def test_read_group_names_of_the_report_and_samples_of_lines_without_an_id(w, env, tmp_path):
    few = w.records[:300]
    bam = S.write_bam(tmp_path / "rg.bam", few, header=RG_HEADER)
    p = run("baserecal", w.ref, bam, tmp_path / "rg.grp", env=env, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    text = (tmp_path / "rg.grp").read_text()
    table0 = text.split("#:GATKTable:RecalTable0:\n")[1].split("\n\n")[0].split("\n")
    assert [ln.split()[0] for ln in table0] == ["ReadGroup", "unitA", "b"]
    assert "ghost" not in text
    p = run("depth", w.ref, bam, tmp_path / "cov", env=env, cwd=tmp_path)
    assert p.returncode == 0 and "sample s1: 300 records" in last_line(p), p.stderr[-2000:]
    # the SM of a line without an ID counts; an empty SM does not
    other = S.write_bam(tmp_path / "sm.bam", few, header=RG_HEADER.replace("ghost\tSM:s1", "ghost\tSM:s2") + "@RG\tID:c\tSM:\n")
    for cmd in ("depth", "ug"):
        p = run(cmd, w.ref, other, tmp_path / "x", env=env, cwd=tmp_path)
        assert (p.returncode, last_line(p)) == (1, f"{INVALID}the BAM header names 2 samples (s1, s2); {cmd} takes one")
    p = run("baserecal", w.ref, other, tmp_path / "sm.grp", env=env, cwd=tmp_path)
    assert p.returncode == 0 and (tmp_path / "sm.grp").read_text() == text


def test_read_groups_that_share_a_library_are_marked_together(env, tmp_path):
    """Markdup's two-library hand case under the header above: a and b share lib1, so one pair of the two is flagged."""
    _, recs, _ = M.hand_cases()[9]
    assert {r["lib"] for r in recs} == {0, 1}
    flags = {}
    for name, header in (("shared", RG_HEADER), ("apart", RG_HEADER.replace("ID:b\tSM:s1\tLB:lib1", "ID:b\tSM:s1\tLB:lib3")),
                         ("no_lb", RG_HEADER.replace("\tLB:lib1", ""))):
        txt = tmp_path / f"{name}.txt"
        txt.write_text(header + sam_text(recs, rgs=()))
        H.check(H.lib.fcsg_text_to_bam(str(txt).encode(), str(tmp_path / "plain.bam").encode(), b"chr1", b"900000"))
        add_rg_tags(tmp_path / "plain.bam", tmp_path / f"{name}.bam", ["ab"[r["lib"]] for r in recs])
        p = H.run_cli("markdup", "-i", tmp_path / f"{name}.bam", "-o", tmp_path / f"{name}.out.bam", env=env, cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-2000:]
        flags[name] = [r["flag"] for r in H.read_bam(tmp_path / f"{name}.out.bam")[2]]
    before = [r["flag"] for r in recs]
    assert flags["apart"] == before
    assert flags["shared"] == flags["no_lb"] != before   # read groups without an LB are one library too
    assert [a ^ b for a, b in zip(flags["shared"], before)] == [0, 0, 0x400, 0x400, 0, 0x400]


# ------------------------------------------------------------------ bam_stream.h under sanitizers
@pytest.fixture(scope="module")
def stream_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    subprocess.run(["make", "-C", f"{ROOT}/tests/cpu_mock"], check=True, capture_output=True)
    exe = tmp_path_factory.mktemp("bsx") / "bam_stream_test"
    pkg, mock = os.path.join(ROOT, "falcon-genome_amd"), os.path.join(ROOT, "tests", "cpu_mock", "build")
    host = [os.path.join(pkg, "host", f) for f in ("bam_stream.cpp", "bam.cpp", "bgzf.cpp", "fasta.cpp", "intervals.cpp",
                                                   "common.cpp")]
    # bgzf.cpp reads through fcs_bgzf_index and fcs_bgzf_inflate_try: the CPU mock of libfcship has them, no device library
    subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(pkg, "csrc"), "-I" + os.path.join(pkg, "host"),
                    os.path.join(ROOT, "tools", "micro", "bam_stream_test.cpp"), *host, "-L" + mock, "-lfcship",
                    "-Wl,-rpath," + mock, "-lz", "-ldl", "-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_stream_windows_and_rg_lines_under_sanitizers(stream_exe, seed, tmp_path):
    r = subprocess.run([str(stream_exe), str(seed), str(tmp_path)], capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "MISMATCH" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    fig = dict(zip(r.stdout.split()[0::2], r.stdout.split()[1::2]))
    assert int(fig["reads"]) > 0 and int(fig["windows"]) > 0 and int(fig["rg_lines"]) == 3
