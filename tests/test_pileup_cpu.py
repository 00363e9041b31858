"""CPU: the callers' pileup (host/pileup.h).  The exported host
statement of fcspu_pile (the oracle of the device path, the same code htc and
mutect2 run) equals the Python restatement (tests/pu_cases.py) on every hand
case and on the random world, the doubles bit for bit; and htc and mutect2 write
the same bytes with htc.gpu_pileup on, when the loaded library has no
fcspu_pile and the run takes the host path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fcship
import host_lib as H
import pu_cases as P
import ug_cases as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = P.hand_cases()
REFS = U.hand_refs()
TAB = fcship.pu_table()
TABLE = TAB.tolist()


def host_entry(batches, n, prm, w, ref, events_in, out):
    H.check(H.lib.fcsg_pu_pile(C.c_void_p(batches), n, C.c_void_p(prm), C.c_void_p(w), C.c_void_p(ref), C.c_void_p(events_in),
                               C.c_void_p(out)))


def host_pile(batches, window, refseq, **kw):
    ref, start, length = window
    return fcship.pu_pile([U.flatten(b) for b in batches], (ref, start, length, len(refseq)), refseq[start:start + length], TAB,
                          entry=host_entry, **kw)


def host_op_events(records, window, refseq):
    ref, start, length = window
    arrays = fcship.ug_arrays(*U.flatten(records))
    b = fcship.ug_batch(arrays)
    w = fcship.UgWindow(ref, 0, start, length, len(refseq))
    out = np.zeros(length, np.int32)
    H.check(H.lib.fcsg_pu_op_events(C.c_void_p(C.addressof(b)), C.c_void_p(C.addressof(w)), C.c_char_p(refseq.encode()),
                                    C.c_void_p(out.ctypes.data)))
    return out


def test_table_is_log10_of_the_documented_formulas():
    want = np.array(P.table_formulas())
    assert TAB.shape == (94, 3) and np.all(TAB < 0)
    assert np.max(np.abs(TAB - want) / np.abs(want)) <= 1e-14
    assert np.array_equal(TAB[0], np.full(3, TAB[0][0]))   # e is capped at 0.75: the three entries of q = 0 are log10(0.25)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_case(case):
    refseq = REFS[case["window"][0]]
    ops = P.op_events(case["batches"][0], case["window"], refseq)
    assert np.array_equal(ops, P.sparse(case["window"][2], case["ops"]))
    assert np.array_equal(host_op_events(case["batches"][0], case["window"], refseq), ops)
    want = P.pile(case["batches"], case["window"], refseq, TABLE, frac=case["frac"], events_in=ops)
    assert P.same(dict(want, snvs=[dict(offset=o, alt=ord(b), count=c) for o, b, c in want["snvs"]]), P.want_of(case))
    assert P.same(host_pile(case["batches"], case["window"], refseq, frac=case["frac"], events_in=ops), want)


def test_quality_above_93_adds_row_93():
    case = next(c for c in CASES if c["name"] == "quality_94_and_above_takes_row_93")
    got = host_pile(case["batches"], case["window"], REFS[0])
    for off, row in ((800, 93), (801, 93), (802, 93), (803, 30)):
        assert got["gl"][off].tolist() == [TABLE[row][0], TABLE[row][1], TABLE[row][2]]


def test_op_events_feed_the_site_predicate():
    """Two reads with the same insertion: no mismatch event, but the anchor is a site through events_in."""
    records = [P.read(REFS, 40, "6M2I6M")] * 2
    ops = P.op_events(records, (0, 0, 100), REFS[0])
    assert ops[45] == 2 and ops.sum() == 2
    assert host_pile([records], (0, 0, 100), REFS[0])["sites"].tolist() == []
    got = host_pile([records], (0, 0, 100), REFS[0], events_in=ops)
    assert got["sites"].tolist() == [45] and got["events"].sum() == 0


@pytest.fixture(scope="module")
def world():
    return P.random_world()


def test_random_world(world):
    records = P.random_batch(world)
    assert 1400 <= len(records) <= 1600
    for c, seq in enumerate(world):
        window = (c, 0, len(seq))
        ops = P.op_events(records, window, seq)
        assert np.array_equal(host_op_events(records, window, seq), ops) and ops.sum() > 50
        want = P.pile([records], window, seq, TABLE, events_in=ops)
        assert len(want["sites"]) > 20 and len(want["snvs"]) > 20 and want["depth"].max() > 10
        assert P.same(host_pile([records], window, seq, events_in=ops), want)
        assert P.same(host_pile([records], window, seq, want_gl=False), P.pile([records], window, seq, TABLE, want_gl=False))
    other = P.random_batch(world, seed=12, n=600)
    want = P.pile([records, other], (0, 0, len(world[0])), world[0], TABLE)
    assert P.same(host_pile([records, other], (0, 0, len(world[0])), world[0]), want)
    assert P.same(host_pile([records], (1, 63, 3 * 256 + 5), world[1]),
                  P.cut(P.pile([records], (1, 0, len(world[1])), world[1], TABLE), 63, 3 * 256 + 5))


def test_order_of_equal_positions_changes_the_sums(world):
    """The device test of "gl follows the order given" is not vacuous: reversing the records of equal position changes
    at least one locus's bits."""
    records = P.random_batch(world)
    flipped = P.reversed_ties(records)
    assert flipped != records and sorted(map(id, flipped)) == sorted(map(id, records))
    window = (0, 0, len(world[0]))
    a, b = P.pile([records], window, world[0], TABLE), P.pile([flipped], window, world[0], TABLE)
    assert np.array_equal(a["depth"], b["depth"]) and a["sites"] == b["sites"] and a["snvs"] == b["snvs"]
    differ = np.any(a["gl"].view(np.uint64) != b["gl"].view(np.uint64), axis=1)
    assert differ.sum() >= 1
    assert P.same(host_pile([flipped], window, world[0]), b)


def test_too_small_maxima_are_refused():
    case = next(c for c in CASES if c["name"] == "two_alt_letters_at_one_locus")
    with pytest.raises(RuntimeError, match="1 sites and 2 SNVs, max_sites is 1 and max_snvs 1"):
        host_pile(case["batches"], case["window"], REFS[0], max_snvs=1, max_sites=1)


# ------------------------------------------------------------------ the commands keep their bytes
@pytest.fixture(scope="module")
def mock_dir():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpu_mock")], check=True, capture_output=True)
    return os.path.join(ROOT, "tests", "cpu_mock", "build")


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    d = tmp_path_factory.mktemp("pu")
    p = H.run_cli("synth", "-o", d, "-c", "chr1:60000,chr2:20000", "-x", "6", "--seed", "5", "--no-fastq", "--tumor")
    assert p.returncode == 0, p.stderr[-2000:]
    return d


def run_both(args, out_name, synth, mock_dir, tmp_path):
    logs = {}
    for mode in ("false", "true"):
        env = {"LD_LIBRARY_PATH": mock_dir, "FCS_GPU_DEVICES": "0", "FCS_MOCK_PHMM": "java", "FCS_GATK_NCONTIGS": "4",
               "FCS_LOG_DIR": str(tmp_path / f"log_{mode}"), "FCS_HTC_GPU_PILEUP": mode, "FCS_HTC_PILEUP_CHUNK_BP": "4096"}
        p = H.run_cli(*args, "-o", tmp_path / f"{mode}_{out_name}", env=env, cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-3000:]
        text = p.stderr
        for root, _, files in os.walk(tmp_path / f"log_{mode}"):
            text += "".join(open(os.path.join(root, f), errors="replace").read() for f in files)
        logs[mode] = text
    notice = "htc.gpu_pileup: the loaded libfcship has no fcspu_pile entry point"
    assert logs["true"].count(notice) == 1 and notice not in logs["false"]
    for s in ("", ".gz", ".gz.tbi"):
        a, b = tmp_path / f"true_{out_name}{s}", tmp_path / f"false_{out_name}{s}"
        assert a.read_bytes() == b.read_bytes(), s
    return (tmp_path / f"true_{out_name}").read_text()


def test_htc_gvcf_keeps_its_bytes_with_the_key_on_and_no_entry_point(synth, mock_dir, tmp_path):
    text = run_both(["htc", "-f", "-r", synth / "ref.fasta", "-i", synth / "sample.bam"], "g.vcf", synth, mock_dir, tmp_path)
    lines = [ln for ln in text.splitlines() if not ln.startswith("#")]
    assert any("<NON_REF>\t.\t.\tEND=" in ln for ln in lines) and any("END=" not in ln for ln in lines)


def test_mutect2_keeps_its_bytes_with_the_key_on_and_no_entry_point(synth, mock_dir, tmp_path):
    run_both(["mutect2", "-f", "-r", synth / "ref.fasta", "-n", synth / "sample.bam", "-t", synth / "tumor.bam"], "m.vcf", synth,
             mock_dir, tmp_path)
