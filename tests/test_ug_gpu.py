"""GPU: pileup SNP genotyping (fcsug_sites and its _dev twin)
equals the Python restatement of the rules (tests/ug_cases.py) exactly."""
import ctypes as C
import threading

import numpy as np
import pytest

import bam_stream_cases as S
import fcship
import host_lib as H
import ug_cases as U

pytestmark = pytest.mark.gpu
CASES = U.hand_cases()
REFS = U.hand_refs()
TAB = U.table()
T = fcship.FCSUG_TILE
SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
CLEAN = "".join(U.LETTERS[p % 4] for p in range(4 * T))   # a contig without N


def device_sites(records, window, refseq, min_baseq=17, gpu=0, first_offset=0, max_sites=None):
    ref, start, length = window
    return fcship.ug_sites(U.flatten(records, first_offset), (ref, start, length, len(refseq)), refseq[start:start + length], TAB,
                           min_baseq, max_sites, device=gpu)


def clipped(sites, start, length):
    """The whole contig's sites cut to a window."""
    return U.full([dict(s, offset=s["offset"] - start) for s in sites if start <= s["offset"] < start + length])


@pytest.fixture(scope="module")
def world():
    return U.random_world()


@pytest.fixture(scope="module")
def random_case(world):
    """(records, the restatement's sites per contig) of the random batch, computed once."""
    records = U.random_batch(world)
    return records, [U.sites(records, (c, 0, len(s)), s, TAB)[0] for c, s in enumerate(world)]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_case(gpu, case):
    refseq = REFS[case["window"][0]]
    if case["beyond"]:   # the host-pointer call refuses the record; the _dev twin clips it (below)
        with pytest.raises(fcship.FcsError, match="aligned base beyond its contig"):
            device_sites(case["records"], case["window"], refseq, gpu=gpu)
        return
    got = device_sites(case["records"], case["window"], refseq, gpu=gpu)
    assert U.brief(got) == U.want_sites(case)
    assert U.full(got) == U.full(U.sites(case["records"], case["window"], refseq, TAB)[0])


def test_all_hand_cases_as_one_batch_and_the_smallest_batches(gpu):
    records = sorted((r for c in CASES if not c["beyond"] for r in c["records"]), key=lambda r: (r["ref"], r["pos"]))
    for min_baseq in (17, 0, 31):
        for window in ((0, 0, 1200), (0, 100, 50), (0, 12, 1), (0, T - 1, 2), (1, 0, 40)):
            want = U.sites(records, window, REFS[window[0]], TAB, min_baseq)[0]
            assert U.full(device_sites(records, window, REFS[window[0]], min_baseq, gpu)) == U.full(want)
    assert len(U.sites(records, (0, 0, 1200), REFS[0], TAB)[0]) > 15
    assert len(device_sites([], (0, 0, 300), REFS[0], gpu=gpu)) == 0
    one = device_sites([U.rec(0, 0, 1199, "1M", "A")], (0, 0, 1200), REFS[0], gpu=gpu)
    assert U.brief(one) == [dict(offset=1199, ref=3, alt=0, n=[1, 0, 0, 0], n_del=0)]
    assert len(device_sites([U.rec(0, 0, 1199, "1M", "A")], (0, 5, 0), REFS[0], gpu=gpu)) == 0


@pytest.mark.parametrize("start", [0, 1, T - 1])
def test_windows_of_every_length_around_a_tile(gpu, world, random_case, start):
    records, want = random_case
    for length in (1, T - 1, T, T + 1, 3 * T + 5):
        for c in (0, 2):
            got = device_sites(records, (c, start, length), world[c], gpu=gpu)
            assert U.full(got) == clipped(want[c], start, length), (c, start, length)
    assert len(clipped(want[0], start, 3 * T + 5)) > 5


def all_sites_batch():
    """Records of 64 bases that tile loci [3, 3 + 3 T) of CLEAN, every base unlike the reference."""
    return [U.rec(0, 0, p, "64M", "".join(U.other(ch) for ch in CLEAN[p:p + 64])) for p in range(3, 3 + 3 * T, 64)]


def test_every_locus_of_three_tiles_is_a_site(gpu):
    records = all_sites_batch()
    window = (0, 3, 3 * T)
    want = U.sites(records, window, CLEAN, TAB)[0]
    assert [s["offset"] for s in want] == list(range(3 * T))
    got = device_sites(records, window, CLEAN, gpu=gpu, max_sites=3 * T)      # exactly enough
    assert U.full(got) == U.full(want)
    with pytest.raises(fcship.FcsError, match=f"the window has {3 * T} sites, max_sites is {3 * T - 1}"):
        device_sites(records, window, CLEAN, gpu=gpu, max_sites=3 * T - 1)    # one too few


def test_70000_copies_are_exact(gpu):
    seq = "".join(U.other(ch) for ch in CLEAN[10:13])
    records = [U.rec(0, 0, 10, "3M", seq)] * 70000
    got = U.full(device_sites(records, (0, 0, 64), CLEAN, gpu=gpu))
    assert [s["offset"] for s in got] == [10, 11, 12]
    for s in got:
        assert s["n"][s["alt"]] == 70000 and s["qsum"][s["alt"]] == 2100000 and s["mq2"] == 70000 * 3600
        assert s["gl"] == [70000 * TAB[30][2], 70000 * TAB[30][1], 70000 * TAB[30][0]]


@pytest.mark.parametrize("first", [0, 1, 3])
def test_sweep_batch_at_every_offset_residue(gpu, world, first):
    records, n = U.sweep_batch(world), len(world[0])
    assert {r["n_bases"] for r in records} == set(range(1, 201))
    want = U.sites(records, (0, 0, n), world[0], TAB, 5)[0]
    assert len(want) > 1000
    assert U.full(device_sites(records, (0, 0, n), world[0], 5, gpu, first_offset=first)) == U.full(want)


def test_random_batch_in_windows_of_4096(gpu, world, random_case):
    records, want = random_case
    for c, seq in enumerate(world):
        n = len(seq)
        assert len(want[c]) > 100
        assert U.full(device_sites(records, (c, 0, n), seq, gpu=gpu)) == U.full(want[c])
        for start in range(0, n, 4096):   # records straddle the windows and are clipped to each
            length = min(4096, n - start)
            assert U.full(device_sites(records, (c, start, length), seq, gpu=gpu)) == clipped(want[c], start, length)
    other = U.random_batch(world, seed=12, n=600)
    for c, seq in enumerate(world):
        assert U.full(device_sites(other, (c, 0, len(seq)), seq, 0, gpu, first_offset=1)) == U.full(
            U.sites(other, (c, 0, len(seq)), seq, TAB, 0)[0])


def to_dev(torch, dev, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(SIGNED.get(a.dtype, a.dtype)).copy()).to(dev)


def dev_batch(torch, dev, records, **kw):
    arrays = fcship.ug_arrays(*U.flatten(records))
    t = [to_dev(torch, dev, a) for a in arrays]
    flag, ref_id, pos, mapq, cigar, cigar_off, bases, qual, base_off, absent = [x.data_ptr() for x in t]
    return t, fcship.UgBatch(kw.get("n", len(records)), flag, ref_id, pos, mapq, cigar, cigar_off,
                             kw.get("n_cigar", len(arrays[4])), bases, qual, base_off, len(arrays[7]), absent)


class Twin:
    """fcsug_sites_dev on a caller stream with device-resident inputs."""

    def __init__(self, torch, gpu):
        self.torch, self.gpu = torch, gpu
        self.dev = torch.device(f"cuda:{gpu}")
        self.stream = torch.cuda.Stream(device=self.dev)
        with torch.cuda.stream(self.stream):
            self.table = to_dev(torch, self.dev, np.array(TAB, np.int64))
        self.keep = []

    def queue(self, records, window, refseq, max_sites=None, min_baseq=17, **kw):
        """Queues one call; returns (sites tensor, n_sites tensor, status tensor) to read after the stream's end."""
        torch = self.torch
        ref, start, length = window
        max_sites = length if max_sites is None else max_sites
        with torch.cuda.stream(self.stream):
            keep, b = dev_batch(torch, self.dev, records, **kw)
            seq = to_dev(torch, self.dev, np.frombuffer(refseq[start:start + length].encode(), np.uint8))
            sites = torch.full((80 * max(max_sites, 1),), 0x55, dtype=torch.uint8, device=self.dev)
            n = torch.full((1,), -7, dtype=torch.int64, device=self.dev)
            status = torch.zeros(1, dtype=torch.int32, device=self.dev)
            need = fcship.lib.fcsug_workspace_bytes(len(records), length)
            ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
            w, p = fcship.UgWindow(ref, 0, start, length, len(refseq)), fcship.UgParams(min_baseq)
            fcship.check(fcship.lib.fcsug_sites_dev(self.gpu, C.addressof(b), C.addressof(p), C.addressof(w), seq.data_ptr(),
                                                    self.table.data_ptr(), sites.data_ptr(), max_sites, n.data_ptr(),
                                                    ws.data_ptr(), need, status.data_ptr(), C.c_void_p(self.stream.cuda_stream)))
        self.keep.append((keep, seq, ws))
        return sites, n, status

    @staticmethod
    def read(out, written=None):
        sites, n, status = out
        n = int(n.cpu()[0])
        rows = sites.cpu().numpy().view(fcship.UG_SITE)
        return rows[:n if written is None else written], n, int(status.cpu()[0])


def test_dev_twin_on_a_caller_stream(gpu, world, random_case):
    import torch
    records, want = random_case
    twin = Twin(torch, gpu)
    n = len(world[0])
    good = twin.queue(records, (0, 0, n), world[0])
    window = twin.queue(records, (1, 4096, 2904), world[1])
    # a record one past its contig's end sets the status bit and is otherwise clipped
    case = next(c for c in CASES if c["name"] == "ends_one_past_contig_end")
    past = twin.queue(case["records"], case["window"], REFS[1])
    # a cigar_off beyond n_cigar is clamped and reported, and its record adds nothing
    two = [U.rec(0, 0, 10, "10M", U.read_of(REFS[0], 10, "10M", {2: "C"})),
           U.rec(0, 0, 30, "5M2I3M", U.read_of(REFS[0], 30, "5M2I3M", {2: "C"}))]
    field = twin.queue(two, (0, 0, 300), REFS[0], n_cigar=2)           # the second record's words end at 4
    # decreasing positions: no site
    order = twin.queue([two[1], two[0]], (0, 0, 300), REFS[0])
    # every locus of three tiles is a site: exactly enough room, and one too few
    enough = twin.queue(all_sites_batch(), (0, 3, 3 * T), CLEAN, max_sites=3 * T)
    short = twin.queue(all_sites_batch(), (0, 3, 3 * T), CLEAN, max_sites=3 * T - 1)
    empty = twin.queue([], (0, 0, 300), REFS[0])
    twin.stream.synchronize()
    rows, found, status = Twin.read(good)
    assert status == 0 and found == len(want[0]) and U.full(rows) == U.full(want[0])
    assert U.full(rows) == U.full(device_sites(records, (0, 0, n), world[0], gpu=gpu))
    rows, found, status = Twin.read(window)
    assert status == 0 and U.full(rows) == clipped(want[1], 4096, 2904)
    rows, found, status = Twin.read(past)
    assert status == fcship.FCSUG_STATUS_REF and U.brief(rows) == U.want_sites(case)
    rows, found, status = Twin.read(field)
    assert status == fcship.FCSUG_STATUS_FIELD and U.full(rows) == U.full(U.sites(two[:1], (0, 0, 300), REFS[0], TAB)[0])
    assert found == 1
    rows, found, status = Twin.read(order)
    assert status == fcship.FCSUG_STATUS_ORDER and found == 0
    assert (order[0].cpu().numpy() == 0x55).all()
    all_want = U.full(U.sites(all_sites_batch(), (0, 3, 3 * T), CLEAN, TAB)[0])
    rows, found, status = Twin.read(enough)
    assert status == 0 and found == 3 * T and U.full(rows) == all_want
    rows, found, status = Twin.read(short, written=3 * T - 1)
    assert status == fcship.FCSUG_STATUS_SITES and found == 3 * T and U.full(rows) == all_want[:-1]
    rows, found, status = Twin.read(empty)
    assert status == 0 and found == 0


def test_two_threads_each_on_their_own_session(gpu, world):
    n = len(world[0])
    batches = [U.random_batch(world, seed=100 + k, n=300 + 50 * k) for k in range(2)]
    want = [U.full(U.sites(b, (0, 0, n), world[0], TAB)[0]) for b in batches]
    got, errors = [None] * 2, []

    def work(k):
        try:
            for _ in range(3):
                got[k] = U.full(device_sites(batches[k], (0, 0, n), world[0], gpu=gpu))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert got[0] == want[0] and got[1] == want[1]


def test_bad_arguments_write_nothing(gpu):
    records = [U.rec(0, 0, 10 * k, "10M", U.read_of(REFS[0], 10 * k, "10M", {3: "A" if k != 1 else "C"})) for k in range(4)]
    a = U.flatten(records)
    bad = a[:8] + ([0, 10, 9, 30, 40],) + a[9:]
    with pytest.raises(fcship.FcsError, match="base offsets out of order at record 1"):
        fcship.ug_sites(bad, (0, 0, 300, 1200), REFS[0][:300], TAB, device=gpu)
    with pytest.raises(fcship.FcsError):
        fcship.ug_sites(a, (0, 0, 300, 1200), REFS[0][:300], TAB, device=99)
    got = fcship.ug_sites(a, (0, 0, 300, 1200), REFS[0][:300], TAB, device=gpu)
    assert U.full(got) == U.full(U.sites(records, (0, 0, 300), REFS[0], TAB)[0]) and len(got) >= 3


def test_ug_command_gpu_and_host_write_identical_files(gpu, tmp_path):
    d = tmp_path / "s"
    p = H.run_cli("synth", "-o", d, "-c", "chr1:150000,chr2:50000", "-x", "6", "--seed", "8", "--no-fastq")
    assert p.returncode == 0, p.stderr[-2000:]
    logs = {}
    for mode in ("true", "false"):
        p = H.run_cli("ug", "-r", d / "ref.fasta", "-i", d / "sample.bam", "-o", tmp_path / f"{mode}.vcf",
                      env={"FCS_UG_GPU": mode, "FCS_GPU_DEVICES": str(gpu), "FCS_UG_CHUNK_RECORDS": "3000",
                           "FCS_UG_WINDOW_BP": "65536"}, cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-2000:]
        logs[mode] = p.stderr
    assert "(GPU)" in logs["true"] and "(host)" in logs["false"]
    for s in ("", ".gz", ".gz.tbi"):
        assert (tmp_path / f"true.vcf{s}").read_bytes() == (tmp_path / f"false.vcf{s}").read_bytes(), s
    calls = [ln for ln in (tmp_path / "true.vcf").read_text().splitlines() if not ln.startswith("#")]
    assert len(calls) >= 1 and "4 windows" in logs["true"]


def test_ug_command_streams_a_part_directory_gpu_and_host_identical(gpu, tmp_path):
    """Chunks of 128 records, a file boundary and windows of 1,024 loci all fall inside the data (bam_stream_cases)."""
    ref, parts, n = S.part_directory(tmp_path)
    logs = {}
    for mode in ("false", "true"):
        p = H.run_cli("ug", "-r", ref, "-i", parts, "-o", tmp_path / f"{mode}.vcf",
                      env={"FCS_UG_GPU": mode, "FCS_GPU_DEVICES": str(gpu), "FCS_UG_CHUNK_RECORDS": "128",
                           "FCS_UG_WINDOW_BP": str(S.WINDOW_BP)}, cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-2000:]
        logs[mode] = p.stderr.rstrip("\n").split("\n")[-1]
    assert "(host)" in logs["false"] and "(GPU)" in logs["true"]
    assert f": {n} records, 2 intervals, 12 windows, " in logs["true"], logs["true"]
    for s in ("", ".gz", ".gz.tbi"):
        assert (tmp_path / f"true.vcf{s}").read_bytes() == (tmp_path / f"false.vcf{s}").read_bytes(), s
    assert int(logs["true"].split(" sites, ")[1].split(" calls")[0]) > 0
