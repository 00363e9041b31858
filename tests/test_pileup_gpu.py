"""GPU: the callers' pileup (fcspu_pile and its _dev twin) equals
the Python restatement of the rules (tests/pu_cases.py) exactly, the doubles bit
for bit; htc and mutect2 write the same files with htc.gpu_pileup on and off."""
import ctypes as C
import re
import threading

import numpy as np
import pytest

import fcship
import host_lib as H
import pu_cases as P
import ug_cases as U

pytestmark = pytest.mark.gpu
CASES = P.hand_cases()
REFS = U.hand_refs()
TAB = fcship.pu_table()
TABLE = TAB.tolist()
T = fcship.FCSPU_TILE
SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
CLEAN = "".join(U.LETTERS[p % 4] for p in range(4 * T))   # a contig without N


def device_pile(batches, window, refseq, gpu=0, first_offset=0, **kw):
    ref, start, length = window
    return fcship.pu_pile([U.flatten(b, first_offset) for b in batches], (ref, start, length, len(refseq)),
                          refseq[start:start + length], TAB, device=gpu, **kw)


@pytest.fixture(scope="module")
def world():
    return P.random_world()


@pytest.fixture(scope="module")
def random_case(world):
    """(records, per contig the per-op events and the restatement's results with them), computed once."""
    records = P.random_batch(world)
    ops = [P.op_events(records, (c, 0, len(s)), s) for c, s in enumerate(world)]
    return records, ops, [P.pile([records], (c, 0, len(s)), s, TABLE, events_in=ops[c]) for c, s in enumerate(world)]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_case(gpu, case):
    refseq = REFS[case["window"][0]]
    ops = P.sparse(case["window"][2], case["ops"])
    got = device_pile(case["batches"], case["window"], refseq, gpu, frac=case["frac"], events_in=ops)
    assert P.same(got, P.want_of(case))
    assert P.same(got, P.pile(case["batches"], case["window"], refseq, TABLE, frac=case["frac"], events_in=ops))


def test_all_hand_cases_as_one_batch_and_the_smallest_batches(gpu):
    records = sorted((r for c in CASES for b in c["batches"] for r in b), key=lambda r: (r["ref"], r["pos"]))
    whole = P.pile([records], (0, 0, 1200), REFS[0], TABLE)
    assert len(whole["sites"]) >= 8 and len(whole["snvs"]) >= 10
    for start, length in ((0, 1200), (100, 50), (12, 1), (63, 2), (64, 1)):
        assert P.same(device_pile([records], (0, start, length), REFS[0], gpu), P.cut(whole, start, length)), (start, length)
    assert P.same(device_pile([records], (1, 0, 40), REFS[1], gpu), P.pile([records], (1, 0, 40), REFS[1], TABLE))
    empty = device_pile([[]], (0, 0, 300), REFS[0], gpu)
    assert not empty["depth"].any() and not empty["events"].any() and not empty["gl"].any()
    assert len(empty["sites"]) == 0 and len(empty["snvs"]) == 0
    none = device_pile([records], (0, 5, 0), REFS[0], gpu)
    assert len(none["sites"]) == 0 and len(none["snvs"]) == 0 and len(none["depth"]) == 0


@pytest.mark.parametrize("start", [0, 1, 63])
def test_windows_of_every_length_around_a_wave_and_a_tile(gpu, world, random_case, start):
    records, ops, want = random_case
    for length in (1, 63, 64, 65, 3 * T + 5):
        for c in (0, 2):
            for want_gl in (True, False):
                got = device_pile([records], (c, start, length), world[c], gpu, want_gl=want_gl,
                                  events_in=ops[c][start:start + length])
                assert got["gl"] is None or want_gl
                assert P.same(got, P.cut(want[c], start, length), gl=want_gl), (c, start, length, want_gl)
    assert len(P.cut(want[0], start, 3 * T + 5)["sites"]) > 3


def test_whole_contigs_and_both_orders_of_equal_positions(gpu, world, random_case):
    records, ops, want = random_case
    for c, seq in enumerate(world):
        assert P.same(device_pile([records], (c, 0, len(seq)), seq, gpu, events_in=ops[c]), want[c])
    flipped = P.reversed_ties(records)
    window = (0, 0, len(world[0]))
    a, b = P.pile([records], window, world[0], TABLE), P.pile([flipped], window, world[0], TABLE)
    assert np.any(a["gl"].view(np.uint64) != b["gl"].view(np.uint64))      # (test_pileup_cpu.py asserts it too)
    assert P.same(device_pile([records], window, world[0], gpu), a)
    assert P.same(device_pile([flipped], window, world[0], gpu), b)        # the sums follow the order given


def test_a_record_with_a_100_kbp_skip_over_2000_records(gpu):
    n = 100_100
    seq = "".join(U.LETTERS[(p * 7 + p // 5) % 4] for p in range(n))
    long = U.rec(0, 0, 10, "10M100000N10M", U.read_of(seq, 10, "10M100000N10M", {3: U.other(seq[13]), 15: U.other(seq[100025])}))
    under = []
    for k in range(2000):
        pos = 30 + 49 * k
        under.append(U.rec(0, 0, pos, "40M", U.read_of(seq, pos, "40M", {k % 40: U.other(seq[pos + k % 40], 1 + k % 3)})))
    records = [long] + under
    want = P.pile([records, [long, long]], (0, 0, n), seq, TABLE)
    assert want["depth"][13] == 3 and want["depth"][100025] == 3 and (100025, U.other(seq[100025]), 3) in want["snvs"]
    assert P.same(device_pile([records, [long, long]], (0, 0, n), seq, gpu), want)


def test_70000_copies_are_exact(gpu):
    seq = "".join(U.other(ch) for ch in CLEAN[10:13])
    records = [U.rec(0, 0, 10, "3M", seq, qual=[30, 41, 7])] * 70000
    got = device_pile([records], (0, 0, 64), CLEAN, gpu, min_bq=5)
    assert got["depth"][10:13].tolist() == [70000] * 3 and got["events"][10:13].tolist() == [70000] * 3
    assert got["depth"].sum() == 210000 and got["sites"].tolist() == [10, 11, 12]
    assert [(int(v["offset"]), chr(v["alt"]), int(v["count"])) for v in got["snvs"]] == [(10 + i, seq[i], 70000) for i in range(3)]
    for i, q in enumerate((30, 41, 7)):   # 70,000 sequential adds, not a product
        for slot, col in ((0, 2), (1, 1), (2, 0)):
            want = np.add.accumulate(np.full(70000, TAB[q][col], np.float64))[-1]
            assert got["gl"][10 + i][slot].tobytes() == want.tobytes(), (i, slot)
    assert np.add.accumulate(np.full(70000, TAB[30][2]))[-1] != 70000 * TAB[30][2]


def all_sites_batch():
    """Four layers of 64-base records over loci [3, 3 + 3 T) of CLEAN: two layers carry one non-reference letter at
    every base, two another."""
    out = []
    for p in range(3, 3 + 3 * T, 64):
        for k in (1, 1, 2, 2):
            out.append(U.rec(0, 0, p, "64M", "".join(U.other(ch, k) for ch in CLEAN[p:p + 64])))
    return out


def test_every_locus_of_three_tiles_is_a_site_with_two_snvs(gpu):
    records, window = all_sites_batch(), (0, 3, 3 * T)
    want = P.pile([records], window, CLEAN, TABLE)
    assert want["sites"] == list(range(3 * T)) and len(want["snvs"]) == 6 * T
    assert P.same(device_pile([records], window, CLEAN, gpu, max_sites=3 * T, max_snvs=6 * T), want)      # exactly enough
    with pytest.raises(fcship.FcsError, match=f"{3 * T} sites and {6 * T} SNVs, max_sites is {3 * T - 1} and max_snvs {6 * T}"):
        device_pile([records], window, CLEAN, gpu, max_sites=3 * T - 1, max_snvs=6 * T)
    with pytest.raises(fcship.FcsError, match=f"{3 * T} sites and {6 * T} SNVs, max_sites is {3 * T} and max_snvs {6 * T - 1}"):
        device_pile([records], window, CLEAN, gpu, max_sites=3 * T, max_snvs=6 * T - 1)


@pytest.mark.parametrize("first", [0, 1, 3])
def test_batches_at_every_first_offset(gpu, world, first):
    records, n = U.sweep_batch(world), len(world[0])
    want = P.pile([records], (0, 0, n), world[0], TABLE, min_bq=5)
    assert len(want["snvs"]) > 0 and want["events"].sum() > 1000
    assert P.same(device_pile([records], (0, 0, n), world[0], gpu, first_offset=first, min_bq=5), want)


def test_two_batches_and_sites_from_batch_0_alone(gpu, world, random_case):
    records, ops, _ = random_case
    other = P.random_batch(world, seed=12, n=600)
    for c in (0, 1):
        window = (c, 0, len(world[c]))
        want = P.pile([records, other], window, world[c], TABLE, frac=0.10, events_in=ops[c])
        alone = P.pile([records], window, world[c], TABLE, frac=0.10, events_in=ops[c])
        assert want["sites"] == alone["sites"] and len(want["snvs"]) > len(alone["snvs"])
        assert np.array_equal(want["gl"].view(np.uint64), alone["gl"].view(np.uint64))
        assert P.same(device_pile([records, other], window, world[c], gpu, first_offset=1, frac=0.10, events_in=ops[c]), want)
    swapped = P.pile([other, records], (0, 0, len(world[0])), world[0], TABLE)
    assert P.same(device_pile([other, records], (0, 0, len(world[0])), world[0], gpu), swapped)


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
    """fcspu_pile_dev on a caller stream with device-resident inputs."""

    def __init__(self, torch, gpu):
        self.torch, self.gpu = torch, gpu
        self.dev = torch.device(f"cuda:{gpu}")
        self.stream = torch.cuda.Stream(device=self.dev)
        with torch.cuda.stream(self.stream):
            self.table = to_dev(torch, self.dev, TAB)
        self.keep = []

    def queue(self, batches, window, refseq, max_sites=None, max_snvs=None, events_in=None, kw=None):
        """Queues one call; returns the output tensors to read after the stream's end."""
        torch = self.torch
        ref, start, length = window
        max_sites = length if max_sites is None else max_sites
        max_snvs = 4 * length if max_snvs is None else max_snvs
        kw = kw or [{}] * len(batches)
        with torch.cuda.stream(self.stream):
            staged = [dev_batch(torch, self.dev, b, **k) for b, k in zip(batches, kw)]
            arr = (fcship.UgBatch * len(batches))(*[b for _, b in staged])
            seq = to_dev(torch, self.dev, np.frombuffer(refseq[start:start + length].encode(), np.uint8))
            ev = None if events_in is None else to_dev(torch, self.dev, np.asarray(events_in, np.int32))
            o = dict(depth=torch.full((max(length, 1),), -5, dtype=torch.int32, device=self.dev),
                     events=torch.full((max(length, 1),), -5, dtype=torch.int32, device=self.dev),
                     gl=torch.full((3 * max(length, 1),), 7.0, dtype=torch.float64, device=self.dev),
                     sites=torch.full((max(max_sites, 1) + 1,), -5, dtype=torch.int32, device=self.dev),
                     snvs=torch.full((12 * (max(max_snvs, 1) + 1),), 0x55, dtype=torch.uint8, device=self.dev),
                     counts=torch.full((2,), -7, dtype=torch.int64, device=self.dev),
                     status=torch.zeros(1, dtype=torch.int32, device=self.dev))
            out = fcship.PuOut(o["depth"].data_ptr(), o["events"].data_ptr(), o["gl"].data_ptr(), o["sites"].data_ptr(), max_sites,
                               o["counts"].data_ptr(), o["snvs"].data_ptr(), max_snvs, o["counts"].data_ptr() + 8)
            need = fcship.pu_workspace_bytes([len(b) for b in batches], length)
            ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
            w, p = fcship.UgWindow(ref, 0, start, length, len(refseq)), fcship.PuParams(P.MIN_BQ, 1, P.FRAC)
            fcship.check(fcship.lib.fcspu_pile_dev(self.gpu, C.addressof(arr), len(batches), C.addressof(p), C.addressof(w),
                                                   seq.data_ptr(), self.table.data_ptr(), 0 if ev is None else ev.data_ptr(),
                                                   C.addressof(out), ws.data_ptr(), need, o["status"].data_ptr(),
                                                   C.c_void_p(self.stream.cuda_stream)))
        self.keep.append((staged, seq, ev, ws))
        o["length"], o["max_sites"], o["max_snvs"] = length, max_sites, max_snvs
        return o

    @staticmethod
    def read(o):
        """(the results as pu_pile's dict, cut to what was written; n_sites, n_snvs, status; the guard slots)."""
        ns, nv = (int(x) for x in o["counts"].cpu())
        length = o["length"]
        sites, snvs = o["sites"].cpu().numpy(), o["snvs"].cpu().numpy().view(fcship.PU_SNV)
        res = dict(depth=o["depth"].cpu().numpy()[:length], events=o["events"].cpu().numpy()[:length],
                   gl=o["gl"].cpu().numpy()[:3 * length].reshape(length, 3), sites=sites[:min(ns, o["max_sites"])],
                   snvs=snvs[:min(nv, o["max_snvs"])])
        untouched = bool(sites[o["max_sites"]] == -5 and snvs[o["max_snvs"]].tobytes() == b"\x55" * 12)
        return res, ns, nv, int(o["status"].cpu()[0]), untouched


def test_dev_twin_on_a_caller_stream(gpu, world, random_case):
    import torch
    records, ops, want = random_case
    twin = Twin(torch, gpu)
    n = len(world[0])
    good = twin.queue([records], (0, 0, n), world[0], events_in=ops[0])
    window = twin.queue([records], (1, 4096, 1900), world[1], events_in=ops[1][4096:4096 + 1900])
    # a record one past its contig's end sets the status bit; its base beyond the contig is not counted
    past_rec = [P.read(REFS, 31, "10M", {31: "A"}, contig=1)] * 2
    past = twin.queue([past_rec], (1, 0, 40), REFS[1])
    # a cigar_off beyond n_cigar is clamped and reported, and its record adds nothing
    two = [P.read(REFS, 10, "10M", {12: "C"}), P.read(REFS, 30, "5M2I3M", {32: "C"})]
    field = twin.queue([two], (0, 0, 300), REFS[0], kw=[dict(n_cigar=2)])    # the second record's words end at 4
    # decreasing positions: nothing is written
    order = twin.queue([[two[1], two[0]]], (0, 0, 300), REFS[0])
    # a read letter the device does not count
    iupac = [P.read(REFS, 10, "10M", {12: "M"}), P.read(REFS, 10, "10M", {12: "C", 13: "G"})]
    letter = twin.queue([iupac], (0, 0, 300), REFS[0])
    # every locus of three tiles is a site with two SNVs: exactly enough room, and one too few of each
    full = all_sites_batch()
    enough = twin.queue([full], (0, 3, 3 * T), CLEAN, max_sites=3 * T, max_snvs=6 * T)
    short = twin.queue([full], (0, 3, 3 * T), CLEAN, max_sites=3 * T - 1, max_snvs=6 * T - 1)
    empty = twin.queue([[]], (0, 0, 300), REFS[0])
    twin.stream.synchronize()

    res, ns, nv, status, untouched = Twin.read(good)
    assert status == 0 and untouched and ns == len(want[0]["sites"]) and nv == len(want[0]["snvs"]) and P.same(res, want[0])
    assert P.same(device_pile([records], (0, 0, n), world[0], gpu, events_in=ops[0]), want[0])
    res, ns, nv, status, untouched = Twin.read(window)
    assert status == 0 and untouched and P.same(res, P.cut(want[1], 4096, 1900))
    res, ns, nv, status, _ = Twin.read(past)
    assert status == fcship.FCSPU_STATUS_REF and P.same(res, P.pile([past_rec], (1, 0, 40), REFS[1], TABLE))
    assert res["depth"][31:40].tolist() == [2] * 9 and res["sites"].tolist() == [31]
    res, ns, nv, status, _ = Twin.read(field)
    assert status == fcship.FCSPU_STATUS_FIELD and P.same(res, P.pile([two[:1]], (0, 0, 300), REFS[0], TABLE))
    res, ns, nv, status, _ = Twin.read(order)
    assert status == fcship.FCSPU_STATUS_ORDER and ns == 0 and nv == 0
    assert (order["depth"].cpu().numpy() == -5).all() and (order["gl"].cpu().numpy() == 7.0).all()
    assert (order["sites"].cpu().numpy() == -5).all() and (order["snvs"].cpu().numpy() == 0x55).all()
    res, ns, nv, status, _ = Twin.read(letter)
    counted = [P.read(REFS, 10, "10M", qual=[30, 30, 0] + [30] * 7), iupac[1]]     # the letter M is not counted at all
    assert status == fcship.FCSPU_STATUS_LETTER and P.same(res, P.pile([counted], (0, 0, 300), REFS[0], TABLE))
    all_want = P.pile([full], (0, 3, 3 * T), CLEAN, TABLE)
    res, ns, nv, status, untouched = Twin.read(enough)
    assert status == 0 and untouched and (ns, nv) == (3 * T, 6 * T) and P.same(res, all_want)
    res, ns, nv, status, untouched = Twin.read(short)
    assert status == fcship.FCSPU_STATUS_SITES | fcship.FCSPU_STATUS_SNVS and (ns, nv) == (3 * T, 6 * T) and untouched
    assert P.same(res, dict(all_want, sites=all_want["sites"][:-1], snvs=all_want["snvs"][:-1]))
    res, ns, nv, status, _ = Twin.read(empty)
    assert status == 0 and (ns, nv) == (0, 0) and not res["depth"].any() and not res["gl"].any()


def test_a_read_letter_m_is_refused_with_its_record(gpu):
    records = [P.read(REFS, 10, "10M"), P.read(REFS, 12, "10M", {14: "M"}), P.read(REFS, 12, "10M", {15: "M"})]
    with pytest.raises(fcship.FcsError, match="record 1 of batch 0 has a counted read letter other than A C G T N"):
        device_pile([records], (0, 0, 300), REFS[0], gpu)
    with pytest.raises(fcship.FcsError, match="record 2 of batch 1 has a counted read letter"):
        device_pile([records[:1], [records[0], records[0], records[2]]], (0, 0, 300), REFS[0], gpu)
    # below min_bq, or outside the window, the letter is not looked at
    low = [P.read(REFS, 12, "10M", {14: "M"}, qual=[30, 30, 9] + [30] * 7)]
    assert P.same(device_pile([low], (0, 0, 300), REFS[0], gpu), P.pile([low], (0, 0, 300), REFS[0], TABLE))
    assert P.same(device_pile([records], (0, 16, 100), REFS[0], gpu), P.pile([records], (0, 16, 100), REFS[0], TABLE))


def test_two_threads_each_on_their_own_session(gpu, world):
    n = len(world[0])
    batches = [P.random_batch(world, seed=100 + k, n=300 + 50 * k) for k in range(2)]
    want = [P.pile([b], (0, 0, n), world[0], TABLE) for b in batches]
    got, errors = [None] * 2, []

    def work(k):
        try:
            for _ in range(3):
                got[k] = device_pile([batches[k]], (0, 0, n), world[0], gpu)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert P.same(got[0], want[0]) and P.same(got[1], want[1])


def test_bad_arguments_write_nothing(gpu):
    records = [P.read(REFS, 10 * k, "10M", {10 * k + 3: U.other(REFS[0][10 * k + 3])}) for k in range(4)] * 2
    records.sort(key=lambda r: r["pos"])
    a = U.flatten(records)
    window, ref = (0, 0, 300, 1200), REFS[0][:300]

    def refused(match, batches=(a,), window=window, **kw):
        o, arrays = fcship.pu_out(300)
        keep = [fcship.ug_arrays(*b) for b in batches]
        arr = (fcship.UgBatch * max(len(keep), 1))(*[fcship.ug_batch(x) for x in keep])
        w, p = fcship.UgWindow(window[0], 0, *window[1:]), fcship.PuParams(10, 1, kw.get("frac", 0.15))
        seq = np.frombuffer(ref.encode(), np.uint8)
        rc = fcship.lib.fcspu_pile(kw.get("device", gpu), C.addressof(arr), kw.get("n", len(keep)), C.addressof(p), C.addressof(w),
                                   seq.ctypes.data, TAB.ctypes.data, 0, C.addressof(o))
        assert rc != 0 and re.search(match, fcship.lib.fcs_last_error().decode()), fcship.lib.fcs_last_error()
        assert (arrays["depth"] == -1).all() and (arrays["events"] == -1).all() and np.isnan(arrays["gl"]).all()
        assert (arrays["sites"] == -1).all() and arrays["n_sites"][0] == -7 and arrays["n_snvs"][0] == -7

    refused("base offsets out of order at record 1", batches=(a[:8] + ([0, 10, 9, 30, 40, 50, 60, 70, 80],) + a[9:],))
    refused("positions decrease", batches=(U.flatten(records[::-1]),))
    refused("3 batches", n=3)
    refused("0 batches", n=0)
    refused("lies outside its contig", window=(0, 1000, 300, 1200))
    refused("frac", frac=-1.0)
    refused("", device=99)
    got = fcship.pu_pile([a], window, ref, TAB, device=gpu)
    assert P.same(got, P.pile([records], (0, 0, 300), REFS[0], TABLE)) and len(got["sites"]) == 4


# ------------------------------------------------------------------ the commands
@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    d = tmp_path_factory.mktemp("pu")
    p = H.run_cli("synth", "-o", d, "-c", "chr1:150000,chr2:50000", "-x", "6", "--seed", "8", "--no-fastq", "--tumor")
    assert p.returncode == 0, p.stderr[-2000:]
    return d


def run_both(args, name, gpu, tmp_path):
    """The command with htc.gpu_pileup on and off: identical files; (the text, GPU chunks, host chunks of the run with it on)."""
    chunks = {}
    for mode in ("true", "false"):
        env = {"FCS_HTC_GPU_PILEUP": mode, "FCS_HTC_PILEUP_CHUNK_BP": "4096", "FCS_GATK_NCONTIGS": "6", "FCS_GPU_DEVICES": str(gpu),
               "FCS_LOG_DIR": str(tmp_path / f"log_{mode}_{name}")}
        p = H.run_cli(*args, "-o", tmp_path / f"{mode}_{name}", env=env, cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-3000:]
        text = p.stderr
        for f in sorted((tmp_path / f"log_{mode}_{name}").rglob("*")):
            if f.is_file():
                text += f.read_text(errors="replace")
        found = re.findall(r"shard \d+ pileup: (\d+) gpu chunks, (\d+) host chunks, device ", text)
        chunks[mode] = (sum(int(a) for a, _ in found), sum(int(b) for _, b in found), len(found))
    assert chunks["true"][0] > 0 and chunks["true"][2] == 6 and chunks["false"] == (0, 0, 0), chunks
    for s in ("", ".gz", ".gz.tbi"):
        assert (tmp_path / f"true_{name}{s}").read_bytes() == (tmp_path / f"false_{name}{s}").read_bytes(), s
    return (tmp_path / f"true_{name}").read_text(), chunks["true"]


def test_htc_gvcf_and_vcf_write_identical_files(gpu, synth, tmp_path):
    base = ["htc", "-f", "-r", synth / "ref.fasta", "-i", synth / "sample.bam"]
    text, chunks = run_both(base, "g.vcf", gpu, tmp_path)
    lines = [ln for ln in text.splitlines() if not ln.startswith("#")]
    assert sum("END=" not in ln for ln in lines) >= 1 and sum("<NON_REF>\t.\t.\tEND=" in ln for ln in lines) >= 1
    assert chunks[0] >= 40 and chunks[1] == 0    # 200 kbp in chunks of 4,096 loci: records straddle them
    text, _ = run_both(base + ["-v"], "v.vcf", gpu, tmp_path)
    assert sum(not ln.startswith("#") for ln in text.splitlines()) >= 1


def test_mutect2_writes_identical_files(gpu, synth, tmp_path):
    text, chunks = run_both(["mutect2", "-f", "-r", synth / "ref.fasta", "-n", synth / "sample.bam", "-t", synth / "tumor.bam"],
                            "m.vcf", gpu, tmp_path)
    assert sum(not ln.startswith("#") for ln in text.splitlines()) >= 1 and chunks[1] == 0


def test_a_read_with_an_iupac_letter_sends_its_chunk_down_the_host_path(gpu, synth, tmp_path):
    H.lib.fcsg_bam_to_text.argtypes = [C.c_char_p] * 2
    H.lib.fcsg_text_to_bam.argtypes = [C.c_char_p] * 4
    H.check(H.lib.fcsg_bam_to_text(str(synth / "sample.bam").encode(), str(tmp_path / "in.txt").encode()))
    rows = [ln.split("\t")[:8] for ln in (tmp_path / "in.txt").read_text().splitlines() if not ln.startswith("@")]
    k = next(i for i, f in enumerate(rows) if f[2] == "0" and int(f[3]) > 20000 and set(f[5]) <= set("0123456789M"))
    rows[k][6] = rows[k][6][:70] + "R" + rows[k][6][71:]
    (tmp_path / "out.txt").write_text("".join("\t".join(f) + "\n" for f in rows))
    bam = tmp_path / "iupac.bam"
    H.check(H.lib.fcsg_text_to_bam(str(tmp_path / "out.txt").encode(), str(bam).encode(), b"chr1,chr2", b"150000,50000"))
    H.check(H.lib.fcsg_bam_index(str(bam).encode()))
    assert any("R" in r["seq"] for r in H.read_bam(bam)[2])
    _, chunks = run_both(["htc", "-f", "-r", synth / "ref.fasta", "-i", bam], "i.vcf", gpu, tmp_path)
    assert chunks[1] >= 1 and chunks[0] > chunks[1]
