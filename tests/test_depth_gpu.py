"""GPU: depth of coverage (fcsdp_count / fcsdp_stats and their _dev twins,
DESIGN §4.11) equals the Python restatement of the rules
(tests/depth_cases.py) exactly."""
import ctypes as C
import threading

import numpy as np
import pytest

import bam_stream_cases as S
import depth_cases as D
import fcship
import host_lib as H

pytestmark = pytest.mark.gpu
CASES = D.hand_cases()
SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def device_depth(records, window, contig_len, prm=None, gpu=0, first_offset=0, depth=None):
    ref, start, length = window
    return fcship.dp_count(D.flatten(records, first_offset), (ref, start, length, contig_len),
                           fcship.dp_params(**(prm or D.params())), depth, device=gpu)


def device_stats(d, part, pieces, n_long=0, gpu=0, bits=None, **kw):
    hist, long_hist, summary = fcship.dp_stats(d, D.bitmap(part) if bits is None else bits, pieces, n_long, device=gpu, **kw)
    return hist, long_hist, [{k: int(s[k]) for k in ("total", "loci", "above", "q1", "median", "q3")} for s in summary]


@pytest.fixture(scope="module")
def world():
    return D.random_world()


@pytest.fixture(scope="module")
def random_case(world):
    """(records, params, the restatement's depths per contig) of the random batch, computed once."""
    records, prm = D.random_batch(world), D.params(1, 254, 2, 40, True)
    return records, prm, [D.depth(records, (c, 0, len(s)), len(s), prm)[0] for c, s in enumerate(world)]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_case(gpu, case):
    clen = D.LENS[case["window"][0]]
    if case["beyond"]:   # the host-pointer call refuses the record; the _dev twin clips it (below)
        got = np.full(case["window"][2], 7, np.uint32)
        with pytest.raises(fcship.FcsError, match="aligned base beyond its contig"):
            device_depth(case["records"], case["window"], clen, case["prm"], gpu, depth=got)
        assert (got == 7).all()
        return
    assert (device_depth(case["records"], case["window"], clen, case["prm"], gpu) == D.want_depths(case)).all()


def test_all_hand_cases_as_one_batch_and_the_smallest_batches(gpu):
    records = [r for c in CASES for r in c["records"]]
    for prm in (D.params(), D.params(20, 40, 10, 30, True)):
        for window in ((0, 0, 300), (0, 100, 50), (0, 119, 1)):
            assert (device_depth(records, window, 300, prm, gpu) == D.depth(records, window, 300, prm)[0]).all()
    assert not device_depth([], (0, 0, 300), 300, gpu=gpu).any()
    d = device_depth([D.rec(0, 0, 299, "1M")], (0, 0, 300), 300, gpu=gpu)
    assert d[299] == 1 and d.sum() == 1
    assert len(device_depth([D.rec(0, 0, 299, "1M")], (0, 5, 0), 300, gpu=gpu)) == 0


@pytest.mark.parametrize("first", [0, 1, 3])
def test_sweep_batch_at_every_quality_offset_residue(gpu, world, first):
    records, prm, n = D.sweep_batch(world), D.params(min_baseq=5, max_baseq=35), len(world[0])
    assert {r["n_bases"] for r in records} == set(range(1, 201))
    assert (device_depth(records, (0, 0, n), n, prm, gpu, first_offset=first) == D.depth(records, (0, 0, n), n, prm)[0]).all()


def test_copies_reach_499_500_501_and_70000_copies_are_exact(gpu, world):
    n = len(world[0])
    want = D.depth(D.copies_batch(), (0, 0, n), n)[0]
    got = device_depth(D.copies_batch(), (0, 0, n), n, gpu=gpu)
    assert (got == want).all() and {499, 500, 501} <= set(int(v) for v in got)
    part = [True] * n
    hist, _, summary = device_stats(got, part, [(0, n, -1)], gpu=gpu)
    whist, _, wsummary = D.stats(want, part, [(0, n, -1)])
    assert (hist == whist).all() and summary == wsummary and hist[499] == 10 and hist[500] == 20
    many = device_depth([D.rec(0, 0, 10, "3M")] * 70000, (0, 0, 64), n, gpu=gpu)
    assert many.tolist() == [0] * 10 + [70000] * 3 + [0] * 51


def test_random_batch_in_windows_of_4096(gpu, world, random_case):
    records, prm, want = random_case
    for c, seq in enumerate(world):
        n = len(seq)
        assert want[c].sum() > 20000
        for start in range(0, n, 4096):   # records straddle the windows and are clipped to each
            length = min(4096, n - start)
            assert (device_depth(records, (c, start, length), n, prm, gpu) == want[c][start:start + length]).all()
    n = len(world[0])
    d = device_depth(records[:900], (0, 0, n), n, prm, gpu)   # two calls add up
    device_depth(records[900:], (0, 0, n), n, prm, gpu, depth=d)
    assert (d == want[0]).all()


def test_pieces_of_every_length_and_bit_offset(gpu, world, random_case):
    records, prm, want = random_case
    n = 200000
    rng = np.random.default_rng(5)
    depth = rng.integers(0, 40, n).astype(np.uint32)
    depth[:9000] = want[0]
    depth[150000:150600] = rng.integers(480, 520, 600)
    part = list(rng.random(n) < 0.9)
    part[70000:70300] = [False] * 300
    pieces, s = [], 0
    for start_bit in (0, 1, 63):
        s = (s + 63) // 64 * 64 + start_bit
        for length in (1, 63, 64, 65, 255, 256, 257):
            pieces.append((s, s + length, -1))
            s += length
    pieces.append((70000, 70300, -1))                                  # no participating locus
    pieces.append((70300, 70300, -1))                                  # no locus at all
    pieces.append((80000, 80000 + 65536, -1))                          # the longest piece
    pieces += [(s, s + 65536, 1), (s + 65536, s + 65537, 1)]           # an interval of 65,537 loci: two long pieces
    pieces.append((150000, 150600, 0))
    whist, wlong, wsum = D.stats(depth, part, pieces, 2)
    hist, long_hist, summary = device_stats(depth, part, pieces, 2, gpu)
    assert (hist == whist).all() and (long_hist == wlong).all() and summary == wsum
    assert wsum[21] == dict(total=0, loci=0, above=0, q1=1, median=1, q3=1) and wlong[0][500] > 0 and wlong[1].sum() > 50000
    # the tables are added to
    hist2, long2, _ = fcship.dp_stats(depth, D.bitmap(part), pieces, 2, hist.copy(), long_hist.copy(), device=gpu)
    assert (hist2 == 2 * whist).all() and (long2 == 2 * wlong).all()


def test_an_interval_over_three_windows_equals_one_window(gpu, world, random_case):
    records, prm, want = random_case
    depth = np.tile(want[0], 2)[:12000]
    part = [ch not in "Nn" for ch in (world[0] * 2)[:12000]]
    a, b = 1000, 11000                                                # 10,000 loci over windows of 4,096
    hist, long_hist, total = np.zeros(D.BINS, np.uint64), np.zeros((1, D.BINS), np.uint64), dict(total=0, loci=0, above=0)
    for w0 in range(0, 12000, 4096):
        w1 = min(w0 + 4096, 12000)
        s, e = max(a, w0) - w0, min(b, w1) - w0
        _, _, summary = device_stats(depth[w0:w1], part[w0:w1], [(s, e, 0)], 1, gpu, hist=hist, long_hist=long_hist)
        for k in total:
            total[k] += summary[0][k]
    whist, wlong, wsum = D.stats(depth, part, [(a, b, 0)], 1)
    one_hist, one_long, one = device_stats(depth, part, [(a, b, 0)], 1, gpu)
    assert (hist == whist).all() and (long_hist == wlong).all() and (one_hist == whist).all() and (one_long == wlong).all()
    assert {k: wsum[0][k] for k in total} == total == {k: one[0][k] for k in total}
    assert [D.quantile(long_hist[0], k) for k in (1, 2, 3)] == [D.quantile(D.histogram(
        [int(d) for d, p in zip(depth[a:b], part[a:b]) if p]), k) for k in (1, 2, 3)]


def to_dev(torch, dev, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(SIGNED.get(a.dtype, a.dtype)).copy()).to(dev)


def dev_batch(torch, dev, records, **kw):
    arrays = fcship.dp_arrays(*D.flatten(records))
    t = [to_dev(torch, dev, a) for a in arrays]
    flag, ref_id, pos, mapq, cigar, cigar_off, qual, base_off, absent = [x.data_ptr() for x in t]
    return t, fcship.DpBatch(kw.get("n", len(records)), flag, ref_id, pos, mapq, cigar, cigar_off,
                             kw.get("n_cigar", len(arrays[4])), 0, qual, base_off, len(arrays[6]), absent)


def test_dev_twins_on_a_caller_stream(gpu, world, random_case):
    import torch
    records, prm, want = random_case
    n = len(world[0])
    dev = torch.device(f"cuda:{gpu}")
    stream = torch.cuda.Stream(device=dev)
    p, w = fcship.dp_params(**prm), fcship.DpWindow(0, 0, 0, n, n)
    part = [ch not in "Nn" for ch in world[0]]
    pieces = [(0, 4096, 0), (4096, n, 0), (100, 164, -1), (5000, 5001, -1)]
    whist, wlong, wsum = D.stats(want[0], part, pieces, 1)
    with torch.cuda.stream(stream):
        keep1, b1 = dev_batch(torch, dev, records[:700])          # two chunks accumulate before the one scan
        keep2, b2 = dev_batch(torch, dev, records[700:])
        cells = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        status = torch.zeros(4, dtype=torch.int32, device=dev)
        need = fcship.lib.fcsdp_workspace_bytes(n)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        for b in (b1, b2):
            fcship.check(fcship.lib.fcsdp_runs_dev(gpu, C.addressof(b), C.addressof(p), C.addressof(w), cells.data_ptr(),
                                                   status.data_ptr(), C.c_void_p(stream.cuda_stream)))
        fcship.check(fcship.lib.fcsdp_scan_dev(gpu, cells.data_ptr(), n, ws.data_ptr(), need, status.data_ptr(),
                                               C.c_void_p(stream.cuda_stream)))
        bits = to_dev(torch, dev, D.bitmap(part))
        pc = to_dev(torch, dev, np.array([(s, e, li, 0) for s, e, li in pieces], fcship.DP_PIECE).view(np.int32))
        hist = torch.full((D.BINS,), 7, dtype=torch.int64, device=dev)   # the tables are added to
        long_hist = torch.full((1, D.BINS), 7, dtype=torch.int64, device=dev)
        summary = torch.zeros(len(pieces) * 8, dtype=torch.int32, device=dev)
        fcship.check(fcship.lib.fcsdp_stats_dev(gpu, cells.data_ptr(), bits.data_ptr(), n, pc.data_ptr(), len(pieces), 1,
                                                hist.data_ptr(), long_hist.data_ptr(), summary.data_ptr(),
                                                status[1:].data_ptr(), C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    assert status.cpu().tolist() == [0, 0, 0, 0]
    got = cells.cpu().numpy()
    assert (got[:n].view(np.uint32) == want[0]).all()
    assert (got[:n].view(np.uint32) == device_depth(records, (0, 0, n), n, prm, gpu)).all()
    assert (hist.cpu().numpy() == whist.astype(np.int64) + 7).all() and (long_hist.cpu().numpy() == wlong.astype(np.int64) + 7).all()
    sm = summary.cpu().numpy().view(fcship.DP_SUMMARY)
    assert [{k: int(s[k]) for k in wsum[0]} for s in sm] == wsum
    # a record one past its contig's end sets the status bit and is otherwise clipped; a cigar_off beyond n_cigar is
    # clamped, reported, and its record adds nothing
    case = next(c for c in CASES if c["name"] == "ends_one_past_contig_end")
    with torch.cuda.stream(stream):
        keep3, b3 = dev_batch(torch, dev, case["records"])
        small = torch.zeros(41, dtype=torch.int32, device=dev)
        status.zero_()
        w1 = fcship.DpWindow(1, 0, 0, 40, 40)
        p0 = fcship.dp_params()
        fcship.check(fcship.lib.fcsdp_runs_dev(gpu, C.addressof(b3), C.addressof(p0), C.addressof(w1), small.data_ptr(),
                                               status.data_ptr(), C.c_void_p(stream.cuda_stream)))
        fcship.check(fcship.lib.fcsdp_scan_dev(gpu, small.data_ptr(), 40, ws.data_ptr(), need, status.data_ptr(),
                                               C.c_void_p(stream.cuda_stream)))
        two = [D.rec(0, 0, 10, "10M"), D.rec(0, 0, 30, "5M2I3M")]
        keep4, b4 = dev_batch(torch, dev, two, n_cigar=2)            # the second record's words end at 4
        cells2 = torch.zeros(301, dtype=torch.int32, device=dev)
        w0 = fcship.DpWindow(0, 0, 0, 300, 300)
        fcship.check(fcship.lib.fcsdp_runs_dev(gpu, C.addressof(b4), C.addressof(p0), C.addressof(w0), cells2.data_ptr(),
                                               status[1:].data_ptr(), C.c_void_p(stream.cuda_stream)))
        fcship.check(fcship.lib.fcsdp_scan_dev(gpu, cells2.data_ptr(), 300, ws.data_ptr(), need, status[1:].data_ptr(),
                                               C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    assert status.cpu().tolist()[:2] == [fcship.FCSDP_STATUS_REF, fcship.FCSDP_STATUS_FIELD]
    assert (small.cpu().numpy()[:40].view(np.uint32) == D.want_depths(case)).all()
    assert cells2.cpu().numpy()[:300].tolist() == [0] * 10 + [1] * 10 + [0] * 280


def test_two_threads_each_on_their_own_session(gpu, world):
    n = len(world[0])
    batches = [D.random_batch(world, seed=100 + k, n=300 + 50 * k) for k in range(2)]
    want = [D.depth(b, (0, 0, n), n)[0] for b in batches]
    got, errors = [None] * 2, []

    def work(k):
        try:
            for _ in range(3):
                got[k] = device_depth(batches[k], (0, 0, n), n, gpu=gpu)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


def test_bad_arguments_write_nothing(gpu):
    records = [D.rec(0, 0, 10 * k, "10M") for k in range(4)]
    depth = np.full(300, 7, np.uint32)
    a = D.flatten(records)
    bad = (a[0], a[1], a[2], a[3], a[4], a[5], a[6], [0, 10, 9, 30, 40], a[8])
    with pytest.raises(fcship.FcsError, match="base offsets out of order at record 1"):
        fcship.dp_count(bad, (0, 0, 300, 300), depth=depth, device=gpu)
    with pytest.raises(fcship.FcsError):
        fcship.dp_count(a, (0, 0, 300, 300), depth=depth, device=99)
    assert (depth == 7).all()
    fcship.dp_count(a, (0, 0, 300, 300), depth=depth, device=gpu)
    assert depth.tolist() == [8] * 40 + [7] * 260


def test_depth_command_gpu_and_host_write_identical_files(gpu, tmp_path):
    d = tmp_path / "s"
    p = H.run_cli("synth", "-o", d, "-c", "chr1:150000,chr2:50000", "-x", "6", "--seed", "8", "--no-fastq")
    assert p.returncode == 0, p.stderr[-2000:]
    (tmp_path / "l.bed").write_text("chr1\t1000\t1200\nchr1\t60000\t140000\nchr2\t5\t6\n")
    suffixes = ["", ".sample_summary", ".sample_statistics", ".sample_cumulative_coverage_counts",
                ".sample_cumulative_coverage_proportions", ".sample_interval_summary", ".sample_interval_statistics"]
    for tag, extra in (("all", []), ("bed", ["-L", tmp_path / "l.bed"])):
        logs = {}
        for mode in ("true", "false"):
            p = H.run_cli("depth", "-r", d / "ref.fasta", "-i", d / "sample.bam", "-o", tmp_path / f"{tag}_{mode}", *extra,
                          env={"FCS_DEPTH_GPU": mode, "FCS_GPU_DEVICES": str(gpu), "FCS_DEPTH_CHUNK_RECORDS": "3000",
                               "FCS_DEPTH_WINDOW_BP": "65536"}, cwd=tmp_path)
            assert p.returncode == 0, p.stderr[-2000:]
            logs[mode] = p.stderr
        assert "(GPU)" in logs["true"] and "(host)" in logs["false"]
        for s in suffixes:
            assert (tmp_path / f"{tag}_true{s}").read_bytes() == (tmp_path / f"{tag}_false{s}").read_bytes(), s
    assert (tmp_path / "all_true").read_text().count("\n") == 200001
    total = int((tmp_path / "all_true.sample_summary").read_text().split("\n")[1].split("\t")[1])
    assert total > 1000000


def test_depth_command_streams_a_part_directory_gpu_and_host_identical(gpu, tmp_path):
    """Chunks of 128 records, a file boundary and windows of 1,024 loci all fall inside the data (bam_stream_cases)."""
    ref, parts, n = S.part_directory(tmp_path)
    suffixes = ["", ".sample_summary", ".sample_statistics", ".sample_cumulative_coverage_counts",
                ".sample_cumulative_coverage_proportions", ".sample_interval_summary", ".sample_interval_statistics"]
    logs = {}
    for mode in ("false", "true"):
        p = H.run_cli("depth", "-r", ref, "-i", parts, "-o", tmp_path / mode,
                      env={"FCS_DEPTH_GPU": mode, "FCS_GPU_DEVICES": str(gpu), "FCS_DEPTH_CHUNK_RECORDS": "128",
                           "FCS_DEPTH_WINDOW_BP": str(S.WINDOW_BP)}, cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-2000:]
        logs[mode] = p.stderr.rstrip("\n").split("\n")[-1]
    assert "(host)" in logs["false"] and "(GPU)" in logs["true"]
    assert f": {n} records, 2 intervals, 12 windows, " in logs["true"], logs["true"]
    for s in suffixes:
        assert (tmp_path / f"true{s}").read_bytes() == (tmp_path / f"false{s}").read_bytes(), s
    assert int(logs["true"].split("total depth ")[1].split(",")[0]) > 0
