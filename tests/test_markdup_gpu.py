"""GPU: duplicate marking (fcsdup_mark / fcsdup_mark_dev) equals
the Python restatement of the rules (tests/markdup_cases.py) exactly."""
import ctypes as C
import threading

import numpy as np
import pytest

import fcship
import host_lib as H
import markdup_cases as M

pytestmark = pytest.mark.gpu
CASES = M.hand_cases()


def device_mark(records, gpu):
    n_ref, n_lib = M.n_ref_lib(records)
    dup, st = fcship.dup_mark(M.flatten(records), n_ref, n_lib, device=gpu)
    return list(dup), st


def check(records, gpu):
    got, st = device_mark(records, gpu)
    want = M.expected(records)
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b][:20]
    assert st == M.stats(records)
    return want


@pytest.fixture(scope="module")
def random_records():
    return M.random_batch()


@pytest.mark.parametrize("name,records,want", CASES, ids=[c[0] for c in CASES])
def test_hand_case(gpu, name, records, want):
    got, st = device_mark(records, gpu)
    assert got == want
    assert st == M.stats(records)


def test_all_hand_cases_as_one_batch(gpu):
    records = []
    for k, (_, recs, _) in enumerate(CASES):
        base = len(records)
        records += [dict(r, pos=r["pos"] + 3000 * (k + 1), mate=r["mate"] + base if r["mate"] >= 0 else -1) for r in recs]
    assert check(records, gpu) == [f for _, _, want in CASES for f in want]


def test_junk_before_the_first_cigar_word_and_the_first_quality_byte(gpu):
    """Both offset arrays start at 3: only [off[0], off[n]) is staged and the device view keeps the caller's offsets."""
    records = []
    for k, (_, recs, _) in enumerate(CASES):
        base = len(records)
        records += [dict(r, pos=r["pos"] + 3000 * (k + 1), mate=r["mate"] + base if r["mate"] >= 0 else -1) for r in recs]
    flag, ref_id, pos, mate, lib, cigar, cigar_off, qual, qual_off = M.flatten(records)
    padded = (flag, ref_id, pos, mate, lib, np.concatenate([np.full(3, 0xEEEEEEEE, np.uint32), cigar]), cigar_off + 3,
              np.concatenate([np.full(3, 0xEE, np.uint8), qual]), qual_off + 3)
    n_ref, n_lib = M.n_ref_lib(records)
    dup, st = fcship.dup_mark(padded, n_ref, n_lib, device=gpu)
    assert list(dup) == M.expected(records) == [f for _, _, want in CASES for f in want]
    assert st == M.stats(records)


def test_zero_one_and_two_records(gpu):
    assert device_mark([], gpu) == ([], dict(examined=0, pairs=0, fragments=0, duplicates=0))
    assert check([M.rec(0, 0, 5, "10M", 30)], gpu) == [0]
    assert check([M.rec(M.UNMAPPED, -1, -1, "", b"")], gpu) == [0]
    assert check([M.rec(0, 0, 5, "10M", 30), M.rec(0, 0, 5, "10M", 31)], gpu) == [1, 0]
    assert check(M.pair(0, M.rec(M.R1_FWD, 0, 5, "10M", 30), M.rec(M.R2_REV, 0, 50, "10M", 30)), gpu) == [0, 0]


def test_one_group_of_300_identical_pairs(gpu):
    want = check(M.identical_pairs(300), gpu)
    assert sum(want) == 598


def test_one_group_of_70_fragments(gpu):
    want = check(M.fragment_group(70), gpu)
    assert sum(want) == 69 and want[41] == 0


def test_quality_lengths_at_every_byte_offset(gpu):
    records = M.quality_offsets()
    want = check(records, gpu)
    assert sum(want) == 2 * 4 * len(M.QUAL_LENGTHS)


def test_random_batch(gpu, random_records):
    want = check(random_records, gpu)
    assert 0.30 <= sum(want) / len(want) <= 0.50


def test_two_calls_give_identical_bytes(gpu, random_records):
    arrays = M.flatten(random_records)
    a, sa = fcship.dup_mark(arrays, 3, 3, device=gpu)
    b, sb = fcship.dup_mark(arrays, 3, 3, device=gpu)
    assert a.tobytes() == b.tobytes() and sa == sb


def test_dev_entry_point_on_a_caller_stream(gpu, random_records):
    import torch
    records = random_records[:6001]
    if records[-1]["mate"] >= len(records):
        records = records[:-1]
    arrays = fcship.dup_arrays(*M.flatten(records))
    want, want_st = fcship.dup_mark(arrays, 3, 3, device=gpu)
    dev = torch.device("cuda", gpu)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        t = [torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a.view(np.int32) if a.dtype == np.uint32
                              else a).to(dev) for a in arrays]
        need = fcship.lib.fcsdup_workspace_bytes(len(records))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        dup = torch.full((len(records),), 0xEE, dtype=torch.uint8, device=dev)
        st = torch.full((4,), -1, dtype=torch.int64, device=dev)
        status = torch.full((1,), -1, dtype=torch.int32, device=dev)
        b = fcship.DupBatch(len(records), *[x.data_ptr() for x in t[:7]], len(arrays[5]), t[7].data_ptr(),
                            t[8].data_ptr(), len(arrays[7]), 3, 3)
        fcship.check(fcship.lib.fcsdup_mark_dev(gpu, C.addressof(b), ws.data_ptr(), need, dup.data_ptr(), st.data_ptr(),
                                                status.data_ptr(), C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    assert int(status.cpu()[0]) == 0
    assert dup.cpu().numpy().tobytes() == want.tobytes()
    assert dict(zip(("examined", "pairs", "fragments", "duplicates"), map(int, st.cpu().numpy()))) == want_st


def test_four_threads_each_with_their_own_batch(gpu):
    batches = [M.random_batch(seed=100 + k, templates=1500 + 200 * k) for k in range(4)]
    want = [M.expected(b) for b in batches]
    got, errors = [None] * 4, []

    def work(k):
        try:
            for _ in range(3):
                got[k] = device_mark(batches[k], gpu)[0]
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert got == want


def test_bad_arguments_write_nothing(gpu):
    records = CASES[0][1]
    arrays = fcship.dup_arrays(*M.flatten(records))
    dup = np.full(4, 0xEE, np.uint8)
    st = fcship.DupStats(-1, -1, -1, -1)

    def mark(a=arrays, n_ref=1, n_lib=1, **kw):
        b = fcship.dup_batch(a, n_ref, n_lib, **kw)
        return fcship.lib.fcsdup_mark(gpu, C.addressof(b), dup.ctypes.data, C.addressof(st))

    def swapped(k, values):
        a = list(arrays)
        a[k] = np.ascontiguousarray(values, arrays[k].dtype)
        return tuple(a)

    for kw in (dict(n=-1), dict(a=swapped(8, [0, 100, 90, 300, 400])), dict(a=swapped(3, [1, 0, 3, 9])),
               dict(n_ref=fcship.FCSDUP_MAX_REFS + 1),
               dict(a=swapped(2, [100, 300, fcship.FCSDUP_MAX_POS + 5, 300]))):   # a u5 beyond the key's width
        assert mark(**kw) == fcship.FCS_ERR_INVALID, kw
        assert "[E::fcsdup_mark]" in fcship.lib.fcs_last_error().decode(), kw
        assert (dup == 0xEE).all() and st.examined == -1, kw
    assert mark() == fcship.FCS_OK and list(dup) == CASES[0][2]
    b = fcship.dup_batch(arrays, 1, 1)
    assert fcship.lib.fcsdup_mark(99, C.addressof(b), dup.ctypes.data, C.addressof(st)) == fcship.FCS_ERR_INVALID


def test_markdup_command_gpu_and_host_write_identical_bams(gpu, tmp_path):
    d = tmp_path / "s"
    p = H.run_cli("synth", "-o", d, "-c", "chr1:30000,chr2:20000", "-x", "40", "--seed", "8", "--no-fastq")
    assert p.returncode == 0, p.stderr[-2000:]
    logs = {}
    for mode in ("true", "false"):
        p = H.run_cli("markdup", "-i", d / "sample.bam", "-o", tmp_path / f"{mode}.bam",
                      env={"FCS_MARKDUP_GPU": mode, "FCS_GPU_DEVICES": str(gpu)}, cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-2000:]
        logs[mode] = p.stderr
    assert "(GPU)" in logs["true"] and "(host)" in logs["false"]
    assert (tmp_path / "true.bam").read_bytes() == (tmp_path / "false.bam").read_bytes()
    assert (tmp_path / "true.bam.bai").read_bytes() == (tmp_path / "false.bam.bai").read_bytes()
    _, _, recs = H.read_bam(tmp_path / "true.bam")
    assert sum(bool(r["flag"] & M.DUPLICATE) for r in recs) > 0   # 40x of single-end reads: some 5' ends coincide
