"""GPU: base quality recalibration (fcsbq_count / fcsbq_apply and their _dev
twins) equals the Python restatement of the rules
(tests/bqsr_cases.py) exactly."""
import ctypes as C
import threading

import numpy as np
import pytest

import bam_stream_cases as S
import bqsr_cases as B
import fcship
import host_lib as H

pytestmark = pytest.mark.gpu
CASES = B.hand_cases()


@pytest.fixture(scope="module")
def hand_ref(gpu):
    with fcship.bq_ref(*B.flat_reference(B.REFS, B.KNOWN), device=gpu) as ref:
        yield ref


@pytest.fixture(scope="module")
def world(gpu):
    refs, known = B.random_world()
    with fcship.bq_ref(*B.flat_reference(refs, known), device=gpu) as ref:
        yield refs, known, ref


@pytest.fixture(scope="module")
def random_case(world):
    """(records, restatement's ctx, cyc, tables, new qualities) of the random batch, computed once."""
    refs, known, _ = world
    records = B.random_batch(refs=refs)
    ctx, cyc = B.new_tables(3)
    B.count(records, refs, known, 3, ctx, cyc)
    tables = B.finalize(ctx, cyc)
    return records, ctx, cyc, tables, B.apply(records, *tables)


def device_count(ref, records, n_rg, ctx=None, cyc=None, first_offset=0):
    return fcship.bq_count(ref, B.flatten(records, first_offset), n_rg, ctx, cyc)


def device_apply(records, tables, gpu, first_offset=0):
    out = fcship.bq_apply(B.flatten(records, first_offset), *tables, device=gpu)
    assert (out[:first_offset] == 0xEE).all()
    return B.unflatten_quals(records, out, first_offset)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_case(gpu, hand_ref, case):
    n_rg = case["n_rg"]
    want = B.dense(case["want"], n_rg)
    ctx, cyc = device_count(hand_ref, case["records"], n_rg)
    assert (ctx == want[0]).all() and (cyc == want[1]).all()
    if case["table"]:
        assert device_apply(case["records"], B.case_table(case, ctx, cyc), gpu) == case["want_qual"]


def test_all_hand_cases_as_one_batch(gpu, hand_ref):
    records = []
    want = B.new_tables(2)
    for case in CASES:
        records += case["records"]
        w = B.dense(case["want"], 2)
        want[0][...] += w[0]
        want[1][...] += w[1]
    ctx, cyc = device_count(hand_ref, records, 2)
    assert (ctx == want[0]).all() and (cyc == want[1]).all()
    rctx, rcyc = B.new_tables(2)
    B.count(records, B.REFS, B.KNOWN, 2, rctx, rcyc)
    assert (rctx == ctx).all() and (rcyc == cyc).all()
    tables = B.finalize(rctx, rcyc)
    assert device_apply(records, tables, gpu) == B.apply(records, *tables)


def test_zero_records_and_one_record(gpu, hand_ref):
    ctx, cyc = device_count(hand_ref, [], 1)
    assert not ctx.any() and not cyc.any()
    assert device_apply([], B.hand_table(), gpu) == []
    one = [B.rec(0, 0, 4, "1M", "A", 30)]
    ctx, cyc = device_count(hand_ref, one, 1)
    assert ctx.sum() == 0 and cyc.sum() == 1 and tuple(cyc[0, 30, 0]) == (1, 0)
    assert device_apply(one, B.hand_table(), gpu) == [[25]]


def test_lengths_at_every_offset_residue(gpu, world):
    refs, known, ref = world
    for seed, first in ((3, 0), (4, 3), (5, 1)):
        records = B.sweep_batch(refs, seed=seed)
        rctx, rcyc = B.new_tables(3)
        B.count(records, refs, known, 3, rctx, rcyc)
        ctx, cyc = device_count(ref, records, 3, first_offset=first)
        assert (ctx == rctx).all() and (cyc == rcyc).all() and cyc.sum() > 500
        tables = B.finalize(rctx, rcyc)
        assert device_apply(records, tables, gpu, first_offset=first) == B.apply(records, *tables)
        hand = B.hand_table(3)
        assert device_apply(records, hand, gpu, first_offset=first) == B.apply(records, *hand)


def test_junk_before_the_first_cigar_word_and_the_first_base(gpu, hand_ref):
    """Both offset arrays start at 3: only [off[0], off[n]) is staged and the device view keeps the caller's offsets."""
    records = [r for k in (0, 1, 2, 3, 5, 12) for r in CASES[k]["records"]]   # clips, known sites, two read groups
    assert len(records) == 12
    plain = fcship.bq_arrays(*B.flatten(records))
    flag, ref_id, pos, mapq, rg, cigar, cigar_off, bases, qual, base_off, absent = plain
    junk = np.array([0xEE] * 3, np.uint8)
    padded = (flag, ref_id, pos, mapq, rg, np.concatenate([np.full(3, 0xEEEEEEEE, np.uint32), cigar]), cigar_off + 3,
              np.concatenate([junk, bases]), np.concatenate([junk, qual]), base_off + 3, absent)
    assert len(padded[5]) == len(cigar) + 3 and len(padded[7]) == len(padded[8]) == len(bases) + 3
    rctx, rcyc = B.new_tables(2)
    B.count(records, B.REFS, B.KNOWN, 2, rctx, rcyc)
    ctx, cyc = fcship.bq_count(hand_ref, padded, 2)
    assert (ctx == rctx).all() and (cyc == rcyc).all() and cyc.sum() > 0
    pctx, pcyc = fcship.bq_count(hand_ref, plain, 2)
    assert ctx.tobytes() == pctx.tobytes() and cyc.tobytes() == pcyc.tobytes()
    tables = B.hand_table(2)
    out = fcship.bq_apply(padded, *tables, device=gpu)
    assert (out[:3] == 0xEE).all()
    assert B.unflatten_quals(records, out, 3) == B.apply(records, *tables)
    assert out[3:].tobytes() == fcship.bq_apply(plain, *tables, device=gpu).tobytes()


def test_20000_copies_of_one_read_at_one_quality(gpu, hand_ref):
    records = B.one_hot_read(20000)
    rctx, rcyc = B.new_tables(1)
    B.count(records[:1], B.REFS, B.KNOWN, 1, rctx, rcyc)
    ctx, cyc = device_count(hand_ref, records, 1)
    assert (ctx == 20000 * rctx).all() and (cyc == 20000 * rcyc).all()
    assert cyc[0, 33, 0:302:2, 0].tolist() == [20000] * 151 and ctx[..., 0].sum() == 150 * 20000


def test_random_batch_of_three_interleaved_read_groups(gpu, world, random_case):
    """1200 records over 38 blocks' slices, the read groups interleaved: most contexts take the global path."""
    _, _, ref = world
    records, ctx, cyc, tables, new = random_case
    assert len({r["rg"] for r in records[:40]}) >= 3
    got = device_count(ref, records, 3)
    assert (got[0] == ctx).all() and (got[1] == cyc).all()
    assert device_apply(records, tables, gpu) == new
    grouped = sorted(records, key=lambda r: r["rg"])   # as the commands flatten: the LDS path
    got = device_count(ref, grouped, 3)
    assert (got[0] == ctx).all() and (got[1] == cyc).all()


def test_two_calls_add_up_to_one_call_on_the_concatenation(gpu, world, random_case):
    _, _, ref = world
    records, ctx, cyc, _, _ = random_case
    got = device_count(ref, records[:500], 3)
    got = device_count(ref, records[500:], 3, *got)
    assert (got[0] == ctx).all() and (got[1] == cyc).all()


def test_two_identical_calls_give_identical_bytes(gpu, world, random_case):
    _, _, ref = world
    records, _, _, tables, _ = random_case
    a, b = device_count(ref, records, 3), device_count(ref, records, 3)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    arrays = B.flatten(records)
    assert fcship.bq_apply(arrays, *tables, device=gpu).tobytes() == fcship.bq_apply(arrays, *tables, device=gpu).tobytes()


def test_dev_entry_points_on_a_caller_stream(gpu, world, random_case):
    import torch
    _, _, ref = world
    records, ctx, cyc, tables, new = random_case
    arrays = fcship.bq_arrays(*B.flatten(records))
    dev = torch.device("cuda", gpu)
    stream = torch.cuda.Stream(device=dev)
    views = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}
    with torch.cuda.stream(stream):
        t = [torch.from_numpy(a.view(views.get(a.dtype, a.dtype)).copy()).to(dev) for a in arrays]
        flag, ref_id, pos, mapq, rg, cigar, cigar_off, bases, qual, base_off, absent = [x.data_ptr() for x in t]
        b = fcship.BqBatch(len(records), flag, ref_id, pos, mapq, rg, cigar, cigar_off, len(arrays[5]), bases, qual,
                           base_off, len(arrays[7]), absent)
        need = fcship.lib.fcsbq_workspace_bytes(3)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        dctx = torch.full(ctx.shape, 7, dtype=torch.int64, device=dev)   # the counts are added to what is there
        dcyc = torch.full(cyc.shape, 7, dtype=torch.int64, device=dev)
        status = torch.full((2,), -1, dtype=torch.int32, device=dev)
        fcship.check(fcship.lib.fcsbq_count_dev(ref.handle, C.addressof(b), 3, ws.data_ptr(), need, dctx.data_ptr(),
                                                dcyc.data_ptr(), status.data_ptr(), C.c_void_p(stream.cuda_stream)))
        tabs = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in tables]
        out = torch.full((len(arrays[7]),), 0xEE, dtype=torch.uint8, device=dev)
        fcship.check(fcship.lib.fcsbq_apply_dev(gpu, C.addressof(b), 3, tabs[0].data_ptr(), tabs[1].data_ptr(),
                                                tabs[2].data_ptr(), out.data_ptr(), status[1:].data_ptr(),
                                                C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    assert status.cpu().tolist() == [0, 0]
    assert (dctx.cpu().numpy() == ctx + 7).all() and (dcyc.cpu().numpy() == cyc + 7).all()
    assert B.unflatten_quals(records, out.cpu().numpy()) == new
    # a 501-base record: the status says so, nothing is added and nothing is written
    long = fcship.bq_arrays(*B.flatten(CASES[11]["refused"]))
    with torch.cuda.stream(stream):
        t = [torch.from_numpy(a.view(views.get(a.dtype, a.dtype)).copy()).to(dev) for a in long]
        flag, ref_id, pos, mapq, rg, cigar, cigar_off, bases, qual, base_off, absent = [x.data_ptr() for x in t]
        b = fcship.BqBatch(1, flag, ref_id, pos, mapq, rg, cigar, cigar_off, 1, bases, qual, base_off, 501, absent)
        out = torch.full((501,), 0xEE, dtype=torch.uint8, device=dev)
        with fcship.bq_ref(*B.flat_reference(B.REFS, B.KNOWN), device=gpu) as hand_ref:
            fcship.check(fcship.lib.fcsbq_count_dev(hand_ref.handle, C.addressof(b), 3, ws.data_ptr(), need,
                                                    dctx.data_ptr(), dcyc.data_ptr(), status.data_ptr(),
                                                    C.c_void_p(stream.cuda_stream)))
            fcship.check(fcship.lib.fcsbq_apply_dev(gpu, C.addressof(b), 3, tabs[0].data_ptr(), tabs[1].data_ptr(),
                                                    tabs[2].data_ptr(), out.data_ptr(), status[1:].data_ptr(),
                                                    C.c_void_p(stream.cuda_stream)))
            stream.synchronize()
    assert status.cpu().tolist() == [fcship.FCSBQ_STATUS_LONG, fcship.FCSBQ_STATUS_LONG]
    assert (dctx.cpu().numpy() == ctx + 7).all() and (dcyc.cpu().numpy() == cyc + 7).all()
    assert (out.cpu().numpy() == 0xEE).all()


def test_four_threads_each_with_their_own_batch(gpu, world):
    refs, known, ref = world
    batches = [B.random_batch(seed=100 + k, n=150 + 30 * k, refs=refs) for k in range(4)]
    want = []
    for recs in batches:
        ctx, cyc = B.new_tables(3)
        B.count(recs, refs, known, 3, ctx, cyc)
        want.append((ctx, cyc, B.apply(recs, *B.hand_table(3))))
    got, errors = [None] * 4, []

    def work(k):
        try:
            for _ in range(3):
                ctx, cyc = device_count(ref, batches[k], 3)
                got[k] = (ctx, cyc, device_apply(batches[k], B.hand_table(3), gpu))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for g, w in zip(got, want):
        assert (g[0] == w[0]).all() and (g[1] == w[1]).all() and g[2] == w[2]


def test_bad_arguments_and_the_501_base_record_write_nothing(gpu, hand_ref):
    records = CASES[0]["records"] * 4
    arrays = fcship.bq_arrays(*B.flatten(records))
    ctx, cyc = B.new_tables(1)
    ctx[...] = 5
    cyc[...] = 5
    out = np.full(512, 0xEE, np.uint8)
    base, dctx, dcyc = B.hand_table()

    def swapped(a, k, values):
        a = list(a)
        a[k] = np.ascontiguousarray(values, a[k].dtype)
        return tuple(a)

    def both(a=arrays, n_rg=1, **kw):
        b = fcship.bq_batch(a, **kw)
        rc = fcship.lib.fcsbq_count(hand_ref.handle, C.addressof(b), n_rg, ctx.ctypes.data, cyc.ctypes.data)
        ra = fcship.lib.fcsbq_apply(gpu, C.addressof(b), n_rg, base.ctypes.data, dctx.ctypes.data, dcyc.ctypes.data,
                                    out.ctypes.data)
        return rc, ra

    for kw in (dict(n=-1), dict(a=swapped(arrays, 9, [0, 10, 9, 30, 40])), dict(a=swapped(arrays, 4, [0, 0, 1, 0])),
               dict(n_bases=1 << 32), dict(n_bases=39)):
        assert both(**kw) == (fcship.FCS_ERR_INVALID, fcship.FCS_ERR_INVALID), kw
        assert (ctx == 5).all() and (cyc == 5).all() and (out == 0xEE).all(), kw
    # what only count refuses: a reference outside the handle's, an aligned base beyond its contig
    for a, what in ((swapped(arrays, 1, [0, 3, 0, 0]), "ref_id 3 of record 1"),
                    (swapped(arrays, 2, [4, 4, 120, 4]), "record 2 has an aligned base beyond its contig")):
        b = fcship.bq_batch(a)
        assert fcship.lib.fcsbq_count(hand_ref.handle, C.addressof(b), 1, ctx.ctypes.data, cyc.ctypes.data) == fcship.FCS_ERR_INVALID
        assert "[E::fcsbq_count]" in fcship.lib.fcs_last_error().decode() and what in fcship.lib.fcs_last_error().decode()
        assert (ctx == 5).all() and (cyc == 5).all()
    long = fcship.bq_arrays(*B.flatten(CASES[0]["records"] + CASES[11]["refused"]))
    assert both(a=long) == (fcship.FCS_ERR_INVALID, fcship.FCS_ERR_INVALID)
    assert "501 bases, more than 500" in fcship.lib.fcs_last_error().decode()
    assert (ctx == 5).all() and (cyc == 5).all() and (out == 0xEE).all()
    assert both() == (fcship.FCS_OK, fcship.FCS_OK)
    want = B.dense(CASES[0]["want"], 1)
    assert (ctx == 5 + 4 * want[0]).all() and (cyc == 5 + 4 * want[1]).all()
    b = fcship.bq_batch(arrays)
    assert fcship.lib.fcsbq_apply(99, C.addressof(b), 1, base.ctypes.data, dctx.ctypes.data, dcyc.ctypes.data,
                                  out.ctypes.data) == fcship.FCS_ERR_INVALID


def test_bqsr_command_gpu_and_host_write_identical_files(gpu, tmp_path):
    d = tmp_path / "s"
    p = H.run_cli("synth", "-o", d, "-c", "chr1:30000,chr2:20000", "-x", "8", "--seed", "8", "--no-fastq")
    assert p.returncode == 0, p.stderr[-2000:]
    logs = {}
    for mode in ("true", "false"):
        p = H.run_cli("bqsr", "-r", d / "ref.fasta", "-i", d / "sample.bam", "-K", d / "truth.vcf",
                      "-o", tmp_path / f"{mode}.bam", "-b", tmp_path / f"{mode}.grp",
                      env={"FCS_BQSR_GPU": mode, "FCS_GPU_DEVICES": str(gpu), "FCS_BQSR_CHUNK_RECORDS": "1000"},
                      cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-2000:]
        logs[mode] = p.stderr
    assert "(GPU)" in logs["true"] and "(host)" in logs["false"]
    assert (tmp_path / "true.grp").read_bytes() == (tmp_path / "false.grp").read_bytes()
    assert (tmp_path / "true.bam").read_bytes() == (tmp_path / "false.bam").read_bytes()
    assert (tmp_path / "true.bam.bai").read_bytes() == (tmp_path / "false.bam.bai").read_bytes()
    _, _, before = H.read_bam(d / "sample.bam")
    _, _, after = H.read_bam(tmp_path / "true.bam")
    assert sum(a["qual"] != b["qual"] for a, b in zip(before, after)) > 1000


def test_bqsr_command_streams_a_part_directory_gpu_and_host_identical(gpu, tmp_path):
    """Chunks of 128 records and a file boundary fall inside the data (bam_stream_cases); bqsr has no windows."""
    ref, parts, n = S.part_directory(tmp_path)
    logs = {}
    for mode in ("false", "true"):
        p = H.run_cli("bqsr", "-r", ref, "-i", parts, "-o", tmp_path / f"{mode}.bam", "-b", tmp_path / f"{mode}.grp",
                      env={"FCS_BQSR_GPU": mode, "FCS_GPU_DEVICES": str(gpu), "FCS_BQSR_CHUNK_RECORDS": "128"}, cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-2000:]
        logs[mode] = p.stderr.rstrip("\n").split("\n")[-1]
    assert "(host)" in logs["false"] and "(GPU)" in logs["true"]
    assert f"] {n} records, " in logs["true"], logs["true"]
    for s in ("bam", "grp"):
        assert (tmp_path / f"true.{s}").read_bytes() == (tmp_path / f"false.{s}").read_bytes(), s
    assert int(logs["true"].split(" recalibrated")[0].split(", ")[-1]) > 0
