"""GPU: markdup, bqsr, depth and ug at the shapes they really run at
(tests/scale_cases.py): past the first trip of every block- and grid-stride
loop, past the first pass of every one-block scan, and at chr1-sized
coordinates.  Everything is integers: every comparison is exact.  The inputs and
their references are checked on the CPU in tests/test_scale_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import bqsr_cases as B
import depth_cases as D
import fcship
import markdup_cases as M
import scale_cases as S
import ug_cases as U

pytestmark = pytest.mark.gpu
SH = S.SHAPES
SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
TABLE = np.array(S.TAB, np.int64)


def to_dev(torch, dev, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(SIGNED.get(a.dtype, a.dtype)).copy()).to(dev)


# ------------------------------------------------------------------ depth
def device_depth(arrays, window, contig_len, prm, gpu):
    ref, start, length = window
    return fcship.dp_count(arrays, (ref, start, length, contig_len), fcship.dp_params(**prm), device=gpu)


def device_stats(d, part, pieces, n_long, gpu):
    hist, long_hist, summary = fcship.dp_stats(d, S.bitmap_np(part), pieces, n_long, device=gpu)
    return hist, long_hist, S.summaries(summary)


def depth_twin(gpu, arrays, window, contig_len, prm):
    """fcsdp_runs_dev and fcsdp_scan_dev on a caller stream: (depths, status)."""
    import torch
    ref, start, length = window
    dev = torch.device(f"cuda:{gpu}")
    stream = torch.cuda.Stream(device=dev)
    arrays = fcship.dp_arrays(*arrays)
    with torch.cuda.stream(stream):
        t = [to_dev(torch, dev, a) for a in arrays]
        flag, ref_id, pos, mapq, cigar, cigar_off, qual, base_off, absent = [x.data_ptr() for x in t]
        b = fcship.DpBatch(len(arrays[0]), flag, ref_id, pos, mapq, cigar, cigar_off, len(arrays[4]), 0, qual, base_off,
                           len(arrays[6]), absent)
        cells = torch.zeros(length + 1, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        need = fcship.lib.fcsdp_workspace_bytes(length)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        p, w = fcship.dp_params(**prm), fcship.DpWindow(ref, 0, start, length, contig_len)
        fcship.check(fcship.lib.fcsdp_runs_dev(gpu, C.addressof(b), C.addressof(p), C.addressof(w), cells.data_ptr(),
                                               status.data_ptr(), C.c_void_p(stream.cuda_stream)))
        fcship.check(fcship.lib.fcsdp_scan_dev(gpu, cells.data_ptr(), length, ws.data_ptr(), need, status.data_ptr(),
                                               C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    return cells.cpu().numpy()[:length].view(np.uint32), int(status.cpu()[0])


def test_depth_sparse_wide_window_of_4098_tiles(gpu):
    """dp_offsets passes 2 to 17, the second block trip of dp_reduce and dp_scan, the partial last tile; then pieces
    across the tiles 255|256 and 4,095|4,096 and one long interval over the whole window."""
    c = S.depth_sparse()
    want, W = c["want"], c["window"][2]
    got = device_depth(D.flatten(c["records"]), c["window"], c["contig_len"], S.DP_PRM, gpu)
    assert W == SH["dp_window"] and (got == want).all(), np.nonzero(got != want)[0][:10]
    part, pieces = S.depth_sparse_part(W), S.depth_sparse_pieces(W)
    whist, wlong, wrows = S.stats_np(want, part, pieces, 2)
    hist, long_hist, rows = device_stats(got, part, pieces, 2, gpu)
    assert (hist == whist).all() and (long_hist == wlong).all() and rows == wrows


def test_depth_150000_distinct_records(gpu):
    f, window, clen = S.depth_many()
    want = S.depth_np(f, window, clen, S.DP_PRM)
    got = device_depth(f.dp(), window, clen, S.DP_PRM, gpu)
    assert f.n == SH["dp_records"] and (got == want).all(), np.nonzero(got != want)[0][:10]


def test_depth_33068_pieces_and_three_long_rows(gpu):
    depth, part, pieces, n_long = S.depth_pieces()
    whist, wlong, wrows = S.stats_np(depth, part, pieces, n_long)
    hist, long_hist, rows = device_stats(depth, part, pieces, n_long, gpu)
    assert len(pieces) == SH["dp_pieces"] and (hist == whist).all() and (long_hist == wlong).all()
    assert rows == wrows, [k for k, (a, b) in enumerate(zip(rows, wrows)) if a != b][:10]


def test_depth_at_the_end_of_a_contig_of_2_31_minus_1(gpu):
    c = S.depth_high()
    on = D.params(include_deletions=True)
    for window in c["windows"]:
        want = D.depth(c["records"], window, c["contig_len"], on)[0]
        assert (device_depth(D.flatten(c["records"]), window, c["contig_len"], on, gpu) == want).all()
        got, status = depth_twin(gpu, D.flatten(c["records"]), window, c["contig_len"], on)
        assert status == 0 and (got == want).all()
        # a base beyond the contig: the host-pointer call refuses the record, the _dev twin reports and clips it
        more = c["records"] + [c["past"]]
        with pytest.raises(fcship.FcsError, match="aligned base beyond its contig"):
            device_depth(D.flatten(more), window, c["contig_len"], on, gpu)
        got, status = depth_twin(gpu, D.flatten(more), window, c["contig_len"], on)
        clipped, beyond = D.depth(more, window, c["contig_len"], on)
        assert beyond and status == fcship.FCSDP_STATUS_REF and (got == clipped).all() and clipped.sum() > want.sum()


# ------------------------------------------------------------------ ug
def device_sites(arrays, window, contig_len, ref_window, gpu, max_sites=None):
    ref, start, length = window
    return fcship.ug_sites(arrays, (ref, start, length, contig_len), ref_window, TABLE, 17, max_sites, device=gpu)


class Twin:
    """fcsug_sites_dev on a caller stream with device-resident inputs; a batch is uploaded once and may be queued again
    with other positions."""

    def __init__(self, gpu):
        import torch
        self.torch, self.gpu = torch, gpu
        self.dev = torch.device(f"cuda:{gpu}")
        self.stream = torch.cuda.Stream(device=self.dev)
        with torch.cuda.stream(self.stream):
            self.table = to_dev(torch, self.dev, TABLE)
        self.keep = []

    def upload(self, arrays):
        arrays = fcship.ug_arrays(*arrays)
        with self.torch.cuda.stream(self.stream):
            t = [to_dev(self.torch, self.dev, a) for a in arrays]
        return t, (len(arrays[0]), len(arrays[4]), len(arrays[7]))

    def queue(self, batch, window, contig_len, ref_window, max_sites=None, pos=None):
        """Queues one call; returns (sites, n_sites, status) tensors to read after the stream's end."""
        torch = self.torch
        t, (n, n_cigar, n_bases) = batch
        ref, start, length = window
        max_sites = length if max_sites is None else max_sites
        with torch.cuda.stream(self.stream):
            if pos is not None:
                t = t[:2] + [to_dev(torch, self.dev, np.ascontiguousarray(pos, np.int32))] + t[3:]
            flag, ref_id, p, mapq, cigar, cigar_off, bases, qual, base_off, absent = [x.data_ptr() for x in t]
            b = fcship.UgBatch(n, flag, ref_id, p, mapq, cigar, cigar_off, n_cigar, bases, qual, base_off, n_bases, absent)
            seq = to_dev(torch, self.dev, np.ascontiguousarray(ref_window, np.uint8))
            sites = torch.full((80 * max(max_sites, 1),), 0x55, dtype=torch.uint8, device=self.dev)
            found = torch.full((1,), -7, dtype=torch.int64, device=self.dev)
            status = torch.zeros(1, dtype=torch.int32, device=self.dev)
            need = fcship.lib.fcsug_workspace_bytes(n, length)
            ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
            w, prm = fcship.UgWindow(ref, 0, start, length, contig_len), fcship.UgParams(17)
            fcship.check(fcship.lib.fcsug_sites_dev(self.gpu, C.addressof(b), C.addressof(prm), C.addressof(w), seq.data_ptr(),
                                                    self.table.data_ptr(), sites.data_ptr(), max_sites, found.data_ptr(),
                                                    ws.data_ptr(), need, status.data_ptr(), C.c_void_p(self.stream.cuda_stream)))
        self.keep.append((t, seq, ws))
        return sites, found, status

    @staticmethod
    def read(out, written=None):
        sites, found, status = out
        found = int(found.cpu()[0])
        rows = sites.cpu().numpy().view(fcship.UG_SITE)
        return rows[:found if written is None else written], found, int(status.cpu()[0])


def same_sites(got, want):
    assert len(got) == len(want), (len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert not len(bad), (bad[:5], got[bad[:2]], want[bad[:2]])


def test_ug_sparse_wide_window_of_2050_tiles(gpu):
    """ug_slots passes 2 to 9, the second block trip of ug_count and ug_tile with cells zeroed again, the partial last
    tile: the host-pointer call at start 0, the _dev twin at an odd start; then max_sites that just fits, and one less."""
    c = S.ug_sparse(0)
    W = c["window"][2]
    want = S.site_rows(c["want"], fcship.UG_SITE)
    seq = np.frombuffer(c["refseq"][:W].encode(), np.uint8)
    same_sites(device_sites(U.flatten(c["records"]), c["window"], len(c["refseq"]), seq, gpu), want)
    c = S.ug_sparse(1001)
    want = S.site_rows(c["want"], fcship.UG_SITE)
    seq = np.frombuffer(c["refseq"][1001:1001 + W].encode(), np.uint8)
    twin = Twin(gpu)
    batch = twin.upload(U.flatten(c["records"]))
    whole = twin.queue(batch, c["window"], len(c["refseq"]), seq)
    fits = twin.queue(batch, c["window"], len(c["refseq"]), seq, max_sites=len(want))
    short = twin.queue(batch, c["window"], len(c["refseq"]), seq, max_sites=len(want) - 1)
    twin.stream.synchronize()
    for out in (whole, fits):
        rows, found, status = Twin.read(out)
        assert status == 0 and found == len(want)
        same_sites(rows, want)
    rows, found, status = Twin.read(short, written=len(want) - 1)
    assert status == fcship.FCSUG_STATUS_SITES and found == len(want)
    same_sites(rows, want[:-1])


@pytest.fixture(scope="module")
def many():
    c = S.ug_many()
    _, start, W = c["windows"][0]
    c["seq"] = c["refs"][0][start:start + W]
    return c


def test_ug_524549_distinct_records(gpu, many):
    """ug_offsets passes 2 to 9 over tile maxima that differ, the second grid trip of ug_span and ug_scan, the binary
    searches over distinct max_end and key values."""
    f, window = many["flat"], many["windows"][0]
    want = S.sites_np(f, window, many["refs"][0], fcship.UG_SITE)
    assert f.n == SH["ug_records"] and len(want) >= 50000
    same_sites(device_sites(f.ug(), window, many["contig_len"], many["seq"], gpu), want)


def test_ug_positions_out_of_order_across_a_scan_pass(gpu, many):
    f, window = many["flat"], many["windows"][0]
    twin = Twin(gpu)
    batch = twin.upload(f.ug())
    outs = []
    for a, b in S.ug_swaps():
        pos = f.pos.copy()
        pos[a], pos[b] = pos[b], pos[a]
        outs.append(twin.queue(batch, window, many["contig_len"], many["seq"], max_sites=1000, pos=pos))
    twin.stream.synchronize()
    for (a, b), out in zip(S.ug_swaps(), outs):
        rows, found, status = Twin.read(out)
        assert status == fcship.FCSUG_STATUS_ORDER and found == 0, (a, b, status, found)
        assert (out[0].cpu().numpy() == 0x55).all(), (a, b)


def test_ug_every_third_record_on_another_contig(gpu):
    c = S.ug_many(interleaved=True)
    f = c["flat"]
    for window in c["windows"]:
        ref, start, W = window
        want = S.sites_np(f, window, c["refs"][ref], fcship.UG_SITE)
        assert len(want) > 20000
        same_sites(device_sites(f.ug(), window, c["contig_len"], c["refs"][ref][start:start + W], gpu), want)


def test_ug_at_the_end_of_a_contig_of_2_31_minus_1(gpu):
    c = S.ug_high()
    refseq = c["refseq"]
    twin = Twin(gpu)
    good, more = twin.upload(U.flatten(c["records"])), sorted(c["records"] + [c["past"]], key=lambda r: r["pos"])
    past = twin.upload(U.flatten(more))
    outs = []
    for window in c["windows"]:
        _, start, n = window
        seq = np.frombuffer(refseq[start:start + n].encode(), np.uint8)
        want = S.site_rows(U.sites(c["records"], window, refseq, S.TAB)[0], fcship.UG_SITE)
        same_sites(device_sites(U.flatten(c["records"]), window, len(refseq), seq, gpu), want)
        with pytest.raises(fcship.FcsError, match="aligned base beyond its contig"):
            device_sites(U.flatten(more), window, len(refseq), seq, gpu)
        clipped, beyond = U.sites(more, window, refseq, S.TAB)
        assert beyond and len(want) > 60
        outs.append((twin.queue(good, window, len(refseq), seq), want, 0))
        outs.append((twin.queue(past, window, len(refseq), seq), S.site_rows(clipped, fcship.UG_SITE), fcship.FCSUG_STATUS_REF))
    twin.stream.synchronize()
    for out, want, want_status in outs:
        rows, found, status = Twin.read(out)
        assert status == want_status and found == len(want)
        same_sites(rows, want)


# ------------------------------------------------------------------ markdup
@pytest.mark.parametrize("shape,seed", [("md_ends", 102), ("md_all", 103)])
def test_markdup_past_the_first_grid_trip(gpu, shape, seed):
    """131,125 records: the second trip of md_ends; 524,549: the second trip of every kernel with a lane per record, and
    the rocPRIM sorts at a production size.  Fragments and pairs, mates and duplicate sets anywhere in the batch."""
    f = S.FlatDup(SH[shape], seed)
    want, want_st = S.markdup_np(f)
    dup, st = fcship.dup_mark(f.arrays(), f.n_ref, f.n_lib, device=gpu)
    assert f.n == SH[shape] and (dup == want).all(), np.nonzero(dup != want)[0][:10]
    assert st == want_st


def test_markdup_keys_that_differ_in_a_top_bit(gpu):
    """The 11-bit library, 21-bit contig and 31-bit u5 fields to their top bits, and the pair sort's 53 then 64 bits:
    alone, and behind the random batch so that the sorts see them among ordinary keys."""
    records = S.markdup_high_bits()
    for batch in (records, S.markdup_appended(M.random_batch(), records)):
        dup, st = fcship.dup_mark(M.flatten(batch), S.MD_MAX_REFS, S.MD_MAX_LIBS, device=gpu)
        want = M.expected(batch)
        assert list(dup) == want, [i for i, (a, b) in enumerate(zip(dup, want)) if a != b][:20]
        assert st == M.stats(batch)


# ------------------------------------------------------------------ bqsr
@pytest.fixture(scope="module")
def bq_world(gpu):
    refs, known = S.bq_world()
    with fcship.bq_ref(*B.flat_reference(refs, known), device=gpu) as ref:
        yield refs, known, ref


@pytest.mark.parametrize("n_rg", SH["bq_rg"])
def test_bqsr_six_and_ninety_read_groups(gpu, bq_world, n_rg):
    """From six read groups on bq_fold strides over the cells and folds fewer than 16 replicas: 14 at 6, 1 at 90."""
    refs, known, ref = bq_world
    records, grouped, ctx, cyc = S.bq_count_case(refs, known, 1200, n_rg, 115, B.random_batch.__defaults__[-1])
    for batch in (records, grouped):
        got = fcship.bq_count(ref, B.flatten(batch), n_rg)
        assert (got[0] == ctx).all() and (got[1] == cyc).all()


def test_bqsr_count_of_67591_short_records(gpu, bq_world):
    """A slice of 34 records per block: the LDS path (grouped) and the global path (interleaved)."""
    refs, known, ref = bq_world
    records, grouped, ctx, cyc = S.bq_count_case(refs, known, SH["bq_count"], 3, 112, (1, 2, 3))
    for batch in (grouped, records):
        got = fcship.bq_count(ref, B.flatten(batch), 3)
        assert (got[0] == ctx).all() and (got[1] == cyc).all()


def test_bqsr_apply_of_8205_records(gpu, bq_world):
    """The second grid trip of bq_apply; applied and copied records; nothing outside [off[0], off[n]) is written."""
    refs, _, _ = bq_world
    records = B.random_batch(seed=113, n=SH["bq_apply"], n_rg=6, refs=refs, lengths=(1, 2, 30))
    tables = S.bq_tables(6)
    arrays = fcship.bq_arrays(*B.flatten(records, 3))
    out = np.full(len(arrays[7]) + 5, 0xEE, np.uint8)
    fcship.bq_apply(arrays, *tables, device=gpu, out=out)
    assert B.unflatten_quals(records, out, 3) == B.apply(records, *tables)
    assert (out[:3] == 0xEE).all() and (out[-5:] == 0xEE).all()


def test_bqsr_check_finds_a_bad_read_group_in_its_second_grid_trip(gpu):
    import torch
    arrays = fcship.bq_arrays(*S.bq_check_batch(3))
    n = len(arrays[0])
    tables = S.bq_tables(3)
    dev = torch.device("cuda", gpu)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        t = [to_dev(torch, dev, a) for a in arrays]
        flag, ref_id, pos, mapq, rg, cigar, cigar_off, bases, qual, base_off, absent = [x.data_ptr() for x in t]
        b = fcship.BqBatch(n, flag, ref_id, pos, mapq, rg, cigar, cigar_off, n, bases, qual, base_off, n, absent)
        tabs = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in tables]
        out = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        status = torch.full((2,), -1, dtype=torch.int32, device=dev)
        fcship.check(fcship.lib.fcsbq_apply_dev(gpu, C.addressof(b), 3, tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(),
                                                out.data_ptr(), status.data_ptr(), C.c_void_p(stream.cuda_stream)))
        good = t[:4] + [to_dev(torch, dev, np.minimum(arrays[4], 2))] + t[5:]      # the same batch with every read group in range
        b2 = fcship.BqBatch(n, flag, ref_id, pos, mapq, good[4].data_ptr(), cigar, cigar_off, n, bases, qual, base_off, n, absent)
        out2 = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        fcship.check(fcship.lib.fcsbq_apply_dev(gpu, C.addressof(b2), 3, tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(),
                                                out2.data_ptr(), status[1:].data_ptr(), C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    assert status.cpu().tolist() == [fcship.FCSBQ_STATUS_FIELD, 0]
    assert (out.cpu().numpy() == 0xEE).all()
    # one base at Q30, cycle 1: the new quality is the table's
    rgs, letters = np.minimum(arrays[4], 2), arrays[7]
    want = np.array([B.new_quality(30, tables[0][g, 30], 0.0, tables[2][g, 30, 0]) for g in range(3)], np.uint8)[rgs]
    assert (out2.cpu().numpy() == want).all() and len(letters) == n
