"""The FMD seeding kernels past their first grid trip (falcon-genome_amd/csrc/fmd_seed.hip and
fmd_seeds.hip): fmd_scale_cases' batch A (65,540 reads: fmd_seed_order_kernel's second round, the third trip of
fmd_collect_kernel and fmd_seed_expand_kernel, fmd_seed_scan_kernel with 65 reads per lane and 15 empty lanes, and
more than 524,288 located rows for fmd_seed_locate_kernel) and batch B (524,545 rows for fmd_locate_kernel).  Every
expectation is the host index's answer for the whole batch (fcsg_fmd_seeds mode 0), which test_fmd_scale_cpu.py pins
to the host build of the kernels' per-read code; nothing is tiled from a smaller run."""
import ctypes as C

import numpy as np
import pytest

import fcship
import fmd_scale_cases as A
import fmd_seed_cases as S
import fmd_seeds_cases as F

pytestmark = pytest.mark.gpu

U, O, N = A.U, A.O, A.N_READS
FILL = 0x55


@pytest.fixture(scope="module")
def index8():
    occ, Carr, n_rows, sa, rows, ssa, flen = A.index(A.SA_INTV)
    h = fcship.fmd_index_create(occ, Carr, n_rows, sa, A.SA_INTV, rows, ssa, flen)
    yield h
    fcship.fmd_index_destroy(h)


@pytest.fixture(scope="module")
def want_bwa():
    """fcs_fmd_seed's output at bwa's parameters and the default max_mems: the deep reads are handed back."""
    mems5, mem_off = A.host()[:2]
    return A.flat(mems5, mem_off, A.sa_full(), dropped=A.kinds("deep"))


def assert_flat(got, want, dropped):
    mems, mem_off, pos, row_off, overflow, status = got
    assert status == fcship.FCS_OK
    assert list(np.nonzero(overflow)[0]) == sorted(dropped)
    assert np.array_equal(mem_off, want[1]) and np.array_equal(row_off, want[3])
    assert np.array_equal(mems, want[0]) and np.array_equal(pos, want[2])


def test_fused_through_the_aligners_hook(gpu):
    """fcsg_fmd_seeds mode 2 on a sampled index: one fcs_fmd_seed call over all of batch A crosses every cap at once.
    Every integer is the host's; the host collected the eight deep reads (2,700 and 145 SMEMs, above the default
    max_mems) and nothing else, located no row, and the call was not repeated."""
    want = A.host()
    got = A.seeds_np(A.ref(), A.batch_a(), F.FUSED, S.BWA, sa_intv=A.SA_INTV)
    for g, w in zip(got[:4], want[:4]):
        assert np.array_equal(g, w)
    assert got[4] == [len(A.kinds("deep")), 0, 0]


def test_fused_through_the_binding_multi_tile_round(gpu, index8):
    """min_len 1, max_mems 128: the read at O + 1 ranks 113 SMEMs over two tiles in its wave's second round, beside
    one-tile reads and an empty one."""
    mems5, mem_off = A.host(A.MIN1)[:2]
    deep = A.kinds("deep")
    want = A.flat(mems5, mem_off, A.sa_full(), dropped=deep)
    tm, tr = int(want[1][-1]), int(want[3][-1])
    assert want[1][O + 2] - want[1][O + 1] > 64
    got = fcship.fmd_seed(index8, *A.batch_a(), min_len=1, mem_cap=tm, row_cap=tr)
    assert_flat(got, want, deep)


def test_fused_through_the_binding_overflow_in_later_trips(gpu, index8):
    """max_mems 16: the planted reads past U and past O, and the deep reads, set overflow and have empty ranges; no
    other read does."""
    mems5, mem_off = A.host()[:2]
    dropped = sorted(A.kinds("deep") + A.kinds("over"))
    want = A.flat(mems5, mem_off, A.sa_full(), dropped=dropped)
    got = fcship.fmd_seed(index8, *A.batch_a(), max_mems=A.SMALL_MEMS)
    assert_flat(got, want, dropped)
    for r in dropped:
        assert got[1][r] == got[1][r + 1] and got[3][r] == got[3][r + 1]


def test_capacity_is_refused_by_every_trip(gpu, index8, want_bwa):
    """Exactly the totals: the host's content.  One SMEM or one row short: FCS_FMD_SEED_MORE with the true totals, and
    not a byte of mems / pos written, by the blocks of the later trips either."""
    want = want_bwa
    tm, tr = int(want[1][-1]), int(want[3][-1])
    assert tr > A.SH["fmd_seed_locate"]
    for mem_cap, row_cap in ((tm, tr - 1), (tm - 1, tr)):
        mems = np.zeros(tm, fcship.FMD_MEM)
        mems.view(np.uint8)[:] = FILL
        pos = np.zeros(tr, np.int64)
        pos.view(np.uint8)[:] = FILL
        got = fcship.fmd_seed(index8, *A.batch_a(), mem_cap=mem_cap, row_cap=row_cap, mems=mems, pos=pos)
        assert got[5] == fcship.FCS_FMD_SEED_MORE
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
        assert (mems.view(np.uint8) == FILL).all() and (pos.view(np.uint8) == FILL).all()
    got = fcship.fmd_seed(index8, *A.batch_a(), mem_cap=tm, row_cap=tr)
    assert_flat(got, want, A.kinds("deep"))


def slots_of(mems, n_mems):
    """(read, {qb, qe, s, k, l}) of the filled slots of mems[n, max_mems], read by read in slot order."""
    live = np.arange(mems.shape[1])[None, :] < n_mems[:, None]
    m = mems[live]
    return np.repeat(np.arange(len(n_mems)), n_mems), np.stack([m["qb"], m["qe"], m["s"], m["k"], m["l"]], 1).astype(np.int64)


def host_slots(n, max_mems, params=S.BWA):
    """The host's SMEMs of reads [0, n) without the reads with more than max_mems: (counts, read, rows)."""
    mems5, mem_off = A.host(params)[:2]
    c = np.diff(mem_off)[:n]
    over = c > max_mems
    keep = np.repeat(~over, c)
    return np.where(over, 0, c), over, np.repeat(np.arange(n), c)[keep], mems5[:mem_off[n]][keep]


def test_collect_second_trip_longest_first(gpu, index8):
    """fcs_fmd_collect on the first U + 17 reads, max_mems 16: 17 quads take a second read, under the call's
    longest-first order."""
    n = U + 17
    counts, over, read, rows = host_slots(n, A.SMALL_MEMS)
    assert over.sum() >= 4 and (counts > 0).sum() > n // 4
    mems, n_mems, overflow = fcship.fmd_collect(index8, *A.sub_batch(A.batch_a(), np.arange(n)), max_mems=A.SMALL_MEMS)
    assert np.array_equal(overflow != 0, over) and np.array_equal(n_mems, counts)
    got_read, got = slots_of(mems, n_mems)
    assert np.array_equal(got_read, read) and np.array_equal(got, rows)


def test_locate_second_trip(gpu, index8):
    """fcs_fmd_locate on batch B: 257 lanes take a second row, among them a row below 0, a row past the index and one
    beyond the step cap.  At max_steps 1 the rows two or more LF steps from a stored row are flagged, and only they."""
    b = A.batch_b()
    pos, status = fcship.fmd_locate(index8, b["rows"], max_steps=A.FAR_STEPS - 1)
    assert np.array_equal(status, b["status"])
    ok = status == fcship.FCS_FMD_LOCATED
    assert np.array_equal(pos[ok], b["pos"][ok])
    pos, status = fcship.fmd_locate(index8, b["rows"])
    bad = np.zeros(len(status), bool)
    bad[list(b["bad_at"])] = True
    assert np.array_equal(status, np.where(bad, fcship.FCS_FMD_BAD_ROW, fcship.FCS_FMD_LOCATED))
    assert np.array_equal(pos[~bad], b["pos"][~bad])


class Twin:
    """fcs_fmd_collect_dev and fcs_fmd_seed_dev on a caller stream: inputs, scratch and outputs are torch tensors on
    the device, every output byte and the scratch pre-filled."""

    def __init__(self, torch, gpu, handle, batch):
        self.torch, self.handle = torch, handle
        self.dev = torch.device(f"cuda:{gpu}")
        self.stream = torch.cuda.Stream(device=self.dev)
        self.n, self.max_q_len = len(batch[2]), int(batch[2].max())
        with torch.cuda.stream(self.stream):
            self.codes, self.q_off, self.q_len = (self.up(a) for a in batch)

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).copy()).to(self.dev)

    def filled(self, n_bytes, value=FILL):
        return self.torch.full((max(int(n_bytes), 1),), value, dtype=self.torch.uint8, device=self.dev)

    def collect(self, order, max_mems, params=S.BWA):
        n, torch = self.n, self.torch
        with torch.cuda.stream(self.stream):
            need = fcship.lib.fcs_fmd_collect_arena_bytes(n, self.max_q_len)
            arena, mems = self.filled(need, 0xA5), self.filled(n * max_mems * 32)
            n_mems, overflow = self.filled(4 * n), self.filled(4 * n)
            o = None if order is None else self.up(np.asarray(order, np.int32))
            P = fcship.FmdParams(params[0], min(params[1], 2**31 - 1), params[2], max_mems, params[3])
            fcship.check(fcship.lib.fcs_fmd_collect_dev(
                self.handle, self.codes.data_ptr(), len(self.codes), self.q_off.data_ptr(), self.q_len.data_ptr(),
                None if o is None else o.data_ptr(), n, self.max_q_len, C.addressof(P), arena.data_ptr(), need, mems.data_ptr(),
                n_mems.data_ptr(), overflow.data_ptr(), C.c_void_p(self.stream.cuda_stream)))
        self.stream.synchronize()
        return (mems.cpu().numpy().view(fcship.FMD_MEM).reshape(n, max_mems), n_mems.cpu().numpy().view(np.int32),
                overflow.cpu().numpy().view(np.int32))

    def seed(self, order, max_mems, mem_cap, row_cap, room, params=S.BWA, max_occ=500):
        """mems / pos have `room` entries beyond the capacities."""
        n, torch = self.n, self.torch
        with torch.cuda.stream(self.stream):
            need = fcship.lib.fcs_fmd_seed_workspace_bytes(n, self.max_q_len, max_mems, row_cap)
            ws = self.filled(need, 0xA5)
            mems, pos = self.filled(32 * (mem_cap + room)), self.filled(8 * (row_cap + room))
            mem_off, row_off, overflow = self.filled(8 * (n + 1)), self.filled(8 * (n + 1)), self.filled(4 * n)
            o = None if order is None else self.up(np.asarray(order, np.int32))
            P = fcship.FmdSeedParams(fcship.FmdParams(params[0], min(params[1], 2**31 - 1), params[2], max_mems, params[3]),
                                     max_occ, 0)
            fcship.check(fcship.lib.fcs_fmd_seed_dev(
                self.handle, self.codes.data_ptr(), len(self.codes), self.q_off.data_ptr(), self.q_len.data_ptr(),
                None if o is None else o.data_ptr(), n, self.max_q_len, C.addressof(P), ws.data_ptr(), need, mems.data_ptr(),
                mem_cap, mem_off.data_ptr(), pos.data_ptr(), row_cap, row_off.data_ptr(), overflow.data_ptr(),
                C.c_void_p(self.stream.cuda_stream)))
        self.stream.synchronize()
        return (mems.cpu().numpy().view(fcship.FMD_MEM), mem_off.cpu().numpy().view(np.int64), pos.cpu().numpy().view(np.int64),
                row_off.cpu().numpy().view(np.int64), overflow.cpu().numpy().view(np.int32))


def by_content(read, rows):
    """The rows of each read in an order that depends on their content alone (the device's is emission order)."""
    order = np.lexsort((rows[:, 4], rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0], read))
    return read[order], rows[order]


ORDERS = {"as_given": lambda q_len: None, "shortest_first": lambda q_len: np.argsort(q_len, kind="stable").astype(np.int32)}


@pytest.fixture(scope="module")
def twin(gpu, index8):
    import torch
    return Twin(torch, gpu, index8, A.batch_a())


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_collect_dev_quads_reuse_their_stacks(gpu, twin, order):
    """fcs_fmd_collect_dev over batch A.  Without an order, read r + U follows read r in its quad: a 30-mer after the
    150-base poly-A and ACG reads whose stacks ran 100 deep, and the other way round; shortest first, every quad's
    reads grow.  The SMEMs are the host's (in emission order: compared by content), and no slot past n_mems[r] of a
    read that fits is written."""
    max_mems = S.MAX_MEMS_DEFAULT
    counts, over, read, rows = host_slots(N, max_mems)
    assert list(np.nonzero(over)[0]) == A.kinds("deep")
    mems, n_mems, overflow = twin.collect(ORDERS[order](A.batch_a()[2]), max_mems)
    assert np.array_equal(overflow != 0, over) and set(overflow) == {0, 1} and np.array_equal(n_mems, counts)
    got_read, got = by_content(*slots_of(mems, n_mems))
    want_read, want = by_content(read, rows)
    assert np.array_equal(got_read, want_read) and np.array_equal(got, want)
    untouched = (np.arange(max_mems)[None, :] >= n_mems[:, None]) & ~over[:, None]
    assert (mems.view(np.uint8).reshape(N, max_mems, 32)[untouched] == FILL).all()


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_seed_dev_writes_the_totals_and_nothing_beyond(gpu, twin, want_bwa, order):
    """fcs_fmd_seed_dev over batch A with capacities of exactly the totals: the host's content in [0, total) of mems /
    pos, and the 64 entries beyond as they were."""
    want = want_bwa
    tm, tr = int(want[1][-1]), int(want[3][-1])
    mems, mem_off, pos, row_off, overflow = twin.seed(ORDERS[order](A.batch_a()[2]), S.MAX_MEMS_DEFAULT, tm, tr, room=64)
    assert list(np.nonzero(overflow)[0]) == A.kinds("deep") and set(overflow) == {0, 1}
    assert np.array_equal(mem_off, want[1]) and np.array_equal(row_off, want[3])
    assert np.array_equal(mems[:tm], want[0]) and np.array_equal(pos[:tr], want[2])
    assert (mems[tm:].view(np.uint8) == FILL).all() and (pos[tr:].view(np.uint8) == FILL).all()
