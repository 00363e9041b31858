"""The queue-fed column kernel (phmm6, phmm_cols.h) bitwise against the
single-stream column kernel (phmm5) on the same batch, and against the oracle.
phmm5 and phmm6 share their stream body (cols1_stream), so each batch's
`single` run is in turn held bitwise to the packed kernel (phmm4), which shares
no code with them.

FCSHIP_COLS=queue|single|packed forces one kernel for every column class and
FCSHIP_QUEUE_WAVES caps the workgroups of a queue launch (1: one wave works
through the whole class, so each of its four streams runs a quarter of the
class's pairs back to back and refills the slots of its circular segment
table); both are read once per process, so each run of the library is a
child process.  The `single` run of a batch is made once and shared.  A
rescued pair is one whose result changes when the fp64 rescue is switched off.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import fcship
from test_pairhmm_gpu import check_parity, mutate, rand_read
from test_pairhmm_single_gpu import edge_batch

pytestmark = pytest.mark.gpu

LIBDIR = os.path.dirname(os.path.abspath(fcship.__file__))

CHILD = (
    "import sys; sys.path.insert(0, %r)\n"
    "import ctypes as C, numpy as np, fcship\n"
    "d = np.load(sys.argv[1])\n"
    "p = fcship.PhmmPairs(**{f: d[f] for f in d.files})\n"
    "out = fcship.phmm_compute_pairs(p)\n"
    "n = C.c_int64()\n"
    "fcship.lib.fcs_phmm_last_rescued(C.byref(n))\n"
    "raw = fcship.phmm_compute_pairs(p, rescue=False)\n"
    "np.savez(sys.argv[2], out=out, raw=raw, rescued=np.int64(n.value))\n"
    "print('DONE')\n"
) % LIBDIR

# Plan API: one schedule, two forwards, then schedule and forward again; `out`
# holds a sentinel before every forward, so a pair that no wave took keeps it.
CHILD_PLAN = (
    "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import numpy as np, torch, fcship, bench\n"
    "d = np.load(sys.argv[1])\n"
    "p = fcship.PhmmPairs(**{f: d[f] for f in d.files})\n"
    "dev = torch.device('cuda', 0)\n"
    "b, keep = bench.phmm_dev_batch(p, dev)\n"
    "out = torch.empty(p.n_pairs, dtype=torch.float64, device=dev)\n"
    "plan = fcship.C.c_void_p()\n"
    "fcship.check(fcship.lib.fcs_phmm_plan_create(0, p.n_pairs, fcship.C.byref(plan)))\n"
    "opts = fcship.phmm_opts(device=0)\n"
    "sp = torch.cuda.current_stream(dev).cuda_stream\n"
    "B, O = fcship.C.byref(b), fcship.C.byref(opts)\n"
    "res, cnt = [], []\n"
    "def forward():\n"
    "    out.fill_(12345.0)\n"
    "    fcship.check(fcship.lib.fcs_phmm_dev_forward(plan, B, out.data_ptr(), O, sp))\n"
    "    fcship.check(fcship.lib.fcs_phmm_dev_rescue(plan, B, out.data_ptr(), O, sp))\n"
    "    n = fcship.C.c_int64()\n"
    "    fcship.check(fcship.lib.fcs_phmm_plan_rescue_count(plan, sp, fcship.C.byref(n)))\n"
    "    cnt.append(n.value)\n"
    "    res.append(out.cpu().numpy().copy())\n"
    "fcship.check(fcship.lib.fcs_phmm_dev_schedule(plan, B, sp))\n"
    "forward()\n"
    "forward()\n"
    "fcship.check(fcship.lib.fcs_phmm_dev_schedule(plan, B, sp))\n"
    "forward()\n"
    "fcship.lib.fcs_phmm_plan_destroy(plan)\n"
    "np.savez(sys.argv[2], res=np.stack(res), cnt=np.array(cnt, np.int64))\n"
    "print('DONE')\n"
) % (LIBDIR, os.path.dirname(LIBDIR))


def child(code, src, dst, cols, waves):
    env = dict(os.environ, FCSHIP_COLS=cols)
    env.pop("FCSHIP_QUEUE_WAVES", None)
    env.pop("FCSHIP_STREAM_K", None)
    if waves:
        env["FCSHIP_QUEUE_WAVES"] = str(waves)
    r = subprocess.run([sys.executable, "-c", code, str(src), str(dst)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert "DONE" in r.stdout, r.stderr[-3000:]
    return np.load(dst)


def save_batch(path, p):
    src = path / "batch.npz"
    if not src.exists():
        np.savez(src, **{f: getattr(p, f) for f in p.__dataclass_fields__})
    return src


def same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_queue_against_single(path, p, waves, ref=None):
    """The queue run inside the oracle's parity bar, bitwise the single-stream
    kernel's outputs with and without the rescue (NaN patterns included), the
    same rescued set and rescue count.  ref: the batch's `single` run, if it
    was made already; when it is made here, it is checked bitwise (outputs and
    rescue count) against a `packed` run.  Returns (out, the single run)."""
    src = save_batch(path, p)
    if ref is None:
        d = child(CHILD, src, path / "single.npz", "single", 0)
        ref = d["out"], d["raw"], int(d["rescued"])
        # phmm5 and phmm6 share their step; phmm4 (packed) shares no code with them
        d = child(CHILD, src, path / "packed.npz", "packed", 0)
        assert same_bits(d["raw"], ref[1]), np.flatnonzero(d["raw"].view(np.uint64) != ref[1].view(np.uint64))[:8]
        assert same_bits(d["out"], ref[0]), np.flatnonzero(d["out"].view(np.uint64) != ref[0].view(np.uint64))[:8]
        assert int(d["rescued"]) == ref[2], (int(d["rescued"]), ref[2])
    d = child(CHILD, src, path / f"queue_{waves}.npz", "queue", waves)
    out, raw, n = d["out"], d["raw"], int(d["rescued"])
    sout, sraw, sn = ref
    assert same_bits(raw, sraw), np.flatnonzero(raw.view(np.uint64) != sraw.view(np.uint64))[:8]
    assert same_bits(out, sout), np.flatnonzero(out.view(np.uint64) != sout.view(np.uint64))[:8]
    resc, sresc = out.view(np.uint64) != raw.view(np.uint64), sout.view(np.uint64) != sraw.view(np.uint64)
    assert np.array_equal(resc, sresc) and n == sn, (n, sn)
    check_parity(p, out, False)
    return out, ref


@pytest.fixture(scope="module")
def edge(tmp_path_factory):
    """edge_batch() and its `single` run, shared by the two grid sizes."""
    return {"path": tmp_path_factory.mktemp("queue_edge"), "p": edge_batch(), "ref": None}


@pytest.mark.parametrize("waves", [0, 1])
def test_queue_class_edges(gpu, edge, waves):
    """H at and beside every class edge, R from 33 to 160, N bases, a haplotype
    handed back and fp32 underflows that reach the rescue: with the default
    grid (most waves find their class exhausted at the first dequeue) and with
    one wave per class (every pair of a class through the same wave)."""
    out, edge["ref"] = check_queue_against_single(edge["path"], edge["p"], waves, edge["ref"])
    sout, sraw, _ = edge["ref"]
    assert (sout.view(np.uint64) != sraw.view(np.uint64)).sum() > 0, "the fp64 rescue must run on some streamed pairs"


def test_queue_slot_reuse_and_ring_residues(gpu, tmp_path):
    """One class (H = 250), 4 x 16 x 3 + 5 = 197 pairs, R cycling over 33 .. 81,
    one wave: each of its four streams takes about 49 pairs, so every slot of
    the circular segment table is refilled three times, and (R + 2) mod 48
    takes every residue, so pair boundaries, V rows and Z rows land on every
    slot of the ring."""
    rng = np.random.default_rng(6197)
    hap = rng.choice(np.frombuffer(b"ACGT", np.uint8), 250)
    reads = []
    for i in range(197):
        R = 33 + i % 49
        rd = list(rand_read(rng, R, n_frac=0.01))
        rd[0] = mutate(rng, hap, R)
        reads.append(tuple(rd))
    p = fcship.make_pairs(reads, [hap])
    assert p.n_pairs == 4 * 16 * 3 + 5
    check_queue_against_single(tmp_path, p, 1)


def stream_of_position(n, r_of_stream):
    """Which stream of a single wave takes each of the first n positions of a
    class, by the kernel's rules (phmm_cols.h, phmm6_kernel): positions 0..3
    go to streams 0..3 at row 0; at every block top (16 rows) the streams
    asked for one block ago take the next positions in stream order, each pair
    starting at max(end of the stream's last pair, block top + 32); then every
    stream with its end less than 32 + 48 rows after the block top asks."""
    gend = [r_of_stream(s) + 2 for s in range(4)]
    owner, pend, t0 = [0, 1, 2, 3], [], 0
    while len(owner) < n:
        for s in pend:
            owner.append(s)
            gend[s] = max(gend[s], t0 + 32) + r_of_stream(s) + 2
        pend = [s for s in range(4) if gend[s] < t0 + 32 + 48]
        t0 += 16
    return owner[:n]


def test_queue_streams_diverge(gpu, tmp_path):
    """One class, one wave; reads of R = 160 and R = 33 placed so that stream 0
    of the wave gets only long reads and the other three only short ones: the
    read length of the pair at position q of the class is chosen by the stream
    that stream_of_position() says will take it.  Dequeues then serve one, two
    or three streams at a time, and stream 0 runs hundreds of rows past the
    others.  The placement survives the schedule because the in-class key is
    the haplotype length in steps of 16: one haplotype puts every pair in one
    bin, and inside a bin the scatter kernel ranks the pairs by an LDS atomic
    per thread, thread i holding pair i; the 64 pairs here are one wavefront,
    whose lanes the atomic serves in lane order, so position q is pair q.  (The
    assertions do not depend on that order or on the simulation, only the
    coverage does.)"""
    rng = np.random.default_rng(6064)
    hap = rng.choice(np.frombuffer(b"ACGT", np.uint8), 230)
    owner = stream_of_position(64, lambda s: 160 if s == 0 else 33)
    assert 4 <= owner.count(0) <= 12 and owner.count(1) > 12
    reads = []
    for i in range(64):
        R = 160 if owner[i] == 0 else 33
        rd = list(rand_read(rng, R, n_frac=0.01))
        rd[0] = mutate(rng, hap, R)
        reads.append(tuple(rd))
    p = fcship.make_pairs(reads, [hap])
    check_queue_against_single(tmp_path, p, 1)


@pytest.mark.parametrize("waves", [0, 1])
def test_queue_ragged_class_counts(gpu, tmp_path, waves):
    """1, 3, 5 and 65 pairs in four classes (C = 19, 17, 15, 11), the other
    four classes empty: every wave of an empty class leaves at its first
    dequeue, a wave runs with one, three and all four streams filled."""
    rng = np.random.default_rng(6505)
    reads, haps, pairs = [], [], []
    for H, n in ((300, 1), (270, 3), (230, 5), (170, 65)):
        haps.append(rng.choice(np.frombuffer(b"ACGT", np.uint8), H))
        for _ in range(n):
            R = int(rng.integers(33, 152))
            rd = list(rand_read(rng, R))
            rd[0] = mutate(rng, haps[-1], R)
            pairs.append((len(reads), len(haps) - 1))
            reads.append(tuple(rd))
    p = fcship.make_pairs(reads, haps, pairs=pairs)
    out, (sout, _, _) = check_queue_against_single(tmp_path, p, waves)
    assert not np.isnan(sout).any() and not np.isnan(out).any()


def test_queue_two_pairs(gpu, tmp_path):
    """A batch of 2 pairs in all."""
    rng = np.random.default_rng(6002)
    hap = rng.choice(np.frombuffer(b"ACGT", np.uint8), 200)
    reads = []
    for R in (101, 40):
        rd = list(rand_read(rng, R))
        rd[0] = mutate(rng, hap, R)
        reads.append(tuple(rd))
    p = fcship.make_pairs(reads, [hap])
    assert p.n_pairs == 2
    out, (sout, _, _) = check_queue_against_single(tmp_path, p, 0)
    assert not np.isnan(sout).any() and not np.isnan(out).any()


def test_queue_counter_reset(gpu, tmp_path):
    """Plan API on a 300-pair batch: schedule, forward twice, schedule and
    forward again.  A queue head left over from the previous pass would leave
    pairs unwritten (the sentinel survives); all three outputs are bit-equal,
    hold no sentinel, and match the single-stream kernel's and the packed
    kernel's."""
    rng = np.random.default_rng(6300)
    haps = [rng.choice(np.frombuffer(b"ACGT", np.uint8), H) for H in (180, 240, 290)]
    reads = []
    for i in range(100):
        R = int(rng.integers(33, 152))
        rd = list(rand_read(rng, R, n_frac=0.01))
        if i % 9:
            rd[0] = mutate(rng, haps[i % 3], R)
        else:  # unrelated, Q40, gap 60: underflows the fp32 pass, so the rescue count is not zero
            rd[1][:] = 40
            rd[2][:] = rd[3][:] = 60
        reads.append(tuple(rd))
    p = fcship.make_pairs(reads, haps)
    assert p.n_pairs == 300
    src = save_batch(tmp_path, p)
    q = child(CHILD_PLAN, src, tmp_path / "plan_queue.npz", "queue", 0)
    s = child(CHILD_PLAN, src, tmp_path / "plan_single.npz", "single", 0)
    res, cnt = q["res"], q["cnt"]
    assert not (res == 12345.0).any(), np.argwhere(res == 12345.0)[:8]
    assert same_bits(res[0], res[1]) and same_bits(res[0], res[2])
    assert cnt[0] > 0 and cnt[0] == cnt[1] == cnt[2], cnt
    assert same_bits(res[0], s["res"][0]) and cnt[0] == s["cnt"][0]
    k = child(CHILD_PLAN, src, tmp_path / "plan_packed.npz", "packed", 0)
    assert same_bits(res[0], k["res"][0]) and cnt[0] == k["cnt"][0]
    check_parity(p, res[0], False)
