"""fcsir_score on the device (include/fcsir.h, csrc/indel.hip) against the
restatement of tests/ir_cases.py, exactly, at the smallest shapes that can go
wrong; the _dev twin's status bits; and `fcs-genome indel` writing the same
bytes with indel.gpu=true and indel.gpu=false.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fcship
import host_lib as H
import ir_cases as I

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check(bins, gpu, **kw):
    best, off = fcship.ir_score(I.flat(bins, **kw), device=gpu)
    want_best, want_off = I.expected(bins)
    assert np.array_equal(best, want_best), (best[:20], want_best[:20])
    assert np.array_equal(off, want_off), (off[:20], want_off[:20])
    return best, off


def rnd(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def quals(rng, n):
    return rng.integers(1, 94, n).astype(np.uint8)


def edge_bins():
    rng = np.random.default_rng(5)
    bins = []
    bins.append(([[2]], [([2], [30], 0), ([1], [30], 0), ([4], [30], 0)]))                       # L = 1 with len = 1
    s = rnd(rng, 37)
    bins.append(([s], [(s.copy(), quals(rng, 37), 0), (rnd(rng, 37), quals(rng, 37), 0)]))         # L = len
    bins.append(([rnd(rng, 20)], [(rnd(rng, 31), quals(rng, 31), o) for o in (0, 3, 19, 20, 500)]))  # L > len: orig only
    for cands in (63, 64, 65, 129):
        s = rnd(rng, cands + 6)
        reads = [(s[o:o + 7].copy(), quals(rng, 7), 0) for o in (0, cands - 2, cands - 1)] + [(rnd(rng, 7), quals(rng, 7), 1)]
        bins.append(([s], reads))
    s = rnd(rng, 100)
    bins.append(([s, rnd(rng, 71)], [(rnd(rng, L), quals(rng, L), L % 40) for L in range(1, 71)]))   # L = 1 .. 70
    s = rnd(rng, 60)
    bins.append(([s], [(rnd(rng, 12), quals(rng, 12), o) for o in (49, 55, 60, 61, 4000, I.ORIG_MAX)]))  # orig beyond len - L
    # a tie at orig against a smaller offset, and a tie of two non-orig offsets: a period-5 sequence
    s = np.tile(np.array([0, 1, 2, 3, 3], np.uint8), 8)
    r = s[5:17].copy()
    bins.append(([s], [(r, quals(rng, 12), 10), (r, quals(rng, 12), 15), (r, quals(rng, 12), 7), (r, quals(rng, 12), 39)]))
    s, r = rnd(rng, 50), rnd(rng, 20)
    s[[3, 9, 30]] = 4
    r[[0, 7, 19]] = 4
    bins.append(([s], [(r, quals(rng, 20), 3), (np.full(20, 4, np.uint8), quals(rng, 20), 0)]))      # code 4 in both
    bins.append(([rnd(rng, 50)], [(rnd(rng, 20), np.zeros(20, np.uint8), 9)]))                      # every q = 0
    bins.append(([np.zeros(600, np.uint8)], [(np.ones(512, np.uint8), np.full(512, 93, np.uint8), 50)]))  # L = 512, all differ
    bins.append(([rnd(rng, 30)], []))                                                             # no reads
    bins.append(([], [(rnd(rng, 5), quals(rng, 5), 0)]))                                          # no sequences
    bins.append(([], []))
    bins.append(([rnd(rng, I.SEQ_MAX)], [(rnd(rng, 512), quals(rng, 512), 3000), (rnd(rng, 1), quals(rng, 1), 4095)]))
    return bins


def test_the_smallest_shapes_that_can_go_wrong(gpu):
    bins = edge_bins()
    best, off = check(bins, gpu)
    k = fcship.ir_pairs(*[I.flat(bins[:12])[i] for i in (2, 6)])   # L = 512: every offset scores alike, orig wins
    assert (int(best[k]), int(off[k])) == (512 * 93, 50)
    # the ties: orig wins over a smaller offset with the same score; without it the smallest offset
    t = fcship.ir_pairs(*[I.flat(bins[:9])[i] for i in (2, 6)])
    assert [int(x) for x in off[t:t + 4]] == [10, 15, 0, 0] and [int(x) for x in best[t:t + 2]] == [0, 0]


@pytest.mark.parametrize("seq_pad,read_pad", [(0, 0), (1, 3), (2, 2), (3, 1)])
def test_flat_arrays_beginning_at_each_residue(gpu, seq_pad, read_pad):
    check(I.random_bins(40 + seq_pad, 12), gpu, seq_pad=seq_pad, read_pad=read_pad)


def test_the_empty_batch(gpu):
    best, off = fcship.ir_score(I.flat([]), device=gpu)
    assert len(best) == 0 and len(off) == 0
    best, off = fcship.ir_score(I.flat([([], []), ([[1, 2]], [])]), device=gpu)
    assert len(best) == 0


def test_a_seeded_random_batch_of_a_few_hundred_bins(gpu):
    bins = I.random_bins(7, 300) + I.random_bins(8, 6, len_lo=900, len_hi=1300, L_lo=100, L_hi=160)
    best, off = check(bins, gpu)
    assert len(best) > 1000 and len(set(off.tolist())) > 50


def test_more_sequences_than_grid_slots(gpu):
    src = open(os.path.join(ROOT, "falcon-genome_amd", "csrc", "indel.hip")).read()
    cap = int(re.search(r"constexpr int kIrMaxBlocks = (\d+);", src).group(1))
    rng = np.random.default_rng(3)
    bins = [([rnd(rng, 5) for _ in range(1 + k % 2)], [(rnd(rng, 2), quals(rng, 2), k % 5) for _ in range(1 + k % 3)])
            for k in range(cap + 57)]
    best, off = check(bins, gpu)
    assert len(best) > cap and fcship.ir_pairs(*[I.flat(bins)[i] for i in (2, 6)]) == len(best)


def test_dev_twin_sets_its_status_bits_for_a_clamped_offset(gpu):
    import torch
    bins = I.random_bins(11, 20)
    arrays = [np.array(a) for a in I.flat(bins)]
    want_best, want_off = I.expected(bins)
    n_pairs = len(want_best)
    first = np.concatenate([[0], np.cumsum(np.diff(arrays[2]) * np.diff(arrays[6]))])
    last_seq_bin = max(b for b in range(len(bins)) if len(bins[b][0]) and len(bins[b][1]))

    def run(arrays, max_pairs, **kw):
        dev = [torch.from_numpy(a.view(np.uint8).copy()).cuda(gpu) for a in arrays]
        b, _ = fcship.ir_batch(*arrays, **kw)
        for name, t in zip(("seq", "seq_off", "bin_seq", "read", "qual", "read_off", "bin_read", "orig"), dev):
            setattr(b, name, t.data_ptr())
        best = torch.full((max(n_pairs, 1),), 0xFFFFFFFF, dtype=torch.int64, device=f"cuda:{gpu}").to(torch.int32)
        off = torch.full((max(n_pairs, 1),), -7, dtype=torch.int32, device=f"cuda:{gpu}")
        tail = torch.zeros(4, dtype=torch.int64, device=f"cuda:{gpu}")
        need = fcship.lib.fcsir_workspace_bytes(b.n_bins)
        ws = torch.zeros(need, dtype=torch.uint8, device=f"cuda:{gpu}")
        torch.cuda.synchronize()
        fcship.check(fcship.lib.fcsir_score_dev(gpu, C.addressof(b), best.data_ptr(), off.data_ptr(), max_pairs, tail.data_ptr(),
                                                ws.data_ptr(), need, tail.data_ptr() + 8, None))
        torch.cuda.synchronize()
        t = tail.cpu().numpy()
        return best.cpu().numpy().view(np.uint32), off.cpu().numpy(), int(t[0]), int(t[1] & 0xFFFFFFFF)

    best, off, n, status = run(arrays, n_pairs)
    assert (n, status) == (n_pairs, 0) and np.array_equal(best[:n], want_best) and np.array_equal(off[:n], want_off)
    # fewer bytes declared than the last sequence's offsets say: clamped, the bit set, every other pair as before
    s_last = int(arrays[2][last_seq_bin + 1]) - 1
    cut = int(arrays[1][s_last + 1]) - 3
    best, off, n, status = run(arrays, n_pairs, n_seq_bytes=cut)
    assert n == n_pairs and status == fcship.FCSIR_STATUS_FIELD
    later = np.zeros(n_pairs, bool)
    for b in range(len(bins)):
        c0, R = int(arrays[2][b]), int(arrays[6][b + 1] - arrays[6][b])
        for c in range(int(arrays[2][b + 1]) - c0):
            if int(arrays[1][c0 + c + 1]) > cut:
                later[first[b] + c * R: first[b] + (c + 1) * R] = True
    assert later.any() and np.array_equal(best[~later], want_best[~later]) and np.array_equal(off[~later], want_off[~later])
    # room for fewer pairs than there are: the count is the whole, the bit is set, nothing beyond the room is written
    room = n_pairs // 2
    best, off, n, status = run(arrays, room)
    assert n == n_pairs and status == fcship.FCSIR_STATUS_PAIRS
    assert np.array_equal(best[:room], want_best[:room]) and (off[room:] == -7).all()
    # a negative original offset of a read that has pairs: clamped to zero, the bit set
    bad = [np.array(a) for a in arrays]
    bad[7][int(arrays[6][last_seq_bin])] = -5
    _, _, n, status = run(bad, n_pairs)
    assert n == n_pairs and status == fcship.FCSIR_STATUS_FIELD


def run_both(tmp_path, gpu, ref, bam, *extra):
    logs = {}
    for mode in ("true", "false"):
        p = H.run_cli("indel", "-r", ref, "-i", bam, "-o", tmp_path / f"{mode}.bam", "--targets-out", tmp_path / f"{mode}.intervals",
                      *extra, env={"FCS_INDEL_GPU": mode, "FCS_GPU_DEVICES": str(gpu)}, cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-2000:]
        logs[mode] = p.stderr
    assert "(GPU)" in logs["true"] and "(host)" in logs["false"]
    for name in ("bam", "bam.bai", "intervals"):
        assert (tmp_path / f"true.{name}").read_bytes() == (tmp_path / f"false.{name}").read_bytes(), name
    return logs


def test_command_writes_the_same_bytes_on_both_paths_classic_case(gpu, tmp_path):
    s, records, moved = I.classic_case()
    ref = I.write_fasta(tmp_path / "ref.fa", [("ctg", s)])
    bam = I.write_bam(tmp_path / "in.bam", [("ctg", len(s))], records)
    logs = run_both(tmp_path, gpu, ref, bam)
    assert "6 records realigned" in logs["true"], logs["true"]
    recs = {r["name"]: r for r in H.read_bam(tmp_path / "true.bam")[2]}
    assert all(recs[n]["cigar"] == ["45M", "6D", "5M"] and recs[n]["mapq"] == 50 for n in moved)


def test_command_writes_the_same_bytes_on_both_paths_synth(gpu, tmp_path):
    d = tmp_path / "syn"
    p = H.run_cli("synth", "-o", d, "-c", "chr1:60000,chr2:20000", "-x", "12", "--seed", "22", "--no-fastq")
    assert p.returncode == 0, p.stderr[-2000:]
    logs = run_both(tmp_path, gpu, d / "ref.fasta", d / "sample.bam", "--sample-id", "s")
    m = re.search(r"(\d+) targets, (\d+) bins .*?(\d+) pairs, (\d+) bins cleaned, (\d+) records realigned", logs["true"])
    assert m and int(m.group(1)) > 0 and int(m.group(3)) > 0, logs["true"]
