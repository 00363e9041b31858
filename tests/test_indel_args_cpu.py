"""fcsir_score's refusals (include/fcsir.h): every one happens before a device
is looked for (the calls name device 99), with its message; nothing is written
on a refusal; a batch without pairs needs no device at all.
"""
import ctypes as C

import numpy as np

import fcship
import ir_cases as I

BINS = I.random_bins(3, 6, len_lo=30, len_hi=60, L_lo=2, L_hi=20) + [([np.array([0, 1, 2, 3, 0], np.uint8)] * 2,
                                                                      [(np.array([1, 2], np.uint8), np.array([9, 9], np.uint8), 1)] * 3)]
ARRAYS = I.flat(BINS)
NAMES = ("seq", "seq_off", "bin_seq", "read", "qual", "read_off", "bin_read", "orig")


def last_error():
    return fcship.lib.fcs_last_error().decode()


def call(device=99, max_pairs=None, **kw):
    arrays = [np.array(kw.pop(n)) if n in kw else a for n, a in zip(NAMES, ARRAYS)]
    try:
        fcship.ir_score(arrays, max_pairs=max_pairs, device=device, **kw)
    except fcship.FcsError as e:
        return e.code, str(e)
    return 0, ""


def changed(name, index, value):
    a = np.array(ARRAYS[NAMES.index(name)])
    a[index] = value
    return {name: a}


def test_every_refusal_comes_before_the_device_with_its_message():
    n_seq, n_reads, n_bins = len(ARRAYS[1]) - 1, len(ARRAYS[5]) - 1, len(ARRAYS[2]) - 1
    for kw, what in ((dict(n_bins=-1), "negative count: -1 bins"),
                     (dict(n_seq=-2), "negative count"),
                     (dict(n_reads=1 << 31), "a count above 2^31 - 1"),
                     (dict(n_seq_bytes=-1), "negative sequence or read size"),
                     (dict(max_pairs=-1), "max_pairs -1"),
                     (changed("bin_seq", 0, 1), "bin sequence offsets start at 1, not at zero"),
                     (changed("bin_seq", 2, int(ARRAYS[2][3]) + 1), "bin sequence offsets out of order at record 2"),
                     (dict(n_seq=n_seq + 1), "bin sequence offsets end at"),
                     (changed("bin_read", n_bins, n_reads - 1), "bin read offsets"),
                     (changed("seq_off", 1, int(ARRAYS[1][2]) + 1), "sequence offsets out of order at record 1"),
                     (dict(n_seq_bytes=len(ARRAYS[0]) - 1), "sequence offsets end at"),
                     (dict(n_read_bytes=len(ARRAYS[3]) - 1), "read offsets end at"),
                     (changed("seq_off", 1, int(ARRAYS[1][0])), "sequence 0 is empty"),
                     (changed("read_off", 1, int(ARRAYS[5][0])), "read 0 is empty"),
                     (changed("seq", 7, 5), "sequence 0 has code 5 at base 7"),
                     (changed("read", 0, 9), "read 0 has code 9 at base 0"),
                     (changed("orig", 2, -1), "read 2 has the original offset -1 (0 to 1073741824)"),
                     (changed("orig", 2, (1 << 30) + 1), "read 2 has the original offset 1073741825"),
                     (dict(max_pairs=fcship.ir_pairs(ARRAYS[2], ARRAYS[6]) - 1), "pairs, max_pairs is")):
        rc, err = call(**kw)
        assert rc == fcship.FCS_ERR_INVALID and "[E::fcsir_score]" in err and what in err, (list(kw), err)


def test_lengths_above_the_limits_are_refused():
    long_seq = I.flat([([np.zeros(I.SEQ_MAX + 1, np.uint8)], [(np.zeros(3, np.uint8), np.zeros(3, np.uint8), 0)])])
    long_read = I.flat([([np.zeros(600, np.uint8)], [(np.zeros(I.READ_MAX + 1, np.uint8), np.zeros(I.READ_MAX + 1, np.uint8), 0)])])
    for arrays, what in ((long_seq, "4097 sequence bytes, more than 4096"), (long_read, "513 read bytes, more than 512")):
        try:
            fcship.ir_score(arrays, device=99)
            raise AssertionError("not refused")
        except fcship.FcsError as e:
            assert e.code == fcship.FCS_ERR_INVALID and what in str(e), str(e)


def test_nothing_is_written_on_a_refusal_and_null_arguments():
    bad = [np.array(a) for a in ARRAYS]
    bad[7][0] = -3
    b, keep = fcship.ir_batch(*bad)
    room = fcship.ir_pairs(keep[2], keep[6])
    best, off, n = np.full(room, 7, np.uint32), np.full(room, 7, np.int32), C.c_int64(7)
    assert fcship.lib.fcsir_score(0, C.addressof(b), best.ctypes.data, off.ctypes.data, room, C.addressof(n)) == fcship.FCS_ERR_INVALID
    assert (best == 7).all() and (off == 7).all() and n.value == 7
    b, keep = fcship.ir_batch(*ARRAYS)
    assert fcship.lib.fcsir_score(0, None, best.ctypes.data, off.ctypes.data, room, C.addressof(n)) == fcship.FCS_ERR_INVALID
    assert "null batch" in last_error()
    assert fcship.lib.fcsir_score(0, C.addressof(b), best.ctypes.data, off.ctypes.data, room, None) == fcship.FCS_ERR_INVALID
    assert "null pair count" in last_error()
    assert fcship.lib.fcsir_score(0, C.addressof(b), None, off.ctypes.data, room, C.addressof(n)) == fcship.FCS_ERR_INVALID
    assert "null output arrays" in last_error()
    b.orig = None
    assert fcship.lib.fcsir_score(0, C.addressof(b), best.ctypes.data, off.ctypes.data, room, C.addressof(n)) == fcship.FCS_ERR_INVALID
    assert "null offset array" in last_error()


def test_the_device_error_comes_after_every_check_and_no_pairs_need_no_device():
    rc, err = call()
    assert rc in (fcship.FCS_ERR_INVALID, fcship.FCS_ERR_DEVICE) and "[E::fcsir_score]" not in err
    best, off = fcship.ir_score(I.flat([]), device=99)
    assert len(best) == 0 and len(off) == 0
    best, off = fcship.ir_score(I.flat([([[0, 1, 2]], []), ([], [([1], [5], 0)])]), device=99)
    assert len(best) == 0


def test_workspace_and_dev_twin_scalars():
    assert fcship.lib.fcsir_workspace_bytes(-1) == fcship.FCS_ERR_INVALID and "[E::fcsir_workspace_bytes]" in last_error()
    assert 0 < fcship.lib.fcsir_workspace_bytes(0) <= fcship.lib.fcsir_workspace_bytes(1 << 20) <= 1 << 24
    b, keep = fcship.ir_batch(*ARRAYS)
    one = np.zeros(64, np.uint8).ctypes.data   # stands for device memory: never dereferenced
    assert fcship.lib.fcsir_score_dev(0, C.addressof(b), one, one, 10, one, one, 16, one, None) == fcship.FCS_ERR_INVALID
    assert "[E::fcsir_score_dev]" in last_error() and "the workspace holds 16 bytes" in last_error()
    assert fcship.lib.fcsir_score_dev(0, C.addressof(b), one, one, 10, one, one, 1 << 20, None, None) == fcship.FCS_ERR_INVALID
    assert "null workspace or status" in last_error()
    assert fcship.lib.fcsir_score_dev(0, C.addressof(b), one, one, -1, one, one, 1 << 20, one, None) == fcship.FCS_ERR_INVALID
    assert "max_pairs -1" in last_error()
