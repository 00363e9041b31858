"""The argument checks of the banded-SW and FMD seeding entry points, and
fcs_phmm_partition, on the real libfcship.so without a GPU.

Every check these calls make before they look for a device is pinned here by
its return code and the exact fcs_last_error() text: null buffers, negative
counts, extents outside the buffers, h0 <= 0, a negative band, base codes
above 4 (query and target), a CIGAR arena without its offsets, a bad CIGAR
extent, bad gap penalties, a negative read length and a read that leaves the
code bytes.  One case per call has two wrong arguments and pins which message
wins: the order of the checks is part of the C-ABI's behaviour.

fcs_bsw_extend_plan needs a plan, which only a device makes: a zeroed block
stands in for one (device 0, capacity 0), so its "null result buffer" check,
which comes after "batch exceeds plan", is the one message not reached here.

The fcs_ksw_*2 twins' own refusals (another alphabet, a null matrix, a cached
query profile) are pinned the same way.

fcs_phmm_partition runs without a device; tests/sharding.py balanced_slices
is its oracle.
"""
import ctypes as C

import numpy as np
import pytest

import fcship
import sharding

lib = fcship.lib
INVALID, UNSUPPORTED, OK = fcship.FCS_ERR_INVALID, fcship.FCS_ERR_UNSUPPORTED, fcship.FCS_OK
PARAMS_NULL = "[E::fcship] null SW params"
PARAMS_GAPS = "[E::fcship] gap penalties must satisfy o >= 0, e > 0"


def last_error():
    return lib.fcs_last_error().decode()


def expect(rc, code, msg):
    assert rc == code, (rc, last_error())
    assert last_error() == msg


def adr(a):
    return None if a is None else a.ctypes.data


def cptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


class Soa:
    """Two SW tasks as an fcs_bsw_batch over host arrays; fields are replaced by keyword."""

    def __init__(self, **kw):
        self.a = dict(qbuf=np.array([0, 1, 2, 3, 4, 0], np.uint8), qoff=np.array([0, 3], np.int64),
                      qlen=np.array([3, 3], np.int32), tbuf=np.array([0, 1, 2, 3, 4, 0, 1, 2], np.uint8),
                      toff=np.array([0, 4], np.int64), tlen=np.array([4, 4], np.int32),
                      h0=np.array([5, 5], np.int32), w=np.array([10, 10], np.int32))
        self.n, self.qbytes, self.tbytes = 2, 6, 8
        for k, v in kw.items():
            if k in self.a:
                self.a[k] = v
            else:
                setattr(self, k, v)

    def struct(self):
        b = fcship.BswBatch()
        for k, v in self.a.items():
            setattr(b, k, adr(v))
        b.n, b.qbytes, b.tbytes, b.max_qlen, b.max_tlen = self.n, self.qbytes, self.tbytes, 3, 4
        return b


def gaps(**kw):
    p = fcship.bsw_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def aos(items):
    """(fcs_bsw_task array, the arrays it points into) of (query, target, h0, w) items; None stays a null pointer."""
    keep, arr = [], (fcship.BswTask * max(len(items), 1))()
    for k, (q, t, h0, w) in enumerate(items):
        qa = None if q is None else np.asarray(q, np.uint8)
        ta = None if t is None else np.asarray(t, np.uint8)
        keep += [qa, ta]
        arr[k] = fcship.BswTask(0 if qa is None else len(qa), 0 if ta is None else len(ta), h0, w,
                                cptr(qa, fcship.u8p), cptr(ta, fcship.u8p))
    return arr, keep


GOOD = [([0, 1, 2], [0, 1, 2, 3], 5, 10), ([3, 4], [1, 1, 2], 5, 10)]


# ------------------------------------------------------------------ extend
def extend_batch(s=None, params="default", res="default", null_batch=False):
    s = s or Soa()
    b = s.struct()
    p = gaps() if params == "default" else params
    r = np.zeros((2, 6), np.int32) if res == "default" else res
    cells = np.zeros(2, np.int64)
    return lib.fcs_bsw_extend_batch(None if null_batch else C.byref(b), None if p is None else C.byref(p),
                                    cptr(r, fcship.i32p), cells.ctypes.data_as(fcship.i64p), 0)


EXTEND_BATCH = [
    (dict(null_batch=True), "[E::fcship] bad SW batch"),
    (dict(s=Soa(n=-1)), "[E::fcship] bad SW batch"),
    (dict(s=Soa(qoff=None)), "[E::fcship] null pointer in SW batch"),
    (dict(s=Soa(qbuf=None)), "[E::fcship] null pointer in SW batch"),
    (dict(s=Soa(tbuf=None)), "[E::fcship] null pointer in SW batch"),
    (dict(s=Soa(w=None)), "[E::fcship] null pointer in SW batch"),
    (dict(params=None), PARAMS_NULL),
    (dict(params=gaps(e_del=0)), PARAMS_GAPS),
    (dict(params=gaps(o_ins=-1)), PARAMS_GAPS),
    (dict(res=None), "[E::fcs_bsw_extend_batch] null result buffer"),
    (dict(s=Soa(qlen=np.array([3, -1], np.int32))), "[E::fcs_bsw_extend_batch] task extent outside buffers"),
    (dict(s=Soa(qoff=np.array([0, 4], np.int64))), "[E::fcs_bsw_extend_batch] task extent outside buffers"),
    (dict(s=Soa(toff=np.array([-1, 4], np.int64))), "[E::fcs_bsw_extend_batch] task extent outside buffers"),
    (dict(s=Soa(tlen=np.array([4, 5], np.int32))), "[E::fcs_bsw_extend_batch] task extent outside buffers"),
    (dict(s=Soa(h0=np.array([5, 0], np.int32))), "[E::fcs_bsw_extend_batch] h0 must be > 0 (ksw_extend2 assert)"),
    (dict(s=Soa(w=np.array([10, -1], np.int32))), "[E::fcs_bsw_extend_batch] negative band"),
    (dict(s=Soa(qbuf=np.array([0, 1, 2, 3, 4, 5], np.uint8))), "[E::fcs_bsw_extend_batch] query base code > 4"),
    (dict(s=Soa(tbuf=np.array([0, 1, 2, 3, 4, 0, 1, 9], np.uint8))), "[E::fcs_bsw_extend_batch] target base code > 4"),
    # two at once: the first check in the call's order answers
    (dict(s=Soa(n=-1), params=None), "[E::fcship] bad SW batch"),
    (dict(params=None, res=None), PARAMS_NULL),
    (dict(res=None, s=Soa(h0=np.array([0, 5], np.int32))), "[E::fcs_bsw_extend_batch] null result buffer"),
    (dict(s=Soa(h0=np.array([5, 0], np.int32), w=np.array([-1, 10], np.int32))), "[E::fcs_bsw_extend_batch] negative band"),
    (dict(s=Soa(h0=np.array([0, 5], np.int32), w=np.array([-1, 10], np.int32))),
     "[E::fcs_bsw_extend_batch] h0 must be > 0 (ksw_extend2 assert)"),
    (dict(s=Soa(h0=np.array([5, 0], np.int32), qbuf=np.array([9, 1, 2, 3, 4, 0], np.uint8))),
     "[E::fcs_bsw_extend_batch] h0 must be > 0 (ksw_extend2 assert)"),
    (dict(s=Soa(qbuf=np.array([0, 1, 2, 3, 4, 5], np.uint8), tbuf=np.array([7, 1, 2, 3, 4, 0, 1, 2], np.uint8))),
     "[E::fcs_bsw_extend_batch] query base code > 4"),
]


@pytest.mark.parametrize("kw,msg", EXTEND_BATCH, ids=range(len(EXTEND_BATCH)))
def test_extend_batch_checks(kw, msg):
    expect(extend_batch(**kw), INVALID, msg)


def test_extend_batch_empty_returns_before_the_result_check():
    assert extend_batch(s=Soa(n=0), res=None) == OK
    # ... but not before the batch and parameter checks
    expect(extend_batch(s=Soa(n=0), params=None), INVALID, PARAMS_NULL)


def extend(items=GOOD, n=None, params="default", results=True, null_tasks=False):
    arr, keep = aos(items)
    p = gaps() if params == "default" else params
    res = (fcship.BswResult * max(len(items), 1))()
    return lib.fcs_bsw_extend(None if null_tasks else arr, len(items) if n is None else n,
                              None if p is None else C.byref(p), res if results else None, 0)


EXTEND = [
    (dict(n=-1), "[E::fcs_bsw_extend] bad arguments"),
    (dict(null_tasks=True), "[E::fcs_bsw_extend] bad arguments"),
    (dict(results=False), "[E::fcs_bsw_extend] bad arguments"),
    (dict(items=[([0, 1], [0, 1], 5, 10)], params=None), PARAMS_NULL),
    (dict(params=gaps(e_ins=0)), PARAMS_GAPS),
    (dict(items=[([0, 1], [0, 1], 0, 10)]), "[E::fcs_bsw_extend_batch] h0 must be > 0 (ksw_extend2 assert)"),
    (dict(items=[([0, 1], [0, 1], 5, -2)]), "[E::fcs_bsw_extend_batch] negative band"),
    (dict(items=[([0, 5], [0, 1], 5, 10)]), "[E::fcs_bsw_extend_batch] query base code > 4"),
    (dict(items=[([0, 1], [0, 1], 5, 10), ([1], [6], 5, 10)]), "[E::fcs_bsw_extend_batch] target base code > 4"),
    # two at once
    (dict(n=-1, params=None), "[E::fcs_bsw_extend] bad arguments"),
    (dict(items=[([0, 1], [0, 1], 0, 10)], params=None), PARAMS_NULL),
    (dict(items=[([0, 9], [0, 1], 5, -1)]), "[E::fcs_bsw_extend_batch] negative band"),
]


@pytest.mark.parametrize("kw,msg", EXTEND, ids=range(len(EXTEND)))
def test_extend_checks(kw, msg):
    expect(extend(**kw), INVALID, msg)


def malformed():
    """Task arrays with a negative length, and with a null pointer under a positive one."""
    neg, keep = aos(GOOD)
    neg[1].qlen = -1
    null, keep2 = aos(GOOD)
    null[1].target = None
    malformed.keep = keep + keep2
    return [neg, null]


def test_extend_malformed_task_wins_over_params():
    res = (fcship.BswResult * 2)()
    for arr in malformed():
        expect(lib.fcs_bsw_extend(arr, 2, None, res, 0), INVALID, "[E::fcship] malformed SW task")
    assert lib.fcs_bsw_extend(None, 0, None, None, 0) == OK  # empty: before the packer and the parameters


def extend_dev(s=None, params="default", res=True, null_batch=False):
    b = (s or Soa()).struct()
    p = gaps() if params == "default" else params
    r = np.zeros(16, np.int32)  # never dereferenced: stands for a device pointer
    return lib.fcs_bsw_extend_dev(None if null_batch else C.byref(b), None if p is None else C.byref(p),
                                  r.ctypes.data if res else None, None, 0, None)


def extend_plan(s=None, params="default", res=True, plan=True, null_batch=False):
    b = (s or Soa()).struct()
    p = gaps() if params == "default" else params
    r = np.zeros(16, np.int32)
    fake = (C.c_char * 256)()  # device 0, capacity 0
    return lib.fcs_bsw_extend_plan(C.addressof(fake) if plan else None, None if null_batch else C.byref(b),
                                   None if p is None else C.byref(p), r.ctypes.data if res else None, None, None)


def test_extend_dev_and_plan_checks():
    for f in (extend_dev, extend_plan):
        expect(f(null_batch=True), INVALID, "[E::fcship] bad SW batch")
        expect(f(s=Soa(n=-3)), INVALID, "[E::fcship] bad SW batch")
        expect(f(s=Soa(tlen=None)), INVALID, "[E::fcship] null pointer in SW batch")
        expect(f(s=Soa(h0=None)), INVALID, "[E::fcship] null pointer in SW batch")
        expect(f(params=None), INVALID, PARAMS_NULL)
        expect(f(params=gaps(e_del=-1)), INVALID, PARAMS_GAPS)
        expect(f(s=Soa(qlen=None), params=None), INVALID, "[E::fcship] null pointer in SW batch")  # two at once
    expect(extend_dev(res=False), INVALID, "[E::fcs_bsw_extend_dev] null result buffer")
    expect(extend_dev(res=False, params=gaps(o_del=-1)), INVALID, PARAMS_GAPS)  # two at once
    expect(extend_plan(plan=False, null_batch=True), INVALID, "[E::fcs_bsw_extend_plan] null plan")  # two at once
    expect(extend_plan(), INVALID, "[E::fcs_bsw_extend_plan] batch exceeds plan")
    expect(extend_plan(res=False), INVALID, "[E::fcs_bsw_extend_plan] batch exceeds plan")  # two at once
    assert extend_plan(s=Soa(n=0), res=False) == OK


# ------------------------------------------------------------------ global
def glob(items=GOOD, n=None, params="default", scores=True, null_tasks=False, arena=True, off="default", cap="default",
         ncig=True):
    arr, keep = aos(items)
    m = max(len(items), 1)
    p = gaps() if params == "default" else params
    sc, ar, nc = np.zeros(m, np.int32), np.zeros(64, np.uint32), np.zeros(m, np.int32)
    off = np.arange(m, dtype=np.int64) * 16 if isinstance(off, str) else off
    cap = np.full(m, 12, np.int32) if isinstance(cap, str) else cap
    return lib.fcs_bsw_global(None if null_tasks else arr, len(items) if n is None else n,
                              None if p is None else C.byref(p), cptr(sc, fcship.i32p) if scores else None,
                              cptr(ar, fcship.u32p) if arena else None, cptr(off, fcship.i64p),
                              cptr(cap, fcship.i32p), cptr(nc, fcship.i32p) if ncig else None, 0)


CIGAR_NEEDS = "[E::fcs_bsw_global] CIGAR arena needs offsets, caps and counts"
GLOBAL = [
    (dict(n=-1), "[E::fcs_bsw_global] bad arguments"),
    (dict(null_tasks=True), "[E::fcs_bsw_global] bad arguments"),
    (dict(scores=False), "[E::fcs_bsw_global] bad arguments"),
    (dict(off=None), CIGAR_NEEDS),
    (dict(cap=None), CIGAR_NEEDS),
    (dict(ncig=False), CIGAR_NEEDS),
    (dict(params=None), PARAMS_NULL),
    (dict(params=gaps(e_del=0)), PARAMS_GAPS),
    (dict(items=[([0, 1], [0, 1], 1, 10), ([0], [1], 1, -1)]), "[E::fcs_bsw_global] negative band"),
    (dict(cap=np.array([12, -1], np.int32)), "[E::fcs_bsw_global] bad CIGAR extent"),
    (dict(off=np.array([-8, 16], np.int64)), "[E::fcs_bsw_global] bad CIGAR extent"),
    (dict(items=[([0, 1], [0, 1], 1, 10), ([5], [1], 1, 10)]), "[E::fcs_bsw_global] query base code > 4"),
    (dict(items=[([0, 1], [0, 200], 1, 10)]), "[E::fcs_bsw_global] target base code > 4"),
    (dict(items=[([0, 1], [0, 200], 1, 10)], arena=False, off=None, cap=None, ncig=False),
     "[E::fcs_bsw_global] target base code > 4"),  # scores only: no CIGAR arrays needed
    # two at once
    (dict(scores=False, off=None), "[E::fcs_bsw_global] bad arguments"),
    (dict(off=None, params=None), CIGAR_NEEDS),
    (dict(params=None, items=[([0], [1], 1, -1)]), PARAMS_NULL),
    (dict(items=[([0], [1], 1, -1), ([0], [1], 1, 5)], cap=np.array([-1, 4], np.int32)), "[E::fcs_bsw_global] negative band"),
    (dict(items=[([0], [1], 1, 5), ([0], [1], 1, -1)], cap=np.array([-1, 4], np.int32)), "[E::fcs_bsw_global] bad CIGAR extent"),
    (dict(items=[([7], [1], 1, 5)], cap=np.array([-1], np.int32)), "[E::fcs_bsw_global] bad CIGAR extent"),
    (dict(items=[([7], [8], 1, 5)]), "[E::fcs_bsw_global] query base code > 4"),
]


@pytest.mark.parametrize("kw,msg", GLOBAL, ids=range(len(GLOBAL)))
def test_global_checks(kw, msg):
    expect(glob(**kw), INVALID, msg)


def test_global_empty_and_malformed():
    assert glob(items=[], n=0) == OK
    expect(glob(items=[], n=0, params=None), INVALID, PARAMS_NULL)  # the parameters are looked at first
    sc = np.zeros(2, np.int32)
    p = gaps()
    for arr in malformed():
        expect(lib.fcs_bsw_global(arr, 2, C.byref(p), sc.ctypes.data_as(fcship.i32p), None, None, None, None, 0),
               INVALID, "[E::fcship] malformed SW task")
    bad = gaps(e_ins=0)
    arr = malformed()[0]  # two at once: the parameters come before the packer
    expect(lib.fcs_bsw_global(arr, 2, C.byref(bad), sc.ctypes.data_as(fcship.i32p), None, None, None, None, 0),
           INVALID, PARAMS_GAPS)


def global_dev(s=None, params="default", null_batch=False, scores=True, cigar=True, missing=None):
    b = (s or Soa()).struct()
    p = gaps() if params == "default" else params
    x = np.zeros(16, np.int64).ctypes.data  # stands for device pointers: never dereferenced
    a = dict(zbuf=x, zoff=x, cigar=x if cigar else None, coff=x, ccap=x, ncig=x)
    if missing:
        a[missing] = None
    return lib.fcs_bsw_global_dev(None if null_batch else C.byref(b), None if p is None else C.byref(p),
                                  x if scores else None, a["zbuf"], 64, a["zoff"], a["cigar"], a["coff"], a["ccap"],
                                  a["ncig"], 0, None)


def align_dev(s=None, params="default", null_batch=False, xtra=True, out=True):
    b = (s or Soa()).struct()
    p = gaps() if params == "default" else params
    x = np.zeros(16, np.int64).ctypes.data
    return lib.fcs_bsw_align_dev(None if null_batch else C.byref(b), None if p is None else C.byref(p),
                                 x if xtra else None, x if out else None, 0, None)


def test_global_dev_and_align_dev_checks():
    G, A = "[E::fcs_bsw_global_dev] ", "[E::fcs_bsw_align_dev] "
    expect(global_dev(null_batch=True), INVALID, G + "bad arguments")
    expect(global_dev(s=Soa(n=-1)), INVALID, G + "bad arguments")
    expect(global_dev(scores=False), INVALID, G + "bad arguments")
    for m in ("zbuf", "zoff", "coff", "ccap", "ncig"):
        expect(global_dev(missing=m), INVALID, G + "CIGARs need the direction matrix, offsets, caps and counts")
    expect(global_dev(params=None), INVALID, PARAMS_NULL)
    expect(global_dev(params=gaps(o_del=-1)), INVALID, PARAMS_GAPS)
    expect(global_dev(s=Soa(n=1 << 31)), UNSUPPORTED, G + "more than 2^31-1 tasks")
    assert global_dev(s=Soa(n=0), scores=False) == OK
    expect(global_dev(scores=False, missing="zoff"), INVALID, G + "bad arguments")  # two at once
    expect(global_dev(missing="zoff", params=None), INVALID, G + "CIGARs need the direction matrix, offsets, caps and counts")
    expect(global_dev(params=None, s=Soa(n=1 << 31)), INVALID, PARAMS_NULL)
    expect(align_dev(null_batch=True), INVALID, A + "bad arguments")
    expect(align_dev(s=Soa(n=-1)), INVALID, A + "bad arguments")
    expect(align_dev(xtra=False), INVALID, A + "bad arguments")
    expect(align_dev(out=False), INVALID, A + "bad arguments")
    expect(align_dev(params=None), INVALID, PARAMS_NULL)
    expect(align_dev(params=gaps(e_ins=0)), INVALID, PARAMS_GAPS)
    expect(align_dev(s=Soa(n=1 << 31)), UNSUPPORTED, A + "more than 2^31-1 tasks")
    assert align_dev(s=Soa(n=0), xtra=False, out=False) == OK
    expect(align_dev(out=False, params=None), INVALID, A + "bad arguments")  # two at once
    expect(align_dev(params=gaps(e_ins=0), s=Soa(n=1 << 31)), INVALID, PARAMS_GAPS)


# ------------------------------------------------------------------ align
def align(items=GOOD, n=None, params="default", null_tasks=False, xtra=True, out=True):
    arr, keep = aos(items)
    m = max(len(items), 1)
    p = gaps() if params == "default" else params
    x, o = np.full(m, fcship.KSW_XSTART, np.int32), np.zeros((m, 7), np.int32)
    return lib.fcs_bsw_align(None if null_tasks else arr, len(items) if n is None else n,
                             None if p is None else C.byref(p), cptr(x, fcship.i32p) if xtra else None,
                             o.ctypes.data if out else None, 0)


ALIGN = [
    (dict(n=-1), "[E::fcs_bsw_align] bad arguments"),
    (dict(null_tasks=True), "[E::fcs_bsw_align] bad arguments"),
    (dict(xtra=False), "[E::fcs_bsw_align] bad arguments"),
    (dict(out=False), "[E::fcs_bsw_align] bad arguments"),
    (dict(params=None), PARAMS_NULL),
    (dict(params=gaps(o_ins=-2)), PARAMS_GAPS),
    (dict(items=[([0, 1], [0, 1], 0, 0), ([1, 5], [1], 0, 0)]), "[E::fcs_bsw_align] query base code > 4"),
    (dict(items=[([0, 1], [0, 1], 0, 0), ([1, 4], [255], 0, 0)]), "[E::fcs_bsw_align] target base code > 4"),
    # two at once
    (dict(xtra=False, params=None), "[E::fcs_bsw_align] bad arguments"),
    (dict(params=None, items=[([9], [9], 0, 0)]), PARAMS_NULL),
    (dict(items=[([0, 1], [0, 6], 0, 0), ([1, 5], [1], 0, 0)]), "[E::fcs_bsw_align] query base code > 4"),
]


@pytest.mark.parametrize("kw,msg", ALIGN, ids=range(len(ALIGN)))
def test_align_checks(kw, msg):
    expect(align(**kw), INVALID, msg)


def test_align_empty_and_malformed():
    assert align(items=[], n=0) == OK
    expect(align(items=[], n=0, params=None), INVALID, PARAMS_NULL)
    x, o, p = np.zeros(2, np.int32), np.zeros((2, 7), np.int32), gaps()
    for arr in malformed():
        expect(lib.fcs_bsw_align(arr, 2, C.byref(p), x.ctypes.data_as(fcship.i32p), o.ctypes.data, 0), INVALID,
               "[E::fcship] malformed SW task")


# ------------------------------------------------------------------ FMD collect / seed
CODES = np.zeros(100, np.uint8)


def collect(n_bytes=100, off=(0, 50), qlen=(50, 50), n=2, P="default", codes=True, out=True):
    off, qlen = np.array(off, np.int64), np.array(qlen, np.int32)
    mems, nm, ov = np.zeros((2, 4), fcship.FMD_MEM), np.zeros(2, np.int32), np.zeros(2, np.int32)
    P = fcship.FmdParams(19, 28, 10, 4, 20) if isinstance(P, str) else P
    return lib.fcs_fmd_collect(None, CODES.ctypes.data if codes else None, n_bytes, off.ctypes.data, qlen.ctypes.data, n,
                               None if P is None else C.addressof(P), mems.ctypes.data if out else None, nm.ctypes.data,
                               ov.ctypes.data)


def seed(n_bytes=100, off=(0, 50), qlen=(50, 50), n=2, P="default", codes=True, mem_cap=8, row_cap=8, mems=True,
         mem_off=True, overflow=True):
    off, qlen = np.array(off, np.int64), np.array(qlen, np.int32)
    m, pos = np.zeros(8, fcship.FMD_MEM), np.zeros(8, np.int64)
    mo, ro, ov = np.zeros(3, np.int64), np.zeros(3, np.int64), np.zeros(2, np.int32)
    P = fcship.FmdSeedParams(fcship.FmdParams(19, 28, 10, 4, 20), 500, 0) if isinstance(P, str) else P
    return lib.fcs_fmd_seed(None, CODES.ctypes.data if codes else None, n_bytes, off.ctypes.data, qlen.ctypes.data, n,
                            None if P is None else C.addressof(P), m.ctypes.data if mems else None, mem_cap,
                            mo.ctypes.data if mem_off else None, pos.ctypes.data, row_cap, ro.ctypes.data,
                            ov.ctypes.data if overflow else None)


def seed_params(max_mems=4, min_len=19, max_occ=500, max_steps=0, intv=20):
    return fcship.FmdSeedParams(fcship.FmdParams(min_len, 28, 10, max_mems, intv), max_occ, max_steps)


READS = [  # shared by collect and seed: {who} is the call's name
    (dict(n=-1), "[E::{who}] bad arguments"),
    (dict(n_bytes=-1), "[E::{who}] bad arguments"),
    (dict(codes=False), "[E::{who}] bad arguments"),
    (dict(P=None), "[E::{who}] null params"),
    (dict(qlen=(50, -1)), "[E::{who}] read 1 has negative length -1"),
    (dict(off=(0, 51)), "[E::{who}] read 1 at offset 51 leaves the 100 code bytes"),
    (dict(off=(-1, 50)), "[E::{who}] read 0 at offset -1 leaves the 100 code bytes"),
    (dict(qlen=(101, 0)), "[E::{who}] read 0 at offset 0 leaves the 100 code bytes"),
    (dict(n_bytes=99), "[E::{who}] read 1 at offset 50 leaves the 99 code bytes"),
    (dict(), "[E::{who}] null index handle"),
    (dict(n=0), "[E::{who}] null index handle"),  # the handle is looked at before the empty batch returns
    # two at once
    (dict(n=-1, P=None), "[E::{who}] bad arguments"),
    (dict(off=(0, 51), qlen=(-1, 50)), "[E::{who}] read 0 has negative length -1"),
    (dict(off=(51, 50), qlen=(50, -1)), "[E::{who}] read 0 at offset 51 leaves the 100 code bytes"),
    (dict(off=(0, 50), qlen=(50, -7), n_bytes=10), "[E::{who}] read 0 at offset 0 leaves the 10 code bytes"),
]


@pytest.mark.parametrize("kw,msg", READS, ids=range(len(READS)))
def test_collect_and_seed_read_checks(kw, msg):
    expect(collect(**kw), INVALID, msg.format(who="fcs_fmd_collect"))
    expect(seed(**kw), INVALID, msg.format(who="fcs_fmd_seed"))


def test_collect_checks_of_its_own():
    W = "[E::fcs_fmd_collect] "
    expect(collect(out=False), INVALID, W + "bad arguments")
    expect(collect(P=fcship.FmdParams(19, 28, 10, 0, 20)), INVALID, W + "max_mems 0 < 1")
    expect(collect(P=fcship.FmdParams(-1, 28, 10, 4, 20)), INVALID, W + "negative min_len or max_mem_intv")
    expect(collect(P=fcship.FmdParams(19, 28, 10, 4, -1)), INVALID, W + "negative min_len or max_mem_intv")
    # two at once: the parameters before the reads, max_mems before min_len
    expect(collect(P=fcship.FmdParams(-1, 28, 10, 0, 20), qlen=(50, -1)), INVALID, W + "max_mems 0 < 1")
    expect(collect(P=fcship.FmdParams(-1, 28, 10, 4, 20), off=(0, 51)), INVALID, W + "negative min_len or max_mem_intv")


def test_seed_checks_of_its_own():
    W = "[E::fcs_fmd_seed] "
    expect(seed(P=seed_params(max_mems=0)), INVALID, W + "max_mems 0 < 1")
    expect(seed(P=seed_params(min_len=-1)), INVALID, W + "negative min_len or max_mem_intv")
    expect(seed(P=seed_params(max_occ=0)), INVALID, W + "max_occ 0 < 1")
    expect(seed(P=seed_params(max_steps=-1)), INVALID, W + "negative max_steps")
    expect(seed(mem_cap=-1), INVALID, W + "negative capacity (mem_cap -1, row_cap 8)")
    expect(seed(row_cap=-2), INVALID, W + "negative capacity (mem_cap 8, row_cap -2)")
    expect(seed(mems=False), INVALID, W + "null output")
    expect(seed(mem_off=False), INVALID, W + "null output")
    expect(seed(overflow=False), INVALID, W + "null output")
    expect(seed(mems=False, mem_cap=0), INVALID, W + "null index handle")  # nothing to write: no buffer needed
    # two at once: the order is collect's parameters, max_occ, max_steps, capacities, outputs, reads
    expect(seed(P=seed_params(max_mems=0, max_occ=0)), INVALID, W + "max_mems 0 < 1")
    expect(seed(P=seed_params(max_occ=0, max_steps=-1)), INVALID, W + "max_occ 0 < 1")
    expect(seed(P=seed_params(max_steps=-1), mem_cap=-1), INVALID, W + "negative max_steps")
    expect(seed(mem_cap=-1, mems=False), INVALID, W + "negative capacity (mem_cap -1, row_cap 8)")
    expect(seed(mem_off=False, qlen=(50, -1)), INVALID, W + "null output")
    expect(seed(P=seed_params(max_occ=0), off=(0, 51)), INVALID, W + "max_occ 0 < 1")


# ------------------------------------------------------------------ partition
def pairs_of(costs):
    """A batch whose pair p costs costs[p] cells: read p of that length against a one-base
    haplotype, or a one-base read against the empty haplotype for a cost of 0."""
    reads = [(b"A" * max(c, 1),) * 5 for c in costs]
    return fcship.make_pairs(reads, [b"A", b""], [(r, 0 if c else 1) for r, c in enumerate(costs)])


@pytest.mark.parametrize("costs,n", [((), 1), ((), 3), ((5,), 1), ((5,), 3), ((0, 0, 0, 0, 0), 2), ((0, 0, 0, 0, 0), 3),
                                     ((0, 0, 0, 0, 0), 7), ((3, 1, 4, 1, 5, 9, 2), 3), ((3, 1, 4, 1, 5, 9, 2), 1),
                                     ((3, 1, 4, 1, 5, 9, 2), 7), ((3, 1, 4, 1, 5, 9, 2), 9), ((0, 0, 8, 0, 0, 0, 1), 3)])
def test_partition_equals_balanced_slices(costs, n):
    p = pairs_of(costs)
    cuts = fcship.phmm_partition(p, n)
    assert [(int(cuts[k]), int(cuts[k + 1])) for k in range(n)] == sharding.balanced_slices(list(costs), n)
    assert cuts[0] == 0 and cuts[n] == len(costs)


def test_partition_checks():
    p = pairs_of((3, 1, 4))
    b = p.to_struct()
    cuts = np.zeros(4, np.int64)
    expect(lib.fcs_phmm_partition(C.byref(b), 0, cuts.ctypes.data), INVALID,
           "[E::fcs_phmm_partition] need n_slices > 0 and cuts")
    expect(lib.fcs_phmm_partition(C.byref(b), 3, None), INVALID, "[E::fcs_phmm_partition] need n_slices > 0 and cuts")
    expect(lib.fcs_phmm_partition(None, 3, cuts.ctypes.data), INVALID, "[E::fcship] null PairHMM batch")
    p.pair_hap[1] = 2
    expect(lib.fcs_phmm_partition(C.byref(b), 3, cuts.ctypes.data), INVALID,
           "[E::fcs_phmm_partition] pair index out of range")


# ------------------------------------------------------------------ bwa's signature twins
def test_ksw_twins_refuse_other_alphabets_and_null_matrices():
    q, m = np.zeros(4, np.uint8), fcship.default_mat()
    qp, mp = q.ctypes.data_as(fcship.u8p), m.ctypes.data_as(fcship.i8p)
    FAILED = fcship.FCS_KSW_FAILED
    calls = {"fcs_ksw_align2": lambda a, mat: lib.fcs_ksw_align2(4, qp, 4, qp, a, mat, 6, 1, 6, 1, 0, None).score,
             "fcs_ksw_extend2": lambda a, mat: lib.fcs_ksw_extend2(4, qp, 4, qp, a, mat, 6, 1, 6, 1, 10, 5, 100, 5,
                                                                   None, None, None, None, None),
             "fcs_ksw_global2": lambda a, mat: lib.fcs_ksw_global2(4, qp, 4, qp, a, mat, 6, 1, 6, 1, 10, None, None)}
    for who, f in calls.items():
        assert f(4, mp) == FAILED and last_error() == f"[E::{who}] only m == 5 (bwa's alphabet) is supported"
        assert f(5, None) == FAILED and last_error() == f"[E::{who}] null matrix"
        assert f(4, None) == FAILED and last_error() == f"[E::{who}] only m == 5 (bwa's alphabet) is supported"
    cached = C.c_void_p(1)  # a cached query profile: after the alphabet and the matrix
    assert lib.fcs_ksw_align2(4, qp, 4, qp, 5, mp, 6, 1, 6, 1, 0, C.byref(cached)).score == FAILED
    assert last_error() == "[E::fcs_ksw_align2] cached query profiles unsupported"
    assert lib.fcs_ksw_align2(4, qp, 4, qp, 5, None, 6, 1, 6, 1, 0, C.byref(cached)).score == FAILED
    assert last_error() == "[E::fcs_ksw_align2] null matrix"
