"""ctypes binding of libfcship.so (include/fcship.h) for tests, bench and tools.

This module is plumbing: every computation goes through the C-ABI into the
gfx950 HIP kernels.  There is no CPU fallback — if the shared library is
missing, importing this module raises, and if no GPU is present the compute
entry points return FCS_ERR_DEVICE, which is raised as FcsError.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

try:  # one HIP runtime per process: torch bundles its own libamdhip64, so when
    # torch is present it must be loaded first and libfcship binds to that copy.
    import torch  # noqa: F401
except ImportError:  # pragma: no cover - torch is optional plumbing
    torch = None

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FCSHIP_LIB") or os.path.join(HERE, "libfcship.so")  # override: A/B builds
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "fcship.h")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"libfcship.so not built at {LIB_PATH}; run `make -C falcon-genome_amd` "
        "or __graft_entry__.build() (the HIP path has no CPU fallback)")

lib = C.CDLL(LIB_PATH)

FCS_OK = 0
FCS_ERR_INVALID = -1
FCS_ERR_DEVICE = -2
FCS_ERR_NOMEM = -3
FCS_ERR_UNSUPPORTED = -4
FCS_KSW_FAILED = -2147483648


class FcsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"fcship error {code}: {msg}")
        self.code = code


u8p = C.POINTER(C.c_uint8)
i8p = C.POINTER(C.c_int8)
i32p = C.POINTER(C.c_int32)
i64p = C.POINTER(C.c_int64)
u32p = C.POINTER(C.c_uint32)
f64p = C.POINTER(C.c_double)


class PhmmRead(C.Structure):
    _fields_ = [("bases", u8p), ("base_q", u8p), ("ins_q", u8p), ("del_q", u8p), ("gcp", u8p),
                ("len", C.c_int32)]


class PhmmHap(C.Structure):
    _fields_ = [("bases", u8p), ("len", C.c_int32)]


class PhmmRegion(C.Structure):
    _fields_ = [("reads", C.POINTER(PhmmRead)), ("n_reads", C.c_int32), ("haps", C.POINTER(PhmmHap)),
                ("n_haps", C.c_int32), ("out_log10", f64p)]


class PhmmOpts(C.Structure):
    _fields_ = [("device", C.c_int32), ("use_fp64_rescue", C.c_int32), ("rescue_threshold", C.c_float),
                ("exact_order", C.c_int32)]


class PhmmBatch(C.Structure):
    _fields_ = [("read_bases", C.c_void_p), ("read_bq", C.c_void_p), ("read_iq", C.c_void_p),
                ("read_dq", C.c_void_p), ("read_gcp", C.c_void_p), ("read_off", C.c_void_p),
                ("read_len", C.c_void_p), ("n_reads", C.c_int64), ("hap_bases", C.c_void_p),
                ("hap_off", C.c_void_p), ("hap_len", C.c_void_p), ("n_haps", C.c_int64),
                ("pair_read", C.c_void_p), ("pair_hap", C.c_void_p), ("n_pairs", C.c_int64),
                ("read_bytes", C.c_int64), ("hap_bytes", C.c_int64), ("max_read_len", C.c_int32),
                ("max_hap_len", C.c_int32)]


class BswTask(C.Structure):
    _fields_ = [("qlen", C.c_int32), ("tlen", C.c_int32), ("h0", C.c_int32), ("w", C.c_int32),
                ("query", u8p), ("target", u8p)]


class BswParams(C.Structure):
    _fields_ = [("mat", C.c_int8 * 25), ("o_del", C.c_int32), ("e_del", C.c_int32), ("o_ins", C.c_int32),
                ("e_ins", C.c_int32), ("end_bonus", C.c_int32), ("zdrop", C.c_int32)]


class BswResult(C.Structure):
    _fields_ = [("score", C.c_int32), ("qle", C.c_int32), ("tle", C.c_int32), ("gtle", C.c_int32),
                ("gscore", C.c_int32), ("max_off", C.c_int32)]


class Kswr(C.Structure):  # bwa's kswr_t
    _fields_ = [("score", C.c_int32), ("te", C.c_int32), ("qe", C.c_int32), ("score2", C.c_int32),
                ("te2", C.c_int32), ("tb", C.c_int32), ("qb", C.c_int32)]


KSW_XBYTE, KSW_XSTOP, KSW_XSUBO, KSW_XSTART = 0x10000, 0x20000, 0x40000, 0x80000


class BswBatch(C.Structure):
    _fields_ = [("qbuf", C.c_void_p), ("qoff", C.c_void_p), ("qlen", C.c_void_p), ("tbuf", C.c_void_p),
                ("toff", C.c_void_p), ("tlen", C.c_void_p), ("h0", C.c_void_p), ("w", C.c_void_p),
                ("n", C.c_int64), ("qbytes", C.c_int64), ("tbytes", C.c_int64), ("max_qlen", C.c_int32),
                ("max_tlen", C.c_int32)]


def _sig(name, res, args):
    f = getattr(lib, name, None)
    if f is None:
        if os.environ.get("FCSHIP_LIB"):  # an older A/B variant (tools/ab.sh) may predate an entry point
            return None
        raise AttributeError(f"libfcship.so lacks {name}")
    f.restype = res
    f.argtypes = args
    return f


_sig("fcs_device_count", C.c_int, [])
_sig("fcs_last_error", C.c_char_p, [])
_sig("fcs_version", C.c_char_p, [])
_sig("fcs_abi_symbol_count", C.c_int, [])
_sig("fcs_phmm_opts_default", None, [C.POINTER(PhmmOpts)])
_sig("fcs_phmm_compute", C.c_int, [C.POINTER(PhmmRead), C.c_int32, C.POINTER(PhmmHap), C.c_int32, f64p,
                                   C.POINTER(PhmmOpts)])
_sig("fcs_phmm_compute_regions", C.c_int, [C.POINTER(PhmmRegion), C.c_int32, C.POINTER(PhmmOpts)])
_sig("fcs_phmm_compute_pairs", C.c_int, [C.POINTER(PhmmBatch), f64p, C.POINTER(PhmmOpts)])
_sig("fcs_phmm_plan_create", C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_void_p)])
_sig("fcs_phmm_plan_destroy", C.c_int, [C.c_void_p])
_sig("fcs_phmm_dev_schedule", C.c_int, [C.c_void_p, C.POINTER(PhmmBatch), C.c_void_p])
_sig("fcs_phmm_dev_forward", C.c_int, [C.c_void_p, C.POINTER(PhmmBatch), C.c_void_p, C.POINTER(PhmmOpts),
                                       C.c_void_p])
_sig("fcs_phmm_dev_rescue", C.c_int, [C.c_void_p, C.POINTER(PhmmBatch), C.c_void_p, C.POINTER(PhmmOpts),
                                      C.c_void_p])
_sig("fcs_phmm_dev_run", C.c_int, [C.c_void_p, C.POINTER(PhmmBatch), C.c_void_p, C.POINTER(PhmmOpts),
                                   C.c_void_p])
_sig("fcs_phmm_plan_rescue_count", C.c_int, [C.c_void_p, C.c_void_p, i64p])
_sig("fcs_phmm_last_rescued", C.c_int, [i64p])
_sig("fcs_phmm_last_device_ms", C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double)])
_sig("fcs_device_warmup", C.c_int, [C.c_int32, C.c_int32])
_sig("fcs_stream_release", C.c_int, [C.c_int32, C.c_void_p])
_sig("fcs_device_release", C.c_int, [C.c_int32])
_sig("fcs_phmm_partition", C.c_int, [C.POINTER(PhmmBatch), C.c_int32, C.c_void_p])
_sig("fcs_phmm_compute_pairs_multi", C.c_int, [C.POINTER(PhmmBatch), C.c_void_p, C.POINTER(PhmmOpts), C.c_void_p,
                                               C.c_int32])
_sig("fcs_bsw_params_default", None, [C.POINTER(BswParams)])
_sig("fcs_bsw_extend", C.c_int, [C.POINTER(BswTask), C.c_int32, C.POINTER(BswParams), C.POINTER(BswResult),
                                 C.c_int32])
_sig("fcs_bsw_extend_multi", C.c_int, [C.POINTER(BswTask), C.c_int32, C.POINTER(BswParams), C.POINTER(BswResult),
                                       C.c_void_p, C.c_int32])
_sig("fcs_bsw_extend_dev", C.c_int, [C.POINTER(BswBatch), C.POINTER(BswParams), C.c_void_p, C.c_void_p,
                                     C.c_int32, C.c_void_p])
_sig("fcs_bsw_extend_batch", C.c_int, [C.POINTER(BswBatch), C.POINTER(BswParams), i32p, i64p, C.c_int32])
_sig("fcs_bsw_plan_create", C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_void_p)])
_sig("fcs_bsw_plan_destroy", C.c_int, [C.c_void_p])
_sig("fcs_bsw_extend_plan", C.c_int, [C.c_void_p, C.POINTER(BswBatch), C.POINTER(BswParams), C.c_void_p, C.c_void_p,
                                      C.c_void_p])
_sig("fcs_bsw_global", C.c_int, [C.POINTER(BswTask), C.c_int32, C.POINTER(BswParams), i32p, u32p, i64p, i32p,
                                 i32p, C.c_int32])
_sig("fcs_bsw_align", C.c_int, [C.POINTER(BswTask), C.c_int32, C.POINTER(BswParams), i32p, C.c_void_p, C.c_int32])
_sig("fcs_bsw_align_dev", C.c_int, [C.POINTER(BswBatch), C.POINTER(BswParams), C.c_void_p, C.c_void_p, C.c_int32,
                                    C.c_void_p])
_sig("fcs_ksw_align2", Kswr, [C.c_int, u8p, C.c_int, u8p, C.c_int, i8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                              C.c_void_p])
_sig("fcs_bsw_global_dev", C.c_int, [C.POINTER(BswBatch), C.POINTER(BswParams), C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_void_p])
_sig("fcs_ksw_extend2", C.c_int, [C.c_int, u8p, C.c_int, u8p, C.c_int, i8p, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                  C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)])
_sig("fcs_ksw_global2", C.c_int, [C.c_int, u8p, C.c_int, u8p, C.c_int, i8p, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.POINTER(C.c_int), C.POINTER(u32p)])
_sig("fcs_set_default_device", C.c_int, [C.c_int32])
_sig("fcs_bgzf_index", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, i32p, i64p])
_sig("fcs_bgzf_inflate", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, i64p, i64p, C.c_int32])
_sig("fcs_bgzf_inflate_try", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, i64p, i64p, C.c_int32])
_sig("fcs_bgzf_warmup", C.c_int, [C.c_int32, C.c_int32, C.c_int64])
_sig("fcs_bgzf_inflate_dev", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_int32, C.c_void_p])
_sig("fcs_bgzf_deflate_bound", C.c_int64, [C.c_int64, C.c_int32, C.c_int32])
_sig("fcs_bgzf_deflate", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, i64p,
                                   C.c_void_p, i32p, C.c_int32])
_sig("fcs_bgzf_deflate_try", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, i64p,
                                       C.c_void_p, i32p, C.c_int32])
_sig("fcs_bgzf_deflate_dev", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_void_p])
_sig("fcs_fmd_index_create", C.c_int, [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                       C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                       C.POINTER(C.c_void_p)])
_sig("fcs_fmd_index_destroy", C.c_int, [C.c_void_p])
_sig("fcs_fmd_collect", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p])
_sig("fcs_fmd_collect_arena_bytes", C.c_int64, [C.c_int32, C.c_int32])
_sig("fcs_fmd_collect_dev", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p])
_sig("fcs_fmd_locate", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p])
_sig("fcs_fmd_locate_dev", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p])
_sig("fcs_fmd_seed", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                               C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p])
_sig("fcs_fmd_seed_workspace_bytes", C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int64])
_sig("fcs_fmd_seed_dev", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                   C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                   C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p])
_sig("fcs_synth_phmm_sizes", C.c_int, [C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, i64p, i64p])
_sig("fcs_synth_phmm", C.c_int, [C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 10)
_sig("fcs_synth_bsw_sizes", C.c_int, [C.c_uint64, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, i64p, i64p, i64p])
_sig("fcs_synth_bsw", C.c_int, [C.c_uint64, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                C.c_int32] + [C.c_void_p] * 9)

libc = C.CDLL(None)
libc.free.argtypes = [C.c_void_p]


def check(rc: int) -> None:
    if rc != FCS_OK:
        raise FcsError(rc, lib.fcs_last_error().decode(errors="replace"))


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data if a.size else 0


def device_count() -> int:
    return int(lib.fcs_device_count())


def header_symbols() -> list[str]:
    """Function names declared in include/fcship.h."""
    import re
    txt = open(HEADER_PATH).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fcs_[a-z0-9_]+)\s*\(", txt)))


# ---------------------------------------------------------------- PairHMM
@dataclass
class PhmmPairs:
    """SoA pair batch in host numpy arrays (the layout fcs_phmm_batch describes)."""
    read_bases: np.ndarray
    read_bq: np.ndarray
    read_iq: np.ndarray
    read_dq: np.ndarray
    read_gcp: np.ndarray
    read_off: np.ndarray
    read_len: np.ndarray
    hap_bases: np.ndarray
    hap_off: np.ndarray
    hap_len: np.ndarray
    pair_read: np.ndarray
    pair_hap: np.ndarray

    @property
    def n_pairs(self) -> int:
        return int(self.pair_read.size)

    def cells(self) -> int:
        return int((self.read_len[self.pair_read].astype(np.int64) *
                    self.hap_len[self.pair_hap].astype(np.int64)).sum())

    def to_struct(self, ptr=_ptr) -> PhmmBatch:
        b = PhmmBatch()
        b.read_bases, b.read_bq, b.read_iq = ptr(self.read_bases), ptr(self.read_bq), ptr(self.read_iq)
        b.read_dq, b.read_gcp = ptr(self.read_dq), ptr(self.read_gcp)
        b.read_off, b.read_len, b.n_reads = ptr(self.read_off), ptr(self.read_len), int(self.read_len.size)
        b.hap_bases, b.hap_off, b.hap_len = ptr(self.hap_bases), ptr(self.hap_off), ptr(self.hap_len)
        b.n_haps = int(self.hap_len.size)
        b.pair_read, b.pair_hap, b.n_pairs = ptr(self.pair_read), ptr(self.pair_hap), int(self.pair_read.size)
        b.read_bytes, b.hap_bytes = int(self.read_bases.size), int(self.hap_bases.size)
        b.max_read_len = int(self.read_len.max()) if self.read_len.size else 0
        b.max_hap_len = int(self.hap_len.max()) if self.hap_len.size else 0
        return b


def make_pairs(reads, haps, pairs=None) -> PhmmPairs:
    """reads: list of (bases, bq, iq, dq, gcp) byte strings/arrays; haps: list of bytes.
    pairs: list of (read_idx, hap_idx); default = all reads x haps, read-major."""
    def cat(parts):
        arr = [np.frombuffer(bytes(p), dtype=np.uint8) if not isinstance(p, np.ndarray) else p.astype(np.uint8)
               for p in parts]
        return np.concatenate(arr) if arr else np.zeros(0, np.uint8)
    rl = np.array([len(r[0]) for r in reads], dtype=np.int32)
    ro = np.concatenate([[0], np.cumsum(rl[:-1], dtype=np.int64)]).astype(np.int64) if len(reads) else \
        np.zeros(0, np.int64)
    hl = np.array([len(h) for h in haps], dtype=np.int32)
    ho = np.concatenate([[0], np.cumsum(hl[:-1], dtype=np.int64)]).astype(np.int64) if len(haps) else \
        np.zeros(0, np.int64)
    if pairs is None:
        pairs = [(r, h) for r in range(len(reads)) for h in range(len(haps))]
    pr = np.array([p[0] for p in pairs], dtype=np.int32)
    ph = np.array([p[1] for p in pairs], dtype=np.int32)
    return PhmmPairs(cat([r[0] for r in reads]), cat([r[1] for r in reads]), cat([r[2] for r in reads]),
                     cat([r[3] for r in reads]), cat([r[4] for r in reads]), ro, rl, cat(haps), ho, hl, pr, ph)


def phmm_opts(device=0, rescue=True, threshold=1e-28, exact=False) -> PhmmOpts:
    o = PhmmOpts()
    lib.fcs_phmm_opts_default(C.byref(o))
    o.device, o.use_fp64_rescue, o.rescue_threshold, o.exact_order = device, int(rescue), threshold, int(exact)
    return o


def phmm_compute_pairs(p: PhmmPairs, **kw) -> np.ndarray:
    out = np.zeros(p.n_pairs, dtype=np.float64)
    b = p.to_struct()
    o = phmm_opts(**kw)
    check(lib.fcs_phmm_compute_pairs(C.byref(b), out.ctypes.data_as(f64p), C.byref(o)))
    return out


def phmm_partition(p: PhmmPairs, n: int) -> np.ndarray:
    """Cut points of the multi-GPU static partition (cuts[0..n])."""
    cuts = np.zeros(n + 1, dtype=np.int64)
    b = p.to_struct()
    check(lib.fcs_phmm_partition(C.byref(b), n, cuts.ctypes.data))
    return cuts


def phmm_compute_pairs_multi(p: PhmmPairs, devices, **kw) -> np.ndarray:
    out = np.zeros(p.n_pairs, dtype=np.float64)
    b = p.to_struct()
    o = phmm_opts(**kw)
    d = np.asarray(devices, dtype=np.int32)
    check(lib.fcs_phmm_compute_pairs_multi(C.byref(b), out.ctypes.data, C.byref(o), d.ctypes.data, len(d)))
    return out


def phmm_compute(reads, haps, **kw) -> np.ndarray:
    """GKL computeLikelihoodsNative-style dense call: returns [n_reads, n_haps] log10."""
    keep = []

    def u8(x):
        a = np.ascontiguousarray(np.frombuffer(bytes(x), dtype=np.uint8) if not isinstance(x, np.ndarray)
                                 else x.astype(np.uint8))
        keep.append(a)
        return a.ctypes.data_as(u8p)
    R = (PhmmRead * max(len(reads), 1))()
    for i, r in enumerate(reads):
        R[i] = PhmmRead(u8(r[0]), u8(r[1]), u8(r[2]), u8(r[3]), u8(r[4]), len(r[0]))
    H = (PhmmHap * max(len(haps), 1))()
    for i, h in enumerate(haps):
        H[i] = PhmmHap(u8(h), len(h))
    out = np.zeros((len(reads), len(haps)), dtype=np.float64)
    o = phmm_opts(**kw)
    check(lib.fcs_phmm_compute(R, len(reads), H, len(haps), out.ctypes.data_as(f64p), C.byref(o)))
    return out


def phmm_compute_regions(regions, **kw) -> list:
    """Active-region batching: regions = [(reads, haps), ...] with reads as
    (bases, base_q, ins_q, del_q, gcp) tuples; one device pass for all, returns
    one [n_reads, n_haps] log10 matrix per region."""
    keep, outs = [], []

    def u8(x):
        a = np.ascontiguousarray(np.frombuffer(bytes(x), dtype=np.uint8) if not isinstance(x, np.ndarray)
                                 else x.astype(np.uint8))
        keep.append(a)
        return a.ctypes.data_as(u8p)
    G = (PhmmRegion * max(len(regions), 1))()
    for g, (reads, haps) in enumerate(regions):
        R = (PhmmRead * max(len(reads), 1))()
        for i, r in enumerate(reads):
            R[i] = PhmmRead(u8(r[0]), u8(r[1]), u8(r[2]), u8(r[3]), u8(r[4]), len(r[0]))
        H = (PhmmHap * max(len(haps), 1))()
        for i, h in enumerate(haps):
            H[i] = PhmmHap(u8(h), len(h))
        out = np.zeros((len(reads), len(haps)), dtype=np.float64)
        keep += [R, H]
        outs.append(out)
        G[g] = PhmmRegion(C.cast(R, C.POINTER(PhmmRead)), len(reads), C.cast(H, C.POINTER(PhmmHap)), len(haps),
                          out.ctypes.data_as(f64p))
    o = phmm_opts(**kw)
    check(lib.fcs_phmm_compute_regions(G, len(regions), C.byref(o)))
    return outs


def synth_phmm(seed: int, n_pairs: int, R: int = 101, hmin: int = 150, hmax: int = 300) -> PhmmPairs:
    rb_n, hb_n = C.c_int64(), C.c_int64()
    check(lib.fcs_synth_phmm_sizes(seed, n_pairs, R, hmin, hmax, C.byref(rb_n), C.byref(hb_n)))
    rb = [np.zeros(rb_n.value, np.uint8) for _ in range(5)]
    ro = np.zeros(n_pairs, np.int64)
    rl = np.zeros(n_pairs, np.int32)
    hb = np.zeros(hb_n.value, np.uint8)
    ho = np.zeros(n_pairs, np.int64)
    hl = np.zeros(n_pairs, np.int32)
    check(lib.fcs_synth_phmm(seed, n_pairs, R, hmin, hmax, *[_ptr(a) for a in rb], _ptr(ro), _ptr(rl), _ptr(hb),
                             _ptr(ho), _ptr(hl)))
    idx = np.arange(n_pairs, dtype=np.int32)
    return PhmmPairs(rb[0], rb[1], rb[2], rb[3], rb[4], ro, rl, hb, ho, hl, idx, idx.copy())


# ---------------------------------------------------------------- banded SW
def bsw_params(mat=None, o_del=6, e_del=1, o_ins=6, e_ins=1, end_bonus=5, zdrop=100) -> BswParams:
    p = BswParams()
    lib.fcs_bsw_params_default(C.byref(p))
    if mat is not None:
        for i, v in enumerate(np.asarray(mat, dtype=np.int8).ravel()):
            p.mat[i] = int(v)
    p.o_del, p.e_del, p.o_ins, p.e_ins, p.end_bonus, p.zdrop = o_del, e_del, o_ins, e_ins, end_bonus, zdrop
    return p


def default_mat() -> np.ndarray:
    p = BswParams()
    lib.fcs_bsw_params_default(C.byref(p))
    return np.array(list(p.mat), dtype=np.int8)


@dataclass
class BswTasks:
    qbuf: np.ndarray
    qoff: np.ndarray
    qlen: np.ndarray
    tbuf: np.ndarray
    toff: np.ndarray
    tlen: np.ndarray
    h0: np.ndarray
    w: np.ndarray

    @property
    def n(self) -> int:
        return int(self.qlen.size)

    def to_struct(self, ptr=_ptr) -> BswBatch:
        b = BswBatch()
        b.qbuf, b.qoff, b.qlen = ptr(self.qbuf), ptr(self.qoff), ptr(self.qlen)
        b.tbuf, b.toff, b.tlen = ptr(self.tbuf), ptr(self.toff), ptr(self.tlen)
        b.h0, b.w, b.n = ptr(self.h0), ptr(self.w), self.n
        b.qbytes, b.tbytes = int(self.qbuf.size), int(self.tbuf.size)
        b.max_qlen = int(self.qlen.max()) if self.n else 0
        b.max_tlen = int(self.tlen.max()) if self.n else 0
        return b

    def task(self, k: int):
        q = self.qbuf[self.qoff[k]:self.qoff[k] + self.qlen[k]]
        t = self.tbuf[self.toff[k]:self.toff[k] + self.tlen[k]]
        return q, t, int(self.h0[k]), int(self.w[k])


def make_tasks(items) -> BswTasks:
    """items: list of (query codes, target codes, h0, w)."""
    ql = np.array([len(x[0]) for x in items], np.int32)
    tl = np.array([len(x[1]) for x in items], np.int32)
    qo = np.concatenate([[0], np.cumsum(ql[:-1], dtype=np.int64)]).astype(np.int64) if items else np.zeros(0, np.int64)
    to = np.concatenate([[0], np.cumsum(tl[:-1], dtype=np.int64)]).astype(np.int64) if items else np.zeros(0, np.int64)
    qb = np.concatenate([np.asarray(x[0], np.uint8) for x in items]) if items else np.zeros(0, np.uint8)
    tb = np.concatenate([np.asarray(x[1], np.uint8) for x in items]) if items else np.zeros(0, np.uint8)
    return BswTasks(qb, qo, ql, tb, to, tl, np.array([x[2] for x in items], np.int32),
                    np.array([x[3] for x in items], np.int32))


def bsw_extend_batch(t: BswTasks, params: BswParams | None = None, device=0):
    params = params or bsw_params()
    res = np.zeros((t.n, 6), np.int32)
    cells = np.zeros(t.n, np.int64)
    b = t.to_struct()
    check(lib.fcs_bsw_extend_batch(C.byref(b), C.byref(params), res.ctypes.data_as(i32p),
                                   cells.ctypes.data_as(i64p), device))
    return res, cells


def bsw_extend_tasks(t: BswTasks, params: BswParams | None = None, device=0, devices=None):
    """fcs_bsw_extend over an array of fcs_bsw_task (bwa's per-task pointers);
    devices: a list of device slots -> fcs_bsw_extend_multi (static partition)."""
    params = params or bsw_params()
    arr = (BswTask * max(t.n, 1))()
    base_q, base_t = t.qbuf.ctypes.data, t.tbuf.ctypes.data
    for i in range(t.n):
        arr[i] = BswTask(int(t.qlen[i]), int(t.tlen[i]), int(t.h0[i]), int(t.w[i]),
                         C.cast(base_q + int(t.qoff[i]), u8p), C.cast(base_t + int(t.toff[i]), u8p))
    res = (BswResult * max(t.n, 1))()
    if devices is None:
        check(lib.fcs_bsw_extend(arr, t.n, C.byref(params), res, device))
    else:
        d = np.asarray(devices, np.int32)
        check(lib.fcs_bsw_extend_multi(arr, t.n, C.byref(params), res, d.ctypes.data, len(d)))
    return np.array([[r.score, r.qle, r.tle, r.gtle, r.gscore, r.max_off] for r in res[:t.n]], np.int32)


def bsw_global(t: BswTasks, params: BswParams | None = None, device=0, with_cigar=True):
    params = params or bsw_params()
    n = t.n
    tasks = (BswTask * max(n, 1))()
    for k in range(n):
        q, tg, h0, w = t.task(k)
        tasks[k] = BswTask(int(t.qlen[k]), int(t.tlen[k]), 1, w,
                           q.ctypes.data_as(u8p) if q.size else None, tg.ctypes.data_as(u8p) if tg.size else None)
    scores = np.zeros(n, np.int32)
    if not with_cigar:
        check(lib.fcs_bsw_global(tasks, n, C.byref(params), scores.ctypes.data_as(i32p), None, None, None, None,
                                 device))
        return scores, None
    cap = (t.qlen + t.tlen + 2).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(cap[:-1], dtype=np.int64)]).astype(np.int64)
    arena = np.zeros(int(cap.sum()) if n else 1, np.uint32)
    ncig = np.zeros(n, np.int32)
    check(lib.fcs_bsw_global(tasks, n, C.byref(params), scores.ctypes.data_as(i32p), arena.ctypes.data_as(u32p),
                             off.ctypes.data_as(i64p), cap.ctypes.data_as(i32p), ncig.ctypes.data_as(i32p), device))
    cigars = [arena[off[k]:off[k] + ncig[k]].copy() for k in range(n)]
    return scores, cigars


def bsw_align(t: BswTasks, xtra, params: BswParams | None = None, device=0) -> np.ndarray:
    """Batched ksw_align2 (fcs_bsw_align): (n, 7) int32 rows = bwa's kswr_t
    (score, te, qe, score2, te2, tb, qb)."""
    params = params or bsw_params()
    n = t.n
    tasks = (BswTask * max(n, 1))()
    for k in range(n):
        q, tg, _, _ = t.task(k)
        tasks[k] = BswTask(int(t.qlen[k]), int(t.tlen[k]), 0, 0, q.ctypes.data_as(u8p) if q.size else None,
                           tg.ctypes.data_as(u8p) if tg.size else None)
    x = np.ascontiguousarray(np.broadcast_to(np.asarray(xtra, np.int32), (n,)), np.int32)
    out = np.zeros((max(n, 1), 7), np.int32)
    check(lib.fcs_bsw_align(tasks, n, C.byref(params), x.ctypes.data_as(i32p), out.ctypes.data, device))
    return out[:n]


def ksw_align2(q, t, xtra, mat=None, o_del=6, e_del=1, o_ins=6, e_ins=1):
    """bwa's ksw_align2 signature twin: (score, te, qe, score2, te2, tb, qb)."""
    q = np.ascontiguousarray(q, np.uint8)
    t = np.ascontiguousarray(t, np.uint8)
    m = np.ascontiguousarray(default_mat() if mat is None else mat, np.int8)
    r = lib.fcs_ksw_align2(len(q), q.ctypes.data_as(u8p), len(t), t.ctypes.data_as(u8p), 5, m.ctypes.data_as(i8p),
                           o_del, e_del, o_ins, e_ins, xtra, None)
    if r.score == -2147483648:
        raise FcsError(FCS_ERR_DEVICE, lib.fcs_last_error().decode(errors="replace"))
    return (r.score, r.te, r.qe, r.score2, r.te2, r.tb, r.qb)


def ksw_extend2(q, t, h0, w, mat=None, o_del=6, e_del=1, o_ins=6, e_ins=1, end_bonus=5, zdrop=100):
    q = np.ascontiguousarray(q, np.uint8)
    t = np.ascontiguousarray(t, np.uint8)
    m = np.ascontiguousarray(default_mat() if mat is None else mat, np.int8)
    outs = [C.c_int() for _ in range(5)]
    sc = lib.fcs_ksw_extend2(len(q), q.ctypes.data_as(u8p), len(t), t.ctypes.data_as(u8p), 5, m.ctypes.data_as(i8p),
                             o_del, e_del, o_ins, e_ins, w, end_bonus, zdrop, h0, *[C.byref(o) for o in outs])
    if sc == FCS_KSW_FAILED:
        raise FcsError(sc, lib.fcs_last_error().decode(errors="replace"))
    return (sc,) + tuple(o.value for o in outs)


def ksw_global2(q, t, w, mat=None, o_del=6, e_del=1, o_ins=6, e_ins=1):
    q = np.ascontiguousarray(q, np.uint8)
    t = np.ascontiguousarray(t, np.uint8)
    m = np.ascontiguousarray(default_mat() if mat is None else mat, np.int8)
    n = C.c_int()
    cig = u32p()
    sc = lib.fcs_ksw_global2(len(q), q.ctypes.data_as(u8p), len(t), t.ctypes.data_as(u8p), 5,
                             m.ctypes.data_as(i8p), o_del, e_del, o_ins, e_ins, w, C.byref(n), C.byref(cig))
    if sc == FCS_KSW_FAILED:
        raise FcsError(sc, lib.fcs_last_error().decode(errors="replace"))
    ops = np.array([cig[i] for i in range(n.value)], np.uint32)
    if cig:
        libc.free(cig)
    return sc, ops


def synth_bsw(seed: int, n_reads: int, read_len: int = 151, ref_len: int = 10_000_000, w: int = 100,
              mode: int = 0, fixed_q: int = 151, fixed_t: int = 251) -> BswTasks:
    nt, qb, tb = C.c_int64(), C.c_int64(), C.c_int64()
    check(lib.fcs_synth_bsw_sizes(seed, n_reads, read_len, ref_len, w, mode, fixed_q, fixed_t, C.byref(nt),
                                  C.byref(qb), C.byref(tb)))
    n = nt.value
    t = BswTasks(np.zeros(qb.value, np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int32),
                 np.zeros(tb.value, np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int32),
                 np.zeros(n, np.int32), np.zeros(n, np.int32))
    got = C.c_int64()
    check(lib.fcs_synth_bsw(seed, n_reads, read_len, ref_len, w, mode, fixed_q, fixed_t, _ptr(t.qbuf), _ptr(t.qoff),
                            _ptr(t.qlen), _ptr(t.tbuf), _ptr(t.toff), _ptr(t.tlen), _ptr(t.h0), _ptr(t.w),
                            C.byref(got)))
    assert got.value == n
    return t


def cigar_str(ops) -> str:
    return "".join(f"{int(c) >> 4}{'MID'[int(c) & 0xf]}" for c in ops)


FCS_BGZF_OK, FCS_BGZF_CORRUPT, FCS_BGZF_OVERFLOW, FCS_BGZF_CRC = 0, 1, 2, 3
FCS_BGZF_BUSY = 1  # fcs_bgzf_inflate_try's return when no warm inflate session is idle


def bgzf_index(comp, cap: int | None = None):
    """fcs_bgzf_index: (coff, uoff, comp_used) of the whole BGZF members in
    `comp` (bytes / uint8 array); coff / uoff have n + 1 entries."""
    c = np.frombuffer(bytes(comp), np.uint8) if not isinstance(comp, np.ndarray) else np.ascontiguousarray(comp, np.uint8)
    cap = len(c) // 20 + 1 if cap is None else cap
    coff = np.zeros(cap + 1, np.int64)
    uoff = np.zeros(cap + 1, np.int64)
    n, used = C.c_int32(), C.c_int64()
    check(lib.fcs_bgzf_index(_ptr(c), len(c), coff.ctypes.data, uoff.ctypes.data, cap, C.byref(n), C.byref(used)))
    return coff[:n.value + 1].copy(), uoff[:n.value + 1].copy(), used.value


def bgzf_inflate(comp, out_cap: int | None = None, device: int = 0):
    """fcs_bgzf_inflate: (inflated bytes of the whole members, comp_used)."""
    c = np.frombuffer(bytes(comp), np.uint8) if not isinstance(comp, np.ndarray) else np.ascontiguousarray(comp, np.uint8)
    cap = int(bgzf_index(c)[1][-1]) if out_cap is None else out_cap
    out = np.zeros(max(cap, 1), np.uint8)
    used, got = C.c_int64(), C.c_int64()
    check(lib.fcs_bgzf_inflate(_ptr(c), len(c), out.ctypes.data, cap, C.byref(used), C.byref(got), device))
    return out[:got.value].tobytes(), used.value


FCS_BGZF_BLOCK_MAX = 0xff00


def bgzf_deflate(data, block_bytes: int = FCS_BGZF_BLOCK_MAX, eof: bool = False, device: int = 0):
    """fcs_bgzf_deflate: (the BGZF members of `data` cut into blocks of
    `block_bytes`, coff = the n + 1 member starts); `eof` appends the EOF
    member (not in coff)."""
    d = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
    cap = lib.fcs_bgzf_deflate_bound(len(d), block_bytes, int(eof))
    if cap < 0:
        check(int(cap))
    out = np.zeros(max(cap, 1), np.uint8)
    coff = np.zeros(cap // 65536 + 1, np.int64)
    got, n = C.c_int64(), C.c_int32()
    check(lib.fcs_bgzf_deflate(_ptr(d), len(d), block_bytes, int(eof), out.ctypes.data, cap, C.byref(got),
                               coff.ctypes.data, C.byref(n), device))
    return out[:got.value].tobytes(), coff[:n.value + 1].copy()


# ------------------------------------------------------- FMD-index seeding
FCS_FMD_MAX_MEMS_DEFAULT = 128
FCS_FMD_LOCATED, FCS_FMD_STEP_CAP, FCS_FMD_BAD_ROW = 0, 1, 2
FMD_MEM = np.dtype([("k", np.int64), ("l", np.int64), ("s", np.int64), ("qb", np.int32), ("qe", np.int32)])


class FmdParams(C.Structure):
    _fields_ = [("min_len", C.c_int32), ("split_len", C.c_int32), ("split_width", C.c_int32),
                ("max_mems", C.c_int32), ("max_mem_intv", C.c_int64)]


def fmd_index_create(occ, Carr, n_rows, sa, sa_intv, special_rows, special_sa, flen, device: int = 0):
    """fcs_fmd_index_create over host arrays (sa may be None with sa_intv 1); the handle."""
    occ = np.ascontiguousarray(occ, np.uint64)
    Carr = np.ascontiguousarray(Carr, np.int64)
    sa = None if sa is None else np.ascontiguousarray(sa, np.uint64)
    rows = np.ascontiguousarray(special_rows, np.int64)
    ssa = np.ascontiguousarray(special_sa, np.int64)
    h = C.c_void_p()
    check(lib.fcs_fmd_index_create(device, occ.ctypes.data, len(occ), Carr.ctypes.data, n_rows,
                                   None if sa is None else sa.ctypes.data, 0 if sa is None else len(sa), sa_intv,
                                   rows.ctypes.data, ssa.ctypes.data, len(rows), flen, C.byref(h)))
    return h


def fmd_index_destroy(handle) -> None:
    check(lib.fcs_fmd_index_destroy(handle))


def fmd_collect(handle, codes, q_off, q_len, min_len=19, split_len=28, split_width=10, max_mem_intv=20,
                max_mems=FCS_FMD_MAX_MEMS_DEFAULT):
    """fcs_fmd_collect: (mems[n_reads, max_mems] of FMD_MEM, n_mems, overflow)."""
    codes = np.ascontiguousarray(codes, np.uint8)
    q_off = np.ascontiguousarray(q_off, np.int64)
    q_len = np.ascontiguousarray(q_len, np.int32)
    n = len(q_len)
    mems = np.zeros((n, max(max_mems, 1)), FMD_MEM)
    n_mems, overflow = np.zeros(n, np.int32), np.zeros(n, np.int32)
    P = FmdParams(min_len, split_len, split_width, max_mems, max_mem_intv)
    check(lib.fcs_fmd_collect(handle, codes.ctypes.data, len(codes), q_off.ctypes.data, q_len.ctypes.data, n,
                              C.addressof(P), mems.ctypes.data, n_mems.ctypes.data, overflow.ctypes.data))
    return mems, n_mems, overflow


def fmd_locate(handle, rows, max_steps: int = 0):
    """fcs_fmd_locate: (pos, status) of the BWT rows."""
    rows = np.ascontiguousarray(rows, np.int64)
    pos, status = np.zeros(len(rows), np.int64), np.zeros(len(rows), np.int32)
    check(lib.fcs_fmd_locate(handle, rows.ctypes.data, len(rows), max_steps, pos.ctypes.data, status.ctypes.data))
    return pos, status


FCS_FMD_SEED_MORE = 1


class FmdSeedParams(C.Structure):
    _fields_ = [("collect", FmdParams), ("max_occ", C.c_int32), ("max_steps", C.c_int32)]


def fmd_seed(handle, codes, q_off, q_len, min_len=19, split_len=28, split_width=10, max_mem_intv=20,
             max_mems=FCS_FMD_MAX_MEMS_DEFAULT, max_occ=500, max_steps=0, mem_cap=None, row_cap=None, mems=None,
             pos=None):
    """fcs_fmd_seed: (mems, mem_off, pos, row_off, overflow, status).  status is
    FCS_OK (mems / pos hold mem_off[-1] / row_off[-1] entries) or
    FCS_FMD_SEED_MORE (the totals exceed a capacity: mems / pos are as they
    were passed in, and the caller repeats the call with at least the
    totals); nothing is retried here.  Capacities default to a first guess of
    16 SMEMs and 64 rows per read; mems / pos may be passed in (of at least the
    capacities) to see what the call writes."""
    codes = np.ascontiguousarray(codes, np.uint8)
    q_off = np.ascontiguousarray(q_off, np.int64)
    q_len = np.ascontiguousarray(q_len, np.int32)
    n = len(q_len)
    mem_cap = max(16 * n, 4096) if mem_cap is None else int(mem_cap)
    row_cap = max(64 * n, 65536) if row_cap is None else int(row_cap)
    if mems is None:
        mems = np.zeros(max(mem_cap, 1), FMD_MEM)
    if pos is None:
        pos = np.zeros(max(row_cap, 1), np.int64)
    assert mems.dtype == FMD_MEM and pos.dtype == np.int64 and len(mems) >= mem_cap and len(pos) >= row_cap
    mem_off, row_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    overflow = np.zeros(max(n, 1), np.int32)
    P = FmdSeedParams(FmdParams(min_len, split_len, split_width, max_mems, max_mem_intv), max_occ, max_steps)
    rc = lib.fcs_fmd_seed(handle, codes.ctypes.data, len(codes), q_off.ctypes.data, q_len.ctypes.data, n,
                          C.addressof(P), mems.ctypes.data, mem_cap, mem_off.ctypes.data, pos.ctypes.data, row_cap,
                          row_off.ctypes.data, overflow.ctypes.data)
    if rc == FCS_FMD_SEED_MORE:
        return mems, mem_off, pos, row_off, overflow[:n], rc
    check(rc)
    return mems[:mem_off[-1]], mem_off, pos[:row_off[-1]], row_off, overflow[:n], rc


# ---------------------------------------------------------------- duplicate marking (include/fcsdup.h)
DUP_HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "fcsdup.h")
FCSDUP_MAX_REFS, FCSDUP_MAX_LIBS, FCSDUP_MAX_POS = (1 << 21) - 1, (1 << 11) - 1, 1 << 30
FCSDUP_STATUS_POS, FCSDUP_STATUS_FIELD = 1, 2


class DupBatch(C.Structure):
    _fields_ = [("n", C.c_int64), ("flag", C.c_void_p), ("ref_id", C.c_void_p), ("pos", C.c_void_p),
                ("mate", C.c_void_p), ("lib", C.c_void_p), ("cigar", C.c_void_p), ("cigar_off", C.c_void_p),
                ("n_cigar", C.c_int64), ("qual", C.c_void_p), ("qual_off", C.c_void_p), ("n_qual", C.c_int64),
                ("n_ref", C.c_int32), ("n_lib", C.c_int32)]


class DupStats(C.Structure):
    _fields_ = [("examined", C.c_int64), ("pairs", C.c_int64), ("fragments", C.c_int64), ("duplicates", C.c_int64)]


_sig("fcsdup_mark", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p])
_sig("fcsdup_workspace_bytes", C.c_int64, [C.c_int64])
_sig("fcsdup_mark_dev", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p])


def dup_header_symbols() -> list[str]:
    """Function names declared in include/fcsdup.h."""
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(DUP_HEADER_PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fcsdup_[a-z0-9_]+)\s*\(", txt)))


def dup_arrays(flag, ref_id, pos, mate, lib, cigar, cigar_off, qual, qual_off):
    """The batch's arrays in the dtypes fcsdup_batch names."""
    return (np.ascontiguousarray(flag, np.uint16), np.ascontiguousarray(ref_id, np.int32),
            np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(mate, np.int32),
            np.ascontiguousarray(lib, np.int32), np.ascontiguousarray(cigar, np.uint32),
            np.ascontiguousarray(cigar_off, np.int64), np.ascontiguousarray(qual, np.uint8),
            np.ascontiguousarray(qual_off, np.int64))


def dup_batch(arrays, n_ref: int, n_lib: int, n=None, n_cigar=None, n_qual=None) -> DupBatch:
    """fcsdup_batch over host arrays (dup_arrays' tuple, which the caller keeps alive)."""
    flag, ref_id, pos, mate, lib, cigar, cigar_off, qual, qual_off = arrays
    return DupBatch(len(flag) if n is None else n, _ptr(flag), _ptr(ref_id), _ptr(pos), _ptr(mate), _ptr(lib),
                    _ptr(cigar), _ptr(cigar_off), len(cigar) if n_cigar is None else n_cigar, _ptr(qual),
                    _ptr(qual_off), len(qual) if n_qual is None else n_qual, n_ref, n_lib)


def dup_mark(arrays, n_ref: int, n_lib: int, device: int = 0, **kw):
    """fcsdup_mark: (dup[n] uint8, {examined, pairs, fragments, duplicates})."""
    arrays = dup_arrays(*arrays)
    b = dup_batch(arrays, n_ref, n_lib, **kw)
    dup = np.full(max(len(arrays[0]), 1), 0xEE, np.uint8)
    st = DupStats(-1, -1, -1, -1)
    check(lib.fcsdup_mark(device, C.addressof(b), dup.ctypes.data, C.addressof(st)))
    return dup[:len(arrays[0])], dict(examined=st.examined, pairs=st.pairs, fragments=st.fragments,
                                      duplicates=st.duplicates)


# ---------------------------------------------------------------- base quality recalibration (include/fcsbq.h)
BQ_HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "fcsbq.h")
FCSBQ_NQ, FCSBQ_NCTX, FCSBQ_NCYC, FCSBQ_MAX_CYCLE, FCSBQ_MAX_RG = 94, 16, 1000, 500, 1024
FCSBQ_STATUS_FIELD, FCSBQ_STATUS_REF, FCSBQ_STATUS_LONG = 1, 2, 4


class BqBatch(C.Structure):
    _fields_ = [("n", C.c_int64), ("flag", C.c_void_p), ("ref_id", C.c_void_p), ("pos", C.c_void_p),
                ("mapq", C.c_void_p), ("rg", C.c_void_p), ("cigar", C.c_void_p), ("cigar_off", C.c_void_p),
                ("n_cigar", C.c_int64), ("bases", C.c_void_p), ("qual", C.c_void_p), ("base_off", C.c_void_p),
                ("n_bases", C.c_int64), ("qual_absent", C.c_void_p)]


_sig("fcsbq_ref_create", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)])
_sig("fcsbq_ref_destroy", C.c_int, [C.c_void_p])
_sig("fcsbq_count", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p])
_sig("fcsbq_apply", C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
_sig("fcsbq_workspace_bytes", C.c_int64, [C.c_int32])
_sig("fcsbq_count_dev", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p])
_sig("fcsbq_apply_dev", C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p])


def bq_header_symbols() -> list[str]:
    """Function names declared in include/fcsbq.h."""
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(BQ_HEADER_PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fcsbq_[a-z0-9_]+)\s*\(", txt)))


_BQ_DTYPES = (np.uint16, np.int32, np.int32, np.uint8, np.int32, np.uint32, np.int64, np.uint8, np.uint8, np.int64,
              np.uint8)


def bq_arrays(flag, ref_id, pos, mapq, rg, cigar, cigar_off, bases, qual, base_off, qual_absent):
    """The batch's arrays in the dtypes fcsbq_batch names."""
    return tuple(np.ascontiguousarray(a, t) for a, t in zip(
        (flag, ref_id, pos, mapq, rg, cigar, cigar_off, bases, qual, base_off, qual_absent), _BQ_DTYPES))


def bq_batch(arrays, n=None, n_cigar=None, n_bases=None) -> BqBatch:
    """fcsbq_batch over host arrays (bq_arrays' tuple, which the caller keeps alive)."""
    flag, ref_id, pos, mapq, rg, cigar, cigar_off, bases, qual, base_off, absent = arrays
    return BqBatch(len(flag) if n is None else n, _ptr(flag), _ptr(ref_id), _ptr(pos), _ptr(mapq), _ptr(rg), _ptr(cigar),
                   _ptr(cigar_off), len(cigar) if n_cigar is None else n_cigar, _ptr(bases), _ptr(qual), _ptr(base_off),
                   len(bases) if n_bases is None else n_bases, _ptr(absent))


class bq_ref:
    """fcsbq_ref_create / destroy: a device copy of the reference and its known-sites bitmap."""

    def __init__(self, bases, ref_off, known_bits, device: int = 0):
        bases = np.ascontiguousarray(bases, np.uint8)
        ref_off = np.ascontiguousarray(ref_off, np.int64)
        known_bits = np.ascontiguousarray(known_bits, np.uint64)
        assert len(known_bits) >= (int(ref_off[-1]) + 63) // 64
        self.handle = C.c_void_p()
        check(lib.fcsbq_ref_create(device, bases.ctypes.data, ref_off.ctypes.data, len(ref_off) - 1,
                                   known_bits.ctypes.data, C.byref(self.handle)))

    def close(self):
        if self.handle:
            check(lib.fcsbq_ref_destroy(self.handle))
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def bq_count(ref: "bq_ref", arrays, n_rg: int, ctx=None, cyc=None, **kw):
    """fcsbq_count: the batch's counts added to ctx[n_rg, 94, 16, 2] and cyc[n_rg, 94, 1000, 2] (new when None)."""
    arrays = bq_arrays(*arrays)
    b = bq_batch(arrays, **kw)
    ctx = np.zeros((n_rg, FCSBQ_NQ, FCSBQ_NCTX, 2), np.int64) if ctx is None else ctx
    cyc = np.zeros((n_rg, FCSBQ_NQ, FCSBQ_NCYC, 2), np.int64) if cyc is None else cyc
    assert ctx.dtype == np.int64 and cyc.dtype == np.int64 and ctx.flags.c_contiguous and cyc.flags.c_contiguous
    check(lib.fcsbq_count(ref.handle, C.addressof(b), n_rg, ctx.ctypes.data, cyc.ctypes.data))
    return ctx, cyc


def bq_apply(arrays, base, dctx, dcyc, device: int = 0, out=None, **kw):
    """fcsbq_apply: the new quality bytes in the batch's layout."""
    arrays = bq_arrays(*arrays)
    b = bq_batch(arrays, **kw)
    base, dctx, dcyc = (np.ascontiguousarray(a, np.float64) for a in (base, dctx, dcyc))
    out = np.full(max(len(arrays[7]), 1), 0xEE, np.uint8) if out is None else out
    check(lib.fcsbq_apply(device, C.addressof(b), base.shape[0], base.ctypes.data, dctx.ctypes.data, dcyc.ctypes.data,
                          out.ctypes.data))
    return out[:len(arrays[7])]


# ---------------------------------------------------------------- depth of coverage (include/fcsdp.h)
DP_HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "fcsdp.h")
FCSDP_BINS, FCSDP_PIECE_MAX, FCSDP_WINDOW_MAX, FCSDP_ABOVE = 501, 65536, 1 << 30, 15
FCSDP_STATUS_FIELD, FCSDP_STATUS_REF, FCSDP_STATUS_OVERFLOW = 1, 2, 4


class DpBatch(C.Structure):
    _fields_ = [("n", C.c_int64), ("flag", C.c_void_p), ("ref_id", C.c_void_p), ("pos", C.c_void_p),
                ("mapq", C.c_void_p), ("cigar", C.c_void_p), ("cigar_off", C.c_void_p), ("n_cigar", C.c_int64),
                ("bases", C.c_void_p), ("qual", C.c_void_p), ("base_off", C.c_void_p), ("n_bases", C.c_int64),
                ("qual_absent", C.c_void_p)]


class DpParams(C.Structure):
    _fields_ = [("min_mapq", C.c_int32), ("max_mapq", C.c_int32), ("min_baseq", C.c_int32), ("max_baseq", C.c_int32),
                ("include_deletions", C.c_int32)]


class DpWindow(C.Structure):
    _fields_ = [("ref_id", C.c_int32), ("reserved", C.c_int32), ("start", C.c_int64), ("len", C.c_int64),
                ("contig_len", C.c_int64)]


DP_PIECE = np.dtype([("start", np.int32), ("end", np.int32), ("long_index", np.int32), ("reserved", np.int32)])
DP_SUMMARY = np.dtype([("total", np.uint64), ("loci", np.uint32), ("above", np.uint32), ("q1", np.uint32),
                       ("median", np.uint32), ("q3", np.uint32), ("reserved", np.uint32)])

_sig("fcsdp_count", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
_sig("fcsdp_stats", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                              C.c_void_p, C.c_void_p])
_sig("fcsdp_workspace_bytes", C.c_int64, [C.c_int64])
_sig("fcsdp_runs_dev", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
_sig("fcsdp_scan_dev", C.c_int, [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p])
_sig("fcsdp_stats_dev", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])


def dp_header_symbols() -> list[str]:
    """Function names declared in include/fcsdp.h."""
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(DP_HEADER_PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fcsdp_[a-z0-9_]+)\s*\(", txt)))


_DP_DTYPES = (np.uint16, np.int32, np.int32, np.uint8, np.uint32, np.int64, np.uint8, np.int64, np.uint8)


def dp_arrays(flag, ref_id, pos, mapq, cigar, cigar_off, qual, base_off, qual_absent):
    """The batch's arrays in the dtypes fcsdp_batch names."""
    return tuple(np.ascontiguousarray(a, t) for a, t in zip(
        (flag, ref_id, pos, mapq, cigar, cigar_off, qual, base_off, qual_absent), _DP_DTYPES))


def dp_batch(arrays, n=None, n_cigar=None, n_bases=None) -> DpBatch:
    """fcsdp_batch over host arrays (dp_arrays' tuple, which the caller keeps alive)."""
    flag, ref_id, pos, mapq, cigar, cigar_off, qual, base_off, absent = arrays
    return DpBatch(len(flag) if n is None else n, _ptr(flag), _ptr(ref_id), _ptr(pos), _ptr(mapq), _ptr(cigar),
                   _ptr(cigar_off), len(cigar) if n_cigar is None else n_cigar, 0, _ptr(qual), _ptr(base_off),
                   len(qual) if n_bases is None else n_bases, _ptr(absent))


def dp_params(min_mapq=-1, max_mapq=2147483647, min_baseq=-1, max_baseq=127, include_deletions=False) -> DpParams:
    return DpParams(min_mapq, max_mapq, min_baseq, max_baseq, 1 if include_deletions else 0)


def dp_count(arrays, window, params=None, depth=None, device: int = 0, **kw):
    """fcsdp_count: the batch's depths over window = (ref_id, start, len, contig_len), added to depth (new when None)."""
    arrays = dp_arrays(*arrays)
    b = dp_batch(arrays, **kw)
    ref_id, start, length, contig_len = window
    w = DpWindow(ref_id, 0, start, length, contig_len)
    prm = params if params is not None else dp_params()
    depth = np.zeros(length, np.uint32) if depth is None else depth
    assert depth.dtype == np.uint32 and depth.flags.c_contiguous and len(depth) == length
    check(lib.fcsdp_count(device, C.addressof(b), C.addressof(prm), C.addressof(w), _ptr(depth)))
    return depth


def dp_stats(depth, bitmap, pieces, n_long=0, hist=None, long_hist=None, device: int = 0):
    """fcsdp_stats: (hist[501], long_hist[n_long, 501], summary[n_pieces] of DP_SUMMARY); pieces: (start, end, long_index)."""
    depth = np.ascontiguousarray(depth, np.uint32)
    bitmap = np.ascontiguousarray(bitmap, np.uint64)
    assert len(bitmap) >= (len(depth) + 63) // 64
    pc = np.zeros(len(pieces), DP_PIECE)
    for k, (s, e, li) in enumerate(pieces):
        pc[k] = (s, e, li, 0)
    hist = np.zeros(FCSDP_BINS, np.uint64) if hist is None else hist
    long_hist = np.zeros((n_long, FCSDP_BINS), np.uint64) if long_hist is None else long_hist
    summary = np.zeros(len(pieces), DP_SUMMARY)
    check(lib.fcsdp_stats(device, _ptr(depth), _ptr(bitmap), len(depth), _ptr(pc), len(pc), n_long, hist.ctypes.data,
                          _ptr(long_hist), _ptr(summary)))
    return hist, long_hist, summary


# ---------------------------------------------------------------- pileup SNP genotyping (include/fcsug.h)
UG_HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "fcsug.h")
FCSUG_TILE, FCSUG_WINDOW_MAX, FCSUG_TABLE_ROWS = 256, 1 << 24, 94
FCSUG_STATUS_FIELD, FCSUG_STATUS_REF, FCSUG_STATUS_ORDER, FCSUG_STATUS_SITES = 1, 2, 4, 8


class UgBatch(C.Structure):
    _fields_ = DpBatch._fields_


class UgParams(C.Structure):
    _fields_ = [("min_baseq", C.c_int32)]


class UgWindow(C.Structure):
    _fields_ = DpWindow._fields_


UG_SITE = np.dtype([("offset", np.int32), ("ref", np.uint8), ("alt", np.uint8), ("reserved", np.uint16),
                    ("n", np.uint32, 4), ("qsum", np.uint32, 4), ("n_del", np.uint32), ("reserved2", np.uint32),
                    ("mq2", np.uint64), ("gl", np.int64, 3)])

_sig("fcsug_table", C.c_int, [C.c_double, C.c_void_p])
_sig("fcsug_sites", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                              C.c_void_p])
_sig("fcsug_workspace_bytes", C.c_int64, [C.c_int64, C.c_int64])
_sig("fcsug_sites_dev", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                  C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p])


def ug_header_symbols() -> list[str]:
    """Function names declared in include/fcsug.h."""
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(UG_HEADER_PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fcsug_[a-z0-9_]+)\s*\(", txt)))


_UG_DTYPES = (np.uint16, np.int32, np.int32, np.uint8, np.uint32, np.int64, np.uint8, np.uint8, np.int64, np.uint8)


def ug_arrays(flag, ref_id, pos, mapq, cigar, cigar_off, bases, qual, base_off, qual_absent):
    """The batch's arrays in the dtypes fcsug_batch names (bases: ASCII bytes)."""
    return tuple(np.ascontiguousarray(a, t) for a, t in zip(
        (flag, ref_id, pos, mapq, cigar, cigar_off, bases, qual, base_off, qual_absent), _UG_DTYPES))


def ug_batch(arrays, n=None, n_cigar=None, n_bases=None) -> UgBatch:
    """fcsug_batch over host arrays (ug_arrays' tuple, which the caller keeps alive)."""
    flag, ref_id, pos, mapq, cigar, cigar_off, bases, qual, base_off, absent = arrays
    return UgBatch(len(flag) if n is None else n, _ptr(flag), _ptr(ref_id), _ptr(pos), _ptr(mapq), _ptr(cigar),
                   _ptr(cigar_off), len(cigar) if n_cigar is None else n_cigar, _ptr(bases), _ptr(qual), _ptr(base_off),
                   len(qual) if n_bases is None else n_bases, _ptr(absent))


def ug_table(pcr_error: float = 1e-4):
    """fcsug_table: T[94][3] as int64."""
    t = np.zeros((FCSUG_TABLE_ROWS, 3), np.int64)
    check(lib.fcsug_table(pcr_error, t.ctypes.data))
    return t


def ug_sites(arrays, window, ref, table, min_baseq: int = 17, max_sites=None, device: int = 0, **kw):
    """fcsug_sites: the sites (UG_SITE) of window = (ref_id, start, len, contig_len); ref: the window's len ASCII
    reference bytes."""
    arrays = ug_arrays(*arrays)
    b = ug_batch(arrays, **kw)
    ref_id, start, length, contig_len = window
    w = UgWindow(ref_id, 0, start, length, contig_len)
    prm = UgParams(min_baseq)
    ref = np.frombuffer(ref.encode() if isinstance(ref, str) else bytes(ref), np.uint8)
    assert len(ref) == length
    table = np.ascontiguousarray(table, np.int64)
    max_sites = length if max_sites is None else max_sites
    sites = np.zeros(max(max_sites, 1), UG_SITE)
    n = C.c_int64(-1)
    check(lib.fcsug_sites(device, C.addressof(b), C.addressof(prm), C.addressof(w), _ptr(ref), _ptr(table), _ptr(sites),
                          max_sites, C.addressof(n)))
    return sites[:n.value]


# ---------------------------------------------------------------- joint genotyping (include/fcsjg.h)
JG_HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "fcsjg.h")
FCSJG_SAMPLES_MAX, FCSJG_ALTS_MAX, FCSJG_PL_MAX, FCSJG_UNIT_BITS, FCSJG_S_ROWS, FCSJG_GENOTYPES_MAX = 1024, 6, (1 << 20) - 1, 20, 1282, 28
FCSJG_KIND_BLOCK, FCSJG_KIND_CALL, FCSJG_NO_CALL = 0, 1, 255
FCSJG_STATUS_FIELD, FCSJG_STATUS_PL = 1, 2


class JgCohort(C.Structure):
    _fields_ = [("n_samples", C.c_int32), ("reserved", C.c_int32), ("n_records", C.c_int64), ("rec_off", C.c_void_p),
                ("beg", C.c_void_p), ("end", C.c_void_p), ("kind", C.c_void_p), ("alt", C.c_void_p), ("dp", C.c_void_p),
                ("pl", C.c_void_p)]


class JgSites(C.Structure):
    _fields_ = [("n_sites", C.c_int64), ("pos", C.c_void_p), ("n_alt", C.c_void_p)]


class JgModel(C.Structure):
    _fields_ = [("S", C.c_void_p), ("LG", C.c_void_p), ("LP", C.c_void_p), ("min_qual", C.c_int64)]


class JgOut(C.Structure):
    _fields_ = [("q", C.c_void_p), ("mle", C.c_void_p), ("qual", C.c_void_p), ("kept", C.c_void_p), ("ac", C.c_void_p),
                ("an", C.c_void_p), ("dp", C.c_void_p), ("pl_off", C.c_void_p), ("src", C.c_void_p), ("gt", C.c_void_p),
                ("gq", C.c_void_p), ("pl", C.c_void_p), ("max_pl", C.c_int64), ("n_pl", C.c_void_p)]


_sig("fcsjg_tables", C.c_int, [C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p])
_sig("fcsjg_genotype", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
_sig("fcsjg_workspace_bytes", C.c_int64, [C.c_int64, C.c_int32])
_sig("fcsjg_genotype_dev", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_void_p])


def jg_header_symbols() -> list[str]:
    """Function names declared in include/fcsjg.h."""
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(JG_HEADER_PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fcsjg_[a-z0-9_]+)\s*\(", txt)))


# (name, dtype, entries per site, entries per (site, sample)) of fcsjg_out's arrays, in the struct's order
JG_OUT_FIELDS = (("q", np.int64, 6, 0), ("mle", np.int32, 6, 0), ("qual", np.int64, 1, 0), ("kept", np.uint8, 1, 0),
                 ("ac", np.int32, 6, 0), ("an", np.int32, 1, 0), ("dp", np.int64, 1, 0), ("pl_off", np.int64, 1, 0),
                 ("src", np.int64, 0, 1), ("gt", np.uint8, 0, 2), ("gq", np.uint8, 0, 1))
_JG_COHORT_DTYPES = (np.int64, np.int32, np.int32, np.uint8, np.uint8, np.int32, np.int32)


def jg_tables(heterozygosity: float, n_samples: int):
    """fcsjg_tables: (S[1282], LG[4 n + 1], LP[2 n + 1]) as int32."""
    S, LG, LP = np.zeros(FCSJG_S_ROWS, np.int32), np.zeros(4 * n_samples + 1, np.int32), np.zeros(2 * n_samples + 1, np.int32)
    check(lib.fcsjg_tables(heterozygosity, n_samples, S.ctypes.data, LG.ctypes.data, LP.ctypes.data))
    return S, LG, LP


def jg_cohort(rec_off, beg, end, kind, alt, dp, pl, n_samples=None, n_records=None):
    """(fcsjg_cohort over host arrays, the arrays in its dtypes, which the caller keeps alive)."""
    arrays = tuple(np.ascontiguousarray(a, t) for a, t in zip((rec_off, beg, end, kind, alt, dp, pl), _JG_COHORT_DTYPES))
    c = JgCohort(len(arrays[0]) - 1 if n_samples is None else n_samples, 0, len(arrays[1]) if n_records is None else n_records,
                 *(_ptr(a) for a in arrays))
    return c, arrays


def jg_out_arrays(n_sites: int, n_samples: int, max_pl: int, fill=0):
    """{name: array} of fcsjg_out for n_sites x n_samples, pl of max_pl entries and n_pl of one."""
    out = {name: np.full(n_sites * (per_site + per_cell * n_samples), fill, dt) for name, dt, per_site, per_cell in JG_OUT_FIELDS}
    out["pl"] = np.full(max_pl, fill, np.int32)
    out["n_pl"] = np.full(1, fill, np.int64)
    return out


def jg_out(arrays, max_pl=None) -> JgOut:
    return JgOut(*(_ptr(arrays[name]) for name, *_ in JG_OUT_FIELDS), _ptr(arrays["pl"]),
                 len(arrays["pl"]) if max_pl is None else max_pl, arrays["n_pl"].ctypes.data)


def jg_genotype(cohort_arrays, pos, n_alt, tables, min_qual: int, max_pl=None, device: int = 0, entry=None, **kw):
    """fcsjg_genotype: {name: array} of the outputs (pl cut to n_pl) for the cohort's arrays (rec_off, beg, end, kind,
    alt, dp, pl[.][6]) and the sites; entry: another function of the same arguments after the device."""
    c, keep = jg_cohort(*cohort_arrays, **kw)
    pos, n_alt = np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(n_alt, np.uint8)
    S, LG, LP = (np.ascontiguousarray(t, np.int32) for t in tables)
    st = JgSites(len(pos), _ptr(pos), _ptr(n_alt))
    m = JgModel(_ptr(S), _ptr(LG), _ptr(LP), min_qual)
    n = c.n_samples
    max_pl = len(pos) * n * FCSJG_GENOTYPES_MAX if max_pl is None else max_pl
    arrays = jg_out_arrays(len(pos), max(n, 0), max(max_pl, 0))
    o = jg_out(arrays, max_pl)
    if entry is None:
        check(lib.fcsjg_genotype(device, C.addressof(c), C.addressof(st), C.addressof(m), C.addressof(o)))
    else:
        entry(C.addressof(c), C.addressof(st), C.addressof(m), C.addressof(o))
    arrays["pl"] = arrays["pl"][:int(arrays["n_pl"][0])]
    return arrays


# ---------------------------------------------------------------- indel realignment (include/fcsir.h)
IR_HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "fcsir.h")
FCSIR_READ_MAX, FCSIR_SEQ_MAX, FCSIR_OVERHANG, FCSIR_ORIG_MAX = 512, 4096, 99, 1 << 30
FCSIR_STATUS_FIELD, FCSIR_STATUS_PAIRS = 1, 2


class IrBatch(C.Structure):
    _fields_ = [("n_bins", C.c_int64), ("n_seq", C.c_int64), ("n_reads", C.c_int64), ("n_seq_bytes", C.c_int64),
                ("n_read_bytes", C.c_int64), ("seq", C.c_void_p), ("seq_off", C.c_void_p), ("bin_seq", C.c_void_p),
                ("read", C.c_void_p), ("qual", C.c_void_p), ("read_off", C.c_void_p), ("bin_read", C.c_void_p),
                ("orig", C.c_void_p)]


_sig("fcsir_score", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
_sig("fcsir_workspace_bytes", C.c_int64, [C.c_int64])
_sig("fcsir_score_dev", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                  C.c_void_p, C.c_void_p])


def ir_header_symbols() -> list[str]:
    """Function names declared in include/fcsir.h."""
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(IR_HEADER_PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fcsir_[a-z0-9_]+)\s*\(", txt)))


_IR_DTYPES = (np.uint8, np.int64, np.int64, np.uint8, np.uint8, np.int64, np.int64, np.int32)


def ir_batch(seq, seq_off, bin_seq, read, qual, read_off, bin_read, orig, **kw):
    """(fcsir_batch over host arrays, the arrays in its dtypes, which the caller keeps alive); kw overrides the counts."""
    a = tuple(np.ascontiguousarray(x, t) for x, t in zip((seq, seq_off, bin_seq, read, qual, read_off, bin_read, orig), _IR_DTYPES))
    counts = dict(n_bins=len(a[2]) - 1, n_seq=len(a[1]) - 1, n_reads=len(a[5]) - 1, n_seq_bytes=len(a[0]), n_read_bytes=len(a[3]))
    counts.update(kw)
    b = IrBatch(counts["n_bins"], counts["n_seq"], counts["n_reads"], counts["n_seq_bytes"], counts["n_read_bytes"],
                *(_ptr(x) for x in a))
    return b, a


def ir_pairs(bin_seq, bin_read) -> int:
    return int(np.sum(np.diff(np.asarray(bin_seq, np.int64)) * np.diff(np.asarray(bin_read, np.int64))))


def ir_score(arrays, max_pairs=None, device: int = 0, entry=None, **kw):
    """fcsir_score: (best uint32[n_pairs], off int32[n_pairs]) for the arrays (seq, seq_off, bin_seq, read, qual,
    read_off, bin_read, orig); entry: another function (batch, best, off) in its place."""
    b, keep = ir_batch(*arrays, **kw)
    room = ir_pairs(keep[2], keep[6]) if max_pairs is None else max_pairs
    best, off = np.zeros(max(room, 0), np.uint32), np.zeros(max(room, 0), np.int32)
    n = C.c_int64(-1)
    if entry is None:
        check(lib.fcsir_score(device, C.addressof(b), _ptr(best), _ptr(off), room, C.addressof(n)))
    else:
        entry(C.addressof(b), _ptr(best), _ptr(off))
        n.value = room
    return best[:n.value], off[:n.value]


# ---------------------------------------------------------------- the callers' pileup (include/fcspu.h)
PU_HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "fcspu.h")
FCSPU_TILE, FCSPU_WINDOW_MAX, FCSPU_TABLE_ROWS, FCSPU_BATCHES_MAX = 256, 1 << 24, 94, 2
(FCSPU_STATUS_FIELD, FCSPU_STATUS_REF, FCSPU_STATUS_ORDER, FCSPU_STATUS_SITES, FCSPU_STATUS_SNVS,
 FCSPU_STATUS_LETTER) = 1, 2, 4, 8, 16, 32


class PuParams(C.Structure):
    _fields_ = [("min_bq", C.c_int32), ("want_gl", C.c_int32), ("frac", C.c_double)]


class PuOut(C.Structure):
    _fields_ = [("depth", C.c_void_p), ("events", C.c_void_p), ("gl", C.c_void_p), ("sites", C.c_void_p),
                ("max_sites", C.c_int64), ("n_sites", C.c_void_p), ("snvs", C.c_void_p), ("max_snvs", C.c_int64),
                ("n_snvs", C.c_void_p)]


PU_SNV = np.dtype([("offset", np.int32), ("alt", np.uint8), ("reserved", np.uint8, 3), ("count", np.int32)])
assert PU_SNV.itemsize == 12

_sig("fcspu_pile", C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p])
_sig("fcspu_workspace_bytes", C.c_int64, [C.c_void_p, C.c_int32, C.c_int64])
_sig("fcspu_pile_dev", C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p])


def pu_header_symbols() -> list[str]:
    """Function names declared in include/fcspu.h (fcspu_table is libfcsgenome's)."""
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(PU_HEADER_PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fcspu_[a-z0-9_]+)\s*\(", txt)))


def pu_table():
    """fcspu_table: the callers' reference model T[94][3] as float64, from libfcsgenome.so (host only)."""
    host = C.CDLL(os.path.join(HERE, "libfcsgenome.so"))
    t = np.zeros((FCSPU_TABLE_ROWS, 3), np.float64)
    if host.fcspu_table(C.c_void_p(t.ctypes.data)) != 0:
        raise RuntimeError("fcspu_table failed")
    return t


def pu_workspace_bytes(n_records, length) -> int:
    n = np.ascontiguousarray(n_records, np.int64)
    return int(lib.fcspu_workspace_bytes(n.ctypes.data, len(n), length))


def pu_out(length, want_gl=True, max_sites=None, max_snvs=None):
    """(fcspu_out over fresh host arrays, the arrays by name, which the caller keeps alive)."""
    max_sites = length if max_sites is None else max_sites
    max_snvs = 4 * length if max_snvs is None else max_snvs
    a = dict(depth=np.full(length, -1, np.int32), events=np.full(length, -1, np.int32),
             gl=np.full(3 * length if want_gl else 0, np.nan, np.float64), sites=np.full(max(max_sites, 1), -1, np.int32),
             snvs=np.zeros(max(max_snvs, 1), PU_SNV), n_sites=np.full(1, -7, np.int64), n_snvs=np.full(1, -7, np.int64))
    o = PuOut(_ptr(a["depth"]), _ptr(a["events"]), _ptr(a["gl"]), a["sites"].ctypes.data, max_sites, a["n_sites"].ctypes.data,
              a["snvs"].ctypes.data, max_snvs, a["n_snvs"].ctypes.data)
    return o, a


def pu_pile(batches, window, ref, table, min_bq: int = 10, frac: float = 0.15, want_gl: bool = True, events_in=None,
            max_sites=None, max_snvs=None, device: int = 0, entry=None, kw=None, clock=None):
    """fcspu_pile over one or two batches (ug_arrays' argument tuples) and window = (ref_id, start, len, contig_len);
    ref: the window's len ASCII reference bytes.  Returns dict(depth, events, gl[len][3] or None, sites, snvs (PU_SNV)).
    entry: another function (batches, n, params, window, ref, events_in, out) in its place (the host statement);
    kw: per batch, ug_batch's count overrides; clock: a dict that takes the seconds spent inside the entry."""
    import time
    keep = [ug_arrays(*b) for b in batches]
    kw = kw or [{}] * len(keep)
    arr = (UgBatch * len(keep))(*[ug_batch(a, **k) for a, k in zip(keep, kw)])
    ref_id, start, length, contig_len = window
    w = UgWindow(ref_id, 0, start, length, contig_len)
    prm = PuParams(min_bq, int(want_gl), frac)
    ref = np.frombuffer(ref.encode() if isinstance(ref, str) else bytes(ref), np.uint8)
    assert len(ref) == length
    table = np.ascontiguousarray(table, np.float64)
    ev = None if events_in is None else np.ascontiguousarray(events_in, np.int32)
    o, a = pu_out(length, want_gl, max_sites, max_snvs)
    evp = 0 if ev is None else ev.ctypes.data
    t0 = time.perf_counter()
    if entry is None:
        check(lib.fcspu_pile(device, C.addressof(arr), len(keep), C.addressof(prm), C.addressof(w), _ptr(ref), table.ctypes.data,
                             evp, C.addressof(o)))
    else:
        entry(C.addressof(arr), len(keep), C.addressof(prm), C.addressof(w), _ptr(ref), evp, C.addressof(o))
    if clock is not None:
        clock["seconds"] = time.perf_counter() - t0
    ns, nv = int(a["n_sites"][0]), int(a["n_snvs"][0])
    return dict(depth=a["depth"], events=a["events"], gl=a["gl"].reshape(length, 3) if want_gl else None,
                sites=a["sites"][:ns].copy(), snvs=a["snvs"][:nv].copy())


# ---------------------------------------------------------------- minimizer chaining (include/fcsmm.h)
MM_HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "fcsmm.h")
FCSMM_LOOKBACK, FCSMM_SPAN_MAX, FCSMM_GAP_MAX, FCSMM_READ_ANCHORS = 64, 64, 1 << 20, 1 << 24
FCSMM_STATUS_FIELD, FCSMM_STATUS_ORDER = 1, 2


class MmBatch(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_anchors", C.c_int64), ("t", C.c_void_p), ("q", C.c_void_p),
                ("read_off", C.c_void_p), ("max_gap", C.c_int32), ("bw", C.c_int32), ("span", C.c_int32),
                ("reserved", C.c_int32)]


_sig("fcsmm_chain", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p])
_sig("fcsmm_workspace_bytes", C.c_int64, [C.c_int64, C.c_int64])
_sig("fcsmm_chain_dev", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p])


def mm_header_functions() -> list[str]:
    """Function names declared in include/fcsmm.h."""
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(MM_HEADER_PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fcsmm_[a-z0-9_]+)\s*\(", txt)))


_MM_DTYPES = (np.int64, np.int32, np.int64)


def mm_batch(t, q, read_off, max_gap: int = 100, bw: int = 50, span: int = 21, **kw):
    """(fcsmm_batch over host arrays, the arrays in its dtypes, which the caller keeps alive); kw overrides the counts."""
    a = tuple(np.ascontiguousarray(x, d) for x, d in zip((t, q, read_off), _MM_DTYPES))
    counts = dict(n_reads=len(a[2]) - 1, n_anchors=len(a[0]))
    counts.update(kw)
    b = MmBatch(counts["n_reads"], counts["n_anchors"], *(_ptr(x) for x in a), max_gap, bw, span, 0)
    return b, a


def mm_chain(arrays, max_gap: int = 100, bw: int = 50, span: int = 21, device: int = 0, entry=None, fill=-7, **kw):
    """fcsmm_chain: (f int32[n_anchors], p int32[n_anchors]) for the arrays (t, q, read_off); entries no read holds keep
    `fill`.  entry: another function (batch, f, p) in its place (the host statement)."""
    b, keep = mm_batch(*arrays, max_gap=max_gap, bw=bw, span=span, **kw)
    f, p = np.full(len(keep[0]), fill, np.int32), np.full(len(keep[0]), fill, np.int32)
    if entry is None:
        check(lib.fcsmm_chain(device, C.addressof(b), _ptr(f), _ptr(p)))
    else:
        entry(C.addressof(b), _ptr(f), _ptr(p))
    return f, p
