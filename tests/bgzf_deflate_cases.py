"""Inputs and checks shared by the BGZF deflate tests (SURVEY.md §8 row f3,
the writing side): the shapes at which the encoder can still go wrong, and
the member checks both the host build (tools/micro/deflate_test.cpp) and the
GPU kernel (fcs_bgzf_deflate) have to pass."""
import functools
import struct
import zlib

import numpy as np

import bgzf_cases

BLOCK_MAX = 0xff00
BLOCK_BYTES = (1, 64, 4096, BLOCK_MAX)
KINDS = ("random", "runs", "gvcf", "bam")


def no_repeats(n: int) -> bytes:
    """n <= 0xff00 bytes in which no three consecutive bytes occur twice: the
    16-bit counters 0, 1, 2, ... high byte first."""
    a = np.arange((n + 1) // 2, dtype=np.uint16)
    d = np.stack([a >> 8, a & 255], axis=1).astype(np.uint8).reshape(-1)[:n]
    tri = d[:-2].astype(np.uint32) << 16 | d[1:-1].astype(np.uint32) << 8 | d[2:]
    assert len(np.unique(tri)) == len(tri)
    return d.tobytes()


def fibonacci(rng) -> bytes:
    """22 byte values with Fibonacci counts, shuffled (46,367 bytes): the
    unconstrained Huffman tree is 21 deep, so the 15-bit limit is exercised."""
    f = [1, 1]
    while len(f) < 22:
        f.append(f[-1] + f[-2])
    d = np.repeat(np.arange(22, dtype=np.uint8) * 7 + 40, f)
    rng.shuffle(d)
    return d.tobytes()


@functools.lru_cache(maxsize=None)
def special():
    """[(label, bytes)]: one block of 0xff00 bytes (or less) each."""
    rng = np.random.default_rng(41)
    pre = bgzf_cases.payload(rng, "random", 32769)
    half = no_repeats(BLOCK_MAX // 2)
    out = [("one-byte-run", b"G" * BLOCK_MAX),
           ("no-repeats", no_repeats(BLOCK_MAX)),            # all literals, no distance code
           ("one-distance", half + half),                    # every match 32,640 back
           ("window-limit", (pre[:32768] * 2)[:BLOCK_MAX]),  # matches exactly 32,768 back
           ("past-window", (pre * 2)[:BLOCK_MAX]),           # 32,769 back: must not match
           ("fibonacci", fibonacci(rng))]
    return out


@functools.lru_cache(maxsize=None)
def kinds():
    """[(label, bytes)]: the four payload kinds at 300, 4,000 and 0xff00 bytes."""
    rng = np.random.default_rng(17)
    return [(f"{k}-{n}", bgzf_cases.payload(rng, k, n)) for k in KINDS for n in (300, 4000, BLOCK_MAX)]


def lengths(bb: int):
    return sorted({0, 1, 2, 3, 4, 257, 258, 259, bb - 1, bb, bb + 1, 3 * bb + 7})


@functools.lru_cache(maxsize=None)
def text(n: int) -> bytes:
    return bgzf_cases.payload(np.random.default_rng(n + 5), "gvcf", n)


@functools.lru_cache(maxsize=None)
def cases():
    """[(label, bytes, block_bytes)]: every length at every block size, then
    the special and the kind payloads at the largest block."""
    out = [(f"len{n}-bb{bb}", text(n), bb) for bb in BLOCK_BYTES for n in lengths(bb)]
    out += [(lab, d, BLOCK_MAX) for lab, d in special() + kinds()]
    return out


def blocks(data: bytes, bb: int):
    return [data[k:k + bb] for k in range(0, len(data), bb)]


def zsize(block: bytes, level: int, strategy: int) -> int:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return len(c.compress(block) + c.flush())


def check_payload(label: str, raw: bytes, block: bytes):
    """One raw-DEFLATE payload of one block: zlib gives the block back, the
    payload is no larger than the stored form, and the size conditions hold."""
    d = zlib.decompressobj(-15)
    assert d.decompress(raw) == block and d.eof and not d.unused_data, label
    assert len(raw) <= len(block) + 5, (label, len(raw))
    kind = label.split("-")[0]
    if len(block) == BLOCK_MAX and kind in ("gvcf", "bam", "runs"):
        # only real matches and dynamic codes together get below both
        bound = min(zsize(block, 1, zlib.Z_FIXED), zsize(block, 1, zlib.Z_HUFFMAN_ONLY))
        print(f"{label}: payload {len(raw)}, zlib level 1 {zsize(block, 1, zlib.Z_DEFAULT_STRATEGY)}, "
              f"min(level 1 Z_FIXED, Z_HUFFMAN_ONLY) {bound}")
        assert len(raw) <= bound, (label, len(raw), bound)


def check_member(label: str, m: bytes, block: bytes):
    """One whole BGZF member of one block."""
    assert m[:16] == bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0]), label
    assert struct.unpack("<H", m[16:18])[0] == len(m) - 1, label
    assert len(m) <= 65536 and len(m) <= len(block) + 5 + 26, (label, len(m))
    crc, isize = struct.unpack("<II", m[-8:])
    assert isize == len(block) and crc == (zlib.crc32(block) & 0xFFFFFFFF), label
    check_payload(label, m[18:-8], block)
