"""Four waves per SIMD for the queue-fed column kernel (phmm6_kernel,
falcon-genome_amd/csrc/phmm_cols.h), from the compiler's resource remarks
(tools/kernel_resources.py; about a minute of compile, no GPU).  Four waves
share a SIMD's 512 VGPRs per lane, so a four-wave class holds <= 128 of them,
with no scratch and no AGPRs, and sixteen waves share the CU's 163,840 B of LDS
in 1,280-byte granules, so the dynamic LDS per wave is <= 10,240 B.  That is
asserted for every class `cols6_waves` puts at 4, and for C = 11..14 whatever
the table says: they fitted before the staged row was packed and must keep
fitting.  (The measurement of DESIGN §4.1j left the table at 3 for every
class: the fourth wave is resident and buys nothing.  The table decides the
launch bound and the grid; what is held here is that the option stays open.)
"""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

CSRC = os.path.join(ROOT, "falcon-genome_amd", "csrc")
CLASSES = (11, 12, 13, 14, 15, 16, 17, 19)


def header():
    return open(os.path.join(CSRC, "phmm_cols.h")).read()


def header_constant(name):
    text = header()

    def const(n):
        expr = re.search(r"constexpr int %s = ([^;]+);" % n, text).group(1)
        return int(eval(re.sub(r"kCols[16]\w+", lambda m: str(const(m.group(0))), expr)))
    return const(name)


def cols6_waves():
    """{C: waves per SIMD} from the header's `cols6_waves`: its body is one
    return of an expression in C (?: and comparisons)."""
    m = re.search(r"constexpr int cols6_waves\(int C\) \{ return ([^;]+); \}", header())
    assert m, "cols6_waves(int C) not found in phmm_cols.h"
    expr = m.group(1).strip()

    def ev(e, C):
        e = e.strip()
        depth = 0
        for i, ch in enumerate(e):  # the outermost ?: (right-associative)
            depth += ch == "("
            depth -= ch == ")"
            if ch == "?" and depth == 0:
                j, nest = i + 1, 0
                while e[j] != ":" or nest:
                    nest += e[j] == "?"
                    nest -= e[j] == ":"
                    j += 1
                return ev(e[i + 1:j], C) if ev(e[:i], C) else ev(e[j + 1:], C)
        assert re.fullmatch(r"[C\d\s<>=!&|()+\-]+", e), e
        return int(eval(e.replace("&&", " and ").replace("||", " or "), {"C": C}))
    return {C: ev(expr, C) for C in CLASSES}


def test_table_parses():
    w = cols6_waves()
    assert set(w.values()) <= {3, 4}, w


@pytest.mark.skipif(kernel_resources.hipcc() is None or shutil.which("make") is None, reason="hipcc not installed")
def test_four_wave_classes_fit():
    waves = cols6_waves()
    four = sorted({C for C, w in waves.items() if w >= 4} | {11, 12, 13, 14})
    lds = header_constant("kCols6Lds")
    assert lds <= 10240, lds
    rows = {r["name"]: r for r in kernel_resources.kernel_resources() if r["name"].startswith("phmm6_kernel<")}
    for C in CLASSES:
        r = rows["phmm6_kernel<%d>" % C]
        print(f"phmm6_kernel<{C}>: table {waves[C]}, {r['vgprs']} VGPRs, {r['agprs']} AGPRs, scratch {r['scratch']}, "
              f"{r['occupancy']} waves/SIMD, dynamic LDS {lds} B")
    for C in four:
        r = rows["phmm6_kernel<%d>" % C]
        assert r["occupancy"] >= 4, (C, r)
        assert r["vgprs"] <= 128, (C, r)
        assert r["scratch"] == 0 and r["agprs"] == 0, (C, r)
        assert r["lds_static"] == 0, (C, r)
