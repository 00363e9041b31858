"""Register, scratch and LDS budgets of the queue-fed column kernel
(phmm6_kernel, falcon-genome_amd/csrc/phmm_cols.h), from the compiler's
resource remarks (tools/kernel_resources.py; about a minute of compile, no
GPU).  The kernel runs 3 waves per SIMD, 12 per CU: no scratch, no AGPRs,
<= 168 VGPRs (512 per SIMD lane, allocation granule 8), no static LDS and
dynamic LDS <= 13,653 B per wave (12 waves share the CU's 163,840 B).  It must
exist for every class the launcher can dispatch it for.
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


def header_constant(name):
    text = open(os.path.join(CSRC, "phmm_cols.h")).read()

    def const(n):
        expr = re.search(r"constexpr int %s = ([^;]+);" % n, text).group(1)
        return int(eval(re.sub(r"kCols[16]\w+", lambda m: str(const(m.group(0))), expr)))
    return const(name)


def dispatched_classes():
    """The C of every `launch(phmm6_kernel<C>)` in the launcher."""
    text = open(os.path.join(CSRC, "phmm_kernels.hip")).read()
    return sorted({int(c) for c in re.findall(r"launch\(phmm6_kernel<(\d+)>\)", text)})


@pytest.mark.skipif(kernel_resources.hipcc() is None or shutil.which("make") is None, reason="hipcc not installed")
def test_queue_kernel_fits_three_waves():
    lds = header_constant("kCols6Lds")
    classes = dispatched_classes()
    assert classes, "the launcher dispatches phmm6_kernel for no class"
    assert set(classes) <= {11, 12, 13, 14, 15, 16, 17, 19}, classes
    rows = {r["name"]: r for r in kernel_resources.kernel_resources() if r["name"].startswith("phmm6_kernel<")}
    assert sorted(rows) == sorted("phmm6_kernel<%d>" % c for c in classes), sorted(rows)
    for name, r in rows.items():
        print(f"{name}: {r['vgprs']} VGPRs, {r['sgprs']} SGPRs, scratch {r['scratch']}, "
              f"{r['occupancy']} waves/SIMD, dynamic LDS {lds} B")
        assert r["occupancy"] >= 3, (name, r)
        assert r["scratch"] == 0, (name, r)
        assert r["agprs"] == 0, (name, r)
        assert r["vgprs"] <= 168, (name, r)
        assert r["lds_static"] == 0 and lds <= 13653, (name, lds)
