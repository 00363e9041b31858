"""Register, scratch and LDS budgets of the single-stream column kernel
(phmm5_kernel, falcon-genome_amd/csrc/phmm_cols.h), from the compiler's
resource remarks (tools/kernel_resources.py; about a minute of compile, no
GPU).  Every class must fit the waves per SIMD it is compiled for: no
scratch, <= 168 VGPRs at 3 waves and <= 128 at 4 (512 VGPRs per SIMD lane,
allocation granule 8), dynamic LDS <= 10,240 B per wave at 4 waves (16 waves
share the CU's 163,840 B) and <= 13,653 B at 3.  Only the figures are read.
"""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402


def header_constants():
    text = open(os.path.join(ROOT, "falcon-genome_amd", "csrc", "phmm_cols.h")).read()

    def const(name):
        expr = re.search(r"constexpr int %s = ([^;]+);" % name, text).group(1)
        return int(eval(re.sub(r"kCols1\w+", lambda m: str(const(m.group(0))), expr)))
    return const("kCols1Lds")


@pytest.mark.skipif(kernel_resources.hipcc() is None or shutil.which("make") is None, reason="hipcc not installed")
def test_single_stream_kernel_fits_its_declared_occupancy():
    lds = header_constants()
    rows = {r["name"]: r for r in kernel_resources.kernel_resources() if r["name"].startswith("phmm5_kernel<")}
    assert sorted(rows) == sorted("phmm5_kernel<%d>" % c for c in (11, 12, 13, 14, 15, 16, 17, 19)), sorted(rows)
    for name, r in rows.items():
        w = r["occupancy"]  # what __launch_bounds__ and the registers give: a class declared 4-wave spills or shows 4
        print(f"{name}: {r['vgprs']} VGPRs, {r['sgprs']} SGPRs, scratch {r['scratch']}, {w} waves/SIMD, "
              f"dynamic LDS {lds} B")
        assert w >= 3, (name, r)
        assert r["scratch"] == 0, (name, r)
        assert r["agprs"] == 0, (name, r)
        assert r["vgprs"] <= (128 if w >= 4 else 168), (name, r)
        assert r["lds_static"] == 0 and lds <= (10240 if w >= 4 else 13653), (name, lds)
