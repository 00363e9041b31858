"""Scratch, registers and LDS of the callers' pileup kernels
(falcon-genome_amd/csrc/pileup.hip) from the compiler's resource remarks
(tools/kernel_resources.py; no GPU): no kernel uses scratch, each reaches the
waves per SIMD the file's header comment says it is built for, the VGPR and LDS
figures are the ones in DESIGN §4.15's table, and no kernel's static LDS is
above 64 KB.
"""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

SOURCE = "csrc/pileup.hip"
KERNELS = {"pu_span_kernel", "pu_offsets_kernel", "pu_scan_kernel", "pu_pile_kernel", "pu_slots_kernel", "pu_emit_kernel"}


def design_table():
    """{kernel: (VGPRs, LDS bytes, waves per SIMD)} of the §4.15 resource table."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text.split("### 4.15", 1)[1].split("\n### ", 1)[0]
    return {m.group(1): tuple(int(m.group(k)) for k in (2, 3, 4))
            for m in re.finditer(r"^\| `(pu_\w+_kernel)` \| (\d+) \| (\d+) \| (\d+) \|", sec, re.M)}


@pytest.mark.skipif(kernel_resources.hipcc() is None or shutil.which("make") is None, reason="hipcc not installed")
def test_pileup_kernels_have_no_scratch_and_the_design_table_s_figures():
    text = open(os.path.join(ROOT, "falcon-genome_amd", SOURCE)).read()
    claimed = {k: int(w) for k, w in re.findall(r"(pu_\w+_kernel) is built for (\d+) waves per SIMD", text)}
    found = [r for r in kernel_resources.kernel_resources(SOURCE) if re.search(r"\d+pu_\w+?_kernelE", r["mangled"])]
    names = {re.search(r"pu_\w+?_kernel(?=E)", r["mangled"]).group(0) for r in found}
    table = design_table()
    assert names == KERNELS == set(claimed) == set(table), (names, set(claimed), set(table))
    for r in found:
        name = re.search(r"pu_\w+?_kernel(?=E)", r["mangled"]).group(0)
        print(f"{name}: {r['vgprs']} VGPRs, {r['agprs']} AGPRs, {r['sgprs']} SGPRs, scratch {r['scratch']}, "
              f"static LDS {r['lds_static']} B, {r['occupancy']} waves/SIMD; built for {claimed[name]}")
        assert r["scratch"] == 0, r
        assert r["occupancy"] >= claimed[name] >= 1, r
        assert r["lds_static"] <= 65536, r
        assert (r["vgprs"], r["lds_static"], claimed[name]) == table[name], (name, r, table[name])
