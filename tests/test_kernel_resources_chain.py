"""Scratch, registers and LDS of the chaining kernel
(falcon-genome_amd/csrc/mm_chain.hip) from the compiler's resource remarks
(tools/kernel_resources.py; no GPU): the kernel uses no scratch, reaches the
waves per SIMD the file's header comment says it is built for, the VGPR and LDS
figures are the ones in DESIGN §4.16's table, and its static LDS is not above
64 KB.
"""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

SOURCE = "csrc/mm_chain.hip"
KERNELS = {"mm_chain_kernel"}
NAME = r"mm_\w+?_kernel"


def design_table():
    """{kernel: (VGPRs, LDS bytes, waves per SIMD)} of the §4.16 resource table."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text.split("### 4.16", 1)[1].split("\n### ", 1)[0].split("\n## ", 1)[0]
    return {m.group(1): tuple(int(m.group(k)) for k in (2, 3, 4))
            for m in re.finditer(rf"^\| `({NAME})` \| (\d+) \| (\d+) \| (\d+) \|", sec, re.M)}


def kernel_name(mangled):
    m = re.search(r"\d+(mm_\w+?_kernel)E", mangled)
    return None if m is None else m.group(1)


@pytest.mark.skipif(kernel_resources.hipcc() is None or shutil.which("make") is None, reason="hipcc not installed")
def test_chain_kernel_has_no_scratch_and_the_design_table_s_figures():
    text = open(os.path.join(ROOT, "falcon-genome_amd", SOURCE)).read()
    claimed = {k: int(w) for k, w in re.findall(rf"({NAME}) is built for (\d+) waves per SIMD", text)}
    found = [r for r in kernel_resources.kernel_resources(SOURCE) if kernel_name(r["mangled"])]
    names = {kernel_name(r["mangled"]) for r in found}
    table = design_table()
    assert names == KERNELS == set(claimed) == set(table), (names, set(claimed), set(table))
    assert "asm" not in re.sub(r"//.*", "", text)   # plain C++ and builtins: no inline assembly in this file
    for r in found:
        name = kernel_name(r["mangled"])
        print(f"{name}: {r['vgprs']} VGPRs, {r['agprs']} AGPRs, {r['sgprs']} SGPRs, scratch {r['scratch']}, "
              f"static LDS {r['lds_static']} B, {r['occupancy']} waves/SIMD; built for {claimed[name]}")
        assert r["scratch"] == 0, r
        assert r["occupancy"] >= claimed[name] >= 1, r
        assert r["lds_static"] <= 65536, r
        assert (r["vgprs"], r["lds_static"], claimed[name]) == table[name], (name, r, table[name])
