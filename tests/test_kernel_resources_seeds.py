"""Scratch and occupancy of the fused seeding call's kernels
(falcon-genome_amd/csrc/fmd_seeds.hip) from the compiler's resource remarks
(tools/kernel_resources.py; no GPU): no kernel uses scratch, each reaches the
waves per SIMD the file's header comment says it is built for, and the header
speaks of exactly the kernels the file holds.
"""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

SOURCE = "csrc/fmd_seeds.hip"


@pytest.mark.skipif(kernel_resources.hipcc() is None or shutil.which("make") is None, reason="hipcc not installed")
def test_seeds_kernels_have_no_scratch_and_their_declared_occupancy():
    text = open(os.path.join(ROOT, "falcon-genome_amd", SOURCE)).read()
    claimed = {k: int(w) for k, w in re.findall(r"(fmd_seed_\w+_kernel) is built for (\d+) waves per SIMD", text)}
    found = kernel_resources.kernel_resources(SOURCE)
    # by the mangled name: the kernels sit in an anonymous namespace, which the tool's demangled names drop
    names = {m.group(0) for r in found for m in [re.search(r"fmd_seed_\w+?_kernel", r["mangled"])] if m}
    assert len(names) == len(found), [r["mangled"] for r in found]
    assert set(claimed) == names and {"fmd_seed_order_kernel", "fmd_seed_expand_kernel"} <= names, (claimed, names)
    for name, waves in claimed.items():
        match = [r for r in found if name in r["mangled"]]
        assert len(match) == 1, [r["mangled"] for r in found]
        r = match[0]
        print(f"{name}: {r['vgprs']} VGPRs, {r['agprs']} AGPRs, {r['sgprs']} SGPRs, scratch {r['scratch']}, "
              f"static LDS {r['lds_static']} B, {r['occupancy']} waves/SIMD; built for {waves}")
        assert r["scratch"] == 0, r
        assert waves >= 1 and r["occupancy"] >= waves, r
