"""Scratch and occupancy of the FMD-index seeding kernels
(falcon-genome_amd/csrc/fmd_seed.hip) from the compiler's resource remarks
(tools/kernel_resources.py; no GPU): neither kernel uses scratch (the shared
per-read logic of csrc/fmd_smem.h keeps no dynamically indexed array and no
struct temporary), and each reaches the waves per SIMD its header comment says
it is built for.
"""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

SOURCE = "csrc/fmd_seed.hip"


@pytest.mark.skipif(kernel_resources.hipcc() is None or shutil.which("make") is None, reason="hipcc not installed")
def test_seed_kernels_have_no_scratch_and_their_declared_occupancy():
    text = open(os.path.join(ROOT, "falcon-genome_amd", SOURCE)).read()
    claimed = {k: int(w) for k, w in re.findall(r"(fmd_\w+_kernel) is built for (\d+) waves per SIMD", text)}
    assert sorted(claimed) == ["fmd_collect_kernel", "fmd_locate_kernel"], claimed
    found = kernel_resources.kernel_resources(SOURCE)
    for name, waves in claimed.items():
        # by the mangled name: the kernels sit in an anonymous namespace, which the tool's demangled names drop
        match = [r for r in found if name in r["mangled"]]
        assert len(match) == 1, [r["mangled"] for r in found]
        r = match[0]
        print(f"{name}: {r['vgprs']} VGPRs, {r['agprs']} AGPRs, {r['sgprs']} SGPRs, scratch {r['scratch']}, "
              f"static LDS {r['lds_static']} B, {r['occupancy']} waves/SIMD; built for {waves}")
        assert r["scratch"] == 0, r
        assert r["lds_static"] == 0, r
        assert waves >= 1 and r["occupancy"] >= waves, r
