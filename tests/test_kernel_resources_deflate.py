"""Scratch, LDS and register budget of bgzf_deflate_kernel
(falcon-genome_amd/csrc/bgzf_deflate.hip) from the compiler's resource remarks
(tools/kernel_resources.py; no GPU): no scratch, and the members per CU that
the kernel's header comment claims fit the CU's 163,840 B of LDS and the
512 VGPRs per SIMD lane (one 64-lane wave per member, spread over 4 SIMDs).
"""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

SOURCE = "csrc/bgzf_deflate.hip"


@pytest.mark.skipif(kernel_resources.hipcc() is None or shutil.which("make") is None, reason="hipcc not installed")
def test_deflate_kernel_fits_its_declared_members_per_cu():
    text = open(os.path.join(ROOT, "falcon-genome_amd", SOURCE)).read()
    claimed = int(re.search(r"so (\d+) members per CU", text).group(1))
    rows = {r["name"]: r for r in kernel_resources.kernel_resources(SOURCE)}
    assert "bgzf_deflate_kernel" in rows, sorted(rows)
    r = rows["bgzf_deflate_kernel"]
    waves = -(-claimed // 4)  # per SIMD
    print(f"bgzf_deflate_kernel: {r['vgprs']} VGPRs, {r['agprs']} AGPRs, {r['sgprs']} SGPRs, scratch {r['scratch']}, "
          f"static LDS {r['lds_static']} B, {r['occupancy']} waves/SIMD; claimed {claimed} members per CU")
    assert r["scratch"] == 0, r
    assert r["agprs"] == 0, r
    assert claimed >= 1 and r["lds_static"] * claimed <= 163840, r
    assert r["lds_static"] <= 65536, r
    assert (r["vgprs"] + 7) // 8 * 8 * waves <= 512, r
    assert r["occupancy"] >= waves, r
