"""The fp32 arithmetic of the single-stream column kernels' pass loop, counted
in the gfx950 assembly (no GPU; about a minute of compile).

The pass loop of phmm5_kernel<C> and phmm6_kernel<C> is eight steps of C
cells.  A cell is six fp32 operations: E = fma(E, yy, M),
M' = X~ * prior, X~ = fma(E, b, fma(I, a, M)), I' = fma(M, mx, I * xx), so the
loop holds 48 C of v_mul_f32 / v_fma_f32 / v_fmac_f32 / v_add_f32 and no other
fp32 arithmetic.  Measured on the parent commit with this same count: 56 C for
every class of both kernels (24 C v_mul_f32, 8 C v_fma_f32, 24 C v_fmac_f32),
i.e. the seven-op cell with D = fma(M, my, D * yy).
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402
import phmm_step_hist  # noqa: E402

FP32 = re.compile(r"v_(mul|fma|fmac|add)_f32")
CLASSES = (11, 12, 13, 14, 15, 16, 17, 19)


@pytest.mark.skipif(kernel_resources.hipcc() is None, reason="hipcc not installed")
def test_pass_loop_has_six_fp32_ops_per_cell(tmp_path):
    pkg = os.path.join(ROOT, "falcon-genome_amd")
    asm = tmp_path / "phmm_kernels.s"
    cmd = [kernel_resources.hipcc(), *kernel_resources.make_flags(), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(pkg, "csrc"), "--cuda-device-only", "-S", "-o", str(asm),
           os.path.join(pkg, "csrc", "phmm_kernels.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels = phmm_step_hist.kernels(str(asm))
    assert sorted(kernels) == sorted(f"phmm{k}_kernel<{c}>" for k in (5, 6) for c in CLASSES), sorted(kernels)
    for name, (lines, _, _) in kernels.items():
        c = int(name[name.index("<") + 1:-1])
        ops = phmm_step_hist.ops(phmm_step_hist.pass_loop(lines))
        fp = {op: n for op, n in ops.items() if FP32.match(op)}
        print(f"{name}: {sum(fp.values())} fp32 ops in 8 steps of {c} cells {fp}")
        assert not any(op.startswith("v_pk_") and op.endswith("_f32") for op in ops), (name, ops)
        assert sum(fp.values()) == 48 * c, (name, fp)
