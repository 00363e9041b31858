#!/usr/bin/env python3
"""Register, scratch and occupancy figures of the PairHMM kernels (no GPU).

Compiles falcon-genome_amd/csrc/phmm_kernels.hip with the Makefile's flags
plus the compiler's kernel-resource-usage remarks into a temporary directory
and prints one line per kernel: VGPRs, AGPRs, SGPRs, scratch bytes per lane,
static LDS and occupancy (waves per SIMD).  --json prints the same as a JSON
list; --match RE keeps the kernels whose demangled name matches.

  tools/kernel_resources.py --match 'phmm[45]_kernel' > profiles/r7/resources_new.txt
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "falcon-genome_amd")

FIELDS = {
    "VGPRs": "vgprs",
    "AGPRs": "agprs",
    "TotalSGPRs": "sgprs",
    "ScratchSize [bytes/lane]": "scratch",
    "Occupancy [waves/SIMD]": "occupancy",
    "LDS Size [bytes/block]": "lds_static",
}


def hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or (
        "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def make_flags():
    """HIPFLAGS as the Makefile sets them (its ?= default, ARCH expanded)."""
    text = open(os.path.join(PKG, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    flags = re.search(r"^HIPFLAGS \?= (.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return out.splitlines()
    except (OSError, subprocess.CalledProcessError):
        return list(names)


def kernel_resources(source="csrc/phmm_kernels.hip"):
    """[{name, mangled, vgprs, agprs, sgprs, scratch, occupancy, lds_static}] in source order."""
    cc = hipcc()
    if cc is None:
        raise FileNotFoundError("hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [cc, *make_flags(), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"),
               "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o",
               os.path.join(tmp, "k.o"), os.path.join(PKG, source)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-4000:])
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            cur = {"mangled": text.split(":", 1)[1].strip()}
            rows.append(cur)
            continue
        if cur is None or ":" not in text:
            continue
        key, val = (s.strip() for s in text.rsplit(":", 1))
        if key in FIELDS:
            cur[FIELDS[key]] = int(val)
    for row, name in zip(rows, demangle([r_["mangled"] for r_ in rows])):
        row["name"] = re.sub(r"\(.*", "", name).replace("void ", "").replace("fcs::", "")
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--match", default="", help="regular expression on the demangled kernel name")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    rows = [r for r in kernel_resources() if re.search(a.match, r["name"])]
    if a.json:
        print(json.dumps(rows, indent=1))
        return 0
    print(f"{'kernel':44s} {'VGPR':>5s} {'AGPR':>5s} {'SGPR':>5s} {'scratch':>8s} {'LDS(static)':>11s} {'waves/SIMD':>10s}")
    for r in rows:
        print(f"{r['name']:44s} {r.get('vgprs', -1):5d} {r.get('agprs', -1):5d} {r.get('sgprs', -1):5d} "
              f"{r.get('scratch', -1):8d} {r.get('lds_static', -1):11d} {r.get('occupancy', -1):10d}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
