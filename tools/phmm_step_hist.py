#!/usr/bin/env python3
"""Compare the pass loop of phmm5/phmm6_kernel<C> between two gfx950 assembly
files (phmm_kernels.hip compiled with the Makefile's flags plus
--cuda-device-only -S): tools/phmm_step_hist.py OLD.s NEW.s

The pass loop is the 8-step unrolled body: the blocks of the innermost loop
around the kernel's eight exec-masked ds_write_b32.
Prints per kernel the VGPR/SGPR counts (next_free_*, before the extra SGPRs
the resource remarks add), the instruction totals of the kernel
and of the loop, and every opcode whose count in the loop differs; exits 1 if
any loop histogram differs.
"""
import collections
import re
import sys

INSTR = re.compile(r"^\s+([vsd][a-z0-9_]+|global_\w+|buffer_\w+|flat_\w+|scratch_\w+)\b")


def kernels(path):
    """{C-tagged name: (lines, vgprs, sgprs)} of every phmm5/phmm6 kernel."""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_ZN3fcs12phmm([56])_kernelILi(\d+)EE\w+):[^\n]*\n(.*?)\n\s+s_endpgm", text, re.M | re.S):
        meta = text[text.index(".amdhsa_kernel " + m.group(1)):]
        vg = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
        sg = int(re.search(r"\.amdhsa_next_free_sgpr (\d+)", meta).group(1))
        out[f"phmm{m.group(2)}_kernel<{m.group(3)}>"] = (m.group(4).splitlines(), vg, sg)
    return out


def ops(lines):
    return collections.Counter(m.group(1) for m in map(INSTR.match, lines) if m)


def pass_loop(lines):
    w = [i for i, l in enumerate(lines) if "ds_write_b32" in l and "s_mov_b64 exec" in lines[i - 1]]
    assert len(w) == 8, len(w)
    # the loop's blocks are the labels the compiler marks with the depth of the writes' block
    labels = [i for i, l in enumerate(lines) if l.startswith(".LBB")]
    depth = re.search(r"Depth=\d", lines[max(i for i in labels if i < w[0])]).group(0)
    outer = [i for i in labels if depth not in lines[i]]
    start = min(i for i in labels if i > max(o for o in outer if o < w[0]))
    end = min(o for o in outer if o > w[-1])
    return lines[start:end]


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for k in sorted(new, key=lambda s: (s[4], int(s[13:-1]))):
        (lo, vo, so), (ln, vn, sn) = old[k], new[k]
        ho, hn = ops(pass_loop(lo)), ops(pass_loop(ln))
        diff = {op: (ho[op], hn[op]) for op in sorted(set(ho) | set(hn)) if ho[op] != hn[op]}
        bad += bool(diff)
        print(f"{k:18s} VGPR {vo:3d} -> {vn:3d}  SGPR {so:3d} -> {sn:3d}  instr {sum(ops(lo).values()):5d} -> "
              f"{sum(ops(ln).values()):5d}  loop {sum(ho.values()):4d} -> {sum(hn.values()):4d}  "
              f"loop diff {diff or 'none'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
