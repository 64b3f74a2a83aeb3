#!/usr/bin/env python3
"""Compare two builds of one kernel file kernel by kernel in their device assembly.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -Ipinn_fem_amd/csrc -Iinclude FILE.hip -o FILE.s
    asm_compare.py parent/FILE.s new/FILE.s

Per kernel: "identical" when the instruction sequences (comments and directives dropped, branch labels numbered in order of
appearance, symbol names replaced) and .vgpr_count / .sgpr_count are equal; otherwise the line and register counts and
whether the float64 instructions still follow each other in the same kind and order (operands aside)."""
import re
import sys


def short(name):
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", name)
    if not m:
        return name
    k, rest = int(m.group(1)), name[m.end():]
    t = re.match(r"ILi(\d+)E", rest[k:])
    return rest[:k] + (f"<{t.group(1)}>" if t else "")


def kernels(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\s*\.section\s+\.rodata", txt, re.S | re.M):
        labels, ins = {}, []
        for line in m.group(2).splitlines():
            line = line.split(";")[0].strip()
            if re.match(r"\.LBB\d+_\d+:", line):
                labels[line[:-1]] = f"L{len(labels)}"
                ins.append("LABEL")
            elif line and not line.startswith("."):
                ins.append(line)
        ins = [re.sub(r"_Z\w+", "SYM", re.sub(r"\.LBB\d+_\d+", lambda t: labels.get(t.group(0), t.group(0)), l)) for l in ins]
        out[short(m.group(1))] = {"ins": ins}
    for blk in re.split(r"\n  - \.agpr_count", txt)[1:]:
        k = out[short(re.search(r"\.name:\s+(_Z\w+)", blk).group(1))]
        k["vgpr"], k["sgpr"] = (int(re.search(rf"\.{r}_count:\s+(\d+)", blk).group(1)) for r in ("vgpr", "sgpr"))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    differ = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"{k}: only in {'the first' if k in a else 'the second'}")
            differ += 1
            continue
        x, y = a[k], b[k]
        regs = f"vgpr {x['vgpr']}/{y['vgpr']} sgpr {x['sgpr']}/{y['sgpr']}"
        if x == y:
            print(f"{k}: identical ({len(x['ins'])} lines; {regs})")
            continue
        differ += 1
        fx, fy = ([l.split()[0] for l in z["ins"] if "f64" in l.split()[0]] for z in (x, y))
        print(f"{k}: differs ({len(x['ins'])} vs {len(y['ins'])} lines; {regs}); float64 instructions in kind and order: "
              f"{'same' if fx == fy else 'DIFFERENT'} ({len(fx)} vs {len(fy)})")
    print(f"kernels that differ: {differ} of {len(set(a) | set(b))}")


if __name__ == "__main__":
    main()
