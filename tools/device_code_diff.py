"""Per-kernel comparison of two builds' device assembly (profiles/r13_device_code_parent_vs_change.txt).

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off --cuda-device-only -S FILE.hip -o DIR/FILE.s     (both trees)
    python tools/device_code_diff.py PARENT_DIR CHANGE_DIR

A file's assembly is cut into its functions (from `.type NAME,@function` to the kernel descriptor or `.Lfunc_endN:`); local labels carry the
function's position in the file (.LBB12_3, BB12_3, .Lfunc_end12), so the position is taken out before two bodies are compared
(and with it the blanks between a label and its comment, whose number depends on the position's digits).
A kernel that exists in both builds must not differ in a single line; kernels of one build only are listed.  The kernel
descriptors (.amdhsa_* blocks: registers, LDS, scratch) are compared the same way, under NAME.kd.
"""
import glob
import os
import re
import sys


def functions(path):
    out, name, body, kd = {}, None, [], None
    for line in open(path):
        line = re.sub(r"__hip_cuid_[0-9a-f]*", "__hip_cuid", line.rstrip("\n"))
        if re.match(r"\s*\.file", line):
            continue
        m = re.match(r"\s*\.type\s+([A-Za-z_0-9$.]+),@function", line)
        if m:
            name, body = m.group(1), []
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:  # the code is over (what follows up to .Lfunc_end is the descriptor)
            if name is not None:
                out[name] = body
                name = None
            kd, body = m.group(1) + ".kd", []
            continue
        line = re.sub(r"(\.?L?BB|\.Lfunc_(?:begin|end)|\.Ltmp)\d+", r"\1#", line)
        # the assembler pads a label up to the column of its comment: a position of one digit more or less moves the blanks
        line = re.sub(r"^(\.LBB#_\d+:)\s+;", r"\1 ;", line)
        if kd is not None:
            if re.match(r"\s*\.end_amdhsa_kernel", line):
                out[kd] = body
                kd = None
            else:
                body.append(line)
        elif name is not None:
            if re.match(r"\s*\.Lfunc_end#:", line):
                out[name] = body
                name = None
            else:
                body.append(line)
    return out


def main(parent, change):
    names = sorted({os.path.basename(p)[:-2] for d in (parent, change) for p in glob.glob(f"{d}/*.s")})
    for f in names:
        a = functions(f"{parent}/{f}.s") if os.path.exists(f"{parent}/{f}.s") else {}
        b = functions(f"{change}/{f}.s") if os.path.exists(f"{change}/{f}.s") else {}
        both = sorted(set(a) & set(b))
        bad = {}
        for k in both:
            if a[k] != b[k]:
                n = sum(1 for x, y in zip(a[k], b[k]) if x != y) + abs(len(a[k]) - len(b[k]))
                bad[k] = n
        kern = [k for k in both if k.endswith(".kd")]
        print(f"{f}: {len(kern)} kernels in both builds ({len(both) - len(kern)} function bodies, {len(kern)} descriptors compared), "
              f"{sum(bad.values())} differing lines in them")
        for k, n in bad.items():
            print(f"    DIFFERS ({n} lines): {k}")
        for k in sorted(set(b) - set(a)):
            print(f"    new in the change: {k}")
        for k in sorted(set(a) - set(b)):
            print(f"    only in the parent: {k}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
