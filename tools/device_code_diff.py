"""Per-kernel comparison of two builds' device assembly (profiles/r13_device_code_parent_vs_change.txt).

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off --cuda-device-only -S FILE.hip -o DIR/FILE.s     (both trees)
    python tools/device_code_diff.py PARENT_DIR CHANGE_DIR

A file's assembly is cut into its functions (from `.type NAME,@function` to the kernel descriptor or `.Lfunc_endN:`); local labels carry the
function's position in the file (.LBB12_3, BB12_3, .Lfunc_end12), so the position is taken out before two bodies are compared
(and with it the blanks between a label and its comment, whose number depends on the position's digits).
A build's functions are pooled over all its files by symbol name, so a kernel that moved to another source file is compared with
itself.  A symbol that two files of one build define is compared file against file, counted, and named where the files are not
the same in both builds.  A kernel that exists in both builds must not differ in a single
line; kernels of one build only are listed.  The kernel descriptors (.amdhsa_* blocks: registers, LDS, scratch) are compared the
same way, under NAME.kd.
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


def pooled(build):
    """name -> {file: body} over every *.s of a build"""
    out = {}
    for path in sorted(glob.glob(f"{build}/*.s")):
        for k, body in functions(path).items():
            out.setdefault(k, {})[os.path.basename(path)[:-2]] = body
    return out


def main(parent, change):
    a, b = pooled(parent), pooled(change)
    # an entry: a symbol that one file of each build defines, wherever it is (a kernel that moved is compared with itself), or one copy of
    # a symbol that several files define (template instantiations, which the linker folds), compared file against file
    pa, pb = {}, {}
    for k in sorted(set(a) | set(b)):
        fa, fb = a.get(k, {}), b.get(k, {})
        if len(fa) <= 1 and len(fb) <= 1:
            pa.update({(k, ""): (f, body) for f, body in fa.items()})
            pb.update({(k, ""): (f, body) for f, body in fb.items()})
        else:
            if sorted(fa) != sorted(fb):
                print(f"    TWICE, and not in the same files of both builds: {k} (parent: {', '.join(sorted(fa))}; change: {', '.join(sorted(fb))})")
            pa.update({(k, f): (f, body) for f, body in fa.items()})
            pb.update({(k, f): (f, body) for f, body in fb.items()})
    both = sorted(set(pa) & set(pb))
    bad = {}
    for e in both:
        x, y = pa[e][1], pb[e][1]
        if x != y:
            bad[e] = sum(1 for u, v in zip(x, y) if u != v) + abs(len(x) - len(y))
    for f in sorted({pb[e][0] for e in pb}):
        mine = [e for e in both if pb[e][0] == f]
        kern = [e for e in mine if e[0].endswith(".kd")]
        moved = sorted({pa[e][0] for e in mine} - {f})
        print(f"{f}: {len(kern)} kernels in both builds ({len(mine) - len(kern)} function bodies, {len(kern)} descriptors compared), "
              f"{sum(bad.get(e, 0) for e in mine)} differing lines in them" + (f"; the parent has some in {', '.join(moved)}" if moved else ""))
        for e in mine:
            if e in bad:
                print(f"    DIFFERS ({bad[e]} lines): {e[0]}")
    for e in sorted(set(pb) - set(pa)):
        print(f"    new in the change: {e[0]} ({pb[e][0]})")
    for e in sorted(set(pa) - set(pb)):
        print(f"    only in the parent: {e[0]} ({pa[e][0]})")
    shared = [sum(1 for fs in x.values() if len(fs) > 1) for x in (a, b)]
    print(f"all files: {len(both)} of {len(pa)} entries of the parent are in both builds, {sum(bad.values())} differing lines, "
          f"{len(set(pb) - set(pa))} new in the change, {len(set(pa) - set(pb))} only in the parent; "
          f"symbols that several files define: {shared[0]} in the parent, {shared[1]} in the change")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
