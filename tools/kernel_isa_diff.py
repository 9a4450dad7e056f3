"""Is the device code of two builds the same, kernel by kernel?   python tools/kernel_isa_diff.py DIR_A DIR_B [OLD=NEW ...]

Each directory holds the device assembly of one build, one .s per translation unit:
    hipcc <the Makefile's FLAGS> --cuda-device-only -S -o DIR/<unit>.s hdpgpc_amd/csrc/<unit>.hip
Kernels are paired by mangled name, whichever unit they sit in, so a kernel that moved between units pairs with itself.
Reported per kernel: present / missing, whether the .amdhsa_kernel block (registers, LDS, scratch) is identical, and whether the
body is identical once comments are gone and the per-unit counters are taken out of the local labels (.LBB<n>_<m>,
.Lfunc_end<n>, .Lpost_getpc<n>).  OLD=NEW rewrites DIR_A's text first, for a kernel whose mangled name changed because an argument type moved
(NS_9PotrfArgsE=9PotrfArgs: out of the anonymous namespace).  A plain text comparison: it knows no instruction.  Exit status 0
only when nothing differs."""
import difflib
import glob
import os
import re
import sys


def normalise(lines):
    out = []
    for l in lines:
        l = l.split(";", 1)[0].rstrip()
        l = re.sub(r"\.LBB\d+_", ".LBB_", l)
        l = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", l)
        l = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", l)
        if l.strip():
            out.append(l)
    return out


def kernels(directory, renames=()):
    """{mangled name: (unit, descriptor lines, normalised body lines)} of every kernel in directory/*.s"""
    found = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        unit = os.path.basename(path)[:-2]
        text = open(path).read()
        for old, new in renames:
            text = text.replace(old, new)
        lines = text.split("\n")
        labels = {l.split(":", 1)[0]: i for i, l in enumerate(lines) if re.match(r"^[A-Za-z_$][\w$.]*:", l)}
        for i, l in enumerate(lines):
            m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", l)
            if not m:
                continue
            name = m.group(1)
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
            b0 = labels[name] + 1
            b1 = next(j for j in range(b0, len(lines)) if re.match(r"^\s*\.section\b", lines[j]) or lines[j].startswith(".Lfunc_end"))
            assert name not in found, f"{name} defined twice ({found[name][0]}, {unit})"
            found[name] = (unit, normalise(lines[i:end + 1]), normalise(lines[b0:b1]))
    return found


def main(dir_a, dir_b, renames=()):
    a, b = kernels(dir_a, renames), kernels(dir_b)
    same, diffs = 0, []
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            diffs.append(f"{name}: only in {dir_a if name in a else dir_b} ({(a.get(name) or b.get(name))[0]})")
            continue
        (ua, da, ba), (ub, db, bb) = a[name], b[name]
        if da == db and ba == bb:
            same += 1
            continue
        what = [w for w, x, y in (("descriptor", da, db), ("body", ba, bb)) if x != y]
        diffs.append(f"{name} ({ua} -> {ub}): {' and '.join(what)} differ; body {len(ba)} -> {len(bb)} lines")
        for x, y in ((da, db), (ba, bb)):
            diffs += ["    " + d for d in list(difflib.unified_diff(x, y, lineterm="", n=0))[2:12]]
    print(f"kernels: {len(a)} in {dir_a}, {len(b)} in {dir_b}; identical (descriptor and normalised body): {same}")
    print(f"differences: {len([d for d in diffs if not d.startswith('    ')])}")
    for d in diffs:
        print(d)
    return 1 if diffs else 0


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2], [r.split("=", 1) for r in sys.argv[3:]]))
