"""Instruction counts of the static sweeps of the band pair kernel.   python tools/band_region_counts.py UNIT.s [NB ...]

UNIT.s is the device assembly of hgp_pairs.hip (see tools/kernel_isa_diff.py for the compile line).  For k_pairs<NB, true>
(default NB = 8 and 6) the region of the two sweeps runs from the first 128-bit global load (the first M' fill of the operand
ring) to the first v_fmac_f64_dpp (the first pivot step of the factorisation).  Printed per kernel: MFMAs in the region and by
source-B register class in the whole kernel, the other VALU instructions of the region by opcode, LDS and global loads by
addressing form, and the long s_nop."""
import collections
import re
import sys


def body(lines, name):
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    out = []
    for l in lines[start + 1:end]:
        l = l.split(";", 1)[0].strip()
        if l and not l.startswith(".") and not l.endswith(":"):
            out.append(l)
    return out


def report(lines, nb, tag="9PairsArgs"):
    name = f"_ZN12_GLOBAL__N_17k_pairsILi{nb}ELb1EEEv{tag}"
    ins = body(lines, name)
    first = next(i for i, l in enumerate(ins) if l.startswith("global_load_dwordx4"))
    last = next(i for i, l in enumerate(ins) if l.startswith("v_fmac_f64_dpp"))
    reg = ins[first:last]
    ops = collections.Counter(l.split()[0] for l in reg)
    mfma = [l for l in ins if l.startswith("v_mfma")]
    srcb = collections.Counter("AGPR" if re.split(r",\s*", l.split(None, 1)[1])[2].startswith("a") else "VGPR" for l in mfma)
    valu = {k: v for k, v in ops.items() if k.startswith("v_") and not k.startswith("v_mfma")}
    print(f"k_pairs<{nb}, true>: {len(ins)} instructions, region {len(reg)}")
    print(f"  region: MFMA {sum(v for k, v in ops.items() if k.startswith('v_mfma'))}, other VALU {sum(valu.values())}")
    for k, v in sorted(valu.items(), key=lambda kv: -kv[1]):
        print(f"    {k:28s} {v}")
    gl = [l for l in reg if l.startswith("global_load")]
    sbase = re.compile(r", s\[\d+:\d+\]")
    print(f"  region: global loads {len(gl)}, scalar-base form {sum(1 for l in gl if sbase.search(l))}, "
          f"'off' form {sum(1 for l in gl if ', off' in l)}")
    ds = [l for l in reg if l.startswith("ds_read")]
    print(f"  region: ds_read {len(ds)} ({dict(collections.Counter(l.split()[0] for l in ds))}), with offset {sum(1 for l in ds if 'offset' in l)}")
    print(f"  region: s_nop {ops.get('s_nop', 0)}, of >= 9 wait states {sum(1 for l in reg if l.startswith('s_nop') and int(l.split()[1]) >= 8)}; "
          f"s_waitcnt {ops.get('s_waitcnt', 0)}; SALU {sum(v for k, v in ops.items() if k.startswith('s_') and k not in ('s_nop', 's_waitcnt'))}")
    print(f"  kernel: MFMA {len(mfma)}, srcB from {dict(srcb)}; s_nop >= 9 wait states "
          f"{sum(1 for l in ins if l.startswith('s_nop') and int(l.split()[1]) >= 8)}")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    text = open(sys.argv[1]).read().split("\n")
    for nb in ([int(x) for x in sys.argv[2:]] or [8, 6]):
        report(text, nb)
