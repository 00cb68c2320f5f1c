#!/usr/bin/env python3
"""Compare two device-assembly listings (hipcc -S --cuda-device-only) kernel by kernel, for a change that must not
touch a hand-scheduled loop:

  resources   the .amdhsa_kernel descriptor block and the "; Kernel info" figures (VGPR / AGPR / SGPR counts, scratch,
              LDS, occupancy), code length left out;
  MFMA span   the sequence of instruction mnemonics from the kernel's first v_mfma to its last, register numbers,
              operands and labels ignored;
  MFMA blocks the same for each basic block that holds a v_mfma, one by one: in a kernel with two consumer loops the
              span also covers what the compiler laid out between them.

usage: isa_span_diff.py OLD.s NEW.s        one line per kernel symbol; exit status 1 when anything differs
"""
import re
import sys

INFO = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "LDSByteSize", "SGPRBlocks", "VGPRBlocks",
        "NumSGPRsForWavesPerEU", "NumVGPRsForWavesPerEU", "AccumOffset", "Occupancy", "WaveLimiterHint")


def kernels(path):
    """symbol -> (resource lines, mnemonics of the MFMA span)."""
    lines = open(path).read().splitlines()
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel")]
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.split(";")[0].strip() == name + ":")
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        ops, blocks = [], [[]]
        for ln in lines[start + 1:end]:
            if ln.startswith(".L") and ln.rstrip().split(";")[0].strip().endswith(":"):
                blocks.append([])                                  # a label opens a basic block ...
            elif ln.startswith("\t") and not ln.lstrip().startswith((".", ";")):
                ops.append(ln.split()[0])
                blocks[-1].append(ops[-1])
                if ops[-1].startswith(("s_cbranch", "s_branch")):
                    blocks.append([])                              # ... and so does the instruction behind a branch
        mf = [i for i, op in enumerate(ops) if op.startswith("v_mfma")]
        span = (ops[mf[0]:mf[-1] + 1] if mf else [], [b for b in blocks if any(o.startswith("v_mfma") for o in b)])
        d0 = next(i for i in range(start, len(lines)) if lines[i].strip() == ".amdhsa_kernel " + name)
        d1 = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        res = [ln.strip() for ln in lines[d0 + 1:d1]]
        k0 = next(i for i in range(d1, len(lines)) if lines[i].startswith("; Kernel info"))
        for ln in lines[k0:k0 + 24]:
            m = re.match(r"; (\w+)[:=]? ", ln)
            if m and m.group(1) in INFO:
                res.append(ln)
        out[name] = (res, span)
    return out


def main(old, new):
    a, b = kernels(old), kernels(new)
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{name}: only in {'OLD' if name in a else 'NEW'}")
            bad += 1
            continue
        (ra, sa), (rb, sb) = a[name], b[name]
        r = "equal" if ra == rb else "differ"
        s = "equal" if sa[0] == sb[0] else "differ"
        k = "equal" if sa[1] == sb[1] else "differ"
        print(f"{name}: resources {r} / MFMA span {s} ({len(sa[0])} instructions, "
              f"{sum(o.startswith('v_mfma') for o in sa[0])} MFMAs) / MFMA blocks {k} ({len(sa[1])})")
        if ra != rb:
            for x, y in zip(ra, rb):
                if x != y:
                    print(f"    {x}  ->  {y}")
        bad += (ra != rb) + (sa[0] != sb[0])
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
