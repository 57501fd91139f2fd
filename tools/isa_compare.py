"""Compare the device assembly of two builds of one .hip file, kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-fast-math --cuda-device-only -S old/x.hip -o old.s     (and new.s)
    python tools/isa_compare.py old.s new.s [--rename 'REGEX=REPLACEMENT' ...]

A kernel's text runs from its label through `.end_amdhsa_kernel` to the end of the `; Kernel info:` block behind it: every
instruction, the kernel descriptor's fields and the compiler's resource comments (registers, LDS, scratch, occupancy).  Before the comparison the kernel's own mangled name becomes
KERNEL and the function index leaves the local labels (`.LBB7_12` -> `.LBB_12`, also in the loop comments): the position
of a kernel in its file is not part of its code.  `--rename` is applied to the OLD file's kernel names to find their partners in the new one (a
template parameter that went away); kernels without a partner are listed as such.  Exit status 1 if any pair differs."""
import argparse
import re
import sys


def kernels(path):
    lines = open(path).read().split("\n")
    out = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", ln)
        if not m:
            continue
        name = m.group(1)
        begin = next(j for j in range(i) if lines[j].startswith(name + ":"))
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        info = next((j for j in range(end, min(end + 40, len(lines))) if lines[j].startswith("; Kernel info:")), None)
        if info is not None:
            while end + 1 < len(lines) and (end < info or lines[end + 1].startswith(";")):
                end += 1
        text = [re.sub(r"\b(L?BB|Lfunc_end|Lfunc_begin)\d+", r"\1", t.replace(name, "KERNEL")) for t in lines[begin:end + 1]]
        text = [re.sub(r"\s+;", " ;", t) for t in text]          # (a comment's column moves with the label's length)
        out[name] = text
    return out


def resources(text):
    get = lambda key: next((t.split(key, 1)[1].split()[0] for t in text if t.startswith(key)), "?")
    return (f"vgpr {get('; NumVgprs: ')} agpr {get('; NumAgprs: ')} sgpr {get('; TotalNumSgprs: ')} scratch {get('; ScratchSize: ')} "
            f"lds {get('; LDSByteSize: ')} occupancy {get('; Occupancy: ')}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[])
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    bad = 0
    for name, text in old.items():
        partner = name
        for r in a.rename:
            pat, rep = r.split("=", 1)
            partner = re.sub(pat, rep, partner)
        if partner not in new:
            print(f"ONLY IN OLD   {name}  ({len(text)} lines)")
            continue
        same = text == new[partner]
        bad += not same
        insts = sum(1 for t in text if t.startswith("\t") and not t.startswith("\t.") and not t.startswith("\t;"))
        print(f"{'IDENTICAL    ' if same else 'DIFFERENT    '} {partner}  ({len(text)} lines, {insts} instructions; {resources(text)})"
              + ("" if partner == name else f"  was {name}"))
    for name in new:
        if not any(name == n or any(re.sub(*r.split("=", 1), n) == name for r in a.rename) for n in old):
            print(f"ONLY IN NEW   {name}")
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
