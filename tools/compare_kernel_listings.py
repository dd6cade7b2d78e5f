#!/usr/bin/env python3
"""Compare the kernels of two device listings, kernel by kernel: which exist in one only, and which differ in their instructions or in
their kernel descriptor.  The way to show that a change which adds kernels to the library's single translation unit left every existing
kernel as it was.  Make the listings with the library's flags and one fingerprint for both trees:
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC '-DZSMI_SOURCE_FP="x"' --cuda-device-only -S -o OLD.s OLD_TREE/zstandard_amd/csrc/zsmi_api.hip
  hipcc ... -o NEW.s NEW_TREE/zstandard_amd/csrc/zsmi_api.hip
  python tools/compare_kernel_listings.py OLD.s NEW.s
Comments, debug directives and the numbers of local labels (which count functions from the top of the file) are left out of the
comparison; everything else - every instruction, operand, register and descriptor field - has to be the same.  Exit status 1 when a
kernel that both listings hold differs."""
import re, sys


def functions(path):
    """name -> the lines from the function's label to its end (its kernel descriptor included), normalised"""
    out, name, buf = {}, None, []
    for line in open(path):
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and not m.group(1).startswith(".L"):
            if name:
                out[name] = buf
            name, buf = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith("\t.end_amdhsa_kernel"):
            buf.append(line); out[name] = buf; name = None
            continue
        if line.lstrip().startswith((";", ".loc", ".file", ".cfi", ".Ltmp", ".Lfunc")):
            continue
        line = re.sub(r"\s*;.*$", "", line)
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        line = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", line)
        line = re.sub(r"__unnamed_\d+", "__unnamed", line)
        line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", line)                 # (the compile unit's id, behind the file's last function)
        buf.append(line)
    if name:
        out[name] = buf
    return {k: v for k, v in out.items() if k.startswith("_Z")}


def main():
    old, new = functions(sys.argv[1]), functions(sys.argv[2])
    differing = [k for k in sorted(set(old) & set(new)) if old[k] != new[k]]
    print("functions: %d and %d; in both: %d; differing: %d" % (len(old), len(new), len(set(old) & set(new)), len(differing)))
    for k in sorted(set(new) - set(old)):
        print("  only in the second:", k)
    for k in sorted(set(old) - set(new)):
        print("  only in the first: ", k)
    for k in differing:
        print("  differs:", k)
        shown = 0
        for a, b in zip(old[k], new[k]):
            if a != b and shown < 5:
                print("    -", a.rstrip()); print("    +", b.rstrip()); shown += 1
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
