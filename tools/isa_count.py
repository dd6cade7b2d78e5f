#!/usr/bin/env python3
"""Development aid (no GPU): static instruction counts of one kernel, or of one loop of it, in a listing saved by
hipcc --save-temps (the *-gfx950.s file).

    python tools/isa_count.py LISTING.s MANGLED_PREFIX                 the whole kernel
    python tools/isa_count.py LISTING.s MANGLED_PREFIX --loop .LBB287_40   from that label to the last branch back to it
    python tools/isa_count.py LISTING.s MANGLED_PREFIX --lines 1200-1650    those lines of the file (1-based, inclusive)
    python tools/isa_count.py LISTING.s MANGLED_PREFIX --loops         every label a later branch returns to, with its size

Instructions are sorted by the prefix of their mnemonic: v_ vector, s_ scalar, ds_ LDS, global_ / flat_ / buffer_ / scratch_
memory.  The quarter-rate integer multiplies (v_mul_lo_u32, v_mul_hi_u32, v_mad_u64_u32) are counted on their own as well.
These are counts of the text, not of what runs: a loop's body counts once, both sides of a branch count.  One JSON line."""
import argparse, json, re, sys

CLASSES = (("vector", ("v_",)), ("scalar", ("s_",)), ("lds", ("ds_",)), ("memory", ("global_", "flat_", "buffer_", "scratch_")))
QUARTER_RATE = ("v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32")
_INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")
_LABEL = re.compile(r"^([.\w$]+):")
_BRANCH = re.compile(r"^\s+s_c?branch\w*\s+([.\w$]+)")


def kernel_lines(lines, prefix):
    """(first, last) 0-based line numbers of the body of the first function whose label starts with prefix"""
    start = None
    for i, ln in enumerate(lines):
        m = _LABEL.match(ln)
        if start is None:
            if m and m.group(1).startswith(prefix):
                start = i
        elif ln.startswith(".Lfunc_end"):
            return start, i
    if start is None:
        raise SystemExit("no function label starts with %r" % prefix)
    return start, len(lines) - 1


def loops(lines, first, last):
    """{label: (line of the label, line of the last branch back to it)} for the labels of the range a later branch names"""
    at = {}
    for i in range(first, last + 1):
        m = _LABEL.match(lines[i])
        if m:
            at[m.group(1)] = i
    out = {}
    for i in range(first, last + 1):
        m = _BRANCH.match(lines[i])
        if m and m.group(1) in at and at[m.group(1)] <= i:
            out[m.group(1)] = (at[m.group(1)], i)
    return out


def count(lines, first, last):
    c = {name: 0 for name, _ in CLASSES}
    c["other"] = 0
    q = {name: 0 for name in QUARTER_RATE}
    for i in range(first, last + 1):
        ln = lines[i]
        if ln.lstrip().startswith((";", ".", "//")) or _LABEL.match(ln):
            continue
        m = _INSN.match(ln)
        if not m:
            continue
        op = m.group(1)
        for name, prefixes in CLASSES:
            if op.startswith(prefixes):
                c[name] += 1
                break
        else:
            c["other"] += 1
        for name in QUARTER_RATE:
            if op.startswith(name):
                q[name] += 1
    c["quarter_rate"] = q
    c["total"] = sum(c[name] for name, _ in CLASSES) + c["other"]
    return c


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing"); ap.add_argument("prefix")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--loop", metavar="LABEL"); g.add_argument("--lines", metavar="A-B"); g.add_argument("--loops", action="store_true")
    a = ap.parse_args(argv)
    lines = open(a.listing, "r", errors="replace").read().split("\n")
    first, last = kernel_lines(lines, a.prefix)
    name = _LABEL.match(lines[first]).group(1)
    if a.loops:
        found = loops(lines, first, last)
        print(json.dumps({"kernel": name, "loops": {k: dict(lines=[v[0] + 1, v[1] + 1], **count(lines, v[0], v[1])) for k, v in found.items()}}))
        return 0
    if a.loop:
        found = loops(lines, first, last)
        if a.loop not in found:
            raise SystemExit("no branch of %s returns to %s" % (name, a.loop))
        first, last = found[a.loop]
    elif a.lines:
        lo, hi = (int(x) for x in a.lines.split("-"))
        first, last = lo - 1, hi - 1
    print(json.dumps(dict(kernel=name, lines=[first + 1, last + 1], **count(lines, first, last))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
