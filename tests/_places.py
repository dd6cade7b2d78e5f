"""Real places beyond 2 GiB and 4 GiB in a caller's buffer (test infrastructure for tests/test_gpu_wide_words.py, part B): where the items
of a batch go inside one big buffer, and the checks around them.

geometry(lens, layout) gives every item an offset.  Two layouts, because an item that straddles a crossing excludes one that ends at it:
  "edges":    an item whose last byte is T - 1 and one whose first byte is T, for T = 2^31 and 2^32;
  "straddle": an item with T in its middle, for both T;
both with two low controls (64 MiB + 1, 100 MiB + 3), an item that ends at 2^32 + 48 MiB, and the rest at odd offsets in groups below and
above each crossing and at 2^32 + 30 MiB.  The items are dealt onto the slots from another start in each layout.  The host-buffer calls
stage the span from their lowest to their highest item, so their layout (host=True) keeps to 2^32: the same edge or straddling items,
the rest within 3 MiB below and 21 MiB above it.

A truncated offset stays inside the buffer: off mod 2^32 and off mod 2^31 are places of it too.  So besides the 4 KiB in front of and
behind every item, the windows at those two aliases must keep their fill (guard_windows); bytes that belong to another item of the call
are left to that item's own comparison."""
import numpy as np
from _hip import CANARY, PAD

T31, T32 = 1 << 31, 1 << 32
MIB = 1 << 20
FAR_END = T32 + 48 * MIB
LOWS = (64 * MIB + 1, 100 * MIB + 3)
LAYOUTS = ("edges", "straddle")


def _fills(stride, crossings, far, each):
    out = []
    for t in crossings:
        out += [t - (k + 2) * stride + 1 + 2 * k for k in range(each)] + [t + (k + 1) * stride + 3 + 2 * k for k in range(each)]
    return out + [far + k * stride + 9 for k in range(4)]


def geometry(lens, layout, host=False):
    """offsets (Python ints) for items of these lengths.  host: the layout of the host-buffer calls, every item within 64 MiB around 2^32
    (their staging uploads the span from the lowest to the highest item)"""
    n = len(lens)
    stride = -(-(max(lens) + 2 * PAD + 4096) // (256 << 10)) * (256 << 10)
    assert stride <= 5 * MIB // 4
    crossings = (T32,) if host else (T31, T32)
    slots = []                                             # (kind, argument)
    for t in crossings:
        slots += [("ends", t), ("begins", t)] if layout == "edges" else [("straddles", t)]
    if not host:
        slots += [("begins", LOWS[0]), ("begins", LOWS[1]), ("ends", FAR_END)]
    slots += [("begins", o) for o in _fills(stride, crossings, T32 + (20 if host else 30) * MIB, 10 if host else 4)]
    assert n <= len(slots), (n, len(slots))
    shift = 0 if layout == "edges" else 5
    offs = [None] * n
    for s in range(n):
        i = (s + shift) % n
        kind, t = slots[s]
        if t in (T31, T32):
            assert lens[i] >= 2, ("an item at a crossing must have bytes", i, lens[i])
        offs[i] = t - lens[i] if kind == "ends" else t if kind == "begins" else t - lens[i] // 2
    regions = sorted((o, o + ln) for o, ln in zip(offs, lens))
    assert all(a[1] <= b[0] for a, b in zip(regions, regions[1:])), "items overlap"
    assert regions[0][0] >= PAD
    if host:
        assert regions[-1][1] - regions[0][0] < 64 * MIB
    return offs


def holds_what_it_is_for(offs, lens, layout, host=False):
    """the places the issue lists are there"""
    ends = {o + ln for o, ln in zip(offs, lens) if ln}
    starts = {o for o, ln in zip(offs, lens) if ln}
    for t in ((T32,) if host else (T31, T32)):
        if layout == "edges":
            assert t in ends and t in starts, (layout, hex(t))
        else:
            assert any(o < t < o + ln for o, ln in zip(offs, lens)), (layout, hex(t))
    if not host:
        assert FAR_END in ends and sum(1 for o in starts if o < T31 - 512 * MIB) >= 2


def pieces(o, n):
    cuts = [o] + [t for t in (T31, T32) if o < t < o + n] + [o + n]
    return [(a, b - a) for a, b in zip(cuts, cuts[1:])]


def guard_windows(offs, lens):
    """[(offset, length, what)] that must keep their fill: 4 KiB in front of and behind every item, and for every part of an item at or
    above 2^31 (2^32) the window at its offset mod 2^31 (mod 2^32)"""
    out = []
    for i, (o, ln) in enumerate(zip(offs, lens)):
        out += [(o - PAD, PAD, (i, "in front")), (o + ln, PAD, (i, "behind"))]
        for a, m in pieces(o, ln):
            for mod in (T31, T32):
                if a >= mod and m:
                    out.append((a % mod, m, (i, "alias mod 2^%d" % (31 if mod == T31 else 32))))
    return out


def assert_guards(read, offs, lens, fill=CANARY, what=""):
    """read(offset, length) -> bytes.  Every guard window holds `fill`, but for bytes inside another item's place"""
    regions = [(o, o + ln) for o, ln in zip(offs, lens) if ln]
    for o, ln, name in guard_windows(offs, lens):
        got = np.frombuffer(read(o, ln), dtype=np.uint8)
        keep = np.ones(ln, dtype=bool)
        for a, b in regions:
            lo, hi = max(a, o), min(b, o + ln)
            if lo < hi:
                keep[lo - o:hi - o] = False
        bad = np.flatnonzero(keep & (got != fill))
        assert bad.size == 0, (what, name, "changed at", [hex(o + int(k)) for k in bad[:4]])
