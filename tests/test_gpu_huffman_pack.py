"""Huffman symbol packing (huffEncodeStream in zstandard_amd/csrc/entropy_kernels.hip: eight codes a lane looked up as one batch and
merged as a tree) at the borders of its tiles: blocks whose literal count is 63, 64, 255 .. 257 (one stream, then four), 511 .. 513,
1023 .. 1025 and 2049 = 4 x 512 + 1 (a stream of 512 symbols = one full tile, and the first with a second tile of one symbol).  Every
frame is compared byte for byte with oracle E's and decoded back (oracle D, the library, libzstd), and what a case exists for is asserted
on oracle E's own frame: the literal count, the streams, the coded symbols, the longest code and how many symbols have it.

GATHERED (a block with sequences: the literals are collected first).  The chunk is a text over the values 0 .. 199, zeros up to 64 KiB, and
in its second block the text again with runs of 3 bytes >= 200 punched into it every 12 (tests/_encoder_edges.py's `punched`
construction): every run is a literal run in front of a repeat-offset match, so the block's literals are exactly the punched bytes, in
order, whatever their histogram.  Two histograms:
  two symbols - codes of 1 bit: the merge's short extreme (a pair is 2 bits, a lane 8, the high word never used);
  a comb - eight symbols once each under a chain of counts 8, 9, 17, 26, 43, 69, 112, 181 (each one more than the sum two below it, so
  the Huffman tree is a comb and the eight are its deepest leaves, 3 + the chain's length deep) with the rest on the last count.  The
  chain takes 473 literals for depth 11 = ZS_HUF_MAXBITS, so from 511 literals on the eight have 11-bit codes; 255 .. 257 hold six
  links (180): 9 bits; 64 holds three (42): 6 bits.  The eight stand in a row, once where one lane takes all eight (counted from the
  first stream's end in eights, as the kernel deals them: 88 bits in a lane from 511 on, 72 at 255 .. 257: the high word either way)
  and once three symbols off (two lanes share them); both are asserted from the text.
IN PLACE (a block without a match: the literals are read where they lie).  Here no four bytes may repeat, which a comb's skew does not
allow, so the histogram is flat above a short comb, and a symbol that occurs once among N gets about log2 N bits: 11 only at 2049,
floor(log2 N) or one more below, asserted as such.  The same eight-in-a-row placement.

63 literals: the encoder tries Huffman from 64 literals on, so these blocks carry raw literals (or are stored raw); the cases stay for
the comparison."""
import functools
import numpy as np
import pytest
import _batch as B
import _framewriter as W

pytestmark = pytest.mark.gpu

COUNTS = (63, 64, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049)
RARE = 8
CHAIN = (8, 9, 17, 26, 43, 69, 112, 181)
FIRST_LITERAL = 200                                  # gathered: the text stays below it, the literals at or above


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    return BatchCodec(0)


def first_stream(n):
    return n if n < 256 else (n + 3) // 4


def run_start(n, off):
    """where the RARE rarest start: they end 16 + off symbols in front of the first stream's end"""
    return first_stream(n) - 16 - off - RARE


def lanes_of(text, rare):
    """the lanes of the first stream's last tile that hold a symbol of `rare`: lane l takes the symbols 8 l .. 8 l + 7 counted from the stream's end"""
    seg = first_stream(len(text))
    return {(seg - 1 - i) // 8 for i in range(seg) if text[i] in rare}


# ------------------------------------------------------------------ in place
def flat_histogram(n):
    """counts by symbol: RARE ones, a comb while it takes at most half of n, the rest over symbols that each count more than the comb's last"""
    c, acc = [1] * RARE, RARE
    while 2 * acc + 1 <= n // 2:
        c.append(acc + 1); acc += acc + 1
    rest = n - acc
    flat = max(1, min(40, rest // (c[-1] + 1)))
    return c + [rest // flat + (i < rest % flat) for i in range(flat)]


def arrange(counts, seed, run_at):
    """the symbols in an order without a repeated four-byte piece, the RARE rarest in a row at run_at; None if this seed gets stuck"""
    rng = np.random.default_rng(seed)
    n, left, out, seen = sum(counts), list(counts), [], set()
    while len(out) < n:
        if len(out) == run_at:
            take = list(range(RARE))
        else:
            order = np.argsort(-(np.array(left) * rng.random(len(left))))
            take = next(([int(s)] for s in order if s >= RARE and left[s] and tuple(out[-3:] + [int(s)]) not in seen), None)
            if take is None:
                return None
        for s in take:
            out.append(s); left[s] -= 1
            seen.add(tuple(out[-4:]))
    return (np.array(out, dtype=np.uint8) * 9 + 5).tobytes()


def matchless_text(n, off):
    text = next(filter(None, (arrange(flat_histogram(n), seed, run_start(n, off)) for seed in range(64))), None)
    assert text is not None and len(text) == n, n
    return text


# ------------------------------------------------------------------ gathered
def comb_histogram(n):
    """(counts by symbol, depth of the RARE rarest): the chain's links that fit, the rest on the last"""
    c, total = [1] * RARE, RARE
    for x in CHAIN:
        if total + x > n:
            break
        c.append(x); total += x
    depth = 3 + len(c) - RARE
    c[-1] += n - total
    return c, depth


def comb_text(n, off, seed):
    counts, depth = comb_histogram(n)
    rest = np.repeat(np.arange(RARE, len(counts)), counts[RARE:])
    np.random.default_rng(seed).shuffle(rest)
    at = run_start(n, off)
    return (np.array(list(rest[:at]) + list(range(RARE)) + list(rest[at:]), dtype=np.uint8) + FIRST_LITERAL).tobytes(), depth


def two_symbol_text(n, seed):
    return (np.random.default_rng(seed).integers(0, 2, n, dtype=np.uint8) + 254).tobytes()


def punched_chunk(lits, seed, seg=9, run=3):
    """a text, zeros up to 64 KiB, the text again with `lits` punched into it, `run` bytes behind every `seg` of text: the second
    block's literals are `lits`"""
    n = len(lits)
    punches = (n + run - 1) // run
    text = np.random.default_rng(seed).integers(0, FIRST_LITERAL, punches * (seg + run) + seg, dtype=np.uint8)
    copy = text.copy()
    for k in range(punches):
        a, m = k * (seg + run) + seg, min(run, n - k * run)
        copy[a:a + m] = np.frombuffer(lits[k * run:k * run + m], dtype=np.uint8)
    return text.tobytes() + bytes(65536 - len(text)) + copy.tobytes()


class Case:
    def __init__(self, name, chunk, text, block, gathered, coded=None, depth=None, lanes=None):
        self.name, self.chunk, self.text, self.block, self.gathered = name, chunk, text, block, gathered
        self.coded, self.depth, self.lanes = coded, depth, lanes      # coded symbols, the longest code, lanes that share the rarest (None: not asserted)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for n in COUNTS:
        t = two_symbol_text(n, n)
        out.append(Case(f"{n} literals of two symbols, gathered", punched_chunk(t, n), t, 1, True, coded=2, depth=1))
        for off in (0, 3):
            t, depth = comb_text(n, off, n + off)
            out.append(Case(f"{n} literals of the comb, run {off} off, gathered", punched_chunk(t, n + off), t, 1, True,
                            coded=len(set(t)), depth=depth, lanes=1 + (off != 0)))
            t = matchless_text(n, off)
            out.append(Case(f"{n} literals, run {off} off, in place", t, t, 0, False, lanes=1 + (off != 0)))
    return out


@functools.lru_cache(maxsize=None)
def oracle(level):
    return B.oracle_frames([c.chunk for c in cases()], level)


def test_the_cases_reach_their_borders():
    """on oracle E's frames at level 3 (this part needs no GPU, but belongs with the comparison below)"""
    for c, frame in zip(cases(), oracle(3)):
        n, name = len(c.text), c.name
        if c.lanes is not None:
            rare = set(range(FIRST_LITERAL, FIRST_LITERAL + RARE)) if c.gathered else {9 * s + 5 for s in range(RARE)}
            lanes = lanes_of(c.text, rare)
            assert len(lanes) == c.lanes and max(lanes) < 64 and sum(x in rare for x in c.text) == RARE, (name, lanes)
        b = W.section_shapes(frame)[c.block]
        if n == 63 and not c.gathered:
            assert b.type == 0 and b.size == 63, name                 # (stored raw: see the module's text)
            continue
        assert b.type == 2 and b.regen == n and (b.nseq >= 1) == c.gathered, (name, b.type, b.regen, b.nseq)
        if c.gathered:
            assert b.nseq == (n + 2) // 3 + 1, (name, b.nseq)          # a sequence a punched run, and the text behind the last
        if n == 63:
            assert b.lit_type == 0, name                              # (raw literals: Huffman is tried from 64 on)
            continue
        assert b.lit_type == 2 and b.streams == (1 if n < 256 else 4), (name, b.lit_type, b.streams)
        if c.gathered:
            assert b.coded == c.coded and b.max_bits == c.depth, (name, b.coded, b.max_bits, c.depth)
            if c.lanes is not None:                                   # the eight rarest, and only they, have the longest code
                longest = {s for s, w in enumerate(b.huf_weights) if w == 1}
                assert longest == set(range(FIRST_LITERAL, FIRST_LITERAL + RARE)), (name, sorted(longest))
                assert c.depth == (11 if n >= 511 else 9 if n >= 255 else 6), (name, c.depth)
        else:
            assert b.max_bits >= n.bit_length() - 1, (name, b.max_bits)
            if n >= 2049:
                assert b.max_bits == 11, (name, b.max_bits)


@pytest.mark.parametrize("level", [1, 3])
def test_packed_literals_match_the_oracle(codec, level):
    chunks = [c.chunk for c in cases()]
    got = B.compress_many(codec, chunks, level)
    differ = [(c.name, len(g), len(x), B.first_difference(g, x)) for c, g, x in zip(cases(), got, oracle(level)) if g != x]
    assert not differ, (f"level {level}", "frames differ from oracle E's: (case, sizes, first difference)", differ[:12])
    B.assert_round_trip(codec, got, chunks, b"", f"level {level}")
