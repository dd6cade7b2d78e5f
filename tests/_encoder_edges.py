"""A seeded catalogue of chunks that steer the ENCODER onto the borders of its section rules: the block type, the literals type and its
header width, 1 or 4 Huffman streams, the not-smaller-than-raw tests, the weight description's form, the 11-bit code-length cap, the width
of Number_of_Sequences, the predefined-table rule, the long length and offset codes, the gather's 16384-byte regions and the sequence
counts at which the FSE chain is cut in other segments (zstandard_amd/csrc/entropy_kernels.hip; every rule is stated a second time in
oracle/zso_encoder.c).  TEST INFRASTRUCTURE, no fixture files: every chunk is made from a seed.

An entry is a name, a family, a chunk, an optional raw-content dictionary, and a predicate over _framewriter.section_shapes(oracle E's
frame) at level 3: the decision the entry exists for.  Reach is a CPU fact, read from oracle E's own frames; the tests re-assert it
on the frames they compare against, so a change of numpy's generator or of the LZ stage fails them instead of silently shrinking them.

Two things make a chunk's parse predictable.  The LZ stage's hash tables have 2^13 slots (2^14 for a unit above 64 KiB) and the last
writer keeps a slot, so a copy is found reliably only when its source is recent, or when what lies between is zeros (which all hash to
one slot and evict nothing).  And after a match the walker tries its last offset again, so a copy with single bytes changed
("punches") becomes one repeat-offset sequence with one literal per punch."""
import functools, heapq, zlib
import numpy as np
import _batch as B
import _framewriter as W

LEVELS = (1, 3, 4)
MAX_CHUNK, MAX_BYTES, MAX_ENTRIES = 131073, 32 << 20, 800

# the sequence counts the catalogue holds one chunk for: the header width at 127 / 128, the predefined rule at 63 / 64, and for the
# chain (ZS_CHAIN_MINSEG = 4 blocks of 16 steps, ZS_CHAIN_MAXSEG = 21 segments, ZS_CHAIN_WARM = 512 steps): every count up to 130, every
# multiple of 16 and its neighbours up to 1441 (the 16-step tail; 4 blocks a segment hold up to 21 * 64 = 1344, where a segment first
# grows past 4 blocks; 512 + 64 where a segment first starts inside the warm-up), 2687 .. 2690 (21 * 128 = 2688: past 8 blocks) and
# 4095 .. 4097 (the toggles' second sweep)
S = sorted(set(range(131)) | {16 * m + d for m in range(8, 91) for d in (-1, 0, 1)} | {2687, 2688, 2689, 2690, 4095, 4096, 4097})

# What no input can reach, with the arithmetic.  The list is fixed; each item is a predicate over one block's shape that must hold for no
# block of any frame of the catalogue (tests/test_encoder_edges_host.py).
DECLARED_UNREACHABLE = {
    # every sequence of this encoder has a match of >= 4 bytes (a repeat offset's shortest), so a block of <= 65536 bytes holds <= 16384 of
    # them, and 0x7F00 = 32512
    "Number_of_Sequences >= 0x7F00 (the 3-byte form)": lambda b: b.type == 2 and (b.nseq >= 0x7F00 or b.nseq_bytes == 3),
    # LL code 35 is a literal length >= 65536 in front of a match and ML code 52 a match of >= 65539 bytes: a block is <= 65536 bytes
    "literal-length code 35": lambda b: b.type == 2 and b.nseq > 0 and _codes(b.ll, 35),
    "match-length code 52": lambda b: b.type == 2 and b.nseq > 0 and _codes(b.ml, 52),
    # a stream codes <= ceil(65536 / 4) = 16384 literals at <= 11 bits: <= 22529 bytes (and one stream is used below 256 literals only)
    "a Huffman stream above 65535 bytes": lambda b: b.type == 2 and b.lit_type == 2 and _longest_stream(b) > 65535,
    # four streams: 6 bytes of jump table + 4 streams of >= 1 byte + a description of >= 2 bytes = 12 > 10
    "four streams stored in fewer than 10 bytes": lambda b: b.type == 2 and b.lit_type == 2 and b.streams == 4 and b.csize < 10,
}


def _codes(table, c):
    """does this table description give code c a cell (None: the predefined table hides it)"""
    if table.mode == "rle":
        return table.symbol == c
    return bool(table.norm[c]) if table.mode == "fse" else False


def _longest_stream(b):
    if b.streams == 1:
        return b.csize
    j = b.frame_bytes[b.jump_pos:b.jump_pos + 6]
    s = [int.from_bytes(j[i:i + 2], "little") for i in (0, 2, 4)]
    return max(s + [b.end_of_literals - b.jump_pos - 6 - sum(s)])


def shapes(frame):
    """section_shapes with what _longest_stream needs (where the jump table lies)"""
    out = W.section_shapes(frame)
    for b in out:
        if b.type == 2 and b.lit_type == 2:
            b.frame_bytes, b.jump_pos, b.end_of_literals = frame, W.huf_weights(frame, b.huf_pos)[1], b.seq_pos
    return out


def describe(sh):
    """one line per frame: what its blocks are"""
    out = []
    for b in sh:
        if b.type != 2:
            out.append(f"{('raw', 'rle')[b.type]}({b.size})"); continue
        lit = ("rawlit", "rlelit", "huf", "treeless")[b.lit_type] + f"({b.regen}, sf{b.size_format}"
        if b.lit_type == 2:
            lit += f", {b.streams} stream{'s' * (b.streams > 1)}, weights {b.weights}, {b.coded} coded <= {b.max_symbol}, longest {b.max_bits}"
        seq = f"nseq {b.nseq}/{b.nseq_bytes}B"
        if b.nseq:
            seq += " " + " ".join(t.mode + (f"={t.symbol}" if t.mode == "rle" else f"@{t.al}" if t.mode == "fse" else "")
                                  for t in (b.ll, b.of, b.ml))
        out.append(f"comp({b.size}: {lit}) {seq})")
    return " | ".join(out)


def huffman_depth(data):
    """the longest code of a Huffman code without a length limit for the bytes' histogram (heapq; of equal weights the shallower tree is
    merged first, which keeps the tree as flat as an optimal one can be)"""
    h = [(int(c), 0) for c in np.bincount(np.frombuffer(data, dtype=np.uint8)) if c]
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


class Entry:
    def __init__(self, name, family, chunk, reached, what, dic=b"", level3_only=False, last=False):
        self.name, self.family, self.chunk, self.reached, self.what, self.dic = name, family, bytes(chunk), reached, what, dic
        self.level3_only, self.last = level3_only, last
        assert len(self.chunk) <= MAX_CHUNK, name

    @property
    def id(self):
        return f"{self.family}/{self.name}"

    def holds(self, frame):
        try:
            return bool(self.reached(shapes(frame)))
        except (IndexError, AttributeError, TypeError):       # another block structure than the predicate reads
            return False


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def alpha(name, n, k):
    """n uniform bytes over k values"""
    return _rng(name).integers(0, k, n, dtype=np.uint8).tobytes()


def noise(name, n):
    return alpha(name, n, 256)


def punched(t, n, period, byte=0xFF):
    """n bytes of t (wrapping) with every period-th byte set to `byte`"""
    p = np.frombuffer((t * (n // len(t) + 1))[:n], dtype=np.uint8).copy()
    p[period - 1::period] = byte
    return p.tobytes()


def ordered(entries, turn=0, reverse=False):
    """the entries in catalogue order (or reversed) with one of those marked `last` moved to the end: the turn-th of them, so that each
    batch of a test ends in another one (their sources end where the batch's buffer ends)"""
    es = list(entries)[::-1] if reverse else list(entries)
    lasts = [e for e in es if e.last]
    if lasts:
        pick = lasts[turn % len(lasts)]
        es.remove(pick); es.append(pick)
    return es


def oracle_frames(entries, level):
    """oracle E's frames of the entries (one batch call per dictionary) -> [frame] in their order"""
    out = [None] * len(entries)
    for dic in sorted({e.dic for e in entries}):
        idx = [i for i, e in enumerate(entries) if e.dic == dic]
        for i, f in zip(idx, B.oracle_frames([entries[i].chunk for i in idx], level, dic)):
            out[i] = f
    return out


# ---------------------------------------------------------------------------------------------------------------- predicates
def one(pred):
    """a frame of one block for which pred holds"""
    return lambda sh: len(sh) == 1 and pred(sh[0])


def block(i, pred):
    return lambda sh: pred(sh[i])


def comp(b, lit_type=None, regen=None, nseq=None, sf=None, streams=None):
    return (b.type == 2 and (lit_type is None or b.lit_type == lit_type) and (regen is None or b.regen == regen)
            and (nseq is None or b.nseq == nseq) and (sf is None or b.size_format == sf) and (streams is None or b.streams == streams))


RAW, RLE, HUF = 0, 1, 2


# ---------------------------------------------------------------------------------------------------------------- the catalogue
UNREACHED = {}     # name -> (in S or not, the nearest shape that was reached); filled by catalogue()


def _search_compressed_or_raw(add):
    """the compressed-or-raw rule, lit + seq < n: among alpha(n, k), n in 64 .. 400, the chunk whose compressed block is the least
    smaller than n, and one of the same generator left raw"""
    cands = [(n, k) for k in (24, 40, 64, 100) for n in range(64, 401, 3)]
    chunks = [alpha(f"margin{n}_{k}", n, k) for n, k in cands]
    best, raws = None, {}
    for (n, k), c, f in zip(cands, chunks, B.oracle_frames(chunks, 3)):
        b = W.section_shapes(f)[0]
        if b.type == 2 and n - b.size in (1, 2) and (best is None or n - b.size < best[0]):
            best = (n - b.size, n, k, c)
        if b.type == 0:
            raws[k] = (n, k, c)                                  # (ascending n: the largest n of this k left raw)
    margins = {}
    if best:
        m, n, k, c = best
        add(f"compressed_by_{m}_alpha({n},{k})", "block", c, one(lambda b, n=n, m=m: comp(b) and b.size == n - m),
            f"compressed with Block_Size n - {m}")
        margins["compressed"] = (n, k, m)
    if best and best[2] in raws:
        n, k, c = raws[best[2]]
        add(f"left_raw_alpha({n},{k})", "block", c, one(lambda b, n=n: b.type == 0 and b.size == n), "not smaller than n: raw block")
        margins["raw"] = (n, k)
    return margins


def _seq_generator(seed, kmax):
    """chunks of 4096 high-entropy bytes followed by k pieces of 16 bytes copied from them, each followed by 2 fresh bytes: chunk k is a
    prefix of chunk k + 1 and has about k + 1 sequences"""
    r = _rng(f"seqcount{seed}")
    base = r.integers(0, 256, 4096, dtype=np.uint8).tobytes()
    out, cur = [], bytearray(base)
    for k in range(kmax + 1):
        out.append(bytes(cur))
        a = int(r.integers(0, 4080))
        cur += base[a:a + 16] + r.integers(0, 256, 2, dtype=np.uint8).tobytes()
    return out


def _sweep_sequence_counts(add, want):
    """one chunk for each sequence count in `want` (<= 2690), from up to 8 seeds of the generator; -> the counts not reached"""
    missing = set(want)
    for seed in range(8):
        if not missing:
            break
        gen = _seq_generator(seed, 2400)
        ks = [k for k in range(len(gen)) if k <= 1300 or 2250 <= k] if seed == 0 else None
        if ks is None:          # later seeds: only around what is still missing (a chunk of k pieces has k + 1 .. 1.2 k + 3 sequences)
            ks = sorted({k for s in missing for k in range(int(s / 1.22) - 2, s + 1) if 0 <= k < len(gen)})
        for k, f in zip(ks, B.oracle_frames([gen[k] for k in ks], 3)):
            sh = W.section_shapes(f)
            if len(sh) == 1 and sh[0].type == 2 and sh[0].nseq in missing:
                n = sh[0].nseq
                missing.discard(n)
                add(f"nseq{n}", "seqcount", gen[k], one(lambda b, n=n: comp(b, nseq=n)), f"{n} sequences")
    return missing


def _settle(E, pending, variants=6):
    """Where a chunk's parse depends on chance (a hash slot lost to a later position, a byte that happens to extend a match backwards), its
    entry gives a function of a variant number.  Takes for each the first variant whose predicate holds at every level; failing that the
    first that holds at level 3, marked level-3-only; failing that variant 0, which the tests then report."""
    at3 = {}
    for v in range(variants):
        if not pending:
            break
        es = [Entry(E[i].name, E[i].family, make(v), E[i].reached, E[i].what, E[i].dic, last=E[i].last) for i, make in pending]
        ok = {lv: [e.holds(f) for e, f in zip(es, oracle_frames(es, lv))] for lv in LEVELS}
        left = []
        for j, (i, make) in enumerate(pending):
            if all(ok[lv][j] for lv in LEVELS):
                E[i] = es[j]; at3.pop(i, None)
            else:
                if ok[3][j] and i not in at3:
                    at3[i] = es[j]
                left.append((i, make))
        pending = left
    for i, e in at3.items():
        e.level3_only = True; E[i] = e


@functools.lru_cache(maxsize=1)
def catalogue():
    """-> (entries, notes): notes holds what the searches found (the margins of the compressed-or-raw rule)"""
    E, notes = [], {}
    UNREACHED.clear()
    pending = []                                                 # (index in E, make): chunks that depend on chance, see _settle

    def add(name, family, chunk, reached, what, **kw):
        if callable(chunk):
            pending.append((len(E), chunk)); chunk = chunk(0)
        E.append(Entry(name, family, chunk, reached, what, **kw))

    # ------------------------------------------------------------------ block: the block type
    fam = "block"
    add("empty", fam, b"", one(lambda b: b.type == 0 and b.size == 0), "a raw block of 0")
    for n in range(2, 16):
        add(f"short{n}", fam, noise(f"short{n}", n), one(lambda b, n=n: b.type == 0 and b.size == n), "raw by the n < 16 rule")
    for n in (1, 15, 16, 17, 4095, 4096, 4097, 65535, 65536):
        add(f"constant{n}", fam, b"\x07" * n, one(lambda b, n=n: b.type == 1 and b.size == n), "one RLE block")
    add("constant65537", fam, b"\x07" * 65537, lambda sh: [(b.type, b.size) for b in sh] == [(1, 65536), (1, 1)], "two RLE blocks")
    for n, where in ((4097, (0, 15, 16, 4095, 4096)), (65536, (0, 15, 16, 4095, 4096, 65535))):
        for p in where:                                         # the all-equal scan: 16-byte lanes, 4096-byte rounds, byte-wise tail
            c = bytearray(b"\x07" * n); c[p] = 0x70
            add(f"constant{n}_but_{p}", fam, c, one(lambda b: b.type == 2), "not an RLE block: compressed")
    notes["margins"] = _search_compressed_or_raw(add)

    # ------------------------------------------------------------------ literals: type and header
    fam = "literals"
    T = alpha("T", 4096, 200)
    for k, (lt, lh) in {4: (RAW, 1), 5: (RLE, 1), 31: (RLE, 1), 32: (RLE, 2)}.items():
        P = punched(T, k * 40, 40)
        what = f"{('raw', 'RLE')[lt]} literals of {k}, {k} sequences, " + (f"a section of {lh + 1} bytes" if lt == RLE else f"a {lh}-byte header")
        pred = lambda b, k=k, lt=lt, lh=lh: comp(b, lt, k, k) and b.lit_header == lh
        add(f"punched{k}_second_block", fam, T + bytes(61440) + P, block(1, pred), what)
        add(f"punched{k}_dictionary", fam, P, one(pred), what, dic=T)
    for n in (32, 63, 4095, 4096):
        def make(v, n=n):                                        # (a copy from the chunk's second byte on: a match is not extended
            x = alpha(f"rawlit{n}_{v}", n, 256 if n > 63 else 64)    # backwards onto the chunk's first byte)
            return x + x[1:]
        add(f"rawlit{n}", fam, make, one(lambda b, n=n: comp(b, RAW, n, 1) and b.lit_header == 1 + (n > 31) + (n > 4095)),
            f"raw literals of {n} with one sequence")
    x = noise("rawlit31", 31)
    add("rawlit31", fam, x * 4, one(lambda b: comp(b, RAW, 31, 1) and b.lit_header == 1), "raw literals of 31 with the one-byte header")
    x = alpha("huf64", 64, 16)
    add("huf64_with_sequence", fam, x + x[:40], one(lambda b: comp(b, HUF, 64, 1, sf=0)), "Huffman at the smallest size that tries it, one sequence")
    for n in (255, 256, 257, 258, 259, 260, 1023, 1024, 16383, 16384, 65532, 65533, 65534, 65535, 65536):
        sf = 0 if n < 256 else 1 if n < 1024 else 2 if n < 16384 else 3
        add(f"huf{n}", fam, alpha(f"huf{n}", n, 100), one(lambda b, n=n, sf=sf: comp(b, HUF, n, 0, sf=sf, streams=1 if n < 256 else 4)),
            f"Huffman literals of {n}, no sequence: size format {sf}" + (", the ungathered path" if n > 60000 else ""),
            last=n % 4 != 0 and n > 60000)
    # RLE literals of >= 4096 (the 4-byte section) need >= 4096 matches whose sources all differ from the literal's byte where the chunk has
    # it: 4096 copies of >= 5 bytes from >= 20 KiB of unpunched text that no copy repeats, each found at its first byte.  The hash tables
    # lose most of 20 KiB (a walk range's first bytes stay literals until a slot survives), and a wrapping text matches its last punched
    # copy, punches included (4369 punches of period 15 over T wrapping 16 times: Huffman literals of 8183, 4237 sequences).
    UNREACHED["literals/rle_literals_4096"] = (False, "RLE literals of 100 in a 3-byte section (codes/repeat_after_literal)")

    add("huf256_dictionary", fam, alpha("huf256d", 256, 100), one(lambda b: comp(b, HUF, 256, 0, sf=1, streams=4)),
        "Huffman literals of 256 in four streams behind a dictionary", dic=T)
    for k in (63, 64, 127, 128):
        add(f"punched{k}_dictionary", fam, punched(T, k * 30, 30), one(lambda b, k=k: comp(b, RLE, k, k) and b.nseq_bytes == 1 + (k > 127)
                                                                      and (b.ll.mode == "pre") == (k < 64)),
            f"{k} sequences behind a dictionary: " + ("predefined" if k < 64 else "computed") + f" tables, a {1 + (k > 127)}-byte count", dic=T)

    # ------------------------------------------------------------------ Huffman shapes
    fam = "huffman"
    two = np.frombuffer(punched(T, 4000, 40), dtype=np.uint8).copy(); two[79::80] = 0xFE
    add("two_symbols", fam, T + bytes(61440) + two.tobytes(), block(1, lambda b: comp(b, HUF, 100, 100, streams=1) and b.coded == 2),
        "100 literals of 2 coded symbols")
    for k in (128, 129, 130):
        c = np.tile(np.arange(k, dtype=np.uint8), 24); _rng(f"flat{k}").shuffle(c)
        add(f"coded{k}", fam, c.tobytes(), one(lambda b, k=k: comp(b, HUF, nseq=0) and b.coded == k and b.max_symbol == k - 1
                                               and (b.weights == "4bit") == (k == 128)),
            f"exactly {k} coded symbols, as frequent as each other: " + ("127 equal weights, the 4-bit form" if k == 128 else "FSE weights"))
    # the 4-bit form's last size, 128 weights: values 0 .. 127 four times each, every second byte 128.  The 128 rare values get 8 bits and
    # 128 gets 1: the 128 weights written are all equal, which has no FSE form.  Each run of 128 values steps by another odd number, so no
    # pair of neighbours comes twice and no 5 bytes repeat: no match
    c = np.full(1024, 128, dtype=np.uint8)
    c[0::2] = np.concatenate([(np.arange(128) * st) % 128 for st in (1, 3, 5, 7)])
    add("coded129_direct", fam, c.tobytes(), one(lambda b: comp(b, HUF, 1024, 0) and b.coded == 129 and b.max_symbol == 128 and b.weights == "4bit"
                                                 and b.max_bits == 8),
        "129 coded symbols, 128 equal weights in the 4-bit form: its limit")
    c = np.repeat(np.array([0, 3, 50, 51, 200, 255], dtype=np.uint8), [300, 200, 150, 100, 80, 60]); _rng("gaps").shuffle(c)
    add("symbol255_with_gaps", fam, c.tobytes(), one(lambda b: comp(b, HUF) and b.max_symbol == 255 and b.coded == 6),
        "largest symbol 255 with gaps below it")
    add("weights_direct", fam, alpha("direct", 2000, 16), one(lambda b: comp(b, HUF) and b.weights == "4bit"), "the direct weight form")
    add("weights_fse", fam, alpha("fse", 3000, 100), one(lambda b: comp(b, HUF) and b.weights in (5, 6)), "the FSE weight form")
    c = np.tile(np.arange(256, dtype=np.uint8), 128); _rng("flat256").shuffle(c)
    add("flat256", fam, c.tobytes(), one(lambda b: b.type == 0), "flat counts over all 256 values: raw")
    c = np.concatenate([c, np.full(128, 77, dtype=np.uint8)]); _rng("flat256b").shuffle(c)
    add("flat256_one_double", fam, c.tobytes(), one(lambda b: b.type == 0), "all 256 values, one at twice the rarest: still raw")
    x = noise("flatraw", 30000)
    add("flat_literals_raw", fam, x * 2, one(lambda b: comp(b, RAW, nseq=1) or comp(b, RAW)), "flat-count literals left raw, with sequences")
    # the 11-bit cap: 200 values 55 times each and eight rare ones 1, 1, 2, 3, 5, 8, 13, 21 times: the rare ones chain below a leaf of a tree of
    # depth 7 or 8, so the unconstrained code is at least 14 deep; 200 near-uniform values repeat no 5 bytes, so there is no match
    c = np.repeat(np.arange(208, dtype=np.uint8), [55] * 200 + [1, 1, 2, 3, 5, 8, 13, 21]); _rng("cap11").shuffle(c)
    assert huffman_depth(c.tobytes()) >= 13
    add("cap11_binding", fam, c.tobytes(), one(lambda b: comp(b, HUF, 11054, 0) and b.max_bits == 11),
        f"unconstrained Huffman depth {huffman_depth(c.tobytes())}, longest code exactly 11")

    # ------------------------------------------------------------------ gather (blocks with sequences)
    fam = "gather"
    for n in (65536, 40001):
        x = noise(f"period{n}", 300)
        add(f"match_to_last_byte_{n}", fam, (x * 220)[:n], one(lambda b, n=n: comp(b, regen=300, nseq=1) and b.size < 400),
            f"300 literals, then one match that ends on the block's last byte, {n}" + ("; regions 1 .. 3 lie inside it" if n == 65536 else ""))
    x = noise("second_first", 65536)
    add("match_from_second_blocks_first_byte", fam, x + x[-2000:-500] + noise("second_tail", 500),
        block(1, lambda b: comp(b, regen=500, nseq=1)), "a second block of one match from its first byte and 500 literals")
    x = noise("all_literal_region", 36000)
    y = noise("all_literal_period", 300)
    add("regions_all_literals", fam, x + (y * 100)[:29536], one(lambda b: comp(b, regen=36300, nseq=1)),
        "regions 0 and 1 all literals, region 3 inside one match")
    def straddle(tag, first, seg, n, v=0):
        """literal runs and copies of the run before them in turn, seg bytes each (the first run: `first`) -> (chunk, literals, copies)"""
        parts, lits, copies, pos, k = [], 0, 0, 0, 0
        while pos < n:
            ln = min(first if k == 0 else seg, n - pos)
            if k % 2 == 0 or ln < 16:
                parts.append(noise(f"straddle{tag}{k}_{v}", ln)); lits += ln
            else:
                parts.append(parts[-1][-ln:]); copies += 1
            pos += ln; k += 1
        return b"".join(parts), lits, copies
    for tag, first in (("a", 700), ("b", 1400), ("c", 1024)):
        seg = 1024 if tag == "c" else 700
        n = 65531 if tag == "b" else 65536
        _, lits, copies = straddle(tag, first, seg, n)
        add(f"straddle_{tag}", fam, lambda v, a=(tag, first, seg, n): straddle(*a, v)[0], one(lambda b, lits=lits, copies=copies: comp(b, regen=lits, nseq=copies)),
            f"{copies} matches and literal runs of {seg} in turn from {first}: {lits} literals" + (", n % 16 = 11" if tag == "b" else ""))
    add("punched_period13", fam, T + bytes(61440) + punched(T, 65536, 13), block(1, lambda b: comp(b) and b.nseq >= 4098),
        ">= 4098 sequences in a block: the toggles' second sweep")
    # 4095 = 7 * 585 bytes of T wrapping, every 7th byte punched with the wrap's number: a wrap differs from the one before it in the
    # punches alone, so every 6 bytes between two punches are one repeat-offset match
    p = np.frombuffer((T[:4095] * 17)[:65536], dtype=np.uint8).copy()
    i = np.arange(65536)
    p[i % 4095 % 7 == 6] = (0xE0 + i // 4095)[i % 4095 % 7 == 6]
    add("punched_period7", fam, T[:4095] + bytes(61441) + p.tobytes(), block(1, lambda b: comp(b) and b.nseq > 8192), "> 8192 sequences in a block")

    # ------------------------------------------------------------------ sequence count and the chain's cut
    fam = "seqcount"
    add("nseq0", fam, alpha("nseq0", 500, 100), one(lambda b: comp(b, nseq=0)), "0 sequences")
    missing = _sweep_sequence_counts(add, [s for s in S if 0 < s <= 2690])
    found = {}
    cands = [(k, T + bytes(61440) + punched(T, 13 * k + j, 13)) for k in range(4090, 4100) for j in (0, 6)]
    for (k, c), f in zip(cands, B.oracle_frames([c for _, c in cands], 3)):
        found.setdefault(W.section_shapes(f)[1].nseq, c)
    for s in (4095, 4096, 4097):
        if s in found:
            add(f"nseq{s}", fam, found[s], block(1, lambda b, s=s: comp(b, nseq=s)), f"{s} sequences")
        else:
            missing.add(s)
    for s in sorted(missing):
        UNREACHED[f"seqcount/nseq{s}"] = (True, "its neighbours in S")

    # ------------------------------------------------------------------ long codes (one sequence: every table in RLE mode names its code)
    fam = "codes"
    for j in range(4, 16):
        for ll in ((1 << j) - 1, 1 << j):
            def make(v, ll=ll):
                x = noise(f"ll{ll}_{v}", ll)
                return x + (x[-min(ll, 64):] * 8)[:60 if ll < 8192 else 400]
            add(f"literal_length_{ll}", fam, make,
                one(lambda b, ll=ll: comp(b, regen=ll, nseq=1) and b.ll.mode == "rle" and b.ll.symbol == W.code_of(W.LL_CODES, ll)[0]),
                f"literal length {ll}: code {W.code_of(W.LL_CODES, ll)[0]}")
    for j in range(5, 16):
        for ml in ((1 << j) - 1 + 3, (1 << j) + 3):
            x = noise(f"ml{ml}", 64)
            add(f"match_length_{ml}", fam, (x * 520)[:64 + ml],
                one(lambda b, ml=ml: comp(b, regen=64, nseq=1) and b.ml.mode == "rle" and b.ml.symbol == W.code_of(W.ML_CODES, ml)[0]),
                f"match length {ml}: code {W.code_of(W.ML_CODES, ml)[0]}")
    for j in range(3, 17):
        for off in ((1 << j) - 4, (1 << j) - 3):
            x = noise(f"off{off}", off)
            m = 60 if off < 2048 else max(200, off // 16)
            code = (off + 3).bit_length() - 1
            pred = lambda b, code=code: comp(b, nseq=1) and b.of.mode == "rle" and b.of.symbol == code
            if off == 4:        # offset 4 is the second of the starting recent offsets {1, 4, 8}: a first block codes it as a repeat
                add("offset_4_is_a_repeat", fam, (x * 20)[:64], one(lambda b: comp(b, nseq=1) and b.of.mode == "rle" and b.of.symbol == 1),
                    "offset 4 in a first block: the repeat code 2 (offset code 1)")
                add("offset_4", fam, T + bytes(61440) + (x * 20)[:64], block(1, pred), "offset 4 in a second block: code 2")
                continue
            pred = lambda b, code=code: comp(b, nseq=1) and b.of.mode == "rle" and b.of.symbol == code
            add(f"offset_{off}", fam, x + (x * 20)[:m], one(pred) if off + m <= 65536 else block(1, pred), f"offset {off}: code {code}")
    UNREACHED["codes/offset_code_17"] = (False, "offset code 16 (offset 65533); a match of >= 4 bytes in a unit of 131072 bytes starts at "
                                               "<= 131068, its source at >= 0: offset + 3 <= 131071 < 2^17")
    # recent offsets behind one literal (the punched copy) and behind none (every third match touches the one before it)
    add("repeat_after_literal", fam, T + bytes(61440) + punched(T, 4000, 40), block(1, lambda b: comp(b, nseq=100) and _codes(b.of, 0)),
        "100 sequences, all but the first the repeat offset behind one literal")
    parts = []
    for i in range(30):
        x, y = noise(f"adjx{i}", 40), noise(f"adjy{i}", 40)
        parts += [x, y, x[:20], y[10:30], y[:20]]
    add("repeat_without_literal", fam, b"".join(parts), one(lambda b: comp(b, nseq=90) and (_codes(b.of, 0) or _codes(b.of, 1)) and _codes(b.ll, 0)),
        "90 sequences, every third of literal length 0 at the offset before the last")
    _settle(E, pending)
    sweep = [e for e in E if e.family == "seqcount"]           # a sequence count is the LZ stage's, and another level's parse gives another
    for lv in (1, 4):
        for e, f in zip(sweep, oracle_frames(sweep, lv)):
            e.level3_only |= not e.holds(f)
    assert len(E) <= MAX_ENTRIES and sum(len(e.chunk) for e in E) <= MAX_BYTES
    assert len({e.id for e in E}) == len(E)
    return tuple(E), notes
