"""A seeded catalogue of hand-built frames that steer the decoders onto their edges (tests/_framewriter.py writes them).

Each entry: name, family, frame bytes, content (the writer's, None where the plan has none), cap (the output capacity the item is
decoded at) and expect: 'ok' (decodes to content) or the error code of ZStdErrors.cs:61-90 the reference gives (pinned here, checked
against oracle D by tests/test_oracle_edge_frames.py).  TEST INFRASTRUCTURE."""
import functools, random
import _framewriter as W

COR, CK, SRC, DST, PAR, WIN, DIC, DICW = 20, 22, 72, 70, 14, 16, 30, 32


class Entry:
    def __init__(self, name, family, frame, content, expect="ok", cap=None, note=""):
        self.name, self.family, self.frame, self.content, self.expect, self.note = name, family, frame, content, expect, note
        self.cap = cap if cap is not None else (len(content) if content is not None else 4096)
        assert expect != "ok" or content is not None, name

    @property
    def id(self):
        return f"{self.family}/{self.name}"


def _text(rng, n, alphabet=b"etaoin shrdlucmfwyp,.\n"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _seq_block(rng, lits, nseq, maxoff=16, ml=(3, 12)):
    """nseq sequences of small literal lengths over `lits` whose offsets stay inside the output made so far (one-block frames)"""
    seqs, used, made = [], 0, 0
    for i in range(nseq):
        ll = rng.randint(0 if i else 4, 4)
        m = rng.randint(*ml)
        seqs.append((ll, m, rng.randint(1, min(maxoff, made + ll)) + 3))
        used += ll; made += ll + m
    assert used <= len(lits)
    return seqs


@functools.lru_cache(maxsize=1)
def catalogue():
    rng = random.Random(20261016)
    E = []

    def add(name, family, planned, expect="ok", cap=None, note="", frame=None):
        f, c = planned
        E.append(Entry(name, family, f if frame is None else frame, c, expect, cap, note))

    txt = _text(rng, 70000)
    noise = bytes(rng.getrandbits(8) for _ in range(4096))

    # ---- frame header
    fam = "header"
    for n, fb, single in [(0, 1, True), (255, 1, True), (256, 2, True), (65791, 2, True), (0, 4, True), (65792, 4, True),
                          (0, 8, True), (1000, 8, True), (256, 2, False), (65791, 2, False), (5000, 4, False), (5000, 8, False)]:
        blocks = [W.raw(txt[:n])] if n <= 65536 else [W.raw(txt[:65536]), W.raw(txt[65536:n] + txt[:max(0, n - 70000)])]
        add(f"fcs{fb}_{n}_{'single' if single else 'window'}", fam, W.frame(blocks, fcs_bytes=fb, single=single, window=(7, 0)))
    for e in range(0, 22):
        add(f"nofcs_windowlog{10 + e}", fam, W.frame([W.comp(W.Lit("huf", txt[:700]), W.Seqs(_seq_block(rng, txt[:700], 20)))],
                                                     fcs=None, single=False, window=(e, 7 if e == 3 else 0)),
            expect="ok" if e <= 20 else WIN)
    for did, db in [(1, 1), (300, 2), (70000, 4), (5, 4)]:
        add(f"dictid{db}_{did}", fam, W.frame([W.raw(txt[:40])], dict_id=did, dict_bytes=db), expect=DICW)
    add("dictid1_zero", fam, W.frame([W.raw(txt[:40])], dict_id=0, dict_bytes=1))
    add("reserved_bit", fam, W.frame([W.raw(txt[:40])], reserved=True), expect=PAR)
    for d in (-1, 1):
        add(f"fcs_off_by{d:+d}", fam, W.frame([W.raw(txt[:300])], fcs=300 + d), expect=COR, cap=400)
    add("fcs_4gib", fam, W.frame([W.raw(txt[:300])], fcs=1 << 32, fcs_bytes=8), expect=COR, cap=400)
    add("fcs_4gib_minus1", fam, W.frame([W.raw(txt[:300])], fcs=(1 << 32) - 1, fcs_bytes=4), expect=COR, cap=400)
    add("bad_magic", fam, W.frame([W.raw(txt[:40])], magic=0xFD2FB527), expect=10, cap=40)
    # the order of refusals inside a header - too few bytes for it and a block header, then the reserved bit, then the window log: three
    # header shapes (and the windowed one with window log 31) over one 40-byte raw block, each cut to every length from 5 bytes up to the
    # header and the block header, as written and with the reserved bit set (the windowed shape's 2-byte content size cannot say 40)
    for shape, hs, kw in [("single_did4_fcs8", 17, dict(dict_id=0, dict_bytes=4, fcs_bytes=8)), ("window_fcs2", 8, dict(single=False, window=(0, 0), fcs=300)),
                          ("single_fcs1", 6, {}), ("windowlog31_fcs2", 8, dict(single=False, window=(21, 0), fcs=300))]:
        for res in (False, True):
            f, c = W.frame([W.raw(txt[:40])], reserved=res, **kw)
            assert W.frame_header(f).end == hs
            whole = PAR if res else WIN if "log31" in shape else COR if "fcs" in kw else "ok"
            add(f"{shape}{'_reserved' if res else ''}", fam, (f, c), expect=whole, cap=40)
            for n in range(5, hs + 4):
                add(f"{shape}{'_reserved' if res else ''}_cut{n}", fam, (f, c), expect=SRC if n < hs + 3 or whole in ("ok", COR) else whole, cap=40, frame=f[:n])

    # ---- checksum (XXH64 tails: 32-byte stripes, 8-, 4- and 1-byte rests)
    fam = "checksum"
    for n in (0, 1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 65, 1000):
        for bad in (False, True):
            body = [W.raw(noise[:n])] if n % 2 or n == 0 else [W.comp(W.Lit("raw", txt[:n]))]
            add(f"n{n}_{'bad' if bad else 'ok'}", fam, W.frame(body, checksum=True, bad_checksum=bad), expect=CK if bad else "ok")
    add("window_n1000_ok", fam, W.frame([W.comp(W.Lit("huf", txt[:1000], streams=4))], checksum=True, fcs=None, single=False, window=(0, 0)))
    add("truncated_checksum", fam, W.frame([W.raw(noise[:50])], checksum=True), expect=CK, cap=50,
        frame=W.frame([W.raw(noise[:50])], checksum=True)[0][:-2])

    # ---- blocks
    fam = "blocks"
    big = (txt * 2)[:131073]
    for n in (0, 1, 131072):
        add(f"raw{n}", fam, W.frame([W.raw(big[:n])]))
        add(f"rle{n}", fam, W.frame([W.rle(0x41, n)]))
    # RFC 8878 limits every block to 128 KiB of content; the reference checks it for compressed blocks only (DecompressFrame,
    # ZStdDecompress.cs:2008-2091 copies raw and RLE blocks of any size that fit dst), as does libzstd 1.4.8
    add("raw131073", fam, W.frame([W.raw(big)]), note="spec-invalid, decoded by the reference")
    add("rle131073", fam, W.frame([W.rle(0x42, 131073)]), note="spec-invalid, decoded by the reference")
    add("comp_srcsize_128k", fam, W.frame([W.comp(W.Lit("raw", big[:131068]))]), expect=SRC)
    add("comp_content_128k", fam, W.frame([W.comp(W.Lit("rle", b"z" * 131072))]))
    add("type3", fam, W.frame([W.raw(txt[:10]), W.Block("reserved", b"abc")]), expect=COR, cap=20)
    add("missing_last", fam, W.frame([W.raw(txt[:10], last=False)]), expect=SRC, cap=10)
    add("missing_last_checksum", fam, W.frame([W.raw(txt[:10], last=False)], checksum=True), expect=SRC, cap=10)
    f, c = W.frame([W.raw(txt[:10])])
    add("data_after_last", fam, (f, c), expect=SRC, frame=f + b"\x01\x02")
    add("data_after_last_5", fam, (f, c), expect=10, frame=f + b"\x01\x02\x03\x04\x05")
    add("block_size_past_end", fam, W.frame([W.raw(txt[:10], size=11)]), expect=SRC, cap=11)
    for nb in (15, 16, 17):
        blocks = []
        for i in range(nb):
            lits = txt[i * 1000:i * 1000 + 600]
            seqs = [(100, 2000, 3 + 1 + rng.randint(0, 90))] + [(50, 6000, 1)] * 10
            blocks.append(W.comp(W.Lit("huf", lits, streams=4) if i % 3 == 0 else W.Lit("treeless", lits, streams=4) if i % 3 == 1
                                 else W.Lit("raw", lits), W.Seqs(seqs, ll=("fse", 6) if i == 0 else "rep", of="pre", ml=("fse", 6) if i == 0 else "rep")))
        add(f"blocks{nb}_x64k", fam, W.frame(blocks, checksum=True))
        add(f"blocks{nb}_x1k", fam, W.frame([W.comp(W.Lit("huf", txt[i * 900:i * 900 + 800]), W.Seqs([(20, 30, 20 + 3)]))
                                             for i in range(nb)]))

    # ---- literals
    fam = "literals"
    for kind in ("raw", "rle"):
        for n in (0, 1, 31, 32, 4095, 4096, 65536):
            # raw literals of 0 and no sequences: a compressed block of 2 bytes, below the 3 every decoder asks for (MIN_CBLOCK_SIZE)
            add(f"{kind}{n}", fam, W.frame([W.comp(W.Lit(kind, (txt if kind == "raw" else b"q" * 70000)[:n], rle_byte=0x71))]),
                expect=COR if (kind, n) == ("raw", 0) else "ok", cap=n)
        for sf in (0, 1, 3):
            add(f"{kind}5_sf{sf}", fam, W.frame([W.comp(W.Lit(kind, b"xyzzy" if kind == "raw" else b"yyyyy", sf=sf))]))
    for n in (2, 3, 100, 1023):
        add(f"huf1s_{n}", fam, W.frame([W.comp(W.Lit("huf", txt[:n] if n > 3 else b"abc"[:n]))]))
    for n in (5, 6, 7, 8, 9, 1023, 1024, 16383, 16384, 65536):
        # litSize 5: segments of 2, 2, 2 leave the fourth -1 bytes (RFC 8878 §3.1.1.3.1.6): the plan writes 2, 2, 1, 0 - invalid
        add(f"huf4s_{n}", fam, W.frame([W.comp(W.Lit("huf", txt[:n], streams=4))]), expect=COR if n == 5 else "ok", cap=n)
    add("huf4s_16384_raw_noise", fam, W.frame([W.comp(W.Lit("huf", (noise * 4)[:16384], streams=4, fse=True))]))
    for mb in range(1, 14):
        syms = list(range(97, 97 + mb + 1)) if mb > 1 else [97, 98]
        lengths = W.chain_lengths(syms, mb) if mb > 1 else {97: 1, 98: 1}
        w, _ = W.lengths_to_weights(lengths)
        data = bytes(rng.choice(syms) for _ in range(300)) + bytes(syms)
        for st in (1, 4):
            add(f"maxbits{mb}_{st}s", fam, W.frame([W.comp(W.Lit("huf", data, streams=st, weights=w))]),
                expect="ok" if mb <= 11 else COR, cap=len(data))
    add("two_symbols", fam, W.frame([W.comp(W.Lit("huf", b"ab" * 200 + b"b"))]))
    for st in (1, 4):
        for fse in (None, True):
            syms = [0, 1, 2, 127, 128] if fse is None else [0, 1, 2, 200, 254, 255]
            data = bytes(rng.choice(syms) for _ in range(2000 if st == 4 else 1000))
            add(f"alphabet_top{max(syms)}_{st}s_{'fse' if fse else 'direct'}", fam,
                W.frame([W.comp(W.Lit("huf", data, streams=st, fse=fse))]))
    full = bytes(range(256)) * 8 + txt[:2000]
    for st in (1, 4):
        add(f"alphabet_256_{st}s", fam, W.frame([W.comp(W.Lit("huf", full[:700] if st == 1 else full, streams=st, fse=True))]))
    hdr = W.frame([W.comp(W.Lit("huf", txt[:500])), W.comp(W.Lit("treeless", txt[500:1000], streams=4))])
    add("treeless_second", fam, hdr)
    add("treeless_after_raw", fam, W.frame([W.comp(W.Lit("huf", txt[:500], streams=4)), W.comp(W.Lit("raw", txt[:40])), W.raw(b"xy"),
                                            W.comp(W.Lit("treeless", txt[1000:1400]), W.Seqs([(10, 20, 12)]))]))
    add("treeless_first", fam, W.frame([W.comp(W.Lit("treeless", txt[:500]))]), expect=DIC, cap=500)
    add("treeless_after_raw_only", fam, W.frame([W.comp(W.Lit("raw", txt[:500])), W.comp(W.Lit("treeless", txt[:500]))]), expect=DIC, cap=1000)

    # a literals header the block is too short for: a compressed block of 3 and of 4 bytes that announces Huffman (a block below 5 bytes) or
    # treeless literals (first in its frame: no table comes before that; behind a Huffman block: too short again) in each size format, and
    # RLE literals with the 3-byte header in a block of 3 bytes (no room for the byte)
    for n in (3, 4):
        for sf in range(4):
            for t, kind in ((2, "huf"), (3, "treeless")):
                add(f"short{n}_{kind}_sf{sf}", fam, (_as_compressed(W.frame([W.raw(bytes([t | sf << 2]) + bytes(n - 1))])[0], 0), None),
                    expect=COR if t == 2 else DIC, cap=200)
            add(f"short{n}_treeless_after_huf_sf{sf}", fam,
                (_as_compressed(W.frame([W.comp(W.Lit("huf", txt[:100])), W.raw(bytes([3 | sf << 2]) + bytes(n - 1))])[0], 1), None), expect=COR, cap=200)
    add("rle_sf3_in_3_bytes", fam, (_as_compressed(W.frame([W.raw((1 | 3 << 2 | 5 << 4).to_bytes(3, "little"))])[0], 0), None), expect=COR, cap=200)

    # ---- sequences
    fam = "sequences"
    add("nbseq0", fam, W.frame([W.comp(W.Lit("huf", txt[:300]), W.Seqs())]))
    add("nbseq0_trailing", fam, W.frame([W.comp(W.Lit("huf", txt[:300]), W.Seqs(trailing=b"\x55\x66"))]),
        note="libzstd 1.4.8 also ignores the bytes after an nbSeq of 0")
    for n in (1, 127, 128, 0x7EFF, 0x7F00, 0x7F01):
        seqs = [(0, 3, 1)] * n
        add(f"nbseq{n:#x}", fam, W.frame([W.raw(txt[:8]), W.comp(W.Lit("raw", txt[8:10]), W.Seqs(seqs, ll=("rle", 0), of=("rle", 0), ml=("rle", 0)))]))
    add("nbseq5_2byte_header", fam, W.frame([W.raw(txt[:8]), W.comp(W.Lit("raw", txt[8:10]), W.Seqs([(0, 3, 1)] * 5, nb_bytes=2))]))
    # the most a 128 KiB block can hold: 43690 sequences of 3 bytes (above ZS_FAST_MAXSEQ = 16384)
    add("nbseq43690_128k", fam, W.frame([W.raw(txt[:8]), W.comp(W.Lit("raw", txt[8:10]),
                                                                 W.Seqs([(0, 3, 1)] * 43690, ll=("rle", 0), of=("rle", 0), ml=("rle", 0)))]))
    add("nbseq43690_128k_fse", fam, W.frame([W.raw(txt[:8]), W.comp(W.Lit("raw", txt[8:10]),
                                                                     W.Seqs([(0, 3, 1 + (i % 3 == 2)) for i in range(43690)], ll="pre", of=("fse", 5), ml="pre"))]))
    lits = txt[:2000]
    base = _seq_block(rng, lits, 300, maxoff=200, ml=(3, 20))
    for t in ("ll", "of", "ml"):
        for mode in ("pre", ("fse", 6), ("fse", 5), ("fse", W.MAX_AL[t])):
            modes = {t: mode}
            add(f"{t}_{mode if isinstance(mode, str) else 'fse_al%d' % mode[1]}", fam, W.frame([W.comp(W.Lit("huf", lits, streams=4), W.Seqs(base, **modes))]))
        add(f"{t}_fse_al{W.MAX_AL[t] + 1}", fam, W.frame([W.comp(W.Lit("huf", lits, streams=4), W.Seqs(base, **{t: ("fse", W.MAX_AL[t] + 1)}))]),
            expect=COR, cap=len(W.frame([W.comp(W.Lit("huf", lits, streams=4), W.Seqs(base))])[1]))
        first = W.comp(W.Lit("huf", lits, streams=4), W.Seqs(base, ll=("fse", 6), of=("fse", 6), ml=("fse", 6)))
        again = W.comp(W.Lit("treeless", lits[:1500], streams=4), W.Seqs(base[:200], **{t: "rep"}))
        add(f"{t}_rep_second", fam, W.frame([first, again], checksum=True))
        add(f"{t}_rep_after_raw_block", fam, W.frame([first, W.raw(noise[:100]), W.rle(3, 50), again]))
        add(f"{t}_rep_first", fam, W.frame([W.comp(W.Lit("huf", lits, streams=4), W.Seqs(base, **{t: "rep"}))]), expect=COR, cap=20000)
        add(f"{t}_rep_after_nbseq0", fam, W.frame([W.comp(W.Lit("huf", lits, streams=4), W.Seqs()), W.comp(W.Lit("treeless", lits, streams=4), W.Seqs(base, **{t: "rep"}))]),
            expect=COR, cap=40000)
    add("all_rep_second", fam, W.frame([W.comp(W.Lit("huf", lits, streams=4), W.Seqs(base, ll=("fse", 9), of=("fse", 8), ml=("fse", 9))),
                                        W.comp(W.Lit("treeless", lits, streams=4), W.Seqs(base, ll="rep", of="rep", ml="rep"))]))
    add("all_rle_sym0", fam, W.frame([W.raw(b"abcd"), W.comp(W.Lit("raw", b""), W.Seqs([(0, 3, 1)] * 10, ll=("rle", 0), of=("rle", 0), ml=("rle", 0)))]))
    # RLE at the top of each alphabet, and one above it
    add("ll_rle35", fam, W.frame([W.comp(W.Lit("rle", b"L" * 65536), W.Seqs([(65536, 3, 1)], ll=("rle", 35)))]))
    add("ll_rle36", fam, W.frame([W.comp(W.Lit("rle", b"L" * 65536), W.Seqs([(65536, 3, 1)], ll=("rle", 35)))]), expect=COR, cap=65539,
        frame=_patch_mode_byte(W.frame([W.comp(W.Lit("rle", b"L" * 65536), W.Seqs([(65536, 3, 1)], ll=("rle", 35)))])[0], 36))
    add("ml_rle52", fam, W.frame([W.comp(W.Lit("raw", b"M"), W.Seqs([(1, 65539, 1)], ml=("rle", 52)))]))
    add("ml_rle53", fam, W.frame([W.comp(W.Lit("raw", b"M"), W.Seqs([(1, 65539, 1)], ml=("rle", 52)))]), expect=COR, cap=65540,
        frame=_patch_mode_byte(W.frame([W.comp(W.Lit("raw", b"M"), W.Seqs([(1, 65539, 1)], ml=("rle", 52)))])[0], 53))
    add("of_rle28", fam, W.frame([W.comp(W.Lit("raw", b"O"), W.Seqs([(1, 3, (1 << 28) + 2)], of=("rle", 28)))]), expect=COR, cap=4)
    add("of_rle31", fam, W.frame([W.comp(W.Lit("raw", b"O"), W.Seqs([(1, 3, (1 << 31) + 2)], of=("rle", 31)))]), expect=COR, cap=4)
    add("of_rle32", fam, W.frame([W.comp(W.Lit("raw", b"O"), W.Seqs([(1, 3, (1 << 31) + 2)], of=("rle", 31)))]), expect=COR, cap=4,
        frame=_patch_mode_byte(W.frame([W.comp(W.Lit("raw", b"O"), W.Seqs([(1, 3, (1 << 31) + 2)], of=("rle", 31)))])[0], 32))
    add("of_pre_code28_window", fam, W.frame([W.comp(W.Lit("raw", b"O"), W.Seqs([(1, 3, (1 << 28) + 2)]))], fcs=None, single=False, window=(20, 0)),
        expect=COR, cap=4)
    add("seq_section_short", fam, W.frame([W.comp(W.Lit("raw", b"abcdefgh"), W.Seqs([(8, 3, 4)]))]), expect=SRC, cap=11,
        frame=_cut_block(W.frame([W.comp(W.Lit("raw", b"abcdefgh"), W.Seqs([(8, 3, 4)]))])[0], 3))

    # ---- offsets and matches
    fam = "offsets"
    hist = txt[:64]
    for ll in (0, 5):
        for ov in (1, 2, 3):
            seqs = [(10, 4, 3 + 7), (3, 5, 3 + 12), (2, 4, 3 + 11), (ll, 6, ov), (4, 5, 3 + 2), (ll, 7, ov), (0, 4, 1), (ll, 3, ov)]
            add(f"rep{ov}_ll{ll}", fam, W.frame([W.comp(W.Lit("raw", hist), W.Seqs(seqs))]))
    add("rep0_minus1_is_zero", fam, W.frame([W.comp(W.Lit("raw", hist), W.Seqs([(5, 4, 1 + 3), (0, 4, 3), (0, 5, 3)]))]),
        note="RFC 8878 §3.1.2.5.1 calls a repeat offset of 0 corrupt; the reference and libzstd take 1 (`temp += !temp`)")
    add("rep0_minus1", fam, W.frame([W.comp(W.Lit("raw", hist), W.Seqs([(9, 4, 9 + 3), (0, 4, 3), (0, 5, 3), (2, 4, 3)]))]))
    add("match_to_frame_start", fam, W.frame([W.comp(W.Lit("raw", hist[:10]), W.Seqs([(5, 4, 5 + 3), (0, 30, 9 + 3)]))]))
    add("match_before_frame_start", fam, W.frame([W.comp(W.Lit("raw", hist[:10]), W.Seqs([(5, 4, 6 + 3)]))]), expect=COR, cap=14)
    add("match_before_start_later", fam, W.frame([W.raw(hist[:20]), W.comp(W.Lit("raw", hist[:10]), W.Seqs([(5, 4, 10 + 3), (0, 40, 30 + 3)]))]),
        expect=COR, cap=100)
    add("match_to_start_later_block", fam, W.frame([W.raw(hist[:20]), W.comp(W.Lit("raw", hist[:10]), W.Seqs([(5, 4, 10 + 3), (0, 40, 29 + 3)]))]))
    for k in range(1, 17):                                 # offset k on the first sequence of each 64-sequence tile, long overlapping copies
        seqs, made = [(16, 5, k + 3)], 21
        for i in range(1, 200):
            s_ = (0, 40, k + 3) if i % 64 == 0 else (2, rng.randint(3, 9), rng.randint(1, min(40, made + 2)) + 3)
            seqs.append(s_); made += s_[0] + s_[1]
        add(f"tile_offset{k}", fam, W.frame([W.comp(W.Lit("raw", txt[:16 + 2 * 196]), W.Seqs(seqs, of=("fse", 6)))]))
    add("longest_ml", fam, W.frame([W.comp(W.Lit("raw", b"m"), W.Seqs([(1, 131071, 1)]))]))
    add("longest_ml_plus", fam, W.frame([W.comp(W.Lit("raw", b"mn"), W.Seqs([(1, 131072, 1)]))]), expect=DST, cap=131072,
        note="131074 bytes from one block: the capacity (128 KiB) stops it")
    add("longest_ll", fam, W.frame([W.comp(W.Lit("rle", b"l" * 131069), W.Seqs([(131069, 3, 1)]))]))
    add("ll_sum_below_litsize", fam, W.frame([W.comp(W.Lit("huf", txt[:400]), W.Seqs([(10, 20, 5 + 3), (7, 9, 1), (100, 4, 30 + 3)]))]))
    add("ll_sum_above_litsize", fam, W.frame([W.comp(W.Lit("huf", txt[:100]), W.Seqs([(60, 20, 5 + 3), (41, 9, 1)]))]), expect=COR, cap=200)
    add("ml_past_capacity", fam, W.frame([W.comp(W.Lit("raw", txt[:100]), W.Seqs([(60, 200, 5 + 3)]))]), expect=DST, cap=259)
    add("last_literals_past_capacity", fam, W.frame([W.comp(W.Lit("raw", txt[:100]), W.Seqs([(60, 20, 5 + 3)]))]), expect=DST, cap=119)

    # ---- several frames in one item
    fam = "frames"
    f1, c1 = W.frame([W.comp(W.Lit("huf", txt[:800], streams=4), W.Seqs(_seq_block(rng, txt[:800], 30)))], checksum=True)
    f2, c2 = W.frame([W.raw(noise[:300]), W.comp(W.Lit("huf", txt[:500]), W.Seqs([(3, 100, 1)]))])
    add("then_empty_skippable", fam, (f1 + W.skippable(b""), c1))
    add("then_skippable", fam, (f1 + W.skippable(b"x" * 100, nibble=15), c1))
    add("skippable_first", fam, (W.skippable(b"abc", nibble=3) + f1, c1))
    add("two_frames", fam, (f1 + f2, c1 + c2))
    add("two_frames_skippable_between", fam, (f1 + W.skippable(b"zz", nibble=7) + f2, c1 + c2))
    add("then_truncated_skippable", fam, (f1 + W.skippable(b"x" * 10, size=11), c1), expect=SRC, cap=len(c1))
    add("then_skippable_header_only", fam, (f1 + W.skippable(b"")[:6], c1), expect=SRC, cap=len(c1))
    add("only_skippable", fam, (W.skippable(b"abc"), b""))
    add("second_frame_bad", fam, (f1 + f2[:-3], c1), expect=SRC, cap=len(c1 + c2))
    return E


def _as_compressed(frame, index):
    """the frame with its raw block number `index` called a compressed block: the same bytes, read as a literals section"""
    b = bytearray(frame)
    blk = list(W.blocks(frame))[index]
    assert blk.type == 0
    b[blk.pos - 3] |= 2 << 1
    return bytes(b)


def _patch_mode_byte(frame, symbol):
    """replace the RLE symbol byte after the compression-modes byte of a frame's only block (raw or RLE literals): the writer does
    not write a code outside the alphabet itself"""
    b = bytearray(frame)
    fhd = frame[4]
    fhs = 5 + (not fhd & 0x20) + [0, 1, 2, 4][fhd & 3] + ([1 if fhd & 0x20 else 0, 2, 4, 8][fhd >> 6])
    p = fhs + 3                                            # block header
    lt, sf = b[p] & 3, (b[p] >> 2) & 3
    if lt == 0:
        sz = b[p] >> 3 if sf in (0, 2) else (int.from_bytes(b[p:p + 2], "little") >> 4 if sf == 1 else int.from_bytes(b[p:p + 3], "little") >> 4)
        p += {0: 1, 2: 1, 1: 2, 3: 3}[sf] + sz
    elif lt == 1:
        p += {0: 1, 2: 1, 1: 2, 3: 3}[sf] + 1
    else:
        raise AssertionError("raw or RLE literals only")
    p += 1 if b[p] < 128 else 2 if b[p] < 255 else 3       # nbSeq
    assert b[p + 1] in (35, 52, 31)
    b[p + 1] = symbol
    return bytes(b)


def _cut_block(frame, k):
    """drop the last k bytes of a one-block, single-segment frame and shrink the block size to match"""
    b = bytearray(frame[:-k])
    fhs = 6
    h = int.from_bytes(b[fhs:fhs + 3], "little")
    h -= k << 3
    b[fhs:fhs + 3] = h.to_bytes(3, "little")
    return bytes(b)
