"""Hand-built dictionaries and dictionary frames for the digested decode dictionaries (zsmi_createDDict; tests/test_ddict_frames_host.py pins
them under oracle D on the CPU, tests/test_gpu_ddict.py decodes them on the GPU).  The frames are written with tests/_framewriter.py, whose
state starts from the dictionary here: its content in front of the frame, its recent offsets, its Huffman codes and its three FSE tables
(ZSTD_decompress_insertDictionary).  Every case is (name, dictionary name, frame, content or None, error code or 0)."""
import struct
import _framewriter as W

MAGIC_DICT = 0xEC30A437
DICT_ID = 77
ALPHABET = b"abcdefgh"
# the entropy tables every small dictionary carries: offset codes 0 - 9, match length codes 0 - 31, literal length codes 0 - 31
OF_NORM, ML_NORM, LL_NORM = ([4, 4, 4, 4, 4, 4, 2, 2, 2, 2], 5), ([2] * 32, 6), ([2] * 32, 6)
CONTENT = b"abcdefgh" * 12 + bytes(range(48, 112)) + b"hgfedcba" * 12 + b"The quick brown fox jumps over the lazy dog. " * 2 + b"0123456789"


def formatted(weights, reps=(1, 4, 8), content=CONTENT, dict_id=DICT_ID, fse=None):
    """a formatted dictionary: magic, ID, Huffman description of `weights`, the OF / ML / LL counts above, recent offsets, content"""
    return struct.pack("<II", MAGIC_DICT, dict_id) + W.huf_description(weights, fse) + W.ncount(*OF_NORM) + W.ncount(*ML_NORM) + W.ncount(*LL_NORM) + \
        b"".join(r.to_bytes(4, "little") for r in reps) + content


def narrow_weights():
    """a Huffman table over 'a'..'h', 3 bits each"""
    return W.lengths_to_weights(W.flat_lengths(ALPHABET))[0]


def wide_lengths():
    """195 symbols, longest code 11 bits: three short codes (1/2, 1/4, 1/8 of the code space), 64 codes of 10 bits and 128 of 11 bits - 64
    nine-bit prefixes hold longer codes, more than the two-level table's 32 sub-tables: the flat table class"""
    lengths = {0: 1, 1: 2, 2: 3}
    lengths.update({3 + i: 10 for i in range(64)})
    lengths.update({67 + i: 11 for i in range(128)})
    return lengths


def long_prefixes(lengths):
    """nine-bit prefixes under which codes of more than nine bits sit (ZS_HUF2_SUBS = 32 of them fit the two-level table)"""
    codes, _ = W.huf_codes(W.lengths_to_weights(lengths)[0])
    return len({c >> (nb - 9) for c, nb in codes.values() if nb > 9})


def log12_lengths():
    """14 symbols, longest code 12 bits (no weight above 11): a table the fast path does not hold"""
    lengths = {0: 2, 1: 2, 2: 2}
    lengths.update({3 + i: 3 + i for i in range(10)})
    lengths[13] = 12
    return lengths


_dicts = {}


def dictionaries():
    """name -> dictionary: narrow (recent offsets 1, 4, 8), reps (7, 33, 120), wide (flat Huffman class), log12 (Huffman log 12), raw (content only)"""
    if not _dicts:
        _dicts["narrow"] = formatted(narrow_weights())
        _dicts["reps"] = formatted(narrow_weights(), reps=(7, 33, 120))
        _dicts["wide"] = formatted(W.lengths_to_weights(wide_lengths())[0], fse=True)
        _dicts["log12"] = formatted(W.lengths_to_weights(log12_lengths())[0])
        _dicts["raw"] = CONTENT
    return _dicts


def parts(dic):
    """(content, recent offsets, Huffman weights or None) of one of the dictionaries above"""
    if dic[:4] != struct.pack("<I", MAGIC_DICT):
        return dic, (1, 4, 8), None
    at = len(dic) - len(CONTENT) - 12
    reps = struct.unpack_from("<III", dic, at)
    name = next(k for k, v in dictionaries().items() if v == dic)
    weights = {"narrow": narrow_weights, "reps": narrow_weights, "wide": lambda: W.lengths_to_weights(wide_lengths())[0],
               "log12": lambda: W.lengths_to_weights(log12_lengths())[0]}[name]()
    return dic[at + 12:], reps, weights


def frame(blocks, dic, dict_id=None, dict_bytes=None, checksum=False, bad_checksum=False, fcs="auto"):
    """(frame bytes, content or None) of a single-segment frame written against the dictionary: W.frame with the writer's state started from it"""
    content, reps, weights = parts(dic)
    st = W._State()
    st.out = bytearray(content); st.rep = list(reps)
    if weights is not None:
        st.huf = W.huf_codes(weights)[0]
        st.tables = {"ll": W.FSE(*LL_NORM), "of": W.FSE(*OF_NORM), "ml": W.FSE(*ML_NORM)}
    body = b"".join(W._block(b, st, i == len(blocks) - 1) for i, b in enumerate(blocks))
    out = bytes(st.out[len(content):])
    n = len(out)
    fcs_v = n if fcs == "auto" else fcs
    fcs_bytes = 1 if fcs_v < 256 else 2 if fcs_v < 65792 else 4
    if dict_bytes is None:
        dict_bytes = 0 if dict_id is None else 1 if dict_id < 256 else 2 if dict_id < 65536 else 4
    fhd = ({1: 0, 2: 1, 4: 2}[fcs_bytes] << 6) | (1 << 5) | (int(checksum) << 2) | {0: 0, 1: 1, 2: 2, 4: 3}[dict_bytes]
    hdr = struct.pack("<I", W.MAGIC) + bytes([fhd])
    if dict_bytes:
        hdr += (dict_id or 0).to_bytes(dict_bytes, "little")
    hdr += (fcs_v - 256 if fcs_bytes == 2 else fcs_v).to_bytes(fcs_bytes, "little")
    tail = struct.pack("<I", (W.xxh64(out) & 0xFFFFFFFF) ^ (0x5A5A5A5A if bad_checksum else 0)) if checksum else b""
    return hdr + body + tail, (out if st.ok else None)


def text(k, seed=1, alphabet=ALPHABET):
    """k bytes over the alphabet, from a small generator (no two runs alike: nothing for a match finder, plenty for Huffman)"""
    x, out = seed * 2654435761 & 0xFFFFFFFF, bytearray()
    for _ in range(k):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append(alphabet[(x >> 16) % len(alphabet)])
    return bytes(out)


_cases = []


def cases():
    """[(name, dictionary name, frame, content or None, error code)]: the frames (a) - (l) of the edge catalogue; the letter leads the name"""
    if _cases:
        return _cases
    Lit, Seqs, comp, raw, rle = W.Lit, W.Seqs, W.comp, W.raw, W.rle
    C = len(CONTENT)
    D = dictionaries()

    def add(name, dname, blocks, code=0, **kw):
        f, content = frame(blocks, D[dname], **kw)
        assert (content is None) == (code == 20), name
        _cases.append((name, dname, f, None if code else content, code))

    lits = text(40, 3)
    for dname in ("narrow", "raw"):
        # (a) the first sequence: no literals, a match wholly inside the dictionary
        add(f"a first sequence ll 0 in the dictionary [{dname}]", dname, [comp(Lit("raw", lits), Seqs([(0, 8, 50 + 3), (5, 4, 2 + 3)]))])
        add(f"a long match wholly in the dictionary [{dname}]", dname, [comp(Lit("raw", lits), Seqs([(0, 70, 200 + 3), (9, 33, 150 + 9 + 70 + 3)]))])
        # (b) from the dictionary over its end into the output: the continuation reads literals; reads what the same match wrote
        add(f"b match over the content's end [{dname}]", dname, [comp(Lit("raw", lits), Seqs([(30, 25, 30 + 10 + 3)]))])
        add(f"b match over the content's end, overlapping [{dname}]", dname, [comp(Lit("raw", lits), Seqs([(5, 25, 5 + 10 + 3), (3, 60, 33 + 40 + 3)]))])
        add(f"b long match over the content's end, overlapping [{dname}]", dname, [comp(Lit("raw", lits), Seqs([(2, 300, 2 + 50 + 3)]))])
        # (c) the farthest legal offset, and one further
        add(f"c offset of position + content size [{dname}]", dname, [comp(Lit("raw", lits), Seqs([(4, 9, 4 + C + 3)]))])
        add(f"c offset past the content's first byte [{dname}]", dname, [comp(Lit("raw", lits), Seqs([(4, 9, 4 + C + 1 + 3)]))], code=20)
    # (d) the first sequence is a repeat code, against the default list and another one
    for dname in ("narrow", "reps", "raw"):
        for ov in (1, 2, 3):
            for ll in (0, 3):
                add(f"d repeat code {ov} ll {ll} [{dname}]", dname, [comp(Lit("raw", lits), Seqs([(ll, 6, ov), (2, 5, 1), (0, 4, 3)]))])
    tl = text(64, 5)
    for dname in ("narrow", "reps"):
        # (e) Treeless literals in the first block
        add(f"e treeless 1 stream [{dname}]", dname, [comp(Lit("treeless", tl, streams=1), Seqs([(10, 8, 20 + 3)]))])
        add(f"e treeless 4 streams [{dname}]", dname, [comp(Lit("treeless", tl + text(200, 6), streams=4), Seqs([(10, 8, 20 + 3)]))])
        add(f"e treeless, no sequences [{dname}]", dname, [comp(Lit("treeless", tl, streams=1))])
        # (f) Repeat_Mode in the first block: each table alone, all three
        sq = [(3, 5, 40 + 3), (0, 7, 2), (12, 20, 300 + 3), (1, 3, 1)]
        for modes in ({"ll": "rep"}, {"of": "rep"}, {"ml": "rep"}, {"ll": "rep", "of": "rep", "ml": "rep"}):
            add(f"f repeat mode {'+'.join(sorted(modes))} [{dname}]", dname, [comp(Lit("raw", lits), Seqs(sq, **modes))])
        add(f"f repeat mode all, treeless [{dname}]", dname, [comp(Lit("treeless", tl, streams=1), Seqs(sq, ll="rep", of="rep", ml="rep"))])
        # (g) two blocks: the second repeats the first's own tables (not the dictionary's) and reaches into the dictionary
        own = Lit("huf", text(80, 7, b"abcdwxyz"))
        add(f"g second block repeats block 1's tables: own Huffman, LL of the dictionary [{dname}]", dname,
            [comp(own, Seqs(sq, ll="rep", of=("fse", 6), ml=("fse", 6))),
             comp(Lit("treeless", text(50, 8, b"abcdwxyz")), Seqs([(3, 5, 300 + 3), (1, 3, 1)], ll="rep", of="rep", ml="rep"))])      # (block 1's tables hold block 1's codes only)
        add(f"g second block repeats block 1's tables: Huffman of the dictionary, own sequence tables [{dname}]", dname,
            [comp(Lit("treeless", tl), Seqs(sq, ll=("fse", 6), of=("fse", 6), ml=("fse", 6))),
             comp(Lit("treeless", text(50, 9)), Seqs(sq, ll="rep", of="rep", ml="rep"))])
        # (h) a raw or RLE first block: the dictionary's Huffman table is still the current one
        add(f"h raw block, then treeless [{dname}]", dname, [raw(b"first block, raw"), comp(Lit("treeless", tl), Seqs(sq, ll="rep", of="rep", ml="rep"))])
        add(f"h RLE block, then treeless [{dname}]", dname, [rle(0x2E, 37), comp(Lit("treeless", tl), Seqs([(10, 8, 37 + 10 + 60 + 3)]))])
        # (i) content checksum
        add(f"i checksum [{dname}]", dname, [comp(Lit("treeless", tl), Seqs(sq, ll="rep", of="rep", ml="rep"))], checksum=True)
        add(f"i wrong checksum [{dname}]", dname, [comp(Lit("treeless", tl), Seqs(sq, ll="rep", of="rep", ml="rep"))], checksum=True, bad_checksum=True, code=22)
    # (j) frame header variants
    one = [comp(Lit("treeless", tl), Seqs([(0, 8, 50 + 3)], ll="rep", of="rep", ml="rep"))]
    for nbytes in (1, 2, 4):
        add(f"j dictionary ID in {nbytes} bytes", "narrow", one, dict_id=DICT_ID, dict_bytes=nbytes)
        add(f"j another ID in {nbytes} bytes", "narrow", one, dict_id=DICT_ID + 1, dict_bytes=nbytes, code=32)
    add("j ID field of 0", "narrow", one, dict_id=0, dict_bytes=1)
    add("j no ID field", "narrow", one)
    add("j an ID with raw content", "raw", [comp(Lit("raw", lits), Seqs([(0, 8, 50 + 3)]))], dict_id=DICT_ID, code=32)
    # (k) a dictionary whose Huffman table takes the flat class
    wl = text(300, 11, bytes(range(195)))
    add("k treeless with a flat-class table, 1 stream", "wide", [comp(Lit("treeless", wl[:60], streams=1), Seqs([(10, 8, 20 + 3)], ll="rep", of="rep", ml="rep"))])
    add("k treeless with a flat-class table, 4 streams", "wide", [comp(Lit("treeless", wl, streams=4), Seqs([(10, 8, 20 + 3)]))])
    # a Huffman table of 2^12: the frame may leave the fast path
    add("m treeless with a table of 12 bits", "log12", [comp(Lit("treeless", text(90, 12, bytes(range(14)))), Seqs([(10, 8, 20 + 3)], ll="rep", of="rep", ml="rep"))])
    add("m no treeless, dictionary with a table of 12 bits", "log12", [comp(Lit("raw", lits), Seqs([(0, 8, 50 + 3)], ll="rep", of="rep", ml="rep"))])
    # (l) frames of 0 bytes and 1 byte
    for dname in ("narrow", "raw"):
        add(f"l empty frame [{dname}]", dname, [raw(b"")])
        add(f"l one byte, raw block [{dname}]", dname, [raw(b"x")])
        add(f"l one byte, compressed block [{dname}]", dname, [comp(Lit("raw", b"y"))])
        add(f"l one byte, RLE block [{dname}]", dname, [rle(0x41, 1)])
    return _cases


def may_fall_back(name):
    """the only frames that may leave the fast path: a Treeless first block whose dictionary holds a Huffman table of more than 11 bits"""
    return name.startswith("m treeless")


# ------------------------------------------------------------------ decoding with a digested dictionary (GPU)
def decode_many(codec, frames, caps, ddict, min_cap=0):
    """_batch.decode_many through a DecompressionDict (zsmi_decompressBatchHost_usingDDict) -> [(size or error word, bytes)]"""
    import numpy as np
    import _batch as B
    src, offs, sizes = B.batch(frames)
    out, oo, osz = codec.decompress_host(src, offs, sizes, np.maximum(np.array(caps, dtype=np.uint32), min_cap), ddict=ddict)
    return [(int(s), out[int(o):int(o) + (int(s) if s < B.ERR else 0)].tobytes()) for o, s in zip(oo, osz)]


def oracle_many(frames, caps, dic):
    """oracle D item by item, in the library's words: (size, bytes) or (the error word, b"")"""
    import _oracle as O
    out = []
    for f, cap in zip(frames, caps):
        try:
            got = O.decompress_using_dict(f, cap, dic) if dic else O.decompress(f, cap)
            out.append((len(got), got))
        except O.OracleError as e:
            out.append((0x100000000 - e.code, b""))
    return out


def cases_of(dname, short_cap=512, two_block_cap=65537):
    """(names, frames, capacities) of the catalogue's frames for one dictionary: a valid frame gets its content's size, an invalid one short_cap.
    A valid frame of more than one block gets two_block_cap: a call reserves block slots by its capacities (one slot while no item can hold
    more than one 64 KiB block), so 64 KiB + 1 is the smallest capacity at which a two-block frame can stay on the fast path, with or
    without a dictionary"""
    mine = [c for c in cases() if c[1] == dname]
    caps = [short_cap if c[4] else (two_block_cap if len(list(W.blocks(c[2]))) > 1 else len(c[3])) for c in mine]
    return [c[0] for c in mine], [c[2] for c in mine], caps
