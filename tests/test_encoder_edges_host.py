"""The encoder edge catalogue (tests/_encoder_edges.py) on the CPU: the frame reader it rests on (_framewriter.section_shapes) against what
the writer side of the same module was told, and every entry's reach as a fact about oracle E's own frames: the predicate at level 3, at
levels 1 and 4 unless the entry is marked level-3-only, a round trip through oracle D and libzstd, the declared-unreachable list and the
caps on what the builder may leave unreached.  The reach table is printed (pytest -s shows it)."""
import functools
import pytest
import _dicts as X
import _encoder_edges as C
import _framewriter as W
import _oracle as O


# ------------------------------------------------------------------------------------------------ the reader against the writer
def _weights(n_symbols, maxbits, top=None):
    """weights of a chain code (lengths 1 .. maxbits, maxbits) over symbols spread up to `top`"""
    top = n_symbols - 1 if top is None else top
    symbols = [i * top // (n_symbols - 1) for i in range(n_symbols)]
    return W.lengths_to_weights(W.chain_lengths(symbols, maxbits))[0], symbols


@pytest.mark.parametrize("streams", [1, 4])
@pytest.mark.parametrize("form", ["4bit", "fse", "fse_given"])
def test_reader_gives_back_the_huffman_description(streams, form):
    weights, symbols = _weights(8, 7, top=255 if form != "4bit" else 100)
    data = bytes(symbols[i % 8] for i in range(301))
    fse = {"4bit": None, "fse": True, "fse_given": ([40, 18, 1, 1, 1, 1, 1, 1], 6)}[form]
    frame, _ = W.frame([W.comp(W.Lit("huf", data, streams=streams, weights=weights, fse=fse))])
    b, = W.section_shapes(frame)
    assert (b.lit_type, b.regen, b.streams, b.nseq, b.nseq_bytes) == (2, 301, streams, 0, 1)
    assert b.huf_weights == weights and b.coded == 8 and b.max_symbol == symbols[-1] and b.max_bits == 7
    assert b.weights == ("4bit" if form == "4bit" else 6)
    assert W.huf_weights(frame, b.huf_pos)[1] + (6 if streams == 4 else 0) < b.seq_pos


def test_reader_gives_back_flat_weights_in_both_forms():
    for n, fse in ((128, None), (129, True), (256, True), (2, None)):      # 127 and 128 weights in the direct form are its last sizes
        data = bytes(range(n)) * 3 if n > 2 else bytes([7, 100]) * 40
        frame, _ = W.frame([W.comp(W.Lit("huf", data, fse=fse))])
        b, = W.section_shapes(frame)
        want = W.lengths_to_weights(W.flat_lengths(set(data)))[0]
        assert b.huf_weights == want and b.coded == n and b.max_symbol == max(data), n
        assert b.max_bits == max(W.flat_lengths(set(data)).values())


@pytest.mark.parametrize("nseq, width", [(1, 1), (127, 1), (128, 2), (0x7EFF, 2), (0x7F00, 3)])
def test_reader_gives_back_the_sequence_count_and_its_width(nseq, width):
    seqs = [(4, 3, 5)] + [(0, 3, 4)] * (nseq - 1)                              # (all codes equal but the first literal length: RLE tables)
    frame, _ = W.frame([W.comp(W.Lit("raw", b"abcd"), W.Seqs(seqs, ll="pre" if nseq < 2 else ("fse", [63, 0, 0, 0, 1], 6),
                                                           of=("rle", 2), ml=("rle", 0)))])
    b, = W.section_shapes(frame)
    assert (b.nseq, b.nseq_bytes) == (nseq, width)
    assert (b.of.mode, b.of.symbol, b.ml.mode, b.ml.symbol) == ("rle", 2, "rle", 0)
    if nseq > 1:
        assert (b.ll.mode, b.ll.al) == ("fse", 6) and b.ll.norm == [63, 0, 0, 0, 1] + [0] * 31


def test_reader_gives_back_every_table_mode():
    seqs = [(1 + i % 20, 3 + i % 40, 4 + i % 5) for i in range(70)]
    codes = {"ll": [W.code_of(W.LL_CODES, s[0])[0] for s in seqs], "ml": [W.code_of(W.ML_CODES, s[1])[0] for s in seqs],
             "of": [s[2].bit_length() - 1 for s in seqs]}
    lits = bytes(sum(s[0] for s in seqs))
    first = W.comp(W.Lit("raw", lits), W.Seqs(seqs, ll=("fse", 7), of=("fse", 5), ml=("fse", 8)))
    second = W.comp(W.Lit("rle", lits), W.Seqs(seqs, ll="rep", of="pre", ml="rep"))
    frame, content = W.frame([first, second])
    a, b = W.section_shapes(frame)
    for name, al, top in (("ll", 7, 35), ("of", 5, 31), ("ml", 8, 52)):
        hist = {}
        for c in codes[name]:                                                  # (in the writer's order: normalize breaks ties by it)
            hist[c] = hist.get(c, 0) + 1
        norm = W.normalize(hist, al)
        t = getattr(a, name)
        assert (t.mode, t.al, t.symbol) == ("fse", al, None) and t.norm == norm + [0] * (top + 1 - len(norm)), name
        assert all((t.norm[c] != 0) == (c in hist) for c in range(top + 1))
    assert [t.mode for t in (b.ll, b.of, b.ml)] == ["repeat", "pre", "repeat"] and (b.lit_type, b.streams, b.huf_weights) == (1, None, None)
    assert a.tables == [7, 5, 8] and O.decompress(frame, len(content)) == content


# ------------------------------------------------------------------------------------------------ the catalogue
@functools.lru_cache(maxsize=None)
def frames(level):
    return C.oracle_frames(C.catalogue()[0], level)


def test_catalogue_is_within_its_caps():
    entries, _ = C.catalogue()
    assert len(entries) <= C.MAX_ENTRIES == 800 and sum(len(e.chunk) for e in entries) <= C.MAX_BYTES == 32 << 20
    assert max(len(e.chunk) for e in entries) <= C.MAX_CHUNK == 131073
    assert {e.family for e in entries} == {"block", "literals", "huffman", "gather", "seqcount", "codes"}
    assert sorted({len(e.chunk) % 4 for e in entries if e.last}) == [1, 2, 3]        # the ungathered path's tails


def test_every_entry_reaches_its_decision_at_level_3(capsys):
    entries, notes = C.catalogue()
    missed = [e.id for e, f in zip(entries, frames(3)) if not e.holds(f)]
    with capsys.disabled():
        print("\nencoder edges: family / name | the decision | oracle E's frame at level 3")
        for e, f in zip(entries, frames(3)):
            print(f"{e.id} | {e.what}{' | level 3 only' * e.level3_only} | {C.describe(C.shapes(f))}")
        print("margins of the compressed-or-raw rule, alpha(n, k):", notes["margins"])
        print("UNREACHED:", C.UNREACHED or "nothing")
    assert not missed, missed
    assert set(notes["margins"]) == {"compressed", "raw"} and notes["margins"]["compressed"][2] in (1, 2)


def test_the_11_bit_cap_binds():
    """a histogram whose Huffman code without a limit is deeper than 11 (worked out here from the chunk's own bytes), no match, and a longest
    code of exactly 11 in the frame"""
    entries, _ = C.catalogue()
    i = [e.id for e in entries].index("huffman/cap11_binding")
    b, = C.shapes(frames(3)[i])
    assert C.huffman_depth(entries[i].chunk) > 11 and (b.nseq, b.lit_type, b.regen, b.max_bits) == (0, 2, len(entries[i].chunk), 11)


@pytest.mark.parametrize("level", [1, 4])
def test_the_decision_holds_at_the_other_levels_or_the_entry_says_not(level):
    entries, _ = C.catalogue()
    missed = [e.id for e, f in zip(entries, frames(level)) if not e.level3_only and not e.holds(f)]
    assert not missed, missed
    # the marks are few outside the sequence-count sweep, whose counts are the LZ stage's and differ from level to level
    assert sum(e.level3_only for e in entries if e.family != "seqcount") <= 8


@pytest.mark.parametrize("level", C.LEVELS)
def test_every_frame_decodes(level):
    for e, f in zip(C.catalogue()[0], frames(level)):
        assert O.decompress_using_dict(f, len(e.chunk), e.dic) == e.chunk, (e.id, "oracle D")
        if X.zstd():
            assert X.zstd_decompress_dict(f, len(e.chunk), e.dic) == e.chunk, (e.id, "libzstd")


@pytest.mark.parametrize("level", C.LEVELS)
def test_declared_unreachable_is_not_reached(level):
    assert len(C.DECLARED_UNREACHABLE) == 5
    for e, f in zip(C.catalogue()[0], frames(level)):
        for b in C.shapes(f):
            for what, reached in C.DECLARED_UNREACHABLE.items():
                assert not reached(b), (e.id, what, C.describe([b]))


def test_unreached_is_within_its_caps():
    entries, _ = C.catalogue()
    reached = {e.name for e in entries if e.family == "seqcount"}
    in_s = [k for k, (s, _) in C.UNREACHED.items() if s]
    assert all(f"nseq{s}" in reached or f"seqcount/nseq{s}" in in_s for s in C.S)
    assert len(in_s) <= len(C.S) // 20, in_s
    assert not {f"seqcount/nseq{s}" for s in (0, 1, 63, 64, 127, 128)} & set(in_s)
    assert len(C.UNREACHED) - len(in_s) <= 3, C.UNREACHED
    names = {e.id for e in entries}
    must = ({f"literals/punched{k}_second_block" for k in (5, 31, 32)} | {f"literals/rawlit{n}" for n in (31, 32, 63, 4095, 4096)}
            | {f"literals/huf{n}" for n in (255, 256, 1023, 1024, 16383, 16384, 65535, 65536)}
            | {"literals/punched4_second_block", "literals/huf64_with_sequence", "huffman/cap11_binding"})
    assert must <= names and not must & set(C.UNREACHED)
