"""Oracle D (oracle/zso_decoder.c) on the hand-built edge catalogue (tests/_edge_catalogue.py, written by tests/_framewriter.py).
Valid frames decode to the writer's content; invalid ones fail with the error code pinned in the catalogue.  Where libzstd is on the
machine it decodes the valid frames to the same content and rejects the invalid ones, except at the places listed in
REFERENCE_DIFFERS_FROM_UPSTREAM.  CPU only."""
import ctypes, time
import numpy as np
import pytest
import _oracle as O
import _edge_catalogue as C
import _framewriter as W

FAMILIES = ["header", "checksum", "blocks", "literals", "sequences", "offsets", "frames"]

# frames on which the reference (and so oracle D) and upstream libzstd 1.4.8 part ways.  Each is a property of the reference, restated
# by the oracle on purpose; the HIP decoder follows the reference.
REFERENCE_DIFFERS_FROM_UPSTREAM = {
    # the reference is built for a 32-bit size_t: ZSTD_WINDOWLOG_MAX = ZSTD_WINDOWLOG_MAX_32 = 30 (csharp/src/ZStd.cs:390-392), checked at
    # csharp/src/ZStdDecompress.cs:468 -> frameParameter_windowTooLarge; 64-bit libzstd allows 31
    "header/nofcs_windowlog31",
    # an nbSeq of 0 returns at once (csharp/src/ZStdDecompress.cs:1122) and nothing checks the bytes after it; libzstd 1.4.8 asks
    # that the sequences section be exactly one byte then (srcSize_wrong)
    "sequences/nbseq0_trailing",
}


def _run(e):
    try:
        return O.decompress(e.frame, e.cap), None
    except O.OracleError as x:
        return None, x.code


def test_catalogue_is_deterministic_and_quick():
    C.catalogue.cache_clear()
    t = time.perf_counter()
    a = C.catalogue()
    dt = time.perf_counter() - t
    C.catalogue.cache_clear()
    b = C.catalogue()
    assert [(e.id, e.frame) for e in a] == [(e.id, e.frame) for e in b]
    assert len({e.id for e in a}) == len(a), "entry names must be unique"
    assert sorted({e.family for e in a}) == sorted(FAMILIES)
    assert len(a) >= 200
    assert dt < 15, f"catalogue generation took {dt:.1f} s"


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_on_edge_family(family):
    entries = [e for e in C.catalogue() if e.family == family]
    assert entries
    bad = []
    for e in entries:
        out, code = _run(e)
        if e.expect == "ok":
            if out != e.content:
                bad.append((e.id, "error %s" % code if code else "wrong bytes"))
        elif code != e.expect:
            bad.append((e.id, f"expected error {e.expect}, got {code if code else 'success'}"))
    assert not bad, bad
    assert any(e.expect == "ok" for e in entries) and any(e.expect != "ok" for e in entries)


@pytest.mark.parametrize("family", FAMILIES)
def test_libzstd_on_edge_family(family):
    if not O.libzstd():
        pytest.skip("libzstd is not on this machine")
    disagree = []
    for e in C.catalogue():
        if e.family != family:
            continue
        z = O.zstd_decompress(e.frame, e.cap)
        agrees = (z == e.content) if e.expect == "ok" else (z is None)
        if agrees == (e.id in REFERENCE_DIFFERS_FROM_UPSTREAM):
            disagree.append(e.id)
    assert not disagree, ("oracle D and libzstd part ways (a writer bug, or a reference difference to list)", disagree)


def test_writer_checksum_is_xxh64():
    L = O.lib()
    for n in (0, 1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 65, 1000):
        d = bytes((i * 37 + 11) & 0xFF for i in range(n))
        assert W.xxh64(d) == L.zso_xxh64(d, n, 0), n


def test_edge_catalogue_coverage():
    """the catalogue reaches what it claims (oracle D's construct counters, as test_fixture_coverage)"""
    L = O.lib()
    L.zso_statsGet40.argtypes = [ctypes.c_void_p]
    tot = np.zeros(40, dtype=np.uint64)
    for e in C.catalogue():
        if e.expect != "ok":
            continue
        L.zso_statsReset()
        assert O.decompress(e.frame, e.cap) == e.content
        st = np.zeros(40, dtype=np.uint32)
        L.zso_statsGet40(st.ctypes.data_as(ctypes.c_void_p))
        tot += st
    must = {0: "raw literals", 1: "rle literals", 2: "huffman literals", 3: "treeless literals", 4: "1-stream", 5: "4-stream",
            8: "LL predefined", 9: "LL rle", 10: "LL fse", 11: "LL repeat", 12: "OF predefined", 13: "OF rle", 14: "OF fse",
            15: "OF repeat", 16: "ML predefined", 17: "ML rle", 18: "ML fse", 19: "ML repeat", 20: "raw block", 21: "rle block",
            22: "compressed block", 25: "checksum", 26: "nbSeq==0", 27: ">= 0x7F00 sequences", 28: "repcode", 29: "multi-block",
            34: "double-symbol (X4) Huffman decoder"}
    missing = [v for k, v in must.items() if tot[k] == 0]
    assert not missing, missing
    assert tot[5] > tot[34] > 0, "both Huffman decoders: some 4-stream sections by the single-symbol one too"
    assert tot[27] >= 4 and tot[30] > 190000                  # sequences decoded


def test_writer_hits_its_size_formats():
    """the header forms the catalogue claims: every FCS field size, 1/2/3-byte raw and RLE headers, 10/14/18-bit Huffman sizes,
    1/2/3-byte nbSeq"""
    cat = {e.id: e.frame for e in C.catalogue()}
    fcs_flags = {f[4] >> 6 for f in cat.values() if f[:4] == b"\x28\xb5\x2f\xfd"}
    assert fcs_flags == {0, 1, 2, 3}
    def lit_sf(f):                                        # size format of the first block's literals section
        fhd = f[4]
        fhs = 5 + (not fhd & 0x20) + [0, 1, 2, 4][fhd & 3] + [1 if fhd & 0x20 else 0, 2, 4, 8][fhd >> 6]
        return (f[fhs + 3] >> 2) & 3
    assert [lit_sf(cat[f"literals/huf4s_{n}"]) for n in (1023, 1024, 16383, 16384)] == [1, 2, 2, 3]
    hdr_bytes = {0: 1, 2: 1, 1: 2, 3: 3}                    # raw / RLE: formats 0 and 2 are the 1-byte header
    assert [hdr_bytes[lit_sf(cat[f"literals/raw{n}"])] for n in (31, 32, 4095, 4096)] == [1, 2, 2, 3]
    assert [hdr_bytes[lit_sf(cat[f"literals/rle5_sf{k}"])] for k in (0, 1, 3)] == [1, 2, 3]
