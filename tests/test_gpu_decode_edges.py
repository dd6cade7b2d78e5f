"""The HIP decoder on the hand-built edge catalogue (tests/_edge_catalogue.py), in several placements.  In each, every item's status must
equal oracle D's at the same capacity: the same bytes, or the same error code ((1 << 32) - code).  Plus output bounds on the device
API: no byte outside an item's [dstOffset, dstOffset + dstCap) changes, for decode, and outside [dstOffset, + compressBound) for encode."""
import json, os
import pytest
import _oracle as O
import _edge_catalogue as C
import _framewriter as W
import _data as D
import _batch as B
from _batch import ROOT

pytestmark = pytest.mark.gpu
MIB = 1 << 20


def _want(frame, cap):
    """oracle D at this capacity: bytes, or the status word the batch API writes for an error"""
    try:
        return O.decompress(frame, cap)
    except O.OracleError as e:
        return (1 << 32) - e.code


@pytest.fixture(scope="module")
def bc():
    from zstandard_amd import BatchCodec
    b = BatchCodec(0)
    yield b
    b.close()


def _batch(bc, items):
    """items: [(frame, cap)] -> [bytes or status word] from one decompress_host call"""
    return [sz if sz > B.ERR else got for sz, got in B.decode_many(bc, [f for f, _ in items], [c for _, c in items], min_cap=0)]


def _check(names, items, got):
    bad = []
    for name, (f, cap), g in zip(names, items, got):
        w = _want(f, cap)
        if g != w:
            bad.append((name, cap, "error %d" % ((1 << 32) - g) if isinstance(g, int) else "%d bytes" % len(g),
                        "oracle: error %d" % ((1 << 32) - w) if isinstance(w, int) else "oracle: %d bytes" % len(w)))
    assert not bad, bad[:20]


def test_edges_exact_capacity(bc):
    """(a) one batch, capacities exact"""
    cat = C.catalogue()
    items = [(e.frame, e.cap) for e in cat]
    _check([e.id for e in cat], items, _batch(bc, items))


def test_edges_generous_capacity(bc):
    """(b) 1 MiB each: other blockCap / seqCap / block slots, so other frames take the fast path"""
    cat = C.catalogue()
    items = [(e.frame, MIB) for e in cat]
    _check([e.id for e in cat], items, _batch(bc, items))


def test_edges_followed_by_skippable(bc):
    """(c) each frame and an empty skippable frame in one item (several frames: the general kernel)"""
    cat = C.catalogue()
    items = [(e.frame + W.skippable(b""), e.cap) for e in cat]
    _check([e.id for e in cat], items, _batch(bc, items))


def test_edges_one_byte_short_among_valid_neighbours(bc):
    """(d) capacity one byte short, with and without FCS, each between two valid items of the same call"""
    cat = C.catalogue()
    short = [e for e in cat if e.expect == "ok" and len(e.content) > 0]
    txt = D.zipf_log(1 << 20).tobytes()
    names, items = [], []
    for i, e in enumerate(short):
        c = txt[i * 997:i * 997 + 2000 + 300 * (i % 7)]
        nf, _ = W.frame([W.comp(W.Lit("huf", c[:1000], streams=4)), W.raw(c[1000:])], fcs=None if i % 2 else "auto",
                        single=not i % 2 == 1, window=(10, 0))
        names += [f"neighbour{i}", e.id, f"neighbour{i}b"]
        items += [(nf, len(c)), (e.frame, len(e.content) - 1), (O.compress(c[::-1], 3), len(c))]
    got = _batch(bc, items)
    _check(names, items, got)
    assert all(isinstance(got[k], int) for k in range(1, len(items), 3)), "one byte short must fail"


def test_edges_second_call_other_order(bc):
    """(e) a second call on the same context, other order: the repeat-mode-first-block frames right after items that had valid FSE and
    Huffman tables, so stale slot contents would show"""
    cat = C.catalogue()
    _batch(bc, [(e.frame, e.cap) for e in cat])
    with_tables = [e for e in cat if e.expect == "ok" and e.family == "sequences" and "fse" in e.name]
    stale = [e for e in cat if e.name.endswith(("_rep_first", "_rep_after_nbseq0")) or e.name in ("treeless_first", "treeless_after_raw_only")]
    assert len(stale) >= 8 and with_tables
    order = []
    for i, e in enumerate(stale):
        order += [with_tables[i % len(with_tables)], e]
    rest = [e for e in reversed(cat) if e not in order]
    order += rest
    items = [(e.frame, e.cap) for e in order]
    _check([e.id for e in order], items, _batch(bc, items))


def test_edges_one_shot_apis_keep_outside_bytes():
    """(f) ZStdDecompress.Decompress and ZstdDecompressor.decompress(..., outputOffset, maxOutputLength): bytes of the output array
    outside [outputOffset, outputOffset + maxOutputLength) stay as they were"""
    from zstandard_amd import ZStdDecompress, ZstdDecompressor
    cat = {e.id: e for e in C.catalogue()}
    pick = ["literals/huf4s_6", "sequences/nbseq0x7f00", "offsets/tile_offset3", "checksum/n33_ok", "checksum/n33_bad",
            "sequences/of_rep_first", "offsets/longest_ml", "frames/two_frames", "header/fcs2_65791_window", "offsets/ml_past_capacity"]
    jd = ZstdDecompressor()
    for name in pick:
        e = cat[name]
        w = _want(e.frame, e.cap)
        r = ZStdDecompress.Decompress(bytearray(e.cap), e.frame)
        assert r == (w if isinstance(w, int) else len(w)), name
        off, pad = 37, 101
        arr = bytearray(b"\xa5" * (off + e.cap + pad))
        try:
            n = jd.decompress(e.frame, 0, len(e.frame), arr, off, e.cap)
            assert not isinstance(w, int) and n == len(w) and bytes(arr[off:off + n]) == w, name
        except RuntimeError:
            assert isinstance(w, int), name
        assert arr[:off] == b"\xa5" * off and arr[off + e.cap:] == b"\xa5" * pad, name
        dst = bytearray(b"\x5a" * (e.cap + pad))
        r = ZStdDecompress.Decompress(dst, e.frame, e.cap)
        assert dst[e.cap:] == b"\x5a" * pad, name


# ---------------------------------------------------------------- output bounds on the device API
def test_device_api_stays_inside_each_item(capsys):
    """decompress_device / compress_device on torch buffers filled with a canary, items with gaps and tightly packed: no byte outside
    an item's region changes (tools/bounds_edges.py, a process of its own: torch has to be loaded before libzsmi.so)"""
    rep = json.loads(B.run_child(os.path.join(ROOT, "tools", "bounds_edges.py"), cwd=ROOT, marker=None).strip().splitlines()[-1])
    assert rep["decode_items"] >= 7 * 200 and rep["compress_items"] >= 24
    with capsys.disabled():
        print(f"\n[device bounds] decoded items whose bytes between the produced size and dstCap were touched: {rep['tail_touched']}, "
              f"untouched: {rep['tail_kept']}")


# ---------------------------------------------------------------- which path ran
# entries the decoder's fast path is meant to take, in placement (a) exact capacities or (b) 1 MiB capacities
FAST_EXPECTED = {
    "a": ["literals/huf4s_6", "literals/huf4s_7", "literals/huf4s_8", "checksum/n1000_ok", "checksum/n64_ok", "checksum/n65_ok",
          "literals/treeless_second", "sequences/ll_rep_second", "sequences/of_rep_second", "sequences/ml_rep_second",
          "sequences/all_rep_second", "header/fcs1_255_single", "header/fcs2_256_single", "header/fcs4_65792_single",
          "header/fcs8_1000_single", "header/fcs2_256_window", "header/fcs4_5000_window", "header/fcs8_5000_window",
          "header/fcs1_0_single", "header/nofcs_windowlog10", "header/nofcs_windowlog30", "literals/maxbits11_4s", "literals/alphabet_256_4s",
          "literals/alphabet_top255_1s_fse", "sequences/ll_rle35", "sequences/ml_rle52", "offsets/rep3_ll0", "offsets/rep0_minus1_is_zero"],
    # (a block of more than ZS_FAST_MAXSEQ = 16384 sequences, e.g. sequences/nbseq0x7f00, is the general kernel's by design)
    "b": ["literals/huf4s_6", "blocks/blocks16_x64k", "blocks/blocks16_x1k", "literals/treeless_after_raw", "sequences/ll_rep_after_raw_block",
          "sequences/of_rep_after_raw_block", "sequences/ml_rep_after_raw_block", "header/nofcs_windowlog30", "blocks/raw131072",
          "offsets/longest_ml", "offsets/longest_ll", "offsets/tile_offset1", "offsets/tile_offset16"],
}


def test_edge_shapes_stay_on_the_fast_path():
    """a child process with the debug library (tools/fastpath_edges.py) reads back each item's fast-path descriptor"""
    env = dict(os.environ, ZSMI_DEBUG_LIB="1")
    res = json.loads(B.run_child(os.path.join(ROOT, "tools", "fastpath_edges.py"), env=env, cwd=ROOT, marker=None).strip().splitlines()[-1])
    for placement, names in FAST_EXPECTED.items():
        slow = [n for n in names if res[placement].get(n) != 1]
        assert not slow, (placement, slow)
