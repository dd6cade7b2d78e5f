"""The inputs of tests/test_gpu_borders.py, checked on the host (no GPU): the borders they are built on are still the constants of the
source text; the index streams have the entries they were built to have, with every aimed offset hit; oracle D alone rejects enough of the
damaged frames of the 66 000 and accepts every other; the long chunk of the 16 500 straddles block 16 384; the running sums of the uneven
batch differ at every border."""
import numpy as np
import pytest
import _batch as B
import _borders as BD
import _frames_index as F


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    _lib.build()
    return _lib.lib()


def test_borders_are_the_constants_of_the_source():
    got = BD.source_constants()
    want = {name: getattr(BD, name) for name in got}
    assert got == want, "a tile or a limit was retuned: move the cases of tests/_borders.py to its new border"
    assert BD.SCAN_LEVEL == 2097152 and BD.TINY_N == (1024, 1025, 2049) and BD.CUT_AT == 16383 and BD.DECODE_BORDER == (65535, 65536, 65537)
    assert BD.INDEX_TILE == 4 * BD.INDEX_STEP == 4 * 256 * BD.INDEX_LANE           # 4 steps x 256 threads x 16 bytes


# ------------------------------------------------------------------ A
def test_tiny_chunks_hold_what_they_are_for():
    for n in BD.TINY_N:
        chunks = BD.tiny_chunks(n)
        sizes = [len(c) for c in chunks]
        assert len(chunks) == n and max(sizes) == 400 and sizes.count(0) >= 3
        above = [s > BD.TOLD for s in sizes]
        assert 0 < sum(above) < n
        for border in range(BD.PLAN_TILE, n, BD.PLAN_TILE):                          # the last thread of a tile, the first of the next
            for i in (border - 1, border):
                assert sizes[i] == 0 or above[i], (n, i)
            assert any(c == bytes(len(c)) and len(c) for c in chunks[border - 2:border + 3]), (n, border, "zeros")


def test_uneven_batch_differs_at_every_border():
    sizes = BD.uneven_sizes()
    K, T = BD.UNEVEN_K, BD.PLAN_TILE
    assert BD.counts(BD.UNEVEN_MAX)[0] == 4 and K == 1100 and T < K < 2 * T and len(sizes) == 2500          # a tile of 1024 and one of 76
    assert [BD.counts(s) for s in BD.LONG] == [(1, 1, 0), (2, 0, 1), (2, 0, 1), (3, 1, 1), (4, 0, 2)]
    assert 40 <= sum(s > 65535 for s in sizes) <= 60 and sum(sizes) < 7 << 20
    totals = []
    for c0 in range(0, len(sizes), K):
        cc = np.array([BD.counts(s) for s in sizes[c0:c0 + K]])
        run = np.concatenate([[[0, 0, 0]], np.cumsum(cc, axis=0)])
        if len(cc) > T:                                                              # the sums k_plan_chunks carries into its second tile
            b, s, g = (int(v) for v in run[T])
            assert len({b, s, g, T}) == 4 and min(b, s, g) > 0, (c0, b, s, g)
            assert cc[T - 1][0] > 1 and cc[T][0] > 1, "a long chunk on both sides of the tile border"
        totals.append(tuple(int(v) for v in run[-1]))
        assert len(set(totals[-1])) == 3
    assert len(set(totals)) == 3
    assert BD.counts(sizes[K - 1])[0] > 1 and BD.counts(sizes[K])[0] > 1             # ... and of the sub-batch border
    items = BD.with_choices(BD.uneven_chunks())
    for border in (T, K, K + T):
        assert {ch for _, ch in items[border - 2:border + 3]} == set(BD.CYCLE)
    assert [len(c) for c, _ in items] == sizes


def test_records_hold_what_they_are_for():
    parts, index = BD.records()
    assert len(parts) == 3000 > 2 * BD.PLAN_TILE and min(map(len, parts)) == 1 and max(map(len, parts)) == 300
    assert set(index.tolist()) == {0, 1, 2, BD.NO_DICT}


# ------------------------------------------------------------------ C
def test_long_chunk_straddles_the_default_blocks_in_flight():
    chunks = BD.cut_chunks()
    blocks = [BD.counts(len(c))[0] for c in chunks]
    first = sum(blocks[:BD.CUT_AT])
    assert len(chunks) == 16500 and blocks[BD.CUT_AT] == 3 and blocks.count(1) == len(chunks) - 1
    # its blocks are 16 383, 16 384 and 16 385: the first would fit the sub-batch of 16 384, the chunk does not - the cut falls in front of it
    assert first == BD.BLOCKS_IN_FLIGHT - 1 and first < BD.BLOCKS_IN_FLIGHT < first + blocks[BD.CUT_AT]
    assert sum(blocks) - first <= BD.BLOCKS_IN_FLIGHT                                # ... and the rest is one more sub-batch
    assert 64 <= min(map(len, chunks)) and sorted(map(len, chunks))[-2] <= 700


def test_oracle_d_on_the_66000_frames():
    items, contents, want = BD.decode_items()
    assert len(items) == 66000 > BD.ITEMS_IN_FLIGHT and 20 <= min(map(len, contents)) and max(map(len, contents)) <= 120
    BD.assert_decode_condition(items, contents, want)
    a, b, c = BD.DECODE_BORDER
    assert want[b] == (len(contents[b]), contents[b]) and items[b].endswith(b"behind the frame") and want[c][0] == len(contents[c])
    kinds = {(i & 1, bool(i & 2)) for i, (sz, _) in enumerate(want) if sz >= B.ERR}
    assert len(kinds) >= 2, "rejected frames of more than one make"


# ------------------------------------------------------------------ D
@pytest.mark.parametrize("name", sorted(BD.STREAMS))
def test_index_streams_have_the_entries_they_were_built_for(L, name):
    stream, entries, contents = BD.index_stream(name)
    total, targets = BD.STREAMS[name]
    assert len(stream) == total
    rows, code = F.index(L, stream)
    assert code == 0 and rows == entries
    hit = [t for t in targets if t in contents]
    assert set(contents) == set(hit) and len(hit) >= len(targets) - 1 and all(d == len(contents[p]) for p, _, d in rows if p in contents)
    for t in hit:                                                                    # a frame's magic number, nothing else, at every aimed offset
        assert stream[t:t + 4] == BD.ZSTD_MAGIC.to_bytes(4, "little")
    if name != "one_tile":
        for b, ms in BD.BORDER_M.items():                                            # the four bytes across the border in every way
            assert len(ms) == 5 and all(b * m - d in hit for d, m in enumerate(ms)), b
        assert all(m % 4 for m in BD.BORDER_M[BD.INDEX_STEP]) and all(m % 256 for m in BD.BORDER_M[BD.INDEX_LANE])      # a step border that is no tile border, ...
        assert len({m for ms in BD.BORDER_M.values() for m in ms}) == 15
    # false magic numbers of both kinds in the payloads, across tile and step borders too, and one that opens a whole valid frame
    payload = bytearray(stream)
    for p, c, _ in rows:
        if p in contents:
            payload[p:p + c] = bytes(c)
    zs, sk = BD.ZSTD_MAGIC.to_bytes(4, "little"), BD.SKIP_MAGIC.to_bytes(4, "little")[1:]
    false_z = [i for i in range(len(payload) - 3) if payload[i:i + 4] == zs]
    false_s = [i for i in range(8, len(payload) - 3) if payload[i + 1:i + 4] == sk and payload[i] >> 4 == 5 and i not in {p for p, _, _ in rows}]
    assert len(false_z) > 10 and len(false_s) > 10
    for border in (BD.INDEX_STEP, BD.INDEX_TILE)[:0 if name == "one_tile" else 2]:        # (the one tile's borders carry frames)
        assert {(-i) % border for i in false_z + false_s} >= {1, 2, 3}, border
    inner = next(i for i in false_z if F.index(L, stream[i:i + 28]) == ([(0, 28, 19)], 0))
    assert (inner + 1) % BD.INDEX_LANE == 0
    if name == "ends_with_3_magic_bytes":
        assert stream[-3:] == zs[:3]
