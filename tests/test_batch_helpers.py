"""The helpers the GPU tests stand on (tests/_batch.py, and the NCount reader and frame walker of tests/_framewriter.py), checked where a
bug in one would hide a failure elsewhere.  CPU only: the codec is a stub that returns prepared arrays."""
import numpy as np
import pytest
import _batch as B
import _corpus as C
import _framewriter as W
import _oracle as O


def test_layout_and_batch():
    assert B.layout([]).tolist() == [] and B.layout([]).dtype == np.uint64
    assert B.layout([7]).tolist() == [0]
    assert B.layout(np.array([3, 0, 0, 5, 1], dtype=np.uint32)).tolist() == [0, 3, 3, 3, 8]
    assert B.layout([3, 0, 5], gaps=[2, 0, 7]).tolist() == [2, 5, 12]
    big = B.layout(np.array([0xFFFFFFFF, 0xFFFFFFFF, 1], dtype=np.uint32))          # sums in 64 bits, not in the sizes' 32
    assert big.tolist() == [0, 0xFFFFFFFF, 0x1FFFFFFFE] and big.dtype == np.uint64
    for chunks, want_src, want_offs in (([], b"\0", []), ([b""], b"\0", [0]), ([b"", b""], b"\0", [0, 0]), ([b"abc"], b"abc", [0]),
                                        ([b"ab", b"", b"cde", b""], b"abcde", [0, 2, 2, 5])):
        src, offs, sizes = B.batch(chunks)
        assert src.dtype == np.uint8 and src.tobytes() == want_src
        assert offs.dtype == np.uint64 and offs.tolist() == want_offs
        assert sizes.dtype == np.uint32 and sizes.tolist() == [len(c) for c in chunks]
        assert B.cut(src, offs, sizes) == chunks


class StubCodec:
    """compress_host / decompress_host give back what they were made with, and keep the arguments of the last call"""
    def __init__(self, result):
        self.result = result

    def compress_host(self, *args, **kw):
        self.args, self.kw = args, kw
        return self.result

    decompress_host = compress_host


def _result(sizes):
    arena = np.frombuffer(b"aaaabbcccccc", dtype=np.uint8)
    return arena, np.array([0, 4, 6], dtype=np.uint64), np.array(sizes, dtype=np.uint32)


def test_frames_of_refuses_error_sizes():
    assert B.frames_of(_result([4, 2, 6]), 3) == [b"aaaa", b"bb", b"cccccc"]
    assert B.frames_of(_result([4, 0, 6])) == [b"aaaa", b"", b"cccccc"]
    assert B.ERR == (1 << 32) - 120                                                  # a size is an error code above (uint32)-120
    for bad in (B.ERR, B.ERR + 1, 0xFFFFFFBA, 0xFFFFFFFF):
        for at in range(3):
            sizes = [4, 2, 6]; sizes[at] = bad
            with pytest.raises(AssertionError):
                B.frames_of(_result(sizes), 3)
            with pytest.raises(AssertionError):
                B.compress_many(StubCodec(_result(sizes)), [b"x", b"y", b"z"])
    assert B.frames_of(_result([4, 2, B.ERR - 1]), 2) == [b"aaaa", b"bb"]              # (only the first n are looked at)


def test_compress_many_passes_the_batch_on():
    codec = StubCodec(_result([4, 2, 6]))
    assert B.compress_many(codec, [b"uv", b"", b"w"], 4, b"dict") == [b"aaaa", b"bb", b"cccccc"]
    src, offs, sizes, level, dic = codec.args
    assert (src.tobytes(), offs.tolist(), sizes.tolist(), level, dic, codec.kw) == (b"uvw", [0, 2, 2], [2, 0, 1], 4, b"dict", {})
    B.compress_many(codec, [b"uv", b"", b"w"], cdict="CD")
    assert len(codec.args) == 3 and codec.kw == {"cdict": "CD"}


def test_decode_many_gives_no_bytes_for_an_error():
    codec = StubCodec(_result([4, 0xFFFFFFBA, 6]))
    assert B.decode_many(codec, [b"f0", b"f1", b"f2"], [4, 0, 6], b"dict") == [(4, b"aaaa"), (0xFFFFFFBA, b""), (6, b"cccccc")]
    src, offs, sizes, caps, dic = codec.args
    assert (src.tobytes(), offs.tolist(), sizes.tolist(), caps.tolist(), dic) == (b"f0f1f2", [0, 2, 4], [2, 2, 2], [4, 1, 6], b"dict")
    B.decode_many(codec, [b"f0", b"f1", b"f2"], [4, 0, 6], min_cap=0)
    assert codec.args[3].tolist() == [4, 0, 6] and codec.args[4] == b""
    assert B.decode_many(StubCodec(_result([B.ERR + 1, 2, B.ERR])), [b"", b"", b""], [1, 1, 1]) == [(B.ERR + 1, b""), (2, b"bb"), (B.ERR, b"")]


def test_assert_only_frames_written():
    offs, sizes, bounds = [10, 40, 70], [5, 0, 12], [20, 20, 20]
    def arena(*stray):
        host = np.full(100, B.CANARY, dtype=np.uint8)
        for o, s in zip(offs, sizes):
            host[o:o + s] = 1
        host[30] = B.CANARY                                                        # (a frame may hold the canary's value)
        for at in stray:
            host[at] = 0
        return host
    B.assert_only_frames_written(arena(), offs, sizes, bounds, B.CANARY, "clean")
    B.assert_only_frames_written(arena(10, 14, 70, 81), offs, sizes, bounds, B.CANARY, "inside the frames")
    for what, at in (("before a frame", 9), ("after a frame", 15), ("before the last", 69), ("after the last", 82), ("in a gap", 50),
                     ("where the empty frame sits", 40), ("first byte", 0), ("last byte", 99), ("within the bound, behind the frame", 19)):
        with pytest.raises(AssertionError, match="written outside the frames"):
            B.assert_only_frames_written(arena(at), offs, sizes, bounds, B.CANARY, what)
    with pytest.raises(AssertionError, match="size above its bound"):
        B.assert_only_frames_written(arena(), offs, [5, 0, 21], bounds, B.CANARY, "bound")
    with pytest.raises(AssertionError, match="size above its bound"):
        B.assert_only_frames_written(arena(), offs, np.array([5, 0xFFFFFFBA, 12], dtype=np.uint32), bounds, B.CANARY, "error word")


def test_ragged_device_layout():
    class Lib:
        zsmi_compressBound = staticmethod(lambda n: n + 10)
    sizes = np.array([5, 0, 7, 3], dtype=np.uint32)
    so, do, bounds, total = B.ragged_device_layout(Lib, sizes, np.random.default_rng(4))
    gaps = np.random.default_rng(4).integers(0, 300, 4) * [0, 1, 0, 1]
    assert so.tolist() == [0, 5, 5, 12] and bounds.tolist() == [15, 10, 17, 13]
    assert do.tolist() == [0, 15 + gaps[1], 25 + gaps[1], 42 + gaps[1] + gaps[3]] and total == int(do[3]) + 13 + 4096


def test_run_child():
    assert "CHILD-OK" in B.run_child("-c", "import sys\nprint(sys.argv[1], 'CHILD-OK')", "arg")
    assert B.run_child("-c", "import os\nprint(os.environ['ZZ'], os.getcwd())", env={"ZZ": "zz"}, cwd="/", marker="zz /").strip() == "zz /"
    assert B.run_child("-c", "import sys\nsys.exit(0)", marker=None) == ""
    with pytest.raises(AssertionError):
        B.run_child("-c", "import sys\nprint('CHILD-OK')\nsys.exit(3)")
    with pytest.raises(AssertionError):
        B.run_child("-c", "import sys\nprint('nothing')")


ZERO_RUNS = [1] + [0] * 1 + [1] + [0] * 3 + [2] + [0] * 4 + [3] + [0] * 25 + [-1, 0, 1] + [0] * 10 + [23]      # sums to 32


@pytest.mark.parametrize("norm,log", [W.LL_PRE, W.ML_PRE, W.OF_PRE, (ZERO_RUNS, 5), ([32], 5), ([0] * 24 + [64], 6), ([-1] * 31 + [1], 5)],
                         ids=["ll_default", "ml_default", "of_default", "zero_runs_1_3_4_25", "one_symbol", "run_of_24", "all_below_one"])
def test_read_ncount_inverts_ncount(norm, log):
    desc = W.ncount(norm, log)
    for front in (b"", b"\xff\x00\x7f"):
        assert W.read_ncount(front + desc + b"\xa5" * 9, len(front), len(norm) - 1) == (norm, log, len(front) + len(desc))
    if 0 in norm:                                                                   # a run of zeros past the last symbol allowed
        last_zero = len(norm) - 1 - norm[::-1].index(0)
        with pytest.raises(AssertionError):
            W.read_ncount(desc, 0, last_zero - 1)


@pytest.mark.parametrize("level", [1, 3])
def test_blocks_agrees_with_oracle_d(level):
    """oracle E's frames of every corpus class: the walker finds the blocks oracle D decodes - as many of each type, the same number of
    literals and of sequences (zso_statsGet: [20 + type] blocks, [30] sequences, [31] literals), every block of content accounted for"""
    seen = set()
    for k, (name, data) in enumerate(sorted(C.corpus(1 << 18).items())):
        data = data[:200000 + 4099 * k]
        frame = O.compress(data, level)
        out, st = O.decode_stats(frame, len(data))
        assert out == data
        h = W.frame_header(frame)
        found = list(W.blocks(frame))
        assert h.single and h.content_size == len(data) and found[-1].last and found[-1].end + 4 * h.checksum == len(frame), name
        assert [sum(b.type == t for b in found) for t in (0, 1, 2)] == [int(st[20]), int(st[21]), int(st[22])], name
        comp = [b for b in found if b.type == 2]
        assert sum(b.regen for b in comp) == int(st[31]) and sum(b.nseq for b in comp) == int(st[30]), name
        # oracle E cuts 64 KiB blocks: a raw or RLE block states its content, a compressed one holds what is left of its 64 KiB
        assert len(found) == (len(data) + 65535) // 65536, name
        sizes = [min(65536, len(data) - 65536 * i) for i in range(len(found))]
        assert all(b.size == n for b, n in zip(found, sizes) if b.type != 2) and sum(sizes) == h.content_size, name
        assert all(b.regen <= n and b.pos + b.size == b.end and b.seq_pos < b.end for b, n in zip(found, sizes) if b.type == 2), name
        for b in comp:
            seen.add(("lit", b.lit_type)); seen.add(("fmt", b.size_format)); seen.add(("nseq", min(b.nseq, 128) // 127))
            assert (b.modes is None) == (b.nseq == 0) and (b.huf_pos is None) == (b.lit_type != 2), name
    assert {("lit", 0), ("lit", 2)} <= seen and len({k for k in seen if k[0] == "fmt"}) >= 3 and ("nseq", 1) in seen, seen
