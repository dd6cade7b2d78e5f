"""The frame index on the host (no GPU): zsmi_countFrames, zsmi_buildSeekTable and the host checks of zsmi_openFrames against the Python
statement of the index (tests/_frames_index.py: the loop over zsmi_findFrameCompressedSize and zsmi_getFrameContentSize) - a good stream
of every kind of frame, false magic numbers in payloads included; bad streams, each with the statement's code from all three calls; the
empty stream; an archive that has a table.  The CPU walk loop and the table writer also run alone, in a host program under the address and
undefined-behaviour sanitizers (tests/c/frames_index.cpp)."""
import ctypes, os, subprocess
import pytest
import _frames_index as F
import _seekable as S
import test_seekable_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zstandard_amd", "csrc")


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    _lib.build()
    return _lib.lib()


def code(L, r):
    return int(L.zsmi_getErrorCode(r)) if L.zsmi_isError(r) else 0


def build_table(L, stream, cap=None):
    cap = 17 + 8 * 64 if cap is None else cap
    out = ctypes.create_string_buffer(max(cap, 1))
    r = L.zsmi_buildSeekTable(out, cap, stream, len(stream))
    return (None, code(L, r)) if L.zsmi_isError(r) else (out.raw[:r], 0)


def open_null_ctx(L, stream):
    err = ctypes.c_int(-1)
    assert not L.zsmi_openFrames(None, stream, len(stream), ctypes.byref(err))
    return err.value


def test_good_stream(L):
    good = F.good_stream()
    rows, c = F.index(L, good)
    parts = F.good_parts()
    assert c == 0 and len(rows) == len(parts)
    assert [(p, n) for p, n, _ in rows] == [(s, len(f)) for s, (f, _) in zip(F.starts(parts), parts)]
    assert [d for _, _, d in rows] == [len(content) for _, content in parts]
    assert L.zsmi_countFrames(good, len(good)) == len(rows)
    table, c = build_table(L, good)
    assert c == 0 and table == F.table(rows) and len(table) == 17 + 8 * len(rows)
    arc = good + table
    assert L.zsmi_seekableNumFrames(arc, len(arc)) == len(rows)
    co = do = 0
    for i, (pos, c, d) in enumerate(rows):
        assert T.info(L, arc, i) == (0, (co, do, c, d)) and co == pos, i
        co += c; do += d
    assert L.zsmi_seekableContentSize(arc, len(arc)) == do
    for cap in (0, 16, len(table) - 1):
        assert build_table(L, good, cap) == (None, F.E_TOO_SMALL)
    assert code(L, L.zsmi_buildSeekTable(None, 1 << 20, good, len(good))) == F.E_TOO_SMALL
    assert open_null_ctx(L, good) == F.E_INIT


EXPECT = {"wrong_magic_third_frame": F.E_PREFIX, "reserved_block_type": F.E_CORRUPT, "reserved_header_bit": F.E_PARAM, "no_content_size": F.E_PARAM,
          "content_size_over_1gib": F.E_PARAM, "junk_5_behind": F.E_PREFIX, "not_a_frame_at_0": F.E_PREFIX, "three_bytes": F.E_SRC_SIZE}


@pytest.mark.parametrize("name", sorted(F.bad_streams()))
def test_bad_streams(L, name):
    bad = F.bad_streams()[name]
    _, want = F.index(L, bad)
    assert want == EXPECT.get(name, F.E_SRC_SIZE)                          # (the cuts and the short tails: srcSize_wrong)
    assert code(L, L.zsmi_countFrames(bad, len(bad))) == want
    assert build_table(L, bad) == (None, want)
    assert build_table(L, bad, 0) == (None, want)                          # the stream's code comes before the capacity's
    assert open_null_ctx(L, bad) == want


def test_empty_stream_and_null(L):
    assert L.zsmi_countFrames(b"", 0) == 0 and L.zsmi_countFrames(None, 0) == 0
    assert build_table(L, b"") == (S.table([], False), 0) and len(S.table([], False)) == 17
    assert open_null_ctx(L, b"") == F.E_INIT
    assert code(L, L.zsmi_countFrames(None, 12)) == F.E_SRC_SIZE
    err = ctypes.c_int(-1)
    assert not L.zsmi_openFrames(None, None, 12, ctypes.byref(err)) and err.value == F.E_SRC_SIZE
    assert not L.zsmi_openFramesDevice(None, None, 0, ctypes.byref(err)) and err.value == F.E_INIT        # a NULL ctx first


@pytest.mark.parametrize("name", ["oracle_64k_ck", "oracle_100000_nock", "oracle_1", "empty"])
def test_an_archive_shows_its_table_as_a_last_entry(L, name):
    arc, parts = T.archives()[name]
    own, ck = S.parse(arc)
    rows, c = F.index(L, arc)
    assert c == 0 and L.zsmi_countFrames(arc, len(arc)) == len(rows) == len(own) + 1
    assert [(n, d) for _, n, d in rows[:-1]] == [(r[0], r[1]) for r in own]
    assert rows[-1][1:] == (17 + len(own) * (12 if ck else 8), 0)
    frames = arc[:rows[-1][0]]                                             # the table calls keep refusing a stream without one
    assert code(L, L.zsmi_seekableNumFrames(frames, len(frames))) == F.E_PREFIX
    assert L.zsmi_countFrames(frames, len(frames)) == len(own)


def test_python_surface(L):
    from zstandard_amd import api
    good = F.good_stream()
    rows, _ = F.index(L, good)
    assert api.count_frames(good) == len(rows) and api.build_seek_table(good) == F.table(rows)
    with pytest.raises(RuntimeError):
        api.count_frames(good[:-1])
    arc = api.SeekableArchive.from_frames(good)
    assert arc.num_frames == len(rows) and arc.content_size == sum(d for _, _, d in rows)
    co = do = 0
    for i, (pos, c, d) in enumerate(rows):
        assert arc.frame_info(i) == (co, do, c, d)
        co += c; do += d
    with pytest.raises(RuntimeError):
        arc.frame_info(len(rows))
    with pytest.raises(RuntimeError):
        api.SeekableArchive.from_frames(good + b"x")
    assert hasattr(api.BatchCodec, "open_frames_device")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="the sanitizer build is a CPU-side check: it runs on machines without a GPU, never next to one")
def test_walk_loop_and_table_writer_under_sanitizers(L, tmp_path):
    """the header alone, host code only, with -fsanitize=address,undefined: every stream in a heap block of exactly its size"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "frames_index")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unneeded-internal-declaration",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "c", "frames_index.cpp"), "-o", exe])
    streams = [("good", F.good_stream()), ("empty", b"")] + sorted(F.bad_streams().items()) + [("archive_" + n, a) for n, (a, _) in sorted(T.archives().items())]
    files = []
    for name, s in streams:
        files.append(str(tmp_path / name))
        open(files[-1], "wb").write(s)
    out = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(streams)
    for (name, s), line in zip(streams, lines):
        rows, c = F.index(L, s)
        if c:
            assert line.split() == [str(-c), str(-c), "-", "-"], name
        else:
            t = F.table(rows)
            assert line.split() == [str(len(rows)), str(len(t)), t.hex(), str(-F.E_TOO_SMALL)], name
