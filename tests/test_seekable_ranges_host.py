"""Opened seekable archives, the part that needs no GPU: the new names are exported; zsmi_openSeekable judges a host archive's table before it
asks for a context (every table damage of test_seekable_table.py gives the code zsmi_seekableNumFrames gives for it, a valid table
init_missing); the NULL cases of the handle's calls; and the Python statement of the span rule the GPU tests take their expected frame
counts from agrees with zsmi_seekableFrameInfo on which frame holds which offset."""
import ctypes
import pytest
import _seekable as S
import _seekable_ranges as R
import test_seekable_table as T

E_GENERIC, E_PREFIX, E_INIT_MISSING = 1, 10, 62
NEW = ["zsmi_openSeekable", "zsmi_openSeekableDevice", "zsmi_closeSeekable", "zsmi_getNumFrames_fromSeekable", "zsmi_getContentSize_fromSeekable",
       "zsmi_sizeofSeekable", "zsmi_seekableReadRangesDevice", "zsmi_seekableReadRangesHost"]


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    _lib.build()
    return _lib.lib()


def test_new_names_are_exported(L):
    from zstandard_amd import _lib
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    import zstandard_amd
    assert hasattr(zstandard_amd, "SeekableHandle") and hasattr(zstandard_amd.SeekableArchive, "read_many")
    assert hasattr(zstandard_amd.BatchCodec, "open_seekable_device")


def test_open_judges_the_table_before_the_context(L):
    arcs = T.archives()
    assert len(arcs) >= 4
    for name, (arc, _) in arcs.items():
        sk, err = R.open_host(L, None, arc)
        assert sk is None and err == E_INIT_MISSING, name                       # a valid table: only the context is missing
        for what, bad in R.table_damages(arc).items():
            want = T.code(L, L.zsmi_seekableNumFrames(bad, len(bad)))
            assert want != 0, (name, what)
            sk, err = R.open_host(L, None, bad)
            assert sk is None and err == want, (name, what)
    for what, (bad, want) in T.bad_archives()[1].items():                       # that file's own cases, with the codes it pins
        assert R.open_host(L, None, bad) == (None, want), what
    arc = arcs["oracle_64k_ck"][0]
    assert R.open_host(L, None, arc[-8:]) == (None, E_PREFIX)
    err = ctypes.c_int(-1)
    assert L.zsmi_openSeekable(None, None, 100, ctypes.byref(err)) is None and err.value == E_PREFIX
    assert L.zsmi_openSeekable(None, arc, len(arc), None) is None               # err may be NULL
    # the device form has to touch the device to see the table: the context comes first
    assert R.open_device(L, None, 0, 100) == (None, E_INIT_MISSING)


def test_null_handle_and_null_context(L):
    L.zsmi_closeSeekable(None)
    assert L.zsmi_getNumFrames_fromSeekable(None) == 0
    assert L.zsmi_getContentSize_fromSeekable(None) == 0
    assert L.zsmi_sizeofSeekable(None) == 0
    z = (ctypes.c_uint64 * 1)(0)
    w = (ctypes.c_uint64 * 1)(7)
    s = (ctypes.c_uint32 * 1)(7)
    n = ctypes.c_uint32(7)
    dst = ctypes.create_string_buffer(16)
    assert L.zsmi_seekableReadRangesDevice(None, None, z, z, 1, None, z, w, None, ctypes.byref(n)) == E_INIT_MISSING
    assert L.zsmi_seekableReadRangesHost(None, None, z, z, 1, dst, 16, w, s) == E_INIT_MISSING
    assert L.zsmi_seekableReadRangesDevice(None, None, None, None, 0, None, None, None, None, None) == E_INIT_MISSING
    assert (w[0], s[0], n.value) == (7, 7, 7)


def check_span_statement(L, arc):
    rows, _ = S.parse(arc)
    d = R.content_offsets(rows)
    probes = sorted({o for x in d for o in (x - 1, x, x + 1) if 0 <= o < d[-1]} | {0, d[-1] // 2, d[-1] // 3})
    for o in probes:
        if o >= d[-1]:
            continue
        first, last = R.span(d, o, o + 1)
        assert first == last
        rc, (_, do, _, ds) = T.info(L, arc, first)
        assert rc == 0 and do <= o < do + ds, (o, first)
    assert R.span(d, 5, 5) is None
    if len(rows) > 2:
        assert R.span(d, 0, d[-1]) == (0, max(i for i, r in enumerate(rows) if r[1]))
        assert R.span(d, d[1] - 1, d[2] + 1) == (0, bisect_first_nonempty(rows, 2))
    per, union = R.frames_touched(rows, [(0, 0), (d[-1], 10), (0, 1), (0, 1)])
    assert per[0] == [] and per[1] == [] and union == {per[2][0]} and per[2] == per[3]


def bisect_first_nonempty(rows, i):
    """the frame that holds the content byte at the start of frame i (zero-size frames hold none)"""
    while rows[i][1] == 0:
        i += 1
    return i


def test_span_statement_agrees_with_frame_info(L):
    for name, (arc, _) in T.archives().items():
        if name != "empty":
            check_span_statement(L, arc)


def test_span_statement_with_an_empty_part(L):
    import _data as D
    data = D.zipf_log(300000).tobytes()
    arc = S.zstd_archive([data[:70000], data[70000:70001], b"", data[70001:200000], b"", b"", data[200000:]], True)
    if arc is None:
        pytest.skip("libzstd is not on this machine")
    check_span_statement(L, arc)
    rows, _ = S.parse(arc)
    d = R.content_offsets(rows)
    assert R.span(d, 70000, 70001) == (1, 1)                 # the 1-byte part alone
    assert R.span(d, 70001, 70002) == (3, 3)                 # the empty part at 70001 holds no byte: the range starts in the part behind it
    assert R.span(d, 70000, 70002) == (1, 3)                 # ... and lies between the frames of a range across it
    assert R.span(d, 199999, 200001) == (3, 6)
