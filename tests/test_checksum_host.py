"""The checksum parameter, the part that needs no GPU: zsmi_compressBound already holds the 4 bytes of a Content_Checksum (so nothing
that is sized by it changes), the new entry points are exported and refuse a NULL context, and tests/_checksum.py - the contract the GPU
tests hold the library to - is itself right: it rebuilds libzstd's checksummed fixtures from their plain form, and libzstd and oracle D
accept what it makes of oracle E's frames."""
import ctypes
import numpy as np
import pytest
import _oracle as O
import _data as D
import _checksum as CK

INIT_MISSING = 62
CHECKSUM_FLAG = 201


def worst_frame(n):
    """the largest frame the library can write for n content bytes: magic + descriptor (5), a 4-byte dictionary ID, the content size in 4
    bytes for a uint32 size (13 in all), every block raw (3 bytes of header each, one block for an empty chunk), the checksum"""
    n = np.asarray(n, dtype=np.uint64)
    return 13 + n + 3 * np.maximum(1, (n + 65535) // 65536) + 4


def bound(n):
    """zsmi_compressBound, in numpy over uint64 (pinned to the library's below)"""
    n = np.asarray(n, dtype=np.uint64)
    small = np.where(n < (128 << 10), ((128 << 10) - np.minimum(n, 128 << 10)) >> 11, 0).astype(np.uint64)
    return n + (n >> 8) + small + 3 * (n // 65536 + 1) + 18


def test_compress_bound_holds_the_checksum():
    from zstandard_amd import _lib
    L = _lib.lib()
    near = np.concatenate([np.arange(m * 65536 - 300, m * 65536 + 301) for m in range(1, 33)])
    ns = np.unique(np.concatenate([np.arange(0, 70001), near, [2 ** 32 - 1]])).astype(np.uint64)
    assert ns.max() == 2 ** 32 - 1 and (2 << 20) + 300 in ns and 70000 in ns
    for n in list(range(0, 70001, 997)) + [65535, 65536, 65537, 131072, (2 << 20) + 300, 2 ** 32 - 1]:      # the numpy statement is the library's
        assert int(bound(n)) == L.zsmi_compressBound(n), n
    slack = bound(ns).astype(np.int64) - worst_frame(ns).astype(np.int64)
    assert (slack >= 0).all(), (int(ns[slack.argmin()]), int(slack.min()))
    for n in (0, 1, 65536, 65537, 2 ** 32 - 1):                                                              # and straight from the library
        assert 13 + n + 3 * max(1, -(-n // 65536)) + 4 <= L.zsmi_compressBound(n), n


def test_new_entry_points_are_exported():
    from zstandard_amd import _lib
    L = _lib.lib()
    for name in ("zsmi_setParameter", "zsmi_getParameter", "zsmi_compress_advanced", "zsmi_compress_usingCDict_advanced"):
        assert name in _lib.EXPORTS and hasattr(L, name), name


def test_parameter_calls_refuse_a_null_context():
    from zstandard_amd import _lib
    L = _lib.lib()
    v = ctypes.c_int(7)
    assert L.zsmi_setParameter(None, CHECKSUM_FLAG, 1) == INIT_MISSING
    assert L.zsmi_setParameter(None, 12345, 9) == INIT_MISSING                    # (the context is judged first)
    assert L.zsmi_getParameter(None, CHECKSUM_FLAG, ctypes.byref(v)) == INIT_MISSING and v.value == 7
    assert L.zsmi_getParameter(None, CHECKSUM_FLAG, None) == INIT_MISSING


def test_with_checksum_rebuilds_the_libzstd_fixtures():
    fx = {k: v for k, v in D.fixtures().items() if v[0][4] & CK.CHECKSUM_BIT}
    assert len(fx) >= 3, sorted(fx)
    for name, (frame, content) in fx.items():
        plain = CK.without_checksum(frame)
        assert len(plain) == len(frame) - 4 and not plain[4] & CK.CHECKSUM_BIT
        assert O.decompress(plain, len(content)) == content, name                # (still a frame, of the same content)
        assert CK.with_checksum(plain, content) == frame, name
        assert CK.oracle_code(CK.flip(frame, len(frame) - 1, 0), len(content)) == CK.WRONG, name
    assert CK.trailer(b"") == CK.EMPTY_TRAILER


@pytest.mark.parametrize("level", [1, 3])
def test_libzstd_and_oracle_d_accept_with_checksum(level):
    z = D.zipf_log(200000, single=True).tobytes()
    rng = np.random.default_rng(3)
    cases = [b"", b"A", z[:255], z[:256], z[:65536], z[:65537], z[:200000], bytes(70000), rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()]
    for c in cases:
        plain = O.compress(c, level)
        f = CK.with_checksum(plain, c)
        assert len(f) == len(plain) + 4 and f[4] == plain[4] | 4
        assert O.decompress(f, len(c)) == c, len(c)
        if O.libzstd():
            assert O.zstd_decompress(f, len(c)) == c, len(c)
            assert O.zstd_decompress(CK.flip(f, len(f) - 2, 5), len(c)) is None, len(c)
        assert CK.oracle_code(CK.flip(f, len(f) - 2, 5), len(c)) == CK.WRONG, len(c)
