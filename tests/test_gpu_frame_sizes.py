"""zsmi_getFrameSizesBatchDevice (k_frame_sizes: the container walker, a lane an item) against the host calls, which
tests/test_frame_sizes_host.py pins to libzstd and oracle D; and zsmi_layoutOutputsDevice (the packer's tiled offset scan in its general
form) against numpy, below, at and above one tile of 2048 items and on both sides of 1024 tiles, where the one workgroup that scans the
tile sums gives a thread a second sum.  Items sit at odd offsets with gaps in a buffer of canary bytes: a walk
that leaves its item reads something else than the host call, which sees the item alone."""
import numpy as np
import pytest
import _batch as B, _data as D, _resident as R, _sizes as S
from _hip import hip_of, Dev, CANARY

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    bc = BatchCodec(0)
    yield bc
    bc.close()


@pytest.fixture(scope="module")
def H():
    return hip_of()


@pytest.fixture(scope="module")
def batch(codec):
    """(items, src bytes, offsets, sizes, want): the items laid out, and (content size, bound, status) of each by the host calls"""
    rng = np.random.default_rng(300)
    z = D.zipf_log(310000, single=True).tobytes()
    own = B.compress_many(codec, [z[:n] for n in (0, 1, 1024, 65537, 300 << 10)])
    two, unsized = S.two_frame_item(), S.unsized_frame("1k", "comp", 2, checksum=True)
    items = [it for _, it in S.items()] + own + [two[:n] for n in range(len(two))] + [unsized[:n] for n in range(len(unsized))]
    items += [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(5, 400, 16)]
    order = rng.permutation(len(items))
    items = [items[i] for i in order]
    sizes = np.array([len(it) for it in items], dtype=np.uint32)
    _, offs, bounds, total = B.ragged_device_layout(codec.L, sizes, rng)
    assert (offs % 2 == 1).any() and (np.diff(offs.astype(np.int64)) > bounds[:-1].astype(np.int64)).any()
    src = np.full(total, CANARY, dtype=np.uint8)
    for o, it in zip(offs, items):
        src[int(o):int(o) + len(it)] = np.frombuffer(it, dtype=np.uint8)
    want = np.array([S.host_answers(codec.L, it) for it in items], dtype=np.uint64)
    return items, src, offs, sizes, want


def test_batch_holds_what_it_is_for(batch):
    items, _, _, sizes, want = batch
    assert 280 <= len(items) <= 340
    codes = set(want[:, 2].tolist())
    assert {0, 10, 72} <= codes and (want[:, 0] == S.UNKNOWN).any() and (want[:, 0] == S.ERROR).any() and 0 in sizes
    assert ((want[:, 2] != 0) == (want[:, 0] == S.ERROR)).all() and ((want[:, 2] != 0) == (want[:, 1] == S.ERROR)).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, None])
def test_sizes_equal_the_host_calls(codec, H, batch, n):
    items, src_np, offs, sizes, want = batch
    N = len(items)
    n = N if n is None else n
    src, d_off, d_sz = R.up(H, src_np), R.up(H, offs), R.up(H, sizes)
    content, bounds, status = Dev(H, 8 * N), Dev(H, 8 * N), Dev(H, 4 * N)
    codec.frame_sizes_device(src.p, d_off.p, d_sz.p, n, content.p, bounds.p, status.p)
    codec.sync()
    got = [R.down(content, np.uint64)[0], R.down(bounds, np.uint64)[0], R.down(status, np.uint32)[0]]
    for k, what in enumerate(("content size", "bound", "status")):
        bad = np.flatnonzero(got[k][:n] != want[:n, k])
        assert bad.size == 0, (what, [(int(i), len(items[i]), int(got[k][i]), int(want[i, k])) for i in bad[:6]])
    for dev, width in ((content, 8), (bounds, 8), (status, 4)):              # canaries behind entry n, and around the buffers
        R.assert_tail_untouched(dev, n * width, f"n = {n}")
    for d in (src, d_off, d_sz, content, bounds, status):
        d.free()


@pytest.mark.parametrize("without", ["content sizes", "bounds"])
def test_either_output_may_be_null(codec, H, batch, without):
    items, src_np, offs, sizes, want = batch
    N = len(items)
    src, d_off, d_sz = R.up(H, src_np), R.up(H, offs), R.up(H, sizes)
    out, status = Dev(H, 8 * N), Dev(H, 4 * N)
    if without == "content sizes":
        codec.frame_sizes_device(src.p, d_off.p, d_sz.p, N, 0, out.p, status.p)
    else:
        codec.frame_sizes_device(src.p, d_off.p, d_sz.p, N, out.p, 0, status.p)
    codec.sync()
    got, ok = R.down(out, np.uint64)
    assert ok and (got == want[:, 1 if without == "content sizes" else 0]).all()
    st, ok = R.down(status, np.uint32)
    assert ok and (st == want[:, 2]).all()
    for d in (src, d_off, d_sz, out, status):
        d.free()


LIMIT = 0xFFFFFF88            # the largest size that is no error code


@pytest.mark.parametrize("align", [1, 64, 4096])
@pytest.mark.parametrize("n", [1, 1025, 2048, 2049, 3000])
def test_layout_equals_numpy(codec, H, n, align):
    layout_equals_numpy(codec, H, n, align, 300000)


# the single workgroup of 1024 threads that scans the tile sums (k_pack_scan_tiles) gives a thread ceil(tiles / 1024) of them: one up to
# 1024 tiles of 2048 items (tests/_borders.py SCAN_LEVEL, held against the source by tests/test_borders_host.py).  Exactly 1024 tiles, one
# item more (a thread two sums, the last threads none), 1025 tiles and one item
@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("n", [2097152, 2097153, 2099201])
def test_layout_equals_numpy_at_the_scans_second_level(codec, H, n, align):
    layout_equals_numpy(codec, H, n, align, 5001)


def layout_equals_numpy(codec, H, n, align, top):
    rng = np.random.default_rng(n * 8191 + align)
    sizes = rng.integers(0, top, n).astype(np.uint64)
    status = np.zeros(n, dtype=np.uint32)
    special = [LIMIT, LIMIT + 1, S.UNKNOWN, S.ERROR, 1 << 32, 0, 1, align, align + 1, (1 << 40) + 5]
    at = rng.choice(n, min(n, len(special)), replace=False)
    sizes[at] = np.array(special[:len(at)], dtype=np.uint64)
    status[rng.choice(n, max(1, n // 9), replace=False)] = rng.choice([10, 14, 16, 20, 72], max(1, n // 9))
    if n > 1:
        status[at[0]] = 0                                                     # (the largest legal size stays a legal item)
    for use_status in (True, False):
        st = status if use_status else np.zeros(n, dtype=np.uint32)
        want_caps = np.where((st == 0) & (sizes <= LIMIT), sizes, 0).astype(np.uint64)
        step = (want_caps + np.uint64(align - 1)) // np.uint64(align) * np.uint64(align)
        want_off = np.concatenate([[0], np.cumsum(step, dtype=np.uint64)]).astype(np.uint64)
        d_sizes, d_status = R.up(H, sizes), R.up(H, status)
        caps, offs = Dev(H, 4 * (n + 3)), Dev(H, 8 * (n + 4))
        codec.layout_outputs_device(d_sizes.p, d_status.p if use_status else 0, n, caps.p, offs.p, align=align)
        codec.sync()
        got_caps, got_off = R.down(caps, np.uint32)[0], R.down(offs, np.uint64)[0]
        assert (got_caps[:n] == want_caps).all(), np.flatnonzero(got_caps[:n] != want_caps)[:8].tolist()
        assert (got_off[:n + 1] == want_off).all(), np.flatnonzero(got_off[:n + 1] != want_off)[:8].tolist()
        R.assert_tail_untouched(caps, 4 * n, "caps")
        R.assert_tail_untouched(offs, 8 * (n + 1), "offsets")
        for d in (d_sizes, d_status, caps, offs):
            d.free()
    with pytest.raises(RuntimeError, match="out of bound"):
        codec.layout_outputs_device(0, 0, 0, 0, 0, align=align * 3)
