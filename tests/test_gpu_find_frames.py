"""Frame filters and the list search on archives: small record archives written by the resident path - a splitter layout with targetSize 4096 whose long records
are cut, fixed-size frames over text (misaligned, saturated), with and without a CDict / DDict set, with and without an index frame (an
empty last frame) - and on each: zsmi_seekableBuildFrameFilterResident and the host form byte for byte the host build of the text
(tests/_filter.py), a damaged frame's code as the rebuild reports it, the host checks; then the property the filter exists for:
build filter (resident) -> zsmi_filterFramesDevice -> zsmi_seekableFindQueryFramesResident, the count a device word the host never
reads, gives dRecords, dHits and dResult of zsmi_seekableFindQueryResident over the whole archive, and what the rule gives on the text
(tests/_findq.py) - any and all, K = 1, 4 and 8, with and without IGNORE_CASE, patterns absent, rare, in every record, shorter than g,
inside a cut record and across the border of two saturated frames - and so do the host form and SeekableArchive.find_records_query(
frame_filter=...); the list search on hand-made lists against the run rule (tests/_filter.py list_search); its refusals in dResult[0]
with dRecords untouched; and the honest fixture, where the list search's own dResult[3] says it decoded fewer bytes."""
import ctypes
import numpy as np
import pytest
import _filter as F, _findq as Q, _split as S, _recindex as R, _seekable_resident as SR, _resident_cdict_set as RS
from _hip import hip_of, Dev, CANARY
from _resident import up, down

pytestmark = pytest.mark.gpu
p = ctypes.c_void_p
M = 4096
MARK = b"xq7-border-mark"                                                 # lies across the cut of a long record: the border of two saturated frames


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def H():
    return hip_of()


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    bc = BatchCodec(0)
    yield bc
    bc.close()


@pytest.fixture(scope="module")
def text():
    """about 200 KiB of seeded tokens, some in upper case, with three records longer than maxFrameSize; the second holds MARK across its
    first cut, the third a rare word deep inside"""
    body = F.tokens(200000, 41, every=70, upper=0.1)
    cuts = [body.index(b"\n", c) + 1 for c in (len(body) // 5, len(body) // 2, 4 * len(body) // 5)]
    rng = np.random.default_rng(42)
    longs = [rng.integers(97, 123, size, dtype=np.uint8).tobytes() for size in (9000, 13000, 5000)]
    longs[1] = longs[1][:M - 7] + MARK + longs[1][M - 7 + len(MARK):]
    longs[2] = longs[2][:4500] + b"Needle-In-Cut" + longs[2][4513:]
    out = body[:cuts[0]] + longs[0] + b"\n" + body[cuts[0]:cuts[1]] + longs[1] + b"\n" + body[cuts[1]:cuts[2]] + longs[2] + b"\n" + body[cuts[2]:]
    return out[:-1]                                                       # the content ends without a delimiter


def layout(text, kind):
    if kind == "split":
        want = S.Split(text, 10, 4096, M)
        assert want.pieces > want.records and max(want.sizes) == M
        return want.sizes
    return F.fixed(len(text), 3000)


class Archive:
    """a fixture: the archive's bytes, the frames' content sizes as its table states them, and what opens it"""

    def __init__(self, L, H, codec, text, kind, dicts=False, index=False):
        from zstandard_amd import api
        sizes = layout(text, kind)
        self.cset = self.dset = None
        self.kind, self.handles = kind, []
        choice = None
        if dicts:
            self.cset, cds = RS.make_set(codec, 3)
            self.dset, dds = SR.ddict_set(codec)
            self.handles = list(set(cds)) + dds
            choice = SR.u32([SR.PICKS[k % len(SR.PICKS)] for k in range(len(sizes))])
        w = SR.write(L, H, codec, text, sizes, 3, 1, self.cset, choice)
        assert w.rc == 0 and w.archive is not None
        self.archive, self.sizes = w.archive, list(sizes)
        if index:
            first = R.Index(text, 10, R.offsets_of(sizes)).first_record
            self.archive = api.attach_record_index(self.archive, first)
            self.sizes = self.sizes + [0]

    def close(self, codec):
        codec.sync()
        for h in [self.cset, self.dset] + self.handles:
            if h is not None:
                h.close()


KINDS = [("split", False, False), ("split", True, False), ("split", False, True), ("fixed", False, False), ("fixed", True, True)]


@pytest.fixture(scope="module", params=KINDS, ids=lambda k: "%s%s%s" % (k[0], "_dicts" if k[1] else "", "_index" if k[2] else ""))
def arc(request, L, H, codec, text):
    a = Archive(L, H, codec, text, *request.param)
    yield a
    a.close(codec)


def resident_build(L, H, codec, a, g, Lg, damage=None, slack=16):
    """zsmi_seekableBuildFrameFilterResident on the archive in device memory: (the four result words, the filter's bytes)"""
    raw = bytearray(a.archive)
    if damage is not None:
        raw[damage] ^= 0x40
    dev = up(H, np.frombuffer(bytes(raw), dtype=np.uint8))
    assert H.hipDeviceSynchronize() == 0
    h = codec.open_seekable_device(dev.p, len(raw), ddict_set=a.dset)
    n = h.num_frames
    bound, total = h.find_work_bound(0, n), F.FIXED + n * (1 << (Lg - 3))
    work, flt, res = Dev(H, max(bound, 1)), Dev(H, total + slack), Dev(H, 32)
    assert H.hipDeviceSynchronize() == 0
    try:
        h.build_frame_filter_resident(work.p, bound, flt.p, total + slack, res.p, b"\n", g, Lg)
        codec.sync()
        vals = []
        for name, d, t in (("dResult", res, np.uint64), ("dFilter", flt, np.uint8), ("dWork", work, np.uint8)):
            v, ok = down(d, t)
            assert ok, "a guard word in front of or behind " + name + " is gone"
            vals.append(v.copy())
        assert (vals[1][total:] == CANARY).all(), "written behind the frame"
        return [int(v) for v in vals[0]], vals[1][:total].tobytes()
    finally:
        codec.sync(); h.close()
        for d in (dev, work, flt, res):
            d.free()


def test_resident_and_host_builds_equal_the_host_call(L, H, codec, text, arc):
    from zstandard_amd import SeekableArchive
    for g, Lg in ((4, 13), (3, 9)):
        size, want, _ = F.host_build(L, text, arc.sizes, 10, g, Lg)
        assert size == len(want)
        slots, hashed = F.slots_of(text, arc.sizes, 10, g, Lg)
        assert want == F.frame(text, arc.sizes, 10, g, Lg, slots)
        result, got = resident_build(L, H, codec, arc, g, Lg)
        assert result == [0, len(want), F.parse(want)["saturated"], hashed] and got == want, (g, Lg, result)
        sa = SeekableArchive(arc.archive, ddict_set=arc.dset)
        try:
            assert sa.build_frame_filter(b"\n", g, Lg) == want
        finally:
            sa.close()
    assert F.parse(want)["saturated"] >= len(F.saturated_frames(text, arc.sizes, 10)) > 2


def test_a_damaged_frame_gives_the_rebuilds_code(L, H, codec, text):
    a = Archive(L, H, codec, text, "split")
    try:
        at = R.table_of(a.archive)
        inside = sum(r[0] for r in at[3][:7]) + at[3][7][0] // 2                  # the middle of frame 7's compressed bytes
        result, _ = resident_build(L, H, codec, a, 4, 9, damage=inside)
        assert result[0] not in (0, F.E_PARAM) and result[1] == 40 + 64 * len(a.sizes)
        raw = bytearray(a.archive); raw[inside] ^= 0x40
        dev = up(H, np.frombuffer(bytes(raw), dtype=np.uint8))
        h = codec.open_seekable_device(dev.p, len(raw))
        n = h.num_frames
        first, work, res = Dev(H, 8 * (n + 1)), Dev(H, h.find_work_bound(0, n)), Dev(H, 32)
        try:
            h.index_records_resident(0, n, work.p, h.find_work_bound(0, n), first.p, res.p)
            codec.sync()
            assert int(down(res, np.uint64)[0][0]) == result[0]
        finally:
            h.close()
            for d in (dev, first, work, res):
                d.free()
    finally:
        a.close(codec)


def test_host_checks(L, H, codec, text):
    a = Archive(L, H, codec, text[:20000] + b"\n", "fixed")
    dev = up(H, np.frombuffer(a.archive, dtype=np.uint8))
    h = codec.open_seekable_device(dev.p, len(a.archive))
    try:
        n, bound, ctx, sk = h.num_frames, h.find_work_bound(0, h.num_frames), codec.ctx, h.handle
        one, odd = p(8), p(12)
        B, X = L.zsmi_seekableBuildFrameFilterResident, L.zsmi_seekableBuildFrameFilterHost
        need = 40 + 64 * n
        assert B(None, None, 999, 9, 99, None, 0, None, 0, None) == F.E_INIT and X(None, None, 999, 9, 99, None, 0, None) == F.E_INIT
        assert B(ctx, None, 999, 9, 99, None, 0, one, 0, one) == B(ctx, sk, 999, 9, 99, None, 0, None, 0, one) == B(ctx, sk, 999, 9, 99, None, 0, one, 0, None) == F.E_GENERIC
        assert B(ctx, sk, 999, 4, 9, None, 0, odd, 0, one) == B(ctx, sk, 10, 5, 9, None, 0, odd, 0, one) == B(ctx, sk, 10, 4, 17, None, 0, odd, 0, one) == F.E_PARAM
        assert B(ctx, sk, 10, 4, 9, None, bound, odd, 0, one) == F.E_GENERIC
        assert B(ctx, sk, 10, 4, 9, one, bound - 1, odd, 0, one) == F.E_TOO_SMALL
        assert B(ctx, sk, 10, 4, 9, one, bound, odd, need, one) == F.E_PARAM and B(ctx, sk, 10, 4, 9, one, bound, one, need - 1, one) == F.E_TOO_SMALL
        assert X(ctx, None, 10, 4, 9, one, need, one) == X(ctx, sk, 10, 4, 9, None, need, one) == X(ctx, sk, 10, 4, 9, one, need, None) == F.E_GENERIC
        assert X(ctx, sk, 10, 2, 9, one, need, one) == F.E_PARAM and X(ctx, sk, 10, 4, 9, one, need - 1, one) == F.E_TOO_SMALL
    finally:
        codec.sync(); h.close(); dev.free(); a.close(codec)


def queries(text):
    lines = text.split(b"\n")
    rare = lines[len(lines) // 3][5:17]
    assert len(rare) == 12 and text.count(rare) == 1
    out = []
    for flags in (0, Q.IGNORE_CASE):
        for mode in (Q.ANY, Q.ALL):
            out += [([b"zq9zq9zq9"], mode, flags),                                                                    # absent
                    ([rare], mode, flags), ([rare.swapcase()], mode, flags),                                          # rare (with the flag: the same record)
                    ([b"e"], mode, flags), ([b" ", rare[:3]], mode, flags),                                           # in every record; shorter than g
                    ([b"Needle-In-Cut"], mode, flags), ([MARK], mode, flags), ([MARK, b"needle-in-cut"], mode, flags),  # inside a cut record; across two saturated frames
                    ([rare, b"zq9zq9zq9", MARK, lines[7][:9]], mode, flags),                                          # K = 4
                    ([rare, lines[9][2:11], lines[200][1:8], MARK, b"Needle-In-Cut", lines[300][:6], b"zq9z", lines[-1][:5]], mode, flags)]   # K = 8
    return out


class Opened:
    """an archive in device memory with a handle, its firstRecord array and a work buffer for any list"""

    def __init__(self, H, codec, archive, first, dset=None):
        self.dev = up(H, np.frombuffer(archive, dtype=np.uint8))
        assert H.hipDeviceSynchronize() == 0
        self.h = codec.open_seekable_device(self.dev.p, len(archive), ddict_set=dset)
        self.N = self.h.num_frames
        self.first = up(H, np.ascontiguousarray(first, dtype=np.uint64))
        self.bound = self.h.find_frames_work_bound(self.N)
        self.work = Dev(H, max(self.bound, 1))
        assert H.hipDeviceSynchronize() == 0

    def close(self, codec):
        codec.sync(); self.h.close()
        for d in (self.dev, self.first, self.work):
            d.free()


def list_call(L, H, codec, o, patterns, mode, flags, frames, count=None, max_frames=None, capacity=64, work_capacity=None, d_frames=None, d_count=None):
    """zsmi_seekableFindQueryFramesResident: (rc, result words, records written, hits written, whether dRecords and dHits are untouched
    behind them).  frames / count: host values put into device memory here, unless d_frames / d_count (device pointers) are given"""
    q, keep = Q.query(L, patterns, mode, flags)
    own = []
    if d_frames is None:
        arr = np.ascontiguousarray(frames, dtype=np.uint32)
        max_frames = len(arr) if max_frames is None else max_frames
        fr = up(H, arr if len(arr) else np.zeros(1, dtype=np.uint32)); own.append(fr); d_frames = fr.p
        cw = up(H, np.array([len(arr) if count is None else count], dtype=np.uint64)); own.append(cw); d_count = cw.p
    rec, hit, res = Dev(H, max(8 * capacity, 1)), Dev(H, max(capacity, 1)), Dev(H, 32)
    own += [rec, hit, res]
    assert H.hipDeviceSynchronize() == 0
    try:
        rc = L.zsmi_seekableFindQueryFramesResident(codec.ctx, o.h.handle, p(o.first.p), o.N, 10, ctypes.byref(q), p(d_frames), p(d_count), max_frames, p(o.work.p),
                                                    o.bound if work_capacity is None else work_capacity, p(rec.p) if capacity else None, p(hit.p) if capacity else None,
                                                    capacity, p(res.p))
        codec.sync()
        vals = []
        for name, d, t in (("dResult", res, np.uint64), ("dRecords", rec, np.uint64), ("dHits", hit, np.uint8)):
            v, ok = down(d, t)
            assert ok, "a guard word in front of or behind " + name + " is gone"
            vals.append(v.copy())
        assert down(o.work)[1], "written outside dWork"
        result = [int(v) for v in vals[0]]
        n = min(result[1], capacity) if rc == 0 and result[0] < 1 << 63 else 0
        untouched = bool((vals[1][n:capacity].view(np.uint8) == CANARY).all() and (vals[2][n:capacity] == CANARY).all()) if capacity else \
            bool((vals[1].view(np.uint8) == CANARY).all())
        return rc, result, [int(v) for v in vals[1][:n]], [int(v) for v in vals[2][:n]], untouched
    finally:
        for d in own:
            d.free()


def test_filter_then_list_search_is_the_whole_search(L, H, codec, text, arc):
    """the main property, every step in device memory: the filter call's dFrames and dResult[0] go into the list search as they are"""
    from zstandard_amd import SeekableArchive
    first = R.Index(text, 10, R.offsets_of(arc.sizes)).first_record
    size, flt, _ = F.host_build(L, text, arc.sizes, 10, 4, 13)
    o = Opened(H, codec, arc.archive, first, arc.dset)
    d_flt, d_frames, d_res = up(H, np.frombuffer(flt, dtype=np.uint8)), Dev(H, 4 * o.N), Dev(H, 32)
    sa = SeekableArchive(arc.archive, ddict_set=arc.dset)
    cap = text.count(b"\n") + 1
    rec, hit, res = Dev(H, 8 * cap), Dev(H, cap), Dev(H, 32)
    skipped = 0
    try:
        assert sa.first_record(allow_misaligned=True).tolist() == first.tolist()
        for patterns, mode, flags in queries(text):
            name = {v: k for k, v in Q.MODES.items()}[mode]
            want = Q.find(text, patterns, mode, flags)
            o.h.find_query_resident(o.first.p, o.N, patterns, 0, o.N, o.work.p, o.bound, rec.p, hit.p, cap, res.p, mode=name, ignore_case=bool(flags))
            codec.sync()
            whole = [int(v) for v in down(res, np.uint64)[0]]
            n = whole[1]
            whole_records, whole_hits = down(rec, np.uint64)[0][:n].tolist(), down(hit)[0][:n].tolist()
            assert (whole_records, whole_hits, whole[0], whole[2]) == (want[0], want[1], len(want[0]), want[2]), (patterns, mode, flags)
            codec.filter_frames_device(d_flt.p, len(flt), patterns, 0, o.N, d_frames.p, o.N, d_res.p, mode=name, ignore_case=bool(flags))
            rc, result, records, hits, untouched = list_call(L, H, codec, o, patterns, mode, flags, None, max_frames=o.N, capacity=cap, d_frames=d_frames.p, d_count=d_res.p)
            assert rc == 0 and untouched and (records, hits, result[:2]) == (whole_records, whole_hits, whole[:2]), (patterns, mode, flags, result, whole)
            listed = down(d_frames, np.uint32)[0][:int(down(d_res, np.uint64)[0][0])].tolist()
            assert result[3] == sum(arc.sizes[f] for f in listed) <= whole[3]
            assert result[2] == whole[2] if mode == Q.ANY else result[2] <= whole[2]      # an `all` query's occurrences outside the passing frames are not met
            skipped += o.N - len(listed)
            # the host form on the same list, and the archive's own call
            got = sa.find_records_query(first, patterns, name, bool(flags), return_hits=True, frame_filter=flt)
            assert got == (whole_records, whole_hits) == sa.find_records_query(first, patterns, name, bool(flags), return_hits=True), (patterns, mode, flags)
            a, c = o.N // 4, o.N // 2                                      # a window cut anywhere
            assert sa.find_records_query(first, patterns, name, bool(flags), first_frame=a, frame_count=c, frame_filter=flt) == \
                sa.find_records_query(first, patterns, name, bool(flags), first_frame=a, frame_count=c), (patterns, mode, flags, "window")
        assert arc.kind == "fixed" or skipped > 10 * o.N                  # (fixed-size frames over text are nearly all saturated: nothing to skip)
        assert sa.find_records_query(first, [b"zq9zq9zq9"], "none", frame_filter=flt) == sa.find_records_query(first, [b"zq9zq9zq9"], "none")
        with pytest.raises(ValueError):
            sa.find_records_query(first, [b"ab"], frame_filter=F.frame(text[:-5], F.fixed(len(text) - 5, 3000)))
    finally:
        sa.close(); o.close(codec)
        for d in (d_flt, d_frames, d_res, rec, hit, res):
            d.free()


def test_hand_made_lists_follow_the_run_rule(L, H, codec, text):
    """one frame, every other frame, a list with empty frames, the content's last frame (no trailing delimiter), lists that separate a
    record's frames - the record appears once a run"""
    a = Archive(L, H, codec, text, "split", index=True)                   # (the index frame: an empty last frame)
    first = R.Index(text, 10, R.offsets_of(a.sizes)).first_record
    o = Opened(H, codec, a.archive, first)
    at = F.offsets_of(a.sizes)
    cut = next(f for f in range(o.N - 1) if a.sizes[f] == M and text[at[f + 1] - 1] != 10)      # a frame whose record goes on in the next
    marked = next(f for f in range(o.N) if at[f] <= text.index(MARK) < at[f + 1])
    lists = {"one frame": [5], "every other frame": list(range(0, o.N, 2)), "the odd frames": list(range(1, o.N, 2)), "all": list(range(o.N)),
             "the last frame and the empty one": [o.N - 2, o.N - 1], "the empty one alone": [o.N - 1], "the last frame alone": [o.N - 2], "none": [],
             "a cut record's first frame": [cut], "its frames apart": [cut, cut + 2], "across the mark, separated": [marked, marked + 2],
             "around the mark": [marked - 1, marked, marked + 1, o.N - 3, o.N - 2, o.N - 1]}
    tail = text.split(b"\n")[-1]
    assert tail and a.sizes[-1] == 0
    try:
        for what, frames in lists.items():
            for patterns, mode, flags in (([b"e"], Q.ANY, 0), ([tail[:6]], Q.ANY, 0), ([MARK[:8], b"Z"], Q.ANY, Q.IGNORE_CASE), ([b"a", b"th"], Q.ALL, 0),
                                          ([text[at[cut] + 10:at[cut] + 20]], Q.ANY, 0)):
                records, hits, matches, content = F.list_search(text, a.sizes, first, frames, patterns, mode, flags)
                for cap in (len(records) + 3, max(len(records) - 1, 0)):
                    got = list_call(L, H, codec, o, patterns, mode, flags, frames, capacity=cap)
                    assert got == (0, [len(records), min(len(records), cap), matches, content], records[:cap], hits[:cap], True), (what, patterns, cap, got[:2])
        # a record whose frames the list separates appears once a run: the cut record holds `e` in its first frame and in its third
        end = text.index(b"\n", at[cut])
        assert end >= at[cut + 2] and b"e" in text[at[cut]:at[cut + 1]] and b"e" in text[at[cut + 2]:end]
        records = F.list_search(text, a.sizes, first, lists["its frames apart"], [b"e"])[0]
        assert records.count(int(first[cut])) == 2 and records == sorted(records)
        # more entries than the count: the rest of dFrames is not read as frames
        got = list_call(L, H, codec, o, [b"e"], Q.ANY, 0, [3, 4, 0xFFFFFFFF, 1], count=2, max_frames=4, capacity=4000)
        want = F.list_search(text, a.sizes, first, [3, 4], [b"e"])
        assert got == (0, [len(want[0]), len(want[0]), want[2], want[3]], want[0], want[1], True)
        # the host form
        for frames in (lists["every other frame"], lists["around the mark"], []):
            records, hits, matches, content = F.list_search(text, a.sizes, first, frames, [b"e", MARK], Q.ANY, 0)
            q, keep = Q.query(L, [b"e", MARK])
            arr = np.ascontiguousarray(frames, dtype=np.uint32)
            out, hit, res = np.zeros(len(records) + 1, dtype=np.uint64), np.zeros(len(records) + 1, dtype=np.uint8), np.zeros(4, dtype=np.uint64)
            rc = L.zsmi_seekableFindQueryFramesHost(codec.ctx, o.h.handle, p(first.ctypes.data), o.N, 10, ctypes.byref(q), p(arr.ctypes.data) if len(arr) else None, len(arr),
                                                    p(out.ctypes.data), p(hit.ctypes.data), len(records) + 1, p(res.ctypes.data))
            assert rc == 0 and res.tolist() == [len(records), len(records), matches, content] and out[:-1].tolist() == records and hit[:-1].tolist() == hits
    finally:
        o.close(codec); a.close(codec)


def test_list_search_refusals(L, H, codec, text):
    """in dResult[0], dRecords untouched: a count above maxFrames, work too small (dResult[3] sizes a second call that succeeds), a
    descending list, a frame number out of range, a damaged frame in the list; `none` mode and the other host checks"""
    a = Archive(L, H, codec, text, "split")
    first = R.Index(text, 10, R.offsets_of(a.sizes)).first_record
    at = R.table_of(a.archive)
    raw = bytearray(a.archive); raw[sum(r[0] for r in at[3][:7]) + at[3][7][0] // 2] ^= 0x40                  # frame 7 is damaged
    o, bad = Opened(H, codec, a.archive, first), Opened(H, codec, bytes(raw), first)
    code = lambda got: (1 << 64) - got[1][0]
    try:
        def refused(got, want_code):
            assert got[0] == 0 and code(got) == want_code and got[1][1:3] == [0, 0] and got[2] == [] and got[4], got[:2]
            return got[1][3]
        assert refused(list_call(L, H, codec, o, [b"e"], Q.ANY, 0, [1, 2, 3], count=4, max_frames=3), F.E_TOO_SMALL) == o.h.find_frames_work_bound(4)
        frames = [2, 3, 9, 10, 20]
        need = sum(a.sizes[f] for f in frames) + 2                        # three runs: two delimiters between them
        assert refused(list_call(L, H, codec, o, [b"e"], Q.ANY, 0, frames, work_capacity=need - 1), F.E_TOO_SMALL) == need
        want = F.list_search(text, a.sizes, first, frames, [b"e"])
        got = list_call(L, H, codec, o, [b"e"], Q.ANY, 0, frames, work_capacity=need, capacity=len(want[0]))
        assert got == (0, [len(want[0]), len(want[0]), want[2], want[3]], want[0], want[1], True)
        refused(list_call(L, H, codec, o, [b"e"], Q.ANY, 0, [4, 3]), F.E_FRAME_INDEX)
        refused(list_call(L, H, codec, o, [b"e"], Q.ANY, 0, [3, 3]), F.E_FRAME_INDEX)
        refused(list_call(L, H, codec, o, [b"e"], Q.ANY, 0, [3, o.N]), F.E_FRAME_INDEX)
        refused(list_call(L, H, codec, o, [b"e"], Q.ANY, 0, [0xFFFFFFFF]), F.E_FRAME_INDEX)
        failing = list_call(L, H, codec, bad, [b"e"], Q.ANY, 0, [6, 7, 8])
        q, keep = Q.query(L, [b"e"])
        res = Dev(H, 32)
        try:
            bad.h.find_query_resident(bad.first.p, bad.N, [b"e"], 6, 3, bad.work.p, bad.bound, 0, 0, 0, res.p)
            codec.sync()
            window_code = (1 << 64) - int(down(res, np.uint64)[0][0])
        finally:
            res.free()
        assert refused(failing, window_code) is not None and window_code not in (0, F.E_TOO_SMALL, F.E_FRAME_INDEX)
        assert list_call(L, H, codec, bad, [b"e"], Q.ANY, 0, [5, 6, 8])[1][0] < 1 << 63                          # the damaged frame is not in the list
        # on the host
        one, ctx, sk = p(8), codec.ctx, o.h.handle
        X = L.zsmi_seekableFindQueryFramesResident
        qn = Q.query(L, [b"e"], Q.NONE)[0]
        assert X(None, sk, one, o.N, 10, ctypes.byref(q), one, one, 1, one, 8, one, None, 1, one) == F.E_INIT
        for args in ((None, one, one, one, one), (sk, None, one, one, one), (sk, one, None, one, one), (sk, one, one, None, one), (sk, one, one, one, None)):
            assert X(ctx, args[0], args[1], o.N, 999, ctypes.byref(q), args[2], args[3], 1, one, 8, one, None, 1, args[4]) == F.E_GENERIC
        assert X(ctx, sk, one, o.N, 10, None, one, one, 1, one, 8, one, None, 1, one) == X(ctx, sk, one, o.N, 10, ctypes.byref(q), one, one, 1, one, 8, None, None, 1, one) == F.E_GENERIC
        assert X(ctx, sk, one, o.N + 1, 999, ctypes.byref(q), one, one, 1, one, 8, one, None, 1, one) == F.E_PARAM
        assert X(ctx, sk, one, o.N + 1, 10, ctypes.byref(qn), one, one, 1, None, 8, one, None, 1, one) == F.E_UNSUPPORTED
        assert X(ctx, sk, one, o.N + 1, 10, ctypes.byref(q), one, one, 1, None, 8, one, None, 1, one) == F.E_PARAM
        assert X(ctx, sk, one, o.N, 10, ctypes.byref(q), one, one, 1, None, 8, one, None, 1, one) == F.E_GENERIC
        assert L.zsmi_seekableFindFramesWorkBound(sk, 3) == 3 * (M + 1) and L.zsmi_seekableFindFramesWorkBound(None, 3) == 0
        assert L.zsmi_seekableFindQueryFramesHost(None, sk, one, o.N, 10, ctypes.byref(q), one, 1, one, None, 1, one) == F.E_INIT
        assert L.zsmi_seekableFindQueryFramesHost(ctx, sk, one, o.N, 10, ctypes.byref(qn), one, 1, one, None, 1, one) == F.E_UNSUPPORTED
    finally:
        o.close(codec); bad.close(codec); a.close(codec)


def test_the_filter_skips_what_it_can(L, H, codec):
    """the honest fixture on an archive (tests/_filter.py: needle_text): the device list equals the statement's - the needle's frame and
    at most 3 others - and the list search decoded fewer bytes, by its own dResult[3], than the window search by its"""
    data, sizes = F.needle_text()
    w = SR.write(L, H, codec, data, sizes)
    assert w.rc == 0
    first = S.Split(data, 10, 4096, 1 << 16).first_record
    o = Opened(H, codec, w.archive, first)
    flt = Dev(H, F.FIXED + o.N * 1024 + 8)
    d_frames, d_res, res = Dev(H, 4 * o.N), Dev(H, 32), Dev(H, 32)
    rec = Dev(H, 64)
    try:
        o.h.build_frame_filter_resident(o.work.p, o.bound, flt.p, F.FIXED + o.N * 1024, d_res.p)
        codec.filter_frames_device(flt.p, F.FIXED + o.N * 1024, [F.NEEDLE], 0, o.N, d_frames.p, o.N, d_res.p)
        codec.sync()
        want, _ = F.filter_frames(F.frame(data, sizes), [F.NEEDLE])
        listed = down(d_frames, np.uint32)[0][:int(down(d_res, np.uint64)[0][0])].tolist()
        assert listed == want and F.NEEDLE_HOME in want and len(want) <= 4
        got = list_call(L, H, codec, o, [F.NEEDLE], Q.ANY, 0, None, max_frames=o.N, capacity=8, d_frames=d_frames.p, d_count=d_res.p)
        o.h.find_query_resident(o.first.p, o.N, [F.NEEDLE], 0, o.N, o.work.p, o.bound, rec.p, 0, 8, res.p)
        codec.sync()
        whole = [int(v) for v in down(res, np.uint64)[0]]
        assert got[0] == 0 and got[1][:3] == whole[:3] == [1, 1, 1] and got[2] == Q.find(data, [F.NEEDLE])[0] == down(rec, np.uint64)[0][:1].tolist()
        assert got[1][3] == sum(sizes[f] for f in want) < whole[3] == len(data)
    finally:
        o.close(codec)
        for d in (flt, d_frames, d_res, res, rec):
            d.free()
