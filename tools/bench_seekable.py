#!/usr/bin/env python3
"""Seekable archives on one MI355X, against the batch calls on the same chunks in the same process (README).
1 GiB of the Zipf log stream, 64 KiB frames, level 3, checksums on:
  compress:  zsmi_compressSeekableDevice vs zsmi_compressBatchDevice on the same 64 KiB chunks (bound-spaced output, no packing)
  decode:    zsmi_decompressSeekableDevice of the whole archive vs zsmi_decompressBatchDevice of the same frames
  kernels:   k_seek_hash (compress) and k_seek_verify (decode), HIP-event timing of one call each
  latency:   a 4 KiB zsmi_decompressSeekable (one-shot, host buffers) from the middle of the archive, and the frames it overlaps
  ranges:    --ranges N reads of --range-bytes B at seeded uniform offsets through an opened archive (zsmi_openSeekableDevice): ONE
             zsmi_seekableReadRangesDevice call, the same ranges as N zsmi_decompressSeekableDevice calls one after the other, and the whole
             archive as one range through the handle; ms, GiB/s of content delivered, distinct frames decoded
Every call is followed by a synchronisation (the seekable read waits for its stream anyway), rates are the median over --reps calls.
The archive and the decoded content are checked once.  Prints one JSON line.
  python tools/bench_seekable.py [--mib 1024] [--reps 10] [--frame 65536] [--ranges 4096] [--range-bytes 4096]
--records: record archives instead (zsmi_compressSeekableFrames*, zsmi_seekableReadFramesDevice).  --mib (256) of records of --record-bytes
(1024 and 4096: a JSON line each), json_records and binary_table interleaved, one 64 KiB dictionary per class trained (zsmi_trainFromBuffer) on
a disjoint part, both through a CDict set of two.  One process, the legs of a comparison in turn, three rounds:
  size:   archive bytes over content for (a) 64 KiB fixed frames without a dictionary, (b) a frame per record without one, (c) a frame per
          record with the dictionaries
  write:  (c) against zsmi_compressBatchDevice_usingCDictSet + zsmi_packFramesDevice on the same chunks; the difference is the hash, table
          and packing work, reported in ms beside the rates, with the kernels' own times of one call
  fetch:  --ranges seeded random records in ONE zsmi_seekableReadFramesDevice call on (c) against the same records' byte ranges in one
          zsmi_seekableReadRangesDevice call on (a): ms, frames decoded x frame bytes, content bytes delivered
  python tools/bench_seekable.py --records [--mib 256] [--record-bytes 1024 4096] [--ranges 4096]
--records --resident: a second JSON line a record size, the device-resident calls against the host-array calls above on the same records
in the same process, the legs in turn, three rounds:
  write:  zsmi_compressSeekableFramesResident_usingCDictSet (sizes and indices in device memory) against (c)'s call; the archives must be
          equal; the kernels of one resident call, those that plan on the device summed
  fetch:  the same --ranges records through zsmi_seekableReadFramesResident (numbers in device memory, a frame named twice decoded twice)
          against zsmi_seekableReadFramesDevice
--index: streams of frames WITHOUT a table (zsmi_openFramesDevice) - the default archive with its table cut off and --record-mib of 1 KiB
record frames: the open call against zsmi_openSeekableDevice on the same frames with their table, the index kernels one by one, the whole
content through both handles, and the stream as one item of zsmi_decompressBatchDevice (index_legs' docstring).  One JSON line.
  python tools/bench_seekable.py --index [--mib 1024] [--record-mib 256] [--one-item-limit 240]
--split: the record splitter (zsmi_splitRecordsDevice) on the same text stream, split at newlines: the call and its kernels one by one at
targetSize 0 and --target, against k_index_count / k_index_emit on the same buffer (split_legs' docstring).  One JSON line.
  python tools/bench_seekable.py --split [--mib 1024] [--frame 65536] [--target 4096]
--split --lines: lines by number from the split text's archive - zsmi_seekableReadRecordsResident against a host lookup and
zsmi_seekableReadFramesResident of the whole frames, for --ranges random lines and an ascending run (lines_legs' docstring).  A JSON line a
targetSize.
  python tools/bench_seekable.py --split --lines [--mib 1024] [--ranges 4096] [--line-targets 4096 65536 1048576]
--split --find PATTERN ...: find records by content on the same text stream and on its record archive (4 KiB and 64 KiB frames), for each
pattern: zsmi_findRecordsDevice and its kernels one by one against k_split_count / k_split_emit on the same buffer,
zsmi_seekableFindRecordsResident over the whole archive against the whole-content range read of the same handle, and today's way - that
range read, the copy to the host and bytes.find there (find_legs' docstring).  A JSON line a pattern, also appended to
profiles/find_records_bench.jsonl.
  python tools/bench_seekable.py --split --find "ERROR ienwbvuzw" e [--mib 1024] [--find-targets 4096 65536]
--split --find-query: find records by several patterns on the same stream and on its 64 KiB-frame archive, against the single-pattern calls
in the same process (find_query_legs' docstring).  One JSON line, also appended to profiles/find_query_bench.jsonl.
  python tools/bench_seekable.py --split --find-query [--mib 1024]
--split --find-regex: find records by regular expression on the same stream, on a copy with records of a MiB and on the 64 KiB-frame
archive, against the literal searches and against re on the host (find_regex_legs' docstring).  One JSON line, also appended to
profiles/find_regex_bench.jsonl.
  python tools/bench_seekable.py --split --find-regex [--mib 1024]
--split --record-index: the record index on the same stream's archives at targetSize 65536, 4096 and 0 - attach against the resident compress
call it follows, load against zsmi_openSeekableDevice, rebuild against the whole-content range read, the body's kernels against the
splitter's (record_index_legs' docstring).  One JSON line, also appended to profiles/record_index_bench.jsonl.
  python tools/bench_seekable.py --split --record-index [--mib 1024]
--split --filter: frame filters on the same stream's archives at targetSize 65536 (g = 4, L = 13) and 4096 (g = 4, L = 10) - the filter's bytes
over the archive's, the build against the index rebuild, its kernels beside k_split_count, candidates against true frames, and filter ->
list search (zsmi_seekableFindQueryFramesResident, fed in device memory) against the whole-archive query search (filter_legs' docstring).
  python tools/bench_seekable.py --split --filter [--mib 1024] [--filter-patterns "ERROR ienwbvuzw"]"""
import argparse, json, os, sys, time
import torch                                               # before libzsmi.so
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _data as D
from zstandard_amd import BatchCodec, SeekableArchive, _lib, frame_filter_size


def timed(fn, sync, reps):
    fn(); sync()                                           # warm-up: plans, scratch
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); sync(); ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def _json_segment(job):
    import _corpus as C
    return C.json_records(job[1], seed=job[0])


def records_content(size, workers=16, seg=1 << 20):
    """size bytes of each of the two record classes, and 8 MiB of each from other seeds to train on.  The JSON generator is Python: it
    runs as independent segments on a pool of processes, started by fork - before the GPU is touched"""
    import multiprocessing as mp
    import _corpus as C
    nseg, ntrain = (size + seg - 1) // seg, 8
    with mp.get_context("fork").Pool(workers) as pool:
        parts = pool.map(_json_segment, [(11 + 1000 * k, seg) for k in range(nseg + ntrain)], chunksize=1)
    js, js_train = b"".join(parts[:nseg])[:size], b"".join(parts[nseg:])
    return {"json_records": (js, js_train), "binary_table": (C.binary_table(size, seed=14), C.binary_table(ntrain * seg, seed=15))}


def alternating(legs, sync, reps):
    """legs: name -> fn.  One warm-up each, then `reps` rounds, the legs in turn in every round -> name -> the sorted times"""
    for fn in legs.values():
        fn(); sync()
    ts = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            t = time.perf_counter(); fn(); sync(); ts[k].append(time.perf_counter() - t)
    return {k: sorted(v) for k, v in ts.items()}


def records(a):
    """--records: one frame per record against 64 KiB fixed frames, on records of two classes interleaved (see the module's docstring)"""
    from zstandard_amd import CompressionDict, CompressionDictSet, DecompressionDict, DecompressionDictSet, train_dictionary
    size, level, reps, N = (a.mib or 256) << 20, a.level, 3, a.ranges
    classes = ("json_records", "binary_table")
    corp = records_content(size // 2)
    bc = BatchCodec(0)
    L = bc.L
    med = lambda v: float(np.median(v))
    for R in a.record_bytes:
        n = size // R // 2 * 2
        rows = [np.frombuffer(corp[c][0], dtype=np.uint8)[:n // 2 * R].reshape(-1, R) for c in classes]
        data = np.stack(rows, axis=1).reshape(-1)                              # record i: class i % 2
        total = data.size
        dics = [train_dictionary((corp[c][1], np.full(len(corp[c][1]) // R, R)), capacity=65536, level=level) for c in classes]
        cds = [CompressionDict(bc, d, level) for d in dics]
        cset = CompressionDictSet(bc, cds, level)
        dds = [DecompressionDict(bc, d) for d in dics]
        dset = DecompressionDictSet(bc, dds)
        src = torch.from_numpy(data).cuda()
        fs = np.full(n, R, dtype=np.uint32)
        index = (np.arange(n) % 2).astype(np.uint32)
        bound_c = bc.seekable_frames_bound(fs, True)
        bound_a = bc.seekable_bound(total, 65536, True)
        arcs = {k: torch.empty(b, dtype=torch.uint8, device="cuda") for k, b in (("a", bound_a), ("b", bound_c), ("c", bound_c))}
        asz = torch.zeros(1, dtype=torch.int64, device="cuda")
        # the batch call and the packer on the same chunks, at the layout the archive's staging has
        so = np.arange(n, dtype=np.uint64) * R
        do = np.arange(n, dtype=np.uint64) * int(L.zsmi_compressBound(R))
        stage = torch.empty(n * int(L.zsmi_compressBound(R)), dtype=torch.uint8, device="cuda")
        bsz = torch.zeros(n, dtype=torch.int32, device="cuda")
        packed = torch.empty(bound_c, dtype=torch.uint8, device="cuda")
        poff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def size_of(fn):
            fn(); bc.sync()
            v = int(asz.item())
            assert 0 < v < (1 << 62), "a frame failed"
            return v
        size_a = size_of(lambda: bc.compress_seekable_device(src.data_ptr(), total, arcs["a"].data_ptr(), bound_a, asz.data_ptr(), level, 65536, True))
        size_b = size_of(lambda: bc.compress_seekable_frames_device(src.data_ptr(), fs, arcs["b"].data_ptr(), bound_c, asz.data_ptr(), level, True))
        write_c = lambda: bc.compress_seekable_frames_device(src.data_ptr(), fs, arcs["c"].data_ptr(), bound_c, asz.data_ptr(), checksum=True, cdict_set=cset, dict_index=index)
        size_c = size_of(write_c)

        def batch_pack():
            bc.compress_device(src.data_ptr(), so, fs, stage.data_ptr(), do, bsz.data_ptr(), cdict_set=cset, dict_index=index)
            bc.pack_device(stage.data_ptr(), do, bsz.data_ptr(), n, packed.data_ptr(), poff.data_ptr())
        tw = alternating({"archive": write_c, "batch_pack": batch_pack}, bc.sync, reps)
        frames_bytes = int(poff[n].item())
        assert frames_bytes == size_c - 17 - 12 * n and torch.equal(packed[:frames_bytes], arcs["c"][:frames_bytes]), "the archive's frames differ from the batch call's"
        bc.enable_timing(True); write_c(); kt = bc.kernel_times(); bc.enable_timing(False)
        # fetch: N seeded random records - by number from (c), as byte ranges from (a)
        pick = np.random.default_rng(7).integers(0, n, N).astype(np.uint32)
        place = np.arange(N, dtype=np.uint64) * R
        out = torch.zeros(N * R, dtype=torch.uint8, device="cuda")
        st = torch.ones(N, dtype=torch.int32, device="cuda")
        want = src.reshape(n, R)[torch.from_numpy(pick.astype(np.int64)).cuda()].reshape(-1)
        ha = bc.open_seekable_device(arcs["a"].data_ptr(), size_a)
        hc = bc.open_seekable_device(arcs["c"].data_ptr(), size_c, ddict_set=dset)
        decoded = {}

        def fetch_c():
            decoded["c"] = hc.read_frames_device(pick, out.data_ptr(), place, st.data_ptr())[1]

        def fetch_a():
            decoded["a"] = ha.read_ranges_device(pick.astype(np.uint64) * R, np.full(N, R, dtype=np.uint64), out.data_ptr(), place, st.data_ptr())[1]
        for f in (fetch_a, fetch_c):
            out.zero_(); st.fill_(1); f(); bc.sync()
            assert not st.any().item() and torch.equal(out, want), "fetched records differ from the content"
        tf = alternating({"records_c": fetch_c, "ranges_a": fetch_a}, bc.sync, reps)
        gib = total / float(1 << 30)
        ms = lambda k: round(kt.get(k, (0.0, 0))[0] * 1e3, 4)
        resident = resident_legs(a, bc, locals()) if a.resident else None
        print(json.dumps({
            "metric": "seekable_records", "mib": total >> 20, "record_bytes": R, "records": n, "level": level, "classes": classes,
            "size_over_content": {"a_64k_frames_no_dict": round(size_a / total, 4), "b_frame_per_record_no_dict": round(size_b / total, 4),
                                  "c_frame_per_record_dicts": round(size_c / total, 4)},
            "write_c_gibs": round(gib / med(tw["archive"]), 2), "write_c_ms": [round(t * 1e3, 3) for t in tw["archive"]],
            "batch_pack_gibs": round(gib / med(tw["batch_pack"]), 2), "batch_pack_ms": [round(t * 1e3, 3) for t in tw["batch_pack"]],
            "write_c_minus_batch_pack_ms": round((med(tw["archive"]) - med(tw["batch_pack"])) * 1e3, 3),
            "k_seek_hash_ms": ms("k_seek_hash"), "k_seek_table_ms": ms("k_seek_table"), "k_pack_copy_ms": ms("k_pack_copy"), "k_pack_offsets_ms": ms("k_pack_offsets"),
            "fetch_records": N, "fetch_delivered_bytes": N * R,
            "fetch_c_ms": [round(t * 1e3, 4) for t in tf["records_c"]], "fetch_c_frames_decoded": decoded["c"], "fetch_c_decoded_bytes": decoded["c"] * R,
            "fetch_a_ms": [round(t * 1e3, 4) for t in tf["ranges_a"]], "fetch_a_frames_decoded": decoded["a"], "fetch_a_decoded_bytes": decoded["a"] * 65536,
            "small_frame_packer_leg": "not tried"}), flush=True)
        if resident:
            print(json.dumps(resident), flush=True)
        ha.close(); hc.close(); cset.close(); dset.close()
        for x in cds + dds:
            x.close()
        del src, arcs, stage, packed, out
    bc.close()


PLAN_KERNELS = ("k_pack_offsets", "k_seek_guard", "k_compress_bounds", "k_plan_chunks", "k_plan_blocks", "k_plan_refuse", "k_seek_refuse")


def resident_legs(a, bc, v):
    """--resident: the device-resident write and fetch against the host-array calls of records(), whose locals are v"""
    src, total, n, R, N, reps, cset, hc = v["src"], v["total"], v["n"], v["R"], v["N"], v["reps"], v["cset"], v["hc"]
    med = lambda t: float(np.median(t))
    d_fs = torch.from_numpy(v["fs"].astype(np.int32)).cuda()
    d_ix = torch.from_numpy(v["index"].astype(np.int32)).cuda()
    bound = bc.seekable_frames_resident_bound(total, n, True)
    arc = torch.empty(bound, dtype=torch.uint8, device="cuda")
    asz = v["asz"]
    write_r = lambda: bc.compress_seekable_frames_resident(src.data_ptr(), total, d_fs.data_ptr(), n, R, arc.data_ptr(), bound, asz.data_ptr(), checksum=True,
                                                           cdict_set=cset, d_dict_index_ptr=d_ix.data_ptr())
    size_r = v["size_of"](write_r)
    assert size_r == v["size_c"] and torch.equal(arc[:size_r], v["arcs"]["c"][:size_r]), "the resident archive differs from the host-array call's"
    tw = alternating({"resident": write_r, "host_arrays": v["write_c"]}, bc.sync, reps)
    bc.enable_timing(True); write_r(); kt = bc.kernel_times(); bc.enable_timing(False)
    d_pick = torch.from_numpy(v["pick"].astype(np.int32)).cuda()
    out, st, want = v["out"], v["st"], v["want"]
    off = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    wr = torch.zeros(N, dtype=torch.int32, device="cuda")
    fetch_r = lambda: hc.read_frames_resident(d_pick.data_ptr(), N, out.data_ptr(), N * R, off.data_ptr(), wr.data_ptr(), st.data_ptr())
    out.zero_(); st.fill_(1); fetch_r(); bc.sync()
    assert not st.any().item() and torch.equal(out, want) and int(off[N].item()) == N * R, "the resident fetch differs from the content"
    tf = alternating({"resident": fetch_r, "host_arrays": v["fetch_c"]}, bc.sync, reps)
    gib = total / float(1 << 30)
    return {"metric": "seekable_records_resident", "mib": total >> 20, "record_bytes": R, "records": n, "level": v["level"],
            "write_resident_gibs": round(gib / med(tw["resident"]), 2), "write_resident_ms": [round(t * 1e3, 3) for t in tw["resident"]],
            "write_host_arrays_gibs": round(gib / med(tw["host_arrays"]), 2), "write_host_arrays_ms": [round(t * 1e3, 3) for t in tw["host_arrays"]],
            "write_resident_minus_host_arrays_ms": round((med(tw["resident"]) - med(tw["host_arrays"])) * 1e3, 3),
            "device_plan_kernels_ms": round(sum(kt.get(k, (0.0, 0))[0] for k in PLAN_KERNELS) * 1e3, 4),
            "write_resident_kernels_ms": {k: round(t[0] * 1e3, 4) for k, t in kt.items()},
            "fetch_records": N, "fetch_distinct_records": int(len(set(v["pick"].tolist()))),
            "fetch_resident_ms": [round(t * 1e3, 4) for t in tf["resident"]], "fetch_host_arrays_ms": [round(t * 1e3, 4) for t in tf["host_arrays"]]}


def magic_positions(t):
    """how many positions of the device byte tensor t hold one of the two frame magic numbers (the index's candidates, offset 0 apart)"""
    total, step = 0, 64 << 20
    for at in range(0, t.numel() - 3, step):
        x = t[at:min(t.numel(), at + step + 3)].to(torch.int64)
        w = x[:-3] | (x[1:-2] << 8) | (x[2:-1] << 16) | (x[3:] << 24)
        total += int(((w == 0xFD2FB528) | ((w & 0xFFFFFFF0) == 0x184D2A50)).sum().item())
    return total


def index_one_item(a):
    """--index-one-item (a process of its own, started by --index under a time limit): the stream of 64 KiB frames as ONE item of
    zsmi_decompressBatchDevice - frame after frame on one wavefront, the only way in without the index.  Prints the seconds of one call."""
    size, F = (a.mib or 1024) << 20, a.frame
    bc = BatchCodec(0)
    src = torch.from_numpy(D.zipf_log(size)).cuda()
    bound = bc.seekable_bound(size, F, False)
    arc = torch.empty(bound, dtype=torch.uint8, device="cuda"); asz = torch.zeros(1, dtype=torch.int64, device="cuda")
    bc.compress_seekable_device(src.data_ptr(), size, arc.data_ptr(), bound, asz.data_ptr(), a.level, F, False); bc.sync()
    n = (size + F - 1) // F
    stream = int(asz.item()) - 17 - 8 * n
    out = torch.empty(size, dtype=torch.uint8, device="cuda"); dsz = torch.zeros(1, dtype=torch.int32, device="cuda")
    z = np.zeros(1, dtype=np.uint64)
    t = time.perf_counter()
    bc.decompress_device(arc.data_ptr(), z, np.array([stream], dtype=np.uint32), out.data_ptr(), z, np.array([size], dtype=np.uint32), dsz.data_ptr()); bc.sync()
    t = time.perf_counter() - t
    assert int(dsz.item()) == size and torch.equal(out, src), "the one item decoded to something else"
    print(json.dumps({"one_item_seconds": round(t, 3)}), flush=True)
    bc.close()


def index_legs(a):
    """--index: what it costs to have no table, and what the index buys.  The 1 GiB / 64 KiB-frame archive with its table cut off, and
    --record-mib of 1 KiB record frames packed by zsmi_packFramesDevice; the legs of a comparison in turn in one process, three rounds:
      open:   zsmi_openFramesDevice on the frames against zsmi_openSeekableDevice on the same frames with their table; the index kernels'
              own times of one call; the candidates (places that hold a magic number) against the frames
      read:   the whole content as one range through the indexed handle against the table-opened handle (the same frames, the same path)
      item:   the same 64 KiB-frame stream as ONE item of zsmi_decompressBatchDevice, once, in a process of its own under --one-item-limit
              seconds (sized from the general kernel's ~53 GiB/s over its pool of 3072 wavefronts: ~17 MiB/s a wavefront, a minute a GiB);
              not finished inside it: said so, not tried again.  It runs last."""
    import subprocess
    size, F, level, reps = (a.mib or 1024) << 20, a.frame, a.level, 3
    gib = size / float(1 << 30)
    bc = BatchCodec(0)
    L = bc.L
    data = D.zipf_log(size)
    src = torch.from_numpy(data).cuda()
    n = (size + F - 1) // F
    bound = bc.seekable_bound(size, F, False)
    arc = torch.empty(bound, dtype=torch.uint8, device="cuda"); asz = torch.zeros(1, dtype=torch.int64, device="cuda")
    bc.compress_seekable_device(src.data_ptr(), size, arc.data_ptr(), bound, asz.data_ptr(), level, F, False); bc.sync()
    asize = int(asz.item()); stream = asize - 17 - 8 * n
    ms = lambda v: [round(t * 1e3, 4) for t in v]
    rep = {"metric": "frames_index", "gib": gib, "frame": F, "level": level, "frames": n, "stream_bytes": stream}

    def open_close(fn):
        def run():
            fn().close()
        return run

    def open_legs(p, with_table, without, frames, key):
        t = alternating({"table": open_close(lambda: bc.open_seekable_device(p, with_table)), "index": open_close(lambda: bc.open_frames_device(p, without))}, bc.sync, reps)
        bc.enable_timing(True); h = bc.open_frames_device(p, without); kt = bc.kernel_times(); bc.enable_timing(False)
        assert h.num_frames == frames
        rep[key] = {"open_with_table_ms": ms(t["table"]), "open_frames_ms": ms(t["index"]), "no_table_costs_ms": round((np.median(t["index"]) - np.median(t["table"])) * 1e3, 4),
                    "index_kernels_ms": {k: round(v[0] * 1e3, 4) for k, v in kt.items() if k.startswith("k_index")},
                    "index_kernel_launches": {k: v[1] for k, v in kt.items() if k.startswith("k_index")}}
        return h
    hi = open_legs(arc.data_ptr(), asize, stream, n, "frames_64k")
    rep["frames_64k"]["candidates"] = magic_positions(arc[:stream]) + 1
    ht = bc.open_seekable_device(arc.data_ptr(), asize)
    out = torch.empty(size, dtype=torch.uint8, device="cuda"); status = torch.ones(1, dtype=torch.int32, device="cuda")
    whole = lambda h: (lambda: h.read_ranges_device([0], [size], out.data_ptr(), [0], status.data_ptr()))
    for h in (hi, ht):
        out.zero_(); status.fill_(1); whole(h)(); bc.sync()
        assert int(status.item()) == 0 and torch.equal(out, src), "the whole content as one range differs"
    t = alternating({"index": whole(hi), "table": whole(ht)}, bc.sync, reps)
    rep["whole_content_indexed_ms"], rep["whole_content_table_ms"] = ms(t["index"]), ms(t["table"])
    rep["whole_content_indexed_gibs"] = round(gib / float(np.median(t["index"])), 2); rep["whole_content_table_gibs"] = round(gib / float(np.median(t["table"])), 2)
    hi.close(); ht.close()
    # the record stream: 1 KiB frames from the batch call, packed - and the same frames as an archive of records, for its table
    R = 1024
    rsize = a.record_mib << 20
    rn = rsize // R
    fs = np.full(rn, R, dtype=np.uint32)
    rbound = bc.seekable_frames_bound(fs, False)
    rarc = torch.empty(rbound, dtype=torch.uint8, device="cuda")
    bc.compress_seekable_frames_device(src.data_ptr(), fs, rarc.data_ptr(), rbound, asz.data_ptr(), level, False); bc.sync()
    rasize = int(asz.item()); rstream = rasize - 17 - 8 * rn
    rep["records_1k"] = {}
    open_legs(rarc.data_ptr(), rasize, rstream, rn, "records_1k").close()
    rep["records_1k"].update({"frames": rn, "stream_bytes": rstream, "candidates": magic_positions(rarc[:rstream]) + 1})
    del out, rarc, arc, src
    bc.close()
    torch.cuda.empty_cache()
    # last: the one item, once, in its own process under its limit (--one-item-limit 0: not run)
    if a.one_item_limit <= 0:
        rep["one_item"] = "not run"
        print(json.dumps(rep), flush=True)
        return
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--index-one-item", "--mib", str(size >> 20), "--frame", str(F), "--level", str(level)],
                           capture_output=True, text=True, timeout=a.one_item_limit)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode == 0 and line:
            sec = json.loads(line[-1])["one_item_seconds"]
            rep["one_item_seconds"] = sec; rep["one_item_gibs"] = round(gib / sec, 4)
            rep["indexed_over_one_item"] = round(sec / float(np.median(t["index"])), 1)
        else:
            rep["one_item"] = "failed: exit %d: %s" % (r.returncode, r.stderr[-300:])
    except subprocess.TimeoutExpired:
        rep["one_item"] = "not finished inside %d s; not tried again" % a.one_item_limit
    print(json.dumps(rep), flush=True)


def split_legs(a):
    """--split: the record splitter on the Zipf log stream (text lines, ~150 bytes each) in device memory.  For targetSize 0 and --target:
    zsmi_splitRecordsDevice, three calls each followed by a synchronisation; its kernels one by one (HIP events, three calls: the sorted
    times of each); and, on the same buffer in the same process, k_index_count / k_index_emit - zsmi_openFramesDevice refuses text, but
    only after both have scanned it - three calls too.  The chain cost (rounds x nodes of k_index_jump, targetSize > 0 only) is listed apart."""
    size, M, reps = (a.mib or 1024) << 20, a.frame, 3
    gib = size / float(1 << 30)
    bc = BatchCodec(0)
    src = torch.from_numpy(D.zipf_log(size)).cuda()
    words = torch.zeros(4, dtype=torch.int64, device="cuda")
    bc.count_records_device(src.data_ptr(), size, words.data_ptr()); bc.sync()
    records = int(words[0].item())
    mp = BatchCodec.split_pieces_bound(records, size, M)
    fs = torch.zeros(mp, dtype=torch.int32, device="cuda"); fr = torch.zeros(mp + 1, dtype=torch.int64, device="cuda")
    ms = lambda v: [round(t * 1e3, 4) for t in v]

    def kernels(fn, prefix):
        runs = []
        for _ in range(reps):
            bc.enable_timing(True)
            try:
                fn()
            except RuntimeError:
                pass                                               # (the index refuses text - behind its scan)
            runs.append(bc.kernel_times()); bc.enable_timing(False)
        names = [k for k in runs[0] if k.startswith(prefix)]
        return {k: sorted(round(r[k][0] * 1e3, 4) for r in runs) for k in names}, {k: runs[0][k][1] for k in names}
    rep = {"metric": "split_records", "gib": gib, "max_frame_size": M, "records": records, "max_pieces": mp,
           "count_records_ms": ms(alternating({"count": lambda: bc.count_records_device(src.data_ptr(), size, words.data_ptr())}, bc.sync, reps)["count"])}
    rep["index_kernels_ms"], _ = kernels(lambda: bc.open_frames_device(src.data_ptr(), size), "k_index")
    rep["index_kernels_ms"] = {k: v for k, v in rep["index_kernels_ms"].items() if k in ("k_index_count", "k_index_emit")}
    for T in (0, a.target):
        call = lambda: bc.split_records_device(src.data_ptr(), size, mp, fs.data_ptr(), fr.data_ptr(), words.data_ptr() + 8, target_size=T, max_frame_size=M)
        t = alternating({"split": call}, bc.sync, reps)["split"]
        n, recs, pieces = (int(v) for v in words[1:4].tolist())
        assert recs == records and pieces <= mp and 0 < n <= pieces, (n, recs, pieces)
        assert int(fs[:n].to(torch.int64).sum().item()) == size and int(fr[n].item()) == records, "the sizes do not sum to the source"
        kt, launches = kernels(call, "k_")
        rounds = launches.get("k_index_jump", 0)
        rep["target_%d" % T] = {"frames": n, "pieces": pieces, "split_call_ms": ms(t), "split_call_gibs": round(gib / float(np.median(t)), 1), "kernels_ms": kt,
                                "chain_rounds": rounds, "chain_nodes": mp, "chain_rounds_x_nodes": rounds * mp, "chain_ms": kt.get("k_index_jump", [0.0] * reps)}
    c0 = rep["target_0"]["kernels_ms"]
    rep["k_split_count_over_k_index_count"] = round(c0["k_split_count"][1] / rep["index_kernels_ms"]["k_index_count"][1], 3)
    rep["k_split_emit_over_k_index_emit"] = round(c0["k_split_emit"][1] / rep["index_kernels_ms"]["k_index_emit"][1], 3)
    bc.close()
    print(json.dumps(rep), flush=True)


def lines_legs(a):
    """--split --lines: lines by number from the record archive of the Zipf log stream, for each targetSize of --line-targets (4096 and
    65536 with maxFrameSize --frame, and 1 MiB frames - the case in which every follower rescans a long frame).  The text is split and
    compressed by the resident calls and opened; then, for --ranges seeded random lines and for one ascending run of as many, the legs in
    turn, three rounds, every call followed by a synchronisation:
      records:  zsmi_seekableReadRecordsResident, its numbers and firstRecord in device memory
      today:    firstRecord read back, the lookup in numpy, the frame numbers uploaded, zsmi_seekableReadFramesResident of the WHOLE frames
                (the lines are not cut out of them: that part of today's way is left out of its time); `today_read_only` is that call
                alone, its numbers already in device memory
    and the kernels of one records call one by one (three calls: the sorted times of each), with dResult.  A JSON line a targetSize."""
    size, reps, k = (a.mib or 1024) << 20, 3, a.ranges
    bc = BatchCodec(0)
    src = torch.from_numpy(D.zipf_log(size)).cuda()
    words = torch.zeros(4, dtype=torch.int64, device="cuda")
    bc.count_records_device(src.data_ptr(), size, words.data_ptr()); bc.sync()
    records = int(words[0].item())
    ms = lambda v: [round(t * 1e3, 4) for t in v]
    rng = np.random.default_rng(8)
    sets = {"random": rng.integers(0, records, k).astype(np.uint64), "ascending": (np.arange(k, dtype=np.uint64) + np.uint64(records // 3))}
    for T in a.line_targets:
        M = max(T, a.frame)
        mp = BatchCodec.split_pieces_bound(records, size, M)
        fs = torch.zeros(mp, dtype=torch.int32, device="cuda"); fr = torch.zeros(mp + 1, dtype=torch.int64, device="cuda")
        bc.split_records_device(src.data_ptr(), size, mp, fs.data_ptr(), fr.data_ptr(), words.data_ptr() + 8, target_size=T, max_frame_size=M); bc.sync()
        n = int(words[1].item())
        bound = bc.seekable_frames_resident_bound(size, n, True)
        arc = torch.empty(bound, dtype=torch.uint8, device="cuda"); arc_size = torch.zeros(1, dtype=torch.int64, device="cuda")
        bc.compress_seekable_frames_resident(src.data_ptr(), size, fs.data_ptr(), n, M, arc.data_ptr(), bound, arc_size.data_ptr(), level=a.level, checksum=True); bc.sync()
        m = int(arc_size.item())
        assert 0 < m <= bound, hex(m)
        sk = bc.open_seekable_device(arc.data_ptr(), m)
        rep = {"metric": "read_records", "gib": size / float(1 << 30), "target_size": T, "max_frame_size": M, "frames": n, "records": records, "lines": k,
               "archive_over_content": round(m / size, 4)}
        work_cap = sk.records_work_bound(k)
        work = torch.empty(max(work_cap, 1), dtype=torch.uint8, device="cuda")
        dst = torch.empty(max(work_cap, 1), dtype=torch.uint8, device="cuda")      # (today's way delivers whole frames: the same room)
        off = torch.zeros(k + 1, dtype=torch.int64, device="cuda"); wr = torch.zeros(k, dtype=torch.int64, device="cuda")
        st = torch.zeros(k, dtype=torch.int32, device="cuda"); res = torch.zeros(4, dtype=torch.int64, device="cuda")
        wr32 = torch.zeros(k, dtype=torch.int32, device="cuda")
        for name, picks in sets.items():
            d_idx = torch.from_numpy(picks.view(np.int64)).cuda()
            d_frames = torch.zeros(k, dtype=torch.int32, device="cuda")

            def new():
                sk.read_records_resident(fr.data_ptr(), n, d_idx.data_ptr(), k, k, work.data_ptr(), work_cap, dst.data_ptr(), work_cap, off.data_ptr(), wr.data_ptr(),
                                         st.data_ptr(), res.data_ptr())

            def lookup():
                first = fr[:n + 1].cpu().numpy().view(np.uint64)
                i = np.searchsorted(first, picks)
                return np.where(first[np.minimum(i, n)] == picks, i, i - 1).astype(np.int32)

            def today():
                d_frames.copy_(torch.from_numpy(lookup()))
                sk.read_frames_resident(d_frames.data_ptr(), k, dst.data_ptr(), work_cap, off.data_ptr(), wr32.data_ptr(), st.data_ptr())

            def today_read_only():
                sk.read_frames_resident(d_frames.data_ptr(), k, dst.data_ptr(), work_cap, off.data_ptr(), wr32.data_ptr(), st.data_ptr())
            sync = lambda: (bc.sync(), torch.cuda.synchronize())
            t = alternating({"records": new, "today": today, "today_read_only": today_read_only}, sync, reps)
            today(); sync()
            assert not st.any().item(), "a frame read failed"
            frame_bytes = int(off[k].item())
            new(); sync()
            assert not st.any().item() and int(res[0].item()) == k, "a record read failed"
            lens, offs = wr.cpu().numpy(), off.cpu().numpy()
            runs = []
            for _ in range(reps):
                bc.enable_timing(True); new(); bc.sync()
                runs.append(bc.kernel_times()); bc.enable_timing(False)
            kt = {kn: sorted(round(r[kn][0] * 1e3, 4) for r in runs) for kn in runs[0]}
            rep[name] = {"records_ms": ms(t["records"]), "today_ms": ms(t["today"]), "today_read_only_ms": ms(t["today_read_only"]),
                         "records_over_today": round(float(np.median(t["records"]) / np.median(t["today"])), 3),
                         "frame_reads": int(res[1].item()), "work_bytes": int(res[2].item()), "line_bytes": int(res[3].item()), "today_bytes": frame_bytes,
                         "kernels_ms": kt}
            for q in (0, k - 1):                                               # what was delivered is one line each
                line = dst[int(offs[q]):int(offs[q]) + int(lens[q])].cpu().numpy().tobytes()
                assert line.endswith(b"\n") and line.count(b"\n") == 1, "not one line"
        bc.sync(); sk.close()
        print(json.dumps(rep), flush=True)
        del arc, work, dst
    bc.close()


def host_grep(data, pattern):
    """today's way on the host: the numbers of the lines that hold the pattern, by bytes.find - the next occurrence, the newlines in front
    of it, then on from the line's end"""
    out, at, seen, counted = [], 0, 0, 0
    while True:
        p = data.find(pattern, at)
        if p < 0:
            return out
        seen += data.count(b"\n", counted, p); counted = p
        out.append(seen)
        at = data.find(b"\n", p) + 1
        if at == 0:
            return out


def find_legs(a):
    """--split --find: find records by content on the Zipf log stream (text lines, ~150 bytes each), 1 GiB in device memory, for every
    pattern of --find.  Legs in turn in one process, three rounds, every call followed by a synchronisation.
      text:     zsmi_findRecordsDevice; its kernels one by one (HIP events, three calls: the sorted times of each) next to k_split_count /
                k_split_emit of a zsmi_splitRecordsDevice call (targetSize 0) on the same buffer in the same process - the yardsticks
                of a tile scan here
      archive:  for each targetSize of --find-targets the text is split, compressed and opened by the resident calls; then
                find:       zsmi_seekableFindRecordsResident over all frames
                range_read: the whole content as one range of the same handle (zsmi_seekableReadRangesDevice) - the decode a search of an
                            archive cannot avoid
                today:      that range read, the copy to the host, bytes.find there (host_grep)
    The numbers are held against host_grep on the text."""
    size, M, reps = (a.mib or 1024) << 20, a.frame, 3
    gib = size / float(1 << 30)
    bc = BatchCodec(0)
    host = D.zipf_log(size)
    text = host.tobytes()
    src = torch.from_numpy(host).cuda()
    words = torch.zeros(4, dtype=torch.int64, device="cuda")
    bc.count_records_device(src.data_ptr(), size, words.data_ptr()); bc.sync()
    records = int(words[0].item())
    ms = lambda v: [round(t * 1e3, 4) for t in v]
    sync = lambda: (bc.sync(), torch.cuda.synchronize())
    found = torch.zeros(records, dtype=torch.int64, device="cuda"); res = torch.zeros(4, dtype=torch.int64, device="cuda")

    def kernels(fn):
        runs = []
        for _ in range(reps):
            bc.enable_timing(True); fn(); bc.sync()
            runs.append(bc.kernel_times()); bc.enable_timing(False)
        return {k: sorted(round(r[k][0] * 1e3, 4) for r in runs) for k in runs[0]}
    reports = {}
    for pattern in a.find:
        pat = pattern.encode()
        want = host_grep(text, pat)
        call = lambda: bc.find_records_device(src.data_ptr(), size, pat, found.data_ptr(), records, res.data_ptr())
        mp = BatchCodec.split_pieces_bound(records, size, M)
        fs = torch.zeros(mp, dtype=torch.int32, device="cuda"); fr = torch.zeros(mp + 1, dtype=torch.int64, device="cuda")
        split = lambda: bc.split_records_device(src.data_ptr(), size, mp, fs.data_ptr(), fr.data_ptr(), words.data_ptr() + 8, target_size=0, max_frame_size=M)
        t = alternating({"find": call, "split": split}, sync, reps)
        call(); sync()
        total, written, matches, scanned = (int(v) for v in res.tolist())
        assert (total, written, scanned) == (len(want), len(want), size) and found[:total].cpu().numpy().tolist() == want, "the device call and the host search differ"
        kf, ks = kernels(call), kernels(split)
        mid = lambda v: v[len(v) // 2]
        rep = {"metric": "find_records", "gib": gib, "pattern": pattern, "records": records, "records_found": total, "matches": matches,
               "find_call_ms": ms(t["find"]), "find_call_gibs": round(gib / float(np.median(t["find"])), 1), "split_call_ms": ms(t["split"]),
               "find_kernels_ms": {k: v for k, v in kf.items() if k.startswith("k_find")},
               "split_kernels_ms": {k: v for k, v in ks.items() if k in ("k_split_count", "k_split_emit")}}
        rep["k_find_count_over_k_split_count"] = round(mid(kf["k_find_count"]) / mid(ks["k_split_count"]), 3)
        rep["k_find_emit_over_k_split_emit"] = round(mid(kf["k_find_emit"]) / mid(ks["k_split_emit"]), 3)
        del fs, fr
        reports[pattern] = (rep, want)
    for T in a.find_targets:
        Mx = max(T, M)
        mp = BatchCodec.split_pieces_bound(records, size, Mx)
        fs = torch.zeros(mp, dtype=torch.int32, device="cuda"); fr = torch.zeros(mp + 1, dtype=torch.int64, device="cuda")
        bc.split_records_device(src.data_ptr(), size, mp, fs.data_ptr(), fr.data_ptr(), words.data_ptr() + 8, target_size=T, max_frame_size=Mx); bc.sync()
        n = int(words[1].item())
        bound = bc.seekable_frames_resident_bound(size, n, True)
        arc = torch.empty(bound, dtype=torch.uint8, device="cuda"); arc_size = torch.zeros(1, dtype=torch.int64, device="cuda")
        bc.compress_seekable_frames_resident(src.data_ptr(), size, fs.data_ptr(), n, Mx, arc.data_ptr(), bound, arc_size.data_ptr(), level=a.level, checksum=True); bc.sync()
        m = int(arc_size.item())
        assert 0 < m <= bound, hex(m)
        sk = bc.open_seekable_device(arc.data_ptr(), m)
        work_cap = sk.find_work_bound(0, n)
        assert work_cap == size
        work = torch.empty(size, dtype=torch.uint8, device="cuda"); st = torch.zeros(1, dtype=torch.int32, device="cuda")
        pinned = torch.empty(size, dtype=torch.uint8).pin_memory()
        for pattern in a.find:
            pat = pattern.encode()
            rep, want = reports[pattern]
            got = {}

            def find():
                sk.find_records_resident(fr.data_ptr(), n, pat, 0, n, work.data_ptr(), work_cap, found.data_ptr(), records, res.data_ptr())

            def range_read():
                sk.read_ranges_device([0], [size], work.data_ptr(), [0], st.data_ptr())

            def today():
                range_read(); sync()
                pinned.copy_(work); torch.cuda.synchronize()
                got["today"] = host_grep(pinned.numpy().tobytes(), pat)
            t = alternating({"find": find, "range_read": range_read, "today": today}, sync, reps)
            find(); sync()
            total = int(res[0].item())
            assert total == len(want) and found[:total].cpu().numpy().tolist() == want and got["today"] == want, "the archive call, today's way and the host search differ"
            bc.enable_timing(True); find(); bc.sync()
            out = (_lib.KernelTime * 64)()                                     # (more names than kernel_times() holds: the decoder's lie between)
            kt = {out[i].name.decode(): round(out[i].seconds * 1e3, 4) for i in range(bc.L.zsmi_getKernelTimes(bc.ctx, out, 64))}
            kt = {k: v for k, v in kt.items() if k.startswith("k_find") or k.startswith("k_seek")}
            bc.enable_timing(False)
            rep["target_%d" % T] = {"frames": n, "archive_over_content": round(m / size, 4), "find_ms": ms(t["find"]), "range_read_ms": ms(t["range_read"]),
                                    "today_ms": ms(t["today"]), "find_over_range_read": round(float(np.median(t["find"]) / np.median(t["range_read"])), 3),
                                    "today_over_find": round(float(np.median(t["today"]) / np.median(t["find"])), 1), "find_kernels_once_ms": kt}
        bc.sync(); sk.close()
        del arc, work, pinned, fs, fr
    bc.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(a.out or os.path.join(ROOT, "profiles", "find_records_bench.jsonl"), "a") as f:
        for pattern in a.find:
            line = json.dumps(reports[pattern][0])
            print(line, flush=True); f.write(line + "\n")


def find_query_legs(a):
    """--split --find-query: find records by several patterns (zsmi_findRecordsQueryDevice, zsmi_seekableFindQueryResident) on the Zipf
    log stream, 1 GiB in device memory, against the single-pattern calls in the same process.  Legs in turn, three rounds, every call
    followed by a synchronisation; the sorted times of each leg.
      k1:       the query call with one pattern, `any`, against zsmi_findRecordsDevice on that pattern - a rare one and one most lines hold
      k4, k8:   K patterns, `any`, against K single-pattern calls one after the other (their answers are NOT merged: the merge on the
                host, and the K - 1 copies it needs, are not counted against them)
      fold:     the K = 4 query with ZSMI_FIND_IGNORE_CASE against the same query without
      none:     `none` of the rare pattern, which writes nearly every record number, against `any` of it
      archive:  on the 64 KiB-frame archive, K = 4 `any` against 4 zsmi_seekableFindRecordsResident calls: one decode against four
    Every answer is held against the single-pattern calls' - the union for `any`, the complement's count for `none` - and the folded
    query against the unfolded one with both cases spelled out."""
    size, M, reps = (a.mib or 1024) << 20, a.frame, 3
    gib = size / float(1 << 30)
    bc = BatchCodec(0)
    host = D.zipf_log(size)
    src = torch.from_numpy(host).cuda()
    del host
    words = torch.zeros(4, dtype=torch.int64, device="cuda")
    bc.count_records_device(src.data_ptr(), size, words.data_ptr()); bc.sync()
    records = int(words[0].item())
    ms = lambda v: [round(t * 1e3, 4) for t in v]
    mid = lambda v: float(np.median(v))
    sync = lambda: (bc.sync(), torch.cuda.synchronize())
    found = torch.zeros(records, dtype=torch.int64, device="cuda"); hits = torch.zeros(records, dtype=torch.uint8, device="cuda")
    res = torch.zeros(4, dtype=torch.int64, device="cuda")
    rare, common = b"ERROR ienwbvuzw", b"e"
    eight = [b"ERROR", b"WARN", b"jzpvzxzz", b"dwon", b"DEBUG ienwbvuzw", b"qky", b"vhgovduu", b"INFO ang"]

    def single(pat):
        return lambda: bc.find_records_device(src.data_ptr(), size, pat, found.data_ptr(), records, res.data_ptr())

    def query(pats, mode="any", fold=False):
        return lambda: bc.find_records_query_device(src.data_ptr(), size, pats, found.data_ptr(), hits.data_ptr(), records, res.data_ptr(), mode=mode, ignore_case=fold)

    def singles(pats):
        calls = [single(p) for p in pats]
        return lambda: [c() for c in calls]

    def answer(fn):
        fn(); sync()
        total, written, matches, scanned = (int(v) for v in res.tolist())
        assert written == total and scanned == size
        return found[:total].clone(), matches

    def union(pats):
        rows, matches = [], 0
        for p in pats:
            r, m = answer(single(p))
            rows.append(r); matches += m
        return torch.unique(torch.cat(rows)), matches          # (sorted)
    rep = {"metric": "find_query", "gib": gib, "records": records}
    for name, pat in (("k1_rare", rare), ("k1_common", common)):
        t = alternating({"query": query([pat]), "single": single(pat)}, sync, reps)
        got, want = answer(query([pat])), answer(single(pat))
        assert torch.equal(got[0], want[0]) and got[1] == want[1], "the query call with one pattern and the single-pattern call differ"
        rep[name] = {"pattern": pat.decode(), "records_found": int(got[0].numel()), "query_ms": ms(t["query"]), "single_ms": ms(t["single"]),
                     "query_over_single": round(mid(t["query"]) / mid(t["single"]), 3)}
    for K in (4, 8):
        pats = eight[:K]
        t = alternating({"query": query(pats), "singles": singles(pats)}, sync, reps)
        got, want = answer(query(pats)), union(pats)
        assert torch.equal(got[0], want[0]) and got[1] == want[1], "the query's answer is not the union of the single-pattern answers"
        rep["k%d_any" % K] = {"patterns": [p.decode() for p in pats], "records_found": int(got[0].numel()), "query_ms": ms(t["query"]), "singles_ms": ms(t["singles"]),
                              "query_over_singles": round(mid(t["query"]) / mid(t["singles"]), 3)}
    pats = eight[:4]
    lower = [p.lower() for p in pats]
    t = alternating({"fold": query(lower, fold=True), "plain": query(pats)}, sync, reps)
    got, want = answer(query(lower, fold=True)), union(pats + lower)
    assert torch.equal(got[0], want[0]), "the folded query's answer is not the union over both cases"
    rep["k4_fold"] = {"records_found": int(got[0].numel()), "fold_ms": ms(t["fold"]), "plain_ms": ms(t["plain"]), "fold_over_plain": round(mid(t["fold"]) / mid(t["plain"]), 3)}
    t = alternating({"none": query([rare], "none"), "any": query([rare]), "single": single(rare)}, sync, reps)
    got, want = answer(query([rare], "none")), answer(single(rare))
    assert int(got[0].numel()) == records - int(want[0].numel()) and not bool(torch.isin(want[0], got[0]).any()), "`none` is not the complement"
    rep["none_rare"] = {"records_found": int(got[0].numel()), "none_ms": ms(t["none"]), "any_ms": ms(t["any"]), "single_ms": ms(t["single"]),
                        "none_over_single": round(mid(t["none"]) / mid(t["single"]), 3)}
    T = 65536
    Mx = max(T, M)
    mp = BatchCodec.split_pieces_bound(records, size, Mx)
    fs = torch.zeros(mp, dtype=torch.int32, device="cuda"); fr = torch.zeros(mp + 1, dtype=torch.int64, device="cuda")
    bc.split_records_device(src.data_ptr(), size, mp, fs.data_ptr(), fr.data_ptr(), words.data_ptr() + 8, target_size=T, max_frame_size=Mx); bc.sync()
    n = int(words[1].item())
    bound = bc.seekable_frames_resident_bound(size, n, True)
    arc = torch.empty(bound, dtype=torch.uint8, device="cuda"); arc_size = torch.zeros(1, dtype=torch.int64, device="cuda")
    bc.compress_seekable_frames_resident(src.data_ptr(), size, fs.data_ptr(), n, Mx, arc.data_ptr(), bound, arc_size.data_ptr(), level=a.level, checksum=True); bc.sync()
    m = int(arc_size.item())
    assert 0 < m <= bound, hex(m)
    want = union(pats)
    del src
    sk = bc.open_seekable_device(arc.data_ptr(), m)
    work_cap = sk.find_work_bound(0, n)
    assert work_cap == size
    work = torch.empty(size, dtype=torch.uint8, device="cuda")

    def archive_query():
        sk.find_query_resident(fr.data_ptr(), n, pats, 0, n, work.data_ptr(), work_cap, found.data_ptr(), hits.data_ptr(), records, res.data_ptr())

    def archive_singles():
        for p in pats:
            sk.find_records_resident(fr.data_ptr(), n, p, 0, n, work.data_ptr(), work_cap, found.data_ptr(), records, res.data_ptr())
    t = alternating({"query": archive_query, "singles": archive_singles}, sync, reps)
    got = answer(archive_query)
    assert torch.equal(got[0], want[0]) and got[1] == want[1], "the archive query's answer is not the union of the text's single-pattern answers"
    rep["archive_k4_any"] = {"target": T, "frames": n, "query_ms": ms(t["query"]), "singles_ms": ms(t["singles"]), "query_over_singles": round(mid(t["query"]) / mid(t["singles"]), 3)}
    bc.sync(); sk.close(); bc.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    line = json.dumps(rep)
    print(line, flush=True)
    with open(a.out or os.path.join(ROOT, "profiles", "find_query_bench.jsonl"), "a") as f:
        f.write(line + "\n")


def find_regex_legs(a):
    """--split --find-regex: find records by regular expression (zsmi_findRecordsRegexDevice, zsmi_seekableFindRegexResident) on the
    Zipf log stream, 1 GiB in device memory.  Legs in turn in one process, three rounds, every call followed by a synchronisation; the
    sorted times of each leg.  Every answer is held against `re` on the host (finditer over the whole text with [^\\n] where the pattern
    says `.`, an occurrence's record by the newlines in front of it), the one-byte literal against the single-pattern call.
      literal:  `ERROR ienwbvuzw` and `e` as regular expressions against zsmi_findRecordsDevice on the same bytes
      states:   ERROR.*[0-9]{3} and literals of 7, 15, 31 and 63 bytes (8 .. 64 states): the cost against the number of states
      fold:     ignore-case on against off
      invert:   ZSMI_REGEX_INVERT of the rare literal against the `none` query
      long:     the same bytes with every newline but one a MiB turned into a space: long records, the carry's hard case
      archive:  on the 64 KiB-frame archive, against zsmi_seekableFindRecordsResident and against today's way - the window read down
                to the host and `re` run there
      kernels:  the kernels' times one by one, of the rare literal"""
    import re
    from zstandard_amd import compile_regex
    size, M, reps = (a.mib or 1024) << 20, a.frame, 3
    gib = size / float(1 << 30)
    bc = BatchCodec(0)
    host = D.zipf_log(size)
    src = torch.from_numpy(host).cuda()
    words = torch.zeros(4, dtype=torch.int64, device="cuda")
    bc.count_records_device(src.data_ptr(), size, words.data_ptr()); bc.sync()
    records = int(words[0].item())
    ms = lambda v: [round(t * 1e3, 4) for t in v]
    mid = lambda v: float(np.median(v))
    sync = lambda: (bc.sync(), torch.cuda.synchronize())
    found = torch.zeros(records, dtype=torch.int64, device="cuda"); hits = torch.zeros(records, dtype=torch.uint8, device="cuda")
    res = torch.zeros(4, dtype=torch.int64, device="cuda")
    rare, common = b"ERROR ienwbvuzw", b"e"

    def single(pat, text=None):
        text = src if text is None else text
        return lambda: bc.find_records_device(text.data_ptr(), size, pat, found.data_ptr(), records, res.data_ptr())

    def regex(pattern, text=None, **kw):
        prog = compile_regex(pattern, **kw)
        text = src if text is None else text
        return lambda: bc.find_records_regex_device(text.data_ptr(), size, prog, found.data_ptr(), records, res.data_ptr())

    def answer(fn):
        fn(); sync()
        total, written, third, scanned = (int(v) for v in res.tolist())
        assert written == total and scanned == size
        return found[:total].clone(), third

    def by_re(pattern, data, flags=0):
        """the records `re` finds an occurrence in, ascending: the newlines in front of each occurrence's start"""
        newlines = np.flatnonzero(data == 10)
        starts = np.fromiter((m.start() for m in re.finditer(pattern, memoryview(data), flags)), dtype=np.int64)
        return np.unique(np.searchsorted(newlines, starts, side="left"))

    def same(got, want):
        return got.numel() == len(want) and bool((got.cpu().numpy() == want).all())
    rep = {"metric": "find_regex", "gib": gib, "records": records}
    for name, pat in (("literal_rare", rare), ("literal_common", common)):
        t = alternating({"regex": regex(re.escape(pat)), "single": single(pat)}, sync, reps)
        got, want = answer(regex(re.escape(pat))), answer(single(pat))
        assert got[1] == records and torch.equal(got[0], want[0]), "a literal as a regular expression and the single-pattern call differ"
        if pat is rare:
            assert same(got[0], by_re(re.escape(pat), host)), "the rare literal: not what re finds"
        rep[name] = {"pattern": pat.decode(), "states": compile_regex(re.escape(pat)).nStates, "records_found": int(got[0].numel()), "regex_ms": ms(t["regex"]),
                     "single_ms": ms(t["single"]), "regex_over_single": round(mid(t["regex"]) / mid(t["single"]), 3)}
    base = mid(alternating({"regex": regex(re.escape(rare))}, sync, reps)["regex"])
    curve = {}
    line = max(bytes(host[:4096]).split(b"\n")[:20], key=len)
    for name, pattern, on_host in [("ERROR.*[0-9]{3}", b"ERROR.*[0-9]{3}", b"ERROR[^\\n]*[0-9]{3}")] + \
                                  [("literal_%d" % k, re.escape((line * 8)[:k]), re.escape((line * 8)[:k])) for k in (7, 15, 31, 63)]:
        prog = compile_regex(pattern)
        t = alternating({"regex": regex(pattern)}, sync, reps)
        got = answer(regex(pattern))
        assert same(got[0], by_re(on_host, host)), (name, "not what re finds")
        curve[name] = {"states": prog.nStates, "classes": prog.nClasses, "records_found": int(got[0].numel()), "regex_ms": ms(t["regex"]),
                       "over_rare_literal": round(mid(t["regex"]) / base, 3)}
    rep["states"] = curve
    t = alternating({"fold": regex(b"error ienwbvuzw", ignore_case=True), "plain": regex(b"ERROR ienwbvuzw")}, sync, reps)
    got = answer(regex(b"error ienwbvuzw", ignore_case=True))
    assert same(got[0], by_re(b"error ienwbvuzw", host, re.IGNORECASE)), "ignore-case: not what re finds"
    rep["fold"] = {"records_found": int(got[0].numel()), "fold_ms": ms(t["fold"]), "plain_ms": ms(t["plain"]), "fold_over_plain": round(mid(t["fold"]) / mid(t["plain"]), 3)}
    none = lambda: bc.find_records_query_device(src.data_ptr(), size, [rare], found.data_ptr(), 0, records, res.data_ptr(), mode="none")
    t = alternating({"invert": regex(re.escape(rare), invert=True), "none": none}, sync, reps)
    got, want = answer(regex(re.escape(rare), invert=True)), answer(none)
    assert torch.equal(got[0], want[0]) and int(got[0].numel()) == records - len(by_re(re.escape(rare), host)), "invert is not the `none` query's answer"
    rep["invert_rare"] = {"records_found": int(got[0].numel()), "invert_ms": ms(t["invert"]), "none_ms": ms(t["none"]), "invert_over_none": round(mid(t["invert"]) / mid(t["none"]), 3)}
    # long records: every newline but the last of each MiB becomes a space
    flat = host.copy()
    newlines = np.flatnonzero(flat == 10)
    keep = np.unique(np.searchsorted(newlines, np.arange(1 << 20, size + 1, 1 << 20), side="left") - 1)
    flat[newlines] = 32; flat[newlines[keep[keep >= 0]]] = 10
    long_text = torch.from_numpy(flat).cuda()
    t = alternating({"long": regex(b"ERROR.*[0-9]{3}", long_text), "lines": regex(b"ERROR.*[0-9]{3}")}, sync, reps)
    got = answer(regex(b"ERROR.*[0-9]{3}", long_text))
    assert same(got[0], by_re(b"ERROR[^\\n]*[0-9]{3}", flat)), "long records: not what re finds"
    rep["long_records"] = {"records": got[1], "records_found": int(got[0].numel()), "long_ms": ms(t["long"]), "lines_ms": ms(t["lines"]),
                           "long_over_lines": round(mid(t["long"]) / mid(t["lines"]), 3)}
    del long_text, flat
    bc.enable_timing(True); regex(re.escape(rare))(); kt = bc.kernel_times(); bc.enable_timing(False)
    rep["kernels_ms"] = {k: round(v[0] * 1e3, 4) for k, v in kt.items()}
    # the archive
    T = 65536
    Mx = max(T, M)
    mp = BatchCodec.split_pieces_bound(records, size, Mx)
    fs = torch.zeros(mp, dtype=torch.int32, device="cuda"); fr = torch.zeros(mp + 1, dtype=torch.int64, device="cuda")
    bc.split_records_device(src.data_ptr(), size, mp, fs.data_ptr(), fr.data_ptr(), words.data_ptr() + 8, target_size=T, max_frame_size=Mx); bc.sync()
    n = int(words[1].item())
    bound = bc.seekable_frames_resident_bound(size, n, True)
    arc = torch.empty(bound, dtype=torch.uint8, device="cuda"); arc_size = torch.zeros(1, dtype=torch.int64, device="cuda")
    bc.compress_seekable_frames_resident(src.data_ptr(), size, fs.data_ptr(), n, Mx, arc.data_ptr(), bound, arc_size.data_ptr(), level=a.level, checksum=True); bc.sync()
    m = int(arc_size.item())
    assert 0 < m <= bound, hex(m)
    want = by_re(b"ERROR[^\\n]*[0-9]{3}", host)
    del src
    sk = bc.open_seekable_device(arc.data_ptr(), m)
    work_cap = sk.find_work_bound(0, n)
    assert work_cap == size
    work = torch.empty(size, dtype=torch.uint8, device="cuda")
    prog = compile_regex(b"ERROR.*[0-9]{3}")
    rx = re.compile(b"ERROR[^\\n]*[0-9]{3}")
    down = torch.empty(size, dtype=torch.uint8).pin_memory()
    status = torch.ones(1, dtype=torch.int32, device="cuda")

    def archive_regex():
        sk.find_regex_resident(fr.data_ptr(), n, prog, 0, n, work.data_ptr(), work_cap, found.data_ptr(), records, res.data_ptr())

    def archive_single():
        sk.find_records_resident(fr.data_ptr(), n, b"ERROR", 0, n, work.data_ptr(), work_cap, found.data_ptr(), records, res.data_ptr())

    def today():                                                                  # range read, copy down, re in Python
        sk.read_ranges_device([0], [size], work.data_ptr(), [0], status.data_ptr())
        down.copy_(work); torch.cuda.synchronize()
        return sum(1 for _ in rx.finditer(memoryview(down.numpy())))
    t = alternating({"regex": archive_regex, "single": archive_single, "today": today}, sync, reps)
    got = answer(archive_regex)
    assert same(got[0], want), "the archive: not what re finds on the text"
    rep["archive"] = {"target": T, "frames": n, "regex_ms": ms(t["regex"]), "single_ms": ms(t["single"]), "today_ms": ms(t["today"]),
                      "regex_over_single": round(mid(t["regex"]) / mid(t["single"]), 3), "regex_over_today": round(mid(t["regex"]) / mid(t["today"]), 4)}
    bc.sync(); sk.close(); bc.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    line = json.dumps(rep)
    print(line, flush=True)
    with open(a.out or os.path.join(ROOT, "profiles", "find_regex_bench.jsonl"), "a") as f:
        f.write(line + "\n")


def record_index_legs(a):
    """--split --record-index: the record index on the Zipf log stream (text lines, ~150 bytes each) in device memory, for archives of
    targetSize 65536, 4096 and 0 (a frame a record), three rounds of alternating legs each, all in one process:
      attach    zsmi_compressSeekableFramesResident alone against the same call followed by zsmi_seekableAttachRecordIndexResident;
      load      zsmi_seekableLoadRecordIndexResident against zsmi_openSeekableDevice (open + close) on the same archive;
      rebuild   zsmi_seekableIndexRecordsResident over the whole archive against the whole-content range read of the same handle - the
                decode it cannot avoid;
      kernels   k_recidx_tiles and k_recidx_places (zsmi_indexRecordsDevice on the text and the frames' borders, HIP events, three
                calls: the sorted times) beside k_split_count and k_split_emit on the same buffer.
    The loaded and the rebuilt arrays are held against the splitter's.  One JSON line, also appended to profiles/record_index_bench.jsonl."""
    size, M, reps = (a.mib or 1024) << 20, a.frame, 3
    gib = size / float(1 << 30)
    bc = BatchCodec(0)
    src = torch.from_numpy(D.zipf_log(size)).cuda()
    words = torch.zeros(8, dtype=torch.int64, device="cuda")
    bc.count_records_device(src.data_ptr(), size, words.data_ptr()); bc.sync()
    records = int(words[0].item())
    mp = BatchCodec.split_pieces_bound(records, size, M)
    fs = torch.zeros(mp, dtype=torch.int32, device="cuda"); fr = torch.zeros(mp + 1, dtype=torch.int64, device="cuda")
    work = torch.empty(size, dtype=torch.uint8, device="cuda"); dst = torch.empty(size, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ms = lambda v: [round(t * 1e3, 4) for t in v]
    med = lambda v: float(np.median(v))

    def kernels(fn, names):
        runs = []
        for _ in range(reps):
            bc.enable_timing(True); fn(); runs.append(bc.kernel_times()); bc.enable_timing(False)
        return {k: sorted(round(r[k][0] * 1e3, 4) for r in runs) for k in names}
    rep = {"metric": "record_index", "gib": gib, "max_frame_size": M, "records": records, "library": bc.L.zsmi_versionString().decode()}
    for T in (65536, 4096, 0):
        split = lambda: bc.split_records_device(src.data_ptr(), size, mp, fs.data_ptr(), fr.data_ptr(), words.data_ptr() + 8, target_size=T, max_frame_size=M)
        split(); bc.sync()
        n = int(words[1].item())
        room = bc.seekable_frames_resident_bound(size, n, True) + 40 + 4 * n + 12
        arc = torch.empty(room, dtype=torch.uint8, device="cuda"); arc_size = words.data_ptr() + 32
        compress = lambda: bc.compress_seekable_frames_resident(src.data_ptr(), size, fs.data_ptr(), n, M, arc.data_ptr(), room, arc_size, a.level, True)

        def compress_attach():
            compress(); bc.attach_record_index_resident(arc.data_ptr(), room, arc_size, fr.data_ptr(), n)
        t = alternating({"compress": compress, "compress_attach": compress_attach}, bc.sync, reps)
        asize = int(words[4].item())
        assert asize < (1 << 63), "a frame failed, or the attach was refused: %#x" % (asize & ((1 << 64) - 1))
        N = n + 1
        loaded = torch.zeros(N + 1, dtype=torch.int64, device="cuda"); rebuilt = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
        res = torch.zeros(8, dtype=torch.int64, device="cuda")
        h = bc.open_seekable_device(arc.data_ptr(), asize)
        assert h.num_frames == N and h.content_size == size

        def open_close():
            bc.open_seekable_device(arc.data_ptr(), asize).close()
        load = lambda: h.load_record_index_resident(loaded.data_ptr(), res.data_ptr())
        rebuild = lambda: h.index_records_resident(0, N, work.data_ptr(), size, rebuilt.data_ptr(), res.data_ptr() + 32)
        read = lambda: h.read_ranges_device([0], [size], dst.data_ptr(), [0], status.data_ptr())
        t.update(alternating({"open": open_close, "load": load}, bc.sync, reps))
        t.update(alternating({"range_read": read, "rebuild": rebuild}, bc.sync, reps))
        got = res.tolist()
        assert got[0] == 0 and got[1] == records and got[3] == n, ("load", got[:4])
        assert got[4] == 0 and got[5] == records and got[6] == 0, ("rebuild", got[4:])
        want = torch.cat([fr[:n + 1], fr[n:n + 1]])
        assert bool((loaded == want).all()) and bool((rebuilt == want).all()) and int(status.item()) == 0 and bool((dst == src).all())
        places = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(fs[:n].to(torch.int64), 0)])
        text = lambda: bc.index_records_device(src.data_ptr(), size, places.data_ptr(), n, rebuilt.data_ptr(), res.data_ptr() + 32)
        kt = kernels(text, ("k_recidx_tiles", "k_recidx_places"))
        kt.update(kernels(split, ("k_split_count", "k_split_emit")))
        bc.sync()
        assert bool((rebuilt[:n + 1] == fr[:n + 1]).all())
        row = {"frames": n, "archive_bytes": asize, "index_frame_bytes": 40 + 4 * n, "ms": {k: ms(v) for k, v in t.items()}, "kernels_ms": kt,
               "attach_ms": round((med(t["compress_attach"]) - med(t["compress"])) * 1e3, 4),
               "attach_over_compress": round((med(t["compress_attach"]) - med(t["compress"])) / med(t["compress"]), 4),
               "load_over_open": round(med(t["load"]) / med(t["open"]), 3), "rebuild_over_range_read": round(med(t["rebuild"]) / med(t["range_read"]), 3),
               "rebuild_gibs": round(gib / med(t["rebuild"]), 1), "range_read_gibs": round(gib / med(t["range_read"]), 1),
               "k_recidx_tiles_over_k_split_count": round(kt["k_recidx_tiles"][1] / kt["k_split_count"][1], 3),
               "k_recidx_places_over_k_split_emit": round(kt["k_recidx_places"][1] / kt["k_split_emit"][1], 3)}
        rep["target_%d" % T] = row
        bc.sync(); h.close()
        del arc, loaded, rebuilt
    bc.close()
    line = json.dumps(rep)
    print(line, flush=True)
    with open(a.out or os.path.join(ROOT, "profiles", "record_index_bench.jsonl"), "a") as f:
        f.write(line + "\n")


def filter_legs(a):
    """--split --filter: frame filters on the Zipf log stream (text lines, ~150 bytes each) in device memory, for the archives of targetSize
    65536 (g = 4, L = 13; then L = 16) and 4096 (g = 4, L = 10; then L = 13), three rounds of alternating legs each, all in one process:
      bytes      the filter frame's bytes over the archive's;
      build      zsmi_seekableBuildFrameFilterResident against zsmi_seekableIndexRecordsResident on the same handle - both decode the archive;
      kernels    k_filter_tiles and k_filter_check (zsmi_buildFrameFilterDevice on the text and the frames' borders, HIP events, three
                 calls: the sorted times) beside k_split_count on the same buffer; k_filter_test and k_filter_list of one filter call;
      candidates the frames zsmi_filterFramesDevice passes against the frames that truly hold a record of the answer, for a needle (the
                 first 24 bytes of one line), a rare pattern (one line in 2000), `e` and a pattern shorter than g;
      search     zsmi_filterFramesDevice and, fed by its dFrames and dResult[0] as they lie in device memory,
                 zsmi_seekableFindQueryFramesResident (maxFrames = all frames, the work bound of that many) - against
                 zsmi_seekableFindQueryResident over the whole archive for the same query; the answers are held against each other; the
                 k_findsel_* kernels of one call.
    One JSON line, also appended to profiles/frame_filter_bench.jsonl."""
    size, M, reps = (a.mib or 1024) << 20, a.frame, 3
    gib = size / float(1 << 30)
    bc = BatchCodec(0)
    src = torch.from_numpy(D.zipf_log(size)).cuda()
    words = torch.zeros(8, dtype=torch.int64, device="cuda")
    bc.count_records_device(src.data_ptr(), size, words.data_ptr()); bc.sync()
    records = int(words[0].item())
    mp = BatchCodec.split_pieces_bound(records, size, M)
    fs = torch.zeros(mp, dtype=torch.int32, device="cuda"); fr = torch.zeros(mp + 1, dtype=torch.int64, device="cuda")
    work = torch.empty(size, dtype=torch.uint8, device="cuda")
    ms = lambda v: [round(t * 1e3, 4) for t in v]
    med = lambda v: float(np.median(v))
    mid = bytes(src[size // 2:size // 2 + 4096].cpu().numpy())
    needle = mid[mid.index(b"\n") + 1:][:24].split(b"\n")[0]                # the start of one line in the middle of the stream: in a frame or two
    patterns = {"needle": needle, "rare": a.filter_patterns[0].encode(), "e": b"e", "short": a.filter_patterns[0].encode()[:3]}

    def kernels(fn, names):
        runs = []
        for _ in range(reps):
            bc.enable_timing(True); fn(); runs.append(bc.kernel_times()); bc.enable_timing(False)
        return {k: sorted(round(r[k][0] * 1e3, 4) for r in runs) for k in names}
    rep = {"metric": "frame_filter", "gib": gib, "max_frame_size": M, "records": records, "patterns": {k: v.decode("latin-1") for k, v in patterns.items()},
           "library": bc.L.zsmi_versionString().decode()}
    for T, g, Lg in ((65536, 4, 13), (4096, 4, 10), (65536, 4, 16), (4096, 4, 13)):      # the two sets the archives were planned with; then the most bits a 64 KiB frame can have, and 2 bits a byte at 4 KiB
        split = lambda: bc.split_records_device(src.data_ptr(), size, mp, fs.data_ptr(), fr.data_ptr(), words.data_ptr() + 8, target_size=T, max_frame_size=M)
        split(); bc.sync()
        n = int(words[1].item())
        room = bc.seekable_frames_resident_bound(size, n, True)
        arc = torch.empty(room, dtype=torch.uint8, device="cuda"); arc_size = words.data_ptr() + 32
        bc.compress_seekable_frames_resident(src.data_ptr(), size, fs.data_ptr(), n, M, arc.data_ptr(), room, arc_size, a.level, True); bc.sync()
        asize = int(words[4].item())
        assert asize < (1 << 63), "a frame failed: %#x" % (asize & ((1 << 64) - 1))
        h = bc.open_seekable_device(arc.data_ptr(), asize)
        fbytes = frame_filter_size(n, Lg)
        flt = torch.zeros(fbytes, dtype=torch.uint8, device="cuda"); flt_text = torch.zeros(fbytes, dtype=torch.uint8, device="cuda")
        rebuilt = torch.zeros(n + 1, dtype=torch.int64, device="cuda"); res = torch.zeros(16, dtype=torch.int64, device="cuda")
        build = lambda: h.build_frame_filter_resident(work.data_ptr(), size, flt.data_ptr(), fbytes, res.data_ptr(), gram=g, log2_bits=Lg)
        rebuild = lambda: h.index_records_resident(0, n, work.data_ptr(), size, rebuilt.data_ptr(), res.data_ptr() + 32)
        t = alternating({"index_rebuild": rebuild, "filter_build": build}, bc.sync, reps)
        got = res.tolist()
        assert got[0] == 0 and got[1] == fbytes and got[4] == 0 and got[5] == records, got[:8]
        saturated, grams = got[2], got[3]
        places = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(fs[:n].to(torch.int64), 0)])
        text = lambda: bc.build_frame_filter_device(src.data_ptr(), size, places.data_ptr(), n, flt_text.data_ptr(), fbytes, res.data_ptr() + 64, gram=g, log2_bits=Lg)
        kt = kernels(text, ("k_filter_tiles", "k_filter_check"))
        kt.update(kernels(split, ("k_split_count",)))
        bc.sync()
        assert bool((flt == flt_text).all()), "the archive's filter is not the text's"
        bc.check_frame_filter_device(flt.data_ptr(), fbytes, res.data_ptr() + 64); bc.sync()
        assert res.tolist()[8:15] == [0, n, 10, g, Lg, size, saturated]
        # the searches: the whole archive against filter -> list search, nothing read back between the two calls
        cap = records
        out_whole = torch.zeros(cap, dtype=torch.int64, device="cuda"); out_runs = torch.zeros(cap, dtype=torch.int64, device="cuda")
        frames = torch.zeros(n, dtype=torch.int32, device="cuda")
        lbound = h.find_frames_work_bound(n)
        lwork = torch.empty(lbound, dtype=torch.uint8, device="cuda")
        row_q = {}
        for name, pat in patterns.items():
            def whole():
                h.find_query_resident(fr.data_ptr(), n, [pat], 0, n, work.data_ptr(), size, out_whole.data_ptr(), 0, cap, res.data_ptr())

            def filtered():                                               # nothing comes to the host between the two calls
                bc.filter_frames_device(flt.data_ptr(), fbytes, [pat], 0, n, frames.data_ptr(), n, res.data_ptr() + 32)
                h.find_query_frames_resident(fr.data_ptr(), n, [pat], frames.data_ptr(), res.data_ptr() + 32, n, lwork.data_ptr(), lbound, out_runs.data_ptr(), 0, cap,
                                             res.data_ptr() + 64)
            tq = alternating({"whole": whole, "filtered": filtered}, bc.sync, reps)
            got = res.tolist()
            total, candidates, decoded = got[0], got[4], got[11]
            assert got[8] == total and got[9] == got[1] and bool((out_whole[:total] == out_runs[:total]).all()), (name, got[:12])
            hits = out_whole[:total]
            true_frames = int(torch.unique(torch.searchsorted(fr[:n + 1], hits, right=True) - 1).numel()) if total else 0
            kq = kernels(lambda: bc.filter_frames_device(flt.data_ptr(), fbytes, [pat], 0, n, frames.data_ptr(), n, res.data_ptr() + 32), ("k_filter_test", "k_filter_list"))
            kq.update(kernels(filtered, ("k_findsel_list", "k_findsel_code", "k_findsel_fill", "k_findsel_prefix", "k_findsel_renumber", "k_findq_count", "k_findq_emit")))
            row_q[name] = {"records_found": total, "frames_with_a_record": true_frames, "candidates": candidates, "bytes_decoded": decoded,
                           "ms": {k: ms(v) for k, v in tq.items()}, "kernels_ms": kq, "filtered_over_whole": round(med(tq["filtered"]) / med(tq["whole"]), 3)}
        rep["target_%d_L%d" % (T, Lg)] = {"frames": n, "gram": g, "log2_bits": Lg, "archive_bytes": asize, "filter_bytes": fbytes, "filter_over_archive": round(fbytes / asize, 5),
                                "saturated_frames": saturated, "grams_hashed": grams, "ms": {k: ms(v) for k, v in t.items()}, "kernels_ms": kt,
                                "build_over_index_rebuild": round(med(t["filter_build"]) / med(t["index_rebuild"]), 3),
                                "k_filter_tiles_over_k_split_count": round(kt["k_filter_tiles"][1] / kt["k_split_count"][1], 3),
                                "k_filter_tiles_gibs": round(gib / (kt["k_filter_tiles"][1] * 1e-3), 1), "queries": row_q}
        bc.sync(); h.close()
        del arc, flt, flt_text, out_whole, out_runs, lwork
    bc.close()
    line = json.dumps(rep)
    print(line, flush=True)
    with open(a.out or os.path.join(ROOT, "profiles", "frame_filter_bench.jsonl"), "a") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filter", action="store_true", help="with --split: frame filters - build, kernels, candidates and the filtered search against the whole one (filter_legs' docstring)")
    ap.add_argument("--filter-patterns", nargs="+", default=["ERROR ienwbvuzw"], help="with --split --filter: the rare pattern (its first three bytes are the short one)")
    ap.add_argument("--record-index", action="store_true", help="with --split: the record index - attach, load and rebuild against the calls they follow or replace (record_index_legs' docstring)")
    ap.add_argument("--find-regex", action="store_true", help="with --split: find records by regular expression against the literal searches and re on the host (find_regex_legs' docstring)")
    ap.add_argument("--find-query", action="store_true", help="with --split: find records by several patterns against the single-pattern calls (find_query_legs' docstring)")
    ap.add_argument("--find", nargs="+", default=None, help="with --split: find records by content, a leg set a pattern (a rare one and one most lines hold)")
    ap.add_argument("--find-targets", type=int, nargs="+", default=[4096, 65536], help="with --split --find: the archives' targetSizes")
    ap.add_argument("--out", default=None, help="with --split --find: the file the JSON lines are appended to (default profiles/find_records_bench.jsonl)")
    ap.add_argument("--lines", action="store_true", help="with --split: lines by number from the split text's archive, zsmi_seekableReadRecordsResident against today's way")
    ap.add_argument("--line-targets", type=int, nargs="+", default=[4096, 65536, 1 << 20], help="with --split --lines: the targetSizes")
    ap.add_argument("--split", action="store_true", help="the record splitter on the text stream: the call, its kernels, k_index_count / k_index_emit on the same buffer")
    ap.add_argument("--target", type=int, default=4096, help="with --split: the targetSize of the second leg")
    ap.add_argument("--index", action="store_true", help="streams without a table: zsmi_openFramesDevice against zsmi_openSeekableDevice, reads through both, the stream as one item")
    ap.add_argument("--index-one-item", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--record-mib", type=int, default=256, help="with --index: MiB of 1 KiB record frames")
    ap.add_argument("--one-item-limit", type=int, default=240, help="with --index: seconds the one-item leg may take")
    ap.add_argument("--mib", type=int, default=0, help="content: 1024 MiB, or 256 MiB with --records")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frame", type=int, default=65536)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--range-bytes", type=int, default=4096)
    ap.add_argument("--records", action="store_true", help="record archives: one frame per record with dictionaries against 64 KiB fixed frames")
    ap.add_argument("--record-bytes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--resident", action="store_true", help="with --records: the device-resident write and fetch against the host-array calls")
    a = ap.parse_args()
    if a.index_one_item:
        return index_one_item(a)
    if a.index:
        return index_legs(a)
    if a.split:
        if a.filter:
            return filter_legs(a)
        if a.record_index:
            return record_index_legs(a)
        if a.find_query:
            return find_query_legs(a)
        if a.find_regex:
            return find_regex_legs(a)
        return find_legs(a) if a.find else (lines_legs(a) if a.lines else split_legs(a))
    if a.records:
        return records(a)
    a.mib = a.mib or 1024
    size, F, level = a.mib << 20, a.frame, a.level
    gib = size / float(1 << 30)
    data = D.zipf_log(size)
    bc = BatchCodec(0)
    L = bc.L
    src = torch.from_numpy(data).cuda()
    n = (size + F - 1) // F
    so = np.arange(n, dtype=np.uint64) * F
    ss = np.minimum(F, size - so).astype(np.uint32)
    bF = int(L.zsmi_compressBound(F))
    batch_out = torch.empty(n * bF, dtype=torch.uint8, device="cuda")
    batch_sizes = torch.zeros(n, dtype=torch.int32, device="cuda")
    bound = bc.seekable_bound(size, F, True)
    arc = torch.empty(bound, dtype=torch.uint8, device="cuda")
    arc_size = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    do = np.arange(n, dtype=np.uint64) * bF
    t_batch_c = timed(lambda: bc.compress_device(src.data_ptr(), so, ss, batch_out.data_ptr(), do, batch_sizes.data_ptr(), level), bc.sync, a.reps)
    t_seek_c = timed(lambda: bc.compress_seekable_device(src.data_ptr(), size, arc.data_ptr(), bound, arc_size.data_ptr(), level, F, True), bc.sync, a.reps)
    asize = int(arc_size.item())
    assert asize < (1 << 63), "a frame failed"
    host_arc = arc[:asize].cpu().numpy().tobytes()
    sa = SeekableArchive(host_arc)
    assert sa.num_frames == n and sa.content_size == size
    bs = batch_sizes.cpu().numpy().view(np.uint32)
    info = [sa.frame_info(i) for i in range(n)]
    assert all(info[i][2] == bs[i] for i in range(n)), "seekable frames differ from the batch frames"
    # kernels of one call each
    bc.enable_timing(True)
    bc.compress_seekable_device(src.data_ptr(), size, arc.data_ptr(), bound, arc_size.data_ptr(), level, F, True)
    kt_c = bc.kernel_times()
    # decode: the same frames through the batch call, and the archive whole
    fo = np.array([i[0] for i in info], dtype=np.uint64); fs = np.array([i[2] for i in info], dtype=np.uint32)
    out_batch = torch.empty(size, dtype=torch.uint8, device="cuda")
    out_seek = torch.empty(size, dtype=torch.uint8, device="cuda")
    dsz = torch.zeros(n, dtype=torch.int32, device="cuda")
    status = torch.ones(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bc.enable_timing(False)
    t_batch_d = timed(lambda: bc.decompress_device(arc.data_ptr(), fo, fs, out_batch.data_ptr(), so, ss, dsz.data_ptr()), bc.sync, a.reps)
    t_seek_d = timed(lambda: bc.decompress_seekable_device(arc.data_ptr(), asize, 0, size, out_seek.data_ptr(), status.data_ptr()), bc.sync, a.reps)
    bc.enable_timing(True)
    bc.decompress_seekable_device(arc.data_ptr(), asize, 0, size, out_seek.data_ptr(), status.data_ptr())
    kt_d = bc.kernel_times()
    bc.enable_timing(False)
    assert int(status.item()) == 0 and torch.equal(out_seek, src) and torch.equal(out_batch, src), "decoded content differs"
    # 4 KiB from the middle, one-shot
    mid = size // 2 + 1000
    lat = []
    for _ in range(max(a.reps, 20) + 3):
        t = time.perf_counter(); got = sa.read(mid, 4096); lat.append(time.perf_counter() - t)
    assert got == data[mid:mid + 4096].tobytes()
    frames_4k = sum(1 for i in info if i[1] < mid + 4096 and i[1] + i[3] > mid)
    # N short reads through an opened archive: one call, N single calls, and the whole archive as one range
    N, B = a.ranges, a.range_bytes
    offs = np.random.default_rng(7).integers(0, size - B, N).astype(np.uint64)
    lens = np.full(N, B, dtype=np.uint64)
    place = np.arange(N, dtype=np.uint64) * B
    out_r = torch.zeros(N * B, dtype=torch.uint8, device="cuda")
    st_r = torch.ones(N, dtype=torch.int32, device="cuda")
    want_r = src[(torch.from_numpy(offs.astype(np.int64)).cuda()[:, None] + torch.arange(B, device="cuda")[None, :]).reshape(-1)]
    torch.cuda.synchronize()
    h = bc.open_seekable_device(arc.data_ptr(), asize)
    assert h.num_frames == n and h.content_size == size and h.device_bytes == 0
    frames_r = [0]
    def one_call():
        frames_r[0] = h.read_ranges_device(offs, lens, out_r.data_ptr(), place, st_r.data_ptr())[1]
    t_ranges = timed(one_call, bc.sync, a.reps)
    assert not st_r.any().item() and torch.equal(out_r, want_r), "the batch of ranges differs from the content"
    out_r.zero_()
    def single_calls():
        for i in range(N):
            bc.decompress_seekable_device(arc.data_ptr(), asize, int(offs[i]), B, out_r.data_ptr() + i * B, status.data_ptr())
    t_singles = timed(single_calls, bc.sync, min(a.reps, 3))
    assert torch.equal(out_r, want_r), "the single reads differ from the content"
    out_seek.zero_()
    t_whole = timed(lambda: h.read_ranges_device([0], [size], out_seek.data_ptr(), [0], status.data_ptr()), bc.sync, a.reps)
    assert int(status.item()) == 0 and torch.equal(out_seek, src), "the archive as one range differs from the content"
    h.close()
    rgib = N * B / float(1 << 30)
    ms = lambda kt, k: round(kt.get(k, (0.0, 0))[0] * 1e3, 4)
    rep = {"metric": "seekable", "gib": gib, "frame": F, "level": level, "frames": n, "archive_bytes": asize, "ratio": round(size / asize, 4),
           "compress_batch_gibs": round(gib / t_batch_c, 2), "compress_seekable_gibs": round(gib / t_seek_c, 2),
           "compress_ratio_to_batch": round(t_batch_c / t_seek_c, 3),
           "decode_batch_gibs": round(gib / t_batch_d, 2), "decode_seekable_gibs": round(gib / t_seek_d, 2),
           "decode_ratio_to_batch": round(t_batch_d / t_seek_d, 3),
           "k_seek_hash_ms": ms(kt_c, "k_seek_hash"), "k_seek_hash_ms_per_gib": round(ms(kt_c, "k_seek_hash") / gib, 4),
           "k_seek_verify_ms": ms(kt_d, "k_seek_verify"),
           "compress_kernels_ms": {k: round(v[0] * 1e3, 4) for k, v in kt_c.items()},
           "decode_kernels_ms": {k: round(v[0] * 1e3, 4) for k, v in kt_d.items()},
           "read_4k_ms_median": round(float(np.median(lat[3:])) * 1e3, 4), "read_4k_ms_min": round(float(np.min(lat[3:])) * 1e3, 4),
           "read_4k_frames": frames_4k,
           "ranges": N, "range_bytes": B, "ranges_frames_decoded": frames_r[0],
           "ranges_one_call_ms": round(t_ranges * 1e3, 4), "ranges_one_call_gibs": round(rgib / t_ranges, 3),
           "ranges_single_calls_ms": round(t_singles * 1e3, 3), "ranges_single_calls_gibs": round(rgib / t_singles, 4),
           "ranges_one_call_speedup": round(t_singles / t_ranges, 1),
           "whole_as_one_range_ms": round(t_whole * 1e3, 3), "whole_as_one_range_gibs": round(gib / t_whole, 2)}
    bc.close()
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
