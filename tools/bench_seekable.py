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
  python tools/bench_seekable.py [--mib 1024] [--reps 10] [--frame 65536] [--ranges 4096] [--range-bytes 4096]"""
import argparse, json, os, sys, time
import torch                                               # before libzsmi.so
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _data as D
from zstandard_amd import BatchCodec, SeekableArchive


def timed(fn, sync, reps):
    fn(); sync()                                           # warm-up: plans, scratch
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); sync(); ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frame", type=int, default=65536)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--range-bytes", type=int, default=4096)
    a = ap.parse_args()
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
