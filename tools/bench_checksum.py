#!/usr/bin/env python3
"""GPU box: what the checksum parameter costs a compress call (device-resident, per-call wall time, like tools/bench_dict.py).
One JSON line per shape - chunks x chunk size of a Zipf log, the bench workload's data: 4096 x 64 KiB (bench.py's own shape), 32768 x 1 KiB,
2048 x 128 KiB, 256 x 1 MiB.  The same chunks, the same process and context, flag off and flag on ALTERNATING, --repeats timings of --steps
calls each: comp_gib_s_off / comp_gib_s_on are the medians as rates, *_min / *_max the slowest and fastest repeat, spread_* their
(max - min) / median, on_over_off the ratio of the medians, and apart says that the flag-on call's fastest repeat was slower than the
flag-off call's slowest (the difference is beyond both spreads).  checksum_kernel_ms: k_frame_checksum of one flag-on call
(zsmi_enableKernelTiming), with the call's other kernels in kernels_ms_on.  Before anything is timed the flag-on frames are checked: each is
the flag-off frame with bit 2 of byte 4 set and 4 more bytes, and the first and last decode under oracle D (which verifies the checksum)."""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import _data as D, _oracle as O
from zstandard_amd import BatchCodec, _lib

SHAPES = "4096x65536,32768x1024,2048x131072,256x1048576"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="chunks x chunk size, comma separated")
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    bc = BatchCodec(device=0); Z = _lib.lib()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    data = D.zipf_log(max(n * cs for n, cs in shapes), seed_lo=0x5EED, threads=min(16, os.cpu_count() or 1))
    dsrc = torch.from_numpy(data).to(dev)
    for n, cs in shapes:
        off = np.arange(n, dtype=np.uint64) * cs; sz = np.full(n, cs, dtype=np.uint32)
        bound = int(Z.zsmi_compressBound(cs)); doff = np.arange(n, dtype=np.uint64) * bound
        ddst = torch.empty(n * bound, dtype=torch.uint8, device=dev); dsz = torch.empty(n, dtype=torch.int32, device=dev)
        run = lambda: bc.compress_device(dsrc.data_ptr(), off, sz, ddst.data_ptr(), doff, dsz.data_ptr(), a.level)
        rec = {"chunks": n, "chunk": cs, "level": a.level, "steps": a.steps, "repeats": a.repeats, "library": Z.zsmi_versionString().decode()}
        # the frames, before anything is timed (and both forms warmed up)
        got = {}
        for flag in (0, 1):
            bc.set_parameter("checksum", flag)
            for _ in range(2):
                run()
            bc.sync()
            sizes = dsz.cpu().numpy().view(np.uint32).copy()
            assert (sizes < 0xFFFFFF88).all()
            k = min(n, 64)
            host = ddst[:k * bound].cpu().numpy()
            got[flag] = (sizes, [host[int(doff[i]):int(doff[i]) + int(sizes[i])].tobytes() for i in range(k)])
        assert (got[1][0] == got[0][0] + 4).all()
        for f0, f1 in zip(got[0][1], got[1][1]):
            assert f1[:-4] == f0[:4] + bytes([f0[4] | 4]) + f0[5:]
        for i in (0, len(got[1][1]) - 1):
            assert O.decompress(got[1][1][i], cs) == data[i * cs:(i + 1) * cs].tobytes()
        rec["ratio_off"] = round(n * cs / float(got[0][0].sum()), 4); rec["ratio_on"] = round(n * cs / float(got[1][0].sum()), 4)
        times = {0: [], 1: []}
        for _ in range(a.repeats):
            for flag in (0, 1):
                bc.set_parameter("checksum", flag)
                bc.sync(); t0 = time.perf_counter()
                for _ in range(a.steps):
                    run()
                bc.sync(); times[flag].append((time.perf_counter() - t0) / a.steps)
        gib = n * cs / 2**30
        for flag, tag in ((0, "off"), (1, "on")):
            t = times[flag]; dt = float(np.median(t))
            rec["comp_gib_s_" + tag] = round(gib / dt, 2); rec["comp_ms_" + tag] = round(dt * 1e3, 4)
            rec["comp_gib_s_%s_min" % tag] = round(gib / max(t), 2); rec["comp_gib_s_%s_max" % tag] = round(gib / min(t), 2)
            rec["spread_" + tag] = round((max(t) - min(t)) / dt, 3)
        rec["on_over_off"] = round(rec["comp_gib_s_on"] / rec["comp_gib_s_off"], 4)
        rec["apart"] = bool(min(times[1]) > max(times[0]))
        for flag, tag in ((0, "off"), (1, "on")):
            bc.set_parameter("checksum", flag)
            bc.enable_timing(True); run(); bc.sync()
            rec["kernels_ms_" + tag] = {k2: round(v[0] * 1e3, 4) for k2, v in bc.kernel_times().items()}
            bc.enable_timing(False)
        assert "k_frame_checksum" not in rec["kernels_ms_off"]
        rec["checksum_kernel_ms"] = rec["kernels_ms_on"]["k_frame_checksum"]
        bc.set_parameter("checksum", 0)
        print(json.dumps(rec), flush=True)
        del ddst, dsz
    bc.close()


if __name__ == "__main__":
    main()
