#!/usr/bin/env python3
"""Dictionary training on the GPU (zsmi_trainFromBuffer: fastCover, d = 8, 4 k steps, split 0.75, level 3) against libzstd's CPU trainer.
One JSON line per case: json_records and binary_table at 3, 24 and 256 MiB of 1 - 4 KiB samples (the class generators of tests/_corpus.py,
in 8 MiB pieces at seeds 1011.. / 1014..).  Each line: the GPU train time (search and finalize included; median of --reps after a warm-up
call), the kernel times of one call (zsmi_enableKernelTiming), the held-out total (tests/_train.py's chunks, compressed by this library at
level 3) with our dictionary, with libzstd's and with none; where libzstd is present its ZDICT_trainFromBuffer time and its
ZDICT_optimizeTrainFromBuffer_fastCover time with 16 threads (d = 8, steps 4, as ours).
usage: python tools/bench_train.py [--sizes 3,24,256] [--classes json_records,binary_table] [--reps 3]"""
import argparse, ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _corpus as C
import _train as T
import _batch as B
from _hip import hip_of

SEEDS = {"json_records": 1011, "binary_table": 1014}


def class_bytes(cls, mib):
    piece = 8 << 20
    parts, seed, have = [], SEEDS[cls], 0
    while have < (mib << 20):
        n = min(piece, (mib << 20) - have)
        parts.append(getattr(C, cls)(n, seed=seed)[:n]); seed += 100; have += n
    return b"".join(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3,24,256")
    ap.add_argument("--classes", default="json_records,binary_table")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--capacity", type=int, default=65536)
    a = ap.parse_args()
    from zstandard_amd import _lib, BatchCodec
    L = _lib.lib()
    Z = T.zdict()
    bc = BatchCodec(0)
    H = hip_of()
    cap = a.capacity
    for cls in a.classes.split(","):
        held = T.held_out(cls)
        src, ho, hs = B.batch(held)

        def held_total(dic):
            _, _, dsz = bc.compress_host(src, ho, hs, 3, dic)
            return int(dsz.astype(np.uint64).sum())
        none = held_total(b"")
        for mib in (int(s) for s in a.sizes.split(",")):
            parts = T.cut(class_bytes(cls, mib), 5)
            buf, ssz = T.flat(parts)
            out = ctypes.create_string_buffer(cap)
            times = []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                n = L.zsmi_trainFromBuffer(out, cap, buf, ssz, len(parts))
                times.append(time.perf_counter() - t0)
                if L.zsmi_isError(n):
                    raise SystemExit(f"zsmi_trainFromBuffer: {L.zsmi_getErrorName(n).decode()}")
            ours = out.raw[:n]
            # kernel times of one call of the device form (samples already in device memory), same parameters
            dptr = ctypes.c_void_p()
            assert H.hipMalloc(ctypes.byref(dptr), len(buf) + 64) == 0 and H.hipMemcpy(dptr, buf, len(buf), 1) == 0
            ss = np.array([len(x) for x in parts], dtype=np.uint32)
            so = B.layout(ss)
            bc.enable_timing(True)
            t0 = time.perf_counter()
            dev, kk, dd = bc.train_device(dptr.value, so, ss, cap, d=8, steps=4, split_point=0.75, level=3)
            dev_s = time.perf_counter() - t0
            kt = bc.kernel_times()
            bc.enable_timing(False)
            H.hipFree(dptr)
            line = {"class": cls, "samples_mib": mib, "samples": len(parts), "capacity": cap, "gpu_train_s": round(float(np.median(times[1:])), 4),
                    "gpu_train_first_call_s": round(times[0], 4), "device_form_timed_s": round(dev_s, 4), "k": kk, "d": dd, "identical_forms": dev == ours,
                    "kernels_ms": {k: round(v[0] * 1e3, 3) for k, v in sorted(kt.items(), key=lambda kv: -kv[1][0])},
                    "held_out": {"ours": held_total(ours), "none": none}}
            if Z:
                zo = ctypes.create_string_buffer(cap)
                t0 = time.perf_counter(); r = Z.ZDICT_trainFromBuffer(zo, cap, buf, ssz, len(parts)); t1 = time.perf_counter()
                zdic = zo.raw[:r]
                zp = T.ZFastCover(k=0, d=8, f=20, steps=4, nbThreads=16, splitPoint=0.75, accel=1, zParams=T.ZParams(3, 0, 0))
                zo2 = ctypes.create_string_buffer(cap)
                t2 = time.perf_counter(); Z.ZDICT_optimizeTrainFromBuffer_fastCover(zo2, cap, buf, ssz, len(parts), ctypes.byref(zp)); t3 = time.perf_counter()
                line["libzstd_trainFromBuffer_s"] = round(t1 - t0, 4)
                line["libzstd_optimize_fastCover_16t_s"] = round(t3 - t2, 4)
                line["held_out"]["libzstd_dict"] = held_total(zdic)
                line["held_out"]["ours_over_libzstd"] = round(line["held_out"]["ours"] / line["held_out"]["libzstd_dict"], 4)
                line["speedup_vs_libzstd_1t"] = round((t1 - t0) / line["gpu_train_s"], 2)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
