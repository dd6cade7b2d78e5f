#!/usr/bin/env python3
"""GPU box: zsmi_compressBatchResident against zsmi_compressBatchDevice on the same chunks of the Zipf log, level 3 - the bench workload
(4096 x 64 KiB), 32768 x 1 KiB, 2048 x 128 KiB, and a SKEWED call: 4096 chunks of which every 64th is 1 MiB and the rest 4 KiB, told
maxSrcSize = 1 MiB (the price of a loose bound).  One JSON line per workload, appended to --out (profiles/resident_compress_bench.jsonl):
  leg (a)  zsmi_compressBatchDevice, the three descriptor arrays from the host (the layout repeats: its plan is reused);
  leg (b)  zsmi_compressBatchResident, the same arrays in device memory, maxSrcSize = the largest chunk: the plan is built every call.
The legs run in the same process and context, ALTERNATING, --repeats timings of --steps calls each, every repeat under its own time limit
(--limit seconds: a repeat that passes it ends the tool; nothing more is started on the device).  gib_s_a / _b are the medians as rates of
input bytes, *_min / *_max the slowest and fastest repeat, spread_* their (max - min) / median, b_over_a the ratio of the medians,
b_below_a says that (b)'s fastest repeat was slower than (a)'s slowest.  kernels_ms_a / _b: the kernels of one call (zsmi_getKernelTimes),
plan_ms: the sum of (b)'s k_plan_* kernels, plan_kernels_ms each of them.  Before anything is timed the size words and every byte of
the destination of the two legs are compared.
--cdict-set K: the dictionary forms instead - (a) zsmi_compressBatchDevice_usingCDictSet with the choice from the host (layout and choice
repeat: its plan is reused), (b) zsmi_compressBatchResident_usingCDictSet with the choice in device memory; a set of K members digested
from the trained dictionaries of tests/golden/libzstd_fixtures_dict_compress.npz (the Zipf log's first, then the other record classes',
in turn), chunk i with member i % K.  Its workloads: 32768 x 1 KiB, 8192 x 4 KiB, 512 x 64 KiB; its lines go to
profiles/resident_cdict_set_bench.jsonl."""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import _data as D
from bench_resident import Limit, kernels
from zstandard_amd import BatchCodec, CompressionDict, CompressionDictSet

SET_WORKLOADS = "32768x1KiB,8192x4KiB,512x64KiB"
SET_CLASSES = ("zipf", "json_records", "xml_records", "csv_records", "binary_table")


def make_set(bc, k, level):
    """a CompressionDictSet of k members (a CDict each, the trained dictionaries in turn) and the members"""
    fix = np.load(os.path.join(D.GOLDEN, "libzstd_fixtures_dict_compress.npz"))
    cds = [CompressionDict(bc, fix["trained_" + SET_CLASSES[i % len(SET_CLASSES)]].tobytes(), level) for i in range(k)]
    return CompressionDictSet(bc, cds, level), cds


WORKLOADS = {
    "4096x64KiB": lambda: np.full(4096, 65536, dtype=np.uint32),
    "32768x1KiB": lambda: np.full(32768, 1024, dtype=np.uint32),
    "2048x128KiB": lambda: np.full(2048, 131072, dtype=np.uint32),
    "8192x4KiB": lambda: np.full(8192, 4096, dtype=np.uint32),
    "512x64KiB": lambda: np.full(512, 65536, dtype=np.uint32),
    "skewed": lambda: np.where(np.arange(4096) % 64 == 31, 1 << 20, 4096).astype(np.uint32),
}


def stats(times, gib, tag, rec):
    dt = float(np.median(times))
    rec["gib_s_" + tag] = round(gib / dt, 2); rec["ms_" + tag] = round(dt * 1e3, 4)
    rec["gib_s_%s_min" % tag] = round(gib / max(times), 2); rec["gib_s_%s_max" % tag] = round(gib / min(times), 2)
    rec["spread_" + tag] = round((max(times) - min(times)) / dt, 3)


def dev_of(x, dev):
    return torch.from_numpy(x.view(np.int64 if x.dtype == np.uint64 else np.int32).copy()).to(dev)


def workload(bc, a, name, dev):
    Z = bc.L
    sizes = WORKLOADS[name]()
    n, total, max_src = len(sizes), int(sizes.sum(dtype=np.uint64)), int(sizes.max())
    data = D.zipf_log(total, seed_lo=0x5EED, threads=min(16, os.cpu_count() or 1))
    d_src = torch.from_numpy(data).to(dev)
    offs = (np.cumsum(sizes, dtype=np.uint64) - sizes).astype(np.uint64)
    strides = np.array([(int(Z.zsmi_compressBound(int(s))) + 255) // 256 * 256 for s in np.unique(sizes)], dtype=np.uint64)
    stride_of = dict(zip(np.unique(sizes).tolist(), strides.tolist()))
    room = np.array([stride_of[int(s)] for s in sizes], dtype=np.uint64)
    foffs = (np.cumsum(room, dtype=np.uint64) - room).astype(np.uint64)
    d_offs, d_sizes, d_foffs = dev_of(offs, dev), dev_of(sizes, dev), dev_of(foffs, dev)
    d_frames = {t: torch.empty(int(room.sum()), dtype=torch.uint8, device=dev) for t in "ab"}
    d_fsz = {t: torch.zeros(n, dtype=torch.int32, device=dev) for t in "ab"}
    torch.cuda.synchronize()                                        # (the codec has a stream of its own)
    cset, index = None, None
    if a.cdict_set:
        cset, cds = make_set(bc, a.cdict_set, a.level)
        index = (np.arange(n) % a.cdict_set).astype(np.uint32)
        d_index = dev_of(index, dev)
        torch.cuda.synchronize()
    legs = {
        "a": lambda: bc.compress_device(d_src.data_ptr(), offs, sizes, d_frames["a"].data_ptr(), foffs, d_fsz["a"].data_ptr(), a.level),
        "b": lambda: bc.compress_resident(d_src.data_ptr(), d_offs.data_ptr(), d_sizes.data_ptr(), n, max_src, d_frames["b"].data_ptr(), d_foffs.data_ptr(),
                                          d_fsz["b"].data_ptr(), a.level),
    }
    if cset is not None:
        legs = {
            "a": lambda: bc.compress_device(d_src.data_ptr(), offs, sizes, d_frames["a"].data_ptr(), foffs, d_fsz["a"].data_ptr(), cdict_set=cset, dict_index=index),
            "b": lambda: bc.compress_resident(d_src.data_ptr(), d_offs.data_ptr(), d_sizes.data_ptr(), n, max_src, d_frames["b"].data_ptr(), d_foffs.data_ptr(),
                                              d_fsz["b"].data_ptr(), cdict_set=cset, d_dict_index_ptr=d_index.data_ptr()),
        }
    rec = {"workload": name, "chunks": n, "bytes": total, "max_src_size": max_src, "level": a.level, "steps": a.steps, "repeats": a.repeats,
           "library": Z.zsmi_versionString().decode()}
    if cset is not None:
        rec["cdict_set"] = a.cdict_set
    for tag, run in legs.items():                                   # both legs warmed up, their results compared before anything is timed
        with Limit(a.limit, "check of leg " + tag):
            d_frames[tag].zero_(); d_fsz[tag].zero_(); torch.cuda.synchronize()
            for _ in range(2):
                run()
            bc.sync()
    fsz = d_fsz["a"].cpu().numpy().view(np.uint32)
    assert (fsz < 0xFFFFFF88).all() and torch.equal(d_fsz["a"], d_fsz["b"]), "the legs' size words differ"
    assert torch.equal(d_frames["a"], d_frames["b"]), "the legs' frames differ"
    rec["ratio"] = round(total / float(fsz.sum(dtype=np.uint64)), 4)
    times = {"a": [], "b": []}
    for r in range(a.repeats):
        for tag, run in legs.items():
            with Limit(a.limit, "repeat %d of leg %s" % (r, tag)):
                bc.sync(); t0 = time.perf_counter()
                for _ in range(a.steps):
                    run()
                bc.sync(); times[tag].append((time.perf_counter() - t0) / a.steps)
    gib = total / 2**30
    for tag in legs:
        stats(times[tag], gib, tag, rec)
    rec["b_over_a"] = round(rec["gib_s_b"] / rec["gib_s_a"], 4)
    rec["b_below_a"] = bool(min(times["b"]) > max(times["a"]))
    with Limit(a.limit, "kernel times"):
        rec["kernels_ms_a"] = kernels(bc, legs["a"]); rec["kernels_ms_b"] = kernels(bc, legs["b"])
    rec["plan_kernels_ms"] = {k: v for k, v in rec["kernels_ms_b"].items() if k.startswith("k_plan_")}
    rec["plan_ms"] = round(sum(v for k, v in rec["kernels_ms_b"].items() if k.startswith("k_plan_")), 4)
    if cset is not None:
        bc.sync(); cset.close()
        for cd in cds:
            cd.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=None, help="comma separated, of: " + ", ".join(WORKLOADS) + " (default: all but the two below; with --cdict-set: " + SET_WORKLOADS + ")")
    ap.add_argument("--cdict-set", type=int, default=0, metavar="K", help="the dictionary forms, with a set of K members")
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds a repeat (or a check) may take")
    ap.add_argument("--out", default=None, help="default: profiles/resident_compress_bench.jsonl, with --cdict-set profiles/resident_cdict_set_bench.jsonl")
    a = ap.parse_args()
    a.workloads = a.workloads or (SET_WORKLOADS if a.cdict_set else "4096x64KiB,32768x1KiB,2048x128KiB,skewed")
    a.out = a.out or os.path.join(ROOT, "profiles", "resident_cdict_set_bench.jsonl" if a.cdict_set else "resident_compress_bench.jsonl")
    dev = torch.device("cuda:0")
    bc = BatchCodec(device=0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for name in a.workloads.split(","):
            line = json.dumps(workload(bc, a, name, dev))
            print(line, flush=True); out.write(line + "\n"); out.flush()
            torch.cuda.empty_cache()
    bc.close()


if __name__ == "__main__":
    main()
