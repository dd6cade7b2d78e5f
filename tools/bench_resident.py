#!/usr/bin/env python3
"""GPU box: zsmi_decompressBatchResident against zsmi_decompressBatchDevice on the same frames - the README's decode workloads, 57344 and
8192 frames of 32 KiB of the Zipf log built by this codec's encoder (--million: 1 048 576 frames as well, on a box with the memory).
One JSON line per workload, appended to --out (profiles/resident_bench.jsonl):
  leg (a)  zsmi_decompressBatchDevice, the four descriptor arrays from the host;
  leg (b)  zsmi_decompressBatchResident, the same arrays in device memory, maxDstCap = the chunk size.
The legs run in the same process and context, ALTERNATING, --repeats timings of --steps calls each, every repeat under its own time limit
(--limit seconds: a repeat that passes it ends the tool; nothing more is started on the device).  dec_gib_s_a / _b are the medians as
rates of output bytes, *_min / *_max the slowest and fastest repeat, spread_* their (max - min) / median, b_over_a the ratio of the
medians, b_below_a says that (b)'s fastest repeat was slower than (a)'s slowest.  kernels_ms_b: the kernels of one (b) call with
k_dec_items among them; sizes_ms / layout_ms: k_frame_sizes and the layout kernel over the same items (zsmi_getKernelTimes).
--layout-items N (with no workload: --frames ""): the layout kernel alone over N sizes, the single-workgroup scan at scale.
Before anything is timed both legs' outputs are compared with the input, and the sizes and layout with the chunk sizes."""
import argparse, json, os, signal, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import _data as D
from zstandard_amd import BatchCodec, _lib


class Limit:
    """a wall-clock limit around one repeat: passing it ends the process at once (a hung device call is not waited for)"""
    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        def fire(*_):
            sys.stderr.write("time limit passed: %s\n" % self.what); sys.stderr.flush(); os._exit(3)
        signal.signal(signal.SIGALRM, fire); signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)


def stats(times, gib, tag, rec):
    dt = float(np.median(times))
    rec["dec_gib_s_" + tag] = round(gib / dt, 2); rec["dec_ms_" + tag] = round(dt * 1e3, 4)
    rec["dec_gib_s_%s_min" % tag] = round(gib / max(times), 2); rec["dec_gib_s_%s_max" % tag] = round(gib / min(times), 2)
    rec["spread_" + tag] = round((max(times) - min(times)) / dt, 3)


def kernels(bc, run):
    bc.enable_timing(True); run(); bc.sync()
    out = {k: round(v[0] * 1e3, 4) for k, v in bc.kernel_times().items()}
    bc.enable_timing(False)
    return out


def workload(bc, a, n, cs, dev):
    Z = bc.L
    data = D.zipf_log(n * cs, seed_lo=0x5EED, threads=min(16, os.cpu_count() or 1))
    d_src = torch.from_numpy(data).to(dev)
    bound = int(Z.zsmi_compressBound(cs)); stride = (bound + 255) // 256 * 256
    offs = np.arange(n, dtype=np.uint64) * cs; sizes = np.full(n, cs, dtype=np.uint32); foffs = np.arange(n, dtype=np.uint64) * stride
    d_frames = torch.empty(n * stride, dtype=torch.uint8, device=dev); d_fsz = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()                                        # (the codec has a stream of its own)
    bc.compress_device(d_src.data_ptr(), offs, sizes, d_frames.data_ptr(), foffs, d_fsz.data_ptr(), 3); bc.sync()
    fsz = d_fsz.cpu().numpy().view(np.uint32).copy()
    assert (fsz < 0xFFFFFF88).all()
    # the descriptors in device memory, as an earlier GPU step would have left them
    d_foffs, d_offs, d_caps = (torch.from_numpy(x.view(np.int64 if x.dtype == np.uint64 else np.int32).copy()).to(dev) for x in (foffs, offs, sizes))
    d_out = torch.empty(n * cs, dtype=torch.uint8, device=dev); d_osz = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    legs = {
        "a": lambda: bc.decompress_device(d_frames.data_ptr(), foffs, fsz, d_out.data_ptr(), offs, sizes, d_osz.data_ptr()),
        "b": lambda: bc.decompress_resident(d_frames.data_ptr(), d_foffs.data_ptr(), d_fsz.data_ptr(), n, d_out.data_ptr(), d_offs.data_ptr(), d_caps.data_ptr(), cs, d_osz.data_ptr()),
    }
    rec = {"frames": n, "chunk": cs, "steps": a.steps, "repeats": a.repeats, "library": Z.zsmi_versionString().decode()}
    for tag, run in legs.items():                                   # the outputs, before anything is timed (and both legs warmed up)
        with Limit(a.limit, "check of leg " + tag):
            d_out.zero_(); d_osz.zero_(); torch.cuda.synchronize()
            for _ in range(2):
                run()
            bc.sync()
            assert (d_osz.cpu().numpy() == cs).all() and torch.equal(d_out, d_src), "leg %s: decoded bytes differ from the input" % tag
    # sizes and layout over the same items
    d_content = torch.zeros(n, dtype=torch.int64, device=dev); d_status = torch.ones(n, dtype=torch.int32, device=dev)
    d_lcaps = torch.zeros(n, dtype=torch.int32, device=dev); d_loffs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    sizes_run = lambda: bc.frame_sizes_device(d_frames.data_ptr(), d_foffs.data_ptr(), d_fsz.data_ptr(), n, d_content.data_ptr(), 0, d_status.data_ptr())
    layout_run = lambda: bc.layout_outputs_device(d_content.data_ptr(), d_status.data_ptr(), n, d_lcaps.data_ptr(), d_loffs.data_ptr(), align=1)
    with Limit(a.limit, "sizes and layout"):
        torch.cuda.synchronize()
        for _ in range(2):
            sizes_run(); layout_run()
        bc.sync()
        assert (d_content.cpu().numpy() == cs).all() and not d_status.cpu().numpy().any()
        assert (d_lcaps.cpu().numpy() == cs).all() and (d_loffs.cpu().numpy() == np.arange(n + 1, dtype=np.int64) * cs).all()
        rec["sizes_ms"] = kernels(bc, sizes_run)["k_frame_sizes"]; rec["layout_ms"] = kernels(bc, layout_run)["k_layout_outputs"]
    times = {"a": [], "b": []}
    for r in range(a.repeats):
        for tag, run in legs.items():
            with Limit(a.limit, "repeat %d of leg %s" % (r, tag)):
                bc.sync(); t0 = time.perf_counter()
                for _ in range(a.steps):
                    run()
                bc.sync(); times[tag].append((time.perf_counter() - t0) / a.steps)
    gib = n * cs / 2**30
    for tag in legs:
        stats(times[tag], gib, tag, rec)
    rec["b_over_a"] = round(rec["dec_gib_s_b"] / rec["dec_gib_s_a"], 4)
    rec["b_below_a"] = bool(min(times["b"]) > max(times["a"]))
    with Limit(a.limit, "kernel times"):
        rec["kernels_ms_a"] = kernels(bc, legs["a"]); rec["kernels_ms_b"] = kernels(bc, legs["b"])
    rec["dec_items_ms"] = rec["kernels_ms_b"]["k_dec_items"]
    rec["decode_scratch_bytes"] = int(Z.zsmi_decodeScratchBytes(bc.ctx))
    return rec


def layout_alone(bc, a, n, dev):
    """the layout kernel over n sizes of 32 KiB: its time alone (the scan is one workgroup)"""
    d_sizes = torch.full((n,), 32768, dtype=torch.int64, device=dev)
    d_caps = torch.zeros(n, dtype=torch.int32, device=dev); d_offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    run = lambda: bc.layout_outputs_device(d_sizes.data_ptr(), 0, n, d_caps.data_ptr(), d_offs.data_ptr(), align=64)
    with Limit(a.limit, "layout alone"):
        torch.cuda.synchronize()
        for _ in range(2):
            run()
        bc.sync()
        assert int(d_offs[n].item()) == n * 32768 and (d_caps.cpu().numpy() == 32768).all()
        ms = [kernels(bc, run)["k_layout_outputs"] for _ in range(a.repeats)]
    return {"layout_items": n, "layout_ms": ms, "library": bc.L.zsmi_versionString().decode()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="57344,8192", help="frames a call, comma separated (empty: no decode workload)")
    ap.add_argument("--million", action="store_true", help="1 048 576 frames as well (about 50 GiB of device memory)")
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds a repeat (or a check) may take")
    ap.add_argument("--layout-items", type=int, default=0, help="the layout kernel alone over this many sizes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    bc = BatchCodec(device=0)
    counts = [int(v) for v in a.frames.split(",") if v] + ([1 << 20] if a.million else [])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for n in counts:
            line = json.dumps(workload(bc, a, n, a.chunk, dev))
            print(line, flush=True); out.write(line + "\n"); out.flush()
            torch.cuda.empty_cache()
        if a.layout_items:
            line = json.dumps(layout_alone(bc, a, a.layout_items, dev))
            print(line, flush=True); out.write(line + "\n"); out.flush()
    bc.close()


if __name__ == "__main__":
    main()
