#!/usr/bin/env python3
"""GPU box: compression with a dictionary against compression without one (device-resident, per-call wall time, like tools/bench_sizes.py).
One JSON line per (class, chunk size, level): GiB/s and ratio with and without the dictionary (the class's 64 KiB trained dictionary of
tests/golden/libzstd_fixtures_dict_compress.npz), and our compressed size over libzstd's with the trained dictionary and with its content
alone (the first 64 chunks; absent without libzstd).  The same call with the dictionary digested once (CompressionDict,
zsmi_compressBatchDevice_usingCDict) is measured next to it in the same process: gib_s_cdict, ratio_cdict, vs_libzstd_trained_cdict, and
gap_closed = the share of the _usingDict call's excess over libzstd that the CDict call removes.  Every rate is the median of --repeats
timings of --steps calls; spread_* is (max - min) / median of those timings.  --kernels: per-kernel times of one call of each dictionary
form (zsmi_enableKernelTiming).
The decode leg runs on the frames the record has just made: dec_gib_s_dict (the _usingDict frames through zsmi_decompressBatchDevice_usingDict:
the general kernel), dec_gib_s_ddict (the CDict frames through a DecompressionDict: the fast path) and dec_gib_s_plain (the no-dictionary
frames of the same chunks, plain decode), GiB/s of decoded bytes; dec_min_* / dec_max_* are the slowest and fastest of the --repeats timings
as rates, dec_spread_* their spread; ddict_over_dict and ddict_over_plain the ratios of the medians; dec_ranges_apart says that the DDict's
slowest repeat beat the _usingDict call's fastest.  --kernels adds dec_kernels_ms_*.
--loader: instead of all that, what LOADING a dictionary costs at each entry point that reads its bytes (one JSON line; per call, in
microseconds: median, min and max of --repeats timings of --steps calls): the device _usingDict compress of one 1 KiB chunk and of 4096
chunks of 4 KiB, the host _usingDict compress of 64 chunks of 1 KiB, zsmi_createCDict, zsmi_createDDict (each with its free), and the
_usingDict decode of 4096 frames of 4 KiB (k_decode_frames_dict loads the dictionary in front of every frame).  ZSMI_LIB_FILE names another
build of the library to measure with the same tool.
--dict-set K: instead of all that, a decode call whose frames name K dictionaries (one JSON line per chunk size of 1, 4 and 64 KiB): one
32 MB call of CDict frames, item i of dictionary i % K, through a DecompressionDictSet (zsmi_decompressBatchDevice_usingDDictSet) against
what a caller had to do without one - K zsmi_decompressBatchDevice_usingDDict calls one after the other, each over its dictionary's frames -
in the same process, on the same frames.  set_gib_s / seq_gib_s: the median of --repeats timings of --steps calls (of K calls each), with the
slowest and fastest as rates (*_min, *_max) and their spread; set_over_seq the ratio of the medians; slower_beyond_spreads says that the set
call is slower by more than both spreads together.  The K dictionaries are the trained ones of --classes in turn, each under an ID of its own
(the fixtures hold five: a dictionary met again is another DDict with its own device image and ID, over that class's next chunks).
--cdict-set K: the same for the compress side (one JSON line per chunk size of 1, 4 and 64 KiB): one 32 MB call of chunks, chunk i with
dictionary i % K, through a CompressionDictSet (zsmi_compressBatchDevice_usingCDictSet) against K zsmi_compressBatchDevice_usingCDict calls
one after the other, each over its dictionary's chunks, in the same process; both outputs are compared byte for byte.  Fields as --dict-set's."""
import argparse, ctypes, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import _data as D, _oracle as O, _corpus as C
from zstandard_amd import BatchCodec, CompressionDict, CompressionDictSet, DecompressionDict, DecompressionDictSet, _lib

FIXC = os.path.join(ROOT, "tests", "golden", "libzstd_fixtures_dict_compress.npz")


def class_bytes(cls, n):
    if cls == "zipf":
        return D.zipf_log(n).tobytes()
    return getattr(C, cls)(n)[:n]


def zstd_sizes(chunks, dic, level):
    Z = O.libzstd()
    if not Z:
        return None
    sz, vp, cp = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p
    Z.ZSTD_createCCtx.restype = vp
    Z.ZSTD_compress_usingDict.restype = sz; Z.ZSTD_compress_usingDict.argtypes = [vp, vp, sz, cp, sz, cp, sz, ctypes.c_int]
    cctx = Z.ZSTD_createCCtx(); total = 0
    for c in chunks:
        cap = Z.ZSTD_compressBound(len(c)); out = ctypes.create_string_buffer(cap)
        r = Z.ZSTD_compress_usingDict(cctx, out, cap, c, len(c), dic, len(dic), level); assert not Z.ZSTD_isError(r)
        total += r
    return total


def loader_leg(a):
    cls = a.classes.split(",")[0]
    dic = np.load(FIXC)["trained_" + cls].tobytes()
    data = class_bytes(cls, 4096 * 4096)
    dev = torch.device("cuda:0")
    bc = BatchCodec(device=0); Z = _lib.lib()
    vp = ctypes.c_void_p
    pa = lambda x: x.ctypes.data_as(vp)
    dsrc = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    ddict = torch.from_numpy(np.frombuffer(dic, dtype=np.uint8).copy()).to(dev)
    hsrc = np.frombuffer(data, dtype=np.uint8)

    def layout(n, cs):
        bound = int(Z.zsmi_compressBound(cs))
        return np.arange(n, dtype=np.uint64) * cs, np.full(n, cs, dtype=np.uint32), np.arange(n, dtype=np.uint64) * bound, bound
    off, sz, doff, bound = layout(4096, 4096)
    ddst = torch.empty(4096 * bound, dtype=torch.uint8, device=dev); dsz = torch.empty(4096, dtype=torch.int32, device=dev)
    dout = torch.empty(4096 * 4096, dtype=torch.uint8, device=dev); dosz = torch.empty(4096, dtype=torch.int32, device=dev)
    o1, s1, d1, _ = layout(1, 1024)
    o64, s64, _, _ = layout(64, 1024)
    legs = {}
    legs["device_usingDict_1x1KiB"] = lambda: bc.compress_device(dsrc.data_ptr(), o1, s1, ddst.data_ptr(), d1, dsz.data_ptr(), 3, ddict.data_ptr(), len(dic))
    legs["device_usingDict_4096x4KiB"] = lambda: bc.compress_device(dsrc.data_ptr(), off, sz, ddst.data_ptr(), doff, dsz.data_ptr(), 3, ddict.data_ptr(), len(dic))
    legs["host_usingDict_64x1KiB"] = lambda: bc.compress_host(hsrc, o64, s64, 3, dic)
    legs["createCDict"] = lambda: CompressionDict(bc, dic, 3).close()
    legs["createDDict"] = lambda: DecompressionDict(bc, dic).close()
    caps = np.full(4096, 4096, dtype=np.uint32)
    rec = {"loader": True, "class": cls, "dict_bytes": len(dic), "library": Z.zsmi_versionString().decode(), "steps": a.steps, "repeats": a.repeats, "unit": "us per call"}
    for name in list(legs) + ["usingDict_decode_4096x4KiB"]:
        if name == "usingDict_decode_4096x4KiB":                       # the frames the second leg left in ddst
            legs["device_usingDict_4096x4KiB"](); bc.sync()
            fsz = dsz.cpu().numpy().view(np.uint32).copy()
            run = lambda: Z.zsmi_decompressBatchDevice_usingDict(bc.ctx, vp(ddst.data_ptr()), pa(doff), pa(fsz), 4096, vp(dout.data_ptr()), pa(off), pa(caps),
                                                                 vp(dosz.data_ptr()), vp(ddict.data_ptr()), len(dic))
        else:
            run = legs[name]
        for _ in range(3):
            run()
        times = []
        for _ in range(a.repeats):
            bc.sync(); t0 = time.perf_counter()
            for _ in range(a.steps):
                run()
            bc.sync(); times.append((time.perf_counter() - t0) / a.steps * 1e6)
        rec[name] = {"median": round(float(np.median(times)), 1), "min": round(min(times), 1), "max": round(max(times), 1)}
    assert torch.equal(dout, dsrc[:4096 * 4096]) and bool((dosz == 4096).all())
    print(json.dumps(rec), flush=True)


def interleaved_chunks(classes, K, cs):
    """(n, per, an (n, cs) array): per chunks of cs bytes for each of K dictionaries - item i holds chunk i // K of dictionary i % K, cut from
    its class's data (a class met again: its next chunks) - 32 MB in all"""
    per = (32 << 20) // cs // K; n = per * K
    rounds = (K + len(classes) - 1) // len(classes)
    data = {c: np.frombuffer(class_bytes(c, rounds * per * cs), dtype=np.uint8) for c in classes[:min(K, len(classes))]}
    src = np.empty((n, cs), dtype=np.uint8)
    for k in range(K):
        at = (k // len(classes)) * per * cs
        src[k::K] = data[classes[k % len(classes)]][at:at + per * cs].reshape(per, cs)
    return n, per, src


def dict_set_leg(a):
    K = a.dict_set
    fix = np.load(FIXC)
    classes = a.classes.split(",")
    dev = torch.device("cuda:0")
    bc = BatchCodec(device=0); Z = _lib.lib()
    dics = [fix["trained_" + classes[k % len(classes)]].tobytes() for k in range(K)]
    dics = [d[:4] + (1000 + k).to_bytes(4, "little") + d[8:] for k, d in enumerate(dics)]
    dds = [DecompressionDict(bc, d) for d in dics]
    order = np.random.default_rng(1).permutation(K)                       # (the set sorts its members itself)
    dset = DecompressionDictSet(bc, [dds[k] for k in order])
    assert len(dset) == K
    for cs in (1024, 4096, 65536):
        n, per, src = interleaved_chunks(classes, K, cs)                  # item i holds chunk i // K of dictionary i % K
        dsrc = torch.from_numpy(src.reshape(-1)).to(dev)
        off = np.arange(n, dtype=np.uint64) * cs; sz = np.full(n, cs, dtype=np.uint32); caps = sz.copy()
        bound = int(Z.zsmi_compressBound(cs)); doff = np.arange(n, dtype=np.uint64) * bound
        dfr = torch.empty(n * bound, dtype=torch.uint8, device=dev)
        fsz = np.zeros(n, dtype=np.uint32)
        part = torch.empty(per, dtype=torch.int32, device=dev)
        sub = [tuple(np.ascontiguousarray(x[k::K]) for x in (off, doff, caps)) for k in range(K)]
        for k in range(K):
            cd = CompressionDict(bc, dics[k], 3)
            bc.compress_device(dsrc.data_ptr(), sub[k][0], np.ascontiguousarray(sz[k::K]), dfr.data_ptr(), sub[k][1], part.data_ptr(), cdict=cd)
            bc.sync(); cd.close()
            fsz[k::K] = part.cpu().numpy().view(np.uint32)
        assert (fsz < 0xFFFFFF88).all()
        subsz = [np.ascontiguousarray(fsz[k::K]) for k in range(K)]
        dout = torch.empty(n * cs, dtype=torch.uint8, device=dev); dosz = torch.empty(n, dtype=torch.int32, device=dev)

        def run_set():
            bc.decompress_device(dfr.data_ptr(), doff, fsz, dout.data_ptr(), off, caps, dosz.data_ptr(), ddict_set=dset)

        def run_seq():
            for k in range(K):
                bc.decompress_device(dfr.data_ptr(), sub[k][1], subsz[k], dout.data_ptr(), sub[k][0], sub[k][2], dosz.data_ptr() + 4 * k * per, ddict=dds[k])
        rec = {"dict_set": K, "chunk": cs, "chunks": n, "library": Z.zsmi_versionString().decode(), "steps": a.steps, "repeats": a.repeats}
        gib = n * cs / 2**30
        for tag, run in (("set", run_set), ("seq", run_seq)):
            dout.zero_(); dosz.zero_()
            for _ in range(2):
                run()
            bc.sync()
            assert torch.equal(dout, dsrc) and bool((dosz == cs).all()), ("dict-set leg", tag, cs)
            times = []
            for _ in range(a.repeats):
                bc.sync(); t0 = time.perf_counter()
                for _ in range(a.steps):
                    run()
                bc.sync(); times.append((time.perf_counter() - t0) / a.steps)
            dt = float(np.median(times))
            rec[tag + "_gib_s"] = round(gib / dt, 2); rec[tag + "_min"] = round(gib / max(times), 2); rec[tag + "_max"] = round(gib / min(times), 2)
            rec[tag + "_spread"] = round((max(times) - min(times)) / dt, 3)
            if a.kernels:
                bc.enable_timing(True); run(); bc.sync()
                rec["dec_kernels_ms_" + tag] = {k2: round(v[0] * 1e3, 3) for k2, v in bc.kernel_times().items()}
                bc.enable_timing(False)
        rec["set_over_seq"] = round(rec["set_gib_s"] / rec["seq_gib_s"], 3)
        rec["slower_beyond_spreads"] = bool(rec["set_over_seq"] < 1.0 - rec["set_spread"] - rec["seq_spread"])
        print(json.dumps(rec), flush=True)
        del dfr, dout, dosz, dsrc
    bc.sync(); dset.close()
    for d in dds:
        d.close()


def cdict_set_leg(a):
    K = a.cdict_set
    fix = np.load(FIXC)
    classes = a.classes.split(",")
    dev = torch.device("cuda:0")
    bc = BatchCodec(device=0); Z = _lib.lib()
    dics = [fix["trained_" + classes[k % len(classes)]].tobytes() for k in range(K)]
    dics = [d[:4] + (1000 + k).to_bytes(4, "little") + d[8:] for k, d in enumerate(dics)]
    cds = [CompressionDict(bc, d, 3) for d in dics]
    cset = CompressionDictSet(bc, cds, 3)
    assert len(cset) == K
    for cs in (1024, 4096, 65536):
        n, per, src = interleaved_chunks(classes, K, cs)
        dsrc = torch.from_numpy(src.reshape(-1)).to(dev)
        off = np.arange(n, dtype=np.uint64) * cs; sz = np.full(n, cs, dtype=np.uint32)
        index = (np.arange(n) % K).astype(np.uint32)
        bound = int(Z.zsmi_compressBound(cs)); doff = np.arange(n, dtype=np.uint64) * bound
        sub = [tuple(np.ascontiguousarray(x[k::K]) for x in (off, sz, doff)) for k in range(K)]
        outs = {}

        def run_set(ddst, dsz):
            bc.compress_device(dsrc.data_ptr(), off, sz, ddst.data_ptr(), doff, dsz.data_ptr(), cdict_set=cset, dict_index=index)

        def run_seq(ddst, dsz):                                       # (chunk i's size lands at i % K * per + i // K)
            for k in range(K):
                bc.compress_device(dsrc.data_ptr(), sub[k][0], sub[k][1], ddst.data_ptr(), sub[k][2], dsz.data_ptr() + 4 * k * per, cdict=cds[k])
        rec = {"cdict_set": K, "chunk": cs, "chunks": n, "library": Z.zsmi_versionString().decode(), "steps": a.steps, "repeats": a.repeats}
        gib = n * cs / 2**30
        for tag, run in (("set", run_set), ("seq", run_seq)):
            ddst = torch.zeros(n * bound, dtype=torch.uint8, device=dev); dsz = torch.zeros(n, dtype=torch.int32, device=dev)
            for _ in range(2):
                run(ddst, dsz)
            times = []
            for _ in range(a.repeats):
                bc.sync(); t0 = time.perf_counter()
                for _ in range(a.steps):
                    run(ddst, dsz)
                bc.sync(); times.append((time.perf_counter() - t0) / a.steps)
            dt = float(np.median(times))
            rec[tag + "_gib_s"] = round(gib / dt, 2); rec[tag + "_min"] = round(gib / max(times), 2); rec[tag + "_max"] = round(gib / min(times), 2)
            rec[tag + "_spread"] = round((max(times) - min(times)) / dt, 3)
            if a.kernels:
                bc.enable_timing(True); run(ddst, dsz); bc.sync()
                rec["kernels_ms_" + tag] = {k2: round(v[0] * 1e3, 3) for k2, v in bc.kernel_times().items()}
                bc.enable_timing(False)
            sizes = dsz.cpu().numpy().view(np.uint32)
            if tag == "seq":
                sizes = sizes.reshape(K, per).T.reshape(-1)
            assert (sizes < 0xFFFFFF88).all()
            outs[tag] = (ddst, sizes.copy())
            del dsz
        # byte for byte: the sizes, and every frame (the slots were zeroed, and a call writes a chunk's frame only)
        assert (outs["set"][1] == outs["seq"][1]).all(), ("cdict-set leg: sizes differ", cs)
        assert torch.equal(outs["set"][0], outs["seq"][0]), ("cdict-set leg: frames differ", cs)
        host = outs["set"][0][:min(n, 64) * bound].cpu().numpy()
        for i in (0, min(n, 64) - 1):                                 # spot check under oracle D
            f = host[int(doff[i]):int(doff[i]) + int(outs["set"][1][i])].tobytes()
            assert O.decompress_using_dict(f, cs, dics[i % K]) == src[i].tobytes()
        rec["ratio"] = round(n * cs / float(outs["set"][1].sum()), 4)
        rec["set_over_seq"] = round(rec["set_gib_s"] / rec["seq_gib_s"], 3)
        rec["slower_beyond_spreads"] = bool(rec["set_over_seq"] < 1.0 - rec["set_spread"] - rec["seq_spread"])
        print(json.dumps(rec), flush=True)
        del outs, dsrc
    bc.sync(); cset.close()
    for cd in cds:
        cd.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=64 << 20, help="input bytes per class")
    ap.add_argument("--classes", default="zipf,json_records,xml_records,csv_records,binary_table")
    ap.add_argument("--chunks", default="1024,4096,16384,65536")
    ap.add_argument("--levels", default="3")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--loader", action="store_true", help="only the cost of loading a dictionary at each entry point that reads its bytes")
    ap.add_argument("--dict-set", type=int, default=0, metavar="K", help="only the decode of one 32 MB call whose frames name K dictionaries: a DDict set against K _usingDDict calls")
    ap.add_argument("--cdict-set", type=int, default=0, metavar="K", help="only the compress of one 32 MB call whose chunks use K dictionaries: a CDict set against K _usingCDict calls")
    a = ap.parse_args()
    if a.loader:
        return loader_leg(a)
    if a.cdict_set:
        return cdict_set_leg(a)
    if a.dict_set:
        return dict_set_leg(a)
    fix = np.load(FIXC)
    dev = torch.device("cuda:0")
    bc = BatchCodec(device=0)
    Z = _lib.lib()
    for cls in a.classes.split(","):
        data = class_bytes(cls, a.bytes)
        dsrc = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
        dic = fix["trained_" + cls].tobytes()
        content = dic[dic.find(bytes([1, 0, 0, 0, 4, 0, 0, 0, 8, 0, 0, 0]), 8) + 12:]
        ddict = torch.from_numpy(np.frombuffer(dic, dtype=np.uint8).copy()).to(dev)
        for cs in [int(x) for x in a.chunks.split(",")]:
            n = len(data) // cs
            off = np.arange(n, dtype=np.uint64) * cs; sz = np.full(n, cs, dtype=np.uint32)
            bound = int(Z.zsmi_compressBound(cs)); doff = np.arange(n, dtype=np.uint64) * bound
            ddst = torch.empty(n * bound, dtype=torch.uint8, device=dev); dsz = torch.empty(n, dtype=torch.int32, device=dev)
            for lvl in [int(x) for x in a.levels.split(",")]:
                rec = {"class": cls, "chunk": cs, "level": lvl, "chunks": n}
                cdict = CompressionDict(bc, dic, lvl)
                made = {}                                             # tag -> (frames on the device, their sizes): the decode leg's input
                for tag, dp, dn, cd in (("plain", 0, 0, None), ("dict", ddict.data_ptr(), len(dic), None), ("cdict", 0, len(dic), cdict)):
                    run = lambda: bc.compress_device(dsrc.data_ptr(), off, sz, ddst.data_ptr(), doff, dsz.data_ptr(), lvl, dp, dn if dp else 0, cdict=cd)
                    for _ in range(2):
                        run()
                    times = []
                    for _ in range(a.repeats):
                        bc.sync(); t0 = time.perf_counter()
                        for _ in range(a.steps):
                            run()
                        bc.sync(); times.append((time.perf_counter() - t0) / a.steps)
                    dt = float(np.median(times))
                    rec["spread_" + tag] = round((max(times) - min(times)) / dt, 3)
                    sizes = dsz.cpu().numpy().view(np.uint32)
                    assert (sizes < 0xFFFFFF88).all()
                    made[tag] = (ddst.clone(), sizes.copy())
                    host = ddst[:min(n, 64) * bound].cpu().numpy()
                    for i in (0, min(n, 64) - 1):                     # spot check under oracle D
                        f = host[int(doff[i]):int(doff[i]) + int(sizes[i])].tobytes()
                        c = data[i * cs:(i + 1) * cs]
                        assert (O.decompress_using_dict(f, cs, dic) if dn else O.decompress(f, cs)) == c
                    rec["gib_s_" + tag] = round(n * cs / dt / 2**30, 2)
                    rec["ratio_" + tag] = round(n * cs / float(sizes.sum()), 4)
                    if dn:
                        k = min(n, 64); ours = float(sizes[:k].sum())
                        chunks = [data[i * cs:(i + 1) * cs] for i in range(k)]
                        if cd is None:
                            zt, zc = zstd_sizes(chunks, dic, lvl), zstd_sizes(chunks, content, lvl)
                            if zt:
                                rec["vs_libzstd_trained"] = round(ours / zt, 4); rec["vs_libzstd_content"] = round(ours / zc, 4)
                        elif zt:
                            rec["vs_libzstd_trained_cdict"] = round(ours / zt, 4)
                            gap = rec["vs_libzstd_trained"] - 1.0
                            rec["gap_closed"] = round((rec["vs_libzstd_trained"] - rec["vs_libzstd_trained_cdict"]) / gap, 3) if gap > 0 else None
                        if a.kernels:
                            bc.enable_timing(True); run(); bc.sync()
                            rec["kernels_ms" + ("_cdict" if cd else "")] = {k2: round(v[0] * 1e3, 3) for k2, v in bc.kernel_times().items()}
                            bc.enable_timing(False)
                bc.sync(); cdict.close()
                # ---- the decode leg: the frames above, back into chunk-sized slots
                dd = DecompressionDict(bc, dic)
                dout = torch.empty(n * cs, dtype=torch.uint8, device=dev); dosz = torch.empty(n, dtype=torch.int32, device=dev)
                want = dsrc[:n * cs]
                caps = np.full(n, cs, dtype=np.uint32)
                vp = ctypes.c_void_p
                pa = lambda x: x.ctypes.data_as(vp)
                for tag, frames_tag in (("plain", "plain"), ("dict", "dict"), ("ddict", "cdict")):
                    dfr, fsz = made[frames_tag]
                    if tag == "dict":
                        run = lambda: Z.zsmi_decompressBatchDevice_usingDict(bc.ctx, vp(dfr.data_ptr()), pa(doff), pa(fsz), n, vp(dout.data_ptr()), pa(off), pa(caps),
                                                                             vp(dosz.data_ptr()), vp(ddict.data_ptr()), len(dic))
                    else:
                        run = lambda: bc.decompress_device(dfr.data_ptr(), doff, fsz, dout.data_ptr(), off, caps, dosz.data_ptr(), ddict=dd if tag == "ddict" else None)
                    dout.zero_()
                    for _ in range(2):
                        run()
                    bc.sync()
                    assert torch.equal(dout, want) and bool((dosz == cs).all()), ("decode leg", tag)
                    times = []
                    for _ in range(a.repeats):
                        bc.sync(); t0 = time.perf_counter()
                        for _ in range(a.steps):
                            run()
                        bc.sync(); times.append((time.perf_counter() - t0) / a.steps)
                    dt = float(np.median(times)); gib = n * cs / 2**30
                    rec["dec_gib_s_" + tag] = round(gib / dt, 2)
                    rec["dec_min_" + tag] = round(gib / max(times), 2); rec["dec_max_" + tag] = round(gib / min(times), 2)
                    rec["dec_spread_" + tag] = round((max(times) - min(times)) / dt, 3)
                    if a.kernels:
                        bc.enable_timing(True); run(); bc.sync()
                        rec["dec_kernels_ms_" + tag] = {k2: round(v[0] * 1e3, 3) for k2, v in bc.kernel_times().items()}
                        bc.enable_timing(False)
                bc.sync(); dd.close()
                rec["ddict_over_dict"] = round(rec["dec_gib_s_ddict"] / rec["dec_gib_s_dict"], 3)
                rec["ddict_over_plain"] = round(rec["dec_gib_s_ddict"] / rec["dec_gib_s_plain"], 3)
                rec["dec_ranges_apart"] = rec["dec_min_ddict"] > rec["dec_max_dict"]
                del made, dout, dosz
                rec["dict_over_plain"] = round(rec["gib_s_dict"] / rec["gib_s_plain"], 3)
                rec["cdict_over_dict"] = round(rec["gib_s_cdict"] / rec["gib_s_dict"], 3)
                print(json.dumps(rec), flush=True)
            del ddst, dsz


if __name__ == "__main__":
    main()
