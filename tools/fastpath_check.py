#!/usr/bin/env python3
"""GPU check (run by tests/test_gpu_codec.py::test_intended_shapes_stay_on_the_decode_fast_path, in a process of its own because it loads
the library built with the debug hooks): frames of the shapes the decoder's fast path is meant to take are decoded, and the per-item
descriptors (ZsFastDesc.fast) are read back.  A shape that silently falls back to the general kernel decodes correctly and 4 x slower -
only this count shows it (ELF-class frames did so for two rounds).  Rows "ddict ..." are dictionary frames decoded with a DecompressionDict
(zsmi_createDDict): own CDict frames with a trained dictionary, own frames with a raw-content one, libzstd's with the trained one.  Rows
"ddict set ..." are mixed batches through a DecompressionDictSet (zsmi_createDDictSet): own CDict frames of three trained dictionaries,
interleaved, and a committed libzstd frame of a fourth - every frame decoded with the dictionary it names.  Rows "cdict set -> ddict set ..."
are such batches compressed in one call through a CompressionDictSet (zsmi_createCDictSet) first.  Rows "record archive -> ddict set ..." are such
batches written as a record archive (zsmi_compressSeekableFrames*) and read by frame number through a handle opened with the DDict set: the
dictionary frames of a read take the fast kernels.  Row "checksum ..." is own frames written
with the context's checksum parameter on (zsmi_setParameter): the fast path verifies their Content_Checksum itself.
Prints one JSON object: shape -> [items on the fast path, items]."""
import os; os.environ["ZSMI_DEBUG_LIB"] = "1"
import sys, ctypes, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _data as D, _oracle as O, _corpus as C, _batch as B, _dicts as X, _ddict as DD
from zstandard_amd import BatchCodec, CompressionDict, CompressionDictSet, NO_DICT, DecompressionDict, DecompressionDictSet, _lib


def desc_layout(Z):
    """words of a ZsFastDesc and the word index of `fast`: asked of the library itself (zsmi_dbg_descLayout), so a field added to the descriptor
    cannot make this check read the wrong word"""
    lay = (ctypes.c_uint32 * 6)()
    Z.zsmi_dbg_descLayout(lay)
    return int(lay[0]), int(lay[1])



def main():
    if _lib.built_fingerprint() != _lib.source_fingerprint():
        _lib.build()                                      # (a stale debug build would check yesterday's kernels)
    bc = BatchCodec(0); Z = _lib.lib()
    DESC_WORDS, FAST_AT = desc_layout(Z)
    assert 8 <= DESC_WORDS <= 256 and FAST_AT < DESC_WORDS
    rng = np.random.default_rng(5)
    text = D.zipf_log(6 << 20, seed_lo=41).tobytes()
    noise = rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    elf = dict(C.corpus(1 << 20)).get("elf", None)
    res = {}

    def run(label, chunks, own=True, lvl=3, frames=None, dic=None, dset=None):
        """frames: made by the caller (dictionary frames); dic: decoded with a DecompressionDict of it; dset: with this DecompressionDictSet"""
        if frames is not None:
            pass
        elif own:
            frames = B.cut(*bc.compress_host(*B.batch(chunks), lvl))
        else:
            frames = [O.zstd_compress(c, lvl) for c in chunks]
        if dset is not None:
            out, oo, osz = bc.decompress_host(*B.batch(frames), np.array([len(c) for c in chunks], dtype=np.uint32), ddict_set=dset)
            ok = (osz < B.ERR).all() and B.cut(out, oo, osz) == chunks
        elif dic is not None:
            dd = DecompressionDict(bc, dic)
            ok = DD.decode_many(bc, frames, [len(c) for c in chunks], dd) == [(len(c), c) for c in chunks]
            dd.close()
        else:
            ok = B.decode_many(bc, frames, [len(c) for c in chunks], min_cap=0) == [(len(c), c) for c in chunks]
        n = len(chunks)
        buf = np.zeros(n * DESC_WORDS, dtype=np.uint32)
        rc = Z.zsmi_dbg_copyScratch(bc.ctx, b"fastDesc", buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(buf.nbytes)); assert rc == 0, rc
        res[label] = [int((buf.reshape(-1, DESC_WORDS)[:n, FAST_AT] == 1).sum()) if ok else -1, n]

    run("own 32 KiB", [text[i * 32768:(i + 1) * 32768] for i in range(64)])
    chunks = [text[i * 32768:(i + 1) * 32768] for i in range(64)]
    bc.set_parameter("checksum", 1)
    frames = B.frames_of(bc.compress_host(*B.batch(chunks), 3))
    bc.set_parameter("checksum", 0)
    assert all(f[4] & 4 for f in frames), "frames carry a Content_Checksum"
    run("checksum: own 32 KiB frames that carry a Content_Checksum", chunks, frames=frames)
    run("own 128 KiB", [text[i * 40000:i * 40000 + 131072] for i in range(32)])
    run("own 1 MiB", [text[i * 70000:i * 70000 + (1 << 20)] for i in range(16)])
    run("own, raw and RLE blocks among compressed ones", [text[i * 50000:i * 50000 + 200000] + noise[i * 1000:i * 1000 + 70000] + bytes(70000) + text[:100000] for i in range(16)])
    skew = np.minimum(rng.geometric(0.05, 1 << 20), 255).astype(np.uint8).tobytes()
    run("own, compressed blocks of literals only (no sequences: Huffman pays, no match does)", [skew[i * 65536:(i + 1) * 65536] for i in range(16)])
    run("own, raw blocks only", [noise[i * 100:i * 100 + 65536] for i in range(16)])
    run("own, RLE blocks only: 1 MiB of zeros (BASELINE config 1)", [bytes(1 << 20)])
    run("own, raw blocks only, 300 KB", [noise[i * 100:i * 100 + 300000] for i in range(8)])
    if elf is not None:
        run("own, ELF class (wide alphabets: flat Huffman table)", [elf[i * 65536:(i + 1) * 65536] for i in range(16)])
    if O.libzstd():
        run("libzstd 32 KiB", [text[i * 32768:(i + 1) * 32768] for i in range(64)], own=False)
        run("libzstd 300 KB level 1", [text[i * 70000:i * 70000 + 300000] for i in range(16)], own=False, lvl=1)
        run("libzstd 1 MiB level 3 (repeated tables)", [text[i * 70000:i * 70000 + (1 << 20)] for i in range(16)], own=False)
        run("libzstd 400 KB level 9", [text[i * 70000:i * 70000 + 400000] for i in range(16)], own=False, lvl=9)
    # dictionary frames through a digested decode dictionary
    cls = "json_records"
    trained, records = X.trained(cls), X.class_data(cls)
    cd = CompressionDict(bc, trained, 3)
    for cs, n in ((1024, 256), (4096, 64), (65536, 8)):
        chunks = [records[i * cs:(i + 1) * cs] for i in range(n)]
        run("ddict, own CDict frames of %d KiB, trained dictionary" % (cs >> 10), chunks, frames=B.compress_many(bc, chunks, cdict=cd), dic=trained)
    cd.close()
    rawdic = X.STREAM[:6000]
    chunks = [X.STREAM[6000 + i * 4096:6000 + (i + 1) * 4096] for i in range(64)]
    run("ddict, own frames of 4 KiB, raw-content dictionary", chunks, frames=B.compress_many(bc, chunks, 3, rawdic), dic=rawdic)
    if X.zstd():
        chunks = [records[i * 4096:(i + 1) * 4096] for i in range(64)]
        run("ddict, libzstd frames of 4 KiB, trained dictionary", chunks, frames=[X.zstd_compress_dict(c, trained, 3) for c in chunks], dic=trained)
    # a mixed batch through a DDict set: item i names dictionary i % 3; the last one is libzstd's frame of the 8 KiB trained dictionary
    classes = ("json_records", "zipf", "xml_records")
    dics = [X.trained(c) for c in classes] + [X.TRAINED8K]
    datas = [X.class_data(c, 1 << 20) for c in classes]
    dds = [DecompressionDict(bc, d) for d in dics]
    dset = DecompressionDictSet(bc, dds)
    cds = [CompressionDict(bc, d, 3) for d in dics[:3]]
    for cs, n in ((1024, 255), (4096, 63), (65536, 9)):
        chunks = [datas[i % 3][(i // 3) * cs:(i // 3 + 1) * cs] for i in range(n)]
        frames = [None] * n
        for k in range(3):
            for i, f in zip(range(k, n, 3), B.compress_many(bc, chunks[k::3], cdict=cds[k])):
                frames[i] = f
        chunks.append(X.FIX["trained_small_l3_want"].tobytes()); frames.append(X.FIX["trained_small_l3_frame"].tobytes())
        run("ddict set, own CDict frames of %d KiB of 3 trained dictionaries interleaved, and a libzstd frame of a fourth" % (cs >> 10), chunks, frames=frames, dset=dset)
    # the same batches compressed in ONE call through a CDict set of the three dictionaries (chunk i: member i % 3, every fourth chunk without a
    # dictionary) and decoded in one call through the DDict set of the same dictionaries
    cset = CompressionDictSet(bc, cds, 3)
    for cs, n in ((1024, 256), (4096, 64), (65536, 8)):
        chunks = [datas[i % 3][(i // 3) * cs:(i // 3 + 1) * cs] for i in range(n)]
        index = np.array([NO_DICT if i % 4 == 3 else i % 3 for i in range(n)], dtype=np.uint32)
        frames = B.frames_of(bc.compress_host(*B.batch(chunks), cdict_set=cset, dict_index=index))
        named = sum((f[4] & 3) != 0 for f in frames)
        assert named == int((index != NO_DICT).sum()), (named, "frames name a dictionary")
        run("cdict set -> ddict set, own frames of %d KiB: 3 trained dictionaries and no dictionary interleaved, one call each way" % (cs >> 10), chunks, frames=frames, dset=dset)
    # a record archive: one frame a record, the dictionaries chosen as above, written in one call (zsmi_compressSeekableFramesHost_usingCDictSet)
    # and read by frame number through a handle opened with the DDict set - every frame its own range, so one decode call holds them all
    for cs, n in ((1024, 256), (4096, 64)):
        chunks = [datas[i % 3][(i // 3) * cs:(i // 3 + 1) * cs] for i in range(n)]
        index = np.array([NO_DICT if i % 4 == 3 else i % 3 for i in range(n)], dtype=np.uint32)
        arc = bc.compress_seekable_frames_host(b"".join(chunks), [cs] * n, cdict_set=cset, dict_index=index)
        err = ctypes.c_int(0)
        sk = Z.zsmi_openSeekable_usingDDictSet(bc.ctx, arc, len(arc), dset.handle, ctypes.byref(err)); assert sk, err.value
        idx = np.arange(n, dtype=np.uint32)
        out = np.zeros(n * cs, dtype=np.uint8); written = np.zeros(n, dtype=np.uint64); codes = np.ones(n, dtype=np.uint32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = Z.zsmi_seekableReadFramesHost(bc.ctx, sk, p(idx), n, p(out), out.nbytes, p(written), p(codes)); assert rc == 0, rc
        Z.zsmi_closeSeekable(sk)
        ok = not codes.any() and out.tobytes() == b"".join(chunks)
        buf = np.zeros(n * DESC_WORDS, dtype=np.uint32)
        rc = Z.zsmi_dbg_copyScratch(bc.ctx, b"fastDesc", p(buf), ctypes.c_size_t(buf.nbytes)); assert rc == 0, rc
        res["record archive -> ddict set, records of %d KiB: 3 trained dictionaries and no dictionary interleaved, read by frame number" % (cs >> 10)] = \
            [int((buf.reshape(-1, DESC_WORDS)[:n, FAST_AT] == 1).sum()) if ok else -1, n]
    cset.close()
    dset.close()
    for x in cds + dds:
        x.close()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
