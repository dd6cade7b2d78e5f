#!/usr/bin/env python3
"""GPU check (run by tests/test_gpu_decode_edges.py::test_device_api_stays_inside_each_item, in a process of its own: torch has to be
loaded before libzsmi.so): output bounds of the device batch API.  Output buffers are filled with a canary; items sit with gaps between
them and tightly packed, with a canary tail after the last.
  decode: the edge catalogue (exact, 1 MiB and one-byte-short capacities; each frame alone and followed by a skippable frame) and ordinary
          frames of 32 KiB - 1 MiB: no byte outside [dstOffset, dstOffset + dstCap) changes, for successful and failing items alike, and
          each status equals oracle D's at that capacity;
  encode: ragged chunks (size 0, incompressible, up to 1 MiB): no byte outside [dstOffset, dstOffset + zsmi_compressBound(size)) changes.
Reports (does not assert) whether bytes between a decoded item's produced size and its dstCap are touched.  Prints one JSON line."""
import os, sys, json
import torch                                               # before libzsmi.so
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _oracle as O, _edge_catalogue as C, _framewriter as W, _data as D, _batch as B
from zstandard_amd import BatchCodec, _lib

MIB = 1 << 20
CANARY = 0xA5
REPORT = {"tail_touched": 0, "tail_kept": 0, "decode_items": 0, "compress_items": 0}


def want(frame, cap):
    try:
        return O.decompress(frame, cap)
    except O.OracleError as e:
        return (1 << 32) - e.code


def place(caps, gaps):
    do = B.layout(caps, gaps)
    return do, int(do[-1]) + int(caps[-1]) + 4096


def outside(host, do, caps):
    inside = np.zeros(len(host), dtype=bool)
    for o, c in zip(do, caps):
        inside[int(o):int(o) + int(c)] = True
    return np.flatnonzero(~inside & (host != CANARY))


def decode_case(bc, frames, caps, gaps):
    caps = np.array(caps, dtype=np.uint32)
    do, total = place(caps, gaps)
    blob, fo, fsz = B.batch(frames)
    src = torch.from_numpy(blob.copy()).cuda()
    dst = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(len(frames), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bc.decompress_device(src.data_ptr(), fo, fsz, dst.data_ptr(), do, caps, sizes.data_ptr())
    bc.sync()
    host = dst.cpu().numpy(); sz = sizes.cpu().numpy().view(np.uint32)
    bad = outside(host, do, caps)
    assert bad.size == 0, f"decode wrote outside the items' regions at {bad[:10].tolist()}"
    for i, f in enumerate(frames):
        w, s = want(f, int(caps[i])), int(sz[i])
        if isinstance(w, int):
            assert s == w, (i, s, w)
        else:
            assert s == len(w) and host[int(do[i]):int(do[i]) + s].tobytes() == w, i
            tail = host[int(do[i]) + s:int(do[i]) + int(caps[i])]
            REPORT["tail_touched" if (tail != CANARY).any() else "tail_kept"] += 1
    REPORT["decode_items"] += len(frames)


def main():
    bc = BatchCodec(0)
    rng = np.random.default_rng(11)
    cat = C.catalogue()
    frames = [e.frame for e in cat]
    n = len(cat)
    for caps in ([e.cap for e in cat], [MIB] * n, [max(e.cap - 1, 0) for e in cat]):
        decode_case(bc, frames, caps, rng.integers(1, 300, n))            # gaps between the items
        decode_case(bc, frames, caps, np.zeros(n, dtype=np.int64))        # tightly packed
    decode_case(bc, [f + W.skippable(b"") for f in frames], [e.cap for e in cat], np.zeros(n, dtype=np.int64))
    text = D.zipf_log(8 << 20).tobytes()
    sizes = [32768, 65536, 65537, 131072, 200000, 524288, MIB]
    ordinary = [text[i * 100000:i * 100000 + k] for i, k in enumerate(sizes * 2)]
    of = [O.compress(c, 3) for c in ordinary[:len(sizes)]] + \
         [O.zstd_compress(c, 3) if O.libzstd() else O.compress(c, 1) for c in ordinary[len(sizes):]]
    for caps in ([len(c) for c in ordinary], [len(c) - 1 for c in ordinary], [len(c) + 4096 for c in ordinary]):
        decode_case(bc, of, caps, np.zeros(len(of), dtype=np.int64))
        decode_case(bc, of, caps, rng.integers(1, 64, len(of)))

    L = _lib.lib()
    noise = rng.integers(0, 256, 2 << 20, dtype=np.uint8).tobytes()
    chunks = [(noise if i % 3 == 1 else text)[i * 50000:i * 50000 + k]
              for i, k in enumerate([0, 1, 17, 4095, 65535, 65536, 65537, 131072, 300000, 0, MIB, 7])]
    blob, so, csz = B.batch(chunks)
    bounds = np.array([L.zsmi_compressBound(int(s)) for s in csz], dtype=np.uint64)
    for gaps in (np.zeros(len(chunks), dtype=np.int64), rng.integers(1, 200, len(chunks))):
        do, total = place(bounds, gaps)
        src = torch.from_numpy(blob.copy()).cuda()
        dst = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
        dsz = torch.zeros(len(chunks), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        bc.compress_device(src.data_ptr(), so, csz, dst.data_ptr(), do, dsz.data_ptr(), 3)
        bc.sync()
        host = dst.cpu().numpy(); zs = dsz.cpu().numpy().view(np.uint32)
        bad = outside(host, do, bounds)
        assert bad.size == 0, f"compress wrote outside the compressBound regions at {bad[:10].tolist()}"
        for i, (f, c) in enumerate(zip(B.cut(host, do, zs), chunks)):
            assert int(zs[i]) <= int(bounds[i]) and O.decompress(f, len(c)) == c, i
        REPORT["compress_items"] += len(chunks)
    bc.close()
    print(json.dumps(REPORT))
    return 0


if __name__ == "__main__":
    sys.exit(main())
