"""The scalar finalize of the oracle (zso_finalizeDictionary, zso_trainStats in oracle/zso_encoder.c) and the reference of a whole training
call (tests/_train.py: reference_train), held to what can be held without a GPU: oracle E's 448 counters equal oracle D's counters of
the frames E wrote; the finalized dictionary is well formed, loads in oracle D, carries the derived ID, works in libzstd (where present)
within the bounds the GPU finalize is held to; every border case of tests/_dictfin.py reaches its border; and the C code runs clean under
the address and undefined-behaviour sanitizers as a stand-alone program (tests/c/dict_finalize.c).

Case (h) of the finalize cases, a literal distribution whose Huffman description does not fit at 11 bits so that finalize retries with
flatter codes, is dropped: a seeded search (numpy default_rng(20261021); counts 2^uniform, 2^integer levels, Dirichlet-weighted levels
and Zipf draws in turn) tried 476183 distributions in 60 s of CPU on zso_trainHuffDescription at maxBits 11 and the largest description
was 91 bytes of the 127 allowed: 255 weights of at most 12 values, bound by Kraft's sum, do not get near 4 bits a weight.  The retry loop
of k_train_tables is therefore still held by no test; the one description no maxBits can write (256 equal counts) is case c_no_literals."""
import ctypes, os, subprocess
import numpy as np
import pytest
import _oracle as O
import _dicts as X
import _train as T
import _framewriter as W
import _dictfin as F

ROOT = T.ROOT
FINALIZE_BOUND = T.FINALIZE_BOUND                                   # the bounds tests/test_gpu_dict_train.py holds the GPU finalize to; 1.01 for the other classes

# No (class, level) pair is left out of the counters test: measured, 106 of 106 frames have only compressed blocks in every class, at level 1
# as at level 3.


@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("cls", X.RECORD_CLASSES)
def test_encoder_counters_equal_decoder_counters(cls, level):
    """what oracle E counts where it hands a block's parse to its entropy stage is what oracle D finds in the frames E wrote"""
    parts = F.class_samples(cls)
    content = F.class_content(cls)
    frames = [O.compress_using_dict(p, content, level) for p in parts]
    compressed = sum(all(b.type == 2 for b in W.blocks(f)) for f in frames)
    print(f"{cls} level {level}: {compressed} of {len(frames)} frames all compressed")
    assert compressed == len(frames)                                  # the precondition: D sees every block's parse
    want, out = O.decode_train_stats(frames, [len(p) for p in parts], content)
    assert out == parts
    got = O.train_stats(content, parts, level)
    assert got.tolist() == want.tolist()
    assert int(got[:256].sum()) > 0 and int(got[256:320].sum()) == int(got[320:384].sum()) == int(got[384:].sum()) > 0


@pytest.mark.parametrize("cls", X.RECORD_CLASSES)
def test_finalized_dictionary(cls):
    parts, content = F.class_samples(cls), F.class_content(cls)
    dic = O.finalize_dictionary(content, parts, 65536)
    assert T.check_format(dic, 65536) == content
    off, did, reps = O.dict_params(dic)                               # oracle D loads it
    assert did == T.derived_id(content) == int.from_bytes(dic[4:8], "little")
    held = T.held_out(cls)[:100]
    for c in held[:20]:                                               # oracle E and D with it, tables and all
        assert O.decompress_using_dict(O.compress_using_dict(c, dic), len(c), dic) == c
    assert O.finalize_dictionary(content, parts, 65536, dict_id=77)[4:8] == (77).to_bytes(4, "little")


@pytest.mark.parametrize("cls", X.RECORD_CLASSES)
def test_finalized_dictionary_in_libzstd(cls):
    """libzstd compresses and decompresses held-out chunks with the oracle's dictionary, and over libzstd's own content its total stays
    within the bounds the GPU finalize is held to (the GPU must equal this oracle byte for byte)"""
    if not X.zstd():
        pytest.skip("libzstd not available")
    ref = X.trained(cls)
    dic = O.finalize_dictionary(X.content_of(ref), T.samples(cls), len(ref))
    T.check_format(dic, len(ref))
    held = T.held_out(cls)
    for c in held[:50]:
        assert X.zstd_decompress_dict(X.zstd_compress_dict(c, dic, 3), len(c), dic) == c
    mine, theirs = T.zstd_total(held, dic), T.zstd_total(held, ref)
    print(f"{cls}: oracle finalize {mine} libzstd {theirs} ratio {mine / theirs:.4f}")
    assert mine <= FINALIZE_BOUND.get(cls, 1.01) * theirs


@pytest.mark.parametrize("case", sorted(F.FINALIZE))
def test_finalize_case_reaches_its_border(case):
    F.reach_finalize(case)
    out = F.outcome(case)
    if isinstance(out, bytes):
        T.check_format(out, F.FINALIZE[case]()[2])


def test_empty_sample_changes_nothing():
    assert F.outcome("d_size_edges") == F.outcome("d_size_edges_without_empty")


def test_hidden_parses_count_the_same_in_either_order():
    assert F.stats_of("f_hidden_parses").tolist() == F.stats_of("f_hidden_parses_reversed").tolist()
    assert F.outcome("f_hidden_parses") == F.outcome("f_hidden_parses_reversed")


def test_finalize_refusals():
    parts = F.class_samples("csv_records")
    for cap, content, want in ((255, b"x" * 1000, 70), (4096, b"x" * 127, 72)):
        with pytest.raises(O.OracleError) as e:
            O.finalize_dictionary(content, parts, cap)
        assert e.value.code == want


@pytest.mark.parametrize("case", sorted(F.SELECT))
def test_selection_case_reaches_its_border(case):
    F.reach_select(case)
    dic, k, d, content, _ = F.select_reference(case)
    parts, cap, wk, wd, f = F.SELECT[case]()
    assert (k, d) == (wk, wd) and isinstance(dic, bytes) and content.endswith(T.check_format(dic, cap))


@pytest.mark.parametrize("case", sorted(F.SEARCH))
def test_search_case_reaches_its_border(case):
    F.reach_search(case)


def test_decoder_counters_count_only_where_armed():
    """oracle D's counters belong to the thread that armed them, from the reset to the get: a decode outside that pair and the batch
    driver's worker threads leave them alone (and pay nothing for them)"""
    parts, content = F.class_samples("json_records")[:8], F.class_content("json_records")
    frames = [O.compress_using_dict(p, content, 3) for p in parts]
    caps = [len(p) for p in parts]
    first, _ = O.decode_train_stats(frames, caps, content)
    assert int(first.sum()) > 0
    for f, c in zip(frames, caps):                                    # unarmed
        O.decompress_using_dict(f, c, content)
    L = O.lib()
    plain = [O.compress(p, 3) for p in parts]
    src = np.frombuffer(b"".join(plain), dtype=np.uint8)
    so = np.cumsum([0] + [len(f) for f in plain[:-1]]).astype(np.uint64); ss = np.array([len(f) for f in plain], dtype=np.uint32)
    do = np.cumsum([0] + caps[:-1]).astype(np.uint64); dc = np.array(caps, dtype=np.uint32)
    out = np.zeros(sum(caps), dtype=np.uint8); got = np.zeros(len(caps), dtype=np.uint32)
    vp = ctypes.c_void_p
    L.zso_trainStatsReset()                                           # armed here: the two workers below are other threads
    try:
        rc = L.zso_decompressBatch(out.ctypes.data_as(vp), do.ctypes.data_as(vp), dc.ctypes.data_as(vp), got.ctypes.data_as(vp),
                                   src.ctypes.data_as(vp), so.ctypes.data_as(vp), ss.ctypes.data_as(vp), len(caps), 2)
    finally:
        st = np.ones(O.TRAIN_STATS, dtype=np.uint32)
        L.zso_trainStatsGet(st.ctypes.data_as(vp))
    assert rc == 0 and out.tobytes() == b"".join(parts) and int(st.sum()) == 0
    again, _ = O.decode_train_stats(frames, caps, content)
    assert again.tolist() == first.tolist()


def test_candidates_of_the_reference():
    assert T.candidates(65536, 0, 8, 4) == [(k, 8) for k in (50, 537, 1024, 1511, 1998)]
    assert T.candidates(600, 0, 0, 2) == [(50, 6), (50, 8)] and T.candidates(4096, 7, 0, 0) == [(7, 6)]


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="the sanitizer build is a CPU-side check: it runs on machines without a GPU, never next to one")
def test_finalize_under_sanitizers(tmp_path):
    """oracle E's finalize and counters and the trainer's model as one stand-alone program with -fsanitize=address,undefined: every input and
    every output in a heap block of exactly its size; its answers are the library's"""
    exe = str(tmp_path / "dict_finalize")
    oracle = os.path.join(ROOT, "oracle")
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Wno-comment", "-Wno-misleading-indentation", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                           "-I", oracle, os.path.join(ROOT, "tests", "c", "dict_finalize.c"), os.path.join(ROOT, "tests", "c", "train_model.c"),
                           os.path.join(oracle, "zso_encoder.c"), os.path.join(oracle, "zso_decoder.c"), os.path.join(oracle, "zso_batch.c"), "-ldl", "-o", exe])
    inputs = {
        "records": (F.class_samples("json_records")[:24], 4096, 100, 8, 14),
        "edges": ([b"", b"q", F.class_samples("zipf")[0], F.noise(4096, 41), b"\x5A" * 4096, F.noise(4096, 42, 64), F.class_samples("zipf")[1][:17]] + F.class_samples("zipf")[2:8], 2048, 50, 6, 12),
        "blocks": ([X.class_data("xml_records")[:131073]], 8192, 300, 8, 16),
    }
    args = []
    for name, (parts, cap, k, d, f) in sorted(inputs.items()):
        open(str(tmp_path / name), "wb").write(b"".join(parts))
        open(str(tmp_path / (name + ".sizes")), "w").write(" ".join(str(len(p)) for p in parts))
        args += [str(tmp_path / name), str(tmp_path / (name + ".sizes")), str(cap), str(k), str(d), str(f), str(tmp_path / (name + ".dict"))]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = out.stdout.splitlines()
    assert len(rows) == len(inputs)
    for row, (name, (parts, cap, k, d, f)) in zip(rows, sorted(inputs.items())):
        content = T.model_content(parts, cap, k, d, f)
        dic = O.finalize_dictionary(content, parts, cap, 3)
        st = O.train_stats(content, parts, 3)
        assert row.split() == [str(len(content)), str(len(dic)), str(int(st[:256].sum())), str(int(st[256:320].sum()))], name
        assert open(str(tmp_path / (name + ".dict")), "rb").read() == dic
