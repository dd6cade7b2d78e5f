"""The scratch-independence tests' inputs reach what they claim, and their hook forgets no buffer - checked on the CPU.
tests/test_gpu_scratch_independence.py runs every call family on a context whose scratch was overwritten (tests/_poison.py); that says
something only if the compress batch really holds a block of every kind the kernels treat differently, if the decode catalogue really
fails in every way, and if the fill covers every buffer a zsmi_ctx owns."""
import ctypes, os, re, subprocess, sys
import pytest
import _cdict as K, _edge_catalogue as C, _framewriter as W, _oracle as O, _poison as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTX_H = os.path.join(ROOT, "zstandard_amd", "csrc", "zsmi_ctx.h")


@pytest.mark.parametrize("level", P.LEVELS)
def test_the_compress_batch_holds_every_kind_of_block(level):
    """oracle E's frames of the batch, parsed: a raw block, an RLE block, a compressed block without sequences, one with the three predefined
    tables, one with three RLE tables, a frame of two blocks and one of four"""
    frames = [O.compress(c, level) for _, c in P.chunks()]
    blocks = [b for f in frames for b in K.blocks_of(f)]
    shapes = [s for f in frames for s in W.entropy_shapes(f)]
    counts = [len(K.blocks_of(f)) for f in frames]
    assert any(b[0] == 0 for b in blocks), "a raw block"
    assert any(b[0] == 1 for b in blocks), "an RLE block"
    assert any(s is not None and s.nseq == 0 for s in shapes), "a compressed block with nseq 0"
    assert any(s is not None and s.tables == ["pre", "pre", "pre"] for s in shapes), "a predefined-table block"
    assert any(s is not None and s.tables == ["rle", "rle", "rle"] for s in shapes), "an all-RLE-table block"
    assert 2 in counts and 4 in counts, counts
    # and the chunks are the sizes the kernels' paths turn on
    sizes = [len(c) for _, c in P.chunks()]
    assert sizes[:10] == [0, 1, 200, 8193, 65536, 65536, 4000, 65537, 131072, 204800]
    by_name = dict(zip((n for n, _ in P.chunks()), frames))
    assert K.blocks_of(by_name["noise 64 KiB"]) == [(0, None, None)] and K.blocks_of(by_name["one byte x 64 KiB"]) == [(1, None, None)]
    assert [b[0] for b in K.blocks_of(by_name["text 65537"])] == [2, 1]                          # the second block is 1 byte: an RLE block
    assert W.entropy_shapes(by_name["noise with one repeat"])[0].nseq == 1


def test_the_dictionary_batch_is_the_batch_trimmed():
    sizes = [len(c) for _, c in P.dict_chunks()]
    assert max(sizes) == 65537 and sorted(sizes)[-2] == 65536 and 0 in sizes and 1 in sizes


def test_the_orders_move_every_chunk():
    n = len(P.chunks())
    o = P.orders(n)
    assert o["reversed"] == o["as listed"][::-1] and o["rotated by three"][0] == 3 and sorted(o["rotated by three"]) == o["as listed"]


def test_the_catalogue_fails_in_every_way():
    """items of every `expect` kind: the frames that decode, and each of the reference's error codes the catalogue pins"""
    kinds = {e.expect for e in C.catalogue()}
    assert kinds == {"ok", 10, C.PAR, C.WIN, C.COR, C.CK, C.DIC, C.DICW, C.DST, C.SRC}
    assert sum(e.expect != "ok" for e in C.catalogue()) >= 100


def declared_buffers(text):
    """[(type, member)] of every DevBuf, PinBuf and TurnBufs member declared in zsmi_ctx.h (an array counts once), outside the
    definitions of those three types themselves"""
    code = re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)
    code = re.sub(r"struct TurnBufs \{.*?\n\};", "", code, flags=re.S)
    found = []
    for m in re.finditer(r"\b(DevBuf|PinBuf|TurnBufs)\s+([A-Za-z_][^;()]*);", code):
        if "typedef" in code[code.rfind("\n", 0, m.start()) + 1:m.start()]:
            continue
        for name in m.group(2).split(","):
            found.append((m.group(1), re.sub(r"\[.*?\]", "", name).strip()))
    return found


@pytest.fixture(scope="module")
def inventory():
    # (the debug-hook library, made if it is missing or stale: tests/test_scratch_layout.py does the same)
    env = dict(os.environ, ZSMI_DEBUG_LIB="1")
    path = subprocess.check_output([sys.executable, "-c", "from zstandard_amd import _lib; print(_lib.build())"], env=env, cwd=ROOT, text=True).strip().splitlines()[-1]
    from zstandard_amd import _lib
    return _lib.scratch_inventory(ctypes.CDLL(path))


def test_every_buffer_of_the_context_is_in_the_inventory(inventory):
    """every DevBuf, PinBuf or TurnBufs member of zsmi_ctx.h is named by zsmi_dbg_scratchInventory, as filled or as state: a buffer added to
    the context cannot be forgotten by the fill"""
    declared = declared_buffers(open(CTX_H).read())
    assert len(declared) >= 55 and ("DevBuf", "dScan") in declared and ("TurnBufs", "hLists") in declared and ("PinBuf", "hCand") in declared
    named = [m for _, kind, m in inventory if kind in ("filled", "state") and not m.endswith(".turns")]
    last = [m.split(".")[-1] for m in named]
    for _, member in declared:
        assert member in last, (member, "is declared in zsmi_ctx.h and missing from zsmi_dbg_scratchInventory")
    # a name declared in two structs (dChunks: the plan's and the resident plan's) is listed once for each
    assert sorted(last) == sorted(m for _, m in declared), (sorted(set(last) ^ {m for _, m in declared}))
    assert len(set(named)) == len(named)


def test_the_inventory_says_what_is_forgotten_and_what_is_kept(inventory):
    groups = {g for g, _, _ in inventory}
    from zstandard_amd import _lib
    assert groups == set(_lib.FILL_GROUPS)
    assert {m for _, kind, m in inventory if kind == "forgotten"} == {"plan.key", "plan.dictKey", "plan.dictKind"}
    assert {m for _, kind, m in inventory if kind == "state"} == {"hItems.turns", "seek.hLists.turns", "plan.hDictList.turns"}
    assert ("compress", "filled", "scratch.buf") in inventory and ("train", "filled", "train.hCand") in inventory


def test_the_hook_is_not_in_the_product():
    """neither the public header nor the product library's export list names it"""
    from zstandard_amd import _lib
    assert "zsmi_dbg_" not in open(os.path.join(ROOT, "include", "zsmi.h")).read()
    assert not [e for e in _lib.EXPORTS if "dbg" in e]
    src = open(os.path.join(ROOT, "zstandard_amd", "csrc", "zsmi_api.hip")).read()
    at = src.rindex("#ifdef ZSMI_DEBUG_HOOKS")
    assert src.index("zsmi_dbg_fillScratch") > at and src.index("zsmi_dbg_scratchInventory") > at and src.rstrip().endswith("#endif")
