"""Dictionaries and one mixed batch for the DDict sets (zsmi_createDDictSet: a decode call whose frames name different dictionaries).
tests/test_ddict_set_host.py pins the batch under oracle D on the CPU, tests/test_gpu_ddict_set.py decodes it on the GPU.

The dictionaries: the hand-built ones of tests/_ddict.py - there they all carry ID 77 - under IDs of their own, and 70 small ones over the
narrow Huffman table with different recent offsets and contents, whose IDs need header fields of 1, 2 and 4 bytes.  The batch: the
catalogue of _ddict.cases() for each dictionary with the frames renamed to the new IDs, a frame for each small dictionary, frames that name
no dictionary or one nobody has, truncated frames and an item of two frames that name two members - laid out so that neighbouring items
name different dictionaries.  An item is a dict: name, frames (the item's frames one behind the other), ids (the ID each names, 0: none),
dnames (the dictionary each was written against), cap, content / code (what _ddict states, for the frames decoded with dnames), cut (truncated)."""
import struct
import numpy as np
import _ddict as DD
import _framewriter as W
import _oracle as O

IDS = {"narrow": 11, "reps": 22, "wide": 33, "log12": 44}            # below 256: a renamed frame keeps its 1-byte field
EDGE_IDS = (255, 256, 65535, 65536, 0x7FFFFFFF, 0xFFFFFFFF)
N_SMALL = 70
UNKNOWN_ID = 0x12345678                                              # (and 77, 78: what _ddict's "another ID" frames name)


def with_id(dic, dict_id):
    return dic[:4] + struct.pack("<I", dict_id) + dic[8:]


def small_id(k):
    return EDGE_IDS[k] if k < len(EDGE_IDS) else (300 + 97 * k if k % 3 else 70000 + 7919 * k)


def small_parts(k):
    """(content, recent offsets) of small dictionary k: no two alike"""
    content = DD.text(150 + 3 * k, 40 + k) + DD.CONTENT[k:k + 120] + bytes((k * 7 + j) & 0xFF for j in range(40))
    return content, (1 + k, 5 + 2 * k, 9 + 3 * k)


_dicts = {}


def dictionaries():
    """name -> dictionary: narrow, reps, wide, log12 under IDS, small00 .. small69, and raw (content only: ID 0)"""
    if not _dicts:
        for name, dic in DD.dictionaries().items():
            _dicts[name] = dic if name == "raw" else with_id(dic, IDS[name])
        for k in range(N_SMALL):
            content, reps = small_parts(k)
            _dicts["small%02d" % k] = DD.formatted(DD.narrow_weights(), reps=reps, content=content, dict_id=small_id(k))
        ids = [dict_id(d) for d in _dicts.values()]
        assert len(set(ids)) == len(ids) and not {77, 78, UNKNOWN_ID} & set(ids)
    return _dicts


def dict_id(dic):
    return struct.unpack_from("<I", dic, 4)[0] if dic[:4] == struct.pack("<I", DD.MAGIC_DICT) else 0


def member_order():
    """the formatted dictionaries' names in the order the tests hand them to a set: the hand-built ones first (so that the first 1, 2 and
    4 are those), the small ones shuffled - not sorted by ID anywhere"""
    small = ["small%02d" % k for k in range(N_SMALL)]
    np.random.default_rng(74).shuffle(small)
    order = ["reps", "wide", "narrow", "log12"] + small
    ids = [dict_id(dictionaries()[n]) for n in order]
    assert ids != sorted(ids) and ids[:4] != sorted(ids[:4])
    return order


# ------------------------------------------------------------------ frames
def id_field(frame):
    """(offset, bytes) of a frame's dictID field"""
    return 5, (0, 1, 2, 4)[frame[4] & 3]


def named_id(frame):
    at, n = id_field(frame)
    return int.from_bytes(frame[at:at + n], "little")


def rename(frame, new_id):
    """the frame naming new_id (< 256): a 1-byte field is rewritten, a wider one keeps its width, an absent one is inserted (single-segment
    frames: the field follows the descriptor byte); everything behind the field stays"""
    assert new_id < 256 and frame[4] & 0x20
    at, n = id_field(frame)
    if n == 0:
        return frame[:4] + bytes([frame[4] | 1, new_id]) + frame[5:]
    return frame[:at] + new_id.to_bytes(n, "little") + frame[at + n:]


def small_frame(k):
    """(frame, content) for small dictionary k: Treeless literals on its Huffman table, all three sequence tables repeated from it, a repeat
    code as first offset, matches into its content"""
    content, reps = small_parts(k)
    st = W._State()
    st.out = bytearray(content); st.rep = list(reps)
    st.huf = W.huf_codes(DD.narrow_weights())[0]
    st.tables = {"ll": W.FSE(*DD.LL_NORM), "of": W.FSE(*DD.OF_NORM), "ml": W.FSE(*DD.ML_NORM)}
    blocks = [W.comp(W.Lit("treeless", DD.text(48 + k, 90 + k), streams=1), W.Seqs([(2, 6, 1 + k % 3), (5, 9, 60 + k + 3), (0, 4, 2)], ll="rep", of="rep", ml="rep"))]
    body = b"".join(W._block(b, st, i == len(blocks) - 1) for i, b in enumerate(blocks))
    assert st.ok
    out = bytes(st.out[len(content):])
    did = small_id(k)
    nb = 1 if did < 256 else 2 if did < 65536 else 4
    fhd = (1 << 5) | {1: 1, 2: 2, 4: 3}[nb]
    assert len(out) < 256
    return struct.pack("<I", W.MAGIC) + bytes([fhd]) + did.to_bytes(nb, "little") + bytes([len(out)]) + body, out


_items = []


def items():
    """the mixed batch"""
    if _items:
        return _items
    per = {}

    def add(key, name, frames, ids, dname, cap, content, code, cut=False):
        per.setdefault(key, []).append(dict(name=name, frames=frames, ids=ids, dnames=dname if isinstance(dname, list) else [dname], cap=cap, content=content, code=code, cut=cut))

    for dname in DD.dictionaries():
        names, frames, caps = DD.cases_of(dname)
        want = {c[0]: c for c in DD.cases()}
        for name, f, cap in zip(names, frames, caps):
            # frames written against a formatted dictionary name it under its new ID; left as they are: raw content's frames, the two that are
            # about naming no dictionary, and those that name another ID (78 - which stays an ID nobody has)
            if dname != "raw" and not name.startswith(("j ID field of 0", "j no ID field")) and named_id(f) in (0, DD.DICT_ID):
                f = rename(f, IDS[dname])
            add(dname, name, [f], [named_id(f)], dname, cap, want[name][3], want[name][4])
    for k in range(N_SMALL):
        f, out = small_frame(k)
        add("small", "small dictionary %d, ID %#x" % (k, small_id(k)), [f], [small_id(k)], "small%02d" % k, len(out), out, 0)
    flat = {it["name"]: it for v in per.values() for it in v}
    a, b = flat["e treeless 4 streams [narrow]"], flat["f repeat mode all, treeless [reps]"]
    add("misc", "two frames, two members", a["frames"] + b["frames"], a["ids"] + b["ids"], a["dnames"] + b["dnames"], len(a["content"]) + len(b["content"]), a["content"] + b["content"], 0)
    f = flat["small dictionary 7, ID %#x" % small_id(7)]["frames"][0]
    assert id_field(f)[1] == 2
    add("misc", "an ID nobody has, 4 bytes", [f[:4] + bytes([f[4] | 3]) + UNKNOWN_ID.to_bytes(4, "little") + f[7:]], [UNKNOWN_ID], "small07", 512, None, 32)
    for key, name in (("narrow", "e treeless 4 streams [narrow]"), ("reps", "f repeat mode all, treeless [reps]"), ("wide", "k treeless with a flat-class table, 4 streams"),
                      ("raw", "b long match over the content's end, overlapping [raw]"), ("small", "small dictionary 3, ID %#x" % small_id(3))):
        it = flat[name]
        f = it["frames"][0]
        for what, g in (("cut in half", f[:len(f) // 2]), ("cut by 3 bytes", f[:-3])):
            add(key, name + ", " + what, [g], it["ids"], it["dnames"], 512, None, None, cut=True)
    # neighbours name different dictionaries: every list is spread evenly over the batch
    order = sorted(((j + 0.5) / len(v), key, j) for key, v in per.items() for j in range(len(v)))
    _items.extend(per[key][j] for _, key, j in order)
    return _items


def single_frame(item):
    return len(item["frames"]) == 1


# ------------------------------------------------------------------ the rule, and oracle D under it
def pick(frame_id, members, unnamed):
    """the name of the dictionary a frame that names frame_id gets from the set (members: names; unnamed: a name or None) - None: no
    dictionary; "wrong": it names an ID nobody has"""
    D = dictionaries()
    if frame_id == 0:
        return unnamed
    for name in list(members) + ([unnamed] if unnamed else []):
        if dict_id(D[name]) == frame_id:
            return name
    return "wrong"


def stated(item, members, unnamed):
    """what the helper states an item gives under the set: (content, 0), (None, code), or None where it states nothing (a truncated frame; a
    frame that names no dictionary decoded with another one than it was written against)"""
    if item["cut"]:
        return None
    picks = [pick(i, members, unnamed) for i in item["ids"]]
    if picks[0] == "wrong":
        return None, 32                                    # (the test behind the frame header: every frame here has a valid one)
    if picks == item["dnames"]:
        return item["content"], item["code"]
    return None


def oracle_item(item, members, unnamed):
    """oracle D frame by frame, each with the dictionary the rule picks, in the library's words: (size, bytes) or (the error word, b"")"""
    D = dictionaries()
    out = b""
    for f, i in zip(item["frames"], item["ids"]):
        p = pick(i, members, unnamed)
        try:
            out += O.decompress_using_dict(f, item["cap"] - len(out), D[p]) if p not in (None, "wrong") else O.decompress(f, item["cap"] - len(out))
        except O.OracleError as e:
            return 0x100000000 - e.code, b""
    return len(out), out


def configurations():
    """(members, unnamed) of the sets the mixed batch is decoded with: the first 1, 2, 4 and 74 of member_order() - more than a wavefront
    has lanes -, without `unnamed`, with the raw-content dictionary, and with a formatted one (narrow, which leaves the list: it is a
    member by being `unnamed`)"""
    out = []
    for unnamed in (None, "raw", "narrow"):
        order = [n for n in member_order() if n != unnamed]
        for k in (1, 2, 4, 74):
            out.append((order[:k], unnamed))
    return out
