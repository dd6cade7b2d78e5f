"""Members and one mixed batch for the CDict sets (zsmi_createCDictSet: a compress call whose chunks use different dictionaries).
tests/test_cdict_set_host.py pins the batch on the CPU, tests/test_gpu_cdict_set.py compresses it on the GPU.

The members, in the order a set gets them: every dictionary of _dicts.identity_dictionaries() (raw content of 1 .. 100 000 bytes, the trained
ones, other recent offsets, content over 64 KiB), the seven _dicts.id_dictionaries() (ID fields of 0, 1, 2 and 4 bytes), the narrow
dictionary of _cdict, an empty CDict, and the first trained dictionary once more - one CDict at two indices.  The batch: each member's
_dicts.prefix_chunks (an empty member: those of a raw dictionary), as many chunks again that use no dictionary, dealt out so that
neighbours differ - see deal().  An item is (chunk, choice): the member's index or NO_DICT."""
import numpy as np
import _dicts as X
import _cdict as K
import _batch as B

NO_DICT = 0xFFFFFFFF
BLOCK = 65536
GROUP = 4                      # ZS_SEQ_GROUP: blocks a workgroup of the sequences kernel
SIZES_EVERY_KIND_HAS = (0, 1, 65536, 65537, 131073, 200 * 1024)

_members = []


def members():
    """[(name, dictionary bytes)]; b"" is the empty CDict; `again` names the member listed a second time (the same CDict object)"""
    if not _members:
        _members.extend(X.identity_dictionaries().items())
        _members.extend(("id_%#x" % i, d) for i, d in X.id_dictionaries().items())
        _members.append(("narrow", K.narrow_dictionary()))
        _members.append(("empty", b""))
        _members.append(("again", X.TRAINED8K))
    return _members


AGAIN_OF = "trained8k"


def kind(choice):
    """"none", "raw" or "formatted": what the chunk's frame is stated by (an empty member: none)"""
    if choice == NO_DICT:
        return "none"
    dic = members()[choice][1]
    return "none" if not dic else ("formatted" if dic[:4] == (0xEC30A437).to_bytes(4, "little") else "raw")


def dictionary(choice):
    """the bytes a chunk with this choice is compressed and decoded with (b"": none)"""
    return b"" if choice == NO_DICT else members()[choice][1]


def blocks_of_size(n):
    return max((n + BLOCK - 1) // BLOCK, 1)


def groups_ok(items, at=None):
    """the dealing's properties, or the index of the first chunk where one fails: neighbours differ; every aligned group of GROUP chunks
    and every aligned group of GROUP blocks holds two different choices"""
    owner = []
    for i, (c, choice) in enumerate(items):
        if i and items[i - 1][1] == choice:
            return i
        owner += [i] * blocks_of_size(len(c))
    for g in range(0, len(items) - GROUP + 1, GROUP):
        if len({ch for _, ch in items[g:g + GROUP]}) < 2:
            return g
    for g in range(0, len(owner) - GROUP + 1, GROUP):
        if len({items[i][1] for i in owner[g:g + GROUP]}) < 2:
            return owner[g]
    return None


_items = []


def deal():
    """the mixed batch.  The members' chunks go round robin - the members in an order that alternates raw and formatted ones while both
    last, each member's list turned by its index - with a NO_DICT chunk in front of each: NO_DICT, a member, NO_DICT, the next member ..."""
    if _items:
        return _items
    M = members()
    per = {}
    for k, (name, dic) in enumerate(M):
        c = X.prefix_chunks(dic if dic else X.STREAM[:6000])
        per[k] = c[k:] + c[:k]                                             # (staggered: the members' long chunks do not meet)
    n_member = sum(len(v) for v in per.values())
    small = [c for k in sorted(per) for c in per[k] if len(c) <= 4096]
    none = list(X.prefix_chunks(X.STREAM[:6000]))
    none += [small[(j * 7) % len(small)] for j in range(n_member - len(none))]
    raw = [k for k in per if kind(k) == "raw"]
    other = [k for k in per if kind(k) != "raw"]
    order = []
    while raw or other:
        if other:
            order.append(other.pop(0))
        if raw:
            order.append(raw.pop(0))
    assert len({len(v) for v in per.values()}) == 1                      # (so that round robin over the members is an even spread)
    ranked = [(j * len(order) + order.index(k), 1, k, j) for k in per for j in range(len(per[k]))]
    ranked += [(j, 0, NO_DICT, j) for j in range(len(none))]
    items = [((none if k == NO_DICT else per[k])[j], k) for _, _, k, j in sorted(ranked)]
    # what is left: a chunk of four blocks that fills an aligned group of four blocks alone.  It changes places with a chunk of the same kind
    # of choice a few places on, the nearest with which the batch is in order up to a later chunk
    for _ in range(len(items)):
        bad = groups_ok(items)
        if bad is None:
            break
        for j in range(bad + 2, len(items), 2):
            items[bad], items[j] = items[j], items[bad]
            now = groups_ok(items)
            if now is None or now > j:
                break
            items[bad], items[j] = items[j], items[bad]
        else:
            raise AssertionError("no place for chunk %d" % bad)
    assert groups_ok(items) is None
    _items.extend(items)
    return _items


def chunks():
    return [c for c, _ in deal()]


def choices():
    return np.array([ch for _, ch in deal()], dtype=np.uint32)


_oracle = {}


def oracle_frames(level):
    """{index in the batch: oracle E's frame} for the chunks whose choice is raw content, NO_DICT or the empty member (a formatted member's
    frames may use its tables: no oracle writes those), computed once a level"""
    if level not in _oracle:
        items = deal()
        by_dic = {}
        for i, (c, choice) in enumerate(items):
            if kind(choice) != "formatted":
                by_dic.setdefault(dictionary(choice), []).append(i)
        out = {}
        for dic, idx in by_dic.items():
            for i, f in zip(idx, B.oracle_frames([items[i][0] for i in idx], level, dic)):
                out[i] = f
        _oracle[level] = out
    return _oracle[level]
