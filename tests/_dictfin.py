"""Inputs of the exact tests of dictionary finalize and of the trainer's search and selection borders, with the reach check of each: what
shows, without a GPU, that the input hits the border it is named for.  tests/test_dict_finalize_host.py runs every reach check on the
oracle and the model; tests/test_gpu_dict_finalize.py and tests/test_gpu_dict_train_exact.py hold the GPU to the same inputs."""
import numpy as np
import _oracle as O
import _dicts as X
import _train as T
import _framewriter as W

TILE = 8192                     # window ends k_train_select scores in one pass: kTrainThreads * kTrainPerThread
LINK_CAP = 65535                # k_train_links: a distance at or beyond this reads "none within reach"
LIT_LIMIT, CODE_LIMIT = 1 << 23, 1 << 30

_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def noise(n, seed, high=256):
    return np.random.default_rng(seed).integers(0, high, n, dtype=np.uint8).tobytes()


def class_samples(cls):
    return T.samples(cls, 1 << 18)


def class_content(cls):
    """the 16 KiB model content of a class's 256 KiB of samples"""
    return memo(("content", cls), lambda: T.model_content(class_samples(cls), 16384, 200, 8, 16))


# ------------------------------------------------------------------ finalize: name -> (content, samples, cap, level, dictID)
def _hidden(reverse):
    o = class_samples("json_records")
    parts = [o[0], noise(4096, 41), o[1], b"\xA5" * 4096, o[2], noise(4096, 42, 64), o[3], o[4][:20], o[5], b"\xC3" * 4100, o[6]]
    return parts[::-1] if reverse else parts


def _halving(short=0):
    """the smallest input that makes the literal counters halve: their sum + 256 is exactly 2^23 (`short`: that many fewer).  8 MiB of
    noise over 31 byte values, nearly all of it literals: those 31 take codes of 5 and 6 bits, the other 225 values codes of 11 bits, and
    what the 31 leave of the code space lets about 31 of the 225 have 10 bits - the most frequent ones.  The 225 are counted only in one
    small sample that holds byte v (v % 7) times: counts of 0 .. 6 whose order, + 1 and halved (1 1 1 2 2 3 3), is another than unhalved
    (1 .. 7) or halved otherwise.  Then noise for most of what the sum still lacks and samples of 15 bytes or fewer (all literals by rule)
    for the rest.  No records among the samples: a value of middling frequency would take the spare code space"""
    def make():
        lits = lambda parts: int(O.train_stats(class_content("xml_records"), parts, 3)[:256].sum())
        rare = np.random.default_rng(9).permutation(np.repeat(np.arange(31, 256, dtype=np.uint8), np.arange(31, 256) % 7)).tobytes()
        parts = [noise(65536, 100 + i, 31) for i in range(128)] + [rare]
        have = lits(parts) + 256
        assert 4096 < LIT_LIMIT - have <= 65536, LIT_LIMIT - have
        parts.append(noise(LIT_LIMIT - have - 2048, 99, 31))
        lack = LIT_LIMIT - 256 - lits(parts)
        assert 0 < lack < 4096, lack
        tail = noise(lack, 98, 31)
        return parts + [tail[i:i + 15] for i in range(0, lack, 15)]
    parts = memo("halving", make)
    return parts[:-1] + [parts[-1][:-1]] if short else parts


def finalize_cases():
    c = {}
    for cls in X.RECORD_CLASSES:
        for cap in (16384, 65536):
            for level in (1, 3):
                c[f"a_{cls}_cap{cap}_l{level}"] = lambda cls=cls, cap=cap, level=level: (class_content(cls), class_samples(cls), cap, level, 0)
    for size in (131071, 131072):
        c[f"b_content{size}"] = lambda size=size: (X.class_data("json_records")[:size], class_samples("json_records"), size + 1024, 3, 0)
    # (the front cut.  Every cap here still gives a dictionary: the other way to "cannot be made", a section that leaves no room for content
    # at cap 256, needs a section of 244 bytes or more, and the largest that mixed classes and synthetic parses gave was 186; unreached)
    content4000 = lambda: class_content("csv_records")[-4000:]
    for cap in (256, 300, 512, 4064):
        c[f"c_cap{cap}"] = lambda cap=cap: (content4000(), class_samples("csv_records"), cap, 3, 0)
    c["c_no_literals"] = lambda: (content4000(), [content4000()[:2000], content4000()[1000:3000]], 4096, 3, 0)
    o = lambda: class_samples("zipf")
    c["d_size_edges"] = lambda: (class_content("zipf"), [o()[0], b"", o()[1], b"q", o()[2], o()[3][:15], o()[4][:16], o()[5][:17], o()[6]], 16384, 3, 0)
    c["d_size_edges_without_empty"] = lambda: (class_content("zipf"), [o()[0], o()[1], b"q", o()[2], o()[3][:15], o()[4][:16], o()[5][:17], o()[6]], 16384, 3, 0)
    big = lambda at, n: X.class_data("xml_records")[at:at + n]
    c["e_three_blocks_and_five"] = lambda: (class_content("xml_records"), [big(0, 131073), big(131073, 300 << 10)], 16384, 3, 0)
    c["f_hidden_parses"] = lambda: (class_content("json_records"), _hidden(False), 16384, 3, 0)
    c["f_hidden_parses_reversed"] = lambda: (class_content("json_records"), _hidden(True), 16384, 3, 0)
    c["g_literal_halving"] = lambda: (class_content("xml_records"), _halving(), 16384, 3, 0)
    c["g_one_below_halving"] = lambda: (class_content("xml_records"), _halving(1), 16384, 3, 0)
    c["j_given_id"] = lambda: (class_content("binary_table"), class_samples("binary_table"), 16384, 3, 77)
    return c


FINALIZE = finalize_cases()


def outcome(case):
    """the oracle's answer to a finalize case, computed once: the dictionary, or the error code the GPU call must return (70 where the
    oracle answers 0: the dictionary cannot be made)"""
    def make():
        content, parts, cap, level, did = FINALIZE[case]()
        try:
            dic = O.finalize_dictionary(content, parts, cap, level, did)
        except O.OracleError as e:
            return e.code
        return T.E_DST_TOO_SMALL if dic is None else dic
    return memo(("outcome", case), make)


def stats_of(case):
    content, parts, cap, level, did = FINALIZE[case]()
    return memo(("stats", case), lambda: O.train_stats(content, parts, level))


def frames_of(case):
    content, parts, cap, level, did = FINALIZE[case]()
    return [O.compress_using_dict(p, content, level) for p in parts]


def of_symbols(dic):
    """symbols of a dictionary's OF table"""
    content = T.check_format(dic, len(dic))
    return min((len(content) + (128 << 10)).bit_length() - 1, 31) + 1


def reach_finalize(case):
    """asserts that the case's input reaches what it is named for (cases without a border of their own: nothing to show)"""
    content, parts, cap, level, did = FINALIZE[case]()
    out = outcome(case)
    if case.startswith("b_"):
        assert (len(content) + (128 << 10)).bit_length() - 1 == (17 if len(content) == 131071 else 18)
        assert len(out) == cap - 1024 + (len(out) - len(content)) and of_symbols(out) == (18 if len(content) == 131071 else 19)   # nothing cut
    elif case == "c_no_literals":
        assert out == T.E_DST_TOO_SMALL and int(stats_of(case)[:256].sum()) == 0       # 256 equal counts: one weight, which no description holds
    elif case.startswith("c_"):
        assert len(out) == cap and out.endswith(content[-(cap - 200):]) and not out.endswith(content)      # cut at the front, the section is < 200 bytes
    elif case.startswith("d_"):
        sizes = sorted(map(len, parts))[:5]
        assert sizes == ([0, 1, 15, 16, 17] if "without" not in case else [1, 15, 16, 17, len(sorted(parts, key=len)[4])])
        assert isinstance(out, bytes)
    elif case.startswith("e_"):
        nblocks = [len(list(W.blocks(f))) for f in frames_of(case)]
        assert nblocks == [3, 5]
        assert len(parts[0]) == 2 * 65536 + 1                                               # a third block of one byte: under 16, all literals
    elif case.startswith("f_"):
        seen = set()
        for p, f in zip(parts, frames_of(case)):
            for b in W.blocks(f):
                seen.add(("raw", "rle", "compressed")[b.type] + ("_nseq0" if b.type == 2 and b.nseq == 0 else ""))
        assert {"raw", "rle", "compressed_nseq0", "compressed"} <= seen, seen
        st = stats_of(case)
        assert int(st[0xA5]) >= 4096, "a unit of one byte, a multiple of 16 long, is not parsed: its bytes are literals"
        assert int(st[0xC3]) < 64, "a ragged unit of one byte is parsed: its bytes are matches"
    elif case.startswith("g_"):
        st = stats_of(case)
        assert int(st[:256].astype(np.uint64).sum()) + 256 == LIT_LIMIT - ("below" in case)
        assert sorted(set(st[31:256].tolist())) == list(range(7))                           # the small counts the rounding shows on
        assert outcome("g_literal_halving") != outcome("g_one_below_halving")
        for lo, n in ((256, 36), (320, 32), (384, 53)):
            assert int(st[lo:lo + n].astype(np.uint64).sum()) + n < CODE_LIMIT                 # (the codes' halving: out of a test's reach)
    elif case.startswith("j_"):
        assert int.from_bytes(out[4:8], "little") == 77


# ------------------------------------------------------------------ selection borders: name -> (samples, cap, k, d, f)
def epochs(total, cap, k):
    """(nbDmers, number of epochs, d-mers an epoch) as k_train_select and the model cut them"""
    nb = total - 7
    num = max(1, cap // k // 4)
    size = nb // num
    if size < 10 * k:
        size = min(10 * k, nb)
        num = nb // size
    return nb, num, size


def _cut(data, seed=7):
    return T.cut(data, seed)


def _island(before, length, after, seed):
    """samples of 7 bytes (no d-mer of theirs lies inside its sample: their frequencies stay 0), one sample of `length` bytes, more of 7"""
    r = noise(7 * (before + after) + length, seed)
    parts = [r[7 * i:7 * i + 7] for i in range(before)] + [r[7 * before:7 * before + length]]
    return parts + [r[7 * before + length + 7 * i:7 * before + length + 7 * i + 7] for i in range(after)]


def _pattern_epochs():
    """five stretches of 12000 bytes, each one 64-byte pattern repeated: every full window of a stretch has the same score; then 12000
    bytes of records (with nothing but the patterns no literal is left to build a Huffman table from)"""
    return [noise(64, 300 + i) * 187 + noise(64, 300 + i)[:32] for i in range(5)] + [X.class_data("json_records")[:12000]]


def _recurrences():
    """a d-mer that recurs at distance 65534, 65535 and 65536 inside the one epoch, as the links store it: exact, at the cap, capped.
    What this can show is limited: a window holds at most L = 65531 d-mers (k = 65536, d = 6; here 65529), so all three distances lie
    outside every window and an exact link and a saturated one must behave alike - a distance that wrapped in 16 bits would show, an
    off-by-one in the cap of 65535 would not."""
    data = bytearray(noise(500000, 77) + noise(10 * 65536 + 7 - 500000, 78, 64))           # (six-bit noise behind: literal counts a table can be built from)
    for at, dist, mark in ((100000, 65534, b"MARKER-A"), (250000, 65535, b"MARKER-B"), (400000, 65536, b"MARKER-C")):
        data[at:at + 8] = mark; data[at + dist:at + dist + 8] = mark
    return _cut(bytes(data))


def select_cases():
    j = lambda n: X.class_data("json_records")[:n]
    c = {}
    for nb in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        c[f"epoch_{nb}"] = lambda nb=nb: (_cut(j(nb + 7)), 4096, 1000, 8, 20)
    c["k_equals_d6"] = lambda: (class_samples("csv_records")[:24], 4096, 6, 6, 16)
    c["k_equals_d8"] = lambda: (class_samples("csv_records")[:24], 4096, 8, 8, 16)
    c["k65536"] = lambda: (_cut(T.TRAINING["xml_records"](10 * 65536 + 7)), 65536, 65536, 8, 20)
    c["ties_everywhere"] = lambda: (_pattern_epochs(), 4800, 200, 8, 20)
    c["best_at_last_end"] = lambda: (_island(1500, 199, 0, 51), 512, 199, 8, 20)
    c["best_at_second_tile"] = lambda: (_island((TILE + 1 - 192) // 7, 199, 600, 52), 512, 199, 8, 20)
    c["recurrences_at_link_cap"] = lambda: (_recurrences(), 65536, 65536, 8, 20)
    c["f12_d6"] = lambda: (class_samples("json_records"), 16384, 200, 6, 12)
    c["cap_over_samples"] = lambda: (T.samples("zipf", 30000), 65536, 500, 8, 20)
    return c


SELECT = select_cases()


def select_reference(case):
    parts, cap, k, d, f = SELECT[case]()
    return memo(("select", case), lambda: T.reference_train(parts, cap, k, d, f, 0, 1.0, 3))


def _hashes(data, d, f):
    """the trainer's hash of every d-mer start (8 bytes readable)"""
    a = np.frombuffer(data, dtype=np.uint8).astype(np.uint64)
    v = np.zeros(len(data) - 7, dtype=np.uint64)
    for i in range(8):
        v |= a[i:len(data) - 7 + i] << np.uint64(8 * i)
    with np.errstate(over="ignore"):
        h = (v << np.uint64(16)) * np.uint64(227718039650203) if d == 6 else v * np.uint64(0xCF1BBCDCB7A56463)
    return (h >> np.uint64(64 - f)).astype(np.int64)


def first_epoch_scores(parts, cap, k, d, f):
    """score of every window end e in [1, size] of epoch 0 at the first visit: the summed frequency of the distinct hashes of the d-mers
    [max(0, e - L), e), frequencies counted over the d-mers that lie inside their sample"""
    data = b"".join(parts)
    nb, num, size = epochs(len(data), cap, k)
    h = _hashes(data, d, f)
    inside = np.zeros(len(h), dtype=bool)
    at = 0
    for p in parts:
        if len(p) >= 8:
            inside[at:at + len(p) - 7] = True
        at += len(p)
    freq = np.bincount(h[inside], minlength=1 << f)
    L = k - d + 1
    return np.array([int(freq[np.unique(h[max(0, e - L):e])].sum()) for e in range(1, size + 1)])


def reach_select(case):
    parts, cap, k, d, f = SELECT[case]()
    total = sum(map(len, parts))
    nb, num, size = epochs(total, cap, k)
    L = k - d + 1
    if case.startswith("epoch_"):
        assert num == 1 and size == nb == int(case.split("_")[1])                      # the ends of the one epoch: 1 .. size
    elif case.startswith("k_equals_d"):
        assert L == 1 and num > 1
    elif case == "k65536":
        assert (L, num, size) == (65529, 1, 655360) and size == nb == 10 * k           # the fewest d-mers an epoch may have
    elif case == "ties_everywhere":
        s = first_epoch_scores(parts, cap, k, d, f)
        best = np.flatnonzero(s == s.max()) + 1
        assert size > TILE and best[0] < 128 and len(best) > TILE and best[-1] > TILE      # ties in the first wavefront, across all and in the second tile
    elif case == "best_at_last_end":
        s = first_epoch_scores(parts, cap, k, d, f)
        assert num == 1 and size > TILE and np.flatnonzero(s == s.max()).tolist() == [size - 1]
    elif case == "best_at_second_tile":
        s = first_epoch_scores(parts, cap, k, d, f)
        assert num == 1 and np.flatnonzero(s == s.max()).tolist() == [TILE]               # end e = TILE + 1: the first of the second pass
    elif case == "recurrences_at_link_cap":
        data = b"".join(parts)
        assert num == 1 and size == 655360
        for mark, dist in ((b"MARKER-A", LINK_CAP - 1), (b"MARKER-B", LINK_CAP), (b"MARKER-C", LINK_CAP + 1)):
            at = data.find(mark)
            assert data.find(mark, at + 1) == at + dist and at + dist < size and dist > L - 1
    elif case == "f12_d6":
        assert (f, d) == (12, 6)
    elif case == "cap_over_samples":
        content = select_reference(case)[3]
        assert num >= 1 and len(content) < cap - 8                                       # not full: the epochs ran dry ten times in a row


# ------------------------------------------------------------------ the search: name -> (samples, cap, the call's parameters)
def search_cases():
    s = lambda cls="json_records": class_samples(cls)
    c = {}
    c["k_searched"] = lambda: (s(), 16384, dict(k=0, d=8, steps=4))
    c["k_and_d_searched"] = lambda: (s("csv_records"), 16384, dict(k=0, d=0, steps=2))
    c["d_searched"] = lambda: (s("xml_records"), 16384, dict(k=200, d=0))
    c["split_half"] = lambda: (s("zipf"), 16384, dict(k=0, d=8, steps=4, split=0.5))
    c["split_three_quarters"] = lambda: (s("binary_table"), 16384, dict(k=0, d=8, steps=4, split=0.75))
    c["split_one"] = lambda: (s("binary_table"), 16384, dict(k=0, d=8, steps=4, split=1.0))
    c["one_sample"] = lambda: ([b"".join(s()[:12])], 8192, dict(k=0, d=8, steps=4))
    c["three_samples"] = lambda: ([b"".join(s()[:8]), b"".join(s()[8:16]), b"".join(s()[16:24])], 8192, dict(k=0, d=6, steps=4))
    tie = lambda j, n: ([b"".join(s()[:8]), b"".join(s()[8:16]), b"".join(s()[16:24]), s()[j][:n]], 8192, dict(k=0, d=0, steps=4))
    c["tie_of_two"] = lambda: tie(32, 400)                 # one short held-out sample: few totals are possible, and the smallest is shared
    c["tie_of_three"] = lambda: tie(45, 300)
    c["level_1"] = lambda: (s("csv_records"), 16384, dict(k=0, d=8, steps=4, level=1))
    c["two_groups_f26"] = lambda: (T.samples("csv_records", 1 << 16), 16384, dict(k=0, d=0, steps=4, f=26))
    return c


SEARCH = search_cases()
GROUP_BYTES = 2 << 30           # trainImpl: candidates go in groups whose frequency tables (4 << f bytes each) fit this


def search_reference(case):
    parts, cap, kw = SEARCH[case]()
    return memo(("search", case), lambda: T.reference_train(parts, cap, **kw))


def reach_search(case):
    parts, cap, kw = SEARCH[case]()
    nt, held = T.training_share(parts, kw.get("k", 0), kw.get("d", 0), kw.get("split", 0.0))
    cands = T.candidates(cap, kw.get("k", 0), kw.get("d", 0), kw.get("steps", 0))
    dic, k, d, content, scores = search_reference(case)
    assert isinstance(dic, bytes) and len(cands) > 1 and len(set(scores)) > 1          # the scores tell candidates apart
    if case.startswith("tie_"):
        tied = [c for c, v in zip(cands, scores) if v == min(scores)]
        assert (len(parts), nt, len(held)) == (4, 3, 1) and len(tied) == int(case == "tie_of_three") + 2
        assert (k, d) == min(tied) != tied[0], tied                    # the smaller k, then the smaller d: not the candidate seen first
        assert case == "tie_of_two" or (k, d) != tied[-1]              # ... nor, of three, the one seen last
    elif case == "split_half":
        assert nt == len(parts) // 2 and len(held) == len(parts) - nt
    elif case == "split_one":
        assert nt == len(parts) and held == parts
    elif case == "one_sample":
        assert (len(parts), nt) == (1, 1) and held == parts
    elif case == "three_samples":
        assert (len(parts), nt, len(held)) == (3, 2, 1)
    elif case == "two_groups_f26":
        group = GROUP_BYTES // (4 << kw["f"])
        assert (len(cands), group) == (10, 8) and group < len(cands)
        assert cands.index((k, d)) >= group                                               # the winner's table is one the second group made
    elif case in ("k_searched", "split_three_quarters", "level_1"):
        assert nt == int(len(parts) * 0.75) and len(cands) == 5
    elif case == "k_and_d_searched":
        assert len(cands) == 6 and {c[1] for c in cands} == {6, 8}
    elif case == "d_searched":
        assert cands == [(200, 6), (200, 8)]
