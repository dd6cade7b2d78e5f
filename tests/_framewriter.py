"""A spec-level zstd frame writer (RFC 8878).  TEST INFRASTRUCTURE, not a compressor: it writes exactly the plan it is given -
header fields, block types, literal and sequence encodings, table modes, sequences - whether that plan is valid or not, and returns the
content the plan stands for (None where the plan has no content, e.g. an offset reaching before the frame start).

FSE and Huffman streams are written by inverting the spec's DECODING tables (RFC 8878 §4.1.1, §4.2.1): to emit a symbol whose
successor state is known, take the state that decodes that symbol and whose [baseline, baseline + 2^nbBits) range covers the successor.
No encoder heuristics; numpy-free plain Python.  Section references below are to RFC 8878."""
import struct
from types import SimpleNamespace

MAGIC = 0xFD2FB528
MASK64 = (1 << 64) - 1

# §3.1.1.3.2.1.1 codes: (baseline, extra bits)
LL_CODES = [(i, 0) for i in range(16)] + [(16, 1), (18, 1), (20, 1), (22, 1), (24, 2), (28, 2), (32, 3), (40, 3), (48, 4), (64, 6),
                                          (128, 7), (256, 8), (512, 9), (1024, 10), (2048, 11), (4096, 12), (8192, 13), (16384, 14),
                                          (32768, 15), (65536, 16)]
ML_CODES = [(i + 3, 0) for i in range(32)] + [(35, 1), (37, 1), (39, 1), (41, 1), (43, 2), (47, 2), (51, 3), (59, 3), (67, 4), (83, 4),
                                              (99, 5), (131, 7), (259, 8), (515, 9), (1027, 10), (2051, 11), (4099, 12), (8195, 13),
                                              (16387, 14), (32771, 15), (65539, 16)]
# §3.1.1.3.2.2 predefined distributions
LL_PRE = ([4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6)
ML_PRE = ([1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7, 6)
OF_PRE = ([1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5, 5)
MAX_AL = {"ll": 9, "of": 8, "ml": 9}


def _highbit(x):
    return x.bit_length() - 1


def code_of(table, value):
    """largest code whose baseline is <= value (the extra bits hold the rest)"""
    c = max(i for i, (b, _) in enumerate(table) if b <= value)
    b, nb = table[c]
    assert value - b < (1 << nb), ("value out of range", value)
    return c, value - b, nb


# ---------------------------------------------------------------- XXH64 (§3.1.1 Content_Checksum: low 32 bits, seed 0)
_P1, _P2, _P3, _P4, _P5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & MASK64


def _round(acc, v):
    return (_rotl((acc + v * _P2) & MASK64, 31) * _P1) & MASK64


def xxh64(data, seed=0):
    n, p = len(data), 0
    if n >= 32:
        v = [(seed + _P1 + _P2) & MASK64, (seed + _P2) & MASK64, seed, (seed - _P1) & MASK64]
        while p + 32 <= n:
            for i in range(4):
                v[i] = _round(v[i], struct.unpack_from("<Q", data, p + 8 * i)[0])
            p += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & MASK64
        for x in v:
            h = ((h ^ _round(0, x)) * _P1 + _P4) & MASK64
    else:
        h = (seed + _P5) & MASK64
    h = (h + n) & MASK64
    while p + 8 <= n:
        h = ((_rotl(h ^ _round(0, struct.unpack_from("<Q", data, p)[0]), 27)) * _P1 + _P4) & MASK64
        p += 8
    if p + 4 <= n:
        h = (_rotl(h ^ (struct.unpack_from("<I", data, p)[0] * _P1 & MASK64), 23) * _P2 + _P3) & MASK64
        p += 4
    while p < n:
        h = (_rotl(h ^ (data[p] * _P5 & MASK64), 11) * _P1) & MASK64
        p += 1
    h = ((h ^ (h >> 33)) * _P2) & MASK64
    h = ((h ^ (h >> 29)) * _P3) & MASK64
    return h ^ (h >> 32)


# ---------------------------------------------------------------- bit streams
class BackwardBits:
    """§4.1 / §4.2.2: bits are appended LSB-first; the decoder starts at the last byte's highest set bit (the marker) and reads towards
    the start, so the value appended last is read first"""
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def add(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0 and value == 0
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF); self.acc >>= 8; self.n -= 8

    def finish(self):
        self.add(1, 1)                                   # the marker bit; the rest of its byte stays 0
        if self.n:
            self.out.append(self.acc & 0xFF)
        return bytes(self.out)


# ---------------------------------------------------------------- FSE (§4.1.1)
class FSE:
    """decoding table of a distribution (normalised counts, -1 = 'less than 1') at accuracy log `al`; `rle` makes the one-cell table of
    RLE mode (state 0, no bits)"""
    def __init__(self, norm=None, al=0, rle=None):
        if rle is not None:
            self.al, self.sym, self.nb, self.base = 0, [rle], [0], [0]
            return
        size = 1 << al
        assert sum(abs(c) for c in norm) == size, ("counts must sum to 2^AL", sum(abs(c) for c in norm), size)
        sym = [None] * size
        high = size - 1
        for s, c in enumerate(norm):                     # 'less than 1' symbols take the last cells, in symbol order
            if c == -1:
                sym[high] = s; high -= 1
        pos, step = 0, (size >> 1) + (size >> 3) + 3
        for s, c in enumerate(norm):
            for _ in range(max(c, 0)):
                sym[pos] = s
                pos = (pos + step) & (size - 1)
                while pos > high:
                    pos = (pos + step) & (size - 1)
        assert pos == 0
        nxt = [1 if c == -1 else c for c in norm]
        self.al, self.sym, self.nb, self.base = al, sym, [0] * size, [0] * size
        for u in range(size):
            s = sym[u]; x = nxt[s]; nxt[s] += 1
            self.nb[u] = al - _highbit(x)
            self.base[u] = (x << self.nb[u]) - size
        self.norm = norm

    def prev_state(self, s, nxt):
        """the state that decodes symbol s and whose transition range covers state nxt"""
        for u, su in enumerate(self.sym):
            if su == s and self.base[u] <= nxt < self.base[u] + (1 << self.nb[u]):
                return u
        raise ValueError(f"symbol {s} not in the table")

    def first_state(self, s):
        return self.sym.index(s)


def ncount(norm, al):
    """§4.1.1 FSE table description (a forward bit stream)"""
    acc, nbits = al - 5, 4
    remaining, threshold, nb = (1 << al) + 1, 1 << al, al + 1
    s, prev0 = 0, False
    while remaining > 1:
        if prev0:
            start = s
            while norm[s] == 0:
                s += 1
            while s >= start + 24:
                start += 24; acc |= 0xFFFF << nbits; nbits += 16
            while s >= start + 3:
                start += 3; acc |= 3 << nbits; nbits += 2
            acc |= (s - start) << nbits; nbits += 2
        c = norm[s]; s += 1
        mx = (2 * threshold - 1) - remaining
        remaining -= abs(c)
        c += 1
        if c >= threshold:
            c += mx
        acc |= c << nbits
        nbits += nb - (c < mx)
        prev0 = c == 1
        while remaining < threshold:
            nb -= 1; threshold >>= 1
    assert remaining == 1 and s == len(norm), "counts must end at the last symbol"
    return acc.to_bytes((nbits + 7) // 8, "little")


def read_ncount(b, pos, max_symbol):
    """the inverse of ncount (FSE_readNCount) on the description at b[pos:]: (normalised counts, accuracy log, position behind the
    description).  Counts are read up to symbol max_symbol; a run of zeros may not lead past the symbol behind it."""
    bits, at = int.from_bytes(b[pos:pos + 256], "little"), 0

    def take(n, keep=False):
        nonlocal at
        v = (bits >> at) & ((1 << n) - 1)
        at += 0 if keep else n
        return v
    al = take(4) + 5
    remaining, threshold, nb = (1 << al) + 1, 1 << al, al + 1
    norm, prev0 = [], False
    while remaining > 1 and len(norm) <= max_symbol:
        if prev0:
            while take(2, keep=True) == 3:               # (the writer's 16 set bits for 24 zeros are eight of these)
                norm += [0] * 3; at += 2
            norm += [0] * take(2)
            assert len(norm) <= max_symbol + 1
        mx = (2 * threshold - 1) - remaining
        if take(nb - 1, keep=True) < mx:
            c = take(nb - 1)
        else:
            c = take(nb)
            if c >= threshold:
                c -= mx
        c -= 1
        remaining -= abs(c)
        norm.append(c); prev0 = c == 0
        while remaining < threshold:
            nb -= 1; threshold >>= 1
    assert remaining == 1
    return norm, al, pos + (at + 7) // 8


def normalize(hist, al, cap=None):
    """some valid normalised counts at accuracy log al for a histogram {symbol: count} (every listed symbol gets >= 1)"""
    size, tot = 1 << al, sum(hist.values())
    top = max(hist)
    norm = [0] * (top + 1)
    for s, c in hist.items():
        norm[s] = max(1, size * c // tot)
    while sum(norm) > size:
        norm[norm.index(max(norm))] -= 1
    while sum(norm) < size:
        i = max(hist, key=lambda s: hist[s] / norm[s])
        norm[i] += 1
    if cap:
        while max(norm) > cap:
            i = norm.index(max(norm)); norm[i] -= 1; norm[min(hist, key=lambda s: norm[s])] += 1
    assert min(norm[s] for s in hist) >= 1 and sum(norm) == size
    return norm


# ---------------------------------------------------------------- Huffman (§4.2.1)
def lengths_to_weights(lengths):
    """{symbol: code length} with Kraft sum exactly 1 -> (weights list up to the last symbol, max bits)"""
    mb = max(lengths.values())
    assert sum(1 << (mb - l) for l in lengths.values()) == 1 << mb, "Kraft sum must be 1"
    w = [0] * (max(lengths) + 1)
    for s, l in lengths.items():
        w[s] = mb + 1 - l
    return w, mb


def flat_lengths(symbols):
    """a complete code over the given symbols: lengths L and L - 1 (no weight dominates)"""
    symbols = sorted(symbols)
    n = len(symbols)
    L = max(1, (n - 1).bit_length())
    short = (1 << L) - n
    return {s: (L - 1 if i < short else L) for i, s in enumerate(symbols)}


def chain_lengths(symbols, maxbits):
    """lengths 1, 2, ..., maxbits - 1, maxbits, maxbits over the first maxbits + 1 of `symbols`: the longest code is maxbits"""
    symbols = sorted(symbols)[:maxbits + 1]
    assert len(symbols) == maxbits + 1
    return {s: min(i + 1, maxbits) for i, s in enumerate(symbols)}


def huf_codes(weights):
    """§4.2.1.3: codes are handed out from the lowest weight up, symbols of equal weight in order -> {symbol: (code, nbits)}"""
    mb = max(weights)  # weight of the most frequent symbol; max bits follows from the total
    total = sum(1 << (w - 1) for w in weights if w)
    maxbits = _highbit(total)
    assert total == 1 << maxbits
    codes, idx = {}, 0
    for w in range(1, mb + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (idx >> (w - 1), maxbits + 1 - w)
                idx += 1 << (w - 1)
    return codes, maxbits


def huf_description(weights, fse=None):
    """§4.2.1.1 tree description: the weights of every symbol but the last (implied).  fse=None: direct (4 bits each, <= 128
    weights); fse=True or (norm, al): FSE-compressed with two interleaved states (§4.2.1.2)"""
    ws = weights[:-1]
    if fse is None:
        assert len(ws) <= 128
        nib = ws + [0] * (len(ws) & 1)
        return bytes([127 + len(ws)]) + bytes((nib[i] << 4) | nib[i + 1] for i in range(0, len(nib), 2))
    if fse is True:
        hist = {}
        for w in ws:
            hist[w] = hist.get(w, 0) + 1
        if len(hist) == 1:
            hist[(next(iter(hist)) + 1) % 12] = 1            # a one-symbol distribution never ends its stream: add a second
        norm, al = normalize(hist, 6, cap=32), 6
    else:
        norm, al = fse
    t = FSE(norm, al)
    n = len(ws)
    st = [None, None]                                     # state 1 decodes the even positions, state 2 the odd ones
    bw = BackwardBits()
    for k in range(n - 1, -1, -1):
        j = k & 1
        if st[j] is None:
            st[j] = t.first_state(ws[k])                  # its last symbol: no transition bits after it
        else:
            u = t.prev_state(ws[k], st[j])
            bw.add(st[j] - t.base[u], t.nb[u]); st[j] = u
    bw.add(st[1], al); bw.add(st[0], al)                  # read first: state 1, then state 2
    body = ncount(norm, al) + bw.finish()
    assert len(body) < 128
    return bytes([len(body)]) + body


def huf_stream(data, codes):
    bw = BackwardBits()
    for b in reversed(data):
        c, nb = codes[b]
        bw.add(c, nb)
    return bw.finish()


# ---------------------------------------------------------------- plan objects
class Lit:
    """literals section (§3.1.1.3.1).  kind: 'raw' | 'rle' | 'huf' | 'treeless'.  data: the literal bytes (rle: data[0] * size).
    sf: size format (default: the smallest that fits).  weights: per-symbol weights (default: flat over the bytes present);
    fse: weights FSE-compressed (True or (norm, al)); streams: 1 or 4; size: regenerated size written (default len(data))"""
    def __init__(self, kind, data=b"", sf=None, streams=1, weights=None, fse=None, size=None, rle_byte=None):
        self.kind, self.data, self.sf, self.streams, self.weights, self.fse = kind, bytes(data), sf, streams, weights, fse
        self.size = len(self.data) if size is None else size
        self.rle_byte = rle_byte


class Seqs:
    """sequences section (§3.1.1.3.2).  seqs: [(literal length, match length, offset value)] (offset value = offset + 3, or a repeat
    code 1..3).  modes: per table ('ll', 'of', 'ml') one of 'pre', ('rle', code), ('fse', norm, al), ('fse', al) (counts from the
    codes used), 'rep'.  nb_bytes: force the 2-byte nbSeq form.  trailing: bytes after the section (nbSeq 0 only)"""
    def __init__(self, seqs=(), ll="pre", of="pre", ml="pre", nb_bytes=None, trailing=b"", nb=None):
        self.seqs, self.modes, self.nb_bytes, self.trailing = list(seqs), {"ll": ll, "of": of, "ml": ml}, nb_bytes, trailing
        self.nb = len(self.seqs) if nb is None else nb


class Block:
    """kind: 'raw' | 'rle' | 'comp' | 'reserved'.  raw: data; rle: data = one byte, n = repeat; comp: lit, seqs.
    size: the Block_Size field written (default: the true one).  last: the Last_Block flag (default: last block of the frame)"""
    def __init__(self, kind, data=b"", n=None, lit=None, seqs=None, size=None, last=None):
        self.kind, self.data, self.n, self.lit, self.seqs, self.size, self.last = kind, bytes(data), n, lit, seqs, size, last


def raw(data, **kw):
    return Block("raw", data, **kw)


def rle(byte, n, **kw):
    return Block("rle", bytes([byte]), n=n, **kw)


def comp(lit, seqs=None, **kw):
    return Block("comp", lit=lit, seqs=seqs if seqs is not None else Seqs(), **kw)


# ---------------------------------------------------------------- writer
class _State:
    def __init__(self):
        self.huf = None                                   # codes of the last Huffman table (treeless literals reuse it)
        self.tables = {"ll": None, "of": None, "ml": None}
        self.rep = [1, 4, 8]
        self.out = bytearray()
        self.ok = True                                    # content is defined


def _lit_header(kind, sf, regen, csize=None):
    t = {"raw": 0, "rle": 1, "huf": 2, "treeless": 3}[kind]
    if kind in ("raw", "rle"):
        if sf == 0:
            assert regen < 32; return bytes([t | (regen << 3)])
        if sf == 1:
            assert regen < 4096; return struct.pack("<H", t | (1 << 2) | (regen << 4))
        assert regen < 1 << 20; return (t | (3 << 2) | (regen << 4)).to_bytes(3, "little")
    bits = {0: 10, 1: 10, 2: 14, 3: 18}[sf]
    assert regen < 1 << bits and csize < 1 << bits, ("sizes do not fit the size format", regen, csize, sf)
    v = t | (sf << 2) | (regen << 4) | (csize << (4 + bits))
    return v.to_bytes({0: 3, 1: 3, 2: 4, 3: 5}[sf], "little")


def _literals(lit, st):
    d = lit.data
    if lit.kind == "raw":
        sf = lit.sf if lit.sf is not None else (0 if lit.size < 32 else 1 if lit.size < 4096 else 3)
        return _lit_header("raw", sf, lit.size) + d, d
    if lit.kind == "rle":
        sf = lit.sf if lit.sf is not None else (0 if lit.size < 32 else 1 if lit.size < 4096 else 3)
        b = lit.rle_byte if lit.rle_byte is not None else d[0]
        return _lit_header("rle", sf, lit.size) + bytes([b]), bytes([b]) * lit.size
    if lit.kind == "huf":
        w = lit.weights or lengths_to_weights(flat_lengths(set(d)))[0]
        codes, _ = huf_codes(w)
        desc = huf_description(w, lit.fse)
        st.huf = codes
    else:
        codes, desc = st.huf, b""
        if codes is None:                                 # no table before: write with a throw-away one (the frame is invalid)
            codes, _ = huf_codes(lengths_to_weights(flat_lengths(set(d) | {0, 1}))[0])
    if lit.streams == 1:
        body = huf_stream(d, codes)
    else:
        seg = (len(d) + 3) // 4
        parts = [huf_stream(d[i * seg:(i + 1) * seg], codes) for i in range(3)] + [huf_stream(d[3 * seg:], codes)]
        body = struct.pack("<HHH", *(len(p) for p in parts[:3])) + b"".join(parts)
    payload = desc + body
    sf = lit.sf
    if sf is None:
        m = max(lit.size, len(payload))
        sf = 0 if lit.streams == 1 else (1 if m < 1024 else 2 if m < 16384 else 3)
    return _lit_header(lit.kind, sf, lit.size, len(payload)) + payload, d


def _seq_table(kind, mode, codes):
    """-> (FSE table or None for repeat, mode number, description bytes)"""
    if mode == "pre":
        return FSE(*{"ll": LL_PRE, "of": OF_PRE, "ml": ML_PRE}[kind]), 0, b""
    if mode == "rep":
        return None, 3, b""
    if mode[0] == "rle":
        return FSE(rle=mode[1]), 1, bytes([mode[1]])
    if len(mode) == 2:                                    # ('fse', al): counts from the codes used
        hist = {}
        for c in codes:
            hist[c] = hist.get(c, 0) + 1
        if len(hist) == 1:
            hist[0 if 0 not in hist else 1] = 1
        norm, al = normalize(hist, mode[1]), mode[1]
    else:
        norm, al = mode[1], mode[2]
    return FSE(norm, al), 2, ncount(norm, al)


def _sequences(sq, st):
    n = sq.nb
    if n == 0:
        out = b"\x00"
    elif sq.nb_bytes == 2 or (n >= 128 and n < 0x7F00):
        out = bytes([(n >> 8) + 0x80, n & 0xFF])
    elif n < 128:
        out = bytes([n])
    else:
        out = b"\xff" + struct.pack("<H", n - 0x7F00)
    if n == 0:
        return out + sq.trailing
    syms = {"ll": [], "of": [], "ml": []}
    extra = []
    for ll, ml, ov in sq.seqs:
        lc, lx, lb = code_of(LL_CODES, ll)
        mc, mx, mb = code_of(ML_CODES, ml)
        oc = _highbit(ov)
        syms["ll"].append(lc); syms["ml"].append(mc); syms["of"].append(oc)
        extra.append(((ov - (1 << oc), oc), (mx, mb), (lx, lb)))
    tabs, hdr, mode_byte = {}, b"", 0
    for kind, shift in (("ll", 6), ("of", 4), ("ml", 2)):
        t, m, desc = _seq_table(kind, sq.modes[kind], syms[kind])
        if t is None:
            t = st.tables[kind] or _seq_table(kind, "pre", ())[0]    # repeat with nothing before: a stand-in (the frame is invalid)
        st.tables[kind] = t
        tabs[kind] = t
        mode_byte |= m << shift
        hdr += desc
    bw = BackwardBits()
    cur = None
    for i in range(len(sq.seqs) - 1, -1, -1):
        if cur is None:
            cur = {k: tabs[k].first_state(syms[k][i]) for k in tabs}
        else:                                             # read after seq i: LL, ML, OF transitions -> written OF, ML, LL
            prev = {k: tabs[k].prev_state(syms[k][i], cur[k]) for k in tabs}
            for k in ("of", "ml", "ll"):
                bw.add(cur[k] - tabs[k].base[prev[k]], tabs[k].nb[prev[k]])
            cur = prev
        (ov, ob), (mx, mb), (lx, lb) = extra[i]           # read: offset, match length, literal length
        bw.add(lx, lb); bw.add(mx, mb); bw.add(ov, ob)
    for k in ("ml", "of", "ll"):                          # initial states, read LL, OF, ML
        bw.add(cur[k], tabs[k].al)
    return out + bytes([mode_byte]) + hdr + bw.finish()


def _execute(st, lits, seqs):
    """§3.1.2.5 sequence execution with §3.1.2.5.1 repeat offsets.  Offset value 3 with literal length 0 when the first repeat offset
    is 1 gives 0, which RFC 8878 calls corrupt; libzstd and the reference both take 1 there (`temp += !temp`), as done here."""
    out, rep, lp = st.out, st.rep, 0
    for ll, ml, ov in seqs:
        if lp + ll > len(lits):
            st.ok = False; return
        out += lits[lp:lp + ll]; lp += ll
        if ov > 3:
            off = ov - 3; rep[:] = [off, rep[0], rep[1]]
        else:
            idx = ov - 1 + (ll == 0)                      # 0: rep[0]; 1, 2: rep[1], rep[2]; 3: rep[0] - 1
            if idx == 0:
                off = rep[0]
            else:
                off = max(rep[0] - 1 if idx == 3 else rep[idx], 1)
                rep[:] = [off, rep[0], rep[2]] if idx == 1 else [off, rep[0], rep[1]]
        if off > len(out):
            st.ok = False; return
        start = len(out) - off
        if off >= ml:
            out += out[start:start + ml]
        else:
            for j in range(ml):
                out.append(out[start + j])
    out += lits[lp:]


def _block(b, st, last):
    if b.kind == "raw":
        payload, size = b.data, len(b.data)
        st.out += b.data
    elif b.kind == "rle":
        payload, size = b.data, b.n
        st.out += b.data * b.n
    elif b.kind == "reserved":
        payload, size = b.data, len(b.data)
        st.ok = False
    else:
        lsec, lits = _literals(b.lit, st)
        payload = lsec + _sequences(b.seqs, st)
        size = len(payload)
        if b.seqs.nb and len(b.seqs.seqs):
            _execute(st, lits, b.seqs.seqs)
        else:
            st.out += lits
    size = size if b.size is None else b.size
    t = {"raw": 0, "rle": 1, "comp": 2, "reserved": 3}[b.kind]
    last = last if b.last is None else b.last
    return (int(last) | (t << 1) | (size << 3)).to_bytes(3, "little") + payload


def frame(blocks, fcs="auto", fcs_bytes=None, single=True, window=None, dict_id=None, dict_bytes=None, checksum=False,
          bad_checksum=False, reserved=False, magic=MAGIC, checksum_value=None):
    """-> (frame bytes, content or None).  fcs: the Frame_Content_Size written ('auto' = the content's size, None = absent);
    fcs_bytes: field size 0 (single-segment only), 1, 2, 4 or 8.  single: Single_Segment flag; window: (exponent, mantissa) when
    not single.  dict_id / dict_bytes: Dictionary_ID and its field size (0, 1, 2, 4).  checksum: Content_Checksum_Flag."""
    st = _State()
    body = b"".join(_block(b, st, i == len(blocks) - 1) for i, b in enumerate(blocks))
    content = bytes(st.out) if st.ok else None
    n = len(st.out)
    fcs_v = n if fcs == "auto" else fcs
    if fcs_v is None:
        fcs_bytes, fflag = 0, 0
    else:
        if fcs_bytes is None:
            fcs_bytes = 1 if single and fcs_v < 256 else 2 if 256 <= fcs_v < 65792 else 4 if fcs_v < 1 << 32 else 8
        fflag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
        assert fcs_bytes != 1 or single, "a 1-byte content size needs the single-segment flag"
    if dict_bytes is None:
        dict_bytes = 0 if dict_id is None else 1 if dict_id < 256 else 2 if dict_id < 65536 else 4
    fhd = (fflag << 6) | (int(single) << 5) | (int(reserved) << 3) | (int(checksum) << 2) | {0: 0, 1: 1, 2: 2, 4: 3}[dict_bytes]
    hdr = struct.pack("<I", magic) + bytes([fhd])
    if not single:
        e, m = window
        hdr += bytes([(e << 3) | m])
    if dict_bytes:
        hdr += (dict_id or 0).to_bytes(dict_bytes, "little")
    if fcs_bytes:
        hdr += (fcs_v - 256 if fcs_bytes == 2 else fcs_v).to_bytes(fcs_bytes, "little")
    tail = b""
    if checksum:
        ck = checksum_value if checksum_value is not None else xxh64(bytes(st.out)) & 0xFFFFFFFF
        tail = struct.pack("<I", ck ^ (0x5A5A5A5A if bad_checksum else 0))
    return hdr + body + tail, content


def skippable(payload, nibble=0, size=None):
    """§3.1.2 skippable frame: magic 0x184D2A50 + nibble, a 4-byte size (default: the payload's), the payload"""
    return struct.pack("<II", 0x184D2A50 + nibble, len(payload) if size is None else size) + bytes(payload)


# ---------------------------------------------------------------- reading a frame's structure back (§3.1.1)
def frame_header(frame):
    """the fields of the header of the frame at frame[0:]: single (segment), dict_desc (the dictionary-ID field's size code), dict_id,
    window (bytes; -1 for a single-segment frame), content_size (None if not stated), checksum (flag), reserved (bit), end (position
    of the first block)"""
    assert frame[:4] == MAGIC.to_bytes(4, "little")
    fhd = frame[4]
    h = SimpleNamespace(single=(fhd >> 5) & 1, dict_desc=fhd & 3, checksum=(fhd >> 2) & 1, reserved=(fhd >> 3) & 1, window=-1)
    pos = 5
    if not h.single:
        base = 1 << (10 + (frame[pos] >> 3)); h.window = base + (base // 8) * (frame[pos] & 7); pos += 1
    did = (0, 1, 2, 4)[h.dict_desc]
    h.dict_id = int.from_bytes(frame[pos:pos + did], "little"); pos += did
    fcs = (h.single, 2, 4, 8)[fhd >> 6]
    h.content_size = int.from_bytes(frame[pos:pos + fcs], "little") + (256 if fcs == 2 else 0) if fcs else None
    h.end = pos + fcs
    return h


def blocks(frame):
    """yields, for every block of the frame at frame[0:]: type (0 raw, 1 RLE, 2 compressed), size (the header's Block_Size), last, pos and
    end (of the block's bytes in the frame).  A compressed block also has lit_type, size_format, regen and csize (its literals' regenerated
    and stored sizes: stored is regen for raw, 1 for RLE literals), lit_header (bytes), huf_pos (where a Huffman description starts, for
    lit_type 2; else None), seq_pos (of the sequences section), nseq, modes (the byte; None where nseq is 0) and tables_pos (behind the
    modes byte: the first table description, or the bit stream).  Nothing beyond what locates these fields is checked."""
    pos = frame_header(frame).end
    last = 0
    while not last:
        h = int.from_bytes(frame[pos:pos + 3], "little"); pos += 3
        last = h & 1
        b = SimpleNamespace(type=(h >> 1) & 3, size=h >> 3, last=last, pos=pos)
        b.end = pos + (1 if b.type == 1 else b.size)
        if b.type == 2:
            b.lit_type, b.size_format = frame[pos] & 3, (frame[pos] >> 2) & 3
            if b.lit_type < 2:                                              # raw, RLE: 5, 12 or 20 bits of size
                b.lit_header = (1, 2, 1, 3)[b.size_format]
                b.regen = int.from_bytes(frame[pos:pos + b.lit_header], "little") >> (3 if b.lit_header == 1 else 4)
                b.csize = b.regen if b.lit_type == 0 else 1
            else:                                                           # compressed, treeless: two sizes of 10, 10, 14 or 18 bits
                b.lit_header, nbits = ((3, 10), (3, 10), (4, 14), (5, 18))[b.size_format]
                v = int.from_bytes(frame[pos:pos + b.lit_header], "little") >> 4
                b.regen, b.csize = v & ((1 << nbits) - 1), v >> nbits
            b.huf_pos = pos + b.lit_header if b.lit_type == 2 else None
            q = b.seq_pos = pos + b.lit_header + b.csize
            b.nseq = frame[q]; q += 1
            if b.nseq == 255:
                b.nseq = int.from_bytes(frame[q:q + 2], "little") + 0x7F00; q += 2
            elif b.nseq >= 128:
                b.nseq = ((b.nseq - 128) << 8) + frame[q]; q += 1
            b.modes = frame[q] if b.nseq else None
            b.tables_pos = q + (1 if b.nseq else 0)
        yield b
        pos = b.end


def entropy_shapes(frame):
    """per block of the frame, how its entropy tables are described: None for a raw or RLE block, else a namespace with nseq, tables
    (None without sequences, else for LL, OF, ML in turn "pre", "rle", "repeat" or the accuracy log of an FSE description) and weights
    (None unless the literals carry a Huffman description, else "4bit" or the accuracy log of its FSE form).  3.1.1.3.2.1, 4.2.1"""
    out = []
    for b in blocks(frame):
        if b.type != 2:
            out.append(None); continue
        s = SimpleNamespace(nseq=b.nseq, tables=None, weights=None)
        if b.lit_type == 2:
            s.weights = "4bit" if frame[b.huf_pos] >= 128 else (frame[b.huf_pos + 1] & 15) + 5
        if b.nseq:
            p, s.tables = b.tables_pos, []
            for shift, max_symbol in ((6, 35), (4, 31), (2, 52)):
                mode = (b.modes >> shift) & 3
                if mode == 2:
                    _, al, p = read_ncount(frame, p, max_symbol)
                    s.tables.append(al)
                else:
                    s.tables.append(("pre", "rle", None, "repeat")[mode]); p += mode == 1
        out.append(s)
    return out


def _read_backward(stream):
    """a reader of the backward bit stream `stream` (§4.1): take(n) gives the next n bits, left() the bits still unread (negative once
    the reader has run past the stream's start, where it reads zeros)"""
    assert stream and stream[-1], "a backward bit stream ends in its marker bit"
    v = int.from_bytes(stream, "little")
    at = [v.bit_length() - 1]

    def take(n):
        at[0] -= n
        return (v >> at[0]) & ((1 << n) - 1) if at[0] >= 0 else (v << -at[0]) & ((1 << n) - 1)
    return take, lambda: at[0]


def huf_weights(frame, pos):
    """the Huffman weights of the tree description at frame[pos:] (§4.2.1.1), the implied last one included, and the position behind the
    description.  Direct form: 4 bits a weight.  FSE form (§4.2.1.2): two interleaved states, read until the stream is exhausted."""
    h = frame[pos]
    if h >= 128:
        n = h - 127
        body = frame[pos + 1:pos + 1 + (n + 1) // 2]
        w = [(body[i >> 1] >> (0 if i & 1 else 4)) & 15 for i in range(n)]
        end = pos + 1 + (n + 1) // 2
    else:
        end = pos + 1 + h
        norm, al, p = read_ncount(frame, pos + 1, 12)
        t = FSE(norm, al)
        take, left = _read_backward(frame[p:end])
        st, w, j = [take(al), take(al)], [], 0
        while True:
            assert len(w) < 255
            u = st[j]
            w.append(t.sym[u]); st[j] = t.base[u] + take(t.nb[u])
            if left() < 0:                                # the stream ran out inside this update: the other state's symbol is the last
                w.append(t.sym[st[j ^ 1]]); break
            j ^= 1
    total = sum(1 << (x - 1) for x in w if x)
    rest = (1 << total.bit_length()) - total
    assert total and rest & (rest - 1) == 0, "the weights must leave a power of two for the last symbol"
    return w + [_highbit(rest) + 1], end


def section_shapes(frame):
    """per block of the frame, what blocks() and entropy_shapes() give (the fields of blocks(); tables and weights as entropy_shapes()
    names them) and the decisions behind a compressed block's two sections:
    literals: streams (1 or 4 for Huffman-coded literals, else None); huf_weights (the decoded weights by symbol, the implied last one
    included; None without a description), and from them coded (symbols with a code), max_symbol and max_bits (the longest code);
    sequences: nseq_bytes (the width of Number_of_Sequences) and, where nseq > 0, ll / of / ml: namespaces with mode ("pre", "rle", "fse",
    "repeat"), al and norm (an FSE description's accuracy log and normalised counts, padded with zeros to the table's last code) and
    symbol (RLE mode).  No bit stream is decoded beyond the weights."""
    out = []
    for b, e in zip(blocks(frame), entropy_shapes(frame)):
        if b.type == 2:
            b.tables, b.weights = e.tables, e.weights
            b.streams = (1 if b.size_format == 0 else 4) if b.lit_type >= 2 else None
            b.huf_weights = b.coded = b.max_symbol = b.max_bits = None
            if b.lit_type == 2:
                b.huf_weights, _ = huf_weights(frame, b.huf_pos)
                present = [s for s, w in enumerate(b.huf_weights) if w]
                b.coded, b.max_symbol = len(present), present[-1]
                b.max_bits = _highbit(sum(1 << (w - 1) for w in b.huf_weights if w)) + 1 - min(b.huf_weights[s] for s in present)
            b.nseq_bytes = 1 if frame[b.seq_pos] < 128 else 2 if frame[b.seq_pos] < 255 else 3
            b.ll = b.of = b.ml = None
            p = b.tables_pos
            for name, shift, max_symbol in (("ll", 6, 35), ("of", 4, 31), ("ml", 2, 52)) if b.nseq else ():
                mode = (b.modes >> shift) & 3
                t = SimpleNamespace(mode=("pre", "rle", "fse", "repeat")[mode], al=None, norm=None, symbol=None)
                if mode == 1:
                    t.symbol = frame[p]; p += 1
                elif mode == 2:
                    norm, t.al, p = read_ncount(frame, p, max_symbol)
                    t.norm = norm + [0] * (max_symbol + 1 - len(norm))
                setattr(b, name, t)
        out.append(b)
    return out
