"""A small DEFLATE (RFC 1951) encoder for tests: the caller says which blocks to write and how,
down to the code lengths, the header counts and the code-length alphabet's run codes, so a test
can hand a decoder the valid streams a compressor never emits (and the invalid ones).  Plain
Python, no project imports.

deflate(blocks) -> (payload, info).  A block is one of
  ("stored", data)                    opts: nlen (the complement field, default ~len)
  ("fixed", tokens)
  ("dynamic", tokens, lit_lens, dist_lens)
                                      opts: hlit, hdist, hclen, cl_lens (the 19 code-length code
                                      lengths), cl_seq (the code-length symbols outright), rle
each optionally followed by a dict of opts; every kind takes final (default: the last block)
and, for the coded kinds, eob (default True: end with symbol 256).

A token is a literal byte (int), a match (length, distance) or (length, distance, length symbol
257..285, to choose 284 + 31 over 285 for length 258), or raw: ("sym", literal/length symbol),
("dsym", distance symbol, extra value), ("bits", value, count).

info[k] describes block k as written: kind, bit and end (its first and past-the-last bit
offsets), tokens, and for a
stored block sbit (the bit offset mod 8 right after the 3 header bits, before the padding to
the byte boundary); for a dynamic block lit_lens, dist_lens, hlit, hdist, hclen, cl_lens and
cl_seq (pairs (symbol, repeat count) — the count is 1 for symbols 0..15)."""

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


def len_symbol(length):
    """257 + the index of the last base <= length (258 -> 285)."""
    k = max(i for i in range(29) if LEN_BASE[i] <= length)
    return 257 + k


def dist_symbol(dist):
    return max(i for i in range(30) if DIST_BASE[i] <= dist)


class Bits:
    """LSB-first bit string."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.k = 0

    @property
    def pos(self):
        return 8 * len(self.out) + self.k

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.k
        self.k += n
        while self.k >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.k -= 8

    def code(self, c, n):  # a Huffman code: most significant bit first
        self.put(int(format(c & ((1 << n) - 1), "0%db" % n)[::-1], 2), n)

    def align(self):
        if self.k:
            self.put(0, 8 - self.k)

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """symbol -> code (RFC 1951 3.2.2).  An over-subscribed set still gets codes (they wrap)."""
    count = [0] * 17
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lengths)
    for s, ln in enumerate(lengths):
        if ln:
            codes[s] = nxt[ln]
            nxt[ln] += 1
    return codes


def kraft(lengths):
    """Sum of 2^-len in units of 2^-15: 32768 is a complete code."""
    return sum(1 << (15 - ln) for ln in lengths if ln)


def balanced(symbols, n):
    """Complete code over `symbols` (most frequent first) with lengths floor/ceil(log2): n entries."""
    m = len(symbols)
    out = [0] * n
    if m == 1:
        out[symbols[0]] = 1
        return out
    a = m.bit_length() - 1
    deep = 2 * (m - (1 << a))
    for i, s in enumerate(symbols):
        out[s] = a if i < m - deep else a + 1
    return out


def chained(symbols, n, max_len=15):
    """Complete code over `symbols` (most frequent first) that uses every length from 9 (or
    less) to max_len: the rarest symbols take lengths s+1, s+2, ..., max_len, max_len (together
    one code word of s bits), the others a balanced code with one leaf of s bits left for them."""
    big = len(symbols)
    for s in range(min(8, max_len - 1), 0, -1):
        tail = max_len - s + 1
        m = big - tail + 1
        if m < 2:
            continue
        a = m.bit_length() - 1
        if not (a <= s <= a + (1 if m > (1 << a) else 0)):
            continue
        lens = balanced(list(range(m)), m)  # leaf i of the balanced code; the tail takes the last leaf of s bits
        slot = max(i for i in range(m) if lens[i] == s)
        out = [0] * n
        head = [lens[i] for i in range(m) if i != slot]
        for sym, ln in zip(symbols, sorted(head)):
            out[sym] = ln
        for sym, ln in zip(symbols[m - 1:], list(range(s + 1, max_len + 1)) + [max_len]):
            out[sym] = ln
        assert kraft(out) == 32768
        return out
    raise ValueError("no chained code over %d symbols" % big)


def rle(seq):
    """Code-length symbols for `seq`, longest runs first: 18 (11..138 zeros), 17 (3..10 zeros),
    16 (3..6 copies of the length before)."""
    out, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        run = j - i
        if seq[i] == 0:
            while run >= 11:
                out.append((18, min(run, 138)))
                run -= min(run, 138)
            if run >= 3:
                out.append((17, run))
                run = 0
        else:
            out.append((seq[i], 1))
            run -= 1
            while run >= 3:
                out.append((16, min(run, 6)))
                run -= min(run, 6)
        out += [(seq[i], 1)] * run
        i = j
    return out


def expand(tokens, prefix=b""):
    """The bytes a list of literal and match tokens decodes to (after `prefix`)."""
    out = bytearray(prefix)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            ln, d = t[0], t[1]
            assert 1 <= d <= len(out), t
            for _ in range(ln):
                out.append(out[-d])
    return bytes(out[len(prefix):])


def tokenize(data, dists=(), lens=None, forced=None):
    """Greedy LZ77 over `data`: at each position the longest match whose distance is in `dists`
    and whose length is in `lens` (None: any of 3..258), else a literal.  forced: position ->
    (length, distance) matches that are taken as given (the parse never runs over their start)."""
    forced = forced or {}
    lens = sorted(lens, reverse=True) if lens is not None else None
    out, p, n = [], 0, len(data)
    stops = sorted(forced)
    while p < n:
        if p in forced:
            ln, d = forced[p][0], forced[p][1]
            assert d <= p and p + ln <= n and data[p:p + ln] == data[p - d:p - d + ln], (p, forced[p])
            out.append(tuple(forced[p]))
            p += ln
            continue
        cap = min(258, n - p, min([s - p for s in stops if s > p] or [258]))
        best = (0, 0)
        for d in dists:
            if d > p or cap < 3:
                continue
            a, b = data[p:p + cap], data[p - d:p - d + cap]
            m = cap if a == b else next(i for i, (x, y) in enumerate(zip(a, b)) if x != y)
            if lens is not None:
                m = next((x for x in lens if x <= m), 0)
            if m >= 3 and m > best[0]:
                best = (m, d)
        if best[0]:
            out.append(best)
            p += best[0]
        else:
            out.append(data[p])
            p += 1
    return out


def histogram(tokens):
    """(literal/length symbol -> count incl. 256, distance symbol -> count) of a token list."""
    lit, dist = {256: 1}, {}
    for t in tokens:
        if isinstance(t, int):
            lit[t] = lit.get(t, 0) + 1
        elif t[0] == "sym":
            lit[t[1]] = lit.get(t[1], 0) + 1
        elif t[0] == "dsym":
            dist[t[1]] = dist.get(t[1], 0) + 1
        elif t[0] != "bits":
            s = t[2] if len(t) > 2 else len_symbol(t[0])
            lit[s] = lit.get(s, 0) + 1
            dist[dist_symbol(t[1])] = dist.get(dist_symbol(t[1]), 0) + 1
    return lit, dist


def by_count(h):
    """Symbols of a histogram, most frequent first (ties by symbol)."""
    return sorted(h, key=lambda s: (-h[s], s))


def _tokens(w, tokens, lit_lens, dist_lens, eob):
    lc, dc = canonical(lit_lens), canonical(dist_lens)

    def lit(s):
        assert lit_lens[s], "literal/length symbol %d has no code" % s
        w.code(lc[s], lit_lens[s])

    for t in tokens:
        if isinstance(t, int):
            lit(t)
        elif t[0] == "sym":
            lit(t[1])
        elif t[0] == "dsym":
            assert dist_lens[t[1]]
            w.code(dc[t[1]], dist_lens[t[1]])
            if t[1] < 30:
                w.put(t[2], DIST_EXTRA[t[1]])
        elif t[0] == "bits":
            w.put(t[1], t[2])
        else:
            ln, d = t[0], t[1]
            s = t[2] if len(t) > 2 else len_symbol(ln)
            assert 0 <= ln - LEN_BASE[s - 257] < (1 << LEN_EXTRA[s - 257]), t
            lit(s)
            w.put(ln - LEN_BASE[s - 257], LEN_EXTRA[s - 257])
            ds = dist_symbol(d)
            assert ds < len(dist_lens) and dist_lens[ds], "distance symbol %d has no code" % ds
            w.code(dc[ds], dist_lens[ds])
            w.put(d - DIST_BASE[ds], DIST_EXTRA[ds])
    if eob:
        lit(256)


def _dynamic_header(w, lit_lens, dist_lens, o, rec):
    def last(v, least):
        return max([least] + [i + 1 for i, x in enumerate(v) if x])
    hlit = o.get("hlit", last(lit_lens, 257))
    hdist = o.get("hdist", last(dist_lens, 1))
    seq = (list(lit_lens) + [0] * 288)[:hlit] + (list(dist_lens) + [0] * 32)[:hdist]
    cl_seq = o.get("cl_seq")
    if cl_seq is None:
        cl_seq = rle(seq) if o.get("rle", True) else [(x, 1) for x in seq]
    cl_lens = o.get("cl_lens")
    if cl_lens is None:
        h = {}
        for s, _ in cl_seq:
            h[s] = h.get(s, 0) + 1
        if len(h) == 1:  # the code-length code must be complete: a second symbol
            h[0 if 0 not in h else 8] = 0
        cl_lens = balanced(by_count(h), 19)
    hclen = o.get("hclen", max(4, 1 + max(k for k in range(19) if cl_lens[CL_ORDER[k]])))
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cl_lens[CL_ORDER[k]], 3)
    cc = canonical(cl_lens)
    for s, cnt in cl_seq:
        assert cl_lens[s], "code-length symbol %d has no code" % s
        w.code(cc[s], cl_lens[s])
        if s == 16:
            w.put(cnt - 3, 2)
        elif s == 17:
            w.put(cnt - 3, 3)
        elif s == 18:
            w.put(cnt - 11, 7)
    rec.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=list(cl_lens), cl_seq=list(cl_seq))


def deflate(blocks):
    w, info = Bits(), []
    for k, b in enumerate(blocks):
        o = b[-1] if isinstance(b[-1], dict) else {}
        kind = b[0]
        rec = {"kind": kind, "bit": w.pos}
        w.put(1 if o.get("final", k == len(blocks) - 1) else 0, 1)
        w.put({"stored": 0, "fixed": 1, "dynamic": 2, "reserved": 3}[kind], 2)
        if kind == "stored":
            data = bytes(b[1])
            rec["sbit"] = w.pos % 8
            rec["tokens"] = list(data)
            w.align()
            w.put(len(data), 16)
            w.put(o.get("nlen", len(data) ^ 0xFFFF), 16)
            w.out += data
        elif kind == "fixed":
            rec["tokens"] = list(b[1])
            _tokens(w, b[1], FIXED_LIT, FIXED_DIST + [5, 5], o.get("eob", True))
        elif kind == "dynamic":
            lit_lens, dist_lens = list(b[2]), list(b[3])
            rec.update(tokens=list(b[1]), lit_lens=lit_lens, dist_lens=dist_lens)
            _dynamic_header(w, lit_lens, dist_lens, o, rec)
            _tokens(w, b[1], lit_lens + [0] * (288 - len(lit_lens)), dist_lens + [0] * (32 - len(dist_lens)),
                    o.get("eob", True))
        rec["end"] = w.pos
        info.append(rec)
    return w.bytes(), info


def header_seq(lit_lens, dist_lens):
    """The code-length sequence a dynamic header carries by default (minimal HLIT and HDIST)."""
    def cut(v, least):
        return list(v[:max([least] + [i + 1 for i, x in enumerate(v) if x])])
    return cut(list(lit_lens) + [0] * 257, 257) + cut(list(dist_lens) + [0], 1)


def auto_dynamic(tokens, lit="balanced", dist="balanced", **opts):
    """A dynamic block for `tokens` with codes fitted to the symbols they use: "balanced" or
    "chained" (every length up to 15) per alphabet."""
    hl, hd = histogram(tokens)
    fit = {"balanced": balanced, "chained": chained}
    return ("dynamic", tokens, fit[lit](by_count(hl), 286), fit[dist](by_count(hd), 30) if hd else [0], opts)
