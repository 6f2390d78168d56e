"""The device BAM decoder (gq_bamdev.hip: inflate_one, bgzf_crc, rec_sync / rec_hop / rec_list)
on streams no compressor emits: BAMs whose BGZF blocks are written by tests/deflate_writer.py
with chosen code lengths, header counts, run codes, block sequences, match (length, distance)
pairs and block cuts.  Every valid file must load on the device into the arrays the host
loader packs (test_gpu_bamdev.compare: every SoA array; the device's CRC kernel has then
checked every inflated byte); every invalid one must raise the host loader's class.

The CPU tests (no gpu mark) are the reference and the cases' own check: each payload inflates
under zlib to its chunk (the rejects fail there), each case contains what it is named for
(from the writer's token lists and code lengths), the host loader reads every valid file and
refuses every invalid one, and the record-boundary cases meet their preconditions under the
Python statement of the plausibility rule (record_at below)."""
import functools
import random
import struct
import types
import zlib

import pytest

from guacamole_amd import bamdev
from guacamole_amd.build import build_ingest
from guacamole_amd.reads import InputFilters, ReadLoadError, _load_bam_py, load_reads
from tests import bam_writer as bw
from tests import deflate_writer as dw
from tests.test_gpu_bamdev import _sorted, compare
from tests.test_ingest import CONTIGS, HEADER, _records, same

gpu = pytest.mark.gpu
PRINT = bytes(range(0x21, 0x7F))
MAX_STORED = 65536 - 26 - 5  # the longest stored block a BGZF block (<= 65536 bytes with its 26 of framing) holds


@pytest.fixture(scope="module", autouse=True)
def _built():
    build_ingest()


def _z(chunk, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(chunk) + c.flush()


def _lits(rng, n, alphabet=PRINT):
    return [rng.choice(alphabet) for _ in range(n)]


def _file(parts, extras=None, eof=True, facts=()):
    """parts: (chunk, blocks) in stream order; blocks None: zlib's encoding of the chunk."""
    pairs, infos = [], []
    for chunk, blocks in parts:
        payload, info = (_z(chunk), None) if blocks is None else dw.deflate(blocks)
        pairs.append((payload, bytes(chunk)))
        infos.append(info)
    return types.SimpleNamespace(pairs=pairs, infos=infos, extras=extras, eof=eof, facts=list(facts))


def _write(built, path):
    offsets = []
    raw = bw.bgzf_blocks(built.pairs, built.extras, built.eof, offsets)
    with open(path, "wb") as fh:
        fh.write(raw)
    return offsets, len(raw)


def _bam(rng, regions=(), n_rec=300):
    """(bytes before the regions, the rest of the header, sorted records): the regions are the
    body of one @CO header line, each to be a BGZF block of its own."""
    text = HEADER + "@CO\t" + b"".join(regions).decode("ascii") + "\n"
    hdr = bw.header(text, CONTIGS)
    start = 8 + len(HEADER) + 4
    stop = start + sum(len(r) for r in regions)
    return hdr[:start], hdr[stop:], _sorted(_records(rng, n_rec, CONTIGS))


def _cut(data, size):
    return [(data[i:i + size], None) for i in range(0, len(data), size)]


def _region_file(rng, region_parts, n_rec=120, facts=()):
    head, rest, recs = _bam(rng, [c for c, _ in region_parts], n_rec)
    return _file([(head, None)] + list(region_parts) + _cut(rest + b"".join(recs), 20000), facts=facts)


def _matches(info):
    return [t for blk in info for t in blk.get("tokens", []) if isinstance(t, tuple) and not isinstance(t[0], str)]


# ---- code shapes ----------------------------------------------------------------------------
def _run_code_region(rng):
    """Literals A B C D H S _ u and lengths 3..7 under hand-made code lengths whose header
    takes 18 x 138, 18 x 11, 17 x 3, 17 x 10, 16 x 3, 16 x 6 and a 16 that starts in the
    literal/length lengths and ends in the distance lengths."""
    abc = b"ABCDHS_u"
    toks = list(abc) + _lits(rng, 80, abc)
    for m in [(3, 1), (4, 2), (5, 3), (6, 4), (7, 5), (3, 7), (4, 9), (7, 12), (5, 6), (6, 8)]:
        toks += [m] + _lits(rng, 5, abc)
    lit = [0] * 262
    for s in (65, 66, 67, 68):
        lit[s] = 3
    for s in (72, 83, 95, 117):
        lit[s] = 5
    for s in range(256, 262):
        lit[s] = 4
    return dw.expand(toks), [("dynamic", toks, lit, [4, 4, 4, 4, 2, 2, 2])]


@functools.lru_cache(None)
def build_codes():
    rng = random.Random(101)
    region, region_blocks = _run_code_region(rng)
    head, rest, recs = _bam(rng, [region], 300)
    body = rest + b"".join(recs)
    chunks = [body[i:i + 3000] for i in range(0, 24000, 3000)] + [body[24000:]]
    far = (1, 2, 4, 8, 36, 51, 100, 300, 1000)
    parts = [(head, None), (region, region_blocks)]
    # every literal/length code length 9..15 (and the short ones), balanced distance code
    parts.append((chunks[0], [dw.auto_dynamic(dw.tokenize(chunks[0], far), lit="chained")]))
    # literals only: HDIST = 1 and that one length 0
    parts.append((chunks[1], [dw.auto_dynamic(list(chunks[1]))]))
    # one distance code, of length 1
    parts.append((chunks[2], [dw.auto_dynamic(dw.tokenize(chunks[2], (1,)))]))
    # the header counts at their largest
    parts.append((chunks[3], [dw.auto_dynamic(dw.tokenize(chunks[3], far), hlit=286, hdist=30, hclen=19)]))
    # HLIT = 257 and the smallest HCLEN a valid block can have: 5 (16, 17, 18, 0, 8) — every
    # literal but an absent one and the end code at 8 bits
    absent = next(v for v in range(255, -1, -1) if v not in chunks[4])
    parts.append((chunks[4], [("dynamic", list(chunks[4]), [0 if s == absent else 8 for s in range(257)], [0])]))
    # code-length codes up to 7 bits (under a chained literal/length code)
    blk = dw.auto_dynamic(dw.tokenize(chunks[5], far), lit="chained")
    h = {}
    for s, _ in dw.rle(dw.header_seq(blk[2], blk[3])):
        h[s] = h.get(s, 0) + 1
    blk[4]["cl_lens"] = dw.chained(dw.by_count(h), 19, max_len=7)
    parts.append((chunks[5], [blk]))
    # the same without run codes (every length spelled out)
    parts.append((chunks[6], [dw.auto_dynamic(dw.tokenize(chunks[6], far), lit="chained", rle=False)]))
    parts.append((chunks[7], [dw.auto_dynamic(dw.tokenize(chunks[7], far), dist="balanced")]))
    parts.append((chunks[8], None))
    return _file(parts)


@functools.lru_cache(None)
def build_dist():
    """Every distance symbol, the rarest under codes of 8..15 bits (past the 7-bit table), each
    at its smallest and largest distance; distance 32768; the last match ends the block."""
    rng = random.Random(102)
    toks = _lits(rng, 32768)
    for s in range(30):
        for d in {dw.DIST_BASE[s], dw.DIST_BASE[s] + (1 << dw.DIST_EXTRA[s]) - 1}:
            toks += [(3 + (s + d) % 40, d)] + _lits(rng, 3)
        toks += [(4, dw.DIST_BASE[s])] * (29 - s)  # symbol 29 the rarest
    toks += _lits(rng, 100) + [(258, 32768)]
    region = dw.expand(toks)
    return _region_file(rng, [(region, [dw.auto_dynamic(toks, lit="chained", dist="chained")])])


# ---- match copy -----------------------------------------------------------------------------
COPY_D = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 31, 32, 33, 64]
COPY_GAPS = [0, 1, 7, 8, 31, 32]


def _copy_lens(d):
    if d < 8:
        f = d * -(-8 // d)
        return sorted({3, f - 1, f, f + 1, 2 * f + 1, 258} - {2})
    return [3, 7, 8, 9, 31, 32, 33, 65, 258]


@functools.lru_cache(None)
def build_copy():
    """One block per (distance, gap): d literals, a match of distance d reaching back to byte
    0, matches of every length of _copy_lens(d), and a last match ending `gap` bytes before the
    block's end.  The blocks are adjacent in the file, fixed and dynamic codes alternating.
    Then one block with every length symbol at its largest extra-bits value (and 284 + 31)."""
    rng = random.Random(103)
    parts = []
    for gap in COPY_GAPS:
        for d in COPY_D:
            toks = _lits(rng, d)
            for ln in _copy_lens(d):
                toks += [(ln, d)] + _lits(rng, 1 + (ln + d) % 3)
            toks += _lits(rng, d) + [(_copy_lens(d)[(gap + d) % len(_copy_lens(d))], d)] + _lits(rng, gap)
            blocks = [("fixed", toks)] if (len(parts) & 1) else [dw.auto_dynamic(toks)]
            parts.append((dw.expand(toks), blocks))
    toks = _lits(rng, 40)
    for s in range(29):
        toks += [(dw.LEN_BASE[s] + (1 << dw.LEN_EXTRA[s]) - 1, 1 + 3 * s, 257 + s)] + _lits(rng, 2)
    parts.append((dw.expand(toks), [("fixed", toks)]))
    return _region_file(rng, parts)


# ---- block structure ------------------------------------------------------------------------
def _split3(chunk, order):
    """The chunk as three deflate blocks of the kinds in `order` (matches may reach back into
    the blocks before)."""
    toks = dw.tokenize(chunk, (1, 4, 36, 200))
    k = len(toks) // 3
    groups, at, blocks = [toks[:k], toks[k:2 * k], toks[2 * k:]], 0, []
    for kind, g in zip(order, groups):
        n = sum(1 if isinstance(t, int) else t[0] for t in g)
        if kind == "stored":
            blocks.append(("stored", chunk[at:at + n]))
        elif kind == "fixed":
            blocks.append(("fixed", g))
        else:
            blocks.append(dw.auto_dynamic(g))
        at += n
    assert at == len(chunk)
    return blocks


def _stored_at(want, rest):
    """A chunk whose stored block (holding `rest`) has its 3 header bits end at bit `want` mod 8:
    empty fixed blocks (10 bits each) and a fixed block of 8 literals (74 bits) or of 5 literals
    and a match (3, 5) (63 bits) come before it."""
    for k in range(8):
        for toks in (list(b"abcdeabc"), list(b"abcde") + [(3, 5)]):
            blocks = [("fixed", [])] * k + [("fixed", toks), ("stored", rest)]
            if dw.deflate(blocks)[1][-1]["sbit"] == want:
                return b"abcdeabc" + rest, blocks
    raise AssertionError(want)


@functools.lru_cache(None)
def build_blocks():
    rng = random.Random(104)
    regions = [_stored_at(w, bytes(_lits(rng, 40 + w))) for w in range(8)]
    head, rest, recs = _bam(rng, [c for c, _ in regions], 420)
    body = rest + b"".join(recs)
    assert len(body) > MAX_STORED + 12000
    c = [body[0:3000], body[3000:6000], body[6000:8000], body[8000:10000], body[10000:10000 + MAX_STORED],
         body[10000 + MAX_STORED:]]
    parts = [(head, None)] + regions
    parts.append((c[0], _split3(c[0], ("stored", "fixed", "dynamic"))))
    parts.append((c[1], _split3(c[1], ("dynamic", "fixed", "stored"))))
    t = dw.tokenize(c[2], (1, 4, 36))
    n0 = sum(1 if isinstance(x, int) else x[0] for x in t[:200])
    assert all(isinstance(x, int) or x[1] <= 36 for x in t)
    parts.append((c[2], [("fixed", t[:200]), ("stored", b""), dw.auto_dynamic(t[200:])]))  # a sync flush's empty block
    assert n0 < len(c[2])
    parts.append((c[3], [dw.auto_dynamic(dw.tokenize(c[3], (1, 4, 36)), final=False), ("fixed", [])]))  # empty final block
    parts.append((c[4], [("stored", c[4])]))  # the longest stored block a BGZF block can hold
    parts.append((c[5], None))
    return _file(parts)


# ---- framing --------------------------------------------------------------------------------
ISIZES = [65536, 1, 2, 3, 4, 5, 0, 700]


def _framing(eof, pad_last=0):
    rng = random.Random(105)
    head, rest, recs = _bam(rng, [], 700)
    data = head + rest + b"".join(recs)
    sizes = [600] * 36 + ISIZES
    chunks, at = [], 0
    for s in sizes:
        chunks.append(data[at:at + s])
        at += s
    chunks += [data[i:i + 9000] for i in range(at, len(data), 9000)]
    pairs, extras, off = [], [], 0
    for k, ch in enumerate(chunks):
        payload = _z(ch) if k % 3 or len(ch) > 20000 else dw.deflate([dw.auto_dynamic(dw.tokenize(ch, (1, 4, 36)))])[0]
        if len(ch) == 0:
            payload = dw.deflate([("fixed", [])])[0]
        # subfields around BC; the one before it sized to put payload k at file offset k mod 16
        after = bw.subfield(88, 65 + k % 5, bytes(k % 4)) if k % 2 else b""
        pad = (k - (off + 12 + 4 + 6 + len(after))) % 16
        if k == len(chunks) - 1:
            pad += pad_last
        before = bw.subfield(82, 65, bytes(pad))
        extras.append((before, after))
        pairs.append((payload, ch))
        off += 12 + len(before) + 6 + len(after) + len(payload) + 8
    assert b"".join(c for _, c in pairs) == data
    return types.SimpleNamespace(pairs=pairs, infos=[None] * len(pairs), extras=extras, eof=eof, facts=[])


@functools.lru_cache(None)
def build_framing():
    return _framing(True)


@functools.lru_cache(None)
def build_noeof(pad_last):
    return _framing(False, pad_last)


VALID = {"codes": build_codes, "dist": build_dist, "copy": build_copy, "blocks": build_blocks,
         "framing": build_framing, "noeof0": lambda: build_noeof(0), "noeof5": lambda: build_noeof(5),
         "noeof11": lambda: build_noeof(11)}


# ---- rejects --------------------------------------------------------------------------------
def _lit_block(T, **opts):
    return dw.auto_dynamic(list(T), **opts)


def _rej_over_lit(T):
    b = _lit_block(T)
    b[2][next(s for s in range(256) if not b[2][s])] = 1
    return dw.deflate([b])[0], T


def _rej_over_dist(T):
    b = _lit_block(T)
    return dw.deflate([(b[0], b[1], b[2], [1, 1, 1])])[0], T


def _rej_over_cl(T):
    b = _lit_block(T)
    used = {s for s, _ in dw.rle(dw.header_seq(b[2], b[3]))}
    assert len(used) >= 3
    b[4]["cl_lens"] = [1 if s in used else 0 for s in range(19)]
    return dw.deflate([b])[0], T


def _rej_type3(T):
    return dw.deflate([("reserved",)])[0], T


def _rej_nlen(T):
    return dw.deflate([("stored", T, {"nlen": 0})])[0], T


def _rej_before0(T):
    return dw.deflate([("fixed", [T[0], (3, 2)] + list(T[4:]))])[0], T


def _rej_long_literal(T):
    return dw.deflate([("fixed", list(T) + [65])])[0], T


def _rej_long_match(T):
    return dw.deflate([("fixed", list(T[:-1]) + [(3, 1)])])[0], T


def _rej_long_stored(T):
    return dw.deflate([("stored", T + b"x")])[0], T


def _rej_short(T):
    return dw.deflate([("fixed", list(T[:-1]))])[0], T


def _rej_first16(T):
    b = _lit_block(T)
    seq = [(16, 3)] + dw.rle(dw.header_seq(b[2], b[3]))
    b[4].update(cl_seq=seq, cl_lens=dw.balanced(sorted({s for s, _ in seq}), 19))
    return dw.deflate([b])[0], T


def _rej_run_past(T):
    b = _lit_block(T)
    seq = dw.rle(dw.header_seq(b[2], b[3]))
    assert seq[-1] == (0, 1)
    seq[-1] = (18, 138)  # 137 entries past the last
    b[4].update(cl_seq=seq, cl_lens=dw.balanced(sorted({s for s, _ in seq}), 19))
    return dw.deflate([b])[0], T


def _rej_no_eob(T):
    cl = [0] * 19
    cl[18] = cl[0] = 1
    return dw.deflate([("dynamic", [], [0] * 257, [0], {"hclen": 4, "cl_lens": cl, "cl_seq": [(18, 138), (18, 120)],
                                                        "eob": False})])[0], T


def _rej_sym286(T):
    return dw.deflate([("fixed", list(T) + [("sym", 286)])])[0], T


def _rej_dsym30(T):
    return dw.deflate([("fixed", list(T) + [("sym", 257), ("dsym", 30, 0)])])[0], T


def _rej_unowned(T):
    toks = list(T) + [("sym", 257), ("bits", 1, 1)]  # the distance code has the one code word 0
    hl, _ = dw.histogram(toks)
    return dw.deflate([("dynamic", toks, dw.balanced(dw.by_count(hl), 286), [1])])[0], T


def _rej_cut1(T):
    """The payload without its last byte, whose stream bits equal the low bits of the byte that
    follows in the file (the CRC field's first): the decode is bit for bit the whole payload's,
    and only the count of bits used against the block's length tells.  A name byte of the last
    record is varied until the CRC fits."""
    T = bytearray(T)
    assert T[-8:-5] == b"XHH"  # the last record ends with the XH:H string: its digits are varied
    for salt in b"0123456789ABCDEF":
        for salt2 in b"0123456789ABCDEF":
            T[-5] = salt
            T[-4] = salt2
            payload, info = dw.deflate([("fixed", list(T))])
            k = info[-1]["end"] - 8 * (len(payload) - 1)
            if (zlib.crc32(bytes(T)) ^ payload[-1]) & ((1 << k) - 1) == 0:
                return payload[:-1], bytes(T)
    raise AssertionError("no fitting CRC")


def _rej_crc(T):
    return dw.deflate([("fixed", list(T))])[0], T[:-2] + bytes([T[-2] ^ 1]) + T[-1:]


def _rej_incomplete_lit(T):
    hl, _ = dw.histogram(list(T))
    spare = next(s for s in range(256) if s not in hl)
    hl[spare] = 0
    lens = dw.balanced(dw.by_count(hl), 286)
    lens[spare] = 0  # its code word is left without an owner and is never used
    return dw.deflate([("dynamic", list(T), lens, [0])])[0], T


def _rej_incomplete_dist(T):
    toks = dw.tokenize(T, (2, 1))
    hl, hd = dw.histogram(toks)
    assert hd and set(hd) <= {0, 1}
    return dw.deflate([("dynamic", toks, dw.balanced(dw.by_count(hl), 286), [2, 2])])[0], T


# name -> (builder, the check in inflate_one that stops the stream)
REJECTS = {
    "over_subscribed_literal": (_rej_over_lit, "huff_build (literal/length) returns false: left < 0"),
    "over_subscribed_distance": (_rej_over_dist, "huff_build (distance) returns false: left < 0"),
    "over_subscribed_code_length": (_rej_over_cl, "huff_build (code-length code) returns false: left < 0"),
    "block_type_3": (_rej_type3, "type == 3"),
    "len_nlen_mismatch": (_rej_nlen, "(ln ^ 0xFFFF) != nln"),
    "match_before_byte_0": (_rej_before0, "dist > op"),
    "output_longer_literal": (_rej_long_literal, "op >= osz"),
    "output_longer_match": (_rej_long_match, "op + len > osz"),
    "output_longer_stored": (_rej_long_stored, "op + ln > osz"),
    "output_shorter": (_rej_short, "op == osz fails at the end: E_SIZE"),
    "run_code_16_first": (_rej_first16, "i == 0"),
    "run_past_hlit_hdist": (_rej_run_past, "i + rep > hlit + hdist"),
    "no_end_of_block_code": (_rej_no_eob, "lens[256] == 0 (HLIT 257, HCLEN 4: only zero lengths can be sent)"),
    "fixed_symbol_286": (_rej_sym286, "sym >= 29"),
    "fixed_distance_symbol_30": (_rej_dsym30, "huff_long returning -1, seen as dsym < 0: the fixed distance code is "
                                              "built over 30 symbols, so no code decodes to 30 and dsym >= 30 is "
                                              "never reached"),
    "unowned_code_word": (_rej_unowned, "huff_long returning -1 (dsym < 0)"),
    "payload_cut_short": (_rej_cut1, "used_bits() > in_bits after the last block"),
    "wrong_crc": (_rej_crc, "bgzf_crc: E_CRC"),
    "incomplete_literal_code": (_rej_incomplete_lit, "huff_build (literal/length) returns false: left > 0"),
    "incomplete_distance_code": (_rej_incomplete_dist, "huff_build (distance) returns false: left > 0, two codes"),
}
# libdeflate, the host loader's inflate where the system has it, lets a run code overrun the
# HLIT + HDIST lengths (zlib, the loader's other backend, does not): no host-loader assertion
HOST_LENIENT = {"run_past_hlit_hdist"}
FOOTER_REJECTS = {"output_longer_literal", "output_longer_match", "output_longer_stored", "output_shorter", "wrong_crc"}


@functools.lru_cache(None)
def build_reject(name):
    rng = random.Random(106)
    head, rest, recs = _bam(rng, [], 60)
    data = head + rest + b"".join(recs)
    cut = len(data) - 400
    payload, chunk = REJECTS[name][0](data[cut:])
    assert len(chunk) == 400
    return _file([(data[:len(head) + len(rest)], None), (data[len(head) + len(rest):cut], None)]), payload, chunk


def _write_reject(name, path):
    ok, payload, chunk = build_reject(name)
    with open(path, "wb") as fh:
        fh.write(bw.bgzf_blocks(ok.pairs + [(payload, chunk)]))


# ---- CPU: the reference and the cases' own check --------------------------------------------
@pytest.mark.parametrize("name", sorted(VALID))
def test_valid_payloads_inflate_under_zlib_and_the_host_loader_reads_the_file(tmp_path, name):
    built = VALID[name]()
    for payload, chunk in built.pairs:
        assert zlib.decompress(payload, -15) == chunk
    p = str(tmp_path / "v.bam")
    _write(built, p)
    rs = load_reads(p, InputFilters())
    assert rs.n > 30
    same(rs, _load_bam_py(p, InputFilters()))


@pytest.mark.parametrize("name", sorted(REJECTS))
def test_reject_payloads_fail_under_zlib_and_the_host_loader(tmp_path, name):
    _, payload, chunk = build_reject(name)
    if name in FOOTER_REJECTS:  # a well-formed stream that is not the footer's: other length or other CRC
        got = zlib.decompress(payload, -15)
        assert len(got) != len(chunk) or zlib.crc32(got) != zlib.crc32(chunk)
    else:
        with pytest.raises(zlib.error):
            zlib.decompress(payload, -15)
    if name == "payload_cut_short":  # with the byte that follows in the file the stream is whole
        assert zlib.decompress(payload + bytes([zlib.crc32(chunk) & 255]), -15) == chunk
    if name in HOST_LENIENT:
        return
    p = str(tmp_path / "r.bam")
    _write_reject(name, p)
    with pytest.raises(ReadLoadError):
        load_reads(p, InputFilters())


def _dyn(info):
    return [b for blk in info if blk for b in blk if b["kind"] == "dynamic"]


def _used_lens(b):
    hl, hd = dw.histogram(b["tokens"])
    return {b["lit_lens"][s] for s in hl}, {b["dist_lens"][s] for s in hd}


def test_code_shape_cases_contain_what_they_are_named_for():
    inf = build_codes().infos
    run, chain, lits, one, big, small, cl7, plain = [inf[k][0] for k in range(1, 9)]
    seq, at, cross = run["cl_seq"], 0, False
    for s, n in seq:
        cross |= s == 16 and at < run["hlit"] < at + n
        at += n
    assert cross and at == run["hlit"] + run["hdist"]
    assert {(18, 138), (18, 11), (17, 3), (17, 10), (16, 3), (16, 6)} <= set(seq)
    assert set(range(9, 16)) <= _used_lens(chain)[0] and max(chain["lit_lens"]) == 15
    assert lits["hdist"] == 1 and lits["dist_lens"] == [0] and not _matches([lits])
    assert [x for x in one["dist_lens"] if x] == [1] and len(_matches([one])) > 20
    assert (big["hlit"], big["hdist"], big["hclen"]) == (286, 30, 19)
    assert (small["hlit"], small["hclen"]) == (257, 5)
    assert max(cl7["cl_lens"][s] for s, _ in cl7["cl_seq"]) == 7 and dw.kraft(cl7["cl_lens"]) == 1 << 15
    assert all(s < 16 for s, _ in plain["cl_seq"]) and max(plain["lit_lens"]) == 15
    for b in _dyn(inf):  # every code here is complete, or the one distance code of length 1, or no distance code
        assert dw.kraft(b["lit_lens"]) == 1 << 15
        assert dw.kraft(b["dist_lens"]) == 1 << 15 or [x for x in b["dist_lens"] if x] in ([1], [])
    d = build_dist().infos[1][0]
    assert set(range(8, 16)) <= _used_lens(d)[1] and len(dw.histogram(d["tokens"])[1]) == 30
    ms = _matches([d])
    assert {m[1] for m in ms} >= {1, 32768, 24577} and ms[-1] == d["tokens"][-1] == (258, 32768)


def test_match_copy_cases_contain_what_they_are_named_for():
    built = build_copy()
    k, kinds = 1, set()
    for gap in COPY_GAPS:
        for d in COPY_D:
            toks = built.infos[k][0]["tokens"]
            chunk = built.pairs[k][1]
            kinds.add((built.infos[k][0]["kind"], d < 8, d >= 32))
            ms = [t for t in toks if isinstance(t, tuple)]
            assert {m[1] for m in ms} == {d} and {m[0] for m in ms} >= set(_copy_lens(d))
            assert toks[:d + 1] == list(chunk[:d]) + [ms[0]]  # the first match reaches back to byte 0
            tail = toks[len(toks) - gap:]
            assert all(isinstance(t, int) for t in tail) and isinstance(toks[len(toks) - gap - 1], tuple)
            assert dw.expand(toks) == chunk and len(chunk) <= 65536
            k += 1
    assert len(kinds) == 6  # both codes for each of d < 8, 8 <= d < 32, d >= 32
    for d in range(1, 8):
        f = d * -(-8 // d)
        assert {3, f - 1, f, f + 1, 258} - {2} <= set(_copy_lens(d))
    last = [t for t in built.infos[k][0]["tokens"] if isinstance(t, tuple)]
    assert [t[2] for t in last] == list(range(257, 286))
    assert all(t[0] == dw.LEN_BASE[t[2] - 257] + (1 << dw.LEN_EXTRA[t[2] - 257]) - 1 for t in last)
    assert last[27][0] == 258 and last[28][0] == 258


def test_block_structure_and_framing_cases_contain_what_they_are_named_for(tmp_path):
    built = build_blocks()
    assert [built.infos[k][-1]["sbit"] for k in range(1, 9)] == list(range(8))
    kinds = [[b["kind"] for b in i] for i in built.infos[9:14]]
    assert kinds[0] == ["stored", "fixed", "dynamic"] and kinds[1] == ["dynamic", "fixed", "stored"]
    assert kinds[2] == ["fixed", "stored", "dynamic"] and built.infos[11][1]["tokens"] == []
    assert kinds[3] == ["dynamic", "fixed"] and built.infos[12][1]["tokens"] == []
    assert kinds[4] == ["stored"] and len(built.pairs[13][1]) == MAX_STORED
    assert 18 + 5 + MAX_STORED + 8 == 65536
    fr = build_framing()
    offsets, _ = _write(fr, str(tmp_path / "f.bam"))
    assert {o % 16 for o in offsets} == set(range(16)) and [o % 16 for o in offsets[:32]] == list(range(16)) * 2
    sizes = [len(c) for _, c in fr.pairs]
    assert sizes[36:36 + len(ISIZES)] == ISIZES
    assert any(b and a for b, a in fr.extras) and all(len(b) >= 4 for b, _ in fr.extras)
    ends = set()
    for pad in (0, 5, 11):
        b = build_noeof(pad)
        _, n = _write(b, str(tmp_path / "n.bam"))
        assert not b.eof and len(b.pairs[-1][1]) > 0
        ends.add(n % 16)
    assert len(ends) == 3


# ---- GPU: the inflate -----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", sorted(VALID))
def test_device_inflates_hand_built_streams(gpu_ctx, tmp_path, name):
    """codes: code lengths 9..15, one distance code, none, the header counts' extremes, 7-bit
    code-length codes, the run codes; dist: distance codes of 8..15 bits, distance 32768; copy:
    the match copy's paths and `room` tails in adjacent blocks; blocks: deflate block sequences,
    stored blocks at each bit offset, empty ones, the longest; framing: payloads at every file
    offset mod 16, ISIZE 65536 / 1..5 / 0, subfields around BC; noeof*: no EOF block."""
    p = str(tmp_path / "v.bam")
    _write(VALID[name](), p)
    d = compare(gpu_ctx, p, InputFilters())
    assert d.n > 30


@gpu
@pytest.mark.parametrize("name", sorted(REJECTS))
def test_device_rejects_what_zlib_rejects(gpu_ctx, tmp_path, name):
    """Each stream and the check in inflate_one (or after it) that stops it: REJECTS.  Every
    write of the decode is behind op + ln > osz, op >= osz or dist > op || op + len > osz, and
    every loop either emits a byte, ends a block or fails, so a rejected stream writes nothing
    outside its block and ends within osz symbols; a stream that runs past its payload reads the
    file's next bytes and then zeros (zero fill past pend), which end it as a fixed end-of-block
    code, a stored LEN/NLEN mismatch or a code-length code without codes."""
    p = str(tmp_path / "r.bam")
    _write_reject(name, p)
    with pytest.raises(ReadLoadError):
        bamdev.load_reads_device(gpu_ctx, p, InputFilters())


# ---- record boundaries ----------------------------------------------------------------------
def record_at(d, n, o, n_ref):
    """gq_bamdev.hip / gq_ingest.cpp record_at: a plausible alignment record at o."""
    if o + 40 > n:
        return False
    bs, ref_id, pos, l_name = struct.unpack_from("<iiiB", d, o)
    n_cig, = struct.unpack_from("<H", d, o + 16)
    l_seq, next_ref = struct.unpack_from("<ii", d, o + 20)
    if bs < 32 or o + 4 + bs > n:
        return False
    if ref_id < -1 or ref_id >= n_ref or next_ref < -1 or next_ref >= n_ref or pos < -1 or l_seq < 0 or l_name < 1:
        return False
    if 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
        return False
    return d[o + 4 + 32 + l_name - 1] == 0


def syncs(d, o, n_ref):
    """rec_sync's test of offset o: it chains into 9 plausible records, or into at least one
    and then the stream's end."""
    q, ok, n = o, 0, len(d)
    while ok < 9 and q < n and record_at(d, n, q, n_ref):
        q += 4 + struct.unpack_from("<i", d, q)[0]
        ok += 1
    return ok == 9 or (ok > 0 and q == n)


def walk(d, rec0):
    out, o = [], rec0
    while o < len(d):
        out.append(o)
        o += 4 + struct.unpack_from("<i", d, o)[0]
    assert o == len(d)
    return out


FAKE = struct.pack("<iiiBBHHHiiii", 33, 0, 0, 1, 0, 4680, 0, 0, 0, -1, -1, 0) + b"\0"


def false_sync_stream(merge, n_before=40, n_after=40, seed=107):
    """(data, rec0, array start, fake chain start): a record whose B:C array holds 0xEE filler
    and nine chained minimal records (block_size 33, refID 0, l_name 1, a NUL name).  merge: the
    array ends the record, so the fake chain's tenth hop is the true next record; else 0x01
    bytes follow the chain (a block_size past the stream's end)."""
    assert len(FAKE) == 37
    rng = random.Random(seed)
    recs = _sorted(_records(rng, n_before + n_after, CONTIGS))
    arr = b"\xEE" * 8 + FAKE * 9 + (b"" if merge else b"\x01" * 16)
    ref, pos = struct.unpack_from("<ii", recs[n_before], 4)
    carrier = bw.record(ref, pos, "carrier", "4M", "ACGT", [30] * 4, tags=bw.tag_z("MD", "4") + bw.tag_b("ZF", "C", arr))
    hdr = bw.header(HEADER, CONTIGS)
    before = hdr + b"".join(recs[:n_before])
    data = before + carrier + b"".join(recs[n_before:])
    arr_at = len(before) + len(carrier) - len(arr)
    return data, len(hdr), arr_at, arr_at + 8


def _cuts_file(data, cuts, path, eof=True):
    edges = [0] + sorted(set(cuts)) + [len(data)]
    with open(path, "wb") as fh:
        fh.write(bw.bgzf_blocks([(_z(data[a:b]), data[a:b]) for a, b in zip(edges, edges[1:])], eof=eof))
    return edges


def false_sync_file(merge, path):
    data, rec0, arr_at, fake_at = false_sync_stream(merge)
    _cuts_file(data, [rec0 + 700, arr_at + 3, arr_at + 3 + 5000], path)
    return data, rec0, arr_at + 3, fake_at


@pytest.mark.parametrize("merge", [False, True])
def test_false_sync_precondition(tmp_path, merge):
    data, rec0, blk_at, fake_at = false_sync_file(merge, str(tmp_path / "f.bam"))
    true = walk(data, rec0)
    first = next(o for o in range(blk_at, blk_at + 5000) if syncs(data, o, len(CONTIGS)))
    assert first == fake_at and fake_at not in true
    nxt = next(o for o in true if o > fake_at)
    assert nxt < blk_at + 5000  # the true next record starts in the same block
    q = fake_at + 9 * 37  # where the nine fakes lead
    assert (q == nxt) if merge else (q not in true and struct.unpack_from("<i", data, q)[0] > len(data))
    same(load_reads(str(tmp_path / "f.bam"), InputFilters()), _load_bam_py(str(tmp_path / "f.bam"), InputFilters()))


@gpu
@pytest.mark.parametrize("merge", [False, True])
def test_device_rehops_a_false_sync(gpu_ctx, tmp_path, merge):
    p = str(tmp_path / "f.bam")
    false_sync_file(merge, p)
    assert compare(gpu_ctx, p, InputFilters()).n > 40


def _tiny(name, pos=19000):
    """A mapped record of 37 + len(name) bytes: no sequence, no CIGAR."""
    return bw.record(2, pos, name, "*", "", [])


def boundary_file(name, path):
    """The record-boundary cases: (data, rec0, block edges)."""
    rng = random.Random(108)
    text, n, tail = HEADER, 200, []
    if name == "long_header":
        text += "@CO\t" + "x" * 3000 + "\n"
    if name.startswith("records_"):
        n = int(name.split("_")[1])
    if name.startswith("tiny_"):
        tail = [_tiny("ab"[:int(name.split("_")[1]) - 37])]
    recs = _sorted(_records(rng, n, CONTIGS))
    if name.startswith("span_"):  # one record over several whole blocks
        ref, pos = struct.unpack_from("<ii", recs[50], 4)
        recs.insert(50, bw.record(ref, pos, "long", "3000M", "ACGT" * 750, [30] * 3000, tags=bw.tag_z("MD", "3000")))
    recs += tail
    hdr = bw.header(text, CONTIGS)
    data = hdr + b"".join(recs)
    starts = walk(data, len(hdr))
    if name.startswith("span_"):
        k = int(name.split("_")[1])
        s = starts[50]
        cuts = [s - 100] + [s + 50 + i * (3000 // (k + 1)) for i in range(k + 1)]
        assert cuts[-1] < starts[51]
    elif name.startswith("split_"):  # block_size's four bytes over a block edge
        cuts = [starts[20 * i] + int(name.split("_")[1]) for i in range(1, 8)]
    elif name == "exact_end":
        cuts = [starts[i] for i in range(10, len(starts), 10)]
    elif name == "long_header":
        cuts = [len(hdr) // 3, 2 * len(hdr) // 3, starts[60] + 7]
    elif name.startswith("records_"):
        cuts = [starts[n // 2] + 5] if n > 1 else []
    else:  # last_one, tiny_*: the last block holds one record
        cuts = [starts[70] + 9, starts[-1]]
    edges = _cuts_file(data, cuts, path)
    return data, len(hdr), edges


BOUNDARY = ["span_3", "span_5", "split_1", "split_2", "split_3", "exact_end", "long_header", "records_1", "records_8",
            "records_9", "records_10", "last_one", "tiny_37", "tiny_38", "tiny_39"]


@pytest.mark.parametrize("name", BOUNDARY)
def test_boundary_case_preconditions(tmp_path, name):
    data, rec0, edges = boundary_file(name, str(tmp_path / "b.bam"))
    starts = walk(data, rec0)
    blocks = list(zip(edges, edges[1:]))
    inside = [(a, b) for a, b in blocks if any(s < a and b < s2 for s, s2 in zip(starts, starts[1:] + [len(data)]))]
    if name.startswith("span_"):
        assert len(inside) == int(name.split("_")[1])
    if name.startswith("split_"):
        assert all(e - int(name.split("_")[1]) in starts for e in edges[1:-1])
    if name == "exact_end":
        assert all(e in starts for e in edges[1:-1])
    if name == "long_header":
        assert edges[2] < rec0 < edges[3]
    if name.startswith("records_"):
        assert len(starts) == int(name.split("_")[1])
    if name in ("last_one",) or name.startswith("tiny_"):
        assert edges[-2] == starts[-1]
    if name.startswith("tiny_"):
        assert len(data) - starts[-1] == int(name.split("_")[1])
        assert not any(syncs(data, o, len(CONTIGS)) for o in range(starts[-1], len(data)))  # only a re-hop finds it
        assert load_reads(str(tmp_path / "b.bam"), InputFilters()).start[-1] == 19000  # the comparison reaches it


@gpu
@pytest.mark.parametrize("name", BOUNDARY)
def test_device_record_boundaries(gpu_ctx, tmp_path, name):
    p = str(tmp_path / "b.bam")
    boundary_file(name, p)
    assert compare(gpu_ctx, p, InputFilters()).n > 0 or name == "records_1"
