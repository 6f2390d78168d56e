"""Pairs and windows shared by test_haplik.py (host twin against the restatement) and
test_gpu_haplik.py and test_gpu_haplik_windows.py (device against the host twin).  A pair is (read,
qualities or None, haplotype), all bytes.  A window case (window_case) is a resident read set, windows
and a hand-built path block; each builder has its preconditions next to it, checked from the twin's
block alone."""
import random

import numpy as np

from guacamole_amd import native

# With the default gap probabilities a run of insertions costs e^-1 a base, so an all-mismatching read
# within the device cap of 512 bases stays near e^-512 and never underflows, whatever its qualities.
# The underflow case therefore makes a gap dear: then both the mismatches (q 60: ~3e-7 a base) and the
# insertions (1e-3 a base) take 512 bases below 2^-1000 * DBL_MIN.
STEEP = dict(close_gap_probability=0.999)

S_EDGES = (1, 2, 63, 64, 65, 128, 129, 448, 512)  # rows a lane, lanes in use, the cap; each against R = 40
R_EDGES = (1, 2, 63, 64, 65, 127, 130)            # chunk reloads and edges; each with S = 70


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def read_of(rng, hap, n, errors=0.05):
    """A read of n bases that follows a stretch of hap, with substitutions."""
    a = rng.randint(0, max(0, len(hap) - n))
    s = bytearray((hap[a:a + n] + rand_seq(rng, n))[:n])
    for i in range(n):
        if rng.random() < errors:
            s[i] = rng.choice(b"ACGT")
    return bytes(s)


def quals(rng, n, lo=0, hi=60):
    return bytes(rng.randint(lo, hi) for _ in range(n))


def shape_pairs(rng):
    """The row-ownership and chunk boundaries, S > R."""
    out = []
    for s in S_EDGES:
        hap = rand_seq(rng, 40)
        out.append((read_of(rng, hap, s), quals(rng, s), hap))
    for r in R_EDGES:
        hap = rand_seq(rng, r)
        out.append((read_of(rng, hap, 70), quals(rng, 70), hap))
    hap = rand_seq(rng, 5)
    out.append((read_of(rng, hap, 200), quals(rng, 200), hap))
    return out


def quality_pairs(rng):
    """All 0 (floored), all 93, mixed."""
    hap = rand_seq(rng, 90)
    read = read_of(rng, hap, 75)
    return [(read, bytes(75), hap), (read, bytes([93]) * 75, hap), (read, quals(rng, 75, 0, 93), hap)]


def underflow_pair(q=60):
    return (b"A" * 512, bytes([q]) * 512, b"C" * 100)


def degenerate_pairs(rng):
    hap = rand_seq(rng, 30)
    return [(b"", b"", hap), (read_of(rng, hap, 20), quals(rng, 20), b""), (b"", b"", b"")]


def random_pairs(rng, n, max_s=200, max_r=300):
    out = []
    for _ in range(n):
        hap = rand_seq(rng, rng.randint(1, max_r), rng.choice([b"ACGT", b"AC", b"ACGTN"]))
        s = rng.randint(1, max_s)
        out.append((read_of(rng, hap, s, rng.choice([0.0, 0.02, 0.3])), quals(rng, s), hap))
    return out


def pack(pairs, with_quals=True):
    return native.haplik_pack([p[0] for p in pairs], [p[1] for p in pairs] if with_quals else None,
                              [p[2] for p in pairs])


def same_pairs(got, want):
    """Two results of haplik_batch / haplik_host, bit for bit (NaN never occurs; -inf compares equal)."""
    assert got["n"] == want["n"]
    for key in ("scaled", "log_likelihood"):
        a, b = got[key].view(np.uint64), want[key].view(np.uint64)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (key, int(bad[0]), got[key][bad[0]], want[key][bad[0]])
    assert np.array_equal(got["flags"], want["flags"])


def host_block(reads, read_quals, window_lists, paths, threads=2, **params):
    """The windows block from the host twins: window w lists the reads window_lists[w] (indexes into
    reads / read_quals, in list order) and has the haplotypes of `paths`; pairs through gq_haplik_host,
    genotypes through gq_haplik_genotypes_host."""
    hap_off, seq_off, bases = paths["hap_off"], paths["hap_seq_off"], paths["bases"]
    pair_reads, pair_quals, pair_haps, lik_off, win_read_off, win_reads = [], [], [], [0], [0], []
    for w, lst in enumerate(window_lists):
        haps = [bases[int(seq_off[h]):int(seq_off[h + 1])] for h in range(int(hap_off[w]), int(hap_off[w + 1]))]
        for r in lst:
            for h in haps:
                pair_reads.append(reads[r])
                pair_quals.append(read_quals[r])
                pair_haps.append(h)
        win_reads += list(lst)
        win_read_off.append(len(win_reads))
        lik_off.append(len(pair_reads))
    res = native.haplik_host(native.haplik_pack(pair_reads, pair_quals, pair_haps), threads=threads, **params)
    gt = native.haplik_genotypes_host(win_read_off, hap_off, lik_off, res["scaled"])
    return dict(win_read_off=np.array(win_read_off, np.int64), win_reads=np.array(win_reads, np.int64),
                lik_off=np.array(lik_off, np.int64), scaled=res["scaled"], log_likelihood=res["log_likelihood"],
                flags=res["flags"], **gt)


def same_block(got, want):
    for key in ("win_read_off", "win_reads", "lik_off", "flags", "gt_off", "best_genotype"):
        assert np.array_equal(got[key], want[key]), (key, got[key], want[key])
    for key in ("scaled", "log_likelihood", "gt_log_likelihood"):
        a, b = np.asarray(got[key]).view(np.uint64), np.asarray(want[key]).view(np.uint64)
        assert np.array_equal(a, b), (key, got[key], want[key])


def rng(seed):
    return random.Random(seed)


# ---- hap_forward_k: every row count a lane, ragged last lanes, byte values, shared bytes ----
LANES = 64
ROW_COUNT_S = tuple(sorted({min(k * LANES + d, 512) for k in range(2, 9) for d in (-1, 0, 1)}))


def row_count_pairs(rng):
    """S on each side of every rows-per-lane step (k * 64 - 1, k * 64, k * 64 + 1 for k = 2 .. 8, within the
    cap of 512), each against R = 40 and against R = 3: 2 to 8 rows a lane."""
    out = []
    for r in (40, 3):
        for s in ROW_COUNT_S:
            hap = rand_seq(rng, r)
            out.append((read_of(rng, hap, s), quals(rng, s), hap))
    assert {-(-len(p[0]) // LANES) for p in out} == set(range(2, 9))
    return out


def ragged_pairs(rng):
    """Every S from 1 to 130 against R = 70 (every ragged last lane, 1 to 64 lanes in use); S = 1 against R
    at the chunk edges and the cap; S = 300 (60 lanes) against R at the edges, the cap, and R = 4 and 68,
    where R + 60 steps end at a chunk reload."""
    out = []
    for s in range(1, 131):
        hap = rand_seq(rng, 70)
        out.append((read_of(rng, hap, s), quals(rng, s), hap))
    for r in (63, 64, 65, 127, 128, 129, 4096):
        hap = rand_seq(rng, r)
        out.append((rand_seq(rng, 1), quals(rng, 1), hap))
    for r in (1, 4, 59, 60, 61, 68, 4096):
        hap = rand_seq(rng, r)
        out.append((read_of(rng, hap, 300), quals(rng, 300), hap))
    return out


def byte_value_pairs(rng):
    """Quality bytes over all of 0 .. 255 and all 255; the byte 0 (the kernel's pad for rows and columns
    outside the pair) as a base on both sides and on one; bases >= 128 on both sides."""
    hap = rand_seq(rng, 300)
    read = read_of(rng, hap, 256)
    every = list(range(256))
    rng.shuffle(every)
    high = bytes(range(128, 256))
    high_hap = rand_seq(rng, 90, high[:6])
    zeros_in = bytearray(rand_seq(rng, 80, b"\0ACGT"))
    zeros_in[0] = zeros_in[-1] = 0
    return [
        (read, bytes(every), hap),
        (read, bytes(range(256)), hap[:70]),
        (read, bytes([255]) * 256, hap),
        (bytes(70), quals(rng, 70), bytes(50)),                  # every cell a match of \0 with \0
        (bytes(70), quals(rng, 70), rand_seq(rng, 50)),          # the same read, no \0 in the haplotype
        (bytes(130), quals(rng, 130), bytes(3)),                 # ragged last lane: its pad rows are \0 too
        (rand_seq(rng, 65), quals(rng, 65), bytes(64)),          # no \0 in the read; pad columns are \0
        (bytes(zeros_in[5:70]), quals(rng, 65), bytes(zeros_in)),
        (read_of(rng, high_hap, 75, 0.1), quals(rng, 75), high_hap),
        (bytes([200]) * 40, bytes(range(128, 168)), bytes([200, 131]) * 30),
    ]


def shared_bytes_pack(rng):
    """haplik_batch's arrays as the window path makes them: pairs that point at the same read bytes and at
    the same haplotype bytes, offsets that do not ascend, and pairs whose bytes overlap in part."""
    reads = [rand_seq(rng, n) for n in (30, 61, 45, 129, 5)]
    haps = [rand_seq(rng, n) for n in (40, 77, 3, 130)]
    seq = np.frombuffer(b"".join(reads), np.uint8)
    qual = np.frombuffer(quals(rng, len(seq)), np.uint8)
    hap = np.frombuffer(b"".join(haps), np.uint8)
    r_at = np.cumsum([0] + [len(x) for x in reads])
    h_at = np.cumsum([0] + [len(x) for x in haps])
    so, sl, ho, hl = [], [], [], []
    for r in (3, 0, 4, 2, 1, 0, 3):          # the window path: every read of a list against every haplotype
        for h in (2, 0, 3, 1):
            so.append(r_at[r]), sl.append(len(reads[r])), ho.append(h_at[h]), hl.append(len(haps[h]))
    # partial overlaps: a read window across two reads, a haplotype window across two haplotypes
    for a, n, b, m in ((10, 60, 20, 70), (25, 70, 35, 50), (0, len(seq), 0, len(hap)), (40, 1, 116, 4)):
        so.append(a), sl.append(n), ho.append(b), hl.append(m)
    return (seq, np.array(so, np.int64), np.array(sl, np.int32), qual, hap, np.array(ho, np.int64),
            np.array(hl, np.int32))


# ---- gq_haplik_windows on hand-built path blocks ----
WK = 10  # the k of the window cases: reads of 30 to 60 bases


def flip(seq, at):
    alt = bytearray(seq)
    alt[at] = b"ACGT"[b"ACGT".index(seq[at]) ^ 1]
    return bytes(alt)


def selected(reads, window, k, min_mapq=0):
    """The front end's rule (asm_test_k) restated: the reads (dicts of contig, start, seq, qual, mapq, all
    aligned as one M run), by index in resident order, that window (contig, start, end) takes."""
    c, a, b = window
    return [i for i, r in enumerate(reads)
            if r["contig"] == c and a < b and r["start"] < b and r["start"] + len(r["seq"]) > a
            and len(r["seq"]) >= k and all(x in b"ACGT" for x in r["seq"]) and r["mapq"] >= min_mapq]


def path_block(haps):
    """The path dict of gq_haplik_windows from a list of haplotypes (bytes) per window."""
    flat = [h for hs in haps for h in hs]
    return dict(hap_off=np.cumsum([0] + [len(hs) for hs in haps]).astype(np.int64),
                hap_seq_off=np.cumsum([0] + [len(h) for h in flat]).astype(np.int64), bases=b"".join(flat))


def window_case(lengths, reads, windows, haps, k=WK):
    """A case: contig lengths, reads sorted by (contig, start) as the resident set keeps them, windows
    (contig, start, end) and a haplotype list per window."""
    assert len(windows) == len(haps)
    reads = sorted(reads, key=lambda r: (r["contig"], r["start"]))
    return dict(lengths=list(lengths), reads=reads, windows=list(windows), haps=[list(h) for h in haps],
                paths=path_block(haps), k=k)


def a_read(rng, contig, start, seq, mapq=30, lo=2, hi=41):
    return dict(contig=contig, start=start, seq=bytes(seq), qual=quals(rng, len(seq), lo, hi), mapq=mapq)


def twin_block(case, min_mapq=0, **params):
    """The expected block of a case: the restated selection, then the host twins."""
    lists = [selected(case["reads"], w, case["k"], min_mapq) for w in case["windows"]]
    return host_block([r["seq"] for r in case["reads"]], [r["qual"] for r in case["reads"]], lists, case["paths"],
                      **params)


def variants(rng, ref, n, lo, hi):
    """n haplotypes of a window's reference: the reference, single-base flips at distinct places in
    [lo, hi), and (from n = 2 on) one of them with a 3-base deletion too, so two lengths."""
    at = rng.sample(range(lo, hi), n)
    out = [ref] + [flip(ref, a) for a in at[1:]]
    if n >= 2:
        d, x = at[0], out[n // 2]
        out[n // 2] = x[:d] + x[d + 3:]
    assert len(set(out)) == n
    return out


ORDER_H = (1, 2, 3, 4, 7, 10)


def order_case(seed=31):
    """Genotype order and pair order: a window of 80 for each H in ORDER_H, 1 to 5 reads each.  Read 0 of
    a window covers every variant place; the reads follow two haplotypes that are not the first, so the
    best genotype is not genotype 0 where H >= 3."""
    r = rng(seed)
    n = len(ORDER_H)
    ref = rand_seq(r, 200 * n)
    reads, windows, haps = [], [], []
    for w, h in enumerate(ORDER_H):
        ws = 200 * w + 20
        windows.append((0, ws, ws + 80))
        hs = variants(r, ref[ws:ws + 80], h, 15, 60)
        haps.append(hs)
        src = [hs[h - 1], hs[h // 2]]
        for i in range(1 + (w + 2) % 5):
            off, ln = (8, 60) if i == 0 else (r.randint(0, 20), r.randint(30, 60))
            seq = bytearray(src[i % 2][off:off + ln])
            if i:
                seq[r.randrange(len(seq))] = r.choice(b"ACGT")
            reads.append(a_read(r, 0, ws + off, seq))
    return window_case([len(ref)], reads, windows, haps)


def order_preconditions(case, block):
    """From the twin's block alone: a transposed n * H + h or a swapped (i, j) cannot give these bits."""
    from guacamole_amd import haplotypes
    hap_off, lik_off, gt_off = case["paths"]["hap_off"], block["lik_off"], block["gt_off"]
    not_first = 0
    for w in range(len(case["windows"])):
        h = int(hap_off[w + 1] - hap_off[w])
        n = int(block["win_read_off"][w + 1] - block["win_read_off"][w])
        assert h == ORDER_H[w] and 1 <= n <= 5
        sc = block["scaled"][lik_off[w]:lik_off[w + 1]].reshape(n, h)
        assert any(len(set(row.tolist())) == h for row in sc), w  # distinct across haplotypes for some read
        gl = block["gt_log_likelihood"][gt_off[w]:gt_off[w + 1]]
        pairs = haplotypes.genotype_pairs(h)
        assert len(gl) == len(pairs) == h * (h + 1) // 2
        if h >= 3:
            assert len(set(gl.tolist())) == len(gl), w
        for g, (i, j) in enumerate(pairs):  # genotype g is the mixed pair of columns i and j, in genotype_pairs' order
            two = np.ascontiguousarray(sc[:, [i, j]])
            alone = native.haplik_genotypes_host([0, n], [0, 2], [0, 2 * n], two.ravel())["gt_log_likelihood"][1]
            assert alone.tobytes() == gl[g].tobytes(), (w, g, i, j)
        if n > 1 and h > 1:
            assert sc.shape[0] != sc.shape[1] or not np.array_equal(sc, sc.T)
        not_first += int(block["best_genotype"][w]) > 0
    assert len({len(x) for hs in case["haps"] if len(hs) >= 2 for x in hs}) >= 2
    assert all(len({len(x) for x in hs}) >= 2 for hs in case["haps"] if len(hs) >= 2)
    assert not_first >= 2
    assert not block["flags"].any()


# the kinds of window: reads and haplotypes, reads alone, haplotypes alone, neither
FULL, READS_ONLY, HAPS_ONLY, NEITHER = "full", "reads", "haps", "neither"
EMPTY_KINDS = (READS_ONLY, HAPS_ONLY, NEITHER)
EMPTY_LAYOUT = ((0, READS_ONLY), (0, HAPS_ONLY), (0, NEITHER), (0, FULL), (0, NEITHER), (0, READS_ONLY),
                (0, HAPS_ONLY), (0, FULL), (0, READS_ONLY), (0, FULL), (1, HAPS_ONLY), (1, FULL), (1, NEITHER),
                (1, FULL), (2, HAPS_ONLY), (1, NEITHER), (1, READS_ONLY))


def empty_case(layout=EMPTY_LAYOUT, seed=32):
    """The empty kinds at the start, as a run of three in the middle, singly between two full windows and
    at the end; contigs 0 and 1 have reads, contig 2 (a window with haplotypes) has none.  Returns the
    case and the kind of every window."""
    r = rng(seed)
    lengths = [100 * len(layout) + 100] * 3
    refs = [rand_seq(r, n) for n in lengths]
    reads, windows, haps = [], [], []
    for w, (c, kind) in enumerate(layout):
        ws = 100 * w + 10
        windows.append((c, ws, ws + 60))
        ref = refs[c][ws:ws + 60]
        haps.append(variants(r, ref, 1 + w % 3, 10, 50) if kind in (FULL, HAPS_ONLY) else [])
        if kind in (FULL, READS_ONLY):
            for i in range(1 + w % 3):
                off = r.randint(0, 20)
                reads.append(a_read(r, c, ws + off, flip(ref, 30)[off:off + r.randint(30, 40)]))
    return window_case(lengths, reads, windows, haps), [kind for _, kind in layout]


def empty_preconditions(case, kinds, block):
    layout_kinds = "".join("F" if k == FULL else "e" for k in kinds)
    if FULL in kinds:
        assert layout_kinds.startswith("eeeF") and layout_kinds.endswith("Feee") and "FeeeF" in layout_kinds
        # each empty kind singly between two full windows
        assert {k for k, a, b in zip(kinds, "F" + layout_kinds, layout_kinds[1:] + "F") if a == b == "F"} >= set(EMPTY_KINDS)
    n = np.diff(block["win_read_off"])
    h = np.diff(case["paths"]["hap_off"])
    for w, kind in enumerate(kinds):
        assert (n[w] > 0, h[w] > 0) == (kind in (FULL, READS_ONLY), kind in (FULL, HAPS_ONLY)), (w, kind)
    contigs = {c for c, _, _ in case["windows"]}
    with_reads = {r["contig"] for r in case["reads"]}
    assert len(with_reads) == 2 and contigs - with_reads
    assert list(np.diff(block["lik_off"])) == list(n * h)
    assert list(np.diff(block["gt_off"])) == [int(b * (b + 1) // 2) if a else 0 for a, b in zip(n, h)]
    assert [int(b) == -1 for b in block["best_genotype"]] == [k != FULL for k in kinds]


WORKGROUP_H = (0, 1, 2, 3, 5)


def workgroup_case(n_windows=301, seed=33):
    """Windows of 40 tiled over one contig, H cycling through 0, 1, 2, 3, 5, reads of 30 every 20 bases:
    every second read straddles a window edge and belongs to both windows."""
    r = rng(seed)
    ref = rand_seq(r, 40 * n_windows)
    windows = [(0, 40 * w, 40 * w + 40) for w in range(n_windows)]
    haps = [variants(r, ref[40 * w:40 * w + 40], WORKGROUP_H[w % 5], 5, 35) if w % 5 else [] for w in range(n_windows)]
    reads = []
    for a in range(0, len(ref) - 30 + 1, 20):
        seq = bytearray(ref[a:a + 30])
        seq[r.randrange(30)] = r.choice(b"ACGT")
        reads.append(a_read(r, 0, a, seq))
    return window_case([len(ref)], reads, windows, haps)


def workgroup_preconditions(case, block):
    counts = dict(windows=len(case["windows"]) + 1, pairs=int(block["lik_off"][-1]), genotypes=int(block["gt_off"][-1]))
    for what, x in counts.items():
        assert x > 256 and x % 256 != 0, (what, x)
    lists = [block["win_reads"][a:b] for a, b in zip(block["win_read_off"][:-1], block["win_read_off"][1:])]
    assert sum(1 for a, b in zip(lists, lists[1:]) if a[-1] == b[0]) >= len(lists) // 2  # straddling reads, in both
    assert set(np.diff(case["paths"]["hap_off"])) == set(WORKGROUP_H)
    return counts


def tie_case(seed=34):
    """Window 0: two identical haplotypes.  Window 1: three, the last two identical, the reads following
    those: the largest genotype is tied at (1, 1), (1, 2), (2, 2) and not at index 0."""
    r = rng(seed)
    ref = rand_seq(r, 400)
    a, b = ref[20:100], ref[220:300]
    alt = flip(flip(b, 30), 50)
    reads = [a_read(r, 0, 20 + o, flip(a, 40)[o:o + 50]) for o in (0, 10, 25)]
    reads += [a_read(r, 0, 220 + o, alt[o:o + 50]) for o in (5, 15, 20, 30)]
    return window_case([len(ref)], reads, [(0, 20, 100), (0, 220, 300)], [[a, a], [b, alt, alt]])


def tie_preconditions(block):
    g = block["gt_log_likelihood"].view(np.uint64)
    assert list(block["gt_off"]) == [0, 3, 9]
    assert g[0] == g[1] == g[2] and block["best_genotype"][0] == 0
    assert g[6] == g[7] == g[8] and block["best_genotype"][1] == 3
    assert all(block["gt_log_likelihood"][x] < block["gt_log_likelihood"][6] for x in (3, 4, 5))
    assert np.isfinite(block["gt_log_likelihood"]).all()


UNDERFLOW_HAPS = (b"C" * 40, b"C" * 50)
DBL_MIN = 2.2250738585072014e-308


def underflow_lengths():
    """Searched with the twin under STEEP: the lengths of a run of A at q 60 whose pairs with both
    UNDERFLOW_HAPS are exactly 0, those whose pairs are non-zero subnormals, and those whose pairs are
    normal: (zero, subnormal, normal), each ascending."""
    ls = list(range(WK, 513))
    pairs = [(b"A" * n, bytes([60]) * n, h) for n in ls for h in UNDERFLOW_HAPS]
    sc = native.haplik_host(pack(pairs), threads=4, **STEEP)["scaled"].reshape(len(ls), len(UNDERFLOW_HAPS))
    zero = [n for n, row in zip(ls, sc) if (row == 0).all()]
    sub = [n for n, row in zip(ls, sc) if ((row > 0) & (row < DBL_MIN)).all()]
    normal = [n for n, row in zip(ls, sc) if (row >= DBL_MIN).all()]
    return zero, sub, normal


def underflow_case():
    """Under STEEP.  Window 0: a read whose pairs are exactly 0 and a normal one: every genotype sum takes
    log(0) and is -inf.  Window 1: a read whose pairs are non-zero subnormals and a normal one: the sums
    take the log of a subnormal and stay finite.  Window 2: the normal read alone."""
    zero, sub, normal = underflow_lengths()
    assert zero and sub and normal, (len(zero), len(sub), len(normal))
    mk = lambda start, n: dict(contig=0, start=start, seq=b"A" * n, qual=bytes([60]) * n, mapq=30)  # noqa: E731
    reads = [mk(0, zero[0]), mk(10, normal[-1]), mk(1000, sub[len(sub) // 2]), mk(1010, normal[-1]), mk(2000, normal[-1])]
    windows = [(0, 0, 600), (0, 1000, 1600), (0, 2000, 2600)]
    return window_case([3000], reads, windows, [list(UNDERFLOW_HAPS)] * 3)


def underflow_preconditions(block):
    sc, fl = block["scaled"], block["flags"]
    assert list(block["lik_off"]) == [0, 4, 8, 10]
    assert (sc[0:2] == 0).all() and ((sc[4:6] > 0) & (sc[4:6] < DBL_MIN)).all()
    assert (sc[2:4] >= DBL_MIN).all() and (sc[6:] >= DBL_MIN).all()
    assert list(fl) == [native.HL_UNDERFLOW] * 2 + [0, 0] + [native.HL_UNDERFLOW] * 2 + [0] * 4
    gl = block["gt_log_likelihood"]
    assert (gl[0:3] == -np.inf).all() and np.isfinite(gl[3:]).all()
    assert (gl[3:6] < gl[6:9]).all() and list(block["best_genotype"][:1]) == [0]


def long_read_case(with_haps=True, seed=36):
    """Two resident reads of 513 bases, one in window 0 (after a short read, so its first pair is pair 2),
    one in the last window; the windows between hold more than 256 pairs.  with_haps False: the two
    windows of the long reads have no haplotypes."""
    r = rng(seed)
    ref = rand_seq(r, 2400)
    windows = [(0, 0, 520)] + [(0, 600 + 50 * w, 640 + 50 * w) for w in range(20)] + [(0, 1700, 2300)]
    reads = [a_read(r, 0, 0, ref[0:40]), a_read(r, 0, 5, ref[5:518])]
    for w in range(20):
        reads += [a_read(r, 0, 600 + 50 * w + o, ref[600 + 50 * w + o:][:32]) for o in (0, 3, 6, 8)]
    reads.append(a_read(r, 0, 1750, ref[1750:2263]))
    haps = [variants(r, ref[a:b], 2 if w in (0, 21) else 4, 5, 35) for w, (_, a, b) in enumerate(windows)]
    if not with_haps:
        haps[0], haps[21] = [], []
    return window_case([len(ref)], reads, windows, haps)


def long_read_preconditions(case):
    """(the smaller over-long pair, the larger's first pair) of long_read_case, from the restated rule."""
    lists = [selected(case["reads"], w, case["k"]) for w in case["windows"]]
    h = np.diff(case["paths"]["hap_off"])
    at, over = 0, []
    for lst, hw in zip(lists, h):
        for i in lst:
            if len(case["reads"][i]["seq"]) > 512 and hw:
                over.append(at)
            at += int(hw)
    return over


def long_hap_case(with_reads=True, seed=37):
    """A haplotype of 4097 bases, the second of three in window 1."""
    r = rng(seed)
    ref = rand_seq(r, 300)
    windows = [(0, 0, 60), (0, 100, 160), (0, 200, 260)]
    reads = [a_read(r, 0, a + o, ref[a + o:a + o + 40]) for a in (0, 100, 200) for o in (0, 10) if with_reads or a != 100]
    haps = [variants(r, ref[0:60], 2, 5, 55), [ref[100:160], rand_seq(r, 4097), flip(ref[100:160], 7)],
            variants(r, ref[200:260], 3, 5, 55)]
    return window_case([len(ref)], reads, windows, haps)


SELECTION_MAPQ = 20


def selection_case(seed=38):
    """One window [100, 160) overlapped by two reads it takes and four it must not: shorter than k, with
    an N, below min_mapq, and starting at the window's end.  Returns (case, index of the low-mapq read)."""
    r = rng(seed)
    ref = rand_seq(r, 300)
    cut = lambda a, n: ref[a:a + n]  # noqa: E731
    with_n = bytearray(cut(115, 35))
    with_n[17] = ord("N")
    reads = [a_read(r, 0, 90, cut(90, 40)), a_read(r, 0, 105, cut(105, WK - 1)), a_read(r, 0, 115, with_n),
             a_read(r, 0, 120, cut(120, 38), mapq=SELECTION_MAPQ - 1), a_read(r, 0, 130, flip(cut(130, 30), 9)),
             a_read(r, 0, 160, cut(160, 40)), a_read(r, 0, 108, cut(108, WK), mapq=SELECTION_MAPQ)]
    case = window_case([len(ref)], reads, [(0, 100, 160)], [variants(r, ref[100:160], 3, 12, 50)])
    low = [i for i, x in enumerate(case["reads"]) if x["mapq"] < SELECTION_MAPQ]
    assert len(low) == 1
    return case, low[0]
