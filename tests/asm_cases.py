"""Windows shared by test_assembly.py (host twin against the restatement) and test_gpu_assembly.py
(device against the host twin): a window is (reads, reference bytes or None, window length), a
read (offset of its start in the window, sequence)."""
import random
import re

import numpy as np

import asm_restatement as R
from guacamole_amd import assemble, native

SUITE_REFERENCE = b"GAGGATCTGCCATGGCCGGGCGAGCTGGAGGAGCGAGGAGGAGGCAGGAGGA"
SUITE_READS = [SUITE_REFERENCE[a:b] for a, b in ((0, 25), (5, 30), (7, 32), (10, 35), (19, 41), (22, 44), (25, 47))] + [
    SUITE_REFERENCE[31:52] + b"TTT"]


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def win(seqs, ref, offsets=None, win_len=None):
    offsets = offsets or [0] * len(seqs)
    return ([(o, bytes(s)) for o, s in zip(offsets, seqs)], ref, len(ref) if win_len is None else win_len)


def tiled(ref, read_len, step, copies=1):
    """Reads of read_len every `step` bases of ref (the last flush with its end), `copies` times."""
    starts = list(range(0, len(ref) - read_len, step)) + [len(ref) - read_len]
    return [(a, ref[a:a + read_len]) for a in starts for _ in range(copies)]


def suite_windows():
    """(k, windows): the reference suite's inputs as windows."""
    s = b"AAATCCCTGGGT"
    return [
        (8, [win([b"TCATCTCAAAAGAGATCGA"], b"TCATCTCAAAAGAGATCGA")]),
        (3, [win([b"TCATCTTAAAAGACATAAA"], b"TCATCTTAAAAGACATAAA")]),
        (4, [win([b"AAATCCCTTTTA"], b"AAATCCCTTTTA"), win([s], s), win([s, b"AAATCCCTGGAT"], s),
             win([s, b"AAATCGCTGGGT"], s), win([s, b"ACATCCCTGGGT"], s)]),
        (15, [win(SUITE_READS, SUITE_REFERENCE, [0, 5, 7, 10, 19, 22, 25, 31])]),
    ]


def edge_windows(k, rng):
    """The edge cases at one k (k >= 2), every window at least 2k + 6 long where
    it has a reference."""
    ref = rand_seq(rng, 3 * k + 20)
    n = len(ref)
    reads = tiled(ref, k + 8, 3, copies=2)
    with_n = bytearray(ref[:k + 8])
    with_n[k // 2] = ord("N")
    lower = ref[2:k + 10].lower()
    mid = n // 2
    alt = bytearray(ref)
    alt[mid] = ord("ACGT"["ACGT".index(chr(ref[mid])) ^ 1])  # a SNV: a bubble of k nodes
    ref_n = bytearray(ref)
    ref_n[1] = ord("N")
    unit = rand_seq(rng, 3, b"ACGT")
    while len(set(unit)) < 2:
        unit = rand_seq(rng, 3, b"ACGT")
    head, tail = rand_seq(rng, k), rand_seq(rng, k)
    cyc = head + unit * (k + 4) + tail  # a tandem repeat longer than k: a cycle between source and sink
    w = [
        win([s for _, s in reads] + [bytes(with_n), lower, ref[:k - 1], ref[:k]], ref,
            [o for o, _ in reads] + [0, 2, 0, 0]),                                         # N, lower case, short, exactly k
        win([ref[:k + 2] + ref[:k + 2]], ref),                                            # a k-mer twice in one read
        win([b"A" * (k + 5)] * 2, b"A" * (2 * k)),                                         # homopolymer: a self-loop
        win([ref[:k]] * 3, ref[:k]),                                                      # a window of exactly k
        win([ref[:k + 3]], ref[:k - 1]),                                                  # SHORT
        win([s for _, s in reads], bytes(ref_n), [o for o, _ in reads]),                  # REF_N: a byte of the source
        win([s for _, s in reads], None, [o for o, _ in reads], win_len=n),               # REF_N: no reference
        win([ref[3:]] * 2, ref, [3, 3]),                                                       # NO_SOURCE
        win([ref[:-3]] * 2, ref),                                                         # NO_SINK
        win([s for _, s in reads] + [s for _, s in tiled(bytes(alt), k + 8, 3)], ref,
            [o for o, _ in reads] + [o for o, _ in tiled(bytes(alt), k + 8, 3)]),          # a bubble
        win([s for _, s in tiled(cyc, k + 6, 1)], cyc, [o for o, _ in tiled(cyc, k + 6, 1)]),  # a cycle
        win([], ref),                                                                     # no reads
    ]
    return w


def random_windows(rng, k, n):
    out = []
    for _ in range(n):
        ref = rand_seq(rng, rng.randint(k, 3 * k + 30), rng.choice([b"ACGT", b"AC", b"ACG"]))
        reads = []
        for _ in range(rng.randint(0, 12)):
            ln = rng.randint(max(1, k - 2), k + 20)
            a = rng.randint(0, max(0, len(ref) - 1))
            s = bytearray(ref[a:a + ln] + rand_seq(rng, ln))[:ln]
            if rng.random() < 0.3:
                s[rng.randrange(len(s))] = rng.choice(b"ACGTNa")
            reads.append((a, bytes(s)))
        out.append((reads, ref, len(ref)))
    return out


def restated(window, k, min_occurrence=1, **caps):
    reads, ref, wl = window
    return R.window([s for _, s in reads], ref, wl, k, min_occurrence, **caps)


def host_graphs(windows, k, min_occurrence=1, threads=1):
    seqs, lists = [], []
    for reads, _, _ in windows:
        lists.append(list(range(len(seqs), len(seqs) + len(reads))))
        seqs += [s for _, s in reads]
    return native.asm_graphs_host(seqs, lists, [ref for _, ref, _ in windows], [wl for _, _, wl in windows],
                                  threads=threads, k=k, min_occurrence=min_occurrence)


def block_windows(g, paths):
    """A graph block and its paths as one restatement-shaped dict per window."""
    a, out = g.a, []
    for w in range(g.n_windows):
        n0, n1 = int(a["node_off"][w]), int(a["node_off"][w + 1])
        h0, h1 = int(paths["hap_off"][w]), int(paths["hap_off"][w + 1])
        u0, u1 = int(paths["unitig_off"][w]), int(paths["unitig_off"][w + 1])
        so, uo = paths["hap_seq_off"], paths["unitig_seq_off"]
        out.append(dict(
            nodes=[assemble.kmer_string(a["key_lo"][i], a["key_hi"][i], g.k) for i in range(n0, n1)],
            count=[int(x) for x in a["count"][n0:n1]], child_mask=[int(x) for x in a["child_mask"][n0:n1]],
            parent_mask=[int(x) for x in a["parent_mask"][n0:n1]], source=int(a["source"][w]), sink=int(a["sink"][w]),
            status=int(a["status"][w]), n_reads=int(a["n_reads"][w]), n_instances=int(a["n_instances"][w]),
            path_status=int(paths["status"][w]), steps=int(paths["steps"][w]),
            haplotypes=[paths["bases"][int(so[h]):int(so[h + 1])].decode() for h in range(h0, h1)],
            support=[int(x) for x in paths["support"][h0:h1]],
            unitigs=[paths["unitig_bases"][int(uo[u]):int(uo[u + 1])].decode() for u in range(u0, u1)]))
    return out


def check_twin(windows, k, min_occurrence=1, threads=1, **caps):
    """The host twin and gq_asm_paths against the restatement, field for field; returns the twin's windows."""
    g = host_graphs(windows, k, min_occurrence, threads)
    got = block_windows(g, g.paths(**caps))
    assert g.n_windows == len(windows) and list(g.a["win_len"]) == [wl for _, _, wl in windows]
    for i, (w, x) in enumerate(zip(windows, got)):
        want = restated(w, k, min_occurrence, **caps)
        for key in want:
            assert x[key] == want[key], (i, key, x[key], want[key])
    return got


def same_graphs(got, want):
    """Two graph blocks: every array equal."""
    assert (got.n_windows, got.n_nodes, got.k, got.min_occurrence) == (want.n_windows, want.n_nodes, want.k,
                                                                       want.min_occurrence)
    for name in native.GRAPH_ARRAYS:
        assert got.a[name].dtype == want.a[name].dtype and np.array_equal(got.a[name], want.a[name]), name


# ---- windows laid out on a contig, as a resident read set ----
def layout(windows, gap=7):
    """The windows one after another on one contig, `gap` loci of N between them: (reference bytes,
    window (start, end) list, reads as (start, sequence) sorted by start)."""
    ref, spans, reads = bytearray(b"N" * gap), [], []
    for rd, r, wl in windows:
        s = len(ref)
        spans.append((s, s + wl))
        reads += [(s + o, q) for o, q in rd]
        ref += (r if r is not None else b"N" * wl) + b"N" * max(gap, max([o + len(q) - wl for o, q in rd] + [0]) + gap)
    return bytes(ref), spans, sorted(reads, key=lambda x: x[0])


def overlapping(reads, span):
    """Indexes of the (start, sequence) reads whose [start, start + len) overlaps span, in order."""
    return [i for i, (s, q) in enumerate(reads) if s < span[1] and s + len(q) > span[0]]


def twin_of_layout(reads, ref, spans, k, min_occurrence=1, no_reference=()):
    """The host twin over laid-out reads: each window lists the reads that overlap it."""
    return native.asm_graphs_host([q for _, q in reads], [overlapping(reads, sp) for sp in spans],
                                  [None if i in no_reference else ref[a:b] for i, (a, b) in enumerate(spans)],
                                  [b - a for a, b in spans], k=k, min_occurrence=min_occurrence)


# ---- the limits cases (test_gpu_assembly_limits.py on the device, test_assembly.py on the CPU) ----
def cover_once(ref, a, b, read_len, k):
    """(start, sequence) reads over ref[a:b] that hold each of its k-mers exactly once: read_len bases
    every read_len - k + 1, the last one cut at b."""
    return [(s, ref[s:min(s + read_len, b)]) for s in range(a, b - k + 1, read_len - k + 1)]


def full_window(rng, distinct, k, read_len=100, step=60):
    """A random window of `distinct` k-mers, every one of them on two or more reads."""
    ref = rand_seq(rng, distinct + k - 1)
    if len(ref) <= read_len:
        return win([ref] * 2, ref)
    reads = tiled(ref, read_len, step, 2)
    return win([s for _, s in reads], ref, [o for o, _ in reads])


def part_window(rng, distinct, survivors, k, read_len=100, step=60):
    """A random window of `distinct` k-mers of which `survivors` stand on two or more reads: doubled
    reads over both ends (so the source and the sink survive), each k-mer between them on one read."""
    ref = rand_seq(rng, distinct + k - 1)
    head = survivors // 2
    z0 = distinct - (survivors - head)  # the doubled k-mers: [0, head) and [z0, distinct)
    reads = tiled(ref[:head + k - 1], read_len, step, 2)
    reads += cover_once(ref, head, z0 + k - 1, read_len, k)
    reads += [(z0 + o, s) for o, s in tiled(ref[z0:], read_len, step, 2)]
    return win([s for _, s in reads], ref, [o for o, _ in reads])


def table_size_windows(k=25, seed=11):
    """The batch around the device table's real size: (windows, distinct k-mers of each, k-mers of each
    that stand twice or more).  The sizes come from asm_limits, not from literals."""
    lim = native.asm_limits()
    threads, slots = lim["threads"], lim["lds_slots_max"]
    rng = random.Random(seed)
    full = [threads - 1, threads, threads + 1, 2 * threads + 1, slots - 1, slots, slots + 1]
    part = [(slots, threads + 1), (3000, threads + 1)]
    small = 40
    windows = [full_window(rng, d, k) for d in full] + [part_window(rng, d, s, k) for d, s in part]
    windows.append(full_window(rng, small, k))
    return windows, full + [d for d, _ in part] + [small], full + [s for _, s in part] + [small]


def shared_word_windows(k, seed=12, copies=64, tail=12, groups=64):
    """Three windows (k > word_bases) whose keys share one word.  The first: reads X_i + C, i = 0..3, the
    X_i of k bases ending in A C G T by i, C a common suffix of word_bases + tail bases; the k-mers that
    begin in X_i and end word_bases or more into C have equal `lo` and different `hi` across i.  The
    second, mirrored: C' + Y_i, equal `hi` and different `lo`.  `copies` of each read; where C holds no
    whole k-mer, so that every count would be `copies`, the first read is there twice as often and a
    threshold of copies + 1 still splits the counts.  The reference of a window is its first read.

    The third packs a table of 4 * groups slots with nothing else: reads of k bases
    P_b + Z[j:j + word_bases], b = 0..3, j = 0..groups - 1, so every key stands in a group of four
    with equal `lo`, and in a table that full a probe chain runs through the slots of its key's own
    group.  (The first window has only min(13, k - word_bases) such groups, and the hash takes both
    words, so at k = 32 and 33 they seldom meet in a slot.)  P_0's reads are there twice as often."""
    word = native.asm_limits()["word_bases"]
    assert k > word
    rng = random.Random(seed + k)
    z = rand_seq(rng, word + groups - 1)
    heads = [b"ACGT"[b:b + 1] + rand_seq(rng, k - word - 1) for b in range(4)]
    packed = [(heads[b] + z[j:j + word], copies * (2 if b == 0 else 1)) for j in range(groups) for b in range(4)]
    out = []
    for mirrored in (False, True):
        common = rand_seq(rng, word + tail)
        own = set()
        while len(own) < 4:
            own.add(rand_seq(rng, k - 1))
        own = sorted(own)
        rng.shuffle(own)
        if mirrored:
            seqs = [common + b"ACGT"[i:i + 1] + x for i, x in enumerate(own)]
        else:
            seqs = [x + b"ACGT"[i:i + 1] + common for i, x in enumerate(own)]
        times = [copies * (2 if i == 0 and k > len(common) else 1) for i in range(4)]
        out.append(win([s for s, t in zip(seqs, times) for _ in range(t)], seqs[0]))
    out.append(win([s for s, t in packed for _ in range(t)], packed[0][0]))
    return out


def shared_word_pairs(g, w, same="key_lo", other="key_hi"):
    """Pairs of window w's nodes in graph block g with equal `same` word and different `other` word."""
    n0, n1 = int(g.a["node_off"][w]), int(g.a["node_off"][w + 1])
    a, b = g.a[same][n0:n1], g.a[other][n0:n1]
    return sum(1 for i in range(n1 - n0) for j in range(i) if a[i] == a[j] and b[i] != b[j])


def cigar_span(cigar):
    """Reference loci a CIGAR string covers."""
    return sum(int(n) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MDN=X")


def window_reads(reads, window, k, min_mapq=0):
    """Indexes of the reads (dicts of contig, start, cigar, seq, mapq) a (contig, start, end) window
    takes: the aligned span [start, start + cigar_span) overlaps it, mapping quality, length >= k and
    every base one of A C G T.  An empty window takes none."""
    c, a, b = window
    return [i for i, r in enumerate(reads)
            if r["contig"] == c and a < b and r["start"] < b and r["start"] + cigar_span(r["cigar"]) > a
            and r["mapq"] >= min_mapq and len(r["seq"]) >= k and R.standard(r["seq"])]


FRONT_END_CONTIGS = ("chrA", "chrB", "chrC", "chrD", "chrE")


def front_end_case(k=25, min_mapq=20, seed=13):
    """A read set on five contigs (A, C and E without reads) and 600 or more windows over it, shuffled:
    dict(lengths, refs (bytes or None a contig), reads (sorted by contig and start), windows,
    long / deleted / clipped (read indexes), far / deleted_only / clipped_only / empty / unit / past
    (windows))."""
    rng = random.Random(seed)
    lengths = [200, 1100, 150, 400, 200]
    refs = [rand_seq(rng, n) for n in lengths]
    refs[2] = None
    ref = refs[1]
    reads = []

    def add(contig, start, cigar, seq, mapq=30, md=None):
        reads.append(dict(contig=contig, start=start, cigar=cigar, seq=bytes(seq), mapq=mapq,
                          md=md if md is not None else str(cigar_span(cigar))))

    def plain(contig, start, n=40, mapq=30):
        add(contig, start, "%dM" % n, refs[contig][start:start + n], mapq)

    def cluster(contig, start, n):
        for _ in range(n):
            plain(contig, start)
            start += rng.choice([0, 1, 1, 2, 3])  # some at equal starts
        return start

    plain(1, 0, 600)
    assert cluster(1, 1, 150) + 40 < 300  # [300, 600) is the long read's alone
    plain(1, 50, k)
    plain(1, 60, k - 1)
    with_n = bytearray(ref[70:110])
    with_n[k // 2] = ord("N")
    add(1, 70, "40M", with_n)
    for s in (80, 81, 90):
        plain(1, s, mapq=min_mapq - 1)
    add(1, 100, "15M5I20M", ref[100:115] + rand_seq(rng, 5) + ref[115:135])
    add(1, 630, "10S30M", rand_seq(rng, 10) + ref[630:660])
    last = cluster(1, 630, 150)
    assert last + 100 < lengths[1]
    add(1, last, "20M10D20M", ref[last:last + 20] + ref[last + 30:last + 50],
        md="20^%s20" % ref[last + 20:last + 30].decode())
    plain(3, 0, 120)
    cluster(3, 2, 60)
    plain(3, 300, k)
    reads.sort(key=lambda r: (r["contig"], r["start"]))  # (stable, as the read set's own order)
    at = lambda cigar: [i for i, r in enumerate(reads) if r["cigar"] == cigar][0]

    case = dict(lengths=lengths, refs=refs, reads=reads, long=at("600M"), deleted=at("20M10D20M"),
                clipped=at("10S30M"), far=(1, 500, 530), deleted_only=(1, last + 41, last + 50),
                clipped_only=(1, 620, 630), empty=(1, 100, 100), unit=(1, 0, 1), past=(1, last + 60, last + 90))
    windows = [(1, a, a + 30) for a in range(0, 960, 2)] + [(3, a, a + 30) for a in range(0, 370, 2)]
    windows += [(c, a, a + 40) for c in (0, 2, 4) for a in (0, 50, 100)]
    windows += [(1, a, a + 30) for a in range(300, 570, 45)]  # the long read's alone
    windows += [case[name] for name in ("far", "deleted_only", "clipped_only", "empty", "unit", "past")]
    windows += [(3, 5, 5), (1, 0, 700), windows[3], windows[3], windows[500], case["far"]]
    rng.shuffle(windows)
    case["windows"] = windows
    return case


def front_end_twin(case, k, min_mapq, min_occurrence=1):
    """The host twin over the front-end case: every window lists window_reads."""
    refs, windows = case["refs"], case["windows"]
    return native.asm_graphs_host([r["seq"] for r in case["reads"]],
                                  [window_reads(case["reads"], w, k, min_mapq) for w in windows],
                                  [None if refs[c] is None or b > len(refs[c]) else refs[c][a:b] for c, a, b in windows],
                                  [b - a for _, a, b in windows], k=k, min_occurrence=min_occurrence)


def front_end_windows(case, k, min_mapq):
    """The front-end case's windows as check_twin takes them."""
    refs, reads = case["refs"], case["reads"]
    return [([(0, reads[i]["seq"]) for i in window_reads(reads, w, k, min_mapq)],
             None if refs[w[0]] is None or w[2] > len(refs[w[0]]) else refs[w[0]][w[1]:w[2]], w[2] - w[1])
            for w in case["windows"]]


# ---- the reference suite's real reads (tests/golden/reference_fixtures/NOTICE.assembly) ----
SAM_FIXTURE = "assemble-reads-set3-chr2-73613071.sam.gz"
SAM_WINDOW = (73613005, 73613151)


def sam_reads(path):
    """(start, cigar, sequence, MD) of the mapped, non-duplicate, QC-passing records, by start."""
    import gzip
    out = []
    with gzip.open(path, "rt") as fh:
        for line in fh:
            if line.startswith("@"):
                continue
            f = line.rstrip("\n").split("\t")
            if int(f[1]) & (4 | 512 | 1024):
                continue
            md = [t[5:] for t in f[11:] if t.startswith("MD:Z:")]
            out.append((int(f[3]) - 1, f[5], f[9].encode(), md[0] if md else None))
    return sorted(out, key=lambda r: r[0])


def md_reference(reads, start, end):
    """MDTagUtils.getReference: the reference bases of [start, end) rebuilt from the reads' CIGARs and
    MD tags (every locus must be covered by a read with an MD tag)."""
    import re
    ref = {}
    for pos, cigar, seq, md in reads:
        if md is None:
            continue
        aligned = bytearray()  # the read's bases over its reference span, deletions as '-'
        at = 0
        for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar):
            n = int(n)
            if op in "M=X":
                aligned += seq[at:at + n]
                at += n
            elif op in "IS":
                at += n
            elif op in "DN":
                aligned += b"-" * n
        i = 0
        for num, dele, sub in re.findall(r"(\d+)|\^([A-Z]+)|([A-Z])", md):
            if num:
                i += int(num)
            elif dele:
                aligned[i:i + len(dele)] = dele.encode()
                i += len(dele)
            else:
                aligned[i] = ord(sub)
                i += 1
        for j, b in enumerate(aligned):
            ref.setdefault(pos + j, b)
    return bytes(ref[p] for p in range(start, end))
