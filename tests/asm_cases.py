"""Windows shared by test_assembly.py (host twin against the restatement) and test_gpu_assembly.py
(device against the host twin): a window is (reads, reference bytes or None, window length), a
read (offset of its start in the window, sequence)."""
import random

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
