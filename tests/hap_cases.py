"""Pairs and windows shared by test_haplik.py (host twin against the restatement) and
test_gpu_haplik.py (device against the host twin).  A pair is (read, qualities or None, haplotype),
all bytes."""
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
