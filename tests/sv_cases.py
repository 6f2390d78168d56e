"""Hand-built inputs for the structural-variant tests: BAM records with their mate fields set,
a reader of a BAM's records for the restatement, and the reference suite's cases retyped as data
(StructuralVariantCallerSuite)."""
import gzip
import struct

import bam_writer as bw
import sv_restatement as R

PAIRED, UNMAPPED, MATE_UNMAPPED, REVERSE, MATE_REVERSE, FIRST, SECOND, DUPLICATE = (0x1, 0x4, 0x8, 0x10, 0x20, 0x40,
                                                                                    0x80, 0x400)
GOOD = PAIRED | FIRST | MATE_REVERSE  # a forward first read whose mate is on the reverse strand


def mate_record(ref_id, pos, name, length, flag, next_ref, next_pos, tlen, cigar=None, tags=b""):
    """bam_writer.record with the three mate fields (bytes 24-36 of the record) overwritten."""
    rec = bytearray(bw.record(ref_id, pos, name, "%dM" % length if cigar is None else cigar, "A" * length,
                              qual=[30] * length, flag=flag, tags=tags))
    struct.pack_into("<iii", rec, 24, next_ref, next_pos, tlen)
    return bytes(rec)


def pair_record(p, name="r", flag_extra=0):
    """The record of a restatement pair (first in pair, mate mapped)."""
    flag = PAIRED | FIRST | flag_extra | (REVERSE if p["strand"] & 1 else 0) | (MATE_REVERSE if p["strand"] & 2 else 0)
    return mate_record(p["contig"], p["start"], name, p["len"], flag, p["mate_contig"], p["mate_start"], p["tlen"])


def bam_records(path):
    """(contig names, [record bytes]) of a BAM file, in file order."""
    data = gzip.decompress(open(path, "rb").read())
    assert data[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", data, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, o)
    o += 4
    names = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, o)
        names.append(data[o + 4:o + 4 + l_name - 1].decode())
        o += 4 + l_name + 4
    recs = []
    while o < len(data):
        bs, = struct.unpack_from("<i", data, o)
        recs.append(data[o:o + 4 + bs])
        o += 4 + bs
    return names, recs


def columns(pairs):
    """Restatement pairs -> the columns of structural.Pairs.from_arrays."""
    return {f: [p[f] for p in pairs] for f in ("contig", "start", "mate_contig", "mate_start", "tlen", "len", "strand")}


# ---- StructuralVariantCallerSuite, retyped -----------------------------------------------------
MEDIAN_STATS = [([2, 4, 1, 1, 2, 6, 9], (2.0, 1.0)), ([0, 1, 2, 2], (1.5, 0.5)), ([1], (1.0, 0.0)), ([], (0.0, 0.0))]

# (pair 1, pair 2 as makePair arguments, N, compatible)
COMPATIBILITY = [
    ((0, 10, 90, 100), (10, 20, 90, 100), 10, False), ((0, 10, 90, 100), (10, 20, 90, 100), 29, True),
    ((0, 10, 90, 100), (10, 20, 90, 100), 30, True), ((0, 10, 90, 100), (10, 20, 90, 100), 40, True),
    ((0, 10, 100, 110), (10, 20, 90, 100), 10, False), ((0, 10, 100, 110), (10, 20, 90, 100), 20, True),
    ((0, 10, 100, 110), (10, 20, 90, 100), 39, True), ((0, 10, 100, 110), (10, 20, 90, 100), 40, True),
    ((0, 10, 100, 110), (10, 20, 90, 100), 50, True),
    ((0, 10, 90, 100), (10, 20, 100, 110), 20, True), ((0, 10, 90, 100), (10, 20, 100, 110), 29, True),
    ((0, 10, 90, 100), (10, 20, 100, 110), 30, True), ((0, 10, 90, 100), (10, 20, 100, 110), 40, True),
    ((0, 10, 90, 100), (95, 105, 195, 205), 1000, False)]


def filtering_pairs():
    """"read filtering": nine pairs of length 12."""
    return [R.pair(9, 97), R.pair(10, 97), R.pair(11, 98), R.pair(12, 101), R.pair(13, 101),
            R.pair(100, 150, reverse=False, mate_reverse=False),  # inverted
            R.pair(1000, 1288), R.pair(1001, 1289), R.pair(2000, 2000000)]


def graph_pairs():
    """"graph construction": with N = 100 the one edge 1-2, weight 0."""
    return [R.pair(100, 288), R.pair(1000, 1288), R.pair(1001, 1289)]


def clique_nodes():
    """"clique detection": a, b, c, d (already in (minPos, file) order)."""
    return [R.pair(1000, 1287), R.pair(1000, 1288), R.pair(1001, 1289), R.pair(1002, 1290)]


A, B, C, D = 0, 1, 2, 3
# (edges (i, j, weight) with i < j, member sets), N = 100
CLIQUE_GRAPHS = [
    ([(A, B, 1)], [{A, B}]),
    ([(A, B, 1), (B, C, 2)], [{A, B}]),
    ([(A, B, 1), (B, C, 2), (A, C, 3)], [{A, B, C}]),
    ([(A, B, 1), (B, C, 2), (C, D, 3), (A, D, 4), (B, D, 5)], [{A, B, D}]),
    ([(A, B, 1), (A, C, 2), (A, D, 3), (C, D, 4)], [{A, B}]),
    ([(A, B, 1), (C, D, 2)], [{A, B}, {C, D}])]


def limited_nodes():
    """"clique detection with alignment limitations": c, a, b in minPos order; N = 400 gives
    {a, b}, span (220, 380), wiggle 260."""
    return [R.make_pair(0, 20, 580, 600), R.make_pair(100, 120, 380, 400), R.make_pair(200, 220, 480, 500)]


LIMITED_EDGES = [(1, 2, 1), (0, 2, 2), (0, 1, 3)]
