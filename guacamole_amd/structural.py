"""structural-variant: large deletions from discordant read pairs (gqpileup.h: gq_sv_*), the
reference's commands/StructuralVariantCaller.scala on the device.

The BAM is inflated in HBM by the device loader (bamdev); ``Pairs`` is the resident table of
its first-in-pair records with a mapped mate (file order), and the stages follow the reference:
statistics of the in-range pairs' oriented insert sizes, the exceptional pairs in (contig,
minPos) order, the compatibility graph, and one greedy clique per connected component (host).
Each stage can be called on its own, and ``Pairs.from_arrays`` takes pairs from any reader.
There is no host fallback: a file the device loader cannot take (a gzip stream without BGZF
block sizes) is an error."""
from __future__ import annotations

import ctypes as C
import os
import time
from typing import Dict, List, Sequence

import numpy as np

from . import native
from .bamdev import MappedBam, _raise

PAIR_FIELDS = ("contig", "start", "mate_contig", "mate_start", "tlen", "len", "strand")
TSV_HEADER = "contig\tstart\tstop\tpairs\twiggle"


def _cliques(res) -> List[dict]:
    c = res.contents
    out = [dict(contig=int(c.contig[k]), start=int(c.start[k]), stop=int(c.stop[k]), pairs=int(c.pairs[k]),
                wiggle=int(c.wiggle[k])) for k in range(int(c.n))]
    native.lib().gq_sv_free_cliques(res)
    return out


class Pairs:
    """Resident pairs (gq_sv_pairs) and, after ``stats`` or ``select``, the node set."""

    def __init__(self, ctx: native.Context, h: C.c_void_p):
        self.ctx = ctx  # (keeps the context alive)
        self.h = h

    @classmethod
    def from_arrays(cls, ctx: native.Context, cols: Dict[str, Sequence[int]]) -> "Pairs":
        """Pairs already through the command's record filter: cols[f] for f in PAIR_FIELDS."""
        a = [np.ascontiguousarray(cols[f], np.uint8 if f == "strand" else np.int32) for f in PAIR_FIELDS]
        n = len(a[0])
        if any(len(x) != n for x in a):
            raise ValueError("pair columns differ in length")
        h = C.c_void_p()
        native._check(native.lib().gq_sv_pairs_from_host(ctx.h, n, *[x.ctypes.data for x in a], C.byref(h)))
        return cls(ctx, h)

    def __len__(self) -> int:
        return int(native.lib().gq_sv_pairs_count(self.h))

    def download(self) -> Dict[str, np.ndarray]:
        n = len(self)
        out = {f: np.empty(n, np.uint8 if f == "strand" else np.int32) for f in PAIR_FIELDS}
        native._check(native.lib().gq_sv_pairs_download(self.h, *[out[f].ctypes.data for f in PAIR_FIELDS]))
        return out

    def stats(self) -> dict:
        """gq_sv_stats_call: the statistics; the node set becomes the exceptional pairs."""
        s = native.gq_sv_stats()
        native._check(native.lib().gq_sv_stats_call(self.h, C.byref(s)))
        return _stats_dict(s)

    def select(self, threshold: int) -> int:
        """gq_sv_select: the node set for a threshold of the caller's; returns its size."""
        n = C.c_int64()
        native._check(native.lib().gq_sv_select(self.h, int(threshold), C.byref(n)))
        self._n_nodes = int(n.value)
        return self._n_nodes

    def nodes(self, n: int) -> Dict[str, np.ndarray]:
        """The node set (n of them): contig, lo, hi, len, pair (index in the pairs table)."""
        out = dict(contig=np.empty(n, np.int32), lo=np.empty(n, np.int32), hi=np.empty(n, np.int32),
                   len=np.empty(n, np.int32), pair=np.empty(n, np.int64))
        native._check(native.lib().gq_sv_nodes_download(self.h, *[out[k].ctypes.data for k in out]))
        return out

    def graph(self, max_normal: int) -> dict:
        """gq_sv_graph_call: dict(n_nodes, i, j, weight, edge_ms)."""
        g = C.POINTER(native.gq_sv_graph)()
        native._check(native.lib().gq_sv_graph_call(self.h, int(max_normal), C.byref(g)))
        c = g.contents
        m = int(c.n_edges)
        out = dict(n_nodes=int(c.n_nodes), edge_ms=float(c.edge_ms),
                   i=np.ctypeslib.as_array(c.i, (m,)).copy() if m else np.zeros(0, np.int32),
                   j=np.ctypeslib.as_array(c.j, (m,)).copy() if m else np.zeros(0, np.int32),
                   weight=np.ctypeslib.as_array(c.weight, (m,)).copy() if m else np.zeros(0, np.int64))
        native.lib().gq_sv_free_graph(g)
        return out

    def call(self) -> dict:
        """gq_sv_call: dict(stats, cliques, edge_ms, clique_ms)."""
        s = native.gq_sv_stats()
        res = C.POINTER(native.gq_sv_cliques)()
        e_ms, c_ms = C.c_float(), C.c_float()
        native._check(native.lib().gq_sv_call(self.h, C.byref(s), C.byref(res), C.byref(e_ms), C.byref(c_ms)))
        return dict(stats=_stats_dict(s), cliques=_cliques(res), edge_ms=float(e_ms.value),
                    clique_ms=float(c_ms.value))

    def free(self) -> None:
        if self.h:
            native.lib().gq_sv_pairs_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _stats_dict(s) -> dict:
    return {k: getattr(s, k) for k in ("n_pairs", "n_in_range", "n_exceptional", "median", "mad", "max_normal",
                                       "stats_ms", "order_ms")}


def cliques(nodes: Dict[str, np.ndarray], i, j, weight, max_normal: int) -> List[dict]:
    """gq_sv_cliques_call (host): cliques of an edge list over nodes in (contig, lo) order."""
    cols = [np.ascontiguousarray(nodes[k], np.int32) for k in ("contig", "lo", "hi", "len")]
    e = [np.ascontiguousarray(i, np.int32), np.ascontiguousarray(j, np.int32), np.ascontiguousarray(weight, np.int64)]
    res = C.POINTER(native.gq_sv_cliques)()
    native._check(native.lib().gq_sv_cliques_call(len(cols[0]), *[x.ctypes.data for x in cols], len(e[0]),
                                                  *[x.ctypes.data for x in e], int(max_normal), C.byref(res)))
    return _cliques(res)


def load_pairs(ctx: native.Context, path: str):
    """BAM -> (Pairs, contig names, timings): the device loader's inflate, the record list and
    pair_parse.  The mapped file and the inflated stream are released before returning."""
    L = native.lib()
    t0 = time.perf_counter()
    m = MappedBam(path)
    if not m.ok:
        raise ValueError("%s: a gzip stream without BGZF block sizes cannot be loaded on the device" % path)
    names, _ = m.contigs()
    h, m.h = m.h, C.c_void_p()
    try:
        _raise(L.gq_bam_dev_load(ctx.h, h))
        t1 = time.perf_counter()
        out = C.c_void_p()
        ms = C.c_float()
        _raise(L.gq_sv_pairs_from_bam(h, C.byref(out), C.byref(ms)))
    finally:
        L.gq_bam_dev_close(h)
    return Pairs(ctx, out), names, dict(load_s=t1 - t0, pairs_s=time.perf_counter() - t1, pair_parse_ms=float(ms.value))


def text_lines(node_contigs: Sequence[int], found: List[dict], contig_names: Sequence[str]) -> List[str]:
    """The reference's saveAsTextFile lines: (contig,List(GenomeRange(contig,start,stop), ...)) for
    every contig with an exceptional pair, contigs in dictionary order."""
    by: Dict[str, List[str]] = {contig_names[int(c)]: [] for c in node_contigs}
    for c in found:
        name = contig_names[c["contig"]]
        by[name].append("GenomeRange(%s,%d,%d)" % (name, c["start"], c["stop"]))
    return ["(%s,List(%s))" % (name, ", ".join(by[name])) for name in sorted(by)]


def tsv_lines(found: List[dict], contig_names: Sequence[str]) -> List[str]:
    rows = sorted(range(len(found)), key=lambda k: (contig_names[found[k]["contig"]], found[k]["start"],
                                                    found[k]["stop"], k))
    return [TSV_HEADER] + ["%s\t%d\t%d\t%d\t%d" % (contig_names[found[k]["contig"]], found[k]["start"],
                                                     found[k]["stop"], found[k]["pairs"], found[k]["wiggle"])
                           for k in rows]


def structural_variant(ctx: native.Context, path: str) -> dict:
    """The whole command on one BAM: dict(contig_names, stats, cliques, node_contigs, timings)."""
    pairs, names, timings = load_pairs(ctx, path)
    try:
        res = pairs.call()
        nodes = pairs.nodes(int(res["stats"]["n_exceptional"]))
    finally:
        pairs.free()
    timings.update(stats_ms=res["stats"]["stats_ms"], order_ms=res["stats"]["order_ms"], edge_ms=res["edge_ms"],
                   clique_ms=res["clique_ms"])
    return dict(contig_names=names, stats=res["stats"], cliques=res["cliques"], node_contigs=nodes["contig"],
                timings=timings)


def write_output(out_dir: str, lines: Sequence[str]) -> str:
    """saveAsTextFile's layout, coalesce(1): DIR/part-00000 and the _SUCCESS marker."""
    os.makedirs(out_dir, exist_ok=False)
    part = os.path.join(out_dir, "part-00000")
    with open(part, "w") as fh:
        fh.writelines(l + "\n" for l in lines)
    open(os.path.join(out_dir, "_SUCCESS"), "w").close()
    return part
