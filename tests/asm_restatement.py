"""A dictionary-based restatement of the local-assembly rules (DESIGN.md "Local assembly";
assembly/DeBruijnGraph.scala): strings and dicts only, nothing shared with the library.  The tests
compare it with the reference suite's expectations, and the host twin with it."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

BASES = "ACGT"
OK, SHORT, REF_N, NO_SOURCE, NO_SINK = 0, 1, 2, 3, 4
PATHS_CAPPED, STEPS_CAPPED, LENGTH_CAPPED = 16, 32, 64


def merge_kmers(kmers: Sequence[str]) -> str:
    """DeBruijnGraph.mergeKmers (296-300)."""
    return (kmers[0][:-1] if kmers else "") + "".join(x[-1] for x in kmers)


def standard(seq: bytes) -> bool:
    """Bases.allStandardBases: upper-case A C G T only."""
    return all(chr(b) in BASES for b in seq)


class Graph:
    def __init__(self, sequences: Sequence[bytes], k: int, min_occurrence: int = 1):
        self.k = k
        self.all_counts: Dict[str, int] = {}
        self.n_reads = 0
        self.n_instances = 0
        for s in sequences:
            s = bytes(s)
            if len(s) < k or not standard(s):
                continue
            self.n_reads += 1
            self.n_instances += len(s) - k + 1
            t = s.decode()
            for i in range(len(t) - k + 1):
                self.all_counts[t[i:i + k]] = self.all_counts.get(t[i:i + k], 0) + 1
        self.counts = {x: c for x, c in self.all_counts.items() if c >= min_occurrence}
        self.nodes = sorted(self.counts)

    def children(self, x: str) -> List[str]:
        return [x[1:] + b for b in BASES if x[1:] + b in self.counts]

    def parents(self, x: str) -> List[str]:
        return [b + x[:-1] for b in BASES if b + x[:-1] in self.counts]

    def mask(self, x: str, forward: bool) -> int:
        near = self.children(x) if forward else self.parents(x)
        return sum(1 << BASES.index(y[-1] if forward else y[0]) for y in near)

    # -- unitigs -----------------------------------------------------------------------------
    def _next(self, x: str) -> Optional[str]:
        c = self.children(x)
        return c[0] if len(c) == 1 and c[0] != x and len(self.parents(c[0])) == 1 else None

    def _prev(self, x: str) -> Optional[str]:
        p = self.parents(x)
        return p[0] if len(p) == 1 and p[0] != x and len(self.children(p[0])) == 1 else None

    def merge_forward(self, x: str) -> List[str]:
        out = [x]
        while self._next(out[-1]) is not None and self._next(out[-1]) not in out:
            out.append(self._next(out[-1]))
        return out

    def merge_backward(self, x: str) -> List[str]:
        out = [x]
        while self._prev(out[0]) is not None and self._prev(out[0]) not in out:
            out.insert(0, self._prev(out[0]))
        return out

    def unitigs(self) -> List[List[str]]:
        seen, out = set(), []
        for x in self.nodes:  # ascending: a cycle is met first at its smallest k-mer
            if x in seen:
                continue
            path = self.merge_forward(x)
            if self._next(path[-1]) != x:  # not a cycle closing on x: it may extend backwards too
                path = self.merge_backward(x)[:-1] + path
            seen.update(path)
            out.append(path)
        return sorted(out, key=lambda p: p[0])

    # -- search ------------------------------------------------------------------------------
    def search(self, source: str, sink: str, max_len: int, max_paths: int = 10,
               max_steps: int = 1000000) -> Tuple[List[List[str]], int, int]:
        """(paths, cap flags, steps)."""
        paths: List[List[str]] = []
        flags, steps = 0, 1
        if source == sink:
            return [[source]], 0, 1
        if max_len < 1:
            return [], LENGTH_CAPPED, 1
        path, it = [source], [0]
        while path:
            x, b = path[-1], it[-1]
            if b == 4:
                path.pop()
                it.pop()
                continue
            it[-1] += 1
            y = x[1:] + BASES[b]
            if y not in self.counts or y in path:
                continue
            if len(path) + 1 > max_len:
                flags |= LENGTH_CAPPED
                continue
            if steps >= max_steps:
                return paths, flags | STEPS_CAPPED, steps
            steps += 1
            if y == sink:
                if len(paths) >= max_paths:
                    return paths, flags | PATHS_CAPPED, steps
                paths.append(path + [y])
                continue
            path.append(y)
            it.append(0)
        return paths, flags, steps


def window(sequences: Sequence[bytes], reference: Optional[bytes], win_len: int, k: int, min_occurrence: int = 1,
           max_paths: int = 10, max_path_length: int = 0, max_steps: int = 1000000) -> Dict[str, object]:
    """Everything the library reports for one window, as plain Python values."""
    g = Graph(sequences, k, min_occurrence)
    source = sink = -1
    ref_ok = False
    if win_len >= k and reference is not None:
        a, z = bytes(reference[:k]), bytes(reference[win_len - k:win_len])
        ref_ok = standard(a) and standard(z)
        if ref_ok:
            source = g.nodes.index(a.decode()) if a.decode() in g.counts else -1
            sink = g.nodes.index(z.decode()) if z.decode() in g.counts else -1
    status = SHORT if win_len < k else REF_N if not ref_ok else NO_SOURCE if source < 0 else NO_SINK if sink < 0 else OK
    paths, flags, steps = [], 0, 0
    if status == OK:
        paths, flags, steps = g.search(g.nodes[source], g.nodes[sink],
                                       max_path_length or win_len - k + 1 + 64, max_paths, max_steps)
    return dict(nodes=g.nodes, count=[g.counts[x] for x in g.nodes], child_mask=[g.mask(x, True) for x in g.nodes],
                parent_mask=[g.mask(x, False) for x in g.nodes], source=source, sink=sink, status=status,
                n_reads=g.n_reads, n_instances=g.n_instances, path_status=status | flags, steps=steps,
                haplotypes=[merge_kmers(p) for p in paths], support=[min(g.counts[x] for x in p) for p in paths],
                unitigs=[merge_kmers(u) for u in g.unitigs()])
