// gq_sv_clique.h — structural-variant: the cliques of the pair graph (gq_sv_cliques_call), plain
// C++ for the host (StructuralVariantCaller.scala:191-271, findCliques / findOneClique /
// SVClique).  Nodes are the exceptional pairs in (contig, lo) order, edges (i, j, weight) with
// i < j, each pair of nodes at most once.  Every connected component with an edge gives one
// clique, grown greedily:
//   edges in (weight, i, j) order; the seed is the first edge's i (the end with the lower lo;
//   i on a tie); svStart = GapMin, svEnd = GapMax, wiggle = N - (insertSize - (svEnd - svStart))
//   each edge with exactly one end inside offers its outside node, taken when it is adjacent to
//   every member, newStart = max(svStart, GapMin) < newEnd = min(svEnd, GapMax) and
//   newWiggle = min(N - (insertSize - (newEnd - newStart)),
//                   wiggle + (newEnd - newStart) - (svEnd - svStart)) >= 0.
// Adjacency to every member is a counter per node (members among its neighbours), raised along
// the new member's neighbour list, so a component costs its edges' sort and one pass.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

namespace gq_sv {

struct Clique {
  int32_t contig;
  int64_t start, stop, pairs, wiggle;
};

inline std::vector<Clique> find_cliques(int64_t n, const int32_t *contig, const int32_t *lo, const int32_t *hi,
                                        const int32_t *len, int64_t m, const int32_t *ei, const int32_t *ej,
                                        const int64_t *w, int64_t N) {
  std::vector<Clique> out;
  if (n <= 0 || m <= 0) return out;
  // components (union-find, the smaller index the root: a component's root is its first node)
  std::vector<int64_t> root((size_t)n);
  std::iota(root.begin(), root.end(), (int64_t)0);
  auto find = [&](int64_t x) {
    while (root[(size_t)x] != x) {
      root[(size_t)x] = root[(size_t)root[(size_t)x]];
      x = root[(size_t)x];
    }
    return x;
  };
  for (int64_t e = 0; e < m; ++e) {
    const int64_t a = find(ei[e]), b = find(ej[e]);
    if (a != b) root[(size_t)std::max(a, b)] = std::min(a, b);
  }
  // neighbour lists (CSR over both ends of every edge)
  std::vector<int64_t> adj_off((size_t)n + 1, 0);
  for (int64_t e = 0; e < m; ++e) {
    ++adj_off[(size_t)ei[e] + 1];
    ++adj_off[(size_t)ej[e] + 1];
  }
  for (int64_t k = 0; k < n; ++k) adj_off[(size_t)k + 1] += adj_off[(size_t)k];
  std::vector<int32_t> adj((size_t)(2 * m));
  {
    std::vector<int64_t> at(adj_off.begin(), adj_off.end() - 1);
    for (int64_t e = 0; e < m; ++e) {
      adj[(size_t)at[(size_t)ei[e]]++] = ej[e];
      adj[(size_t)at[(size_t)ej[e]]++] = ei[e];
    }
  }
  // edges by (component's first node, weight, i, j)
  std::vector<int64_t> ord((size_t)m), comp((size_t)m);
  std::iota(ord.begin(), ord.end(), (int64_t)0);
  for (int64_t e = 0; e < m; ++e) comp[(size_t)e] = find(ei[e]);
  std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) {
    if (comp[(size_t)a] != comp[(size_t)b]) return comp[(size_t)a] < comp[(size_t)b];
    if (w[a] != w[b]) return w[a] < w[b];
    if (ei[a] != ei[b]) return ei[a] < ei[b];
    return ej[a] < ej[b];
  });
  std::vector<char> in((size_t)n, 0);
  std::vector<int64_t> near((size_t)n, 0);  // members among the node's neighbours
  for (int64_t k0 = 0; k0 < m;) {
    int64_t k1 = k0;
    while (k1 < m && comp[(size_t)ord[(size_t)k1]] == comp[(size_t)ord[(size_t)k0]]) ++k1;
    auto gap_min = [&](int64_t x) { return (int64_t)lo[x] + len[x]; };
    auto insert = [&](int64_t x) { return (int64_t)hi[x] - lo[x] + len[x]; };
    int64_t members = 0;
    auto add = [&](int64_t x) {
      in[(size_t)x] = 1;
      ++members;
      for (int64_t q = adj_off[(size_t)x]; q < adj_off[(size_t)x + 1]; ++q) ++near[(size_t)adj[(size_t)q]];
    };
    const int64_t seed = ei[ord[(size_t)k0]];
    int64_t s = gap_min(seed), t = hi[seed];
    int64_t wiggle = N - (insert(seed) - (t - s));
    add(seed);
    for (int64_t k = k0; k < k1; ++k) {
      const int64_t e = ord[(size_t)k];
      const bool a = in[(size_t)ei[e]], b = in[(size_t)ej[e]];
      if (a == b) continue;
      const int64_t x = a ? ej[e] : ei[e];
      if (near[(size_t)x] != members) continue;
      const int64_t ns = std::max(s, gap_min(x)), nt = std::min(t, (int64_t)hi[x]);
      const int64_t nw = std::min(N - (insert(x) - (nt - ns)), wiggle + (nt - ns) - (t - s));
      if (ns < nt && nw >= 0) {
        s = ns;
        t = nt;
        wiggle = nw;
        add(x);
      }
    }
    out.push_back(Clique{contig[seed], s, t, members, wiggle});
    k0 = k1;
  }
  // (components come in first-node order: a stable sort keeps it among equal spans)
  std::stable_sort(out.begin(), out.end(), [](const Clique &a, const Clique &b) {
    if (a.contig != b.contig) return a.contig < b.contig;
    if (a.start != b.start) return a.start < b.start;
    return a.stop < b.stop;
  });
  return out;
}

}  // namespace gq_sv
