// gq_assemble_host.h — local assembly on the CPU (gqpileup.h: gq_asm_graphs_host, gq_asm_paths):
// plain C++, no device.  The graph half is the twin the device graphs (gq_assemble.h) are compared
// with array for array; the path search and the unitigs run here for both, over the graph block.
// A stand-alone program can include this file (tests/native/asm_check.cpp).
//
// Restates assembly/DeBruijnGraph.scala: apply (271-294: all-standard reads, sliding k-mers, counts,
// pruneKmers), children / parents (253-264), findMergeable (130-159) as the set of maximal
// unbranched paths, mergeKmers (296-300).  The search is NOT depthFirstSearch (176-238), see
// DESIGN.md "Local assembly": every simple source-sink path, children in A C G T order.
//
// Packed k-mer: 2 bits a base (A 0, C 1, G 2, T 3), the first base most significant; `lo` holds
// the last min(k, 31) bases, `hi` the k - 31 before them (0 when k <= 31).  Both stay below 2^62,
// so all-ones is free as the hash tables' empty mark, and (hi, lo) orders as the k-mers do.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/gqpileup.h"

#if defined(__HIPCC__)
#define GQ_ASM_HD __host__ __device__ __forceinline__
#else
#define GQ_ASM_HD inline
#endif

namespace gq_asm {

constexpr int kMinK = 2, kMaxK = 62, kWordBases = 31;
constexpr uint64_t kEmpty = ~0ull;

struct Key {
  uint64_t lo, hi;
};
struct Shape {  // of k: bases and masks of the two words
  int L, H;
  uint64_t mask_lo, mask_hi;
};
GQ_ASM_HD Shape shape_of(int k) {
  Shape s;
  s.L = k < kWordBases ? k : kWordBases;
  s.H = k - s.L;
  s.mask_lo = (1ull << (2 * s.L)) - 1;
  s.mask_hi = s.H ? (1ull << (2 * s.H)) - 1 : 0;
  return s;
}
GQ_ASM_HD int base_code(uint8_t b) {  // Bases.isStandardBase: upper case only; -1 otherwise
  return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : -1;
}
// the k-mer one base on: drop the first base, append b (also a node's child by b)
GQ_ASM_HD Key roll(const Shape &s, Key x, int b) {
  Key y;
  y.hi = s.H ? ((x.hi << 2) | (x.lo >> (2 * s.L - 2))) & s.mask_hi : 0;
  y.lo = ((x.lo << 2) | (uint64_t)b) & s.mask_lo;
  return y;
}
// a node's parent by b: drop the last base, put b in front
GQ_ASM_HD Key unroll(const Shape &s, Key x, int b) {
  Key y;
  if (s.H) {
    y.lo = (x.lo >> 2) | ((x.hi & 3) << (2 * s.L - 2));
    y.hi = (x.hi >> 2) | ((uint64_t)b << (2 * s.H - 2));
  } else {
    y.lo = (x.lo >> 2) | ((uint64_t)b << (2 * s.L - 2));
    y.hi = 0;
  }
  return y;
}
GQ_ASM_HD uint64_t hash_of(Key x) {  // a 64-bit finalizer over both words
  uint64_t h = x.lo ^ (x.hi * 0x9E3779B97F4A7C15ull);
  h ^= h >> 33;
  h *= 0xFF51AFD7ED558CCDull;
  h ^= h >> 33;
  h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 33;
  return h;
}
GQ_ASM_HD bool key_less(Key a, Key b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
// the k bytes at p as a key; false when one of them is not A C G T
GQ_ASM_HD bool key_of(const Shape &s, const uint8_t *p, int k, Key *out) {
  Key x{0, 0};
  for (int i = 0; i < k; ++i) {
    const int c = base_code(p[i]);
    if (c < 0) return false;
    x = roll(s, x, c);
  }
  *out = x;
  return true;
}
GQ_ASM_HD int base_at(const Shape &s, Key x, int i) {  // base i of the k-mer (0: first)
  const int k = s.L + s.H;
  const int from_end = k - 1 - i;
  return from_end < s.L ? (int)((x.lo >> (2 * from_end)) & 3) : (int)((x.hi >> (2 * (from_end - s.L))) & 3);
}

inline bool valid(const gq_asm_params &p) {
  return p.k >= kMinK && p.k <= kMaxK && p.min_occurrence >= 1 && p.max_paths >= 1 && p.max_path_length >= 0 &&
         p.max_steps >= 1 && p.min_mapq >= 0;
}
inline void default_params(gq_asm_params *p) {
  memset(p, 0, sizeof(*p));
  p->k = 25;
  p->min_occurrence = 1;
  p->max_paths = 10;
  p->max_path_length = 0;  // window length - k + 1 + 64
  p->max_steps = 1000000;
}

// ---- the graph block: one allocation behind block_ ------------------------------------------
inline gq_asm_graph_block *new_graphs(int64_t W, int64_t N) {
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const size_t w = (size_t)(W > 0 ? W : 1), n = (size_t)(N > 0 ? N : 1);
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += up(bytes);
    return o;
  };
  const size_t o_off = take(8 * (w + 1)), o_lo = take(8 * n), o_hi = take(8 * n), o_cnt = take(4 * n), o_cm = take(n),
               o_pm = take(n), o_src = take(4 * w), o_snk = take(4 * w), o_st = take(4 * w), o_nr = take(4 * w),
               o_wl = take(4 * w), o_ni = take(8 * w);
  gq_asm_graph_block *g = (gq_asm_graph_block *)calloc(1, sizeof(gq_asm_graph_block));
  char *b = (char *)calloc(1, at);
  if (!g || !b) {
    free(g);
    free(b);
    return nullptr;
  }
  g->n_windows = W;
  g->n_nodes = N;
  g->node_off = (int64_t *)(b + o_off);
  g->key_lo = (uint64_t *)(b + o_lo);
  g->key_hi = (uint64_t *)(b + o_hi);
  g->count = (int32_t *)(b + o_cnt);
  g->child_mask = (uint8_t *)(b + o_cm);
  g->parent_mask = (uint8_t *)(b + o_pm);
  g->source = (int32_t *)(b + o_src);
  g->sink = (int32_t *)(b + o_snk);
  g->status = (int32_t *)(b + o_st);
  g->n_reads = (int32_t *)(b + o_nr);
  g->win_len = (int32_t *)(b + o_wl);
  g->n_instances = (int64_t *)(b + o_ni);
  g->block_ = b;
  return g;
}
inline void free_graphs(gq_asm_graph_block *g) {
  if (!g) return;
  free(g->block_);
  free(g);
}

// status of a window from what is known about it (the order of the tests is part of the contract)
GQ_ASM_HD int32_t status_of(int win_len, int k, bool ref_ok, int source, int sink) {
  if (win_len < k) return GQ_ASM_SHORT;
  if (!ref_ok) return GQ_ASM_REF_N;
  if (source < 0) return GQ_ASM_NO_SOURCE;
  if (sink < 0) return GQ_ASM_NO_SINK;
  return GQ_ASM_OK;
}

// ---- the twin: one window ------------------------------------------------------------------
struct KeyHash {
  size_t operator()(const Key &x) const { return (size_t)hash_of(x); }
};
struct KeyEq {
  bool operator()(const Key &a, const Key &b) const { return a.lo == b.lo && a.hi == b.hi; }
};
struct WinGraph {
  std::vector<Key> key;
  std::vector<int32_t> count;
  std::vector<uint8_t> cm, pm;
  int32_t source = -1, sink = -1, status = 0, n_reads = 0;
  int64_t n_instances = 0;
};

inline void window_graph(const uint8_t *seq_pool, const int64_t *seq_off, const int32_t *seq_len, const int64_t *reads,
                         int64_t n_list, const uint8_t *ref, int32_t win_len, const gq_asm_params &p, WinGraph *out) {
  const int k = p.k;
  const Shape s = shape_of(k);
  std::unordered_map<Key, int32_t, KeyHash, KeyEq> counts;
  WinGraph &g = *out;
  for (int64_t i = 0; i < n_list; ++i) {
    const int64_t r = reads[i];
    const uint8_t *q = seq_pool + seq_off[r];
    const int32_t n = seq_len[r];
    if (n < k) continue;  // (sliding(k) would give one short "k-mer")
    bool ok = true;
    for (int32_t j = 0; j < n && ok; ++j) ok = base_code(q[j]) >= 0;
    if (!ok) continue;
    ++g.n_reads;
    g.n_instances += n - k + 1;
    Key x{0, 0};
    for (int32_t j = 0; j < n; ++j) {
      x = roll(s, x, base_code(q[j]));
      if (j >= k - 1) ++counts[x];
    }
  }
  for (const auto &kv : counts)
    if (kv.second >= p.min_occurrence) g.key.push_back(kv.first);
  std::sort(g.key.begin(), g.key.end(), key_less);
  const size_t n = g.key.size();
  g.count.resize(n);
  g.cm.assign(n, 0);
  g.pm.assign(n, 0);
  auto node = [&](Key x) {
    const auto it = counts.find(x);
    return it != counts.end() && it->second >= p.min_occurrence;
  };
  for (size_t i = 0; i < n; ++i) {
    g.count[i] = counts[g.key[i]];
    for (int b = 0; b < 4; ++b) {
      if (node(roll(s, g.key[i], b))) g.cm[i] |= (uint8_t)(1 << b);
      if (node(unroll(s, g.key[i], b))) g.pm[i] |= (uint8_t)(1 << b);
    }
  }
  bool ref_ok = false;
  if (win_len >= k && ref) {
    Key a, z;
    ref_ok = key_of(s, ref, k, &a) && key_of(s, ref + (win_len - k), k, &z);
    if (ref_ok) {
      auto find = [&](Key x) {
        const auto it = std::lower_bound(g.key.begin(), g.key.end(), x, key_less);
        return it != g.key.end() && KeyEq()(*it, x) ? (int32_t)(it - g.key.begin()) : -1;
      };
      g.source = find(a);
      g.sink = find(z);
    }
  }
  g.status = status_of(win_len, k, ref_ok, g.source, g.sink);
}

// 0 ok, 1 out of memory.  ref_off[w] < 0: the window has no reference (REF_N).
inline int graphs_host(int64_t W, const uint8_t *seq_pool, const int64_t *seq_off, const int32_t *seq_len,
                       const int64_t *win_read_off, const int64_t *win_reads, const uint8_t *ref_pool,
                       const int64_t *ref_off, const int32_t *win_len, const gq_asm_params &p, int threads,
                       gq_asm_graph_block **out) {
  std::vector<WinGraph> g((size_t)W);
  auto work = [&](int64_t a, int64_t step) {
    for (int64_t w = a; w < W; w += step)
      window_graph(seq_pool, seq_off, seq_len, win_reads + win_read_off[w], win_read_off[w + 1] - win_read_off[w],
                   ref_off[w] < 0 ? nullptr : ref_pool + ref_off[w], win_len[w], p, &g[(size_t)w]);
  };
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(threads, W));
  if (T <= 1) {
    work(0, 1);
  } else {
    std::vector<std::thread> pool;
    for (int t = 0; t < T; ++t) pool.emplace_back(work, (int64_t)t, (int64_t)T);
    for (auto &t : pool) t.join();
  }
  int64_t N = 0;
  for (const WinGraph &x : g) N += (int64_t)x.key.size();
  gq_asm_graph_block *b = new_graphs(W, N);
  if (!b) return 1;
  b->k = p.k;
  b->min_occurrence = p.min_occurrence;
  int64_t at = 0;
  for (int64_t w = 0; w < W; ++w) {
    const WinGraph &x = g[(size_t)w];
    b->node_off[w] = at;
    for (size_t i = 0; i < x.key.size(); ++i, ++at) {
      b->key_lo[at] = x.key[i].lo;
      b->key_hi[at] = x.key[i].hi;
      b->count[at] = x.count[i];
      b->child_mask[at] = x.cm[i];
      b->parent_mask[at] = x.pm[i];
    }
    b->source[w] = x.source;
    b->sink[w] = x.sink;
    b->status[w] = x.status;
    b->n_reads[w] = x.n_reads;
    b->win_len[w] = win_len[w];
    b->n_instances[w] = x.n_instances;
  }
  b->node_off[W] = at;
  *out = b;
  return 0;
}

// ---- paths and unitigs over a graph block ----------------------------------------------------
struct WinView {  // window w of a block
  int32_t n;
  const uint64_t *lo, *hi;
  const int32_t *count;
  const uint8_t *cm, *pm;
};
inline WinView view_of(const gq_asm_graph_block *g, int64_t w) {
  const int64_t a = g->node_off[w];
  return WinView{(int32_t)(g->node_off[w + 1] - a), g->key_lo + a, g->key_hi + a, g->count + a, g->child_mask + a,
                 g->parent_mask + a};
}
inline int32_t find_node(const WinView &v, Key x) {
  int32_t a = 0, b = v.n;
  while (a < b) {
    const int32_t m = (a + b) >> 1;
    if (key_less(Key{v.lo[m], v.hi[m]}, x)) a = m + 1;
    else b = m;
  }
  return a < v.n && v.lo[a] == x.lo && v.hi[a] == x.hi ? a : -1;
}
inline int bits(uint8_t m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1); }
inline int first_bit(uint8_t m) { return m & 1 ? 0 : m & 2 ? 1 : m & 4 ? 2 : 3; }

// mergeKmers of nodes path[0..n): k - 1 bases of the first, then every node's last base
inline void merge_kmers(const Shape &s, const WinView &v, const int32_t *path, size_t n, std::vector<uint8_t> &out) {
  static const char B[4] = {'A', 'C', 'G', 'T'};
  if (!n) return;
  const int k = s.L + s.H;
  const Key f{v.lo[path[0]], v.hi[path[0]]};
  for (int i = 0; i + 1 < k; ++i) out.push_back((uint8_t)B[base_at(s, f, i)]);
  for (size_t i = 0; i < n; ++i) out.push_back((uint8_t)B[v.lo[path[i]] & 3]);
}

// the unitigs of a window as node lists, sorted by first k-mer.  Step x -> y is mergeable iff y
// is x's only child, x is y's only parent and x != y; those steps form disjoint paths and cycles.
inline void unitigs_of(const Shape &s, const WinView &v, std::vector<std::vector<int32_t>> &out) {
  const int32_t n = v.n;
  std::vector<int32_t> next((size_t)n, -1), prev((size_t)n, -1);
  for (int32_t x = 0; x < n; ++x) {
    if (bits(v.cm[x]) != 1) continue;
    const int32_t y = find_node(v, roll(s, Key{v.lo[x], v.hi[x]}, first_bit(v.cm[x])));
    if (y < 0 || y == x || bits(v.pm[y]) != 1) continue;
    next[(size_t)x] = y;
    prev[(size_t)y] = x;
  }
  std::vector<uint8_t> done((size_t)n, 0);
  for (int32_t x = 0; x < n; ++x)  // paths: from the nodes nothing merges into
    if (prev[(size_t)x] < 0) {
      std::vector<int32_t> u;
      for (int32_t y = x; y >= 0; y = next[(size_t)y]) {
        u.push_back(y);
        done[(size_t)y] = 1;
      }
      out.push_back(std::move(u));
    }
  for (int32_t x = 0; x < n; ++x)  // what is left are unbranched cycles: from the smallest k-mer
    if (!done[(size_t)x]) {
      std::vector<int32_t> u;
      for (int32_t y = x; !done[(size_t)y]; y = next[(size_t)y]) {
        u.push_back(y);
        done[(size_t)y] = 1;
      }
      out.push_back(std::move(u));
    }
  std::sort(out.begin(), out.end(),
            [](const std::vector<int32_t> &a, const std::vector<int32_t> &b) { return a[0] < b[0]; });
}

struct WinPaths {
  std::vector<std::vector<int32_t>> paths;
  int32_t status = 0;
  int64_t steps = 0;
};

// every simple path source -> sink, depth first, children in A C G T order (see the header)
inline void search(const Shape &s, const WinView &v, int32_t source, int32_t sink, int32_t max_len, int32_t max_paths,
                   int64_t max_steps, WinPaths *out) {
  WinPaths &r = *out;
  std::vector<int32_t> path{source};
  std::vector<uint8_t> it{0}, on((size_t)v.n, 0);
  on[(size_t)source] = 1;
  r.steps = 1;
  if (source == sink) {
    r.paths.push_back(path);
    return;
  }
  if (max_len < 1) {
    r.status |= GQ_ASM_LENGTH_CAPPED;
    return;
  }
  while (!path.empty()) {
    const int32_t x = path.back();
    const int b = it.back();
    if (b == 4) {
      on[(size_t)x] = 0;
      path.pop_back();
      it.pop_back();
      continue;
    }
    ++it.back();
    if (!((v.cm[x] >> b) & 1)) continue;
    const int32_t y = find_node(v, roll(s, Key{v.lo[x], v.hi[x]}, b));
    if (y < 0 || on[(size_t)y]) continue;
    if ((int64_t)path.size() + 1 > max_len) {
      r.status |= GQ_ASM_LENGTH_CAPPED;
      continue;
    }
    if (r.steps >= max_steps) {
      r.status |= GQ_ASM_STEPS_CAPPED;
      return;
    }
    ++r.steps;
    if (y == sink) {
      if ((int64_t)r.paths.size() >= max_paths) {
        r.status |= GQ_ASM_PATHS_CAPPED;
        return;
      }
      r.paths.push_back(path);
      r.paths.back().push_back(y);
      continue;
    }
    path.push_back(y);
    it.push_back(0);
    on[(size_t)y] = 1;
  }
}

inline gq_asm_path_block *new_paths(int64_t W, int64_t nh, int64_t nb, int64_t nu, int64_t nub) {
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  auto one = [](int64_t x) { return (size_t)(x > 0 ? x : 1); };
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += up(bytes);
    return o;
  };
  const size_t o_ho = take(8 * (one(W) + 1)), o_so = take(8 * (one(nh) + 1)), o_b = take(one(nb)),
               o_sup = take(4 * one(nh)), o_st = take(4 * one(W)), o_steps = take(8 * one(W)),
               o_uo = take(8 * (one(W) + 1)), o_uso = take(8 * (one(nu) + 1)), o_ub = take(one(nub));
  gq_asm_path_block *p = (gq_asm_path_block *)calloc(1, sizeof(gq_asm_path_block));
  char *b = (char *)calloc(1, at);
  if (!p || !b) {
    free(p);
    free(b);
    return nullptr;
  }
  p->n_windows = W;
  p->n_haplotypes = nh;
  p->n_unitigs = nu;
  p->hap_off = (int64_t *)(b + o_ho);
  p->hap_seq_off = (int64_t *)(b + o_so);
  p->bases = (uint8_t *)(b + o_b);
  p->support = (int32_t *)(b + o_sup);
  p->status = (int32_t *)(b + o_st);
  p->steps = (int64_t *)(b + o_steps);
  p->unitig_off = (int64_t *)(b + o_uo);
  p->unitig_seq_off = (int64_t *)(b + o_uso);
  p->unitig_bases = (uint8_t *)(b + o_ub);
  p->block_ = b;
  return p;
}
inline void free_paths(gq_asm_path_block *p) {
  if (!p) return;
  free(p->block_);
  free(p);
}

// 0 ok, 1 out of memory
inline int paths_host(const gq_asm_graph_block *g, const gq_asm_params &p, gq_asm_path_block **out) {
  const int64_t W = g->n_windows;
  const Shape s = shape_of(g->k);
  std::vector<int64_t> hap_off{0}, seq_off{0}, u_off{0}, useq_off{0}, steps;
  std::vector<uint8_t> bases, ubases;
  std::vector<int32_t> support, status;
  for (int64_t w = 0; w < W; ++w) {
    const WinView v = view_of(g, w);
    WinPaths r;
    r.status = g->status[w];
    if (g->status[w] == GQ_ASM_OK) {
      const int32_t max_len = p.max_path_length > 0 ? p.max_path_length : g->win_len[w] - g->k + 1 + 64;
      search(s, v, g->source[w], g->sink[w], max_len, p.max_paths, p.max_steps, &r);
    }
    for (const auto &path : r.paths) {
      merge_kmers(s, v, path.data(), path.size(), bases);
      seq_off.push_back((int64_t)bases.size());
      int32_t m = INT32_MAX;
      for (int32_t x : path) m = std::min(m, v.count[x]);
      support.push_back(m);
    }
    hap_off.push_back((int64_t)support.size());
    status.push_back(r.status);
    steps.push_back(r.steps);
    std::vector<std::vector<int32_t>> us;
    unitigs_of(s, v, us);
    for (const auto &u : us) {
      merge_kmers(s, v, u.data(), u.size(), ubases);
      useq_off.push_back((int64_t)ubases.size());
    }
    u_off.push_back((int64_t)useq_off.size() - 1);
  }
  gq_asm_path_block *b =
      new_paths(W, (int64_t)support.size(), (int64_t)bases.size(), (int64_t)useq_off.size() - 1, (int64_t)ubases.size());
  if (!b) return 1;
  memcpy(b->hap_off, hap_off.data(), 8 * hap_off.size());
  memcpy(b->hap_seq_off, seq_off.data(), 8 * seq_off.size());
  if (!bases.empty()) memcpy(b->bases, bases.data(), bases.size());
  if (!support.empty()) memcpy(b->support, support.data(), 4 * support.size());
  if (W > 0) memcpy(b->status, status.data(), 4 * (size_t)W);
  if (W > 0) memcpy(b->steps, steps.data(), 8 * (size_t)W);
  memcpy(b->unitig_off, u_off.data(), 8 * u_off.size());
  memcpy(b->unitig_seq_off, useq_off.data(), 8 * useq_off.size());
  if (!ubases.empty()) memcpy(b->unitig_bases, ubases.data(), ubases.size());
  *out = b;
  return 0;
}

}  // namespace gq_asm
