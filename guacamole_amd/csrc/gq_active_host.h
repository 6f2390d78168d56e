// gq_active_host.h — active regions on the CPU (gqpileup.h: gq_active_regions_host): plain C++, no
// device.  The twin the device result (gq_active.h) is compared with field for field, and what a
// stand-alone program can call (tests/native/active_check.cpp).
//
// What both sides must do alike is written once here and called from the kernels too: a locus'
// evidence (evidence), the predicate (is_active), the sort key (key_of), the merge rule (same_region)
// and a region's bounds (region_start, region_end).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/gqpileup.h"
#include "gq_strictmath.h"  // GQ_HD

namespace gq_active {

// e of a locus: the A C G T elements that are not the reference base's, plus Insertion, Deletion and
// MidDeletion elements.  bc: base_count (A C G T N other), kc: kind_count (Insertion, Deletion,
// MidDeletion, Clipped).  No evidence where the reference base is not one of A C G T.
GQ_HD int32_t evidence(uint8_t ref_base, int32_t ref_depth, const int32_t *bc, const int32_t *kc) {
  if (ref_base != 'A' && ref_base != 'C' && ref_base != 'G' && ref_base != 'T') return 0;
  return bc[0] + bc[1] + bc[2] + bc[3] - ref_depth + kc[0] + kc[1] + kc[2];
}

GQ_HD bool is_active(const gq_active_params &p, int32_t depth, int32_t e) {
  const int32_t min_depth = p.min_depth < 1 ? 1 : p.min_depth, min_e = p.min_evidence < 1 ? 1 : p.min_evidence;
  return depth >= min_depth && e >= min_e && (int64_t)100 * e >= (int64_t)p.min_percent * depth;
}

GQ_HD uint64_t key_of(int32_t contig, int64_t pos) { return (uint64_t)(uint32_t)contig << 32 | (uint64_t)(uint32_t)pos; }
GQ_HD int32_t key_contig(uint64_t key) { return (int32_t)(key >> 32); }
GQ_HD int64_t key_pos(uint64_t key) { return (int64_t)(uint32_t)key; }

// Do two active loci, `prev` before `next` in key order, fall in one region?
GQ_HD bool same_region(uint64_t prev, uint64_t next, int32_t pad) {
  return key_contig(prev) == key_contig(next) && key_pos(next) - key_pos(prev) <= 2 * (int64_t)pad + 1;
}
GQ_HD int64_t region_start(int64_t first, int32_t pad) { return first > pad ? first - pad : 0; }
GQ_HD int64_t region_end(int64_t last, int32_t pad) { return last + pad + 1; }

inline bool params_ok(const gq_active_params *p) { return p && p->pad >= 0 && p->min_percent >= 0 && p->min_percent <= 100; }

// byte offsets of the arrays inside the block: the device image and the host block are laid out alike
struct Layout {
  size_t contig, start, end, n_active, evidence, l_contig, l_pos, l_depth, l_evidence, bytes;
};
inline Layout layout(int64_t n_regions, int64_t n_loci) {
  auto al = [](size_t x) { return (x + 63) & ~(size_t)63; };
  const size_t R = (size_t)n_regions, N = (size_t)n_loci;
  Layout L;
  L.contig = 0;
  L.start = al(L.contig + 4 * R);
  L.end = al(L.start + 8 * R);
  L.n_active = al(L.end + 8 * R);
  L.evidence = al(L.n_active + 4 * R);
  L.l_contig = al(L.evidence + 8 * R);
  L.l_pos = al(L.l_contig + 4 * N);
  L.l_depth = al(L.l_pos + 8 * N);
  L.l_evidence = al(L.l_depth + 4 * N);
  L.bytes = al(L.l_evidence + 4 * N + 1);
  return L;
}

inline void free_block(gq_active_regions *r) {
  if (!r) return;
  free(r->block_);  // one block holds every array
  free(r);
}

// A result with its block allocated and its pointers set (the arrays are not filled); null: no memory.
inline gq_active_regions *new_block(int64_t n_regions, int64_t n_loci) {
  gq_active_regions *r = (gq_active_regions *)calloc(1, sizeof(gq_active_regions));
  if (!r) return nullptr;
  const Layout L = layout(n_regions, n_loci);
  uint8_t *blk = (uint8_t *)malloc(L.bytes);
  if (!blk) {
    free(r);
    return nullptr;
  }
  r->block_ = blk;
  r->n = n_regions;
  r->contig = (int32_t *)(blk + L.contig);
  r->start = (int64_t *)(blk + L.start);
  r->end = (int64_t *)(blk + L.end);
  r->n_active = (int32_t *)(blk + L.n_active);
  r->evidence = (int64_t *)(blk + L.evidence);
  r->n_loci = n_loci;
  r->locus_contig = (int32_t *)(blk + L.l_contig);
  r->locus_pos = (int64_t *)(blk + L.l_pos);
  r->locus_depth = (int32_t *)(blk + L.l_depth);
  r->locus_evidence = (int32_t *)(blk + L.l_evidence);
  r->block_bytes = (int64_t)L.bytes;
  return r;
}

struct Locus {
  uint64_t key;
  int32_t depth, e;
};

// The contract over pileup-count columns (rows in any order).  Null: no memory.
inline gq_active_regions *run_host(int64_t n_rows, const int32_t *contig, const int64_t *pos, const uint8_t *ref_base,
                                   const int32_t *depth, const int32_t *ref_depth, const int32_t *base_count,
                                   const int32_t *kind_count, const gq_active_params &p) {
  std::vector<Locus> act;
  for (int64_t i = 0; i < n_rows; ++i) {
    const int32_t e = evidence(ref_base[i], ref_depth[i], base_count + 6 * i, kind_count + 4 * i);
    if (is_active(p, depth[i], e)) act.push_back(Locus{key_of(contig[i], pos[i]), depth[i], e});
  }
  std::sort(act.begin(), act.end(), [](const Locus &a, const Locus &b) { return a.key < b.key; });
  const size_t n = act.size();
  int64_t n_regions = 0;
  for (size_t i = 0; i < n; ++i) n_regions += i == 0 || !same_region(act[i - 1].key, act[i].key, p.pad);
  gq_active_regions *r = new_block(n_regions, (int64_t)n);
  if (!r) return nullptr;
  int64_t k = -1;
  for (size_t i = 0; i < n; ++i) {
    const int64_t at = key_pos(act[i].key);
    r->locus_contig[i] = key_contig(act[i].key);
    r->locus_pos[i] = at;
    r->locus_depth[i] = act[i].depth;
    r->locus_evidence[i] = act[i].e;
    if (i == 0 || !same_region(act[i - 1].key, act[i].key, p.pad)) {
      ++k;
      r->contig[k] = key_contig(act[i].key);
      r->start[k] = region_start(at, p.pad);
      r->n_active[k] = 0;
      r->evidence[k] = 0;
    }
    r->end[k] = region_end(at, p.pad);
    r->n_active[k] += 1;
    r->evidence[k] += act[i].e;
  }
  return r;
}

}  // namespace gq_active
