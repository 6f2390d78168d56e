// The host twin of the active-regions stage (guacamole_amd/csrc/gq_active_host.h, the body of
// gq_active_regions_host) as a stand-alone program over a few hundred generated rows, for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all active_check.cpp
// Prints one line per case.  Exit 0 when every expectation below holds.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../guacamole_amd/csrc/gq_active_host.h"

namespace {

int wrong = 0;
void expect(bool ok, const char *what) {
  if (!ok) {
    fprintf(stderr, "failed: %s\n", what);
    ++wrong;
  }
}

struct Rows {  // exact-size heap arrays, so that a read past an end is caught
  std::vector<int32_t> contig, depth, ref_depth, base_count, kind_count;
  std::vector<int64_t> pos;
  std::vector<uint8_t> ref_base;
  void add(int32_t c, int64_t p, char ref, int32_t n_ref, int32_t n_alt, int32_t n_ins, int32_t n_clip) {
    contig.push_back(c);
    pos.push_back(p);
    ref_base.push_back((uint8_t)ref);
    const int32_t bc[6] = {n_ref, n_alt, 0, 0, 0, 0};  // the reference base A (or N: then A is no reference count)
    const int32_t kc[4] = {n_ins, 0, 0, n_clip};
    base_count.insert(base_count.end(), bc, bc + 6);
    kind_count.insert(kind_count.end(), kc, kc + 4);
    depth.push_back(n_ref + n_alt + n_ins + n_clip);
    ref_depth.push_back(ref == 'A' ? n_ref : 0);
  }
  gq_active_regions *run(const gq_active_params &p) {
    for (auto *v : {&contig, &depth, &ref_depth, &base_count, &kind_count}) v->shrink_to_fit();
    pos.shrink_to_fit();
    ref_base.shrink_to_fit();
    return gq_active::run_host((int64_t)pos.size(), contig.data(), pos.data(), ref_base.data(), depth.data(),
                               ref_depth.data(), base_count.data(), kind_count.data(), p);
  }
};

uint32_t rnd(uint32_t &s) {
  s = s * 1664525u + 1013904223u;
  return s >> 8;
}

}  // namespace

int main() {
  gq_active_params p;
  memset(&p, 0, sizeof(p));
  p.min_mapq = 1, p.min_depth = 4, p.min_evidence = 2, p.min_percent = 8, p.pad = 5;
  // 600 rows over three contigs in a scrambled order; about one in nine is active
  Rows x;
  uint32_t s = 7;
  std::vector<int64_t> order;
  for (int64_t i = 0; i < 600; ++i) order.push_back((i * 77) % 600);
  int64_t n_act = 0, sum_e = 0;
  for (int64_t i : order) {
    const int32_t c = (int32_t)(i / 200);
    const int64_t at = (i % 200) * 3;
    const bool hot = rnd(s) % 9 == 0;
    const int32_t n_alt = hot ? 2 + (int32_t)(rnd(s) % 5) : (int32_t)(rnd(s) % 2), n_ins = hot ? (int32_t)(rnd(s) % 3) : 0;
    x.add(c, at, 'A', 12, n_alt, n_ins, (int32_t)(rnd(s) % 4));
    const int32_t e = n_alt + n_ins;
    if (e >= 2 && 100 * (int64_t)e >= 8 * (int64_t)x.depth.back()) {
      ++n_act;
      sum_e += e;
    }
  }
  gq_active_regions *a = x.run(p);
  if (!a) return 2;
  int64_t loci_in_regions = 0, e_in_regions = 0;
  for (int64_t r = 0; r < a->n; ++r) {
    loci_in_regions += a->n_active[r];
    e_in_regions += a->evidence[r];
    expect(a->end[r] > a->start[r] && a->start[r] >= 0, "a region is not empty");
    if (r > 0) expect(a->contig[r] > a->contig[r - 1] || a->start[r] > a->end[r - 1], "regions ascend and do not touch");
  }
  for (int64_t i = 1; i < a->n_loci; ++i)
    expect(a->locus_contig[i] > a->locus_contig[i - 1] ||
               (a->locus_contig[i] == a->locus_contig[i - 1] && a->locus_pos[i] > a->locus_pos[i - 1]),
           "the active loci ascend");
  printf("generated: %lld rows, %lld active loci, %lld regions, evidence %lld, block %lld bytes\n", (long long)x.pos.size(),
         (long long)a->n_loci, (long long)a->n, (long long)e_in_regions, (long long)a->block_bytes);
  expect(a->n_loci == n_act && n_act > 30, "the active loci are those the generator planted");
  expect(loci_in_regions == n_act && e_in_regions == sum_e, "the regions' counts add up to the loci's");
  expect(a->n >= 3 && a->n < a->n_loci, "some loci merged, some did not");
  gq_active::free_block(a);
  // the merge boundary, the clip at 0, two contigs, a reference N
  Rows y;
  y.add(1, 3, 'A', 5, 5, 0, 0);
  y.add(0, 100, 'A', 5, 5, 0, 0);
  y.add(0, 100 + 11, 'A', 5, 5, 0, 0);
  y.add(0, 100 + 11 + 12, 'A', 5, 5, 0, 0);
  y.add(0, 50, 'N', 5, 5, 4, 0);
  gq_active_regions *b = y.run(p);
  if (!b) return 2;
  printf("hand-built: %lld regions of %lld loci\n", (long long)b->n, (long long)b->n_loci);
  expect(b->n == 3 && b->n_loci == 4, "three regions of four loci");
  expect(b->n == 3 && b->start[0] == 95 && b->end[0] == 117 && b->n_active[0] == 2 && b->evidence[0] == 10,
         "a spacing of 2 * pad + 1 merges");
  expect(b->n == 3 && b->start[1] == 118 && b->end[1] == 129, "a spacing of 2 * pad + 2 does not");
  expect(b->n == 3 && b->contig[2] == 1 && b->start[2] == 0 && b->end[2] == 9, "the start clips to 0");
  gq_active::free_block(b);
  // no row at all, and parameters out of range
  Rows z;
  gq_active_regions *e = z.run(p);
  if (!e) return 2;
  printf("empty: %lld regions\n", (long long)e->n);
  expect(e->n == 0 && e->n_loci == 0 && e->block_ != nullptr && e->block_bytes > 0, "an empty input gives a valid block");
  gq_active::free_block(e);
  gq_active::free_block(nullptr);
  gq_active_params q = p;
  q.pad = -1;
  expect(gq_active::params_ok(&p) && !gq_active::params_ok(&q) && !gq_active::params_ok(nullptr), "a negative pad is refused");
  q = p;
  q.min_percent = 101;
  expect(!gq_active::params_ok(&q), "a percent over 100 is refused");
  return wrong ? 1 : 0;
}
