// The host assembler (guacamole_amd/csrc/gq_assemble_host.h, the bodies of gq_asm_graphs_host and
// gq_asm_paths) as a stand-alone program over the reference suite's cases and the key's word
// boundary, for a sanitizer build:
//   g++ -std=c++17 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all asm_check.cpp
// Prints one line per window: k, status, nodes, haplotypes, unitigs.  Exit 0 when every expectation
// below holds.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../guacamole_amd/csrc/gq_assemble_host.h"

namespace {

struct Case {
  int k, min_occurrence;
  std::vector<std::string> reads;
  std::string ref;
  int status, nodes, haplotypes, unitigs;  // expected; -1 = not pinned here
  std::string first_haplotype;             // empty = not pinned
};

int run(const Case &c, int threads) {
  std::string pool;
  std::vector<int64_t> off, list, roff{0};
  std::vector<int32_t> len;
  for (const std::string &r : c.reads) {
    list.push_back((int64_t)off.size());
    off.push_back((int64_t)pool.size());
    len.push_back((int32_t)r.size());
    pool += r;
  }
  roff.push_back((int64_t)list.size());
  const int64_t ref_off = 0;
  const int32_t wl = (int32_t)c.ref.size();
  gq_asm_params p;
  gq_asm::default_params(&p);
  p.k = c.k;
  p.min_occurrence = c.min_occurrence;
  gq_asm_graph_block *g = nullptr;
  if (!gq_asm::valid(p) ||
      gq_asm::graphs_host(1, (const uint8_t *)pool.data(), off.data(), len.data(), roff.data(), list.data(),
                          (const uint8_t *)c.ref.data(), &ref_off, &wl, p, threads, &g))
    return 1;
  gq_asm_path_block *h = nullptr;
  if (gq_asm::paths_host(g, p, &h)) return 1;
  const std::string first =
      h->n_haplotypes ? std::string((const char *)h->bases, (size_t)h->hap_seq_off[1]) : std::string();
  printf("k %d status %d nodes %lld haplotypes %lld unitigs %lld %s\n", c.k, h->status[0], (long long)g->n_nodes,
         (long long)h->n_haplotypes, (long long)h->n_unitigs, first.c_str());
  int bad = 0;
  bad += c.status >= 0 && h->status[0] != c.status;
  bad += c.nodes >= 0 && g->n_nodes != c.nodes;
  bad += c.haplotypes >= 0 && h->n_haplotypes != c.haplotypes;
  bad += c.unitigs >= 0 && h->n_unitigs != c.unitigs;
  bad += !c.first_haplotype.empty() && first != c.first_haplotype;
  gq_asm::free_paths(h);
  gq_asm::free_graphs(g);
  return bad;
}

}  // namespace

int main() {
  const std::string s = "AAATCCCTGGGT", ref = "GAGGATCTGCCATGGCCGGGCGAGCTGGAGGAGCGAGGAGGAGGCAGGAGGA";
  const int cut[8][2] = {{0, 25}, {5, 30}, {7, 32}, {10, 35}, {19, 41}, {22, 44}, {25, 47}, {31, 52}};
  std::vector<std::string> reads;
  for (const auto &c : cut) reads.push_back(ref.substr((size_t)c[0], (size_t)(c[1] - c[0])));
  reads.back() += "TTT";
  std::string long_ref;  // 140 bases without a repeated 31-mer: a de Bruijn-like walk is not needed, an LCG does
  uint32_t x = 12345;
  for (int i = 0; i < 140; ++i) {
    x = x * 1664525u + 1013904223u;
    long_ref += "ACGT"[(x >> 24) & 3];
  }
  std::vector<Case> cases = {
      {8, 1, {"TCATCTCAAAAGAGATCGA"}, "TCATCTCAAAAGAGATCGA", GQ_ASM_OK, 12, 1, 1, "TCATCTCAAAAGAGATCGA"},
      {3, 1, {"TCATCTTAAAAGACATAAA"}, "TCATCTTAAAAGACATAAA", -1, -1, -1, -1, ""},
      {4, 1, {s}, s, GQ_ASM_OK, 9, 1, 1, s},
      {4, 1, {s, "AAATCCCTGGAT"}, s, GQ_ASM_OK, 11, 1, 3, s},
      {4, 1, {s, "AAATCGCTGGGT"}, s, GQ_ASM_OK, -1, 2, -1, ""},
      {4, 1, {s, "ACATCCCTGGGT"}, s, GQ_ASM_OK, -1, 1, -1, s},
      {15, 1, reads, ref, GQ_ASM_OK, -1, 1, -1, ref},
      {4, 1, {"AAANCCCTGGGT", "aaatccctgggt", "AAA"}, s, GQ_ASM_NO_SOURCE, 0, 0, 0, ""},
      {4, 1, {s}, "AAA", GQ_ASM_SHORT, 9, 0, 1, ""},
      {4, 1, {s}, "AANTCCCTGGGT", GQ_ASM_REF_N, 9, 0, 1, ""},
      {4, 2, {"AAAAAAAAA"}, "AAAAAAAA", GQ_ASM_OK, 1, 1, 1, "AAAA"},
  };
  for (int k : {2, 31, 32, 33, 62}) {
    const std::string r = k == 2 ? std::string("ACGT") : long_ref;
    cases.push_back({k, 1, {r, r}, r, GQ_ASM_OK, k == 2 ? 3 : (int)r.size() - k + 1, 1, 1, r});
  }
  int bad = 0;
  for (const Case &c : cases) bad += run(c, 1);
  for (const Case &c : cases) bad += run(c, 3);
  if (bad) fprintf(stderr, "%d expectations failed\n", bad);
  return bad ? 1 : 0;
}
