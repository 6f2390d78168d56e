// The host haplotype-likelihood twin (guacamole_amd/csrc/gq_haplik_host.h, the bodies of
// gq_haplik_host and gq_haplik_genotypes_host) as a stand-alone program over the edge cases, for a
// sanitizer build:
//   g++ -std=c++17 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all haplik_check.cpp
// Prints one line per pair: scaled log_likelihood flags, then the genotypes.  Exit 0 when every
// expectation below holds.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../guacamole_amd/csrc/gq_haplik_host.h"

namespace {

struct Case {
  std::string seq, qual, hap;  // qual: one byte a base
};

int wrong = 0;
void expect(bool ok, const char *what) {
  if (!ok) {
    fprintf(stderr, "failed: %s\n", what);
    ++wrong;
  }
}

}  // namespace

int main() {
  const std::string hap = "ACGTTGCAAGGCTTACGATCGGATTACAGGCATCGA";
  const std::string read = hap.substr(5, 20);
  std::string one_off = read;
  one_off[9] = one_off[9] == 'A' ? 'C' : 'A';
  const std::string hap_del = hap.substr(0, 15) + hap.substr(18);  // three bases gone
  const std::string read_del = hap_del.substr(5, 20);
  auto q = [](size_t n, int v) { return std::string(n, (char)v); };
  std::vector<Case> cases = {
      {read, q(20, 30), hap},             // 0
      {one_off, q(20, 30), hap},          // 1
      {read_del, q(20, 30), hap},         // 2
      {read_del, q(20, 30), hap_del},     // 3
      {"", "", hap},                      // 4 EMPTY
      {read, q(20, 30), ""},              // 5 EMPTY
      {"A", q(1, 0), "A"},                // 6 floored quality
      {"A", q(1, 93), "C"},               // 7
      {std::string(700, 'A'), q(700, 60), std::string(90, 'C')},  // 8 past the device caps
      {hap + hap, q(2 * hap.size(), 40), "ACG"},                  // 9 S > R
  };
  std::vector<uint8_t> seq_pool, qual_pool, hap_pool;
  std::vector<int64_t> seq_off, hap_off;
  std::vector<int32_t> seq_len, hap_len;
  for (const Case &c : cases) {
    seq_off.push_back((int64_t)seq_pool.size());
    hap_off.push_back((int64_t)hap_pool.size());
    seq_len.push_back((int32_t)c.seq.size());
    hap_len.push_back((int32_t)c.hap.size());
    seq_pool.insert(seq_pool.end(), c.seq.begin(), c.seq.end());
    qual_pool.insert(qual_pool.end(), c.qual.begin(), c.qual.end());
    hap_pool.insert(hap_pool.end(), c.hap.begin(), c.hap.end());
  }
  // exact-size heap copies, so that a read past a pool's end is caught
  std::vector<uint8_t> sp(seq_pool), qp(qual_pool), hp(hap_pool);
  sp.shrink_to_fit();
  qp.shrink_to_fit();
  hp.shrink_to_fit();
  gq_haplik_params p;
  gq_haplik::default_params(&p);
  expect(gq_haplik::valid(p), "default parameters are valid");
  gq_haplik_params bad = p;
  bad.open_gap_probability = 0.5;
  expect(!gq_haplik::valid(bad), "open gap 0.5 is invalid");
  bad = p;
  bad.quality_floor = 6.5;
  expect(!gq_haplik::valid(bad), "a fractional quality floor is invalid");
  std::vector<double> t(gq_haplik::kTableDoubles);
  gq_haplik::flat_tables(p, t.data());
  expect(t[gq_haplik::kMatchAt + 0] == t[gq_haplik::kMatchAt + 6], "qualities below the floor are floored");
  const int64_t n = (int64_t)cases.size();
  expect(gq_haplik::bad_pair(n, seq_off.data(), seq_len.data(), hap_off.data(), hap_len.data()) < 0, "pairs are sane");
  gq_haplik_pairs *a = gq_haplik::new_pairs(n), *b = gq_haplik::new_pairs(n), *c = gq_haplik::new_pairs(n);
  if (!a || !b || !c) return 2;
  gq_haplik::forward_host(n, sp.data(), seq_off.data(), seq_len.data(), qp.data(), hp.data(), hap_off.data(), hap_len.data(),
                          t.data(), 1, a);
  gq_haplik::forward_host(n, sp.data(), seq_off.data(), seq_len.data(), qp.data(), hp.data(), hap_off.data(), hap_len.data(),
                          t.data(), 4, b);
  gq_haplik::forward_host(n, sp.data(), seq_off.data(), seq_len.data(), nullptr, hp.data(), hap_off.data(), hap_len.data(),
                          t.data(), 3, c);
  for (int64_t i = 0; i < n; ++i) printf("%a %.17g %d\n", a->scaled[i], a->log_likelihood[i], (int)a->flags[i]);
  expect(memcmp(a->scaled, b->scaled, 8 * (size_t)n) == 0 && memcmp(a->flags, b->flags, (size_t)n) == 0 &&
             memcmp(a->log_likelihood, b->log_likelihood, 8 * (size_t)n) == 0,
         "four threads give one thread's bits");
  expect(a->scaled[0] > a->scaled[1], "a read equal to the haplotype beats the read with one base changed");
  expect(a->scaled[3] > a->scaled[2], "a read with a deletion prefers the haplotype that carries it");
  expect(a->flags[4] == GQ_HL_EMPTY && a->flags[5] == GQ_HL_EMPTY && a->scaled[4] == 0.0 && a->scaled[5] == 0.0,
         "empty pairs");
  expect(std::isinf(a->log_likelihood[4]) && a->log_likelihood[4] < 0, "an empty pair is -infinity");
  expect(a->flags[0] == 0 && a->log_likelihood[0] < 0 && std::isfinite(a->log_likelihood[0]), "a plain pair");
  // with the default gap probabilities a run of insertions costs e^-1 a base, far less than q 60
  // mismatches: no underflow at 700 bases.  With close_gap_probability 0.999 both ways underflow.
  expect(a->flags[8] == 0 && std::isfinite(a->log_likelihood[8]), "700 mismatches at q 60: insertions, no underflow");
  gq_haplik_params steep = p;
  steep.close_gap_probability = 0.999;
  expect(gq_haplik::valid(steep), "close gap 0.999 is valid");
  std::vector<double> ts(gq_haplik::kTableDoubles);
  gq_haplik::flat_tables(steep, ts.data());
  gq_haplik_pairs *u = gq_haplik::new_pairs(n);
  if (!u) return 2;
  gq_haplik::forward_host(n, sp.data(), seq_off.data(), seq_len.data(), qp.data(), hp.data(), hap_off.data(), hap_len.data(),
                          ts.data(), 2, u);
  expect(u->flags[8] == GQ_HL_UNDERFLOW && std::isinf(u->log_likelihood[8]) && u->log_likelihood[8] < 0 &&
             u->scaled[8] < DBL_MIN,
         "700 mismatches at q 60 underflow when a gap is dear");
  expect(u->flags[0] == 0, "and the plain pair does not");
  gq_haplik::free_pairs(u);
  expect(c->flags[0] == 0 && c->scaled[0] != a->scaled[0], "no qualities: the mismatch probability is used");
  for (int64_t i = 0; i < n; ++i)
    if (hap_len[i] > 0)
      expect(a->scaled[i] <= gq_haplik::init_value() * (hap_len[i] + 1) / hap_len[i], "scaled is bounded");

  // genotypes: window 0 = reads {0, 1} x haplotypes {hap, hap_del} from fresh pairs; window 1 no reads;
  // window 2 no haplotypes; window 3 one haplotype
  const std::vector<std::string> haps = {hap, hap_del, hap};
  const std::vector<std::string> reads = {read, read_del, read};
  std::vector<uint8_t> rp, rq, gp;
  std::vector<int64_t> ro, go;
  std::vector<int32_t> rl, gl;
  auto pair = [&](const std::string &r, const std::string &h) {
    ro.push_back((int64_t)rp.size());
    go.push_back((int64_t)gp.size());
    rl.push_back((int32_t)r.size());
    gl.push_back((int32_t)h.size());
    rp.insert(rp.end(), r.begin(), r.end());
    rq.insert(rq.end(), r.size(), (uint8_t)30);
    gp.insert(gp.end(), h.begin(), h.end());
  };
  for (int r = 0; r < 2; ++r)
    for (int h = 0; h < 2; ++h) pair(reads[(size_t)r], haps[(size_t)h]);
  pair(reads[2], haps[2]);
  const int64_t np = (int64_t)rl.size();
  gq_haplik_pairs *g = gq_haplik::new_pairs(np);
  if (!g) return 2;
  gq_haplik::forward_host(np, rp.data(), ro.data(), rl.data(), rq.data(), gp.data(), go.data(), gl.data(), t.data(), 2, g);
  const int64_t W = 4;
  const int64_t win_read_off[W + 1] = {0, 2, 2, 3, 4}, win_hap_off[W + 1] = {0, 2, 3, 3, 4},
                lik_off[W + 1] = {0, 4, 4, 4, 5};
  int64_t gt_off[W + 1];
  const int64_t G = gq_haplik::genotype_offsets(W, win_read_off, win_hap_off, gt_off);
  expect(G == 4 && gt_off[1] == 3 && gt_off[2] == 3 && gt_off[3] == 3, "genotype offsets");
  std::vector<double> gt((size_t)G);
  gt.shrink_to_fit();
  int32_t best[W];
  gq_haplik::genotypes_host(W, win_read_off, win_hap_off, lik_off, g->scaled, gt_off, gt.data(), best);
  for (double x : gt) printf("%.17g\n", x);
  expect(best[0] == 1 && best[1] == -1 && best[2] == -1 && best[3] == 0, "a read of each haplotype: the mixed genotype");
  int64_t i, j;
  gq_haplik::genotype_pair(3, 4, &i, &j);
  expect(i == 1 && j == 2, "genotype 4 of three haplotypes is (1, 2)");
  gq_haplik::free_pairs(a);
  gq_haplik::free_pairs(b);
  gq_haplik::free_pairs(c);
  gq_haplik::free_pairs(g);
  gq_haplik_block *blk = gq_haplik::new_block(W, 4, np, G);
  if (!blk) return 2;
  blk->best_genotype[W - 1] = 0;
  blk->win_read_off[W] = 4;
  gq_haplik::free_block(blk);
  return wrong ? 1 : 0;
}
