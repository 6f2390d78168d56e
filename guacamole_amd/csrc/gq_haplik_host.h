// gq_haplik_host.h — haplotype likelihoods on the CPU (gqpileup.h: gq_haplik_host,
// gq_haplik_genotypes_host): plain C++, no device, no caps.  The twin the device results
// (gq_haplik.h: hap_forward_k, hap_genotype_k) are compared with bit for bit, and what a stand-alone
// program can call (tests/native/haplik_check.cpp).
//
// The model is gqpileup.h's "Haplotype likelihoods": a pair-HMM forward pass of a read against a
// haplotype, three FP64 values M I D a cell, every product and sum rounded on its own in the written
// order (no fused multiply-add: GQ_NO_CONTRACT in every body that computes), then the diploid
// formula of Likelihood.likelihoodsOfGenotypes (likelihood/Likelihood.scala) over reads.  What both
// sides must compute alike beyond the recurrence (the tables, a pair's result from its sum, a
// genotype's sum) is written once here and called from the kernels too.
#pragma once
#include <stdint.h>

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/gqpileup.h"
#include "gq_strictmath.h"

namespace gq_haplik {

// the transition table's entries (gq_haplik_tables: trans[8])
enum : int { kTMM = 0, kTMI = 1, kTMD = 2, kTII = 3, kTDD = 4, kTIM = 5, kTDM = 6 };
// the tables as one array, for the device: trans, match, mismatch, then the two priors of a read
// without qualities
constexpr int kMatchAt = 8, kMismatchAt = 8 + 256, kNoQualAt = 8 + 512, kTableDoubles = 8 + 512 + 2;

constexpr int kMaxS = 512, kMaxR = 4096;  // device caps (hap_forward_k): the aligner's

inline void default_params(gq_haplik_params *p) {
  memset(p, 0, sizeof(*p));
  p->mismatch_probability = std::exp(-4.0);
  p->open_gap_probability = std::exp(-6.0);
  p->close_gap_probability = 1 - std::exp(-1.0);
  p->quality_floor = 6.0;
}

inline bool valid(const gq_haplik_params &p) {
  const double v[3] = {p.mismatch_probability, p.open_gap_probability, p.close_gap_probability};
  for (double x : v)
    if (!(x > 0.0 && x < 1.0)) return false;
  if (!(p.open_gap_probability < 0.5)) return false;
  return p.quality_floor >= 0.0 && p.quality_floor <= 255.0 && p.quality_floor == (double)(int)p.quality_floor;
}

// trans, match[q] and mismatch[q] for a raw quality byte q (the floor is in the tables), and the two
// priors of a base without a quality
inline void tables(const gq_haplik_params &p, double trans[8], double match[256], double mismatch[256],
                   double no_qual[2]) {
  GQ_NO_CONTRACT
  const double open = p.open_gap_probability;
  const double ext = 1 - p.close_gap_probability;
  trans[kTMM] = 1 - (open + open);
  trans[kTMI] = open;
  trans[kTMD] = open;
  trans[kTII] = ext;
  trans[kTDD] = ext;
  trans[kTIM] = 1 - ext;
  trans[kTDM] = 1 - ext;
  trans[7] = 0.0;
  const int floor_ = (int)p.quality_floor;
  for (int q = 0; q < 256; ++q) {
    const int qe = q < floor_ ? floor_ : q;  // (q <= 255: a byte)
    // PhredUtils.phredToSuccessProbability as the engine's table has it (gq_somatic.hip: g_succ)
    const double succ = 1.0 - std::pow(10.0, -qe / 10.0);
    match[q] = succ;
    mismatch[q] = (1 - succ) / 3.0;
  }
  if (no_qual) {
    no_qual[0] = 1 - p.mismatch_probability;
    no_qual[1] = p.mismatch_probability / 3.0;
  }
}

inline void flat_tables(const gq_haplik_params &p, double t[kTableDoubles]) {
  tables(p, t, t + kMatchAt, t + kMismatchAt, t + kNoQualAt);
}

GQ_HD double init_value() { return __builtin_ldexp(1.0, 1000); }

// a pair's result from the sum over row S
GQ_HD void finish(double sum, double *scaled, double *log_likelihood, uint8_t *flags) {
  GQ_NO_CONTRACT
  *scaled = sum;
  if (sum < DBL_MIN) {  // zero or subnormal
    *log_likelihood = -__builtin_inf();
    *flags = GQ_HL_UNDERFLOW;
  } else {
    *log_likelihood = gq::sm::log(sum) - gq::sm::log(init_value());
    *flags = 0;
  }
}
GQ_HD void finish_empty(double *scaled, double *log_likelihood, uint8_t *flags) {
  *scaled = 0.0;
  *log_likelihood = -__builtin_inf();
  *flags = GQ_HL_EMPTY;
}

// genotype (i, j) of a window with H haplotypes over its N reads; s: the window's scaled[n * H + h]
GQ_HD double genotype_ll(const double *s, int64_t N, int64_t H, int64_t i, int64_t j) {
  GQ_NO_CONTRACT
  const double log_init = gq::sm::log(init_value()), log_two = gq::sm::log(2.0);
  double gl = 0.0;
  for (int64_t n = 0; n < N; ++n) gl = gl + ((gq::sm::log(s[n * H + i] + s[n * H + j]) - log_init) - log_two);
  return gl;
}
GQ_HD int64_t genotypes_of(int64_t N, int64_t H) { return N > 0 && H > 0 ? H * (H + 1) / 2 : 0; }
// (i, j) of a window's genotype `local`, i-major over i <= j
GQ_HD void genotype_pair(int64_t H, int64_t local, int64_t *i, int64_t *j) {
  int64_t a = 0;
  while (local >= H - a) {
    local -= H - a;
    ++a;
  }
  *i = a;
  *j = a + local;
}
// the first largest of g[0, n), -1 when n == 0
GQ_HD int32_t first_largest(const double *g, int64_t n) {
  int32_t best = -1;
  for (int64_t x = 0; x < n; ++x)
    if (best < 0 || g[x] > g[best]) best = (int32_t)x;
  return best;
}

// one pair on the CPU; qual == nullptr: the read has no qualities.  m, i, d: scratch of the caller
inline void forward_one(const uint8_t *seq, const uint8_t *qual, int32_t S, const uint8_t *hap, int32_t R,
                        const double *t, std::vector<double> &m, std::vector<double> &i, std::vector<double> &d,
                        double *scaled, double *log_likelihood, uint8_t *flags) {
  GQ_NO_CONTRACT
  if (S <= 0 || R <= 0) {
    finish_empty(scaled, log_likelihood, flags);
    return;
  }
  const double tMM = t[kTMM], tMI = t[kTMI], tMD = t[kTMD], tII = t[kTII], tDD = t[kTDD], tIM = t[kTIM], tDM = t[kTDM];
  const size_t W = (size_t)R + 1;
  m.assign(2 * W, 0.0);
  i.assign(2 * W, 0.0);
  d.assign(2 * W, 0.0);
  const double d0 = init_value() / (double)R;
  for (size_t r = 0; r < W; ++r) d[r] = d0;
  for (int32_t s = 1; s <= S; ++s) {
    const double *pm = m.data() + (size_t)((s - 1) & 1) * W, *pi = i.data() + (size_t)((s - 1) & 1) * W,
                 *pd = d.data() + (size_t)((s - 1) & 1) * W;
    double *cm = m.data() + (size_t)(s & 1) * W, *ci = i.data() + (size_t)(s & 1) * W, *cd = d.data() + (size_t)(s & 1) * W;
    const double e_match = qual ? t[kMatchAt + qual[s - 1]] : t[kNoQualAt];
    const double e_mismatch = qual ? t[kMismatchAt + qual[s - 1]] : t[kNoQualAt + 1];
    const uint8_t b = seq[s - 1];
    cm[0] = 0.0;
    cd[0] = 0.0;
    ci[0] = pm[0] * tMI + pi[0] * tII;
    for (int32_t r = 1; r <= R; ++r) {
      const double prior = b == hap[r - 1] ? e_match : e_mismatch;
      cm[r] = prior * ((pm[r - 1] * tMM + pi[r - 1] * tIM) + pd[r - 1] * tDM);
      ci[r] = pm[r] * tMI + pi[r] * tII;
      cd[r] = cm[r - 1] * tMD + cd[r - 1] * tDD;
    }
  }
  const double *lm = m.data() + (size_t)(S & 1) * W, *li = i.data() + (size_t)(S & 1) * W;
  double sum = 0.0;
  for (int32_t r = 1; r <= R; ++r) sum = sum + (lm[r] + li[r]);
  finish(sum, scaled, log_likelihood, flags);
}

// the pairs block: one allocation behind block_
inline gq_haplik_pairs *new_pairs(int64_t n) {
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const size_t m = (size_t)(n > 0 ? n : 1);
  const size_t o_sc = 0, o_ll = o_sc + up(8 * m), o_fl = o_ll + up(8 * m), total = o_fl + up(m);
  gq_haplik_pairs *a = (gq_haplik_pairs *)calloc(1, sizeof(gq_haplik_pairs));
  char *b = (char *)calloc(1, total);
  if (!a || !b) {
    free(a);
    free(b);
    return nullptr;
  }
  a->n = n;
  a->scaled = (double *)(b + o_sc);
  a->log_likelihood = (double *)(b + o_ll);
  a->flags = (uint8_t *)(b + o_fl);
  a->block_ = b;
  return a;
}
inline void free_pairs(gq_haplik_pairs *a) {
  if (!a) return;
  free(a->block_);
  free(a);
}

// -1 ok, else the first pair with a negative offset or length
inline int64_t bad_pair(int64_t n, const int64_t *seq_off, const int32_t *seq_len, const int64_t *hap_off,
                        const int32_t *hap_len) {
  for (int64_t p = 0; p < n; ++p)
    if (seq_len[p] < 0 || hap_len[p] < 0 || seq_off[p] < 0 || hap_off[p] < 0) return p;
  return -1;
}

// the pairs into a block of new_pairs(n), `threads` workers over them (<= 1: the calling thread)
inline void forward_host(int64_t n, const uint8_t *seq_pool, const int64_t *seq_off, const int32_t *seq_len,
                         const uint8_t *qual_pool, const uint8_t *hap_pool, const int64_t *hap_off,
                         const int32_t *hap_len, const double *t, int threads, gq_haplik_pairs *out) {
  auto work = [&](int64_t a, int64_t step) {
    std::vector<double> m, i, d;
    for (int64_t p = a; p < n; p += step)
      forward_one(seq_pool + seq_off[p], qual_pool ? qual_pool + seq_off[p] : nullptr, seq_len[p], hap_pool + hap_off[p],
                  hap_len[p], t, m, i, d, out->scaled + p, out->log_likelihood + p, out->flags + p);
  };
  const int T = (int)(threads < 1 ? 1 : (int64_t)threads > n ? (n > 0 ? n : 1) : threads);
  if (T <= 1) {
    work(0, 1);
  } else {
    std::vector<std::thread> pool;
    for (int k = 0; k < T; ++k) pool.emplace_back(work, (int64_t)k, (int64_t)T);
    for (auto &k : pool) k.join();
  }
}

// gt_off[W + 1] from the windows' reads and haplotypes; returns the genotypes in all
inline int64_t genotype_offsets(int64_t W, const int64_t *win_read_off, const int64_t *hap_off, int64_t *gt_off) {
  int64_t at = 0;
  for (int64_t w = 0; w < W; ++w) {
    gt_off[w] = at;
    at += genotypes_of(win_read_off[w + 1] - win_read_off[w], hap_off[w + 1] - hap_off[w]);
  }
  gt_off[W] = at;
  return at;
}

inline void genotypes_host(int64_t W, const int64_t *win_read_off, const int64_t *hap_off, const int64_t *lik_off,
                           const double *scaled, const int64_t *gt_off, double *gt_log_likelihood,
                           int32_t *best_genotype) {
  for (int64_t w = 0; w < W; ++w) {
    const int64_t N = win_read_off[w + 1] - win_read_off[w], H = hap_off[w + 1] - hap_off[w];
    const int64_t G = gt_off[w + 1] - gt_off[w];
    for (int64_t g = 0; g < G; ++g) {
      int64_t i, j;
      genotype_pair(H, g, &i, &j);
      gt_log_likelihood[gt_off[w] + g] = genotype_ll(scaled + lik_off[w], N, H, i, j);
    }
    best_genotype[w] = first_largest(gt_log_likelihood + gt_off[w], G);
  }
}

// the windows block: one allocation behind block_
inline gq_haplik_block *new_block(int64_t W, int64_t n_reads, int64_t n_pairs, int64_t n_gt) {
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  auto one = [](int64_t x) { return (size_t)(x > 0 ? x : 1); };
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += up(bytes);
    return o;
  };
  const size_t o_ro = take(8 * (one(W) + 1)), o_rd = take(8 * one(n_reads)), o_lo = take(8 * (one(W) + 1)),
               o_sc = take(8 * one(n_pairs)), o_ll = take(8 * one(n_pairs)), o_fl = take(one(n_pairs)),
               o_go = take(8 * (one(W) + 1)), o_gl = take(8 * one(n_gt)), o_bg = take(4 * one(W));
  gq_haplik_block *a = (gq_haplik_block *)calloc(1, sizeof(gq_haplik_block));
  char *b = (char *)calloc(1, at);
  if (!a || !b) {
    free(a);
    free(b);
    return nullptr;
  }
  a->n_windows = W;
  a->n_reads = n_reads;
  a->n_pairs = n_pairs;
  a->n_genotypes = n_gt;
  a->win_read_off = (int64_t *)(b + o_ro);
  a->win_reads = (int64_t *)(b + o_rd);
  a->lik_off = (int64_t *)(b + o_lo);
  a->scaled = (double *)(b + o_sc);
  a->log_likelihood = (double *)(b + o_ll);
  a->flags = (uint8_t *)(b + o_fl);
  a->gt_off = (int64_t *)(b + o_go);
  a->gt_log_likelihood = (double *)(b + o_gl);
  a->best_genotype = (int32_t *)(b + o_bg);
  a->block_ = b;
  return a;
}
inline void free_block(gq_haplik_block *a) {
  if (!a) return;
  free(a->block_);
  free(a);
}

}  // namespace gq_haplik
