// gq_align_host.h — affine-gap alignment on the CPU (gqpileup.h: gq_align_host): plain C++, no
// device.  The twin the device results (gq_align.h: align_k) are compared with bit for bit, and
// what a stand-alone program can call (tests/native/align_check.cpp).
//
// The recurrence restates AffineGapPenaltyAlignment.scoreAlignmentPaths / align (alignment/
// AffineGapPenaltyAlignment.scala:20-141).  It is not a three-matrix Gotoh aligner: each cell
// keeps one path (score and last state), and the next step's cost depends on that last state.
// Every step cost is one entry of a 32-entry table (penalty_table) whose terms are added in the
// reference's order, so a cell is one FP64 add and one compare per candidate here and on the device.
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/gqpileup.h"

namespace gq_align {

// last state of a path, next state of a step, BAM op of a next state
enum : int { kLastNone = 0, kLastIns = 1, kLastDel = 2, kLastDiag = 3 };
enum : int { kIns = 0, kDel = 1, kMatch = 2, kMismatch = 3 };
constexpr uint32_t kBamOp[4] = {1, 2, 7, 8};  // I D = X

constexpr int kMaxS = 512, kMaxR = 4096;  // device caps (align_k)

inline bool valid(const gq_align_params &p) {
  const double v[3] = {p.mismatch_probability, p.open_gap_probability, p.close_gap_probability};
  for (double x : v)
    if (!(x > 0.0 && x < 1.0)) return false;
  return true;
}

// transitionPenalty (AffineGapPenaltyAlignment.scala:73-84), the four terms added left to right;
// an absent term is the reference's literal 0
inline void penalty_table(const gq_align_params &p, double t[32]) {
  const double mismatch = -std::log(p.mismatch_probability);
  const double open = -std::log(p.open_gap_probability);
  const double no_gap = -std::log(1 - p.open_gap_probability);
  const double close = -std::log(p.close_gap_probability);
  const double cont = -std::log(1 - p.close_gap_probability);
  for (int end = 0; end < 2; ++end)
    for (int last = 0; last < 4; ++last)
      for (int next = 0; next < 4; ++next) {
        const bool next_gap = next == kIns || next == kDel;
        const bool last_gap = last == kLastIns || last == kLastDel;
        // Match and Mismatch are different states of the reference, but neither is a gap, so
        // whether one follows the other changes no term
        const bool same = (last == kLastIns && next == kIns) || (last == kLastDel && next == kDel);
        const bool open_gap = !same && next_gap;
        const bool close_gap = last_gap && !same;
        const bool continue_gap = same && next_gap;
        const double a = open_gap ? open : 0.0;
        const double b = close_gap ? close : 0.0;
        const double c = continue_gap ? cont : (next == kMismatch ? no_gap + mismatch : no_gap);
        const double d = (end && next_gap) ? close : 0.0;
        t[16 * end + 4 * last + next] = ((a + b) + c) + d;
      }
}

inline int32_t double_to_int(double x) {  // Double.toInt
  if (x != x) return 0;
  if (x >= 2147483647.0) return INT32_MAX;
  if (x <= -2147483648.0) return INT32_MIN;
  return (int32_t)x;
}

struct One {
  int32_t ref_start = 0, ref_end = 0;
  double score = 0.0;
};

// one pair; its CIGAR words are appended to `cigar`.  tb: scratch of the caller (2 bits a cell would
// do; a byte a cell keeps this twin plain)
inline One align_one(const uint8_t *seq, int32_t S, const uint8_t *ref, int32_t R, const double *t,
                     std::vector<uint8_t> &tb, std::vector<double> &sc, std::vector<uint8_t> &st,
                     std::vector<uint32_t> &cigar) {
  One o;
  if (S <= 0) return o;
  const size_t W = (size_t)R + 1;
  tb.assign((size_t)S * W, 0);
  sc.assign(W, 0.0);
  st.assign(W, (uint8_t)kLastNone);
  for (int32_t s = 1; s <= S; ++s) {
    const double *row = t + (s == S ? 16 : 0);
    uint8_t *tr = tb.data() + (size_t)(s - 1) * W;
    double dg_sc = 0.0;  // cell (s - 1, r - 1)
    int dg_st = 0;
    for (int32_t r = 0; r <= R; ++r) {
      const double up_sc = sc[(size_t)r];
      const int up_st = st[(size_t)r];
      double best = up_sc + row[4 * up_st + kIns];
      int next = kIns;
      if (r > 0) {
        const double d = sc[(size_t)r - 1] + row[4 * st[(size_t)r - 1] + kDel];  // (s, r - 1): this row
        if (d < best) best = d, next = kDel;
        const int m = seq[s - 1] == ref[r - 1] ? kMatch : kMismatch;
        const double g = dg_sc + row[4 * dg_st + m];
        if (g < best) best = g, next = m;
      }
      dg_sc = up_sc;
      dg_st = up_st;
      sc[(size_t)r] = best;
      st[(size_t)r] = (uint8_t)(next < kMatch ? next + 1 : kLastDiag);
      tr[r] = (uint8_t)next;
    }
  }
  int32_t end = 0;
  for (int32_t r = 1; r <= R; ++r)
    if (sc[(size_t)r] < sc[(size_t)end]) end = r;
  o.ref_end = end;
  o.score = sc[(size_t)end];
  // the path backwards, its runs appended in reverse and turned round after
  const size_t first = cigar.size();
  int32_t s = S, r = end, run = 0, op = -1;
  while (s > 0) {
    const int next = tb[(size_t)(s - 1) * W + (size_t)r];
    if (next != op) {
      if (run) cigar.push_back((uint32_t)run << 4 | kBamOp[op]);
      op = next;
      run = 0;
    }
    ++run;
    if (next != kDel) --s;
    if (next != kIns) --r;
  }
  if (run) cigar.push_back((uint32_t)run << 4 | kBamOp[op]);
  for (size_t a = first, b = cigar.size(); a + 1 < b; ++a, --b) {
    const uint32_t x = cigar[a];
    cigar[a] = cigar[b - 1];
    cigar[b - 1] = x;
  }
  o.ref_start = r;
  return o;
}

// the result block: one allocation behind block_, the arrays laid out in it
inline gq_alignments *new_block(int64_t n, int64_t n_cigar) {
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const size_t m = (size_t)(n > 0 ? n : 1), mc = (size_t)(n_cigar > 0 ? n_cigar : 1);
  const size_t o_start = 0, o_end = o_start + up(4 * m), o_score = o_end + up(4 * m), o_int = o_score + up(8 * m),
               o_off = o_int + up(4 * m), o_cig = o_off + up(8 * (m + 1)), total = o_cig + up(4 * mc);
  gq_alignments *a = (gq_alignments *)calloc(1, sizeof(gq_alignments));
  char *b = (char *)calloc(1, total);
  if (!a || !b) {
    free(a);
    free(b);
    return nullptr;
  }
  a->n = n;
  a->ref_start = (int32_t *)(b + o_start);
  a->ref_end = (int32_t *)(b + o_end);
  a->score = (double *)(b + o_score);
  a->score_int = (int32_t *)(b + o_int);
  a->cigar_off = (int64_t *)(b + o_off);
  a->cigar = (uint32_t *)(b + o_cig);
  a->block_ = b;
  return a;
}

// 0 ok, 1 out of memory, 2 a bad pair (bad_pair names it)
inline int align_host(int64_t n, const uint8_t *seq_pool, const int64_t *seq_off, const int32_t *seq_len,
                      const uint8_t *ref_pool, const int64_t *ref_off, const int32_t *ref_len, const double *table,
                      gq_alignments **out, int64_t *bad_pair) {
  for (int64_t i = 0; i < n; ++i)
    if (seq_len[i] < 0 || ref_len[i] < 0 || seq_off[i] < 0 || ref_off[i] < 0) {
      *bad_pair = i;
      return 2;
    }
  std::vector<One> res((size_t)n);
  std::vector<int64_t> off((size_t)n + 1, 0);
  std::vector<uint32_t> cigar;
  std::vector<uint8_t> tb, st;
  std::vector<double> sc;
  for (int64_t i = 0; i < n; ++i) {
    res[(size_t)i] = align_one(seq_pool + seq_off[i], seq_len[i], ref_pool + ref_off[i], ref_len[i], table, tb, sc, st,
                               cigar);
    off[(size_t)i + 1] = (int64_t)cigar.size();
  }
  gq_alignments *a = new_block(n, (int64_t)cigar.size());
  if (!a) return 1;
  for (int64_t i = 0; i < n; ++i) {
    a->ref_start[i] = res[(size_t)i].ref_start;
    a->ref_end[i] = res[(size_t)i].ref_end;
    a->score[i] = res[(size_t)i].score;
    a->score_int[i] = double_to_int(res[(size_t)i].score);
  }
  memcpy(a->cigar_off, off.data(), sizeof(int64_t) * ((size_t)n + 1));
  if (!cigar.empty()) memcpy(a->cigar, cigar.data(), sizeof(uint32_t) * cigar.size());
  *out = a;
  return 0;
}

inline void free_block(gq_alignments *a) {
  if (!a) return;
  free(a->block_);
  free(a);
}

}  // namespace gq_align
