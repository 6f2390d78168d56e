// gq_hapvar_host.h — variants from assembled haplotypes on the CPU (gqpileup.h: gq_hapvar_host):
// plain C++, no device, no event cap.  The twin the device results (gq_hapvar.h) are compared with
// bit for bit, and what a stand-alone program can call (tests/native/hapvar_check.cpp).
//
// What both sides must do alike is written once here and called from the kernels too: the CIGAR
// walk with its left-normalisation (walk), the order of events (compare), an event's ALT bytes
// (write_alt), a read's two sides (sides) and a genotype's term and sum (term, add: no fused
// multiply-add, GQ_NO_CONTRACT in every body that computes).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/gqpileup.h"
#include "gq_haplik_host.h"
#include "gq_strictmath.h"

namespace gq_hapvar {

constexpr int kMaxHaps = 64;     // the carrier masks' width
constexpr int kMaxRaw = 1024;    // raw events of a window: the device sort buffer (16 bytes an event in LDS)
constexpr int kSortThreads = 256;
constexpr int kPassReads = 64;   // hv_marginal_k: reads per pass

// an event before dedup: its key, the haplotype (within the window) and where its haplotype bytes
// stand in `bases` (SNV: the ALT byte; INS: the inserted bytes; DEL: 0)
struct Raw {
  int32_t off, ref_len, alt_len;
  int32_t h;
  int64_t hp;
};

GQ_HD int kind_of(int32_t ref_len, int32_t alt_len) {
  return ref_len == 1 && alt_len == 1 ? GQ_HV_SNV : ref_len == 1 ? GQ_HV_INS : GQ_HV_DEL;
}
// haplotype bytes an event's ALT holds (after the anchor, for an insertion)
GQ_HD int32_t hap_bytes_of(int32_t ref_len, int32_t alt_len) {
  return ref_len != 1 ? 0 : alt_len == 1 ? 1 : alt_len - 1;
}

// The events of one usable haplotype: emit(off, ref_len, alt_len, haplotype offset) per event, in
// CIGAR order; *n_drop counts the indels left without an anchor.  ref: the window's bytes, hap: the
// haplotype's; the CIGAR fits both (checked by prepare).
template <class Emit>
GQ_HD void walk(const uint32_t *cigar, int32_t n_cigar, const uint8_t *ref, const uint8_t *hap, Emit &emit,
                int32_t *n_drop) {
  int32_t p = 0, q = 0, run = 0;  // window offset, haplotype offset, matched bases just before them
  for (int32_t c = 0; c < n_cigar; ++c) {
    const int32_t L = (int32_t)(cigar[c] >> 4), op = (int32_t)(cigar[c] & 15);
    if (op == 7) {
      p += L;
      q += L;
      run += L;
    } else if (op == 8) {
      for (int32_t i = 0; i < L; ++i) emit(p + i, 1, 1, q + i);
      p += L;
      q += L;
      run = 0;
    } else if (op == 1) {
      int32_t s = 0;
      while (s < run && ref[p - 1 - s] == hap[q + L - 1 - s]) ++s;
      if (p - s == 0) ++*n_drop;
      else emit(p - s - 1, 1, L + 1, q - s);
      q += L;
      run = 0;
    } else {  // 2
      int32_t s = 0;
      while (s < run && ref[p - 1 - s] == ref[p + L - 1 - s]) ++s;
      if (p - s == 0) ++*n_drop;
      else emit(p - s - 1, L + 1, 1, 0);
      p += L;
      run = 0;
    }
  }
}

// < 0, 0, > 0: the order of two events of one window; hp into bases
GQ_HD int compare(int32_t a_off, int32_t a_rl, int32_t a_al, int64_t a_hp, int32_t b_off, int32_t b_rl, int32_t b_al,
                  int64_t b_hp, const uint8_t *bases) {
  if (a_off != b_off) return a_off < b_off ? -1 : 1;
  if (a_rl != b_rl) return a_rl < b_rl ? -1 : 1;
  if (a_al != b_al) return a_al < b_al ? -1 : 1;
  const int32_t n = hap_bytes_of(a_rl, a_al);
  for (int32_t i = 0; i < n; ++i) {
    const uint8_t x = bases[a_hp + i], y = bases[b_hp + i];
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}

// an event's ALT bytes; ref: the window's bytes
GQ_HD void write_alt(uint8_t *dst, const uint8_t *ref, int32_t off, int32_t ref_len, int32_t alt_len, const uint8_t *bases,
                     int64_t hp) {
  if (ref_len == 1 && alt_len == 1) {
    dst[0] = bases[hp];
    return;
  }
  dst[0] = ref[off];
  for (int32_t i = 1; i < alt_len; ++i) dst[i] = bases[hp + i - 1];
}

// the largest of row[h] over the haplotypes of mask, 0.0 when it is empty
GQ_HD double masked_max(const double *row, uint64_t mask) {
  double m = 0.0;
  bool first = true;
  while (mask) {
    const int h = __builtin_ctzll(mask);
    mask &= mask - 1;
    const double x = row[h];
    if (first || x > m) m = x;
    first = false;
  }
  return m;
}
// a read's two sides; row: its H scaled values
GQ_HD void sides(const double *row, uint64_t carriers, uint64_t rest, double *ref, double *alt) {
  *alt = masked_max(row, carriers);
  *ref = masked_max(row, rest);
}
// one read's term of a genotype with the sides (x, y), and the sum's step
GQ_HD double term(double x, double y) {
  GQ_NO_CONTRACT
  return (gq::sm::log(x + y) - gq::sm::log(gq_haplik::init_value())) - gq::sm::log(2.0);
}
GQ_HD double add(double gl, double t) {
  GQ_NO_CONTRACT
  return gl + t;
}
// the genotype sums, best genotype and counts of one event over its window's N reads (s: the window's
// scaled, read-major over H): the twin's loop; hv_marginal_k runs the same calls, terms in parallel
GQ_HD void event_likelihoods(const double *s, int64_t N, int64_t H, uint64_t carriers, uint64_t rest, double gl[3],
                             int32_t *best, int32_t *ad_ref, int32_t *ad_alt) {
  gl[0] = gl[1] = gl[2] = 0.0;
  int32_t nr = 0, na = 0;
  for (int64_t n = 0; n < N; ++n) {
    double r, a;
    sides(s + n * H, carriers, rest, &r, &a);
    gl[0] = add(gl[0], term(r, r));
    gl[1] = add(gl[1], term(r, a));
    gl[2] = add(gl[2], term(a, a));
    nr += r > a;
    na += a > r;
  }
  *best = gq_haplik::first_largest(gl, 3);
  *ad_ref = nr;
  *ad_alt = na;
}

// ---- what both entries derive from the input before anything runs ----
struct Prepared {
  std::vector<uint8_t> hap_flags;   // [NH]
  std::vector<int64_t> cig_off;     // [NH] into in->cigar (usable haplotypes)
  std::vector<int32_t> n_cigar;     // [NH] 0 unless usable
  std::vector<uint64_t> usable;     // [W] the usable haplotypes of a window
  int64_t ref_bytes = 0, cigar_words = 0;
};

// 0 ok; else the status, with a message in msg
inline int prepare(const gq_hapvar_input *in, Prepared &P, char *msg, size_t msg_len) {
  const int64_t W = in->n_windows, NH = in->n_haplotypes, NA = in->n_align;
  auto fail = [&](int code, const char *what, long long x) {
    snprintf(msg, msg_len, what, x);
    return code;
  };
  if (W < 0 || NH < 0 || NA < 0) return fail(GQ_E_ARG, "gq_hapvar: negative count (%lld windows)", (long long)W);
  if (!in->hap_off || !in->hap_seq_off || !in->win_read_off || !in->lik_off ||
      (W > 0 && (!in->win_start || !in->ref_off || !in->win_len)) || (NH > 0 && (!in->hap_align || !in->bases)) ||
      (NA > 0 && (!in->ref_start || !in->ref_end || !in->cigar_off)))
    return fail(GQ_E_ARG, "gq_hapvar: null array (%lld windows)", (long long)W);
  if (in->hap_off[0] != 0 || in->hap_off[W] != NH || in->hap_seq_off[0] != 0)
    return fail(GQ_E_ARG, "gq_hapvar: the haplotype offsets do not fit the %lld haplotypes", (long long)NH);
  for (int64_t a = 0; a < NA; ++a)
    if (in->cigar_off[a] < 0 || in->cigar_off[a + 1] < in->cigar_off[a])
      return fail(GQ_E_ARG, "gq_hapvar: alignment %lld has a negative CIGAR length", (long long)a);
  P.cigar_words = NA > 0 ? in->cigar_off[NA] : 0;
  if (P.cigar_words > 0 && !in->cigar) return fail(GQ_E_ARG, "gq_hapvar: null CIGAR pool (%lld words)", (long long)P.cigar_words);
  for (int64_t h = 0; h < NH; ++h)
    if (in->hap_seq_off[h + 1] < in->hap_seq_off[h]) return fail(GQ_E_ARG, "gq_hapvar: haplotype %lld has a negative length", (long long)h);
  P.hap_flags.assign((size_t)NH, 0);
  P.cig_off.assign((size_t)NH, 0);
  P.n_cigar.assign((size_t)NH, 0);
  P.usable.assign((size_t)W, 0);
  for (int64_t w = 0; w < W; ++w) {
    const int64_t h0 = in->hap_off[w], h1 = in->hap_off[w + 1];
    const int64_t N = in->win_read_off[w + 1] - in->win_read_off[w];
    if (in->win_len[w] < 0 || h1 < h0 || N < 0 || in->lik_off[w] < 0 || N > INT32_MAX)
      return fail(GQ_E_ARG, "gq_hapvar: window %lld has a negative length, count or offset", (long long)w);
    if (h1 - h0 > kMaxHaps) return fail(GQ_E_CAPACITY, "gq_hapvar: window %lld has more than 64 haplotypes", (long long)w);
    if (N > 0 && h1 > h0 && !in->scaled) return fail(GQ_E_ARG, "gq_hapvar: null likelihoods (window %lld)", (long long)w);
    const bool has_ref = in->ref_off[w] >= 0;
    if (has_ref) {
      if (!in->ref_pool) return fail(GQ_E_ARG, "gq_hapvar: null reference pool (window %lld)", (long long)w);
      P.ref_bytes = std::max(P.ref_bytes, in->ref_off[w] + in->win_len[w]);
    }
    for (int64_t h = h0; h < h1; ++h) {
      const int64_t a = in->hap_align[h];
      if (a < -1 || a >= NA) return fail(GQ_E_ARG, "gq_hapvar: hap_align of haplotype %lld is out of range", (long long)h);
      if (a < 0 || !has_ref) {
        P.hap_flags[(size_t)h] = GQ_HV_HAP_UNALIGNED;
        continue;
      }
      if (in->ref_start[a] != 0 || in->ref_end[a] != in->win_len[w]) {
        P.hap_flags[(size_t)h] = GQ_HV_HAP_PARTIAL;
        continue;
      }
      const int64_t c0 = in->cigar_off[a], nc = in->cigar_off[a + 1] - c0;
      int64_t rb = 0, qb = 0;
      bool ok = nc <= INT32_MAX;
      for (int64_t c = 0; ok && c < nc; ++c) {
        const uint32_t word = in->cigar[c0 + c], op = word & 15;
        const int64_t L = word >> 4;
        ok = L >= 1 && (op == 7 || op == 8 || op == 1 || op == 2);
        if (op != 1) rb += L;
        if (op != 2) qb += L;
      }
      if (!ok || rb != in->win_len[w] || qb != in->hap_seq_off[h + 1] - in->hap_seq_off[h])
        return fail(GQ_E_ARG, "gq_hapvar: the CIGAR of haplotype %lld does not fit its window and bytes", (long long)h);
      P.cig_off[(size_t)h] = c0;
      P.n_cigar[(size_t)h] = (int32_t)nc;
      P.usable[(size_t)w] |= (uint64_t)1 << (h - h0);
    }
  }
  return 0;
}

// ---- the block: one allocation behind block_ ----
inline gq_hapvar_block *new_block(int64_t W, int64_t E, int64_t NH, int64_t n_alt) {
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  auto one = [](int64_t x) { return (size_t)(x > 0 ? x : 1); };
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += up(bytes);
    return o;
  };
  const size_t e = one(E);
  const size_t o_eo = take(8 * (one(W) + 1)), o_pos = take(8 * e), o_kind = take(e), o_rl = take(4 * e), o_ao = take(8 * e),
               o_al = take(4 * e), o_ab = take(one(n_alt)), o_car = take(8 * e), o_gl = take(24 * e), o_best = take(4 * e),
               o_adr = take(4 * e), o_ada = take(4 * e), o_dp = take(4 * e), o_ef = take(e), o_hf = take(one(NH)),
               o_wf = take(one(W));
  gq_hapvar_block *a = (gq_hapvar_block *)calloc(1, sizeof(gq_hapvar_block));
  char *b = (char *)calloc(1, at);
  if (!a || !b) {
    free(a);
    free(b);
    return nullptr;
  }
  a->n_windows = W;
  a->n_events = E;
  a->n_haplotypes = NH;
  a->n_alt_bases = n_alt;
  a->ev_off = (int64_t *)(b + o_eo);
  a->pos = (int64_t *)(b + o_pos);
  a->kind = (uint8_t *)(b + o_kind);
  a->ref_len = (int32_t *)(b + o_rl);
  a->alt_off = (int64_t *)(b + o_ao);
  a->alt_len = (int32_t *)(b + o_al);
  a->alt_bases = (uint8_t *)(b + o_ab);
  a->carriers = (uint64_t *)(b + o_car);
  a->gl = (double *)(b + o_gl);
  a->best = (int32_t *)(b + o_best);
  a->ad_ref = (int32_t *)(b + o_adr);
  a->ad_alt = (int32_t *)(b + o_ada);
  a->dp = (int32_t *)(b + o_dp);
  a->ev_flags = (uint8_t *)(b + o_ef);
  a->hap_flags = (uint8_t *)(b + o_hf);
  a->win_flags = (uint8_t *)(b + o_wf);
  a->block_ = b;
  return a;
}
inline void free_block(gq_hapvar_block *a) {
  if (!a) return;
  free(a->block_);
  free(a);
}

// ---- the twin ----
struct WindowEvents {  // a window's distinct events in order
  std::vector<Raw> ev;
  std::vector<uint64_t> carriers;
  uint8_t flags = 0;
  int64_t dropped = 0;
};

inline void window_events(const gq_hapvar_input *in, const Prepared &P, int64_t w, WindowEvents &out) {
  const int64_t h0 = in->hap_off[w], h1 = in->hap_off[w + 1];
  std::vector<Raw> raw;
  const uint8_t *ref = in->ref_off[w] >= 0 ? in->ref_pool + in->ref_off[w] : nullptr;
  for (int64_t h = h0; h < h1; ++h) {
    if (P.hap_flags[(size_t)h]) continue;
    const int64_t base = in->hap_seq_off[h];
    const int32_t local = (int32_t)(h - h0);
    auto emit = [&](int32_t off, int32_t rl, int32_t al, int32_t q) { raw.push_back(Raw{off, rl, al, local, rl == 1 ? base + q : 0}); };
    int32_t drop = 0;
    walk(in->cigar + P.cig_off[(size_t)h], P.n_cigar[(size_t)h], ref, in->bases + base, emit, &drop);
    out.dropped += drop;
  }
  if (out.dropped) out.flags |= GQ_HV_EDGE_DROPPED;
  if ((int64_t)raw.size() > kMaxRaw) {
    out.flags |= GQ_HV_TOO_MANY_EVENTS;
    return;
  }
  const uint8_t *bases = in->bases;
  std::stable_sort(raw.begin(), raw.end(), [bases](const Raw &a, const Raw &b) {
    return compare(a.off, a.ref_len, a.alt_len, a.hp, b.off, b.ref_len, b.alt_len, b.hp, bases) < 0;
  });
  for (const Raw &r : raw) {
    if (out.ev.empty() || compare(out.ev.back().off, out.ev.back().ref_len, out.ev.back().alt_len, out.ev.back().hp, r.off,
                                  r.ref_len, r.alt_len, r.hp, bases) != 0) {
      out.ev.push_back(r);
      out.carriers.push_back(0);
    }
    out.carriers.back() |= (uint64_t)1 << r.h;
  }
}

// the whole block (prepare passed); null: out of memory
inline gq_hapvar_block *run_host(const gq_hapvar_input *in, const Prepared &P, int threads) {
  const int64_t W = in->n_windows, NH = in->n_haplotypes;
  std::vector<WindowEvents> we((size_t)W);
  auto over_windows = [&](auto &&body) {
    const int T = (int)(threads < 1 ? 1 : (int64_t)threads > W ? (W > 0 ? W : 1) : threads);
    auto work = [&](int64_t a, int64_t step) {
      for (int64_t w = a; w < W; w += step) body(w);
    };
    if (T <= 1) {
      work(0, 1);
    } else {
      std::vector<std::thread> pool;
      for (int k = 0; k < T; ++k) pool.emplace_back(work, (int64_t)k, (int64_t)T);
      for (auto &k : pool) k.join();
    }
  };
  over_windows([&](int64_t w) { window_events(in, P, w, we[(size_t)w]); });
  int64_t E = 0, n_alt = 0, dropped = 0;
  std::vector<int64_t> ev_off((size_t)W + 1), alt_at((size_t)W + 1);
  for (int64_t w = 0; w < W; ++w) {
    ev_off[(size_t)w] = E;
    alt_at[(size_t)w] = n_alt;
    E += (int64_t)we[(size_t)w].ev.size();
    for (const Raw &r : we[(size_t)w].ev) n_alt += r.alt_len;
    dropped += we[(size_t)w].dropped;
  }
  ev_off[(size_t)W] = E;
  gq_hapvar_block *b = new_block(W, E, NH, n_alt);
  if (!b) return nullptr;
  memcpy(b->ev_off, ev_off.data(), 8 * ((size_t)W + 1));
  if (NH > 0) memcpy(b->hap_flags, P.hap_flags.data(), (size_t)NH);
  b->n_edge_dropped = dropped;
  over_windows([&](int64_t w) {
    const WindowEvents &x = we[(size_t)w];
    b->win_flags[w] = x.flags;
    const int64_t N = in->win_read_off[w + 1] - in->win_read_off[w], H = in->hap_off[w + 1] - in->hap_off[w];
    const uint8_t *ref = in->ref_off[w] >= 0 ? in->ref_pool + in->ref_off[w] : nullptr;
    int64_t alt = alt_at[(size_t)w];
    for (size_t i = 0; i < x.ev.size(); ++i) {
      const int64_t e = ev_off[(size_t)w] + (int64_t)i;
      const Raw &r = x.ev[i];
      b->pos[e] = (int64_t)in->win_start[w] + r.off;
      b->kind[e] = (uint8_t)kind_of(r.ref_len, r.alt_len);
      b->ref_len[e] = r.ref_len;
      b->alt_off[e] = alt;
      b->alt_len[e] = r.alt_len;
      write_alt(b->alt_bases + alt, ref, r.off, r.ref_len, r.alt_len, in->bases, r.hp);
      alt += r.alt_len;
      b->carriers[e] = x.carriers[i];
      const uint64_t rest = P.usable[(size_t)w] & ~x.carriers[i];
      b->ev_flags[e] = rest ? 0 : GQ_HV_NO_REF_SIDE;
      event_likelihoods(in->scaled ? in->scaled + in->lik_off[w] : nullptr, N, H, x.carriers[i], rest, b->gl + 3 * e, b->best + e, b->ad_ref + e,
                        b->ad_alt + e);
      b->dp[e] = (int32_t)N;
    }
  });
  return b;
}

}  // namespace gq_hapvar
