// gq_haplik.hip — haplotype likelihoods (gqpileup.h: gq_haplik_*): the C ABI over the host twin
// (gq_haplik_host.h) and the device kernels (gq_haplik.h).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <vector>

#include "../../include/gqpileup.h"
#include "gq_host.h"
#include "gq_winreads.h"
#include "gq_haplik_host.h"
#include "gq_haplik.h"

using namespace gq;

namespace {

struct Span {  // a device span between two events of its own
  hipEvent_t a = nullptr, b = nullptr;
  hipError_t make() {
    hipError_t e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    return e;
  }
  ~Span() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

struct Bufs {  // released when the call returns
  std::vector<DevBuf *> all;
  DevBuf *add() {
    all.push_back(new DevBuf());
    return all.back();
  }
  ~Bufs() {
    for (DevBuf *x : all) {
      x->release();
      delete x;
    }
  }
};

// a result block until it is handed out; on an early return the stream is drained first, since
// copies into the block may still be queued
struct PairsGuard {
  gq_haplik_pairs *p = nullptr;
  hipStream_t stream = nullptr;
  ~PairsGuard() {
    if (p && stream) (void)hipStreamSynchronize(stream);
    gq_haplik::free_pairs(p);
  }
};
struct BlockGuard {
  gq_haplik_block *p = nullptr;
  hipStream_t stream = nullptr;
  ~BlockGuard() {
    if (p && stream) (void)hipStreamSynchronize(stream);
    gq_haplik::free_block(p);
  }
};

gq_status tables_of(const gq_haplik_params *params, double t[gq_haplik::kTableDoubles], const char *who) {
  gq_haplik_params p;
  if (params) p = *params;
  else gq_haplik::default_params(&p);
  if (!gq_haplik::valid(p))
    return set_err(GQ_E_ARG,
                   "%s: probabilities must lie strictly inside (0, 1) and the open gap probability below 0.5: mismatch "
                   "%g, open gap %g, close gap %g; the quality floor must be a whole number in 0 .. 255: %g",
                   who, p.mismatch_probability, p.open_gap_probability, p.close_gap_probability, p.quality_floor);
  gq_haplik::flat_tables(p, t);
  return GQ_OK;
}

gq_status check_pairs(const char *who, int64_t n, const uint8_t *seq_pool, const int64_t *seq_off, const int32_t *seq_len,
                      const uint8_t *hap_pool, const int64_t *hap_off, const int32_t *hap_len, gq_haplik_pairs **out) {
  if (n < 0 || !out) return set_err(GQ_E_ARG, "%s: null or negative argument", who);
  if (n > 0 && (!seq_pool || !seq_off || !seq_len || !hap_pool || !hap_off || !hap_len))
    return set_err(GQ_E_ARG, "%s: null array", who);
  const int64_t bad = gq_haplik::bad_pair(n, seq_off, seq_len, hap_off, hap_len);
  if (bad >= 0) return set_err(GQ_E_ARG, "%s: pair %lld has a negative offset or length", who, (long long)bad);
  return GQ_OK;
}

// hap_forward_k over the n > 0 pairs of P (within the caps) into device arrays; ks spans the kernel
gq_status forward(gq_ctx *c, const hlk::Pairs &P, int64_t n, const double *d_tab, double *d_scaled, double *d_ll,
                  uint8_t *d_flags, Span &ks) {
  const int64_t blocks = (n + hlk::kWaves - 1) / hlk::kWaves;
  if (blocks >= ((int64_t)1 << 31)) return set_err(GQ_E_CAPACITY, "haplik: %lld pairs in one call", (long long)n);
  HIP_TRY(hipEventRecord(ks.a, c->stream));
  hipLaunchKernelGGL(hlk::hap_forward_k, dim3((unsigned)blocks), dim3(hlk::kLanes * hlk::kWaves), 0, c->stream, P, n, d_tab,
                     d_scaled, d_ll, d_flags);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ks.b, c->stream));
  return GQ_OK;
}

}  // namespace

extern "C" {

void gq_haplik_default_params(gq_haplik_params *out) {
  if (out) gq_haplik::default_params(out);
}

gq_status gq_haplik_tables(const gq_haplik_params *params, double trans[8], double match[256], double mismatch[256]) {
  if (!trans || !match || !mismatch) return set_err(GQ_E_ARG, "gq_haplik_tables: null table");
  double t[gq_haplik::kTableDoubles];
  gq_status s;
  if ((s = tables_of(params, t, "gq_haplik_tables"))) return s;
  memcpy(trans, t, 8 * sizeof(double));
  memcpy(match, t + gq_haplik::kMatchAt, 256 * sizeof(double));
  memcpy(mismatch, t + gq_haplik::kMismatchAt, 256 * sizeof(double));
  return GQ_OK;
}

void gq_haplik_free_pairs(gq_haplik_pairs *p) { gq_haplik::free_pairs(p); }
void gq_haplik_free_block(gq_haplik_block *b) { gq_haplik::free_block(b); }

gq_status gq_haplik_host(int64_t n, const uint8_t *seq_pool, const int64_t *seq_off, const int32_t *seq_len,
                         const uint8_t *qual_pool, const uint8_t *hap_pool, const int64_t *hap_off,
                         const int32_t *hap_len, const gq_haplik_params *params, int32_t threads,
                         gq_haplik_pairs **out) {
  gq_status s;
  if ((s = check_pairs("gq_haplik_host", n, seq_pool, seq_off, seq_len, hap_pool, hap_off, hap_len, out))) return s;
  double t[gq_haplik::kTableDoubles];
  if ((s = tables_of(params, t, "gq_haplik_host"))) return s;
  gq_haplik_pairs *res = gq_haplik::new_pairs(n);
  if (!res) return set_err(GQ_E_NOMEM, "gq_haplik_host: result block");
  gq_haplik::forward_host(n, seq_pool, seq_off, seq_len, qual_pool, hap_pool, hap_off, hap_len, t, threads, res);
  *out = res;
  return GQ_OK;
}

gq_status gq_haplik_genotypes_host(int64_t n_windows, const int64_t *win_read_off, const int64_t *hap_off,
                                   const int64_t *lik_off, const double *scaled, int64_t *gt_off,
                                   double *gt_log_likelihood, int64_t gt_capacity, int32_t *best_genotype) {
  if (n_windows < 0 || !win_read_off || !hap_off || !gt_off)
    return set_err(GQ_E_ARG, "gq_haplik_genotypes_host: null or negative argument");
  for (int64_t w = 0; w < n_windows; ++w)
    if (win_read_off[w + 1] < win_read_off[w] || hap_off[w + 1] < hap_off[w])
      return set_err(GQ_E_ARG, "gq_haplik_genotypes_host: window %lld has a negative read or haplotype count", (long long)w);
  const int64_t G = gq_haplik::genotype_offsets(n_windows, win_read_off, hap_off, gt_off);
  if (!gt_log_likelihood) return GQ_OK;
  if (!best_genotype || (n_windows > 0 && !lik_off) || (G > 0 && !scaled))
    return set_err(GQ_E_ARG, "gq_haplik_genotypes_host: null array");
  if (gt_capacity < G)
    return set_err(GQ_E_ARG, "gq_haplik_genotypes_host: room for %lld genotypes, %lld needed", (long long)gt_capacity,
                   (long long)G);
  gq_haplik::genotypes_host(n_windows, win_read_off, hap_off, lik_off, scaled, gt_off, gt_log_likelihood, best_genotype);
  return GQ_OK;
}

gq_status gq_haplik_batch(gq_ctx *c, int64_t n, const uint8_t *seq_pool, const int64_t *seq_off, const int32_t *seq_len,
                          const uint8_t *qual_pool, const uint8_t *hap_pool, const int64_t *hap_off,
                          const int32_t *hap_len, const gq_haplik_params *params, gq_haplik_pairs **out) {
  if (!c) return set_err(GQ_E_ARG, "gq_haplik_batch: null ctx");
  gq_status s;
  if ((s = check_pairs("gq_haplik_batch", n, seq_pool, seq_off, seq_len, hap_pool, hap_off, hap_len, out))) return s;
  double t[gq_haplik::kTableDoubles];
  if ((s = tables_of(params, t, "gq_haplik_batch"))) return s;
  for (int64_t i = 0; i < n; ++i) {
    if (seq_len[i] > gq_haplik::kMaxS)
      return set_err(GQ_E_CAPACITY, "haplik: pair %lld: read length %d is past the device cap of %d", (long long)i,
                     seq_len[i], gq_haplik::kMaxS);
    if (hap_len[i] > gq_haplik::kMaxR)
      return set_err(GQ_E_CAPACITY, "haplik: pair %lld: haplotype length %d is past the device cap of %d", (long long)i,
                     hap_len[i], gq_haplik::kMaxR);
  }
  PairsGuard res;
  res.p = gq_haplik::new_pairs(n);
  if (!res.p) return set_err(GQ_E_NOMEM, "gq_haplik_batch: result block");
  if (n == 0) {
    *out = res.p;
    res.p = nullptr;
    return GQ_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  res.stream = c->stream;
  int64_t seq_bytes = 0, hap_bytes = 0;
  for (int64_t i = 0; i < n; ++i) {
    seq_bytes = std::max(seq_bytes, seq_off[i] + seq_len[i]);
    hap_bytes = std::max(hap_bytes, hap_off[i] + hap_len[i]);
  }
  Span span, ks;
  HIP_TRY(span.make());
  HIP_TRY(ks.make());
  HIP_TRY(hipEventRecord(span.a, c->stream));
  Bufs bufs;
  DevBuf *d_seq = bufs.add(), *d_qual = bufs.add(), *d_hap = bufs.add(), *d_so = bufs.add(), *d_sl = bufs.add(),
         *d_ho = bufs.add(), *d_hl = bufs.add(), *d_tab = bufs.add(), *d_sc = bufs.add(), *d_ll = bufs.add(),
         *d_fl = bufs.add();
  const size_t m = (size_t)n;
  HIP_TRY(d_seq->ensure((size_t)seq_bytes));
  if (qual_pool) HIP_TRY(d_qual->ensure((size_t)seq_bytes));
  HIP_TRY(d_hap->ensure((size_t)hap_bytes));
  HIP_TRY(d_so->ensure(8 * m));
  HIP_TRY(d_sl->ensure(4 * m));
  HIP_TRY(d_ho->ensure(8 * m));
  HIP_TRY(d_hl->ensure(4 * m));
  HIP_TRY(d_tab->ensure(sizeof(t)));
  HIP_TRY(d_sc->ensure(8 * m));
  HIP_TRY(d_ll->ensure(8 * m));
  HIP_TRY(d_fl->ensure(m));
  if (seq_bytes) HIP_TRY(hipMemcpyAsync(d_seq->p, seq_pool, (size_t)seq_bytes, hipMemcpyHostToDevice, c->stream));
  if (seq_bytes && qual_pool)
    HIP_TRY(hipMemcpyAsync(d_qual->p, qual_pool, (size_t)seq_bytes, hipMemcpyHostToDevice, c->stream));
  if (hap_bytes) HIP_TRY(hipMemcpyAsync(d_hap->p, hap_pool, (size_t)hap_bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_so->p, seq_off, 8 * m, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_sl->p, seq_len, 4 * m, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_ho->p, hap_off, 8 * m, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_hl->p, hap_len, 4 * m, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_tab->p, t, sizeof(t), hipMemcpyHostToDevice, c->stream));
  const hlk::Pairs P{(const uint8_t *)d_seq->p, qual_pool ? (const uint8_t *)d_qual->p : nullptr,
                     (const int64_t *)d_so->p,  (const int32_t *)d_sl->p,
                     (const uint8_t *)d_hap->p, (const int64_t *)d_ho->p,
                     (const int32_t *)d_hl->p};
  if ((s = forward(c, P, n, (const double *)d_tab->p, (double *)d_sc->p, (double *)d_ll->p, (uint8_t *)d_fl->p, ks))) {
    (void)hipStreamSynchronize(c->stream);
    return s;
  }
  HIP_TRY(hipMemcpyAsync(res.p->scaled, d_sc->p, 8 * m, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(res.p->log_likelihood, d_ll->p, 8 * m, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(res.p->flags, d_fl->p, m, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipEventRecord(span.b, c->stream));
  HIP_TRY(hipEventSynchronize(span.b));
  HIP_TRY(hipEventElapsedTime(&res.p->ms, span.a, span.b));
  HIP_TRY(hipEventElapsedTime(&res.p->kernel_ms, ks.a, ks.b));
  *out = res.p;
  res.p = nullptr;
  return GQ_OK;
}

gq_status gq_haplik_windows(gq_ctx *c, const gq_dev_reads *d, const gq_reference *ref, int64_t W, const int32_t *contig,
                            const int32_t *start, const int32_t *end, const gq_asm_params *asm_params,
                            const gq_asm_path_block *paths, const gq_haplik_params *params, gq_haplik_block **out) {
  if (!c || !d || !ref || !paths || !out || W < 0) return set_err(GQ_E_ARG, "gq_haplik_windows: null or negative argument");
  if (d->ctx != c) return set_err(GQ_E_ARG, "gq_haplik_windows: the read set belongs to another context");
  if (ref->n_contigs != d->d.n_contigs)
    return set_err(GQ_E_ARG, "reference covers %d contigs, the read set %d", ref->n_contigs, d->d.n_contigs);
  if (ref->device != c->device) return set_err(GQ_E_ARG, "reference uploaded to another device");
  gq_asm_params ap;
  if (asm_params) ap = *asm_params;
  else gq_asm_default_params(&ap);
  if (ap.k < 2 || ap.k > 62 || ap.min_mapq < 0)
    return set_err(GQ_E_ARG, "gq_haplik_windows: k %d outside [2, 62] or min_mapq %d negative", ap.k, ap.min_mapq);
  gq_status s;
  double t[gq_haplik::kTableDoubles];
  if ((s = tables_of(params, t, "gq_haplik_windows"))) return s;
  if (paths->n_windows != W)
    return set_err(GQ_E_ARG, "gq_haplik_windows: %lld windows, the path block has %lld", (long long)W,
                   (long long)paths->n_windows);
  if (W > 0 && (!contig || !start || !end)) return set_err(GQ_E_ARG, "gq_haplik_windows: null array");
  if (W + 1 >= ((int64_t)1 << 31))
    return set_err(GQ_E_CAPACITY, "gq_haplik_windows: %lld windows in one call", (long long)W);
  for (int64_t w = 0; w < W; ++w)
    if (contig[w] < 0 || contig[w] >= d->d.n_contigs || start[w] < 0 || end[w] < start[w])
      return set_err(GQ_E_ARG, "gq_haplik_windows: window %lld: contig %d, [%d, %d)", (long long)w, contig[w], start[w],
                     end[w]);
  const int64_t NH = paths->n_haplotypes;
  if (!paths->hap_off || !paths->hap_seq_off || (NH > 0 && !paths->bases) || paths->hap_off[0] != 0 ||
      paths->hap_off[W] != NH || paths->hap_seq_off[0] != 0)
    return set_err(GQ_E_ARG, "gq_haplik_windows: the path block's haplotype offsets do not fit its counts");
  for (int64_t w = 0; w < W; ++w)
    if (paths->hap_off[w + 1] < paths->hap_off[w])
      return set_err(GQ_E_ARG, "gq_haplik_windows: window %lld has a negative haplotype count", (long long)w);
  for (int64_t h = 0; h < NH; ++h)
    if (paths->hap_seq_off[h + 1] < paths->hap_seq_off[h])
      return set_err(GQ_E_ARG, "gq_haplik_windows: haplotype %lld has a negative length", (long long)h);
  BlockGuard res;
  if (W == 0) {
    res.p = gq_haplik::new_block(0, 0, 0, 0);
    if (!res.p) return set_err(GQ_E_NOMEM, "gq_haplik_windows: result block");
    *out = res.p;
    res.p = nullptr;
    return GQ_OK;
  }
  if ((s = validation_wait(d))) return s;
  HIP_TRY(hipSetDevice(c->device));
  Span span, rs, ks, gs;
  HIP_TRY(span.make());
  HIP_TRY(rs.make());
  HIP_TRY(ks.make());
  HIP_TRY(gs.make());
  HIP_TRY(hipEventRecord(span.a, c->stream));
  HIP_TRY(hipEventRecord(rs.a, c->stream));
  WindowReads wr;
  if ((s = find_window_reads(c, d, W, contig, start, end, ap.k, ap.min_mapq, "gq_haplik_windows", wr))) return s;
  const size_t w1 = (size_t)W + 1;
  Bufs bufs;
  DevBuf *d_wro = bufs.add();
  HIP_TRY(d_wro->ensure(8 * w1));
  hipLaunchKernelGGL(hlk::hap_winoff_k, dim3((unsigned)((w1 + 255) / 256)), dim3(256), 0, c->stream, W,
                     (const int64_t *)wr.coff.p, (const int64_t *)wr.fsum.p, (int64_t *)d_wro->p);
  HIP_TRY(hipGetLastError());
  std::vector<int64_t> wro(w1), lik_off(w1), gt_off(w1);
  HIP_TRY(hipMemcpyAsync(wro.data(), d_wro->p, 8 * w1, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipEventRecord(rs.b, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  // the offsets of pairs and genotypes, from the windows' read counts and the path block
  int64_t n_pairs = 0;
  for (int64_t w = 0; w < W; ++w) {
    lik_off[(size_t)w] = n_pairs;
    n_pairs += (wro[(size_t)w + 1] - wro[(size_t)w]) * (paths->hap_off[w + 1] - paths->hap_off[w]);
  }
  lik_off[(size_t)W] = n_pairs;
  const int64_t n_reads = wro[(size_t)W];
  const int64_t G = gq_haplik::genotype_offsets(W, wro.data(), paths->hap_off, gt_off.data());
  if (n_pairs > 0)  // (a haplotype over the cap that no read meets is no pair)
    for (int64_t w = 0; w < W; ++w)
      if (wro[(size_t)w + 1] > wro[(size_t)w])
        for (int64_t h = paths->hap_off[w]; h < paths->hap_off[w + 1]; ++h)
          if (paths->hap_seq_off[h + 1] - paths->hap_seq_off[h] > gq_haplik::kMaxR)
            return set_err(GQ_E_CAPACITY, "haplik: pair %lld: haplotype length %lld is past the device cap of %d",
                           (long long)(lik_off[(size_t)w] + (h - paths->hap_off[w])),
                           (long long)(paths->hap_seq_off[h + 1] - paths->hap_seq_off[h]), gq_haplik::kMaxR);
  res.p = gq_haplik::new_block(W, n_reads, n_pairs, G);
  if (!res.p) return set_err(GQ_E_NOMEM, "gq_haplik_windows: result block");
  res.stream = c->stream;
  gq_haplik_block *b = res.p;
  memcpy(b->win_read_off, wro.data(), 8 * w1);
  memcpy(b->lik_off, lik_off.data(), 8 * w1);
  memcpy(b->gt_off, gt_off.data(), 8 * w1);
  for (int64_t w = 0; w < W; ++w) b->best_genotype[w] = -1;
  if (n_reads > 0)
    HIP_TRY(hipMemcpyAsync(b->win_reads, wr.list_read.p, 8 * (size_t)n_reads, hipMemcpyDeviceToHost, c->stream));
  if (n_pairs > 0) {
    const size_t m = (size_t)n_pairs, nh1 = (size_t)NH + 1;
    const int64_t hap_bytes = paths->hap_seq_off[NH];
    DevBuf *d_lo = bufs.add(), *d_who = bufs.add(), *d_hso = bufs.add(), *d_hap = bufs.add(), *d_go = bufs.add(),
           *d_so = bufs.add(), *d_sl = bufs.add(), *d_ho = bufs.add(), *d_hl = bufs.add(), *d_bad = bufs.add(),
           *d_tab = bufs.add(), *d_sc = bufs.add(), *d_ll = bufs.add(), *d_fl = bufs.add(), *d_gl = bufs.add(),
           *d_best = bufs.add();
    HIP_TRY(d_lo->ensure(8 * w1));
    HIP_TRY(d_who->ensure(8 * w1));
    HIP_TRY(d_hso->ensure(8 * nh1));
    HIP_TRY(d_hap->ensure((size_t)std::max<int64_t>(hap_bytes, 1)));
    HIP_TRY(d_go->ensure(8 * w1));
    HIP_TRY(d_so->ensure(8 * m));
    HIP_TRY(d_sl->ensure(4 * m));
    HIP_TRY(d_ho->ensure(8 * m));
    HIP_TRY(d_hl->ensure(4 * m));
    HIP_TRY(d_bad->ensure(8));
    HIP_TRY(d_tab->ensure(sizeof(t)));
    HIP_TRY(d_sc->ensure(8 * m));
    HIP_TRY(d_ll->ensure(8 * m));
    HIP_TRY(d_fl->ensure(m));
    HIP_TRY(d_gl->ensure(8 * (size_t)std::max<int64_t>(G, 1)));
    HIP_TRY(d_best->ensure(4 * (size_t)W));
    unsigned long long bad = ~0ull;
    HIP_TRY(hipMemcpyAsync(d_lo->p, lik_off.data(), 8 * w1, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_who->p, paths->hap_off, 8 * w1, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_hso->p, paths->hap_seq_off, 8 * nh1, hipMemcpyHostToDevice, c->stream));
    if (hap_bytes) HIP_TRY(hipMemcpyAsync(d_hap->p, paths->bases, (size_t)hap_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_go->p, gt_off.data(), 8 * w1, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_bad->p, &bad, 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_tab->p, t, sizeof(t), hipMemcpyHostToDevice, c->stream));
    if ((n_pairs + 255) / 256 >= ((int64_t)1 << 31))
      return set_err(GQ_E_CAPACITY, "gq_haplik_windows: %lld pairs in one call", (long long)n_pairs);
    const hlk::PairOut po{(int64_t *)d_so->p, (int32_t *)d_sl->p, (int64_t *)d_ho->p, (int32_t *)d_hl->p};
    hipLaunchKernelGGL(hlk::hap_pairs_k, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, c->stream, d->d, W, n_pairs,
                       (const int64_t *)d_lo->p, (const int64_t *)d_wro->p, (const int64_t *)wr.list_read.p,
                       (const int64_t *)d_who->p, (const int64_t *)d_hso->p, (int32_t)gq_haplik::kMaxS, po,
                       (unsigned long long *)d_bad->p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bad, d_bad->p, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (bad != ~0ull)  // before any pair is run: nothing is truncated
      return set_err(GQ_E_CAPACITY, "haplik: pair %lld: its read is longer than the device cap of %d", (long long)bad,
                     gq_haplik::kMaxS);
    const hlk::Pairs P{d->d.seq, d->d.qual, (const int64_t *)d_so->p, (const int32_t *)d_sl->p,
                       (const uint8_t *)d_hap->p, (const int64_t *)d_ho->p, (const int32_t *)d_hl->p};
    if ((s = forward(c, P, n_pairs, (const double *)d_tab->p, (double *)d_sc->p, (double *)d_ll->p, (uint8_t *)d_fl->p,
                     ks))) {
      (void)hipStreamSynchronize(c->stream);
      return s;
    }
    HIP_TRY(hipEventRecord(gs.a, c->stream));
    if (G > 0) {  // (G > 0 whenever a window has a pair)
      hipLaunchKernelGGL(hlk::hap_genotype_k, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, c->stream, W, G,
                         (const int64_t *)d_go->p, (const int64_t *)d_wro->p, (const int64_t *)d_who->p,
                         (const int64_t *)d_lo->p, (const double *)d_sc->p, (double *)d_gl->p);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(hlk::hap_best_k, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, c->stream, W,
                         (const int64_t *)d_go->p, (const double *)d_gl->p, (int32_t *)d_best->p);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(gs.b, c->stream));
    HIP_TRY(hipMemcpyAsync(b->scaled, d_sc->p, 8 * m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(b->log_likelihood, d_ll->p, 8 * m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(b->flags, d_fl->p, m, hipMemcpyDeviceToHost, c->stream));
    if (G > 0) {
      HIP_TRY(hipMemcpyAsync(b->gt_log_likelihood, d_gl->p, 8 * (size_t)G, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipMemcpyAsync(b->best_genotype, d_best->p, 4 * (size_t)W, hipMemcpyDeviceToHost, c->stream));
    }
  }
  HIP_TRY(hipEventRecord(span.b, c->stream));
  HIP_TRY(hipEventSynchronize(span.b));
  HIP_TRY(hipEventElapsedTime(&b->ms, span.a, span.b));
  HIP_TRY(hipEventElapsedTime(&b->reads_ms, rs.a, rs.b));
  if (n_pairs > 0) {
    HIP_TRY(hipEventElapsedTime(&b->kernel_ms, ks.a, ks.b));
    HIP_TRY(hipEventElapsedTime(&b->genotype_ms, gs.a, gs.b));
  }
  *out = b;
  res.p = nullptr;
  return GQ_OK;
}

}  // extern "C"
