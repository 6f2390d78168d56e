// gq_align.hip — affine-gap alignment (gqpileup.h: gq_align_*): the C ABI over the host twin
// (gq_align_host.h) and the device kernels (gq_align.h).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdlib>
#include <memory>
#include <vector>

#include "../../include/gqpileup.h"
#include "gq_host.h"
#include "gq_align_host.h"
#include "gq_align.h"

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

gq_status table_of(const gq_align_params *params, double t[32], const char *who) {
  gq_align_params p;
  if (params) p = *params;
  else gq_align_default_params(&p);
  if (!gq_align::valid(p))
    return set_err(GQ_E_ARG, "%s: probabilities must lie strictly inside (0, 1): mismatch %g, open gap %g, close gap %g",
                   who, p.mismatch_probability, p.open_gap_probability, p.close_gap_probability);
  gq_align::penalty_table(p, t);
  return GQ_OK;
}

int64_t scratch_limit() {  // bytes of scratch one launch may use
  const int64_t floor_ = aln::scratch_bytes(gq_align::kMaxS, gq_align::kMaxR);
  int64_t lim;
  if (const char *e = getenv("GQ_ALIGN_SCRATCH_BYTES")) {
    lim = atoll(e);
  } else {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = (size_t)1 << 30;
    lim = (int64_t)(fr / 4);
  }
  return std::max(lim, floor_);
}

// The pairs of P (device arrays; h_seq_len / h_ref_len their lengths on the host) through align_k.
gq_status run_pairs(gq_ctx *c, int64_t n, const aln::Pairs &P, const int32_t *h_seq_len, const int32_t *h_ref_len,
                    const double *table, gq_alignments **out) {
  for (int64_t i = 0; i < n; ++i) {
    if (h_seq_len[i] > gq_align::kMaxS)
      return set_err(GQ_E_CAPACITY, "align: pair %lld: sequence length %d is past the device cap of %d", (long long)i,
                     h_seq_len[i], gq_align::kMaxS);
    if (h_ref_len[i] > gq_align::kMaxR)
      return set_err(GQ_E_CAPACITY, "align: pair %lld: reference length %d is past the device cap of %d", (long long)i,
                     h_ref_len[i], gq_align::kMaxR);
  }
  // launches: consecutive pairs whose scratch fits the limit (at most 2^30 pairs each)
  const int64_t limit = scratch_limit();
  std::vector<int64_t> cut{0};
  int64_t max_pairs = 0, max_bytes = 0;
  {
    int64_t used = 0;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t need = aln::scratch_bytes(h_seq_len[i], h_ref_len[i]);
      if (i > cut.back() && (used + need > limit || i - cut.back() >= ((int64_t)1 << 30))) {
        cut.push_back(i);
        used = 0;
      }
      used += need;
      max_bytes = std::max(max_bytes, used);
      max_pairs = std::max(max_pairs, i + 1 - cut.back());
    }
    cut.push_back(n);
  }
  const size_t m = (size_t)max_pairs;
  Bufs bufs;
  DevBuf *d_table = bufs.add(), *d_scr_off = bufs.add(), *d_start = bufs.add(), *d_end = bufs.add(),
         *d_score = bufs.add(), *d_nops = bufs.add(), *d_begin = bufs.add(), *d_off = bufs.add(),
         *d_scratch = bufs.add(), *d_tmp = bufs.add(), *d_cigar = bufs.add();
  HIP_TRY(d_table->ensure(32 * sizeof(double)));
  HIP_TRY(d_scr_off->ensure(8 * m));
  HIP_TRY(d_start->ensure(4 * m));
  HIP_TRY(d_end->ensure(4 * m));
  HIP_TRY(d_score->ensure(8 * m));
  HIP_TRY(d_nops->ensure(8 * (m + 1)));
  HIP_TRY(d_begin->ensure(8 * m));
  HIP_TRY(d_off->ensure(8 * (m + 1)));
  if (d_scratch->ensure((size_t)max_bytes) != hipSuccess)
    return set_err(GQ_E_NOMEM, "align: %lld bytes of device scratch", (long long)max_bytes);
  HIP_TRY(hipMemcpyAsync(d_table->p, table, 32 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  Span ks;
  HIP_TRY(ks.make());

  std::vector<int32_t> r_start((size_t)n), r_end((size_t)n);
  std::vector<double> r_score((size_t)n);
  std::vector<int64_t> r_off((size_t)n + 1, 0), scr_off(m), h_nops(m + 1);
  std::vector<uint32_t> r_cigar;
  float kernel_ms = 0.f;
  int32_t launches = 0;
  for (size_t q = 0; q + 1 < cut.size(); ++q) {
    const int64_t a = cut[q], k = cut[q + 1] - a;
    if (k <= 0) continue;
    int64_t used = 0;
    for (int64_t i = 0; i < k; ++i) {
      scr_off[(size_t)i] = used;
      used += aln::scratch_bytes(h_seq_len[a + i], h_ref_len[a + i]);
    }
    HIP_TRY(hipMemcpyAsync(d_scr_off->p, scr_off.data(), 8 * (size_t)k, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync((int64_t *)d_nops->p + k, 0, 8, c->stream));
    const aln::Out o{(int32_t *)d_start->p, (int32_t *)d_end->p, (double *)d_score->p, (int64_t *)d_nops->p,
                     (int64_t *)d_begin->p};
    HIP_TRY(hipEventRecord(ks.a, c->stream));
    hipLaunchKernelGGL(aln::align_k, dim3((unsigned)k), dim3(aln::kLanes), 0, c->stream, P, a,
                       (const double *)d_table->p, (const int64_t *)d_scr_off->p, (uint8_t *)d_scratch->p, o);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ks.b, c->stream));
    ++launches;
    size_t tb = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (const int64_t *)d_nops->p, (int64_t *)d_off->p, (int)(k + 1),
                                             c->stream));
    HIP_TRY(d_tmp->ensure(tb));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp->p, tb, (const int64_t *)d_nops->p, (int64_t *)d_off->p, (int)(k + 1),
                                             c->stream));
    HIP_TRY(hipMemcpyAsync(h_nops.data(), d_off->p, 8 * (size_t)(k + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ks.a, ks.b));
    kernel_ms += ms;
    const int64_t total = h_nops[(size_t)k];
    HIP_TRY(d_cigar->ensure(4 * (size_t)std::max<int64_t>(total, 1)));
    if (total > 0) {
      hipLaunchKernelGGL(aln::cigar_gather_k, dim3((unsigned)((k * 64 + 255) / 256)), dim3(256), 0, c->stream, k,
                         (const int64_t *)d_nops->p, (const int64_t *)d_begin->p, (const int64_t *)d_off->p,
                         (const uint32_t *)d_scratch->p, (uint32_t *)d_cigar->p);
      HIP_TRY(hipGetLastError());
    }
    const size_t base = r_cigar.size();
    r_cigar.resize(base + (size_t)total);
    HIP_TRY(hipMemcpyAsync(r_start.data() + a, d_start->p, 4 * (size_t)k, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(r_end.data() + a, d_end->p, 4 * (size_t)k, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(r_score.data() + a, d_score->p, 8 * (size_t)k, hipMemcpyDeviceToHost, c->stream));
    if (total > 0)
      HIP_TRY(hipMemcpyAsync(r_cigar.data() + base, d_cigar->p, 4 * (size_t)total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i <= k; ++i) r_off[(size_t)(a + i)] = (int64_t)base + h_nops[(size_t)i];
  }
  gq_alignments *res = gq_align::new_block(n, (int64_t)r_cigar.size());
  if (!res) return set_err(GQ_E_NOMEM, "align: result block");
  for (int64_t i = 0; i < n; ++i) {
    res->ref_start[i] = r_start[(size_t)i];
    res->ref_end[i] = r_end[(size_t)i];
    res->score[i] = r_score[(size_t)i];
    res->score_int[i] = gq_align::double_to_int(r_score[(size_t)i]);
  }
  memcpy(res->cigar_off, r_off.data(), 8 * ((size_t)n + 1));
  if (!r_cigar.empty()) memcpy(res->cigar, r_cigar.data(), 4 * r_cigar.size());
  res->kernel_ms = kernel_ms;
  res->launches = launches;
  *out = res;
  return GQ_OK;
}

gq_status check_pairs(const char *who, int64_t n, const uint8_t *seq_pool, const int64_t *seq_off, const int32_t *seq_len,
                      const uint8_t *ref_pool, const int64_t *ref_off, const int32_t *ref_len, gq_alignments **out) {
  if (n < 0 || !out) return set_err(GQ_E_ARG, "%s: null or negative argument", who);
  if (n > 0 && (!seq_pool || !seq_off || !seq_len || !ref_pool || !ref_off || !ref_len))
    return set_err(GQ_E_ARG, "%s: null array", who);
  for (int64_t i = 0; i < n; ++i)
    if (seq_len[i] < 0 || ref_len[i] < 0 || seq_off[i] < 0 || ref_off[i] < 0)
      return set_err(GQ_E_ARG, "%s: pair %lld has a negative offset or length", who, (long long)i);
  return GQ_OK;
}

}  // namespace

extern "C" {

void gq_align_default_params(gq_align_params *out) {
  if (!out) return;
  memset(out, 0, sizeof(*out));
  out->mismatch_probability = std::exp(-4.0);
  out->open_gap_probability = std::exp(-6.0);
  out->close_gap_probability = 1 - std::exp(-1.0);
}

gq_status gq_align_penalties(const gq_align_params *params, double table[32]) {
  if (!table) return set_err(GQ_E_ARG, "gq_align_penalties: null table");
  return table_of(params, table, "gq_align_penalties");
}

void gq_align_limits(int32_t out[8]) {
  if (!out) return;
  const int32_t v[8] = {gq_align::kMaxS, gq_align::kMaxR, aln::kLanes, aln::kMaxRows, aln::kLdsTb, 0, 0, 0};
  memcpy(out, v, sizeof(v));
}

void gq_free_alignments(gq_alignments *a) { gq_align::free_block(a); }
void gq_align_free_index(void *p) { free(p); }

gq_status gq_align_host(int64_t n, const uint8_t *seq_pool, const int64_t *seq_off, const int32_t *seq_len,
                        const uint8_t *ref_pool, const int64_t *ref_off, const int32_t *ref_len,
                        const gq_align_params *params, gq_alignments **out) {
  gq_status s;
  if ((s = check_pairs("gq_align_host", n, seq_pool, seq_off, seq_len, ref_pool, ref_off, ref_len, out))) return s;
  double t[32];
  if ((s = table_of(params, t, "gq_align_host"))) return s;
  int64_t bad = -1;
  const int rc = gq_align::align_host(n, seq_pool, seq_off, seq_len, ref_pool, ref_off, ref_len, t, out, &bad);
  if (rc == 1) return set_err(GQ_E_NOMEM, "gq_align_host: result block");
  if (rc) return set_err(GQ_E_ARG, "gq_align_host: pair %lld has a negative offset or length", (long long)bad);
  return GQ_OK;
}

gq_status gq_align_batch(gq_ctx *c, int64_t n, const uint8_t *seq_pool, const int64_t *seq_off, const int32_t *seq_len,
                         const uint8_t *ref_pool, const int64_t *ref_off, const int32_t *ref_len,
                         const gq_align_params *params, gq_alignments **out) {
  if (!c) return set_err(GQ_E_ARG, "gq_align_batch: null ctx");
  gq_status s;
  if ((s = check_pairs("gq_align_batch", n, seq_pool, seq_off, seq_len, ref_pool, ref_off, ref_len, out))) return s;
  double t[32];
  if ((s = table_of(params, t, "gq_align_batch"))) return s;
  if (n == 0) {
    gq_alignments *res = gq_align::new_block(0, 0);
    if (!res) return set_err(GQ_E_NOMEM, "gq_align_batch: result block");
    *out = res;
    return GQ_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  int64_t seq_bytes = 0, ref_bytes = 0;
  for (int64_t i = 0; i < n; ++i) {
    seq_bytes = std::max(seq_bytes, seq_off[i] + seq_len[i]);
    ref_bytes = std::max(ref_bytes, ref_off[i] + ref_len[i]);
  }
  Span span;
  HIP_TRY(span.make());
  HIP_TRY(hipEventRecord(span.a, c->stream));
  Bufs bufs;
  DevBuf *d_seq = bufs.add(), *d_ref = bufs.add(), *d_so = bufs.add(), *d_sl = bufs.add(), *d_ro = bufs.add(),
         *d_rl = bufs.add();
  HIP_TRY(d_seq->ensure((size_t)seq_bytes));
  HIP_TRY(d_ref->ensure((size_t)ref_bytes));
  HIP_TRY(d_so->ensure(8 * (size_t)n));
  HIP_TRY(d_sl->ensure(4 * (size_t)n));
  HIP_TRY(d_ro->ensure(8 * (size_t)n));
  HIP_TRY(d_rl->ensure(4 * (size_t)n));
  if (seq_bytes) HIP_TRY(hipMemcpyAsync(d_seq->p, seq_pool, (size_t)seq_bytes, hipMemcpyHostToDevice, c->stream));
  if (ref_bytes) HIP_TRY(hipMemcpyAsync(d_ref->p, ref_pool, (size_t)ref_bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_so->p, seq_off, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_sl->p, seq_len, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_ro->p, ref_off, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_rl->p, ref_len, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  const aln::Pairs P{(const uint8_t *)d_seq->p, (const int64_t *)d_so->p, (const int32_t *)d_sl->p,
                     (const uint8_t *)d_ref->p, (const int64_t *)d_ro->p, (const int32_t *)d_rl->p};
  gq_alignments *res = nullptr;
  if ((s = run_pairs(c, n, P, seq_len, ref_len, t, &res))) {
    (void)hipStreamSynchronize(c->stream);
    return s;
  }
  HIP_TRY(hipEventRecord(span.b, c->stream));
  HIP_TRY(hipEventSynchronize(span.b));
  HIP_TRY(hipEventElapsedTime(&res->ms, span.a, span.b));
  *out = res;
  return GQ_OK;
}

gq_status gq_align_reads(gq_ctx *c, const gq_dev_reads *d, const gq_reference *ref, int32_t pad, int32_t all_reads,
                         const gq_align_params *params, gq_alignments **out, int64_t **read_index_out, int32_t **lo_out,
                         gq_align_reads_info *info) {
  if (!c || !d || !ref || !out || !read_index_out || !lo_out) return set_err(GQ_E_ARG, "gq_align_reads: null argument");
  if (d->ctx != c) return set_err(GQ_E_ARG, "gq_align_reads: the read set belongs to another context");
  if (ref->n_contigs != d->d.n_contigs)
    return set_err(GQ_E_ARG, "reference covers %d contigs, the read set %d", ref->n_contigs, d->d.n_contigs);
  if (ref->device != c->device) return set_err(GQ_E_ARG, "reference uploaded to another device");
  if (pad < 0 || pad > gq_align::kMaxR) return set_err(GQ_E_ARG, "gq_align_reads: pad %d outside [0, %d]", pad, gq_align::kMaxR);
  gq_status s;
  double t[32];
  if ((s = table_of(params, t, "gq_align_reads"))) return s;
  if ((s = validation_wait(d))) return s;
  HIP_TRY(hipSetDevice(c->device));
  const int64_t n = d->d.n_reads;
  gq_align_reads_info inf{};
  inf.n_reads = n;
  Span span, sel;
  HIP_TRY(span.make());
  HIP_TRY(sel.make());
  HIP_TRY(hipEventRecord(span.a, c->stream));
  HIP_TRY(hipEventRecord(sel.a, c->stream));
  Bufs bufs;
  DevBuf *d_flag = bufs.add(), *d_at = bufs.add(), *d_lo = bufs.add(), *d_hi = bufs.add(), *d_ctr = bufs.add(),
         *d_tmp = bufs.add();
  const size_t m = (size_t)std::max<int64_t>(n, 1);
  HIP_TRY(d_flag->ensure(8 * (m + 1)));
  HIP_TRY(d_at->ensure(8 * (m + 1)));
  HIP_TRY(d_lo->ensure(4 * m));
  HIP_TRY(d_hi->ensure(4 * m));
  HIP_TRY(d_ctr->ensure(16));
  unsigned long long ctr[2] = {0ull, ~0ull};
  HIP_TRY(hipMemcpyAsync(d_ctr->p, ctr, 16, hipMemcpyHostToDevice, c->stream));
  const aln::RefView rv{(const uint8_t *)ref->bytes, ref->d_off, ref->d_len};
  hipLaunchKernelGGL(aln::align_select_k, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, c->stream, d->d, rv, pad,
                     all_reads ? 1 : 0, (int64_t *)d_flag->p, (int32_t *)d_lo->p, (int32_t *)d_hi->p,
                     (unsigned long long *)d_ctr->p);
  HIP_TRY(hipGetLastError());
  if (n + 1 >= ((int64_t)1 << 31)) return set_err(GQ_E_CAPACITY, "gq_align_reads: %lld reads in one call", (long long)n);
  size_t tb = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (const int64_t *)d_flag->p, (int64_t *)d_at->p, (int)(n + 1),
                                           c->stream));
  HIP_TRY(d_tmp->ensure(tb));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp->p, tb, (const int64_t *)d_flag->p, (int64_t *)d_at->p, (int)(n + 1),
                                           c->stream));
  int64_t k = 0;
  HIP_TRY(hipMemcpyAsync(&k, (const int64_t *)d_at->p + n, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(ctr, d_ctr->p, 16, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (ctr[1] != ~0ull)
    return set_err(GQ_E_ARG, "align: read %lld lies on a contig the reference lacks", (long long)ctr[1]);
  inf.skipped = (int64_t)ctr[0];
  inf.n_selected = k;
  const size_t mk = (size_t)std::max<int64_t>(k, 1);
  DevBuf *d_idx = bufs.add(), *d_slo = bufs.add(), *d_so = bufs.add(), *d_sl = bufs.add(), *d_ro = bufs.add(),
         *d_rl = bufs.add();
  HIP_TRY(d_idx->ensure(8 * mk));
  HIP_TRY(d_slo->ensure(4 * mk));
  HIP_TRY(d_so->ensure(8 * mk));
  HIP_TRY(d_sl->ensure(4 * mk));
  HIP_TRY(d_ro->ensure(8 * mk));
  HIP_TRY(d_rl->ensure(4 * mk));
  int64_t *h_idx = (int64_t *)malloc(8 * mk);
  int32_t *h_lo = (int32_t *)malloc(4 * mk);
  std::unique_ptr<int64_t, decltype(&free)> g_idx(h_idx, &free);
  std::unique_ptr<int32_t, decltype(&free)> g_lo(h_lo, &free);
  if (!h_idx || !h_lo) return set_err(GQ_E_NOMEM, "gq_align_reads: index arrays");
  std::vector<int32_t> h_sl(mk), h_rl(mk);
  if (k > 0) {
    hipLaunchKernelGGL(aln::align_compact_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d->d, rv,
                       (const int64_t *)d_flag->p, (const int64_t *)d_at->p, (const int32_t *)d_lo->p,
                       (const int32_t *)d_hi->p, (int64_t *)d_idx->p, (int32_t *)d_slo->p, (int64_t *)d_so->p,
                       (int32_t *)d_sl->p, (int64_t *)d_ro->p, (int32_t *)d_rl->p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_idx, d_idx->p, 8 * (size_t)k, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h_lo, d_slo->p, 4 * (size_t)k, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h_sl.data(), d_sl->p, 4 * (size_t)k, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h_rl.data(), d_rl->p, 4 * (size_t)k, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipEventRecord(sel.b, c->stream));
  HIP_TRY(hipEventSynchronize(sel.b));
  HIP_TRY(hipEventElapsedTime(&inf.select_ms, sel.a, sel.b));
  gq_alignments *res = nullptr;
  if (k == 0) {
    res = gq_align::new_block(0, 0);
    if (!res) return set_err(GQ_E_NOMEM, "gq_align_reads: result block");
  } else {
    const aln::Pairs P{d->d.seq, (const int64_t *)d_so->p, (const int32_t *)d_sl->p, (const uint8_t *)ref->bytes,
                       (const int64_t *)d_ro->p, (const int32_t *)d_rl->p};
    if ((s = run_pairs(c, k, P, h_sl.data(), h_rl.data(), t, &res))) {
      (void)hipStreamSynchronize(c->stream);
      return s;
    }
  }
  HIP_TRY(hipEventRecord(span.b, c->stream));
  HIP_TRY(hipEventSynchronize(span.b));
  HIP_TRY(hipEventElapsedTime(&res->ms, span.a, span.b));
  *out = res;
  *read_index_out = g_idx.release();
  *lo_out = g_lo.release();
  if (info) *info = inf;
  return GQ_OK;
}

}  // extern "C"
