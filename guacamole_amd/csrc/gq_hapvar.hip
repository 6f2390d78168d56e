// gq_hapvar.hip — variants from assembled haplotypes (gqpileup.h: gq_hapvar_*): the C ABI over the
// host twin (gq_hapvar_host.h) and the device kernels (gq_hapvar.h).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdlib>
#include <vector>

#include "../../include/gqpileup.h"
#include "gq_host.h"
#include "gq_hapvar_host.h"
#include "gq_hapvar.h"

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

// the result block until it is handed out; on an early return the stream is drained first, since
// copies into the block may still be queued
struct BlockGuard {
  gq_hapvar_block *p = nullptr;
  hipStream_t stream = nullptr;
  ~BlockGuard() {
    if (p && stream) (void)hipStreamSynchronize(stream);
    gq_hapvar::free_block(p);
  }
};

gq_status prepared(const gq_hapvar_input *in, gq_hapvar_block **out, gq_hapvar::Prepared &P, const char *who) {
  if (!in || !out) return set_err(GQ_E_ARG, "%s: null argument", who);
  char msg[200];
  const int rc = gq_hapvar::prepare(in, P, msg, sizeof(msg));
  if (rc) return set_err((gq_status)rc, "%s", msg);
  return GQ_OK;
}

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" {

void gq_hapvar_limits(int32_t out[8]) {
  if (!out) return;
  const int32_t v[8] = {gq_hapvar::kMaxHaps, gq_hapvar::kMaxRaw, gq_hapvar::kSortThreads, 16 * gq_hapvar::kMaxRaw,
                        gq_hapvar::kPassReads, 0, 0, 0};
  memcpy(out, v, sizeof(v));
}

void gq_hapvar_free_block(gq_hapvar_block *b) { gq_hapvar::free_block(b); }

gq_status gq_hapvar_host(const gq_hapvar_input *in, int32_t threads, gq_hapvar_block **out) {
  gq_hapvar::Prepared P;
  gq_status s;
  if ((s = prepared(in, out, P, "gq_hapvar_host"))) return s;
  gq_hapvar_block *b = gq_hapvar::run_host(in, P, threads);
  if (!b) return set_err(GQ_E_NOMEM, "gq_hapvar_host: result block");
  *out = b;
  return GQ_OK;
}

gq_status gq_hapvar_windows(gq_ctx *c, const gq_hapvar_input *in, gq_hapvar_block **out) {
  if (!c) return set_err(GQ_E_ARG, "gq_hapvar_windows: null ctx");
  gq_hapvar::Prepared P;
  gq_status s;
  if ((s = prepared(in, out, P, "gq_hapvar_windows"))) return s;
  const int64_t W = in->n_windows, NH = in->n_haplotypes;
  if (W + 1 >= ((int64_t)1 << 31) || NH + 1 >= ((int64_t)1 << 31))
    return set_err(GQ_E_CAPACITY, "gq_hapvar_windows: %lld windows, %lld haplotypes in one call", (long long)W, (long long)NH);
  bool any = false;
  for (uint64_t u : P.usable) any = any || u != 0;
  BlockGuard res;
  if (!any) {  // no usable haplotype: no events, no launch
    res.p = gq_hapvar::new_block(W, 0, NH, 0);
    if (!res.p) return set_err(GQ_E_NOMEM, "gq_hapvar_windows: result block");
    if (NH > 0) memcpy(res.p->hap_flags, P.hap_flags.data(), (size_t)NH);
    *out = res.p;
    res.p = nullptr;
    return GQ_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  Span span, es, ms;
  HIP_TRY(span.make());
  HIP_TRY(es.make());
  HIP_TRY(ms.make());
  HIP_TRY(hipEventRecord(span.a, c->stream));
  const size_t w1 = (size_t)W + 1, nh = (size_t)NH, nh1 = nh + 1;
  std::vector<int32_t> hap_win(nh);
  for (int64_t w = 0; w < W; ++w)
    for (int64_t h = in->hap_off[w]; h < in->hap_off[w + 1]; ++h) hap_win[(size_t)h] = (int32_t)w;
  const int64_t hap_bytes = in->hap_seq_off[NH];
  Bufs bufs;
  auto up = [&](DevBuf *&d, const void *src, size_t bytes) -> hipError_t {
    d = bufs.add();
    hipError_t e = d->ensure(bytes ? bytes : 1);
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(d->p, src, bytes, hipMemcpyHostToDevice, c->stream);
    return e;
  };
  DevBuf *d_hf, *d_hw, *d_co, *d_nc, *d_cig, *d_hso, *d_bases, *d_who, *d_ref, *d_ro, *d_ws, *d_us;
  HIP_TRY(up(d_hf, P.hap_flags.data(), nh));
  HIP_TRY(up(d_hw, hap_win.data(), 4 * nh));
  HIP_TRY(up(d_co, P.cig_off.data(), 8 * nh));
  HIP_TRY(up(d_nc, P.n_cigar.data(), 4 * nh));
  HIP_TRY(up(d_cig, in->cigar, 4 * (size_t)P.cigar_words));
  HIP_TRY(up(d_hso, in->hap_seq_off, 8 * nh1));
  HIP_TRY(up(d_bases, in->bases, (size_t)hap_bytes));
  HIP_TRY(up(d_who, in->hap_off, 8 * w1));
  HIP_TRY(up(d_ref, in->ref_pool, (size_t)P.ref_bytes));
  HIP_TRY(up(d_ro, in->ref_off, 8 * (size_t)W));
  HIP_TRY(up(d_ws, in->win_start, 4 * (size_t)W));
  HIP_TRY(up(d_us, P.usable.data(), 8 * (size_t)W));
  const hvk::Haps HP{(const uint8_t *)d_hf->p,  (const int32_t *)d_hw->p,  (const int64_t *)d_co->p,    (const int32_t *)d_nc->p,
                     (const uint32_t *)d_cig->p, (const int64_t *)d_hso->p, (const uint8_t *)d_bases->p, (const int64_t *)d_who->p,
                     (const uint8_t *)d_ref->p,  (const int64_t *)d_ro->p};
  // ---- events ----
  HIP_TRY(hipEventRecord(es.a, c->stream));
  DevBuf *d_nraw = bufs.add(), *d_ndrop = bufs.add(), *d_roff = bufs.add(), *d_tmp = bufs.add();
  HIP_TRY(d_nraw->ensure(8 * nh1));
  HIP_TRY(d_ndrop->ensure(4 * nh1));
  HIP_TRY(d_roff->ensure(8 * nh1));
  hipLaunchKernelGGL(hvk::hv_count_k, dim3(blocks_of(NH + 1, 256)), dim3(256), 0, c->stream, HP, NH, (int64_t *)d_nraw->p,
                     (int32_t *)d_ndrop->p);
  HIP_TRY(hipGetLastError());
  size_t tb = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (const int64_t *)d_nraw->p, (int64_t *)d_roff->p, (int)nh1, c->stream));
  HIP_TRY(d_tmp->ensure(tb ? tb : 1));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp->p, tb, (const int64_t *)d_nraw->p, (int64_t *)d_roff->p, (int)nh1, c->stream));
  int64_t n_raw = 0;
  HIP_TRY(hipMemcpyAsync(&n_raw, (const int64_t *)d_roff->p + NH, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const size_t nr = (size_t)(n_raw > 0 ? n_raw : 1);
  DevBuf *r_off = bufs.add(), *r_rl = bufs.add(), *r_al = bufs.add(), *r_hp = bufs.add(), *r_h = bufs.add(),
         *c_off = bufs.add(), *c_rl = bufs.add(), *c_al = bufs.add(), *c_hp = bufs.add(), *c_rel = bufs.add(),
         *c_car = bufs.add(), *d_nev = bufs.add(), *d_nalt = bufs.add(), *d_wf = bufs.add(), *d_drop = bufs.add();
  for (DevBuf *x : {r_off, r_rl, r_al, c_off, c_rl, c_al}) HIP_TRY(x->ensure(4 * nr));
  for (DevBuf *x : {r_hp, c_hp, c_rel, c_car}) HIP_TRY(x->ensure(8 * nr));
  HIP_TRY(r_h->ensure(nr));
  HIP_TRY(d_nev->ensure(4 * (size_t)W));
  HIP_TRY(d_nalt->ensure(8 * (size_t)W));
  HIP_TRY(d_wf->ensure((size_t)W));
  HIP_TRY(d_drop->ensure(8));
  HIP_TRY(hipMemsetAsync(d_drop->p, 0, 8, c->stream));
  const hvk::RawOut RO{(int32_t *)r_off->p, (int32_t *)r_rl->p, (int32_t *)r_al->p, (int64_t *)r_hp->p, (uint8_t *)r_h->p};
  const hvk::Compact CO{(int32_t *)c_off->p, (int32_t *)c_rl->p, (int32_t *)c_al->p,
                        (int64_t *)c_hp->p,  (int64_t *)c_rel->p, (uint64_t *)c_car->p};
  hipLaunchKernelGGL(hvk::hv_write_k, dim3(blocks_of(NH, 256)), dim3(256), 0, c->stream, HP, NH, (const int64_t *)d_roff->p, RO);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(hvk::hv_window_k, dim3((unsigned)W), dim3(hvk::kSortThreads), 0, c->stream, W, (const int64_t *)d_who->p,
                     (const int64_t *)d_roff->p, (const int32_t *)d_ndrop->p, RO, (const uint8_t *)d_bases->p, CO,
                     (int32_t *)d_nev->p, (int64_t *)d_nalt->p, (uint8_t *)d_wf->p, (unsigned long long *)d_drop->p);
  HIP_TRY(hipGetLastError());
  // the windows' counts size the flat arrays
  std::vector<int32_t> n_ev((size_t)W);
  std::vector<int64_t> n_alt((size_t)W), ev_off(w1), win_alt(w1);
  unsigned long long dropped = 0;
  HIP_TRY(hipMemcpyAsync(n_ev.data(), d_nev->p, 4 * (size_t)W, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(n_alt.data(), d_nalt->p, 8 * (size_t)W, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(&dropped, d_drop->p, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  int64_t E = 0, A = 0;
  for (int64_t w = 0; w < W; ++w) {
    ev_off[(size_t)w] = E;
    win_alt[(size_t)w] = A;
    E += n_ev[(size_t)w];
    A += n_alt[(size_t)w];
  }
  ev_off[(size_t)W] = E;
  win_alt[(size_t)W] = A;
  if (E + hvk::kEventWaves >= ((int64_t)1 << 31))
    return set_err(GQ_E_CAPACITY, "gq_hapvar_windows: %lld events in one call", (long long)E);
  res.p = gq_hapvar::new_block(W, E, NH, A);
  if (!res.p) return set_err(GQ_E_NOMEM, "gq_hapvar_windows: result block");
  res.stream = c->stream;
  gq_hapvar_block *b = res.p;
  memcpy(b->ev_off, ev_off.data(), 8 * w1);
  memcpy(b->hap_flags, P.hap_flags.data(), nh);
  b->n_edge_dropped = (int64_t)dropped;
  HIP_TRY(hipMemcpyAsync(b->win_flags, d_wf->p, (size_t)W, hipMemcpyDeviceToHost, c->stream));
  const size_t ne = (size_t)E;
  DevBuf *d_eo, *d_wa, *d_wro, *d_lo, *d_sc;
  DevBuf *e_pos = bufs.add(), *e_kind = bufs.add(), *e_rl = bufs.add(), *e_ao = bufs.add(), *e_al = bufs.add(),
         *e_ab = bufs.add(), *e_car = bufs.add(), *e_gl = bufs.add(), *e_best = bufs.add(), *e_adr = bufs.add(),
         *e_ada = bufs.add(), *e_dp = bufs.add(), *e_ef = bufs.add();
  if (E > 0) {
    HIP_TRY(up(d_eo, ev_off.data(), 8 * w1));
    HIP_TRY(up(d_wa, win_alt.data(), 8 * w1));
    for (DevBuf *x : {e_pos, e_ao, e_car}) HIP_TRY(x->ensure(8 * ne));
    for (DevBuf *x : {e_rl, e_al, e_best, e_adr, e_ada, e_dp}) HIP_TRY(x->ensure(4 * ne));
    for (DevBuf *x : {e_kind, e_ef}) HIP_TRY(x->ensure(ne));
    HIP_TRY(e_ab->ensure((size_t)A));
    HIP_TRY(e_gl->ensure(24 * ne));
    const hvk::Events EV{(int64_t *)e_pos->p, (uint8_t *)e_kind->p, (int32_t *)e_rl->p,   (int64_t *)e_ao->p,
                         (int32_t *)e_al->p,  (uint8_t *)e_ab->p,   (uint64_t *)e_car->p};
    hipLaunchKernelGGL(hvk::hv_gather_k, dim3(blocks_of(E, 256)), dim3(256), 0, c->stream, W, E, (const int64_t *)d_eo->p,
                       (const int64_t *)d_who->p, (const int64_t *)d_roff->p, (const int64_t *)d_wa->p,
                       (const int32_t *)d_ws->p, (const uint8_t *)d_ref->p, (const int64_t *)d_ro->p,
                       (const uint8_t *)d_bases->p, CO, EV);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(es.b, c->stream));
  // ---- marginal ----
  HIP_TRY(hipEventRecord(ms.a, c->stream));
  if (E > 0) {
    int64_t n_scaled = 0;  // the likelihoods the events' windows read
    for (int64_t w = 0; w < W; ++w)
      if (n_ev[(size_t)w] > 0)
        n_scaled = std::max(n_scaled, in->lik_off[w] + (in->win_read_off[w + 1] - in->win_read_off[w]) *
                                                           (in->hap_off[w + 1] - in->hap_off[w]));
    HIP_TRY(up(d_wro, in->win_read_off, 8 * w1));
    HIP_TRY(up(d_lo, in->lik_off, 8 * w1));
    HIP_TRY(up(d_sc, in->scaled, 8 * (size_t)n_scaled));
    hipLaunchKernelGGL(hvk::hv_marginal_k, dim3(blocks_of(E, hvk::kEventWaves)), dim3(64 * hvk::kEventWaves), 0, c->stream, W,
                       E, (const int64_t *)d_eo->p, (const int64_t *)d_wro->p, (const int64_t *)d_who->p,
                       (const int64_t *)d_lo->p, (const double *)d_sc->p, (const uint64_t *)d_us->p,
                       (const uint64_t *)e_car->p, (double *)e_gl->p, (int32_t *)e_best->p, (int32_t *)e_adr->p,
                       (int32_t *)e_ada->p, (int32_t *)e_dp->p, (uint8_t *)e_ef->p);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(ms.b, c->stream));
  if (E > 0) {
    auto down = [&](void *dst, DevBuf *src, size_t bytes) {
      return hipMemcpyAsync(dst, src->p, bytes, hipMemcpyDeviceToHost, c->stream);
    };
    HIP_TRY(down(b->pos, e_pos, 8 * ne));
    HIP_TRY(down(b->kind, e_kind, ne));
    HIP_TRY(down(b->ref_len, e_rl, 4 * ne));
    HIP_TRY(down(b->alt_off, e_ao, 8 * ne));
    HIP_TRY(down(b->alt_len, e_al, 4 * ne));
    HIP_TRY(down(b->alt_bases, e_ab, (size_t)A));
    HIP_TRY(down(b->carriers, e_car, 8 * ne));
    HIP_TRY(down(b->gl, e_gl, 24 * ne));
    HIP_TRY(down(b->best, e_best, 4 * ne));
    HIP_TRY(down(b->ad_ref, e_adr, 4 * ne));
    HIP_TRY(down(b->ad_alt, e_ada, 4 * ne));
    HIP_TRY(down(b->dp, e_dp, 4 * ne));
    HIP_TRY(down(b->ev_flags, e_ef, ne));
  }
  HIP_TRY(hipEventRecord(span.b, c->stream));
  HIP_TRY(hipEventSynchronize(span.b));
  HIP_TRY(hipEventElapsedTime(&b->ms, span.a, span.b));
  HIP_TRY(hipEventElapsedTime(&b->events_ms, es.a, es.b));
  HIP_TRY(hipEventElapsedTime(&b->marginal_ms, ms.a, ms.b));
  *out = b;
  res.p = nullptr;
  return GQ_OK;
}

}  // extern "C"
