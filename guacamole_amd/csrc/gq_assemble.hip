// gq_assemble.hip — local assembly (gqpileup.h: gq_asm_*): the C ABI over the host twin and the path
// search (gq_assemble_host.h) and the device kernels (gq_assemble.h).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cstdlib>
#include <vector>

#include "../../include/gqpileup.h"
#include "gq_host.h"
#include "gq_assemble_host.h"
#include "gq_assemble.h"
#include "gq_winreads.h"

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

gq_status params_of(const gq_asm_params *params, gq_asm_params *p, const char *who) {
  if (params) *p = *params;
  else gq_asm::default_params(p);
  if (!gq_asm::valid(*p))
    return set_err(GQ_E_ARG,
                   "%s: k %d outside [%d, %d], or min_occurrence %d / max_paths %d / max_steps %lld below 1, or "
                   "max_path_length %d negative",
                   who, p->k, gq_asm::kMinK, gq_asm::kMaxK, p->min_occurrence, p->max_paths, (long long)p->max_steps,
                   p->max_path_length);
  return GQ_OK;
}

int32_t lds_slots() {  // the LDS table's slots: kLdsSlots, or GQ_ASM_LDS_SLOTS rounded down to a power of two
  int64_t s = asmk::kLdsSlots;
  if (const char *e = getenv("GQ_ASM_LDS_SLOTS")) {
    const int64_t v = atoll(e);
    s = 2;
    while (s * 2 <= v && s * 2 <= asmk::kLdsSlots) s *= 2;
  }
  return (int32_t)s;
}

constexpr int64_t kStageEntry = 8 + 8 + 4 + 1 + 1;  // bytes of a staged node
constexpr int64_t kTableSlot = 8 + 8 + 4;

int64_t lds_stage_entries(int64_t inst, int32_t slots) { return std::max<int64_t>(1, std::min<int64_t>(inst, slots)); }
int64_t glb_stage_entries(int64_t inst) { return asmk::pow2_ceil(std::max<int64_t>(inst, 1)); }
int64_t glb_table_slots(int64_t inst) { return asmk::pow2_ceil(std::max<int64_t>(2 * inst, 64)); }
int64_t scratch_of(bool lds, int64_t inst, int32_t slots) {
  return lds ? kStageEntry * lds_stage_entries(inst, slots)
             : kStageEntry * glb_stage_entries(inst) + kTableSlot * glb_table_slots(inst);
}

int64_t scratch_limit() {  // bytes of scratch one launch may use
  if (const char *e = getenv("GQ_ASM_SCRATCH_BYTES")) return std::max<int64_t>(atoll(e), 1);
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = (size_t)1 << 30;
  return (int64_t)(fr / 4);
}

struct Piece {  // the flat node arrays one launch downloaded
  std::vector<uint64_t> lo, hi;
  std::vector<int32_t> cnt;
  std::vector<uint8_t> cm, pm;
};

struct HostWin {  // where a window's nodes lie (pieces[piece], [at, at + n)) while the launches run
  int32_t piece = -1, n = 0;
  int64_t at = 0;
  int32_t source = -1, sink = -1, status = 0;
};

struct Run {  // what the launches share
  gq_ctx *c;
  DevReads R;
  asmk::RefView rv;
  asmk::Windows win;
  gq_asm_params p;
  const asmk::WinMeta *d_meta;
  const int64_t *d_list_read, *d_list_chunk;
  const std::vector<asmk::WinMeta> *meta;
  int32_t slots;
  std::vector<HostWin> *res;
  std::vector<Piece> pieces;
  float kernel_ms = 0.f;
  double ticks_count = 0, ticks_rest = 0;
  int32_t launches = 0;
};

// windows `ids` through asm_window_k<lds>; the ids whose table overflowed (lds only) go to `over`
gq_status launch(Run &r, bool lds, const std::vector<int64_t> &ids, std::vector<int64_t> *over) {
  gq_ctx *c = r.c;
  const size_t n = ids.size();
  if (!n) return GQ_OK;
  std::vector<int64_t> tab_off(n, 0), tab_slots(n, 0), stage_off(n, 0), stage_cap(n, 0);
  int64_t n_tab = 0, n_stage = 0;
  for (size_t j = 0; j < n; ++j) {
    const int64_t inst = (*r.meta)[(size_t)ids[j]].inst;
    stage_off[j] = n_stage;
    stage_cap[j] = lds ? lds_stage_entries(inst, r.slots) : glb_stage_entries(inst);
    n_stage += stage_cap[j];
    if (!lds) {
      tab_off[j] = n_tab;
      tab_slots[j] = glb_table_slots(inst);
      n_tab += tab_slots[j];
    }
  }
  Bufs bufs;
  DevBuf *d_ids = bufs.add(), *d_meta5 = bufs.add(), *d_tlo = bufs.add(), *d_thi = bufs.add(), *d_tcnt = bufs.add(),
         *d_slo = bufs.add(), *d_shi = bufs.add(), *d_scnt = bufs.add(), *d_scm = bufs.add(), *d_spm = bufs.add(),
         *d_out = bufs.add(), *d_ticks = bufs.add(), *d_noff = bufs.add();
  HIP_TRY(d_ids->ensure(8 * n));
  HIP_TRY(d_meta5->ensure(8 * 4 * n));
  const size_t ns = (size_t)n_stage, nt = (size_t)std::max<int64_t>(n_tab, 1);
  if (d_tlo->ensure(8 * nt) != hipSuccess || d_thi->ensure(8 * nt) != hipSuccess || d_tcnt->ensure(4 * nt) != hipSuccess ||
      d_slo->ensure(8 * ns) != hipSuccess || d_shi->ensure(8 * ns) != hipSuccess || d_scnt->ensure(4 * ns) != hipSuccess ||
      d_scm->ensure(ns) != hipSuccess || d_spm->ensure(ns) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(GQ_E_NOMEM, "assemble: %lld bytes of device scratch",
                   (long long)(kStageEntry * n_stage + kTableSlot * n_tab));
  }
  HIP_TRY(d_out->ensure(4 * 5 * n));
  HIP_TRY(d_ticks->ensure(16 * n));
  HIP_TRY(d_noff->ensure(8 * n));
  int64_t *m5 = (int64_t *)d_meta5->p;
  HIP_TRY(hipMemcpyAsync(d_ids->p, ids.data(), 8 * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(m5, tab_off.data(), 8 * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(m5 + n, tab_slots.data(), 8 * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(m5 + 2 * n, stage_off.data(), 8 * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(m5 + 3 * n, stage_cap.data(), 8 * n, hipMemcpyHostToDevice, c->stream));
  int32_t *o = (int32_t *)d_out->p;
  asmk::Launch L{};
  L.wid = (const int64_t *)d_ids->p;
  L.tab_off = m5;
  L.tab_slots = m5 + n;
  L.stage_off = m5 + 2 * n;
  L.stage_cap = m5 + 3 * n;
  L.tab_lo = (unsigned long long *)d_tlo->p;
  L.tab_hi = (unsigned long long *)d_thi->p;
  L.tab_cnt = (int *)d_tcnt->p;
  L.st_lo = (unsigned long long *)d_slo->p;
  L.st_hi = (unsigned long long *)d_shi->p;
  L.st_cnt = (int32_t *)d_scnt->p;
  L.st_cm = (uint8_t *)d_scm->p;
  L.st_pm = (uint8_t *)d_spm->p;
  L.n_nodes = o;
  L.ovf = o + n;
  L.source = o + 2 * n;
  L.sink = o + 3 * n;
  L.status = o + 4 * n;
  L.ticks = (unsigned long long *)d_ticks->p;
  L.lds_slots = r.slots;
  Span ks;
  HIP_TRY(ks.make());
  HIP_TRY(hipEventRecord(ks.a, c->stream));
  if (lds)
    hipLaunchKernelGGL(asmk::asm_window_k<true>, dim3((unsigned)n), dim3(asmk::kThreads), 0, c->stream, r.R, r.rv, r.win,
                       r.p.k, r.p.min_occurrence, r.d_meta, r.d_list_read, r.d_list_chunk, L);
  else
    hipLaunchKernelGGL(asmk::asm_window_k<false>, dim3((unsigned)n), dim3(asmk::kThreads), 0, c->stream, r.R, r.rv,
                       r.win, r.p.k, r.p.min_occurrence, r.d_meta, r.d_list_read, r.d_list_chunk, L);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ks.b, c->stream));
  ++r.launches;
  std::vector<int32_t> h_out(5 * n);
  std::vector<unsigned long long> h_ticks(2 * n);
  HIP_TRY(hipMemcpyAsync(h_out.data(), o, 4 * 5 * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(h_ticks.data(), d_ticks->p, 16 * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ks.a, ks.b));
  r.kernel_ms += ms;
  std::vector<int64_t> noff(n);
  int64_t total = 0;
  for (size_t j = 0; j < n; ++j) {
    noff[j] = total;
    total += h_out[j];
    r.ticks_count += (double)h_ticks[2 * j];
    r.ticks_rest += (double)h_ticks[2 * j + 1];
    if (h_out[n + j]) {
      if (!lds) return set_err(GQ_E_CAPACITY, "assemble: window %lld overflowed its global table", (long long)ids[j]);
      over->push_back(ids[j]);
    }
  }
  if (total > 0) {
    const size_t t = (size_t)total;
    DevBuf *f_lo = bufs.add(), *f_hi = bufs.add(), *f_cnt = bufs.add(), *f_cm = bufs.add(), *f_pm = bufs.add();
    HIP_TRY(f_lo->ensure(8 * t));
    HIP_TRY(f_hi->ensure(8 * t));
    HIP_TRY(f_cnt->ensure(4 * t));
    HIP_TRY(f_cm->ensure(t));
    HIP_TRY(f_pm->ensure(t));
    HIP_TRY(hipMemcpyAsync(d_noff->p, noff.data(), 8 * n, hipMemcpyHostToDevice, c->stream));
    const asmk::Flat f{(unsigned long long *)f_lo->p, (unsigned long long *)f_hi->p, (int32_t *)f_cnt->p,
                       (uint8_t *)f_cm->p, (uint8_t *)f_pm->p};
    hipLaunchKernelGGL(asmk::asm_gather_k, dim3((unsigned)n), dim3(256), 0, c->stream, L, (const int64_t *)d_noff->p, f);
    HIP_TRY(hipGetLastError());
    r.pieces.emplace_back();  // kept until the block is filled: each window's nodes are copied once, from here
    Piece &pc = r.pieces.back();
    pc.lo.resize(t);
    pc.hi.resize(t);
    pc.cnt.resize(t);
    pc.cm.resize(t);
    pc.pm.resize(t);
    HIP_TRY(hipMemcpyAsync(pc.lo.data(), f.lo, 8 * t, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(pc.hi.data(), f.hi, 8 * t, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(pc.cnt.data(), f.cnt, 4 * t, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(pc.cm.data(), f.cm, t, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(pc.pm.data(), f.pm, t, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t j = 0; j < n; ++j) {
      if (h_out[n + j]) continue;
      HostWin &hw = (*r.res)[(size_t)ids[j]];
      hw.piece = (int32_t)(r.pieces.size() - 1);
      hw.at = noff[j];
      hw.n = h_out[j];
    }
  }
  for (size_t j = 0; j < n; ++j) {
    if (h_out[n + j]) continue;
    HostWin &hw = (*r.res)[(size_t)ids[j]];
    hw.source = h_out[2 * n + j];
    hw.sink = h_out[3 * n + j];
    hw.status = h_out[4 * n + j];
  }
  return GQ_OK;
}

// `ids` in consecutive pieces whose scratch fits the limit (a piece holds at least one window)
gq_status launch_chunked(Run &r, bool lds, const std::vector<int64_t> &ids, int64_t limit, std::vector<int64_t> *over) {
  std::vector<int64_t> piece;
  int64_t used = 0;
  gq_status s;
  for (int64_t w : ids) {
    const int64_t need = scratch_of(lds, (*r.meta)[(size_t)w].inst, r.slots);
    if (!piece.empty() && (used + need > limit || piece.size() >= ((size_t)1 << 30))) {
      if ((s = launch(r, lds, piece, over))) return s;
      piece.clear();
      used = 0;
    }
    piece.push_back(w);
    used += need;
  }
  return launch(r, lds, piece, over);
}

}  // namespace

namespace gq {

gq_status find_window_reads(gq_ctx *c, const gq_dev_reads *d, int64_t W, const int32_t *contig, const int32_t *start,
                            const int32_t *end, int32_t k, int32_t min_mapq, const char *who, WindowReads &out) {
  out.W = W;
  const size_t w1 = (size_t)W + 1;
  DevBuf *d_win = &out.win, *d_cnt = &out.cnt, *d_coff = &out.coff, *d_ra = &out.ra, *d_tmp = &out.tmp;
  HIP_TRY(d_win->ensure(4 * 3 * (size_t)W));
  HIP_TRY(d_cnt->ensure(8 * w1));
  HIP_TRY(d_coff->ensure(8 * w1));
  HIP_TRY(d_ra->ensure(8 * (size_t)W));
  int32_t *dw = (int32_t *)d_win->p;
  HIP_TRY(hipMemcpyAsync(dw, contig, 4 * (size_t)W, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(dw + W, start, 4 * (size_t)W, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(dw + 2 * W, end, 4 * (size_t)W, hipMemcpyHostToDevice, c->stream));
  const asmk::Windows win{dw, dw + W, dw + 2 * W};
  hipLaunchKernelGGL(asmk::asm_range_k, dim3((unsigned)((W + 1 + 255) / 256)), dim3(256), 0, c->stream, d->d, W, win,
                     (int64_t *)d_cnt->p, (int64_t *)d_ra->p);
  HIP_TRY(hipGetLastError());
  size_t tb = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (const int64_t *)d_cnt->p, (int64_t *)d_coff->p, (int)w1,
                                           c->stream));
  HIP_TRY(d_tmp->ensure(tb));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp->p, tb, (const int64_t *)d_cnt->p, (int64_t *)d_coff->p, (int)w1,
                                           c->stream));
  int64_t C = 0;
  HIP_TRY(hipMemcpyAsync(&C, (const int64_t *)d_coff->p + W, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (C + 1 >= ((int64_t)1 << 31))
    return set_err(GQ_E_CAPACITY, "%s: %lld candidate reads over the windows of one call", who, (long long)C);
  out.C = C;
  const size_t c1 = (size_t)C + 1;
  DevBuf *d_flag = &out.flag, *d_inst = &out.inst, *d_chunks = &out.chunks, *d_fsum = &out.fsum, *d_isum = &out.isum,
         *d_csum = &out.csum, *d_lr = &out.list_read, *d_lc = &out.list_chunk;
  for (DevBuf *b : {d_flag, d_inst, d_chunks, d_fsum, d_isum, d_csum, d_lr, d_lc}) HIP_TRY(b->ensure(8 * c1));
  hipLaunchKernelGGL(asmk::asm_test_k, dim3((unsigned)((c1 + 255) / 256)), dim3(256), 0, c->stream, d->d, W, win, k,
                     min_mapq, (const int64_t *)d_coff->p, (const int64_t *)d_ra->p, C, (int64_t *)d_flag->p, (int64_t *)d_inst->p,
                     (int64_t *)d_chunks->p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (const int64_t *)d_flag->p, (int64_t *)d_fsum->p, (int)c1,
                                           c->stream));
  HIP_TRY(d_tmp->ensure(tb));
  for (auto io : {std::make_pair(d_flag, d_fsum), std::make_pair(d_inst, d_isum), std::make_pair(d_chunks, d_csum)})
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp->p, tb, (const int64_t *)io.first->p, (int64_t *)io.second->p,
                                             (int)c1, c->stream));
  if (C > 0) {
    hipLaunchKernelGGL(asmk::asm_compact_k, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, c->stream, W,
                       (const int64_t *)d_coff->p, (const int64_t *)d_ra->p, C, (const int64_t *)d_flag->p,
                       (const int64_t *)d_fsum->p, (const int64_t *)d_csum->p, (int64_t *)d_lr->p, (int64_t *)d_lc->p);
    HIP_TRY(hipGetLastError());
  }
  return GQ_OK;
}

}  // namespace gq

extern "C" {

void gq_asm_default_params(gq_asm_params *out) {
  if (out) gq_asm::default_params(out);
}

void gq_asm_limits(int32_t out[8]) {
  if (!out) return;
  const int32_t v[8] = {gq_asm::kMinK, gq_asm::kMaxK,   gq_asm::kWordBases, lds_slots(),
                        asmk::kLdsSlots, asmk::kThreads, asmk::kLdsBytes,    0};
  memcpy(out, v, sizeof(v));
}

void gq_asm_free_graphs(gq_asm_graph_block *g) { gq_asm::free_graphs(g); }
void gq_asm_free_paths(gq_asm_path_block *p) { gq_asm::free_paths(p); }

gq_status gq_asm_graphs_host(int64_t n_windows, const uint8_t *seq_pool, const int64_t *seq_off, const int32_t *seq_len,
                             const int64_t *win_read_off, const int64_t *win_reads, const uint8_t *ref_pool,
                             const int64_t *ref_off, const int32_t *win_len, const gq_asm_params *params,
                             int32_t threads, gq_asm_graph_block **out) {
  if (n_windows < 0 || !out) return set_err(GQ_E_ARG, "gq_asm_graphs_host: null or negative argument");
  gq_asm_params p;
  gq_status s;
  if ((s = params_of(params, &p, "gq_asm_graphs_host"))) return s;
  if (n_windows > 0 && (!win_read_off || !ref_off || !win_len))
    return set_err(GQ_E_ARG, "gq_asm_graphs_host: null array");
  for (int64_t w = 0; w < n_windows; ++w) {
    if (win_len[w] < 0 || win_read_off[w + 1] < win_read_off[w] || win_read_off[w] < 0)
      return set_err(GQ_E_ARG, "gq_asm_graphs_host: window %lld has a negative length or read list", (long long)w);
    if (win_read_off[w + 1] > win_read_off[w] && (!seq_pool || !seq_off || !seq_len || !win_reads))
      return set_err(GQ_E_ARG, "gq_asm_graphs_host: null read arrays");
    if (ref_off[w] >= 0 && !ref_pool) return set_err(GQ_E_ARG, "gq_asm_graphs_host: null reference pool");
  }
  if (gq_asm::graphs_host(n_windows, seq_pool, seq_off, seq_len, win_read_off, win_reads, ref_pool, ref_off, win_len, p,
                          threads, out))
    return set_err(GQ_E_NOMEM, "gq_asm_graphs_host: result block");
  return GQ_OK;
}

gq_status gq_asm_paths(const gq_asm_graph_block *graphs, const gq_asm_params *params, gq_asm_path_block **out) {
  if (!graphs || !out) return set_err(GQ_E_ARG, "gq_asm_paths: null argument");
  gq_asm_params p;
  if (params) p = *params;
  else gq_asm::default_params(&p);
  p.k = graphs->k;
  p.min_occurrence = graphs->min_occurrence;
  gq_status s;
  if ((s = params_of(&p, &p, "gq_asm_paths"))) return s;
  const auto t0 = std::chrono::steady_clock::now();
  if (gq_asm::paths_host(graphs, p, out)) return set_err(GQ_E_NOMEM, "gq_asm_paths: result block");
  (*out)->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return GQ_OK;
}

gq_status gq_asm_graphs(gq_ctx *c, const gq_dev_reads *d, const gq_reference *ref, int64_t W, const int32_t *contig,
                        const int32_t *start, const int32_t *end, const gq_asm_params *params,
                        gq_asm_graph_block **out) {
  if (!c || !d || !ref || !out || W < 0) return set_err(GQ_E_ARG, "gq_asm_graphs: null or negative argument");
  if (d->ctx != c) return set_err(GQ_E_ARG, "gq_asm_graphs: the read set belongs to another context");
  if (ref->n_contigs != d->d.n_contigs)
    return set_err(GQ_E_ARG, "reference covers %d contigs, the read set %d", ref->n_contigs, d->d.n_contigs);
  if (ref->device != c->device) return set_err(GQ_E_ARG, "reference uploaded to another device");
  gq_asm_params p;
  gq_status s;
  if ((s = params_of(params, &p, "gq_asm_graphs"))) return s;
  if (W > 0 && (!contig || !start || !end)) return set_err(GQ_E_ARG, "gq_asm_graphs: null array");
  if (W + 1 >= ((int64_t)1 << 31)) return set_err(GQ_E_CAPACITY, "gq_asm_graphs: %lld windows in one call", (long long)W);
  for (int64_t w = 0; w < W; ++w)
    if (contig[w] < 0 || contig[w] >= d->d.n_contigs || start[w] < 0 || end[w] < start[w])
      return set_err(GQ_E_ARG, "gq_asm_graphs: window %lld: contig %d, [%d, %d)", (long long)w, contig[w], start[w],
                     end[w]);
  if (W == 0) {
    gq_asm_graph_block *g = gq_asm::new_graphs(0, 0);
    if (!g) return set_err(GQ_E_NOMEM, "gq_asm_graphs: result block");
    g->k = p.k;
    g->min_occurrence = p.min_occurrence;
    *out = g;
    return GQ_OK;
  }
  if ((s = validation_wait(d))) return s;
  HIP_TRY(hipSetDevice(c->device));
  Span span, rs;
  HIP_TRY(span.make());
  HIP_TRY(rs.make());
  HIP_TRY(hipEventRecord(span.a, c->stream));
  HIP_TRY(hipEventRecord(rs.a, c->stream));
  WindowReads wr;
  if ((s = find_window_reads(c, d, W, contig, start, end, p.k, p.min_mapq, "gq_asm_graphs", wr))) return s;
  Bufs bufs;
  DevBuf *d_meta = bufs.add();
  HIP_TRY(d_meta->ensure(sizeof(asmk::WinMeta) * (size_t)W));
  const asmk::Windows win{wr.contig(), wr.start(), wr.end()};
  DevBuf *d_coff = &wr.coff, *d_fsum = &wr.fsum, *d_isum = &wr.isum, *d_csum = &wr.csum, *d_lr = &wr.list_read,
         *d_lc = &wr.list_chunk;
  hipLaunchKernelGGL(asmk::asm_meta_k, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, c->stream, W,
                     (const int64_t *)d_coff->p, (const int64_t *)d_fsum->p, (const int64_t *)d_isum->p,
                     (const int64_t *)d_csum->p, (asmk::WinMeta *)d_meta->p);
  HIP_TRY(hipGetLastError());
  std::vector<asmk::WinMeta> meta((size_t)W);
  HIP_TRY(hipMemcpyAsync(meta.data(), d_meta->p, sizeof(asmk::WinMeta) * (size_t)W, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipEventRecord(rs.b, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));

  std::vector<HostWin> res((size_t)W);
  Run r{};
  r.c = c;
  r.R = d->d;
  r.rv = asmk::RefView{(const uint8_t *)ref->bytes, ref->d_off, ref->d_len};
  r.win = win;
  r.p = p;
  r.d_meta = (const asmk::WinMeta *)d_meta->p;
  r.d_list_read = (const int64_t *)d_lr->p;
  r.d_list_chunk = (const int64_t *)d_lc->p;
  r.meta = &meta;
  r.slots = lds_slots();
  r.res = &res;
  const int64_t limit = scratch_limit();
  std::vector<int64_t> all((size_t)W), over;
  for (int64_t w = 0; w < W; ++w) all[(size_t)w] = w;
  if ((s = launch_chunked(r, true, all, limit, &over)) || (s = launch_chunked(r, false, over, limit, nullptr))) {
    (void)hipStreamSynchronize(c->stream);
    return s;
  }
  int64_t N = 0;
  for (const HostWin &x : res) N += x.n;
  gq_asm_graph_block *g = gq_asm::new_graphs(W, N);
  if (!g) return set_err(GQ_E_NOMEM, "gq_asm_graphs: result block");
  int64_t at = 0;
  for (int64_t w = 0; w < W; ++w) {
    const HostWin &x = res[(size_t)w];
    const size_t n = (size_t)x.n;
    g->node_off[w] = at;
    if (n) {
      const Piece &pc = r.pieces[(size_t)x.piece];
      memcpy(g->key_lo + at, pc.lo.data() + x.at, 8 * n);
      memcpy(g->key_hi + at, pc.hi.data() + x.at, 8 * n);
      memcpy(g->count + at, pc.cnt.data() + x.at, 4 * n);
      memcpy(g->child_mask + at, pc.cm.data() + x.at, n);
      memcpy(g->parent_mask + at, pc.pm.data() + x.at, n);
    }
    at += (int64_t)n;
    g->source[w] = x.source;
    g->sink[w] = x.sink;
    g->status[w] = x.status;
    g->n_reads[w] = (int32_t)(meta[(size_t)w].l1 - meta[(size_t)w].l0);
    g->win_len[w] = end[w] - start[w];
    g->n_instances[w] = meta[(size_t)w].inst;
  }
  g->node_off[W] = at;
  g->k = p.k;
  g->min_occurrence = p.min_occurrence;
  g->launches = r.launches;
  g->n_global = (int32_t)over.size();
  const double tt = r.ticks_count + r.ticks_rest;
  g->count_ms = tt > 0 ? (float)(r.kernel_ms * (r.ticks_count / tt)) : 0.f;
  g->edges_ms = r.kernel_ms - g->count_ms;
  if (hipEventRecord(span.b, c->stream) != hipSuccess || hipEventSynchronize(span.b) != hipSuccess ||
      hipEventElapsedTime(&g->ms, span.a, span.b) != hipSuccess ||
      hipEventElapsedTime(&g->reads_ms, rs.a, rs.b) != hipSuccess) {
    gq_asm::free_graphs(g);
    return set_err(GQ_E_HIP, "gq_asm_graphs: reading the spans failed");
  }
  *out = g;
  return GQ_OK;
}

}  // extern "C"
