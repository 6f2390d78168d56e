// gq_structural.h — structural-variant (gqpileup.h: gq_sv_*): large deletions from discordant
// read pairs (StructuralVariantCaller.scala).  Included by gq_bamdev.hip, whose record list and
// byte readers it uses.  The device stages:
//   pair_keep / pair_fill   lane / record: the 36 fixed bytes; paired, mapped (rec_parse's
//                           isMapped), first in pair, not a duplicate, mate mapped, tlen != 0;
//                           the kept pairs in file order as a resident SoA
//   sv_in_range             lane / pair: contig == mate_contig, strands differ, raw tlen < 25000
//   sv_oriented             the in-range pairs' oriented sizes, compacted (then a radix sort)
//   sv_median / sv_resid / sv_final   the doubled median 2m (an integer) from the sorted sizes,
//                           the doubled residuals |2x - 2m| (then a second sort), median, MAD and
//                           max_normal = (int)(median + 5 MAD): every value is a multiple of 1/4
//                           below 2^36, so the doubles are exact
//   sv_exceptional / sv_node_keys / sv_nodes   in range and raw tlen > threshold, compacted in
//                           file order, sorted by (contig, lo) (a stable radix sort), gathered
//   sv_edges<FILL>          wave / node i: successors 64 at a time; a ballot finds the first
//                           lane that ends the walk (another contig, the list's end, or
//                           |GapMin_j - Min_i| > N) and the lanes before it test compatibility;
//                           a counting pass, an exclusive sum, a filling pass
// The cliques are the host's (gq_sv_clique.h).
#pragma once
#include "gq_sv_clique.h"

namespace {

constexpr int32_t kSvMaxInsert = 25000;  // StructuralVariant.MAX_INSERT_SIZE

struct SvPairs {  // device SoA of n pairs
  int32_t *contig, *start, *mate_contig, *mate_start, *tlen, *len;
  uint8_t *strand;
};

__device__ __forceinline__ bool pair_kept(const uint8_t *p, int32_t n_ref) {
  const int32_t ref_id = (int32_t)ld32(p), pos = (int32_t)ld32(p + 4), tlen = (int32_t)ld32(p + 28);
  const uint32_t flag = ld16(p + 14);
  const bool mapped = !((flag & 0x4) || ref_id < 0) && pos >= 0 && ref_id < n_ref;  // (rec_parse)
  return mapped && (flag & 0x1) && (flag & 0x40) && !(flag & 0x8) && !(flag & 0x400) && tlen != 0;
}

__global__ void __launch_bounds__(256) pair_keep(const uint8_t *d, const int64_t *rec, int64_t n_rec, int32_t n_ref,
                                                 int64_t *keep) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > n_rec) return;
  keep[r] = r < n_rec && pair_kept(d + rec[r] + 4, n_ref) ? 1 : 0;  // (keep[n_rec] = 0: the scan's total)
}

__global__ void __launch_bounds__(256) pair_fill(const uint8_t *d, const int64_t *rec, int64_t n_rec, int32_t n_ref,
                                                 const int64_t *kidx, SvPairs P) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rec) return;
  const uint8_t *p = d + rec[r] + 4;
  if (!pair_kept(p, n_ref)) return;
  const int64_t k = kidx[r];
  const uint32_t flag = ld16(p + 14);
  P.contig[k] = (int32_t)ld32(p);
  P.start[k] = (int32_t)ld32(p + 4);
  P.len[k] = (int32_t)ld32(p + 16);
  P.mate_contig[k] = (int32_t)ld32(p + 20);
  P.mate_start[k] = (int32_t)ld32(p + 24);
  P.tlen[k] = (int32_t)ld32(p + 28);
  P.strand[k] = (uint8_t)(((flag >> 4) & 1u) | (((flag >> 5) & 1u) << 1));
}

__device__ __forceinline__ bool sv_pair_in_range(const SvPairs &P, int64_t k) {
  const uint32_t s = P.strand[k];
  return P.contig[k] == P.mate_contig[k] && ((s & 1u) != ((s >> 1) & 1u)) && P.tlen[k] < kSvMaxInsert;
}

__global__ void __launch_bounds__(256) sv_in_range(SvPairs P, int64_t n, int64_t *flag) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > n) return;
  flag[k] = k < n && sv_pair_in_range(P, k) ? 1 : 0;
}

__global__ void __launch_bounds__(256) sv_oriented(SvPairs P, int64_t n, const int64_t *flag, const int64_t *at,
                                                   int32_t *sizes) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n || !flag[k]) return;
  const uint32_t t = (uint32_t)P.tlen[k];
  sizes[at[k]] = (int32_t)((P.strand[k] & 1u) ? 0u - t : t);  // (Int negation: INT_MIN stays)
}

struct SvStatsDev {
  int64_t median2;  // twice the median
  double median, mad;
  int32_t max_normal, pad;
};

__global__ void sv_median(const int32_t *sorted, int64_t n, SvStatsDev *st) {
  if (threadIdx.x || blockIdx.x) return;
  int64_t m2 = 0;
  if (n > 0) m2 = (n & 1) ? 2 * (int64_t)sorted[n / 2] : (int64_t)sorted[n / 2 - 1] + (int64_t)sorted[n / 2];
  st->median2 = m2;
}

__global__ void __launch_bounds__(256) sv_resid(const int32_t *sorted, int64_t n, const SvStatsDev *st, int64_t *res) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int64_t v = 2 * (int64_t)sorted[k] - st->median2;
  res[k] = v < 0 ? -v : v;
}

__global__ void sv_final(const int64_t *res_sorted, int64_t n, SvStatsDev *st) {
  if (threadIdx.x || blockIdx.x) return;
  double median = 0.0, mad = 0.0;
  if (n > 0) {
    median = 0.5 * (double)st->median2;
    // doubled residuals d: a residual is d / 2, the mean of two (d1 + d2) / 4
    mad = (n & 1) ? 0.5 * (double)res_sorted[n / 2] : 0.25 * (double)(res_sorted[n / 2 - 1] + res_sorted[n / 2]);
  }
  const double x = median + 5.0 * mad;
  st->median = median;
  st->mad = mad;
  // Double.toInt: toward zero, saturating
  st->max_normal = x >= 2147483647.0 ? 2147483647 : x <= -2147483648.0 ? (int32_t)(-2147483647 - 1) : (int32_t)x;
}

// thr: the threshold (host value), or null: st->max_normal
__global__ void __launch_bounds__(256) sv_exceptional(SvPairs P, int64_t n, const SvStatsDev *st, int32_t thr,
                                                      int use_st, int64_t *flag) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > n) return;
  const int32_t t = use_st ? st->max_normal : thr;
  flag[k] = k < n && sv_pair_in_range(P, k) && P.tlen[k] > t ? 1 : 0;
}

__global__ void __launch_bounds__(256) sv_node_keys(SvPairs P, int64_t n, const int64_t *flag, const int64_t *at,
                                                    uint64_t *key, int64_t *src) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n || !flag[k]) return;
  const int32_t lo = min(P.start[k], P.mate_start[k]);
  // (contig, lo) as one unsigned key: both signed, so their sign bits are flipped
  key[at[k]] = ((uint64_t)((uint32_t)P.contig[k] ^ 0x80000000u) << 32) | (uint64_t)((uint32_t)lo ^ 0x80000000u);
  src[at[k]] = k;
}

struct SvNodes {  // device SoA of the node set, (contig, lo) order
  int32_t *contig, *lo, *hi, *len;
  int64_t *pair;
};

__global__ void __launch_bounds__(256) sv_nodes(SvPairs P, const int64_t *src, int64_t n, SvNodes N) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t k = src[i];
  const int32_t a = P.start[k], b = P.mate_start[k];
  N.contig[i] = P.contig[k];
  N.lo[i] = min(a, b);
  N.hi[i] = max(a, b);
  N.len[i] = P.len[k];
  N.pair[i] = k;
}

// One wave per node i.  FILL = false: cnt[i] = its edges.  FILL = true: they go to
// [off[i], off[i + 1]) in successor order.  Both passes evaluate the same predicates, so the
// fill stays inside the counted range.
template <bool FILL>
__global__ void __launch_bounds__(256) sv_edges(SvNodes V, int64_t n, int64_t N, int64_t *cnt, const int64_t *off,
                                                int32_t *ei, int32_t *ej, int64_t *ew) {
  const int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= n) return;  // (wave-uniform)
  const int32_t ci = V.contig[i];
  const int64_t min_i = V.lo[i], gmax_i = V.hi[i], len_i = V.len[i];
  const int64_t max_i = gmax_i + len_i;
  int64_t made = 0;
  const int64_t base = FILL ? off[i] : 0;
  for (int64_t j0 = i + 1; j0 < n; j0 += 64) {
    const int64_t j = j0 + lane;
    bool stop = true, edge = false;
    int64_t wgt = 0;
    if (j < n && V.contig[j] == ci) {
      const int64_t min_j = V.lo[j], gmax_j = V.hi[j], len_j = V.len[j];
      const int64_t gmin_j = min_j + len_j, max_j = gmax_j + len_j;
      const int64_t dist = gmin_j - min_i;
      stop = (dist < 0 ? -dist : dist) > N;
      const bool bad = dist > N || (gmax_j < gmax_i && max_i - gmax_j > N) || (gmax_j >= gmax_i && max_j - gmax_i > N) ||
                       gmax_i < min_j || gmax_j < min_i;
      edge = !bad;
      const int64_t dw = (gmax_j - min_j) - (gmax_i - min_i);
      wgt = dw < 0 ? -dw : dw;
    }
    const unsigned long long sm = __ballot(stop);
    const int first = sm ? __builtin_ctzll(sm) : 64;  // lanes at or past it are out
    edge = edge && lane < first;
    const unsigned long long em = __ballot(edge);
    if (FILL && edge) {
      const int64_t at = base + made + __popcll(em & ((1ull << lane) - 1ull));
      ei[at] = (int32_t)i;
      ej[at] = (int32_t)j;
      ew[at] = wgt;
    }
    made += __popcll(em);
    if (sm) break;
  }
  if (!FILL && lane == 0) cnt[i] = made;
}

}  // namespace

struct gq_sv_pairs {
  gq_ctx *ctx = nullptr;
  int64_t n = 0;
  DevBuf contig, start, mate_contig, mate_start, tlen, len, strand;
  // the node set (gq_sv_stats_call / gq_sv_select)
  bool selected = false;
  int64_t n_nodes = 0;
  DevBuf n_contig, n_lo, n_hi, n_len, n_pair;
  SvPairs view() const {
    return SvPairs{(int32_t *)contig.p, (int32_t *)start.p, (int32_t *)mate_contig.p, (int32_t *)mate_start.p,
                   (int32_t *)tlen.p,   (int32_t *)len.p,   (uint8_t *)strand.p};
  }
  SvNodes nodes() const {
    return SvNodes{(int32_t *)n_contig.p, (int32_t *)n_lo.p, (int32_t *)n_hi.p, (int32_t *)n_len.p, (int64_t *)n_pair.p};
  }
  gq_status alloc(int64_t k) {
    const size_t m = (size_t)std::max<int64_t>(k, 1);
    for (DevBuf *x : {&contig, &start, &mate_contig, &mate_start, &tlen, &len}) HIP_TRY(x->ensure(sizeof(int32_t) * m));
    HIP_TRY(strand.ensure(m));
    n = k;
    return GQ_OK;
  }
  ~gq_sv_pairs() {
    for (DevBuf *x : {&contig, &start, &mate_contig, &mate_start, &tlen, &len, &strand, &n_contig, &n_lo, &n_hi, &n_len,
                      &n_pair})
      x->release();
  }
};

namespace {

constexpr int64_t kSvMaxPairs = (int64_t)1 << 30;  // the scans and sorts count in 32 bits

struct SvSpan {  // a device span between two events of its own
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t s = nullptr;
  hipError_t begin(hipStream_t st) {
    s = st;
    hipError_t e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    if (e == hipSuccess) e = hipEventRecord(a, s);
    return e;
  }
  hipError_t end(float *ms) {
    hipError_t e = hipEventRecord(b, s);
    if (e == hipSuccess) e = hipEventSynchronize(b);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, a, b);
    return e;
  }
  ~SvSpan() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

// the node set of p: pairs flagged by sv_exceptional (st's max_normal, or thr), in (contig, lo) order
gq_status sv_select(gq_sv_pairs *p, const SvStatsDev *st, int32_t thr, DevBuf &flag, DevBuf &at, DevBuf &tmp) {
  gq_ctx *c = p->ctx;
  const int64_t n = p->n;
  p->selected = false;
  hipLaunchKernelGGL(sv_exceptional, dim3(grid(n + 1, 256)), dim3(256), 0, c->stream, p->view(), n, st, thr,
                     st ? 1 : 0, (int64_t *)flag.p);
  HIP_TRY(hipGetLastError());
  gq_status s;
  if ((s = exclusive_sum(c, (const int64_t *)flag.p, (int64_t *)at.p, n + 1, tmp))) return s;
  int64_t k = 0;
  if ((s = d2h_i64(c, (const int64_t *)at.p + n, &k))) return s;
  const size_t m = (size_t)std::max<int64_t>(k, 1);
  DevBuf key, key2, src, src2;
  for (DevBuf *x : {&key, &key2, &src, &src2}) HIP_TRY(x->ensure(8 * m));
  for (DevBuf *x : {&p->n_contig, &p->n_lo, &p->n_hi, &p->n_len}) HIP_TRY(x->ensure(sizeof(int32_t) * m));
  HIP_TRY(p->n_pair.ensure(sizeof(int64_t) * m));
  if (k) {
    hipLaunchKernelGGL(sv_node_keys, dim3(grid(n, 256)), dim3(256), 0, c->stream, p->view(), n, (const int64_t *)flag.p,
                       (const int64_t *)at.p, (uint64_t *)key.p, (int64_t *)src.p);
    HIP_TRY(hipGetLastError());
    size_t tb = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const uint64_t *)key.p, (uint64_t *)key2.p,
                                               (const int64_t *)src.p, (int64_t *)src2.p, (int)k, 0, 64, c->stream));
    HIP_TRY(tmp.ensure(tb));
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, (const uint64_t *)key.p, (uint64_t *)key2.p,
                                               (const int64_t *)src.p, (int64_t *)src2.p, (int)k, 0, 64, c->stream));
    hipLaunchKernelGGL(sv_nodes, dim3(grid(k, 256)), dim3(256), 0, c->stream, p->view(), (const int64_t *)src2.p, k,
                       p->nodes());
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (DevBuf *x : {&key, &key2, &src, &src2}) x->release();
  p->n_nodes = k;
  p->selected = true;
  return GQ_OK;
}

gq_sv_cliques *sv_cliques_out(const std::vector<gq_sv::Clique> &v) {
  const size_t n = v.size(), m = std::max<size_t>(n, 1);
  gq_sv_cliques *o = new gq_sv_cliques();
  o->n = (int64_t)n;
  o->contig = new int32_t[m];
  o->start = new int64_t[m];
  o->stop = new int64_t[m];
  o->pairs = new int64_t[m];
  o->wiggle = new int64_t[m];
  for (size_t k = 0; k < n; ++k) {
    o->contig[k] = v[k].contig;
    o->start[k] = v[k].start;
    o->stop[k] = v[k].stop;
    o->pairs[k] = v[k].pairs;
    o->wiggle[k] = v[k].wiggle;
  }
  return o;
}

}  // namespace

extern "C" {

gq_status gq_sv_pairs_from_bam(gq_bam_dev *b, gq_sv_pairs **out, float *parse_ms) {
  if (!b || !out) return set_err(GQ_E_ARG, "gq_sv_pairs_from_bam: null argument");
  if (!b->ctx || !b->out.p) return set_err(GQ_E_ARG, "gq_sv_pairs_from_bam before gq_bam_dev_load");
  gq_ctx *c = b->ctx;
  HIP_TRY(hipSetDevice(c->device));
  int64_t n_rec = 0;
  gq_status s;
  if ((s = record_list(b, &n_rec))) return s;
  if (n_rec >= kSvMaxPairs) return set_err(GQ_E_CAPACITY, "structural-variant: %lld records in one load", (long long)n_rec);
  const uint8_t *d = (const uint8_t *)b->out.p;
  const int32_t n_ref = (int32_t)b->names.size();
  SvSpan span;
  HIP_TRY(span.begin(c->stream));
  DevBuf keep, kidx, tmp;
  HIP_TRY(keep.ensure(sizeof(int64_t) * (size_t)(n_rec + 1)));
  HIP_TRY(kidx.ensure(sizeof(int64_t) * (size_t)(n_rec + 1)));
  hipLaunchKernelGGL(pair_keep, dim3(grid(n_rec + 1, 256)), dim3(256), 0, c->stream, d, (const int64_t *)b->rec.p, n_rec,
                     n_ref, (int64_t *)keep.p);
  HIP_TRY(hipGetLastError());
  if ((s = exclusive_sum(c, (const int64_t *)keep.p, (int64_t *)kidx.p, n_rec + 1, tmp))) return s;
  int64_t k = 0;
  if ((s = d2h_i64(c, (const int64_t *)kidx.p + n_rec, &k))) return s;
  std::unique_ptr<gq_sv_pairs> p(new gq_sv_pairs());
  p->ctx = c;
  if ((s = p->alloc(k))) return s;
  if (k) {
    hipLaunchKernelGGL(pair_fill, dim3(grid(n_rec, 256)), dim3(256), 0, c->stream, d, (const int64_t *)b->rec.p, n_rec,
                       n_ref, (const int64_t *)kidx.p, p->view());
    HIP_TRY(hipGetLastError());
  }
  float ms = 0.f;
  HIP_TRY(span.end(&ms));
  if (parse_ms) *parse_ms = ms;
  for (DevBuf *x : {&keep, &kidx, &tmp}) x->release();
  *out = p.release();
  return GQ_OK;
}

gq_status gq_sv_pairs_from_host(gq_ctx *c, int64_t n, const int32_t *contig, const int32_t *start,
                                const int32_t *mate_contig, const int32_t *mate_start, const int32_t *tlen,
                                const int32_t *len, const uint8_t *strand, gq_sv_pairs **out) {
  if (!c || !out || n < 0 || (n > 0 && (!contig || !start || !mate_contig || !mate_start || !tlen || !len || !strand)))
    return set_err(GQ_E_ARG, "gq_sv_pairs_from_host: null argument");
  if (n >= kSvMaxPairs) return set_err(GQ_E_CAPACITY, "structural-variant: %lld pairs in one call", (long long)n);
  HIP_TRY(hipSetDevice(c->device));
  std::unique_ptr<gq_sv_pairs> p(new gq_sv_pairs());
  p->ctx = c;
  gq_status s;
  if ((s = p->alloc(n))) return s;
  if (n) {
    const std::pair<DevBuf *, const void *> cols[] = {{&p->contig, contig},         {&p->start, start},
                                                      {&p->mate_contig, mate_contig}, {&p->mate_start, mate_start},
                                                      {&p->tlen, tlen},             {&p->len, len}};
    for (const auto &x : cols)
      HIP_TRY(hipMemcpyAsync(x.first->p, x.second, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(p->strand.p, strand, (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  *out = p.release();
  return GQ_OK;
}

int64_t gq_sv_pairs_count(const gq_sv_pairs *p) { return p ? p->n : -1; }

gq_status gq_sv_pairs_download(const gq_sv_pairs *p, int32_t *contig, int32_t *start, int32_t *mate_contig,
                               int32_t *mate_start, int32_t *tlen, int32_t *len, uint8_t *strand) {
  if (!p) return set_err(GQ_E_ARG, "gq_sv_pairs_download: null argument");
  if (!p->n) return GQ_OK;
  gq_ctx *c = p->ctx;
  HIP_TRY(hipSetDevice(c->device));
  const std::pair<void *, const DevBuf *> cols[] = {{contig, &p->contig},         {start, &p->start},
                                                    {mate_contig, &p->mate_contig}, {mate_start, &p->mate_start},
                                                    {tlen, &p->tlen},             {len, &p->len}};
  for (const auto &x : cols)
    if (x.first)
      HIP_TRY(hipMemcpyAsync(x.first, x.second->p, sizeof(int32_t) * (size_t)p->n, hipMemcpyDeviceToHost, c->stream));
  if (strand) HIP_TRY(hipMemcpyAsync(strand, p->strand.p, (size_t)p->n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GQ_OK;
}

void gq_sv_pairs_free(gq_sv_pairs *p) { delete p; }

gq_status gq_sv_stats_call(gq_sv_pairs *p, gq_sv_stats *out) {
  if (!p || !out) return set_err(GQ_E_ARG, "gq_sv_stats_call: null argument");
  gq_ctx *c = p->ctx;
  HIP_TRY(hipSetDevice(c->device));
  const int64_t n = p->n;
  gq_status s;
  DevBuf flag, at, tmp, sizes, sorted, res, res2, st;
  HIP_TRY(flag.ensure(sizeof(int64_t) * (size_t)(n + 1)));
  HIP_TRY(at.ensure(sizeof(int64_t) * (size_t)(n + 1)));
  HIP_TRY(st.ensure(sizeof(SvStatsDev)));
  SvSpan sp1;
  HIP_TRY(sp1.begin(c->stream));
  hipLaunchKernelGGL(sv_in_range, dim3(grid(n + 1, 256)), dim3(256), 0, c->stream, p->view(), n, (int64_t *)flag.p);
  HIP_TRY(hipGetLastError());
  if ((s = exclusive_sum(c, (const int64_t *)flag.p, (int64_t *)at.p, n + 1, tmp))) return s;
  int64_t m = 0;
  if ((s = d2h_i64(c, (const int64_t *)at.p + n, &m))) return s;
  const size_t mm = (size_t)std::max<int64_t>(m, 1);
  HIP_TRY(sizes.ensure(sizeof(int32_t) * mm));
  HIP_TRY(sorted.ensure(sizeof(int32_t) * mm));
  HIP_TRY(res.ensure(sizeof(int64_t) * mm));
  HIP_TRY(res2.ensure(sizeof(int64_t) * mm));
  if (m) {
    hipLaunchKernelGGL(sv_oriented, dim3(grid(n, 256)), dim3(256), 0, c->stream, p->view(), n, (const int64_t *)flag.p,
                       (const int64_t *)at.p, (int32_t *)sizes.p);
    HIP_TRY(hipGetLastError());
    size_t tb = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, (const int32_t *)sizes.p, (int32_t *)sorted.p, (int)m, 0, 32,
                                              c->stream));
    HIP_TRY(tmp.ensure(tb));
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(tmp.p, tb, (const int32_t *)sizes.p, (int32_t *)sorted.p, (int)m, 0, 32,
                                              c->stream));
  }
  hipLaunchKernelGGL(sv_median, dim3(1), dim3(64), 0, c->stream, (const int32_t *)sorted.p, m, (SvStatsDev *)st.p);
  HIP_TRY(hipGetLastError());
  if (m) {
    hipLaunchKernelGGL(sv_resid, dim3(grid(m, 256)), dim3(256), 0, c->stream, (const int32_t *)sorted.p, m,
                       (const SvStatsDev *)st.p, (int64_t *)res.p);
    HIP_TRY(hipGetLastError());
    size_t tb = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, (const int64_t *)res.p, (int64_t *)res2.p, (int)m, 0, 64,
                                              c->stream));
    HIP_TRY(tmp.ensure(tb));
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(tmp.p, tb, (const int64_t *)res.p, (int64_t *)res2.p, (int)m, 0, 64,
                                              c->stream));
  }
  hipLaunchKernelGGL(sv_final, dim3(1), dim3(64), 0, c->stream, (const int64_t *)res2.p, m, (SvStatsDev *)st.p);
  HIP_TRY(hipGetLastError());
  float ms1 = 0.f, ms2 = 0.f;
  HIP_TRY(sp1.end(&ms1));
  SvSpan sp2;
  HIP_TRY(sp2.begin(c->stream));
  if ((s = sv_select(p, (const SvStatsDev *)st.p, 0, flag, at, tmp))) return s;
  HIP_TRY(sp2.end(&ms2));
  SvStatsDev h{};
  HIP_TRY(hipMemcpy(&h, st.p, sizeof(h), hipMemcpyDeviceToHost));
  for (DevBuf *x : {&flag, &at, &tmp, &sizes, &sorted, &res, &res2, &st}) x->release();
  *out = gq_sv_stats{n, m, p->n_nodes, h.median, h.mad, h.max_normal, 0, ms1, ms2};
  return GQ_OK;
}

gq_status gq_sv_select(gq_sv_pairs *p, int32_t threshold, int64_t *n_nodes) {
  if (!p) return set_err(GQ_E_ARG, "gq_sv_select: null argument");
  gq_ctx *c = p->ctx;
  HIP_TRY(hipSetDevice(c->device));
  DevBuf flag, at, tmp;
  HIP_TRY(flag.ensure(sizeof(int64_t) * (size_t)(p->n + 1)));
  HIP_TRY(at.ensure(sizeof(int64_t) * (size_t)(p->n + 1)));
  const gq_status s = sv_select(p, nullptr, threshold, flag, at, tmp);
  for (DevBuf *x : {&flag, &at, &tmp}) x->release();
  if (s) return s;
  if (n_nodes) *n_nodes = p->n_nodes;
  return GQ_OK;
}

gq_status gq_sv_nodes_download(const gq_sv_pairs *p, int32_t *contig, int32_t *lo, int32_t *hi, int32_t *len,
                               int64_t *pair) {
  if (!p) return set_err(GQ_E_ARG, "gq_sv_nodes_download: null argument");
  if (!p->selected) return set_err(GQ_E_ARG, "gq_sv_nodes_download before gq_sv_stats_call or gq_sv_select");
  if (!p->n_nodes) return GQ_OK;
  gq_ctx *c = p->ctx;
  HIP_TRY(hipSetDevice(c->device));
  const size_t k = (size_t)p->n_nodes;
  const std::pair<void *, const DevBuf *> cols[] = {{contig, &p->n_contig}, {lo, &p->n_lo}, {hi, &p->n_hi}, {len, &p->n_len}};
  for (const auto &x : cols)
    if (x.first) HIP_TRY(hipMemcpyAsync(x.first, x.second->p, sizeof(int32_t) * k, hipMemcpyDeviceToHost, c->stream));
  if (pair) HIP_TRY(hipMemcpyAsync(pair, p->n_pair.p, sizeof(int64_t) * k, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GQ_OK;
}

void gq_sv_free_graph(gq_sv_graph *g) {
  if (!g) return;
  delete[] g->i;
  delete[] g->j;
  delete[] g->weight;
  delete g;
}

gq_status gq_sv_graph_call(gq_sv_pairs *p, int32_t max_normal, gq_sv_graph **out) {
  if (!p || !out) return set_err(GQ_E_ARG, "gq_sv_graph_call: null argument");
  if (!p->selected) return set_err(GQ_E_ARG, "gq_sv_graph_call before gq_sv_stats_call or gq_sv_select");
  gq_ctx *c = p->ctx;
  HIP_TRY(hipSetDevice(c->device));
  const int64_t n = p->n_nodes;
  gq_status s;
  DevBuf cnt, off, tmp, ei, ej, ew;
  HIP_TRY(cnt.ensure(sizeof(int64_t) * (size_t)(n + 1)));
  HIP_TRY(off.ensure(sizeof(int64_t) * (size_t)(n + 1)));
  SvSpan span;
  HIP_TRY(span.begin(c->stream));
  HIP_TRY(hipMemsetAsync(cnt.p, 0, sizeof(int64_t) * (size_t)(n + 1), c->stream));
  if (n) {
    hipLaunchKernelGGL(sv_edges<false>, dim3(grid(n, 4)), dim3(256), 0, c->stream, p->nodes(), n, (int64_t)max_normal,
                       (int64_t *)cnt.p, (const int64_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr,
                       (int64_t *)nullptr);
    HIP_TRY(hipGetLastError());
  }
  if ((s = exclusive_sum(c, (const int64_t *)cnt.p, (int64_t *)off.p, n + 1, tmp))) return s;
  int64_t total = 0;
  if ((s = d2h_i64(c, (const int64_t *)off.p + n, &total))) return s;
  // 16 bytes an edge, on the device and again on the host
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (total < 0 || (uint64_t)total > (uint64_t)(free_b / 2) / 16)
    return set_err(GQ_E_CAPACITY, "structural-variant: %lld edges over %lld pairs do not fit in device memory",
                   (long long)total, (long long)n);
  const size_t m = (size_t)std::max<int64_t>(total, 1);
  HIP_TRY(ei.ensure(sizeof(int32_t) * m));
  HIP_TRY(ej.ensure(sizeof(int32_t) * m));
  HIP_TRY(ew.ensure(sizeof(int64_t) * m));
  if (total) {
    hipLaunchKernelGGL(sv_edges<true>, dim3(grid(n, 4)), dim3(256), 0, c->stream, p->nodes(), n, (int64_t)max_normal,
                       (int64_t *)nullptr, (const int64_t *)off.p, (int32_t *)ei.p, (int32_t *)ej.p, (int64_t *)ew.p);
    HIP_TRY(hipGetLastError());
  }
  float ms = 0.f;
  HIP_TRY(span.end(&ms));
  gq_sv_graph *g = new (std::nothrow) gq_sv_graph();
  if (g) {
    g->i = new (std::nothrow) int32_t[m];
    g->j = new (std::nothrow) int32_t[m];
    g->weight = new (std::nothrow) int64_t[m];
  }
  if (!g || !g->i || !g->j || !g->weight) {
    gq_sv_free_graph(g);
    return set_err(GQ_E_CAPACITY, "structural-variant: %lld edges do not fit in host memory", (long long)total);
  }
  g->n_nodes = n;
  g->n_edges = total;
  g->edge_ms = ms;
  if (total) {
    HIP_TRY(hipMemcpyAsync(g->i, ei.p, sizeof(int32_t) * m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(g->j, ej.p, sizeof(int32_t) * m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(g->weight, ew.p, sizeof(int64_t) * m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  for (DevBuf *x : {&cnt, &off, &tmp, &ei, &ej, &ew}) x->release();
  *out = g;
  return GQ_OK;
}

gq_status gq_sv_cliques_call(int64_t n_nodes, const int32_t *contig, const int32_t *lo, const int32_t *hi,
                             const int32_t *len, int64_t n_edges, const int32_t *ei, const int32_t *ej,
                             const int64_t *weight, int32_t max_normal, gq_sv_cliques **out) {
  if (!out || n_nodes < 0 || n_edges < 0 || (n_nodes > 0 && (!contig || !lo || !hi || !len)) ||
      (n_edges > 0 && (!ei || !ej || !weight)))
    return set_err(GQ_E_ARG, "gq_sv_cliques_call: null argument");
  for (int64_t e = 0; e < n_edges; ++e)
    if (ei[e] < 0 || ej[e] <= ei[e] || ej[e] >= n_nodes)
      return set_err(GQ_E_ARG, "gq_sv_cliques_call: edge %lld is not (i < j) over %lld nodes", (long long)e,
                     (long long)n_nodes);
  *out = sv_cliques_out(gq_sv::find_cliques(n_nodes, contig, lo, hi, len, n_edges, ei, ej, weight, max_normal));
  return GQ_OK;
}

void gq_sv_free_cliques(gq_sv_cliques *c) {
  if (!c) return;
  delete[] c->contig;
  delete[] c->start;
  delete[] c->stop;
  delete[] c->pairs;
  delete[] c->wiggle;
  delete c;
}

gq_status gq_sv_call(gq_sv_pairs *p, gq_sv_stats *stats, gq_sv_cliques **out, float *edge_ms, float *clique_ms) {
  if (!p || !stats || !out) return set_err(GQ_E_ARG, "gq_sv_call: null argument");
  gq_status s;
  if ((s = gq_sv_stats_call(p, stats))) return s;
  gq_sv_graph *g = nullptr;
  if ((s = gq_sv_graph_call(p, stats->max_normal, &g))) return s;
  const size_t k = (size_t)std::max<int64_t>(p->n_nodes, 1);
  std::vector<int32_t> contig(k), lo(k), hi(k), len(k);
  if ((s = gq_sv_nodes_download(p, contig.data(), lo.data(), hi.data(), len.data(), nullptr))) {
    gq_sv_free_graph(g);
    return s;
  }
  const auto t0 = std::chrono::steady_clock::now();
  *out = sv_cliques_out(gq_sv::find_cliques(p->n_nodes, contig.data(), lo.data(), hi.data(), len.data(), g->n_edges, g->i,
                                            g->j, g->weight, stats->max_normal));
  if (clique_ms) *clique_ms = ms_since(t0);
  if (edge_ms) *edge_ms = g->edge_ms;
  gq_sv_free_graph(g);
  return GQ_OK;
}

}  // extern "C"
