// gq_hapvar.h — variants from assembled haplotypes on the device (gqpileup.h: gq_hapvar_windows).
// Included by gq_hapvar.hip.  The CIGAR walk, the order of events, the ALT bytes and a genotype's
// term and sum are gq_hapvar_host.h's; this file holds the kernels.
//
// hv_count_k    a lane per haplotype walks its CIGAR (normalisation included) and counts its raw
//               events and its indels dropped at the window's edge.
// (hipcub)      exclusive sum of the counts: a haplotype's place in the raw arrays; a window's raw
//               events are those of its haplotypes, consecutive.
// hv_write_k    the same walk, writing the raw events.
// hv_window_k   a workgroup per window: the raw events' keys go to LDS, an index array is bitonic-
//               sorted by (offset, ref_len, alt_len, ALT bytes; the bytes are read from global memory
//               only on a tie of the first three), run heads are marked, each head ORs its run's
//               carrier bits, and the distinct events are compacted (two block scans: their index and
//               their place among the window's ALT bytes).  A window over the cap gets its flag and
//               no events.
// hv_gather_k   a lane per event: the flat arrays and the ALT bytes, once the host has the windows'
//               counts.
// hv_marginal_k a wave per event.  Per pass 64 lanes take 64 consecutive reads; each lane runs the
//               masked maxima over H and its three log terms; then every lane adds the pass's terms
//               in read order, taken from the lanes with readlane, so the logs run in parallel and
//               the sums stay sequential.  The AD counts are ballots.
#pragma once

namespace gq {
namespace hvk {

using gq_hapvar::kMaxRaw;
constexpr int kSortThreads = gq_hapvar::kSortThreads;
constexpr int kPerThread = kMaxRaw / kSortThreads;
static_assert(kPerThread * kSortThreads == kMaxRaw && (kMaxRaw & (kMaxRaw - 1)) == 0, "the sort buffer is a power of two");

struct Haps {  // device pointers, per haplotype unless said
  const uint8_t *flags;        // gq_hapvar::Prepared::hap_flags
  const int32_t *win;          // the haplotype's window
  const int64_t *cig_off;
  const int32_t *n_cigar;
  const uint32_t *cigar;
  const int64_t *seq_off;      // [NH + 1] into bases
  const uint8_t *bases;
  const int64_t *win_hap_off;  // [W + 1]
  const uint8_t *ref_pool;
  const int64_t *ref_off;      // [W]
};

struct CountEmit {
  int64_t n = 0;
  __device__ void operator()(int32_t, int32_t, int32_t, int32_t) { ++n; }
};
struct WriteEmit {
  int32_t *off, *rl, *al;
  int64_t *hp;
  uint8_t *h;
  int64_t at, base;
  uint8_t local;
  __device__ void operator()(int32_t o, int32_t r, int32_t a, int32_t q) {
    off[at] = o;
    rl[at] = r;
    al[at] = a;
    hp[at] = r == 1 ? base + q : 0;
    h[at] = local;
    ++at;
  }
};

// n_raw[h] (n_raw[NH] = 0, for the scan) and n_drop[h]
__global__ void __launch_bounds__(256) hv_count_k(Haps H, int64_t NH, int64_t *__restrict__ n_raw,
                                                  int32_t *__restrict__ n_drop) {
  const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h > NH) return;
  int64_t n = 0;
  int32_t drop = 0;
  if (h < NH && !H.flags[h]) {
    const int32_t w = H.win[h];
    CountEmit emit;
    gq_hapvar::walk(H.cigar + H.cig_off[h], H.n_cigar[h], H.ref_pool + H.ref_off[w], H.bases + H.seq_off[h], emit, &drop);
    n = emit.n;
  }
  n_raw[h] = n;
  if (h < NH) n_drop[h] = drop;
}

struct RawOut {
  int32_t *off, *rl, *al;
  int64_t *hp;
  uint8_t *h;
};
// raw_off: the scan of n_raw.  A window over the cap is not written: hv_window_k does not read it.
__global__ void __launch_bounds__(256) hv_write_k(Haps H, int64_t NH, const int64_t *__restrict__ raw_off, RawOut o) {
  const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= NH || H.flags[h]) return;
  const int32_t w = H.win[h];
  const int64_t h0 = H.win_hap_off[w], h1 = H.win_hap_off[w + 1];
  if (raw_off[h1] - raw_off[h0] > kMaxRaw) return;
  WriteEmit emit{o.off, o.rl, o.al, o.hp, o.h, raw_off[h], H.seq_off[h], (uint8_t)(h - h0)};
  int32_t drop = 0;
  gq_hapvar::walk(H.cigar + H.cig_off[h], H.n_cigar[h], H.ref_pool + H.ref_off[w], H.bases + H.seq_off[h], emit, &drop);
}

struct Compact {  // a window's distinct events, at its raw base
  int32_t *off, *rl, *al;
  int64_t *hp, *alt_rel;   // alt_rel: the event's place among its window's ALT bytes
  uint64_t *carriers;
};

// A workgroup per window.  n_ev[w], n_alt[w], win_flags[w]; *dropped += the window's dropped indels.
__global__ void __launch_bounds__(kSortThreads) hv_window_k(int64_t W, const int64_t *__restrict__ win_hap_off,
                                                            const int64_t *__restrict__ raw_off,
                                                            const int32_t *__restrict__ n_drop, RawOut R,
                                                            const uint8_t *__restrict__ bases, Compact C,
                                                            int32_t *__restrict__ n_ev, int64_t *__restrict__ n_alt,
                                                            uint8_t *__restrict__ win_flags,
                                                            unsigned long long *__restrict__ dropped) {
  __shared__ int32_t s_off[kMaxRaw], s_rl[kMaxRaw], s_al[kMaxRaw], s_ord[kMaxRaw];
  __shared__ uint8_t s_head[kMaxRaw];
  __shared__ int s_drop;
  using Scan = hipcub::BlockScan<int, kSortThreads>;
  __shared__ typename Scan::TempStorage scan_tmp;
  const int64_t w = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t h0 = win_hap_off[w], h1 = win_hap_off[w + 1];
  const int64_t base = raw_off[h0], n_raw = raw_off[h1] - base;
  if (tid == 0) s_drop = 0;
  __syncthreads();
  int drop = 0;
  for (int64_t h = h0 + tid; h < h1; h += kSortThreads) drop += n_drop[h];
  if (drop) atomicAdd(&s_drop, drop);
  __syncthreads();
  uint8_t flags = s_drop ? GQ_HV_EDGE_DROPPED : 0;
  if (tid == 0 && s_drop) atomicAdd(dropped, (unsigned long long)s_drop);
  if (n_raw > kMaxRaw || n_raw == 0) {  // (uniform over the workgroup)
    if (tid == 0) {
      n_ev[w] = 0;
      n_alt[w] = 0;
      win_flags[w] = flags | (n_raw > kMaxRaw ? GQ_HV_TOO_MANY_EVENTS : 0);
    }
    return;
  }
  const int n = (int)n_raw;
  int P = 2;
  while (P < n) P <<= 1;
  for (int i = tid; i < P; i += kSortThreads) {
    if (i < n) {
      s_off[i] = R.off[base + i];
      s_rl[i] = R.rl[base + i];
      s_al[i] = R.al[base + i];
    }
    s_ord[i] = i < n ? i : -1;  // -1: padding, after every event
  }
  __syncthreads();
  auto cmp = [&](int a, int b) {  // a, b: raw indexes within the window
    return gq_hapvar::compare(s_off[a], s_rl[a], s_al[a], R.hp[base + a], s_off[b], s_rl[b], s_al[b], R.hp[base + b], bases);
  };
  auto after = [&](int a, int b) {  // a strict total order: ties by raw index
    if (a < 0 || b < 0) return a < 0 && b >= 0;
    const int c = cmp(a, b);
    return c > 0 || (c == 0 && a > b);
  };
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += kSortThreads) {
        const int x = i ^ j;
        if (x > i) {
          const int a = s_ord[i], b = s_ord[x];
          if (after(a, b) == ((i & k) == 0)) {
            s_ord[i] = b;
            s_ord[x] = a;
          }
        }
      }
      __syncthreads();
    }
  // run heads; thread t owns the sorted places [t * kPerThread, + kPerThread)
  int head[kPerThread], alt[kPerThread], at[kPerThread], alt_at[kPerThread];
#pragma unroll
  for (int u = 0; u < kPerThread; ++u) {
    const int i = tid * kPerThread + u;
    head[u] = i < n && (i == 0 || cmp(s_ord[i - 1], s_ord[i]) != 0);
    alt[u] = head[u] ? s_al[s_ord[i]] : 0;
    s_head[i] = (uint8_t)head[u];
  }
  int total = 0, total_alt = 0;
  Scan(scan_tmp).ExclusiveSum(head, at, total);
  __syncthreads();
  Scan(scan_tmp).ExclusiveSum(alt, alt_at, total_alt);
  __syncthreads();  // s_head is written
#pragma unroll
  for (int u = 0; u < kPerThread; ++u) {
    const int i = tid * kPerThread + u;
    if (!head[u]) continue;
    const int a = s_ord[i];
    uint64_t car = 0;
    for (int j = i; j < n && (j == i || !s_head[j]); ++j) car |= (uint64_t)1 << R.h[base + s_ord[j]];
    const int64_t o = base + at[u];
    C.off[o] = s_off[a];
    C.rl[o] = s_rl[a];
    C.al[o] = s_al[a];
    C.hp[o] = R.hp[base + a];
    C.alt_rel[o] = alt_at[u];
    C.carriers[o] = car;
  }
  if (tid == 0) {
    n_ev[w] = total;
    n_alt[w] = total_alt;
    win_flags[w] = flags;
  }
}

// the last w in [0, W) with off[w] <= x (off ascending, x < off[W])
__device__ __forceinline__ int64_t hv_range_of(const int64_t *off, int64_t W, int64_t x) {
  int64_t lo = 0, hi = W - 1;
  while (lo < hi) {
    const int64_t m = (lo + hi + 1) >> 1;
    if (off[m] <= x) lo = m;
    else hi = m - 1;
  }
  return lo;
}

struct Events {  // the block's per-event arrays on the device
  int64_t *pos;
  uint8_t *kind;
  int32_t *ref_len;
  int64_t *alt_off;
  int32_t *alt_len;
  uint8_t *alt_bases;
  uint64_t *carriers;
};
// a lane per event; win_raw[w]: the window's raw base; win_alt[w]: its first ALT byte
__global__ void __launch_bounds__(256) hv_gather_k(int64_t W, int64_t E, const int64_t *__restrict__ ev_off,
                                                   const int64_t *__restrict__ win_hap_off,
                                                   const int64_t *__restrict__ raw_off, const int64_t *__restrict__ win_alt,
                                                   const int32_t *__restrict__ win_start, const uint8_t *__restrict__ ref_pool,
                                                   const int64_t *__restrict__ ref_off, const uint8_t *__restrict__ bases,
                                                   Compact C, Events o) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int64_t w = hv_range_of(ev_off, W, e);
  const int64_t src = raw_off[win_hap_off[w]] + (e - ev_off[w]);
  const int32_t off = C.off[src], rl = C.rl[src], al = C.al[src];
  const int64_t alt = win_alt[w] + C.alt_rel[src];
  o.pos[e] = (int64_t)win_start[w] + off;
  o.kind[e] = (uint8_t)gq_hapvar::kind_of(rl, al);
  o.ref_len[e] = rl;
  o.alt_off[e] = alt;
  o.alt_len[e] = al;
  o.carriers[e] = C.carriers[src];
  gq_hapvar::write_alt(o.alt_bases + alt, ref_pool + ref_off[w], off, rl, al, bases, C.hp[src]);
}

__device__ __forceinline__ double lane_value(double v, int lane) {  // lane: uniform over the wave
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                          __builtin_amdgcn_readlane(__double2loint(v), lane));
}

constexpr int kEventWaves = 4;  // events per workgroup
// a wave per event
__global__ void __launch_bounds__(64 * kEventWaves) hv_marginal_k(
    int64_t W, int64_t E, const int64_t *__restrict__ ev_off, const int64_t *__restrict__ win_read_off,
    const int64_t *__restrict__ win_hap_off, const int64_t *__restrict__ lik_off, const double *__restrict__ scaled,
    const uint64_t *__restrict__ usable, const uint64_t *__restrict__ carriers, double *__restrict__ gl,
    int32_t *__restrict__ best, int32_t *__restrict__ ad_ref, int32_t *__restrict__ ad_alt, int32_t *__restrict__ dp,
    uint8_t *__restrict__ ev_flags) {
  GQ_NO_CONTRACT
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * kEventWaves + (threadIdx.x >> 6);
  if (e >= E) return;  // (whole waves leave; the kernel has no barrier)
  const int64_t w = hv_range_of(ev_off, W, e);
  const int64_t N = win_read_off[w + 1] - win_read_off[w], H = win_hap_off[w + 1] - win_hap_off[w];
  const uint64_t car = carriers[e], rest = usable[w] & ~car;
  const double *s = scaled + lik_off[w];
  double g0 = 0.0, g1 = 0.0, g2 = 0.0;
  int32_t nr = 0, na = 0;
  for (int64_t n0 = 0; n0 < N; n0 += gq_hapvar::kPassReads) {
    const int64_t n = n0 + lane;
    const int cnt = (int)(N - n0 < gq_hapvar::kPassReads ? N - n0 : gq_hapvar::kPassReads);
    double r = 0.0, a = 0.0, t0 = 0.0, t1 = 0.0, t2 = 0.0;
    if (n < N) {
      gq_hapvar::sides(s + n * H, car, rest, &r, &a);
      t0 = gq_hapvar::term(r, r);
      t1 = gq_hapvar::term(r, a);
      t2 = gq_hapvar::term(a, a);
    }
    nr += __popcll(__ballot(n < N && r > a));
    na += __popcll(__ballot(n < N && a > r));
    for (int k = 0; k < cnt; ++k) {  // every lane keeps the three sums: read order
      g0 = gq_hapvar::add(g0, lane_value(t0, k));
      g1 = gq_hapvar::add(g1, lane_value(t1, k));
      g2 = gq_hapvar::add(g2, lane_value(t2, k));
    }
  }
  if (lane == 0) {
    const double g[3] = {g0, g1, g2};
    gl[3 * e] = g0;
    gl[3 * e + 1] = g1;
    gl[3 * e + 2] = g2;
    best[e] = gq_haplik::first_largest(g, 3);
    ad_ref[e] = nr;
    ad_alt[e] = na;
    dp[e] = (int32_t)N;
    ev_flags[e] = rest ? 0 : GQ_HV_NO_REF_SIDE;
  }
}

}  // namespace hvk
}  // namespace gq
