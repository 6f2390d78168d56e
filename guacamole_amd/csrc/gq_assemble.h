// gq_assemble.h — local assembly on the device (gqpileup.h: gq_asm_graphs).  Included by
// gq_assemble.hip.  The key packing, hash and k-mer steps are gq_assemble_host.h's; this file holds
// the kernels.
//
// Window reads.  asm_range_k, a lane per window: the reads of the window's contig are sorted by
// start and pmax_end is the running maximum of their ends, so two binary searches give the range
// [first read with pmax_end > start, first read with start >= end) that holds every overlapping
// read.  asm_test_k, a lane per candidate of that range: overlap, length >= k and every byte one of
// A C G T (and mapping quality >= min_mapq); it emits the read's k-mer instances and its chunks (kChunk k-mer positions each).  Three
// exclusive sums and asm_compact_k turn that into each window's read list, its instance count and
// its chunk range.
//
// asm_window_k, one workgroup of kThreads per window, does the rest of a window in one kernel,
// because the table it counts into is LDS and does not outlive the kernel:
//   count   a thread takes a chunk of a read, primes the packed key over k - 1 bases and rolls it one
//           shift a base, inserting every k-mer into an open-addressing table lo[] / hi[] / count[].
//           No lane ever waits for another: 64-bit compare-and-swap of lo[s] from empty, then of hi[s]
//           from empty; the slot is the key's iff both words then equal the key's, otherwise the
//           lane probes on (a slot whose lo equals but whose hi was taken by another key is simply
//           not this key's).  Whatever pair a slot ends with is one key; the count is an atomic add.
//           A key that finds no slot in `slots` probes raises the window's overflow flag, the
//           other lanes stop at their next k-mer, and the window is run again by the same code
//           (LDS = false) over a table in global scratch of at least twice its instances.
//   prune   slots with count >= min_occurrence are compacted into a sort buffer (LDS, or the
//           window's staging in global scratch) and padded with empty marks to a power of two;
//   order   bitonic sort by (hi, lo);
//   edges   a thread per node looks its key up for the count and the four children / parents for
//           the masks, and compares it with the source and sink keys thread 0 read off the reference.
// The nodes land in a per-window staging region; the host sums the node counts and asm_gather_k
// moves them to their place in the launch's flat arrays.
#pragma once

namespace gq {
namespace asmk {

using gq_asm::Key;
using gq_asm::kEmpty;
using gq_asm::Shape;

constexpr int kThreads = 1024;
constexpr int kLdsSlots = 4096;  // 80 KiB of table + 64 KiB of sort buffer: one workgroup a CU
constexpr int kChunk = 8;        // k-mer positions a thread rolls over
constexpr int kLdsBytes = kLdsSlots * (8 + 8 + 4) + kLdsSlots * 16;

struct RefView {
  const uint8_t *bytes;
  const int64_t *off, *len;
};

struct Windows {  // device arrays, [W]
  const int32_t *contig, *start, *end;
};

__host__ __device__ __forceinline__ int64_t pow2_ceil(int64_t x) {
  int64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

// cnt[w] = size of window w's candidate range starting at read ra[w]; cnt[W] = 0 (the scan's total)
__global__ void __launch_bounds__(256) asm_range_k(DevReads R, int64_t W, Windows win, int64_t *__restrict__ cnt,
                                                   int64_t *__restrict__ ra) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w > W) return;
  if (w == W) {
    cnt[w] = 0;
    return;
  }
  const int c = win.contig[w];
  const int32_t s = win.start[w], e = win.end[w];
  const int64_t cb = R.contig_read_begin[c], ce = R.contig_read_begin[c + 1];
  int64_t a0 = cb, a1 = ce;
  while (a0 < a1) {  // first read with pmax_end > s
    const int64_t m = (a0 + a1) >> 1;
    if (R.pmax_end[m] > s) a1 = m;
    else a0 = m + 1;
  }
  const int64_t first = a0;
  a1 = ce;
  while (a0 < a1) {  // first read with start >= e
    const int64_t m = (a0 + a1) >> 1;
    if (R.start[m] >= e) a1 = m;
    else a0 = m + 1;
  }
  ra[w] = first;
  cnt[w] = e > s ? a0 - first : 0;
}

// a lane per candidate c of cand_off[W]: flag 1 / instances / chunks of a contributing read, else 0
__global__ void __launch_bounds__(256) asm_test_k(DevReads R, int64_t W, Windows win, int32_t k, int32_t min_mapq,
                                                  const int64_t *__restrict__ cand_off, const int64_t *__restrict__ ra,
                                                  int64_t C, int64_t *__restrict__ flag, int64_t *__restrict__ inst,
                                                  int64_t *__restrict__ chunks) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > C) return;
  int64_t f = 0, ni = 0;
  if (c < C) {
    int64_t lo = 0, hi = W - 1;  // the last window with cand_off[w] <= c: its range holds c
    while (lo < hi) {
      const int64_t m = (lo + hi + 1) >> 1;
      if (cand_off[m] <= c) lo = m;
      else hi = m - 1;
    }
    const int64_t w = lo, r = ra[w] + (c - cand_off[w]);
    const int32_t n = R.seq_len[r];
    bool ok = R.start[r] < win.end[w] && R.end[r] > win.start[w] && n >= k && (int)R.mapq[r] >= min_mapq;
    if (ok) {
      const uint8_t *q = R.seq + R.seq_off[r];
      for (int32_t j = 0; j < n; ++j) ok = ok && gq_asm::base_code(q[j]) >= 0;
    }
    if (ok) {
      f = 1;
      ni = n - k + 1;
    }
  }
  flag[c] = f;
  inst[c] = ni;
  chunks[c] = (ni + kChunk - 1) / kChunk;
}

// the contributing reads in candidate order: list_read[fsum[c]] = read, list_chunk[..] = its first chunk
__global__ void __launch_bounds__(256) asm_compact_k(int64_t W, const int64_t *__restrict__ cand_off,
                                                     const int64_t *__restrict__ ra, int64_t C,
                                                     const int64_t *__restrict__ flag, const int64_t *__restrict__ fsum,
                                                     const int64_t *__restrict__ csum, int64_t *__restrict__ list_read,
                                                     int64_t *__restrict__ list_chunk) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C || !flag[c]) return;
  int64_t lo = 0, hi = W - 1;
  while (lo < hi) {
    const int64_t m = (lo + hi + 1) >> 1;
    if (cand_off[m] <= c) lo = m;
    else hi = m - 1;
  }
  list_read[fsum[c]] = ra[lo] + (c - cand_off[lo]);
  list_chunk[fsum[c]] = csum[c];
}

struct WinMeta {  // per window: its slice of the read list, its chunks, its instances
  int64_t l0, l1, c0, c1, inst;
};
__global__ void __launch_bounds__(256) asm_meta_k(int64_t W, const int64_t *__restrict__ cand_off,
                                                  const int64_t *__restrict__ fsum, const int64_t *__restrict__ isum,
                                                  const int64_t *__restrict__ csum, WinMeta *__restrict__ meta) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  const int64_t a = cand_off[w], b = cand_off[w + 1];
  meta[w] = WinMeta{fsum[a], fsum[b], csum[a], csum[b], isum[b] - isum[a]};
}

struct Table {
  unsigned long long *lo, *hi;
  int *cnt;
  uint32_t mask;  // slots - 1
};

// false: no slot in mask + 1 probes
__device__ __forceinline__ bool table_insert(const Table &t, Key x) {
  const uint32_t h = (uint32_t)gq_asm::hash_of(x);
  for (uint32_t p = 0; p <= t.mask; ++p) {
    const uint32_t s = (h + p) & t.mask;
    unsigned long long cur = *(volatile unsigned long long *)&t.lo[s];
    if (cur == kEmpty) {
      cur = atomicCAS(&t.lo[s], (unsigned long long)kEmpty, (unsigned long long)x.lo);
      if (cur == kEmpty) cur = x.lo;
    }
    if (cur != x.lo) continue;
    cur = *(volatile unsigned long long *)&t.hi[s];
    if (cur == kEmpty) {
      cur = atomicCAS(&t.hi[s], (unsigned long long)kEmpty, (unsigned long long)x.hi);
      if (cur == kEmpty) cur = x.hi;
    }
    if (cur != x.hi) continue;
    atomicAdd(&t.cnt[s], 1);
    return true;
  }
  return false;
}
// the key's count, 0 when absent (after every insertion is done)
__device__ __forceinline__ int table_count(const Table &t, Key x) {
  const uint32_t h = (uint32_t)gq_asm::hash_of(x);
  for (uint32_t p = 0; p <= t.mask; ++p) {
    const uint32_t s = (h + p) & t.mask;
    const unsigned long long l = t.lo[s];
    if (l == kEmpty) return 0;
    if (l == x.lo && t.hi[s] == x.hi) return t.cnt[s];
  }
  return 0;
}

struct Launch {  // one asm_window_k launch: entry j is window wid[j]
  const int64_t *wid;
  const int64_t *tab_off;    // LDS = false: first slot of its table in tab_lo / tab_hi / tab_cnt
  const int64_t *tab_slots;  //              and its slots (a power of two)
  const int64_t *stage_off;  // first entry of its staging region
  const int64_t *stage_cap;  // LDS = false: its entries (a power of two >= its instances)
  unsigned long long *tab_lo, *tab_hi;
  int *tab_cnt;
  unsigned long long *st_lo, *st_hi;  // staging
  int32_t *st_cnt;
  uint8_t *st_cm, *st_pm;
  int32_t *n_nodes, *ovf, *source, *sink, *status;  // [launch entries]
  unsigned long long *ticks;                        // [2 x entries] wall clock of count | the rest
  int32_t lds_slots;                                // LDS = true: slots in use (<= kLdsSlots, a power of two)
};

template <bool LDS>
__global__ void __launch_bounds__(kThreads) asm_window_k(DevReads R, RefView ref, Windows win, int32_t k,
                                                         int32_t min_occ, const WinMeta *__restrict__ meta,
                                                         const int64_t *__restrict__ list_read,
                                                         const int64_t *__restrict__ list_chunk, Launch L) {
  __shared__ unsigned long long l_lo[LDS ? kLdsSlots : 1], l_hi[LDS ? kLdsSlots : 1];
  __shared__ unsigned long long l_slo[LDS ? kLdsSlots : 1], l_shi[LDS ? kLdsSlots : 1];
  __shared__ int l_cnt[LDS ? kLdsSlots : 1];
  __shared__ int sh_n, sh_ovf, sh_src, sh_snk, sh_ref_ok;
  __shared__ Key sh_a, sh_z;
  const int tid = threadIdx.x;
  const int64_t j = blockIdx.x, w = L.wid[j];
  const Shape sp = gq_asm::shape_of(k);
  const unsigned long long t0 = wall_clock64();

  Table t;
  unsigned long long *s_lo, *s_hi;
  int64_t cap;
  if (LDS) {
    t = Table{l_lo, l_hi, l_cnt, (uint32_t)L.lds_slots - 1};
    s_lo = l_slo;
    s_hi = l_shi;
    cap = L.lds_slots;
  } else {
    t = Table{L.tab_lo + L.tab_off[j], L.tab_hi + L.tab_off[j], L.tab_cnt + L.tab_off[j], (uint32_t)L.tab_slots[j] - 1};
    s_lo = L.st_lo + L.stage_off[j];
    s_hi = L.st_hi + L.stage_off[j];
    cap = L.stage_cap[j];
  }
  for (uint32_t i = tid; i <= t.mask; i += kThreads) {
    t.lo[i] = kEmpty;
    t.hi[i] = kEmpty;
    t.cnt[i] = 0;
  }
  const int32_t ws = win.start[w], we = win.end[w], wl = we - ws;
  if (tid == 0) {
    sh_n = 0;
    sh_ovf = 0;
    sh_src = -1;
    sh_snk = -1;
    const int c = win.contig[w];
    bool ok = wl >= k && ref.off[c] >= 0 && (int64_t)we <= ref.len[c];
    Key a{0, 0}, z{0, 0};
    if (ok) {
      const uint8_t *p = ref.bytes + ref.off[c] + ws;
      ok = gq_asm::key_of(sp, p, k, &a) && gq_asm::key_of(sp, p + (wl - k), k, &z);
    }
    sh_ref_ok = ok ? 1 : 0;
    sh_a = a;
    sh_z = z;
  }
  __syncthreads();

  // count
  const WinMeta m = meta[w];
  for (int64_t item = m.c0 + tid; item < m.c1; item += kThreads) {
    if (*(volatile int *)&sh_ovf) break;
    int64_t a = m.l0, b = m.l1 - 1;  // the last read of the list whose first chunk <= item
    while (a < b) {
      const int64_t mid = (a + b + 1) >> 1;
      if (list_chunk[mid] <= item) a = mid;
      else b = mid - 1;
    }
    const int64_t r = list_read[a];
    const uint8_t *q = R.seq + R.seq_off[r];
    const int32_t nk = R.seq_len[r] - k + 1;
    const int32_t j0 = (int32_t)(item - list_chunk[a]) * kChunk, j1 = min(nk, j0 + kChunk);
    Key x{0, 0};
    for (int32_t i = j0; i < j0 + k - 1; ++i) x = gq_asm::roll(sp, x, gq_asm::base_code(q[i]));
    for (int32_t i = j0; i < j1; ++i) {
      x = gq_asm::roll(sp, x, gq_asm::base_code(q[i + k - 1]));
      if (!table_insert(t, x)) {
        sh_ovf = 1;
        break;
      }
    }
  }
  __syncthreads();
  const unsigned long long t1 = wall_clock64();
  if (sh_ovf) {  // (uniform: read after the barrier)
    if (tid == 0) {
      L.ovf[j] = 1;
      L.n_nodes[j] = 0;
      L.source[j] = -1;
      L.sink[j] = -1;
      L.status[j] = 0;
      L.ticks[2 * j] = t1 - t0;
      L.ticks[2 * j + 1] = 0;
    }
    return;
  }

  // prune: the nodes into the sort buffer, in any order
  for (uint32_t i = tid; i <= t.mask; i += kThreads)
    if (t.lo[i] != kEmpty && t.cnt[i] >= min_occ) {
      const int p = atomicAdd(&sh_n, 1);
      s_lo[p] = t.lo[i];
      s_hi[p] = t.hi[i];
    }
  __syncthreads();
  const int n = sh_n;
  const int64_t P = pow2_ceil(n > 0 ? n : 1);  // <= cap: n <= slots (LDS), n <= instances (global)
  for (int64_t i = n + tid; i < P && i < cap; i += kThreads) {
    s_lo[i] = kEmpty;
    s_hi[i] = kEmpty;
  }
  __syncthreads();
  // order: bitonic, empty marks last
  for (int64_t kk = 2; kk <= P; kk <<= 1)
    for (int64_t jj = kk >> 1; jj > 0; jj >>= 1) {
      for (int64_t i = tid; i < P; i += kThreads) {
        const int64_t o = i ^ jj;
        if (o > i) {
          const Key a{s_lo[i], s_hi[i]}, b{s_lo[o], s_hi[o]};
          const bool up = (i & kk) == 0;
          if (up ? gq_asm::key_less(b, a) : gq_asm::key_less(a, b)) {
            s_lo[i] = b.lo;
            s_hi[i] = b.hi;
            s_lo[o] = a.lo;
            s_hi[o] = a.hi;
          }
        }
      }
      __syncthreads();
    }
  // edges
  const int64_t so = L.stage_off[j];
  const int ref_ok = sh_ref_ok;
  const Key ka = sh_a, kz = sh_z;
  for (int i = tid; i < n; i += kThreads) {
    const Key x{s_lo[i], s_hi[i]};
    uint32_t cm = 0, pm = 0;
    for (int b = 0; b < 4; ++b) {
      if (table_count(t, gq_asm::roll(sp, x, b)) >= min_occ) cm |= 1u << b;
      if (table_count(t, gq_asm::unroll(sp, x, b)) >= min_occ) pm |= 1u << b;
    }
    L.st_lo[so + i] = x.lo;
    L.st_hi[so + i] = x.hi;
    L.st_cnt[so + i] = table_count(t, x);
    L.st_cm[so + i] = (uint8_t)cm;
    L.st_pm[so + i] = (uint8_t)pm;
    if (ref_ok && x.lo == ka.lo && x.hi == ka.hi) sh_src = i;
    if (ref_ok && x.lo == kz.lo && x.hi == kz.hi) sh_snk = i;
  }
  __syncthreads();
  if (tid == 0) {
    L.ovf[j] = 0;
    L.n_nodes[j] = n;
    L.source[j] = sh_src;
    L.sink[j] = sh_snk;
    L.status[j] = gq_asm::status_of(wl, k, ref_ok != 0, sh_src, sh_snk);
    L.ticks[2 * j] = t1 - t0;
    L.ticks[2 * j + 1] = wall_clock64() - t1;
  }
}

struct Flat {  // a launch's nodes, window after window
  unsigned long long *lo, *hi;
  int32_t *cnt;
  uint8_t *cm, *pm;
};
// a workgroup per launch entry: its n_nodes staged nodes to flat[node_off[j] ..)
__global__ void __launch_bounds__(256) asm_gather_k(Launch L, const int64_t *__restrict__ node_off, Flat f) {
  const int64_t j = blockIdx.x;
  const int64_t so = L.stage_off[j], o = node_off[j];
  const int n = L.n_nodes[j];
  for (int i = threadIdx.x; i < n; i += 256) {
    f.lo[o + i] = L.st_lo[so + i];
    f.hi[o + i] = L.st_hi[so + i];
    f.cnt[o + i] = L.st_cnt[so + i];
    f.cm[o + i] = L.st_cm[so + i];
    f.pm[o + i] = L.st_pm[so + i];
  }
}

}  // namespace asmk
}  // namespace gq
