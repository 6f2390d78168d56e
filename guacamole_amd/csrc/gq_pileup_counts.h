// gq_pileup_counts.h — pileup-counts (gq_pileup_counts_call): the per-locus table of the pileup
// (pileup/Pileup.scala:49-132, pileup/PileupElement.scala) at every locus whose filtered pileup is
// deep enough: depth, strand-split counts of the Match/Mismatch elements by sequenced base, and the
// counts of Insertion / Deletion / MidDeletion / Clipped elements.  Included by gq_somatic.hip
// inside its anonymous namespace, after the caller's device helpers (make_cover, pileup_ref).
//
// Dense, then compacted, all on the device:
//   pileup_counts_tile<T>   one workgroup per tile of T loci at a time: the walker (walk_read_lane)
//                           with PcSink for the reads the mapq filter keeps and PcDropSink for the
//                           reads it drops (reference-base bits only: the pileup's reference base
//                           is the unfiltered pileup's).  A lane per locus then makes the locus'
//                           row in a dense staging array (T rows per tile a read overlaps, tiles
//                           in call order), with a keep word beside it.  A locus whose
//                           reference-base mask holds more than one base (heap order decides) and
//                           every locus of a tile whose read window could overflow the 16-bit
//                           counters are listed instead.
//   pileup_counts_locus     one wave per listed locus: the cover list (make_cover over the task
//                           window's WinInit), the reference base (heap-order loci through the
//                           AmbItem round trip, as allele-evidence), then the same row from one
//                           pass of classify over the cover, counted with ballots (any depth).
//                           The counts do not depend on the element order, so a cover the list
//                           cannot reorder (Cover::deep) is counted as it is: no deep instantiation.
//   (hipcub)                inclusive scan of the keep words.
//   pileup_counts_gather    a lane per locus: a kept row's fields to the result block's columns at
//                           its scanned position, which is call order.
#pragma once

constexpr int kPcT = 512;          // loci per tile
constexpr int kPcTh = 512;         // reads of a window's initial group make_cover reorders in the work area
constexpr int kPcWork = 2 * kPcTh; // words of a wave's work area

// LDS histogram: P_N u32 words per locus (SoA: word * S + guard + i), two 16-bit counters each.
//   P_F* / P_R*  Match/Mismatch elements of forward / reverse reads the filter keeps:
//                A | C << 16, T | G << 16, other | N << 16  (so an A C G T N byte b lands in word
//                min((b >> 2) & 3, 2), half (b >> 1) & 1 with no table)
//   P_ID, P_MC   Insertion | Deletion << 16, MidDeletion | Clipped << 16 (kept reads, both strands)
//   P_FX         forward elements among those four kinds | reference-base mask << 16 (bits 16-19:
//                the standard MD-derived reference bases under MD events and of the four kinds'
//                elements, of kept and dropped reads alike)
//   P_EAC, P_ETG A C / T G Match/Mismatch elements of kept reads carrying an MD mismatch event
//   P_DAC, P_DTG dropped reads: A C / T G Match/Mismatch elements minus those carrying an MD event
//                (the event subtracts: the sums are exact modulo 2^32 whatever the order, and
//                every final field is a count >= 0)
// A base without an MD event is its own reference base, so base k is in the mask when the kept
// reads' count exceeds their events' or the dropped reads' balance is positive.
enum : int { P_FAC = 0, P_FTG, P_FON, P_RAC, P_RTG, P_RON, P_ID, P_MC, P_FX, P_EAC, P_ETG, P_DAC, P_DTG, P_N };

struct alignas(8) PcRow {  // one locus of the dense staging array
  int32_t contig, pos;
  uint8_t ref_base, flags, pad[2];
  int32_t depth, forward_depth, ref_depth;
  int32_t base_count[6], base_forward[6];  // A C G T N other
  int32_t kind_count[4];                   // Insertion, Deletion, MidDeletion, Clipped
};
static_assert(sizeof(PcRow) == 88, "PcRow layout");

struct PcLayout {  // byte offsets inside the result image
  size_t contig, pos, ref_base, flags, depth, forward_depth, ref_depth, base_count, base_forward, kind_count, bytes;
};

template <int T>
struct PcSink {  // the reads the filter keeps
  uint32_t *cnt;  // P_N arrays of T + 2 * kGuard words
  int32_t L0;
  int *err;
  long long *err_pos;
  static constexpr int S = T + 2 * kGuard;
  __device__ __forceinline__ uint32_t *at(int w, int i) const { return cnt + w * S + kGuard + i; }
  __device__ __forceinline__ void bases4(int i, uint32_t w, uint32_t valid4, uint8_t fl) {
    const uint32_t code4 = (w >> 1) & 0x07070707u;
    const uint32_t exp4 = __builtin_amdgcn_perm(0x4E000000u, 0x47544341u, code4);  // 'A','C','T','G',0,0,0,'N'
    const int so = (fl & 1) ? P_RAC : P_FAC;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t bj = (w >> (8 * j)) & 0xFFu, ej = (exp4 >> (8 * j)) & 0xFFu, cj = (code4 >> (8 * j)) & 7u;
      const bool known = bj == ej;  // A C T G N; anything else is "other": word 2, low half
      const uint32_t ws = known ? min(cj >> 1, 2u) : 2u, hb = known ? (cj & 1u) : 0u;
      atomicAdd(at(so + (int)ws, i + j), ((valid4 >> j) & 1u) << (hb << 4));
    }
  }
  __device__ __forceinline__ void bases4_clean(int i, uint32_t w, uint32_t valid4, uint8_t fl) {
    const int so = (fl & 1) ? P_RAC : P_FAC;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t ws = min((w >> (8 * j + 2)) & 3u, 2u), hb = (w >> (8 * j + 1)) & 1u;
      atomicAdd(at(so + (int)ws, i + j), ((valid4 >> j) & 1u) << (hb << 4));
    }
  }
  __device__ __forceinline__ void event_i(int i, uint8_t b, uint8_t m, uint8_t) {
    const int c = base_cat(b);
    if (c < 4) atomicAdd(at(P_EAC + (c >> 1), i), 1u << ((c & 1) << 4));
    const uint32_t bit = std_bit(m);
    if (bit) atomicOr(at(P_FX, i), bit << 16);
  }
  __device__ __forceinline__ void other_i(int i, int kind, uint8_t mdb, uint8_t fl) {  // kind: K_INS .. K_CLIP
    atomicAdd(at(P_ID + ((kind - K_INS) >> 1), i), 1u << (((kind - K_INS) & 1) << 4));
    if (!(fl & 1)) atomicAdd(at(P_FX, i), 1u);
    const uint32_t bit = std_bit(mdb);
    if (bit) atomicOr(at(P_FX, i), bit << 16);
  }
  __device__ __forceinline__ void elem(int32_t l, int kind, uint8_t base, uint8_t mdb, bool ev, uint8_t fl) {
    const int i = l - L0;
    if (kind == K_SNV) {
      const int sh = (i & 3) * 8;
      bases4(i - (i & 3), (uint32_t)base << sh, 1u << (i & 3), fl);
      if (ev) event_i(i, base, mdb, fl);
    } else {
      other_i(i, kind, mdb, fl);
    }
  }
  __device__ __forceinline__ void clip_run(int i0, int i1, uint8_t fl) {  // CIGAR N: MD-derived reference 'N'
    for (int i = i0; i < i1; ++i) other_i(i, K_CLIP, (uint8_t)'N', fl);
  }
  __device__ __forceinline__ void error(int code, int64_t where) { raise_error(err, (int64_t *)err_pos, code, where); }
};

template <int T>
struct PcDropSink {  // the reads the filter drops: reference-base bits only
  uint32_t *cnt;
  int32_t L0;
  int *err;
  long long *err_pos;
  static constexpr int S = T + 2 * kGuard;
  __device__ __forceinline__ uint32_t *at(int w, int i) const { return cnt + w * S + kGuard + i; }
  __device__ __forceinline__ void bases4(int i, uint32_t w, uint32_t valid4, uint8_t) {
    const uint32_t code4 = (w >> 1) & 0x07070707u;
    const uint32_t exp4 = __builtin_amdgcn_perm(0x4E000000u, 0x47544341u, code4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t bj = (w >> (8 * j)) & 0xFFu, ej = (exp4 >> (8 * j)) & 0xFFu, cj = (code4 >> (8 * j)) & 7u;
      const uint32_t inc = (bj == ej && cj < 4u) ? ((valid4 >> j) & 1u) << ((cj & 1u) << 4) : 0u;
      atomicAdd(at(P_DAC + (int)((cj >> 1) & 1u), i + j), inc);
    }
  }
  __device__ __forceinline__ void bases4_clean(int i, uint32_t w, uint32_t valid4, uint8_t) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t ws = (w >> (8 * j + 2)) & 3u, hb = (w >> (8 * j + 1)) & 1u;
      const uint32_t inc = ws < 2u ? ((valid4 >> j) & 1u) << (hb << 4) : 0u;  // (N: no bit)
      atomicAdd(at(P_DAC + (int)(ws & 1u), i + j), inc);
    }
  }
  __device__ __forceinline__ void event_i(int i, uint8_t b, uint8_t m, uint8_t) {
    const int c = base_cat(b);
    if (c < 4) atomicSub(at(P_DAC + (c >> 1), i), 1u << ((c & 1) << 4));
    const uint32_t bit = std_bit(m);
    if (bit) atomicOr(at(P_FX, i), bit << 16);
  }
  __device__ __forceinline__ void elem(int32_t l, int kind, uint8_t base, uint8_t mdb, bool ev, uint8_t fl) {
    const int i = l - L0;
    if (kind == K_SNV) {
      const int sh = (i & 3) * 8;
      bases4(i - (i & 3), (uint32_t)base << sh, 1u << (i & 3), fl);
      if (ev) event_i(i, base, mdb, fl);
    } else {
      const uint32_t bit = std_bit(mdb);
      if (bit) atomicOr(at(P_FX, i), bit << 16);
    }
  }
  __device__ __forceinline__ void clip_run(int, int, uint8_t) {}
  __device__ __forceinline__ void error(int code, int64_t where) { raise_error(err, (int64_t *)err_pos, code, where); }
};

// A tile some read overlaps takes T rows of the staging array: active[t] scanned (inclusive) is
// its slot + 1.  (Loci ranges far from every read, `all` over a genome, take no staging.)
__global__ __launch_bounds__(kBlock) void pileup_counts_active(const Tile *__restrict__ tiles, int64_t n_tiles,
                                                               uint32_t *__restrict__ active) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_tiles) active[t] = tiles[t].re > tiles[t].rb ? 1u : 0u;
}

// Does the finished row stay?  (min_depth below 1 is 1: an empty pileup is never a row.)
__device__ __forceinline__ bool pc_keep(const gq_pileup_counts_params &prm, int32_t depth, int32_t ref_depth) {
  return depth >= max(1, prm.min_depth) && (!prm.variants_only || depth > ref_depth);
}
// index of a base_cat category (A C T G N other) in the output order A C G T N other
__device__ __forceinline__ int pc_out_index(int cat) { return cat == 2 ? 3 : cat == 3 ? 2 : cat; }
// One staging row, field by field (bc / bf / kc are registers: every index is a constant).
__device__ __forceinline__ void pc_store(PcRow *__restrict__ dst, int32_t contig, int32_t pos, uint8_t ref_base,
                                         uint8_t flags, uint32_t depth, uint32_t fwd, uint32_t ref_depth,
                                         const uint32_t (&bc)[6], const uint32_t (&bf)[6], const uint32_t (&kc)[4]) {
  dst->contig = contig;
  dst->pos = pos;
  *reinterpret_cast<uint32_t *>(&dst->ref_base) = (uint32_t)ref_base | ((uint32_t)flags << 8);  // (and the padding)
  dst->depth = (int32_t)depth;
  dst->forward_depth = (int32_t)fwd;
  dst->ref_depth = (int32_t)ref_depth;
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    dst->base_count[s] = (int32_t)bc[s];
    dst->base_forward[s] = (int32_t)bf[s];
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) dst->kind_count[s] = (int32_t)kc[s];
}

// items[k] = a locus the tile cannot decide; flags bit0: listed unconditionally (a tile whose read
// window could overflow the 16-bit counters): the per-locus kernel counts the visit.
template <int T>
__global__ __launch_bounds__(kBlock) void pileup_counts_tile(const Tile *__restrict__ tiles, int64_t n_tiles, DevReads R,
                                                             gq_pileup_counts_params prm,
                                                             const uint32_t *__restrict__ tslot,
                                                             PcRow *__restrict__ rows, uint32_t *__restrict__ keep,
                                                             int64_t n_slots, ComplexItem *__restrict__ items,
                                                             unsigned long long item_cap, Counters *ctr) {
  constexpr int S = T + 2 * kGuard;
  constexpr int KPT = T / kBlock;
  __shared__ __attribute__((aligned(16))) uint32_t cnt[P_N * S];
  static_assert((P_N * S) % 4 == 0, "cleared four words at a time");
  const int min_mapq = prm.min_mapq;
  unsigned visited = 0;
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const Tile tt = tiles[t];
    const int32_t L0 = tt.L0, L1 = tt.L1;
    const int nloci = L1 - L0;
    if (tt.re <= tt.rb) continue;  // no read overlaps the tile: no staging slot, no row
    if ((tt.re - tt.rb) >= 65535) {
#pragma unroll
      for (int k = 0; k < KPT; ++k) {
        const int i = threadIdx.x + k * kBlock;
        const unsigned long long b = wave_reserve(&ctr->n_complex, i < nloci ? 1u : 0u);
        if (i < nloci && b < item_cap) items[b] = ComplexItem{(int32_t)t, L0 + i, 1};
      }
      continue;
    }
    const int64_t o0 = ((int64_t)tslot[t] - 1) * T;  // the tile's first staging row
    uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
    __syncthreads();  // the previous tile's readers are done
    for (int i = threadIdx.x; i < P_N * S / 4; i += blockDim.x) c4[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    {
      PcSink<T> keep_s{cnt, L0, &ctr->err, &ctr->err_pos};
      PcDropSink<T> drop_s{cnt, L0, &ctr->err, &ctr->err_pos};
      for (int64_t r = tt.rb + threadIdx.x; r < tt.re; r += blockDim.x) {
        if (min_mapq <= 0 || (int)R.mapq[r] >= min_mapq) walk_read_lane(R, r, L0, L1, keep_s);
        else walk_read_lane(R, r, L0, L1, drop_s);
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
      const int i = threadIdx.x + k * kBlock;
      bool q = false;
      if (i < nloci) {
        auto w = [&](int word) { return cnt[word * S + kGuard + i]; };
        // LDS order A C T G other N, per strand
        uint32_t f[6], rv[6];
        {
          const uint32_t fac = w(P_FAC), ftg = w(P_FTG), fon = w(P_FON), rac = w(P_RAC), rtg = w(P_RTG), ron = w(P_RON);
          f[0] = fac & 0xFFFFu, f[1] = fac >> 16, f[2] = ftg & 0xFFFFu, f[3] = ftg >> 16, f[4] = fon & 0xFFFFu, f[5] = fon >> 16;
          rv[0] = rac & 0xFFFFu, rv[1] = rac >> 16, rv[2] = rtg & 0xFFFFu, rv[3] = rtg >> 16, rv[4] = ron & 0xFFFFu, rv[5] = ron >> 16;
        }
        const uint32_t wid = w(P_ID), wmc = w(P_MC), wfx = w(P_FX);
        const uint32_t kc[4] = {wid & 0xFFFFu, wid >> 16, wmc & 0xFFFFu, wmc >> 16};
        uint32_t depth = kc[0] + kc[1] + kc[2] + kc[3], fwd = wfx & 0xFFFFu;
#pragma unroll
        for (int b = 0; b < 6; ++b) {
          depth += f[b] + rv[b];
          fwd += f[b];
        }
        const int64_t o = o0 + i;
        if (depth > 0 && o >= 0 && o < n_slots) {
          ++visited;
          uint32_t mask = (wfx >> 16) & 0xFu;
          const uint32_t eac = w(P_EAC), etg = w(P_ETG), dac = w(P_DAC), dtg = w(P_DTG);
          const uint32_t e[4] = {eac & 0xFFFFu, eac >> 16, etg & 0xFFFFu, etg >> 16};
          const uint32_t d[4] = {dac & 0xFFFFu, dac >> 16, dtg & 0xFFFFu, dtg >> 16};
#pragma unroll
          for (int b = 0; b < 4; ++b)
            if (f[b] + rv[b] > e[b] || d[b] > 0) mask |= 1u << b;
          if ((int)depth >= max(1, prm.min_depth)) {
            if (__popc(mask) > 1) {
              q = true;  // heap order decides the reference base
            } else {
              const int rc = mask ? (__ffs((int)mask) - 1) : 4;  // base_cat of the reference base: A C T G N
              const uint32_t ref_depth = rc == 0   ? f[0] + rv[0]
                                         : rc == 1 ? f[1] + rv[1]
                                         : rc == 2 ? f[2] + rv[2]
                                         : rc == 3 ? f[3] + rv[3]
                                                   : f[5] + rv[5];
              if (pc_keep(prm, (int32_t)depth, (int32_t)ref_depth)) {
                // output order A C G T N other <- LDS order A C T G other N
                const uint32_t bf[6] = {f[0], f[1], f[3], f[2], f[5], f[4]};
                const uint32_t bc[6] = {f[0] + rv[0], f[1] + rv[1], f[3] + rv[3], f[2] + rv[2], f[5] + rv[5], f[4] + rv[4]};
                pc_store(rows + o, tt.contig, L0 + i, cat_base(rc), 0, depth, fwd, ref_depth, bc, bf, kc);
                keep[o] = 1u;
              }
            }
          }
        }
      }
      const unsigned long long b = wave_reserve(&ctr->n_complex, q ? 1u : 0u);
      if (q && b < item_cap) items[b] = ComplexItem{(int32_t)t, L0 + i, 0};
    }
  }
  __shared__ unsigned red;
  if (threadIdx.x == 0) red = 0;
  __syncthreads();
  if (visited) atomicAdd(&red, visited);
  __syncthreads();
  if (threadIdx.x == 0 && red) atomicAdd(&ctr->spread[0][blockIdx.x & (kSpread - 1)], (unsigned long long)red);
}

__global__ __launch_bounds__(kBlock) void pileup_counts_locus(
    const Tile *__restrict__ tiles, const ComplexItem *__restrict__ items, int64_t n_items, DevReads R,
    gq_pileup_counts_params prm, const uint32_t *__restrict__ tslot, PcRow *__restrict__ rows,
    uint32_t *__restrict__ keep, int64_t n_slots, Counters *ctr, SomWin sw, AmbItem *__restrict__ amb_out, unsigned long long amb_cap, const AmbItem *__restrict__ amb_in,
    const uint8_t *__restrict__ amb_ref, int64_t n_amb_in) {
  __shared__ uint32_t work[kSomWaves][kPcWork];
  __shared__ int32_t cover[kSomWaves][kCover];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t gwave = wave_id();
  const int64_t nwaves_total = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int min_mapq = prm.min_mapq;
  const int64_t n = amb_in ? n_amb_in : n_items;
  for (int64_t si = gwave; si < n; si += nwaves_total) {
    const int64_t it = amb_in ? amb_in[si].item : si;
    const ComplexItem item = items[it];
    const Tile tt = tiles[item.tile];
    const int32_t pos = item.pos;
    const int32_t win = sw.range_win[tt.range];
    // (a cover the list cannot hold or reorder is walked in read order: the counts are order-free)
    const Cover ca = make_cover(R, tt.rb, tt.re, pos, cover[wv], work[wv], kCover, kPcTh, sw.wi[2 * win], sw.init_reads,
                                sw.init_rank, ctr);
    uint8_t refbase;
    bool ambiguous;
    pileup_ref(R, ca, pos, ctr, amb_in ? (int)amb_ref[si] : -1, refbase, ambiguous);
    uint32_t cnt[10], fw[6], fwd = 0, depth = 0;  // A C G T N other, Insertion Deletion MidDeletion Clipped
#pragma unroll
    for (int s = 0; s < 10; ++s) cnt[s] = 0;
#pragma unroll
    for (int s = 0; s < 6; ++s) fw[s] = 0;
    for (int64_t k0 = 0; k0 < ca.n; k0 += 64) {
      bool act;
      const int64_t r = ca.read(R, k0 + lane, pos, &act);
      int slot = -1;
      bool forward = false;
      if (act && (min_mapq <= 0 || (int)R.mapq[r] >= min_mapq)) {
        forward = !(R.flags[r] & 1);
        AlleleDesc d;
        int errc = 0;
        if (!classify(R, r, pos, refbase, d, &errc)) raise_at(ctr, errc, pos);
        else slot = d.kind == K_SNV ? pc_out_index(base_cat(d.base)) : 5 + (int)d.kind;
      }
      const unsigned long long passb = __ballot(slot >= 0), fwdb = __ballot(slot >= 0 && forward);
      if (!passb) continue;
      depth += (uint32_t)__popcll(passb);
      fwd += (uint32_t)__popcll(fwdb);
#pragma unroll
      for (int s = 0; s < 10; ++s) {
        const unsigned long long b = __ballot(slot == s);
        cnt[s] += (uint32_t)__popcll(b);
        if (s < 6) fw[s] += (uint32_t)__popcll(b & fwdb);
      }
    }
    if ((item.flags & 1) && !amb_in && depth > 0 && lane == 0) atomicAdd(&ctr->visited, 1ull);  // the tile kernel did not
    if (!amb_in && ambiguous) {  // heap order decides the reference base: list it
      if ((int)depth >= max(1, prm.min_depth) && lane == 0) {
        const unsigned long long k = atomicAdd(&ctr->n_amb, 1ull);
        if (k < amb_cap) amb_out[k] = AmbItem{item.tile, pos, it};
      }
      continue;
    }
    const int64_t o = ((int64_t)tslot[item.tile] - 1) * kPcT + (pos - tt.L0);
    const int rs = pc_out_index(base_cat(refbase));
    uint32_t ref_depth = 0;
#pragma unroll
    for (int s = 0; s < 6; ++s)
      if (s == rs) ref_depth = cnt[s];
    if (lane == 0 && o >= 0 && o < n_slots && pc_keep(prm, (int32_t)depth, (int32_t)ref_depth)) {
      const uint32_t bc[6] = {cnt[0], cnt[1], cnt[2], cnt[3], cnt[4], cnt[5]}, kc[4] = {cnt[6], cnt[7], cnt[8], cnt[9]};
      pc_store(rows + o, tt.contig, pos, refbase, amb_in ? 1 : 0, depth, fwd, ref_depth, bc, fw, kc);
      keep[o] = 1u;
    }
    __builtin_amdgcn_wave_barrier();  // the next locus' cover reorder reuses the work area
  }
}

// Row o of the staging array, when kept, to position inc[o] - 1 of every column (inc: the
// inclusive scan of keep, so the position is the number of kept rows before it: call order).
__global__ __launch_bounds__(kBlock) void pileup_counts_gather(const PcRow *__restrict__ rows,
                                                               const uint32_t *__restrict__ keep,
                                                               const uint32_t *__restrict__ inc, int64_t n_slots,
                                                               int64_t n_rows, PcLayout L, uint8_t *__restrict__ img) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n_slots || !keep[o]) return;
  const int64_t k = (int64_t)inc[o] - 1;
  if (k < 0 || k >= n_rows) return;  // (the image was sized from the scan's total)
  const PcRow row = rows[o];
  ((int32_t *)(img + L.contig))[k] = row.contig;
  ((int64_t *)(img + L.pos))[k] = row.pos;
  img[L.ref_base + k] = row.ref_base;
  img[L.flags + k] = row.flags;
  ((int32_t *)(img + L.depth))[k] = row.depth;
  ((int32_t *)(img + L.forward_depth))[k] = row.forward_depth;
  ((int32_t *)(img + L.ref_depth))[k] = row.ref_depth;
  int32_t *bc = (int32_t *)(img + L.base_count) + 6 * k, *bf = (int32_t *)(img + L.base_forward) + 6 * k;
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    bc[s] = row.base_count[s];
    bf[s] = row.base_forward[s];
  }
  int32_t *kc = (int32_t *)(img + L.kind_count) + 4 * k;
#pragma unroll
  for (int s = 0; s < 4; ++s) kc[s] = row.kind_count[s];
}
