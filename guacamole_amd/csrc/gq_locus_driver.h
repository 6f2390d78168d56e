// gq_locus_driver.h — the listed-locus driver: what allele-evidence, genotype-likelihoods and
// pileup-elements share on both sides of the launch.  Included by gq_somatic.hip inside its
// anonymous namespace, after the caller's device helpers (make_cover, pileup_ref, classify,
// DeepSel, GsMem) and ahead of the three commands' headers.
//
// The protocol.  allele_evidence_list compacts the loci to process into one list (items).  A
// command's call kernel then runs one wave per listed locus, in up to four launches:
//   fast    over items, the working set in LDS.  A locus the working set cannot hold is handed
//           over (an entry of dd.out, counted in Counters::n_deep, its depth in deep_max); a locus
//           whose reference base heap order decides is listed in amb_out (Counters::n_amb).
//   deep    over the handed-over entries (dd.sel), the working set in per-wave HBM scratch sized
//           from deep_max.
//   replay  over the heap-order loci (amb_in) with the bases heap_ref_bases found (amb_ref); fast,
//           and its own hand-overs appended to the same list,
//   deep    over those.
// Every buffer the kernels fill is bounded by a capacity they are given and counted past it, so the
// host reads the counters, grows what overflowed and runs the round again (run_listed_loci).
//
// A hand-over entry (dd.out / dd.sel), the one place its layout is written down:
//   bits 9..   position in the list the fast launch walked (items; amb_in at a replay)
//   bit  8     the locus' visit is already counted in Counters::visited
//   bits 0..7  the first sample left to do (0 where the command has no per-sample pass)
#pragma once

constexpr int kAeT = 512;  // loci per list tile

// items[k] = a locus to process; flags bit0: listed unconditionally (a tile whose read window could
// overflow the 16-bit counters): the call kernel counts the visit and applies variants_only itself.
template <int T>
__global__ __launch_bounds__(kBlock) void allele_evidence_list(const Tile *__restrict__ tiles, int64_t n_tiles, DevReads R,
                                                               int min_mapq, int variants_only,
                                                               ComplexItem *__restrict__ items,
                                                               unsigned long long item_cap, Counters *ctr) {
  constexpr int S = T + 2 * kGuard;
  constexpr int KPT = T / kBlock;
  __shared__ __attribute__((aligned(16))) uint32_t cnt[W_N * S];  // the reads the filter keeps
  __shared__ __attribute__((aligned(16))) uint32_t low[W_N * S];  // the reads it drops (reference-base bits)
  unsigned visited = 0;
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const Tile tt = tiles[t];
    const int32_t L0 = tt.L0, L1 = tt.L1;
    const int nloci = L1 - L0;
    if ((tt.re - tt.rb) >= 65535) {
#pragma unroll
      for (int k = 0; k < KPT; ++k) {
        const int i = threadIdx.x + k * kBlock;
        const unsigned long long b = wave_reserve(&ctr->n_complex, i < nloci ? 1u : 0u);
        if (i < nloci && b < item_cap) items[b] = ComplexItem{(int32_t)t, L0 + i, 1};
      }
      continue;
    }
    uint4 *c4 = reinterpret_cast<uint4 *>(cnt), *l4 = reinterpret_cast<uint4 *>(low);
    __syncthreads();  // the previous tile's readers are done
    for (int i = threadIdx.x; i < W_N * S / 4; i += blockDim.x) c4[i] = l4[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    {
      GermSink<T, 0> keep{cnt, L0, &ctr->err, &ctr->err_pos}, drop{low, L0, &ctr->err, &ctr->err_pos};
      for (int64_t r = tt.rb + threadIdx.x; r < tt.re; r += blockDim.x) {
        if (min_mapq <= 0 || (int)R.mapq[r] >= min_mapq) walk_read_lane(R, r, L0, L1, keep);
        else walk_read_lane(R, r, L0, L1, drop);
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
      const int i = threadIdx.x + k * kBlock;
      bool q = false;
      if (i < nloci) {
        const uint32_t wac = cnt[W_AC * S + kGuard + i], wtg = cnt[W_TG * S + kGuard + i],
                       wox = cnt[W_OX * S + kGuard + i], wnn = cnt[W_NN * S + kGuard + i];
        const uint32_t cA = wac & 0xFFFFu, cC = wac >> 16, cT = wtg & 0xFFFFu, cG = wtg >> 16, cN = wnn >> 16;
        const uint32_t cx = (wox & 0xFFFFu) + (wox >> 16);
        const uint32_t depth = cA + cC + cT + cG + cN + cx;
        if (depth > 0) {
          ++visited;
          // the standard MD-derived reference bases of every covering read, kept or dropped
          uint32_t mask = (wnn | low[W_NN * S + kGuard + i]) & 0xFu;
          const uint32_t eac = cnt[W_EAC * S + kGuard + i], etg = cnt[W_ETG * S + kGuard + i];
          if (cA > (eac & 0xFFFFu)) mask |= 1u;
          if (cC > (eac >> 16)) mask |= 2u;
          if (cT > (etg & 0xFFFFu)) mask |= 4u;
          if (cG > (etg >> 16)) mask |= 8u;
          const uint32_t lac = low[W_AC * S + kGuard + i], ltg = low[W_TG * S + kGuard + i],
                         lea = low[W_EAC * S + kGuard + i], let = low[W_ETG * S + kGuard + i];
          if ((lac & 0xFFFFu) > (lea & 0xFFFFu)) mask |= 1u;
          if ((lac >> 16) > (lea >> 16)) mask |= 2u;
          if ((ltg & 0xFFFFu) > (let & 0xFFFFu)) mask |= 4u;
          if ((ltg >> 16) > (let >> 16)) mask |= 8u;
          const int rc = mask ? (__ffs((int)mask) - 1) : 4;
          const uint32_t c_ref = rc == 0 ? cA : rc == 1 ? cC : rc == 2 ? cT : rc == 3 ? cG : cN;
          // heap order decides the reference base (the call kernel lists the locus, and applies
          // variants_only once the base is known), or a non-Match element
          q = !variants_only || __popc(mask) > 1 || cx > 0 || depth > c_ref;
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

// ---- device: a call kernel's per-locus prologue ------------------------------------------------

// The wave's working set: the fast instantiation's LDS areas (cover lists of kCover reads, a work
// area whose first 2 th words take make_cover's reorder), or the wave's slice of the deep scratch.
template <bool DEEP>
__device__ __forceinline__ GsMem locus_mem(const DeepSel &dd, int32_t *cov_a, int32_t *cov_s, uint32_t *work, int th,
                                           int maxG) {
  if constexpr (DEEP) {
    return gs_deep_mem(dd.scratch + (size_t)wave_id() * gs_wave_bytes(dd.scap, dd.maxG), dd.scap, dd.maxG);
  } else {
    return GsMem{cov_a, cov_s, work, nullptr, nullptr, nullptr, kCover, th, maxG};
  }
}

// The loci a launch walks: the handed-over entries, the heap-order loci, or the whole list.
template <bool DEEP>
__device__ __forceinline__ int64_t locus_count(const DeepSel &dd, const AmbItem *amb_in, int64_t n_amb_in,
                                               int64_t n_items) {
  return DEEP ? dd.n_sel : amb_in ? n_amb_in : n_items;
}

struct LocusItem {
  int64_t li;  // position in the list the fast launch walks (items; amb_in at a replay)
  int64_t it;  // the locus' entry of items
  ComplexItem item;
  Tile tt;
  int32_t pos, win;
  int smp0;      // the first sample to do
  bool counted;  // the visit is in Counters::visited
};
template <bool DEEP>
__device__ __forceinline__ LocusItem locus_item(int64_t si, const Tile *__restrict__ tiles,
                                                const ComplexItem *__restrict__ items, const SomWin &sw,
                                                const AmbItem *__restrict__ amb_in, const DeepSel &dd) {
  LocusItem L;
  L.li = DEEP ? (dd.sel[si] >> 9) : si;
  L.smp0 = DEEP ? (int)(dd.sel[si] & 255) : 0;
  L.counted = DEEP ? ((dd.sel[si] >> 8) & 1) != 0 : false;
  L.it = amb_in ? amb_in[L.li].item : L.li;
  L.item = items[L.it];
  L.tt = tiles[L.item.tile];
  L.pos = L.item.pos;
  L.win = sw.range_win[L.tt.range];
  return L;
}

// A locus (from sample smp on) the working set cannot hold: the deep instantiation's.
template <bool DEEP>
__device__ __forceinline__ void locus_hand_over(Counters *ctr, const DeepSel &dd, const LocusItem &L, int smp,
                                                uint32_t depth) {
  if constexpr (!DEEP) {
    if ((threadIdx.x & 63) == 0) {
      const unsigned long long k = atomicAdd(&ctr->n_deep, 1ull);
      if (k < dd.cap) dd.out[k] = (L.li << 9) | (L.counted ? 256 : 0) | smp;
      atomicMax(&ctr->deep_max, (unsigned long long)depth);
    }
  } else {
    raise_at(ctr, GQ_E_CAPACITY, L.pos);
  }
}

// The cover list over every sample and the pileup's reference base.  -> false: the locus is done
// with in this launch (handed over, listed for the heap-order pass, or variants_only and the
// filtered pileup holds only matches).  need_compact: hand over also where the list is not compact.
template <bool DEEP>
__device__ __forceinline__ bool locus_open(const DevReads &R, LocusItem &L, const GsMem &m, const SomWin &sw, Counters *ctr,
                                           int min_mapq, int variants_only, AmbItem *__restrict__ amb_out,
                                           unsigned long long amb_cap, const AmbItem *__restrict__ amb_in,
                                           const uint8_t *__restrict__ amb_ref, const DeepSel &dd, bool need_compact,
                                           Cover &ca, uint8_t &refbase) {
  const int lane = threadIdx.x & 63;
  const Tile &tt = L.tt;
  const int32_t pos = L.pos;
  ca = make_cover(R, tt.rb, tt.re, pos, m.cov_a, m.ev, m.cap, m.th, sw.wi[2 * L.win], sw.init_reads, sw.init_rank, ctr);
  if (ca.deep || (need_compact && !ca.compact)) {
    locus_hand_over<DEEP>(ctr, dd, L, 0, (uint32_t)(tt.re - tt.rb));
    return false;
  }
  bool ambiguous;
  pileup_ref(R, ca, pos, ctr, amb_in ? (int)amb_ref[L.li] : -1, refbase, ambiguous);
  if ((L.item.flags & 1) && !amb_in && !L.counted) {  // the list kernel did not count this tile's visits
    uint32_t kept = 0;
    for (int64_t k0 = 0; k0 < ca.n; k0 += 64) {
      bool act;
      const int64_t r = ca.read(R, k0 + lane, pos, &act);
      kept += (uint32_t)__popcll(__ballot(act && (min_mapq <= 0 || (int)R.mapq[r] >= min_mapq)));
    }
    if (kept && lane == 0) atomicAdd(&ctr->visited, 1ull);
    L.counted = true;
  }
  if (!amb_in && ambiguous) {  // heap order decides the reference base: list it
    if (lane == 0) {
      const unsigned long long k = atomicAdd(&ctr->n_amb, 1ull);
      if (k < amb_cap) amb_out[k] = AmbItem{L.item.tile, pos, L.it};
    }
    return false;
  }
  if (variants_only && (amb_in || (L.item.flags & 1))) {  // the list kernel could not decide here
    bool any = false;
    for (int64_t k0 = 0; k0 < ca.n; k0 += 64) {
      bool act;
      const int64_t r = ca.read(R, k0 + lane, pos, &act);
      bool nm = false;
      if (act && (min_mapq <= 0 || (int)R.mapq[r] >= min_mapq)) {
        AlleleDesc d;
        int errc = 0;
        if (classify(R, r, pos, refbase, d, &errc)) nm = !(d.kind == K_SNV && d.base == refbase);
      }
      any |= __ballot(nm) != 0;
    }
    if (!any) return false;
  }
  return true;
}

// ---- host: the loop around the launches --------------------------------------------------------

// A buffer that overflowed is grown to what the pass needed and the pass repeated; each buffer has
// its own budget of two growths (the heap-order pass can add to what the first one needed).
struct Growth {
  enum { ITEM, AMB, DEEP, OUT0 };  // OUT0 + k: a command's own buffers
  int grown[8] = {};
  bool spent = false, retry = false;
  bool operator()(int which, unsigned long long &cap, unsigned long long need, unsigned long long slack) {
    if (need <= cap) return false;
    if (++grown[which] > 2) spent = true;
    cap = need + slack;
    return retry = true;
  }
};

struct LocusLaunch {  // what the driver hands a command's launch
  const Tile *tiles;
  const ComplexItem *items;
  int64_t n_items;
  Counters *ctr;
  SomWin sw;
  AmbItem *amb_out;  // the heap-order loci this launch lists ...
  unsigned long long amb_cap;
  const AmbItem *amb_in;  // ... or the ones it replays, with their reference bases
  const uint8_t *amb_ref;
  int64_t n_amb_in;
};

struct ListedLoci {  // what the driver leaves a command
  Plan pl;           // n_tiles == 0: nothing to do, nothing below is set
  SomWin sw;
  Counters hc;       // the counters after the last launch, spread folded into visited
  Counters *ctr;
  int64_t n_items = 0;
};

// The loci of `loci` listed and every one run through a command's call kernel.
//   launch(deep, grid, LocusLaunch, DeepSel)   issues the command's kernel (its <deep> instantiation)
//                                              with its own output arguments.
//   outputs(hc, n_items, grow) -> gq_status    called once n_items is known and after each round:
//                                              ensures the command's own buffers at their current
//                                              capacities and grows the ones hc shows overflowed.
// name prefixes the capacity errors.  Events: ev[1] before the list kernel, ev[2] after it, ev[3]
// after the last call kernel.
template <class Launch, class Outputs>
gq_status run_listed_loci(gq_ctx *c, const gq_dev_reads *rd, const gq_loci *loci, int min_mapq, int variants_only,
                          const char *name, ListedLoci &L, Launch launch, Outputs outputs) {
  gq_status st = ensure_columns(c, rd);  // (the walker's clean fast path)
  if (st) return st;
  Plan &pl = L.pl;
  st = plan(c, rd, loci, kAeT, pl, c->tiles);
  if (st) return st;
  if (pl.n_tiles == 0) return GQ_OK;
  // pileup element order: each window's first visited locus and initial (heap-ordered) group
  L.sw = SomWin{};
  st = build_somwin(c, pl, rd, rd, L.sw);
  if (st) return st;
  if (c->n_cu <= 0 && hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess)
    c->n_cu = 256;
  unsigned long long item_cap = (unsigned long long)std::min<int64_t>(
                         pl.n_loci, std::max<int64_t>(pl.n_loci / 8, 1 << 16)),
                     amb_cap = 4096, deep_cap = 4096;
  Growth grow;
  Counters &hc = L.hc;
  hc = Counters{};
  auto read_counters = [&]() -> gq_status {
    HIP_TRY(hipMemcpyAsync(&hc, L.ctr, kCountersHead, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GQ_OK;
  };
  for (;;) {
    grow.retry = false;
    HIP_TRY(c->amb.ensure(amb_cap * sizeof(AmbItem)));
    HIP_TRY(c->cplx.ensure(item_cap * sizeof(ComplexItem)));
    HIP_TRY(c->counters.ensure(sizeof(Counters)));
    HIP_TRY(c->deep_list.ensure(deep_cap * sizeof(int64_t)));
    Counters *ctr = L.ctr = (Counters *)c->counters.p;
    HIP_TRY(hipMemsetAsync(ctr, 0, sizeof(Counters), c->stream));
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    // the loci to process, found tile-wise (a few resident workgroups per CU over the tiles)
    hipLaunchKernelGGL((allele_evidence_list<kAeT>), dim3((unsigned)std::min<int64_t>(pl.n_tiles, (int64_t)4 * c->n_cu)),
                       dim3(kBlock), 0, c->stream, (const Tile *)c->tiles.p, pl.n_tiles, rd->d, min_mapq, variants_only,
                       (ComplexItem *)c->cplx.p, item_cap, ctr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    st = read_counters();
    if (st) return st;
    if (hc.err) break;
    if (grow(Growth::ITEM, item_cap, hc.n_complex, 1024)) {
      if (grow.spent) return set_err(GQ_E_CAPACITY, "%s: locus list capacity retries exhausted", name);
      continue;
    }
    const int64_t n_items = L.n_items = (int64_t)hc.n_complex;
    if (n_items == 0) break;
    st = outputs(hc, n_items, grow);
    if (st) return st;
    int64_t *dl = (int64_t *)c->deep_list.p;
    const DeepSel fast{dl, deep_cap, nullptr, 0, nullptr, 0, 0};
    LocusLaunch a{(const Tile *)c->tiles.p, (const ComplexItem *)c->cplx.p, n_items, ctr, L.sw,
                  (AmbItem *)c->amb.p, amb_cap, nullptr, nullptr, 0};
    // n loci through the fast instantiation, then the ones its working set handed over
    // [from, hc.n_deep) through the deep one, same mode, its per-wave scratch sized from the
    // deepest of them
    auto run_pass = [&](int64_t n, int64_t from) -> gq_status {
      launch(false, (unsigned)std::min<int64_t>((n + kSomWaves - 1) / kSomWaves, 8192), a, fast);
      HIP_TRY(hipGetLastError());
      gq_status rs = read_counters();
      if (rs) return rs;
      const int64_t nd = (int64_t)std::min<unsigned long long>(hc.n_deep, deep_cap) - from;
      if (nd > 0 && !hc.err) {
        const int scap = (int)std::max<unsigned long long>(hc.deep_max, 64);
        const int64_t waves = std::min<int64_t>(nd, 256);
        HIP_TRY(c->deep_scratch.ensure((size_t)waves * gs_wave_bytes(scap, 16) + 256));
        const DeepSel deep{nullptr, deep_cap, dl + from, nd, (uint8_t *)c->deep_scratch.p, scap, 16};
        launch(true, (unsigned)((waves + kSomWaves - 1) / kSomWaves), a, deep);
        HIP_TRY(hipGetLastError());
        rs = read_counters();
        if (rs) return rs;
      }
      HIP_TRY(hipEventRecord(c->ev[3], c->stream));
      return GQ_OK;
    };
    st = run_pass(n_items, 0);
    if (st) return st;
    grow(Growth::AMB, amb_cap, hc.n_amb, 1024);
    grow(Growth::DEEP, deep_cap, hc.n_deep, 1024);
    if (!grow.retry && hc.n_amb > 0 && !hc.err) {  // heap-order reference bases: replay, then those loci again
      std::vector<AmbItem> amb((size_t)hc.n_amb);
      HIP_TRY(hipMemcpyAsync(amb.data(), c->amb.p, amb.size() * sizeof(AmbItem), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      HIP_TRY(c->amb_ref.ensure(amb.size()));
      st = heap_ref_bases(c, pl, c->tiles, {rd}, amb, (uint8_t *)c->amb_ref.p);
      if (st) return st;
      a.amb_out = nullptr;
      a.amb_cap = 0;
      a.amb_in = (const AmbItem *)c->amb.p;
      a.amb_ref = (const uint8_t *)c->amb_ref.p;
      a.n_amb_in = (int64_t)amb.size();
      st = run_pass((int64_t)amb.size(), (int64_t)hc.n_deep);
      if (st) return st;
      grow(Growth::DEEP, deep_cap, hc.n_deep, 1024);
    }
    st = outputs(hc, n_items, grow);
    if (st) return st;
    if (!grow.retry || hc.err) break;
    if (grow.spent) return set_err(GQ_E_CAPACITY, "%s: output capacity retries exhausted", name);
  }
  for (int k = 0; k < kSpread; ++k) hc.visited += hc.spread[0][k];
  return check_device_error(c, hc);
}
