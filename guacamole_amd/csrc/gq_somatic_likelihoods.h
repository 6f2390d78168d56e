// gq_somatic_likelihoods.h — somatic-likelihoods (gq_somatic_likelihoods_call): what
// SomaticStandard.Caller.findPotentialVariantAtLocus (commands/SomaticStandardCaller.scala:
// 162-245) computes before it keeps one allele and applies --odds: both samples' genotype
// likelihoods (Likelihood.scala:99-201, normalize = true), the most likely tumor genotype, the
// normal's variant mass and the somatic odds, at every locus that passes the caller's gate
// (:184-190, :200).  Included by gq_somatic.hip inside its anonymous namespace, after
// gq_somatic_call.h (CandRec, call_front, Pile, genotypes_el, DeepIO), gq_allele_evidence.h
// (ae_entry_u32) and gq_genotype_likelihoods.h (GlAllele).
//
//   somatic_likelihoods_k   one wave per listed locus (the candidate pass with the hom-ref bound
//                           off, then cand_prep).  The caller's front gives one element record per
//                           covering read of both samples; the pileup reference bases, the allele
//                           tables, the multi-allelic / mapq filters and the gate are the caller's.
//                           A group that passes reserves its record, its allele slots (tumor then
//                           normal) and its likelihood slots (tumor then normal) with one lane's
//                           atomicAdd each, then runs the tumor fold (IncludingAlignment) and the
//                           normal fold (IgnoringAlignment, with the variant mass in the immutable
//                           Map's order, gq_scala_order.h) through genotypes_el, which also stores
//                           each genotype's normalised log-likelihood in the group's slots.
//                           Instantiations and capacities are somatic_call_k's: records in LDS up
//                           to kFastCap elements per sample, 64 distinct alleles and kMaxG genotypes
//                           per sample (fast); per-wave HBM scratch, 128 alleles (deep); 1024
//                           alleles per sample and 256 eligible normal alleles (wide; past them
//                           GQ_E_CAPACITY).  Heap-order loci take the AmbItem round trip.
//   sl_keys / sl_counts / sl_place   the result image: groups sorted by locus ordinal (hipcub),
//                           per sorted group its tumor / normal allele counts, tumor / normal
//                           genotype counts and allele bytes scanned to offsets, then a wave per
//                           group writes every column.  Every store is bounded by the sizes the
//                           group recorded; a disagreement with the scanned totals is GQ_E_ASSERT.
#pragma once

struct SlGroup {  // one locus
  uint64_t key;   // locus ordinal
  int32_t contig, pos;
  int32_t depth[2];      // filtered depths (tumor, normal)
  int32_t n_alleles[2];  // eligible alleles
  uint64_t allele_at, geno_at;  // reserved slots: the tumor's first, the normal's right after
  uint32_t pool_bytes;          // ref + alt bytes of its alleles (both samples)
  int32_t best;                 // first maximum among the tumor genotypes
  double var_total, log_odds;
  uint8_t flags, ref_base[2], has_variant;
  uint8_t pad[4];
};
static_assert(sizeof(SlGroup) == 80, "SlGroup layout");

struct SlOut {
  SlGroup *groups;
  unsigned long long group_cap;
  GlAllele *alleles;
  unsigned long long allele_cap;
  double *ll;
  unsigned long long ll_cap;
  uint8_t *pool;
  unsigned long long pool_cap;
};

// The allele tables of both samples from the element records (somatic_call_k's table pass):
// every active element's allele key looked up / appended (entry j on lane j & 63, slot j >> 6),
// the counts before and after the mapq filter, and each record's table index.
template <int NS>
__device__ __forceinline__ void sl_tables(const DevReads &RT, const DevReads &RN, const int64_t (&rb)[2],
                                          const uint32_t (&nc)[2], int32_t pos, CallMem &m, Pile<NS> (&PS)[2]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const DevReads &R = s ? RN : RT;
    Pile<NS> &P = PS[s];
#pragma unroll
    for (int t = 0; t < NS; ++t) {
      P.klo[t] = P.khi[t] = 0;
      P.n_all[t] = P.n_f[t] = 0;
    }
    P.nt = 0;
    P.depth_all = P.depth_f = P.fwd_f = 0;
    P.overflow = false;
    for (uint32_t c0 = 0; c0 < nc[s]; c0 += 64) {
      const uint32_t k = c0 + lane;
      uint4 e = make_uint4(0, 0, 0, 0);
      if (k < nc[s]) e = m.el[s][k];
      const uint32_t fl = el_flags(e);
      const bool act = k < nc[s] && (fl & kElAct);
      const bool pass = act && (fl & kElPass);
      AlleleDesc d;
      d.read = rb[s] + (k < nc[s] ? m.cov[s][k] : 0);
      d.rp = (int32_t)e.x;
      d.aux = (int32_t)e.y;
      d.base = (uint8_t)(e.z & 0xFFu);
      d.kind = (uint8_t)((e.z >> 8) & 0xFFu);
      d.rb = P.refbase;
      d.pad = 0;
      Key128 key{0, 0};
      if (act) key = allele_key(R, d, pos, 0);
      const unsigned long long actb = __ballot(act), passb = __ballot(pass);
      P.depth_all += (uint32_t)__popcll(actb);
      P.depth_f += (uint32_t)__popcll(passb);
      P.fwd_f += (uint32_t)__popcll(__ballot(pass && (fl & kElFwd)));
      int mine = -1;
      unsigned long long pending = actb;
      while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const uint64_t klo = __shfl(key.lo, leader, 64), khi = __shfl(key.hi, leader, 64);
        const bool match = act && key.lo == klo && key.hi == khi;
        const unsigned long long mb = __ballot(match);
        const uint32_t na = (uint32_t)__popcll(mb), nf = (uint32_t)__popcll(mb & passb);
        int found = -1;
#pragma unroll
        for (int t = 0; t < NS; ++t) {
          const unsigned long long hb = __ballot((t * 64 + lane) < P.nt && P.klo[t] == klo && P.khi[t] == khi);
          if (found < 0 && hb) found = t * 64 + (__ffsll((long long)hb) - 1);
        }
        if (found < 0) {
          if (P.nt >= 64 * NS) {
            P.overflow = true;
          } else {
            found = P.nt++;
            const int owner = found & 63, sl = found >> 6;
            AlleleDesc ldsc;
            ldsc.read = __shfl(d.read, leader, 64);
            ldsc.aux = __shfl(d.aux, leader, 64);
            ldsc.rp = __shfl(d.rp, leader, 64);
            ldsc.kind = (uint8_t)__shfl((int)d.kind, leader, 64);
            ldsc.rb = P.refbase;
            ldsc.base = (uint8_t)__shfl((int)d.base, leader, 64);
            ldsc.pad = 0;
#pragma unroll
            for (int t = 0; t < NS; ++t)
              if (t == sl && lane == owner) {
                P.klo[t] = klo;
                P.khi[t] = khi;
                P.desc[t] = ldsc;
              }
          }
        }
        if (found >= 0) {
          const int owner = found & 63, sl = found >> 6;
#pragma unroll
          for (int t = 0; t < NS; ++t)
            if (t == sl && lane == owner) {
              P.n_all[t] += na;
              P.n_f[t] += nf;
            }
          if (match) mine = found;
        }
        pending &= ~mb;
      }
      if (act && mine >= 0) m.el[s][k].w = (e.w & 0x0007FFFFu) | ((uint32_t)mine << 19);
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// A sample's eligible alleles in Allele order (m.order, as the fold just ranked them) into the
// group's allele slots [at, at + n): ref / alt bytes inline up to 8, longer ones through the pool.
template <int NS>
__device__ __forceinline__ uint32_t sl_write_alleles(const DevReads &R, const Pile<NS> &P, int n, int32_t pos,
                                                     const CallMem &m, const SlOut &out, unsigned long long at,
                                                     Counters *ctr) {
  const int lane = threadIdx.x & 63;
  uint32_t pool_bytes = 0;
  for (int a = 0; a < n; ++a) {
    const int j = m.order[a];
    const AlleleDesc al = pile_entry(P, j);
    const int rl = allele_ref_len(al), alt_l = allele_alt_len(al);
    GlAllele ar;
    ar.depth = (int32_t)ae_entry_u32<NS>(P.n_f, j);
    ar.ref_len = (uint16_t)rl;
    ar.alt_len = (uint16_t)alt_l;
    pool_bytes += (uint32_t)(rl + alt_l);
    if (rl + alt_l <= 8) {
      uint64_t v = 0;
      int q = 0;
      for (int i = 0; i < rl; ++i) v |= (uint64_t)allele_byte(R, al, pos, 0, i) << (8 * q++);
      for (int i = 0; i < alt_l; ++i) v |= (uint64_t)allele_byte(R, al, pos, 1, i) << (8 * q++);
      ar.allele = v;
    } else {
      unsigned long long o = 0;
      if (lane == 0) o = atomicAdd(&ctr->pool_used, (unsigned long long)(rl + alt_l));
      o = __shfl(o, 0, 64);
      if (o + rl + alt_l <= out.pool_cap)
        for (int i = lane; i < rl + alt_l; i += 64)
          out.pool[o + i] = i < rl ? allele_byte(R, al, pos, 0, i) : allele_byte(R, al, pos, 1, i - rl);
      ar.allele = o;
    }
    if (lane == 0) out.alleles[at + a] = ar;
  }
  return pool_bytes;
}

// The register budget is somatic_call_k's: 3 waves per SIMD for the fast instantiation, 2 for the
// deep ones.
template <bool DEEP, int NSD = kSlots>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(DEEP ? 2 : 3))) void somatic_likelihoods_k(
    const CandRec *__restrict__ cands, DevReads RT, DevReads RN, gq_somatic_params prm, SlOut out, Counters *ctr,
    SomWin sw, AmbItem *__restrict__ amb_out, unsigned long long amb_cap, const AmbItem *__restrict__ amb_in,
    const uint8_t *__restrict__ amb_ref, int64_t n_amb_in, int dbg, DeepIO dio) {
  // amb_in == nullptr: the listed loci (fast kernel) or the deep list (deep kernel); loci where a
  // sample's MD-derived reference bases disagree are listed (amb_out) for the heap-order replay.
  // amb_in != nullptr (deep kernels only): those loci with both samples' bases resolved
  // (amb_ref[2 i + set]).  prm: min_mapq, filter_multi_allelic and max_read_depth are read.
  constexpr int FW = kSomWaves;
  constexpr int NS = DEEP ? NSD : 1;  // allele-table slots: 64 NS distinct alleles per sample
  __shared__ int32_t s_cov[DEEP ? 1 : FW][2][kFastCap];
  __shared__ uint4 s_el[DEEP ? 1 : FW][2][kFastCap];
  __shared__ uint32_t s_tmp[DEEP ? 1 : FW][2 * kFastCap];
  __shared__ int16_t s_order[DEEP ? 1 : FW][64 * NS];
  __shared__ uint8_t s_var[DEEP ? 1 : FW][64 * NS];
  __shared__ double s_ll[DEEP ? 1 : FW][kMaxG];
  __shared__ TermRec s_terms[FW][DEEP ? kDeepTermCap : kFastCap];
  __shared__ double s_succ[256];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t gwave = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t nwaves_total = ((int64_t)gridDim.x * blockDim.x) >> 6;
  CallMem m;
  if constexpr (DEEP) {
    m = deep_mem(dio.scratch + (size_t)gwave * deep_wave_bytes(dio.scap, dio.maxG, NS), dio.scap, dio.maxG, NS);
    m.terms = s_terms[wv];
    m.tcap = kDeepTermCap;
  } else {
    m.cov[0] = s_cov[wv][0];
    m.cov[1] = s_cov[wv][1];
    m.el[0] = s_el[wv][0];
    m.el[1] = s_el[wv][1];
    m.tmp = s_tmp[wv];
    m.order = s_order[wv];
    m.is_var = s_var[wv];
    m.ll = s_ll[wv];
    m.gkey = nullptr;
    m.gsum = nullptr;
    m.terms = s_terms[wv];
    m.tcap = kFastCap;
    m.cap = kFastCap;
    m.maxG = kMaxG;
  }
  // amb_sel: a heap-order replay over the amb_in positions listed in dio.list (the wide kernel
  // over the replayed loci the deep kernel's table could not hold), not over all of amb_in
  const bool amb_sel = DEEP && amb_in != nullptr && dio.n_in > 0;
  const unsigned long long n_items = amb_sel  ? (unsigned long long)dio.n_in
                                     : amb_in ? (unsigned long long)n_amb_in
                                     : DEEP ? (unsigned long long)dio.n_in
                                            : ctr->part_off[1][kParts];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) s_succ[i] = g_succ[i];
  __syncthreads();
  m.succ = s_succ;
  // (la: the item's position in amb_in, whose resolved reference bases it reads)
  auto fetch_item = [&](int64_t li, int64_t &it, int64_t &la) -> CandRec {
    la = amb_sel ? dio.list[li] : li;
    it = amb_in ? amb_in[la].item : DEEP ? dio.list[li] : li;
    return cands[it];
  };
  int64_t it_next = 0, la_next = 0;
  CandRec item_next{};
  if (gwave < (int64_t)n_items) item_next = fetch_item(gwave, it_next, la_next);
  for (int64_t li = gwave; li < (int64_t)n_items; li += nwaves_total) {
    const int64_t it = it_next, la = la_next;
    const CandRec item = item_next;
    if (li + nwaves_total < (int64_t)n_items) item_next = fetch_item(li + nwaves_total, it_next, la_next);
    const int32_t pos = item.pos;
    const int64_t rb[2] = {item.rb[0], item.rb[1]};
    uint32_t nc[2], mask[2];
    if (!call_front<DEEP>(item, it, RT, RN, prm, ctr, sw, m, dbg, dio, nc, mask)) continue;
    Pile<NS> PS[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      uint32_t mk = mask[s];
      for (int d = 1; d < 64; d <<= 1) mk |= __shfl_xor(mk, d, 64);
      PS[s].ambiguous = __popc(mk) > 1;
      PS[s].refbase = amb_in ? amb_ref[2 * la + s] : mk ? bit_base(mk) : (uint8_t)'N';
    }
    sl_tables<NS>(RT, RN, rb, nc, pos, m, PS);
    Pile<NS> &PT = PS[0], &PN = PS[1];
    // a table or a genotype count past this kernel's working set: the next kernel up
    auto too_many_g = [&](const DevReads &R, const Pile<NS> &P) {
      int n = 0;
#pragma unroll
      for (int t = 0; t < NS; ++t)
        n += __popcll(__ballot((t * 64 + lane) < P.nt && P.n_f[t] > 0 && allele_std_alt(R, P.desc[t], pos)));
      return n * (n + 1) / 2 > m.maxG;
    };
    if (PT.overflow || PN.overflow || too_many_g(RT, PT) || too_many_g(RN, PN)) {
      if constexpr (!DEEP) {
        if (lane == 0) {
          const unsigned long long k = atomicAdd(&ctr->n_deep, 1ull);
          if (k < dio.cap) dio.list[k] = it;
          atomicMax(&ctr->deep_max, (unsigned long long)max(nc[0], nc[1]));
        }
      } else if (NS < kWideNS) {  // (a replayed locus by its position in amb_in, with its resolved bases)
        if (lane == 0) {
          const unsigned long long k = atomicAdd(&ctr->n_wide, 1ull);
          if (k < dio.wcap) dio.wide[k] = amb_in ? la : it;
        }
      } else {
        raise_at(ctr, GQ_E_CAPACITY, pos);
      }
      continue;
    }
    if ((item.flags & 1) && !amb_in && (PT.depth_all + PN.depth_all) > 0 && lane == 0)
      atomicAdd(&ctr->spread[0][it & (kSpread - 1)], 1ull);
    if (!amb_in && (PT.ambiguous || PN.ambiguous)) {  // heap order decides a reference base: list it
      if (lane == 0) {
        const unsigned long long k = atomicAdd(&ctr->n_amb, 1ull);
        if (k < amb_cap) amb_out[k] = AmbItem{item.tile, pos, it};
        atomicMax(&ctr->deep_max, (unsigned long long)max(nc[0], nc[1]));
      }
      continue;
    }
    if (prm.filter_multi_allelic) {  // MultiAllelicPileupFilter (PileupFilter.scala:29-44)
      if (PT.nt > 2) PT.depth_f = 0;
      if (PN.nt > 2) PN.depth_f = 0;
    }
    // the gate, SomaticStandardCaller.scala:184-190
    if (PT.depth_f == 0 || PN.depth_f == 0 || (int64_t)PT.depth_f > (int64_t)prm.max_read_depth ||
        (int64_t)PN.depth_f > (int64_t)prm.max_read_depth)
      continue;
    {  // the tumor pileup must hold a non-Match element: Match = allele (ref, ref) of one byte
      uint32_t ref_match = 0;
#pragma unroll
      for (int t = 0; t < NS; ++t) {
        const bool mt = (t * 64 + lane) < PT.nt && PT.desc[t].kind == K_SNV && PT.desc[t].base == PT.refbase;
        ref_match += (uint32_t)wave_sum(mt ? (double)PT.n_f[t] : 0.0);
      }
      if (ref_match == PT.depth_f) continue;
    }
    // eligible alleles (Likelihood.scala:106); none in the tumor: an empty Seq, no group (:200)
    auto n_eligible = [&](const DevReads &R, const Pile<NS> &P) {
      int n = 0;
#pragma unroll
      for (int t = 0; t < NS; ++t)
        n += __popcll(__ballot((t * 64 + lane) < P.nt && P.n_f[t] > 0 && allele_std_alt(R, P.desc[t], pos)));
      return n;
    };
    const int naT = n_eligible(RT, PT), naN = n_eligible(RN, PN);
    if (naT == 0) continue;
    const int GT = naT * (naT + 1) / 2, GN = naN * (naN + 1) / 2;
    // the group's output slots, one lane's atomicAdd each
    unsigned long long gk = 0, a_at = 0, g_at = 0;
    if (lane == 0) {
      gk = atomicAdd(&ctr->n_rec, 1ull);
      a_at = atomicAdd(&ctr->n_out, (unsigned long long)(naT + naN));
      g_at = atomicAdd(&ctr->out_pool, (unsigned long long)(GT + GN));
    }
    gk = __shfl(gk, 0, 64);
    a_at = __shfl(a_at, 0, 64);
    g_at = __shfl(g_at, 0, 64);
    // past a capacity: the host grows the buffers and calls again
    if (gk >= out.group_cap || a_at + (unsigned long long)(naT + naN) > out.allele_cap ||
        g_at + (unsigned long long)(GT + GN) > out.ll_cap)
      continue;
    const GenoOut tg = genotypes_el(RT, PT, m.el[0], (int)nc[0], pos, true, false, m, ctr, out.ll + g_at);
    if (tg.G != GT) {  // (the counts above are the fold's own)
      raise_at(ctr, GQ_E_ASSERT, pos);
      continue;
    }
    const bool t_var = m.is_var[tg.bi] || m.is_var[tg.bj];
    uint32_t pool_bytes = sl_write_alleles<NS>(RT, PT, naT, pos, m, out, a_at, ctr);
    __builtin_amdgcn_wave_barrier();  // (the normal's fold rewrites the order and the variant marks)
    const GenoOut ng = genotypes_el(RN, PN, m.el[1], (int)nc[1], pos, false, true, m, ctr, out.ll + g_at + GT);
    if (ng.G != GN) {
      raise_at(ctr, GQ_E_ASSERT, pos);
      continue;
    }
    pool_bytes += sl_write_alleles<NS>(RN, PN, naN, pos, m, out, a_at + (unsigned long long)naT, ctr);
    const double nvs = ng.G == 0 ? 0.0 : ng.var_sum;
    if (lane == 0) {
      SlGroup gr;
      gr.key = (uint64_t)(item.ord0 + (pos - item.L0));
      gr.contig = item.contig;
      gr.pos = pos;
      gr.depth[0] = (int32_t)PT.depth_f;
      gr.depth[1] = (int32_t)PN.depth_f;
      gr.n_alleles[0] = naT;
      gr.n_alleles[1] = naN;
      gr.allele_at = a_at;
      gr.geno_at = g_at;
      gr.pool_bytes = pool_bytes;
      gr.best = tg.best_g;
      gr.var_total = nvs;
      gr.log_odds = sm::log(tg.best_l / nvs);  // SomaticStandardCaller.scala:218, 236
      gr.flags = (uint8_t)((PT.ambiguous ? 1 : 0) | (PN.ambiguous ? 2 : 0));
      gr.ref_base[0] = PT.refbase;
      gr.ref_base[1] = PN.refbase;
      gr.has_variant = t_var ? 1 : 0;
      gr.pad[0] = gr.pad[1] = gr.pad[2] = gr.pad[3] = 0;
      out.groups[gk] = gr;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- the result image: groups by locus ordinal, their alleles and likelihoods at the scanned offsets
struct Sl5 {  // per sorted group: tumor alleles, normal alleles, tumor genotypes, normal genotypes, allele bytes
  int64_t *ta, *na, *tg, *ng, *p;
};

struct SlLayout {  // byte offsets inside the image; header = int64 pool_len, int64 disagreements
  size_t contig, pos, flags, t_ref_base, n_ref_base, t_depth, n_depth, t_n_alleles, n_n_alleles, t_allele_first,
      n_allele_first, t_geno_first, n_geno_first, best, has_variant, var_total, log_odds;  // per group
  size_t a_ref_off[2], a_ref_len[2], a_alt_off[2], a_alt_len[2], a_depth[2];             // per allele (tumor, normal)
  size_t ll[2], pool, bytes;
  int64_t n_alleles[2], n_geno[2], pool_cap;  // the totals the columns were sized for
};

__global__ void sl_keys(const SlGroup *__restrict__ groups, int64_t n, uint64_t *__restrict__ keys,
                        uint32_t *__restrict__ slot) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  keys[k] = groups[k].key;
  slot[k] = (uint32_t)k;
}

__global__ void sl_counts(const SlGroup *__restrict__ groups, const uint32_t *__restrict__ order, int64_t n, Sl5 cnt) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const SlGroup &g = groups[order[k]];
  const int64_t a = g.n_alleles[0], b = g.n_alleles[1];
  cnt.ta[k] = a;
  cnt.na[k] = b;
  cnt.tg[k] = a * (a + 1) / 2;
  cnt.ng[k] = b * (b + 1) / 2;
  cnt.p[k] = (int64_t)g.pool_bytes;
}

// Group k of the output (slot order[k]), one wave per group: its columns, each sample's alleles
// (their bytes at the group's pool offset, tumor then normal, in turn) and likelihoods.  A group
// whose recorded sizes do not fit the columns' totals is counted (image byte 8) and not placed.
__global__ __launch_bounds__(kBlock) void sl_place(const SlGroup *__restrict__ groups, const uint32_t *__restrict__ order,
                                                   Sl5 off, const GlAllele *__restrict__ alleles,
                                                   const double *__restrict__ ll, const uint8_t *__restrict__ dpool,
                                                   int64_t n, SlLayout L, uint8_t *__restrict__ img) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; k < n; k += nw) {
    const SlGroup g = groups[order[k]];
    const int64_t oa[2] = {off.ta[k], off.na[k]}, og[2] = {off.tg[k], off.ng[k]}, op = off.p[k];
    const int64_t na[2] = {g.n_alleles[0], g.n_alleles[1]};
    const int64_t G[2] = {na[0] * (na[0] + 1) / 2, na[1] * (na[1] + 1) / 2};
    if (na[0] < 0 || na[1] < 0 || oa[0] + na[0] > L.n_alleles[0] || oa[1] + na[1] > L.n_alleles[1] ||
        og[0] + G[0] > L.n_geno[0] || og[1] + G[1] > L.n_geno[1] || op + (int64_t)g.pool_bytes > L.pool_cap ||
        g.best < 0 || g.best >= G[0]) {
      if (lane == 0) atomicAdd((unsigned long long *)(img + 8), 1ull);
      continue;
    }
    if (lane == 0) {
      ((int32_t *)(img + L.contig))[k] = g.contig;
      ((int64_t *)(img + L.pos))[k] = g.pos;
      img[L.flags + k] = g.flags;
      img[L.t_ref_base + k] = g.ref_base[0];
      img[L.n_ref_base + k] = g.ref_base[1];
      ((int32_t *)(img + L.t_depth))[k] = g.depth[0];
      ((int32_t *)(img + L.n_depth))[k] = g.depth[1];
      ((int32_t *)(img + L.t_n_alleles))[k] = g.n_alleles[0];
      ((int32_t *)(img + L.n_n_alleles))[k] = g.n_alleles[1];
      ((int64_t *)(img + L.t_allele_first))[k] = oa[0];
      ((int64_t *)(img + L.n_allele_first))[k] = oa[1];
      ((int64_t *)(img + L.t_geno_first))[k] = og[0];
      ((int64_t *)(img + L.n_geno_first))[k] = og[1];
      ((int32_t *)(img + L.best))[k] = g.best;
      img[L.has_variant + k] = g.has_variant;
      ((double *)(img + L.var_total))[k] = g.var_total;
      ((double *)(img + L.log_odds))[k] = g.log_odds;
      if (k == n - 1) *(int64_t *)img = op + g.pool_bytes;
    }
    int64_t at = op;
    const int64_t pool_end = op + (int64_t)g.pool_bytes;
    bool bad = false;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const uint64_t src = g.allele_at + (s ? (uint64_t)na[0] : 0);
      for (int64_t a0 = 0; a0 < na[s]; a0 += 64) {
        const int64_t a = a0 + lane;
        GlAllele r{};
        if (a < na[s]) r = alleles[src + a];
        const int tot = r.ref_len + r.alt_len;
        int x = tot;  // inclusive scan of the lengths
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int y = __shfl_up(x, d, 64);
          if (lane >= d) x += y;
        }
        if (a < na[s]) {
          const int64_t q = oa[s] + a, p = at + x - tot;
          ((int64_t *)(img + L.a_ref_off[s]))[q] = p;
          ((int32_t *)(img + L.a_ref_len[s]))[q] = r.ref_len;
          ((int64_t *)(img + L.a_alt_off[s]))[q] = p + r.ref_len;
          ((int32_t *)(img + L.a_alt_len[s]))[q] = r.alt_len;
          ((int32_t *)(img + L.a_depth[s]))[q] = r.depth;
          if (p + tot > pool_end) {  // (the alleles' lengths exceed the bytes the group recorded)
            bad = true;
          } else {
            uint8_t *w = img + L.pool + p;
            if (tot <= 8)
              for (int i = 0; i < tot; ++i) w[i] = (uint8_t)(r.allele >> (8 * i));
            else
              for (int i = 0; i < tot; ++i) w[i] = dpool[r.allele + (uint64_t)i];
          }
        }
        at += __shfl(x, 63, 64);
      }
      double *w = (double *)(img + L.ll[s]) + og[s];
      const double *src_ll = ll + g.geno_at + (s ? (uint64_t)G[0] : 0);
      for (int64_t q = lane; q < G[s]; q += 64) w[q] = src_ll[q];
    }
    if (__ballot(bad) != 0 && lane == 0) atomicAdd((unsigned long long *)(img + 8), 1ull);
  }
}
