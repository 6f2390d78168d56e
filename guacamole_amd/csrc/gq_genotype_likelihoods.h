// gq_genotype_likelihoods.h — genotype-likelihoods (gq_genotype_likelihoods_call):
// Likelihood.likelihoodsOfAllPossibleGenotypesFromPileup (likelihood/Likelihood.scala:99-201),
// logSpace = true, prior 1, for every sample's mapq-filtered pileup at the listed loci.
// Included by gq_somatic.hip inside its anonymous namespace, after gq_locus_driver.h (the locus
// list, the per-locus prologue, the host loop) and gq_allele_evidence.h (whose ae_entry_u32 reads a
// table column).
//
//   genotype_likelihoods_call  one wave per listed locus.  Per sample: the cover list in pileup
//                              element order and the allele table (make_cover, gather_sample), the
//                              rank of each eligible allele (filtered count > 0, standard alt bases)
//                              by Allele order, then ONE walk over the cover, 64 elements at a time
//                              from the last chunk to the first: each kept element is classified
//                              once, its allele resolved to its rank (or "none"), its three possible
//                              terms log(pc + pc), log(pc + (1 - pc)), log((1 - pc) + (1 - pc))
//                              computed once with StrictMath's log, and the four values stored in a
//                              64-entry LDS element buffer.  Lanes = genotypes then fold the buffer
//                              from its last entry to its first (the Colt aggregate order, see
//                              fold_genotypes): every lane reads the same entry (an LDS broadcast)
//                              and picks its term by comparing the entry's rank with its own (i, j).
//                              Genotypes past 64 take further rounds over the same buffer; the
//                              running sums wait in `ll` between chunks.  Because the buffer holds a
//                              chunk, not the pileup, its size does not depend on the depth.
//                              Fast instantiation: cover lists (kCover) and kMaxG sums in LDS; a
//                              locus past the cover list, the 128-allele table or kMaxG genotypes
//                              goes to the deep instantiation (covers in per-wave HBM scratch, 1024
//                              alleles, the sums in the group's own output slots).
//   gl_counts / gl_place       the result image: per sorted group its allele, genotype and allele-
//                              byte counts (scanned by hipcub), then a wave per group writes the
//                              group columns, its alleles and its likelihoods at their offsets.
#pragma once

constexpr int kGlTh = 384;          // reads of a window's initial group make_cover reorders in the work area
constexpr int kGlWork = 2 * kGlTh;  // words of a wave's work area

struct GlElem {  // one kept element: its three possible terms and its allele's rank (-1: not eligible)
  double t2, th, t0;
  int32_t rank, pad;
};
static_assert(sizeof(GlElem) == 32, "GlElem layout");
// the work area after make_cover: 64 elements, then the fast path's kMaxG running sums
static_assert(64 * sizeof(GlElem) + kMaxG * sizeof(double) <= kGlWork * sizeof(uint32_t), "work area");

struct GlGroup {  // one (locus, sample)
  uint64_t key;   // locus ordinal << 12 | sample
  int32_t contig, pos;
  int32_t depth, n_alleles;
  uint64_t allele_at, geno_at;  // the group's reserved slots in the allele records / likelihoods
  uint32_t pool_bytes;          // ref + alt bytes of its alleles
  uint8_t flags, sample, pad[2];
};
static_assert(sizeof(GlGroup) == 48, "GlGroup layout");

struct GlAllele {
  uint64_t allele;  // ref then alt bytes: inline when they fit 8 bytes, else a pool offset
  int32_t depth;
  uint16_t ref_len, alt_len;
};
static_assert(sizeof(GlAllele) == 16, "GlAllele layout");

struct GlOut {
  GlGroup *groups;
  unsigned long long group_cap;
  GlAllele *alleles;
  unsigned long long allele_cap;
  double *ll;
  unsigned long long ll_cap;
  uint8_t *pool;
  unsigned long long pool_cap;
};

// Genotype g of n alleles -> (i <= j), row-major: rows before i hold S(i) = i n - i (i - 1) / 2.
__device__ __forceinline__ void gl_index(int g, int n, int &i, int &j) {
  auto S = [&](int x) { return (long long)x * n - (long long)x * (x - 1) / 2; };
  const double b = 2.0 * (double)n + 1.0;
  int r = (int)((b - sqrt(fmax(b * b - 8.0 * (double)g, 0.0))) * 0.5);
  r = max(0, min(r, n - 1));
  while (r > 0 && S(r) > g) --r;
  while (r + 1 < n && S(r + 1) <= g) ++r;
  i = r;
  j = r + (int)(g - S(r));
}

template <bool DEEP>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(DEEP ? 1 : 2))) void genotype_likelihoods_call(
    const Tile *__restrict__ tiles, const ComplexItem *__restrict__ items, int64_t n_items, DevReads R,
    gq_genotype_likelihood_params prm, GlOut out, Counters *ctr, SomWin sw, AmbItem *__restrict__ amb_out,
    unsigned long long amb_cap, const AmbItem *__restrict__ amb_in, const uint8_t *__restrict__ amb_ref,
    int64_t n_amb_in, DeepSel dd) {
  constexpr int NS = DEEP ? kDeepNS : kSlots;
  constexpr int FW = DEEP ? 1 : kSomWaves;
  __shared__ __attribute__((aligned(16))) uint32_t work[kSomWaves][kGlWork];
  __shared__ int32_t cover_a[FW][kCover], cover_s[FW][kCover];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  const int64_t gwave = wave_id();
  const int64_t nwaves_total = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const GsMem m = locus_mem<DEEP>(dd, cover_a[DEEP ? 0 : wv], cover_s[DEEP ? 0 : wv], work[wv], kGlTh, kMaxG);
  GlElem *const eb = reinterpret_cast<GlElem *>(work[wv]);
  double *const ll_lds = reinterpret_cast<double *>(work[wv] + 64 * sizeof(GlElem) / sizeof(uint32_t));
  const int min_mapq = prm.min_mapq;
  const bool incl_align = prm.include_alignment != 0;
  const int64_t n = locus_count<DEEP>(dd, amb_in, n_amb_in, n_items);
  for (int64_t si = gwave; si < n; si += nwaves_total) {
    LocusItem L = locus_item<DEEP>(si, tiles, items, sw, amb_in, dd);
    Cover ca;
    uint8_t refbase;
    if (!locus_open<DEEP>(R, L, m, sw, ctr, min_mapq, prm.variants_only, amb_out, amb_cap, amb_in, amb_ref, dd, false, ca,
                          refbase))
      continue;
    const Tile &tt = L.tt;
    const int32_t pos = L.pos, win = L.win;
    const int smp0 = L.smp0;
    auto hand_over = [&](int smp, uint32_t depth) { locus_hand_over<DEEP>(ctr, dd, L, smp, depth); };
    for (int smp = smp0; smp < R.n_samples; ++smp) {
      const Cover cs = R.n_samples == 1 ? ca
                                        : make_cover(R, tt.rb, tt.re, pos, m.cov_s, m.ev, m.cap, m.th, sw.wi[2 * win],
                                                     sw.init_reads, sw.init_rank, ctr, smp);
      if (cs.deep) {
        hand_over(smp, (uint32_t)(tt.re - tt.rb));
        break;
      }
      SamplePile<NS> P;
      gather_sample(R, cs, pos, min_mapq, refbase, ctr, P);
      if (P.overflow) {
        hand_over(smp, (uint32_t)max(cs.n, ca.n));  // (the deep pass covers every sample again)
        break;
      }
      if (P.depth_f == 0) continue;  // the sample is not in the filtered pileup
      // the eligible alleles and each one's rank among them by Allele order (-1: not eligible)
      bool elig[NS];
      int rnk[NS];
      int na = 0;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        elig[s] = (s * 64 + lane) < P.nt && P.n_f[s] > 0 && allele_std_alt(R, P.desc[s], pos);
        na += __popcll(__ballot(elig[s]));
        rnk[s] = elig[s] ? 0 : -1;
      }
      if (na == 0) continue;  // no allele with standard bases: an empty Seq
      const int G = na * (na + 1) / 2;
      if (!DEEP && G > kMaxG) {
        hand_over(smp, (uint32_t)max(cs.n, ca.n));
        break;
      }
      for (int k = 0; k < P.nt; ++k) {
        bool ek = false;
#pragma unroll
        for (int s = 0; s < NS; ++s)
          if (s == (k >> 6)) ek = __shfl((int)elig[s], k & 63, 64) != 0;
        if (!ek) continue;
        const AlleleDesc dk = pile_desc(P, k);
#pragma unroll
        for (int s = 0; s < NS; ++s)
          if (elig[s] && k != s * 64 + lane && allele_cmp(R, dk, P.desc[s], pos) < 0) ++rnk[s];
      }
      // the group's output slots, one lane's atomicAdd each
      unsigned long long gk = 0, a_at = 0, g_at = 0;
      if (lane == 0) {
        gk = atomicAdd(&ctr->n_rec, 1ull);
        a_at = atomicAdd(&ctr->n_out, (unsigned long long)na);
        g_at = atomicAdd(&ctr->out_pool, (unsigned long long)G);
      }
      gk = __shfl(gk, 0, 64);
      a_at = __shfl(a_at, 0, 64);
      g_at = __shfl(g_at, 0, 64);
      // past a capacity: the host grows the buffers and calls again
      if (gk >= out.group_cap || a_at + (unsigned long long)na > out.allele_cap ||
          g_at + (unsigned long long)G > out.ll_cap)
        continue;
      double *const ll = DEEP ? out.ll + g_at : ll_lds;
      // the walk: chunks of 64 elements from the last to the first
      bool started = false;
      for (int64_t c0 = ((cs.n - 1) / 64) * 64; c0 >= 0; c0 -= 64) {
        bool act;
        const int64_t r = cs.read(R, c0 + lane, pos, &act);
        Key128 key{0, 0};
        double t2 = 0.0, th = 0.0, t0 = 0.0;
        bool pass = false;
        if (act) {
          AlleleDesc d;
          int errc = 0;
          const int mq = (int)R.mapq[r];  // issued with classify's loads
          const int64_t so = R.seq_off[r];
          if (classify(R, r, pos, refbase, d, &errc) && (min_mapq <= 0 || mq >= min_mapq)) {
            pass = true;  // (classify's errors were raised by gather_sample)
            key = allele_key(R, d, pos, 0);
            const int q = elem_quality(R, d, so, mq);
            if (q < 0) raise_at(ctr, GQ_E_ASSERT, pos);  // PhredUtils: negative phred
            double pc = phred_success(q);
            if (incl_align) pc = pc * phred_success(mq);  // probabilityCorrectIncludingAlignment
            const double pw = 1.0 - pc;
            t2 = sm::log(pc + pc);
            th = sm::log(pc + pw);
            t0 = sm::log(pw + pw);
          }
        }
        const unsigned long long passb = __ballot(pass);
        if (!passb) continue;
        // each element's allele -> its rank among the eligible alleles
        int er = -1;
        unsigned long long pending = passb;
        while (pending) {
          const int leader = __ffsll((long long)pending) - 1;
          const uint64_t klo = __shfl(key.lo, leader, 64), khi = __shfl(key.hi, leader, 64);
          const bool match = pass && key.lo == klo && key.hi == khi;
          pending &= ~__ballot(match);
          int found = -1;
#pragma unroll
          for (int s = 0; s < NS; ++s) {
            const bool hit = (s * 64 + lane) < P.nt && P.klo[s] == klo && P.khi[s] == khi;
            const unsigned long long hb = __ballot(hit);
            if (found < 0 && hb) found = s * 64 + (__ffsll((long long)hb) - 1);
          }
          if (found < 0) {  // (the table was built from these very elements)
            raise_at(ctr, GQ_E_ASSERT, pos);
            continue;
          }
          int rr = -1;
#pragma unroll
          for (int s = 0; s < NS; ++s)
            if (s == (found >> 6)) rr = __shfl(rnk[s], found & 63, 64);
          if (match) er = rr;
        }
        __builtin_amdgcn_wave_barrier();  // the previous chunk's readers are done
        if (pass) eb[__popcll(passb & lt_mask)] = GlElem{t2, th, t0, er, 0};
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const int cnt = (int)__popcll(passb);
        for (int g0 = 0; g0 < G; g0 += 64) {
          const int g = g0 + lane;
          int gi = -2, gj = -2;
          if (g < G) gl_index(g, na, gi, gj);
          double acc = (started && g < G) ? ll[g] : 0.0;
          bool st = started;
#pragma unroll 4
          for (int e = cnt - 1; e >= 0; --e) {
            const GlElem x = eb[e];
            const bool m1 = x.rank == gi, m2 = x.rank == gj;
            const double term = (m1 && m2) ? x.t2 : (m1 || m2) ? x.th : x.t0;
            acc = st ? acc + term : term;
            st = true;
          }
          if (g < G) ll[g] = acc;
        }
        started = true;
      }
      // + log(prior = 1) - ln 2 * depth (Likelihood.scala:185-187)
      const double ln2d = sm::log(2.0) * (double)P.depth_f;
      for (int g = lane; g < G; g += 64) ll[g] = ll[g] + sm::log(1.0) - ln2d;
      double lt = 0.0;
      if (prm.normalize) {  // the exp(ll) added genotype by genotype, then its log (:191-193)
        double tot = 0.0;
        for (int g0 = 0; g0 < G; g0 += 64) {
          const double e = (g0 + lane < G) ? sm::exp(ll[g0 + lane]) : 0.0;
          for (int j = 0; j < 64 && g0 + j < G; ++j) tot = tot + lane_f64(e, j);
        }
        lt = sm::log(tot);
      }
      for (int g = lane; g < G; g += 64) out.ll[g_at + g] = prm.normalize ? ll[g] - lt : ll[g];
      // the alleles in rank order
      uint32_t pool_bytes = 0;
      for (int a = 0; a < na; ++a) {
        int j = -1;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const unsigned long long hb = __ballot(elig[s] && rnk[s] == a);
          if (j < 0 && hb) j = s * 64 + (__ffsll((long long)hb) - 1);
        }
        if (j < 0) {  // (Allele order is total over distinct alleles)
          raise_at(ctr, GQ_E_ASSERT, pos);
          continue;
        }
        const AlleleDesc al = pile_desc(P, j);
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
        if (lane == 0) out.alleles[a_at + a] = ar;
      }
      if (lane == 0) {
        GlGroup gr;
        gr.key = ((uint64_t)(tt.ordinal0 + (pos - tt.L0)) << 12) | (uint64_t)smp;
        gr.contig = tt.contig;
        gr.pos = pos;
        gr.depth = (int32_t)P.depth_f;
        gr.n_alleles = na;
        gr.allele_at = a_at;
        gr.geno_at = g_at;
        gr.pool_bytes = pool_bytes;
        gr.flags = amb_in ? 1 : 0;
        gr.sample = (uint8_t)smp;
        gr.pad[0] = gr.pad[1] = 0;
        out.groups[gk] = gr;
      }
      __builtin_amdgcn_wave_barrier();  // the next sample's cover reorder reuses the work area
    }
  }
}

// ---- the result image: groups by key, their alleles and likelihoods at the scanned offsets
struct Gl3 {  // per sorted group, three columns of n: alleles, genotypes, allele bytes (counts, or scanned offsets)
  int64_t *a, *g, *p;
};

struct GlLayout {  // byte offsets inside the image; header = int64 pool_len
  size_t contig, pos, sample, depth, n_alleles, allele_first, geno_first, flags;  // per group
  size_t ref_off, ref_len, alt_off, alt_len, allele_depth;                        // per allele
  size_t ll, pool, bytes;
};

__global__ void gl_keys(const GlGroup *__restrict__ groups, int64_t n, uint64_t *__restrict__ keys,
                        uint32_t *__restrict__ slot) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  keys[k] = groups[k].key;
  slot[k] = (uint32_t)k;
}

__global__ void gl_counts(const GlGroup *__restrict__ groups, const uint32_t *__restrict__ order, int64_t n,
                          Gl3 cnt) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const GlGroup &g = groups[order[k]];
  const int64_t na = g.n_alleles;
  cnt.a[k] = na;
  cnt.g[k] = na * (na + 1) / 2;
  cnt.p[k] = (int64_t)g.pool_bytes;
}

// Group k of the output (slot order[k]), one wave per group: its columns, its alleles (their
// bytes at the group's pool offset, in turn) and its likelihoods.
__global__ __launch_bounds__(kBlock) void gl_place(const GlGroup *__restrict__ groups, const uint32_t *__restrict__ order,
                                                   Gl3 off, const GlAllele *__restrict__ alleles,
                                                   const double *__restrict__ ll, const uint8_t *__restrict__ dpool,
                                                   int64_t n, GlLayout L, uint8_t *__restrict__ img) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; k < n; k += nw) {
    const GlGroup g = groups[order[k]];
    const struct { int64_t a, g, p; } o{off.a[k], off.g[k], off.p[k]};
    const int64_t na = g.n_alleles, G = na * (na + 1) / 2;
    if (lane == 0) {
      ((int32_t *)(img + L.contig))[k] = g.contig;
      ((int64_t *)(img + L.pos))[k] = g.pos;
      ((int32_t *)(img + L.sample))[k] = g.sample;
      ((int32_t *)(img + L.depth))[k] = g.depth;
      ((int32_t *)(img + L.n_alleles))[k] = g.n_alleles;
      ((int64_t *)(img + L.allele_first))[k] = o.a;
      ((int64_t *)(img + L.geno_first))[k] = o.g;
      img[L.flags + k] = g.flags;
      if (k == n - 1) *(int64_t *)img = o.p + g.pool_bytes;
    }
    int64_t at = o.p;
    for (int64_t a0 = 0; a0 < na; a0 += 64) {
      const int64_t a = a0 + lane;
      GlAllele r{};
      if (a < na) r = alleles[g.allele_at + a];
      const int tot = r.ref_len + r.alt_len;
      int x = tot;  // inclusive scan of the lengths
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
      }
      if (a < na) {
        const int64_t q = o.a + a, p = at + x - tot;
        ((int64_t *)(img + L.ref_off))[q] = p;
        ((int32_t *)(img + L.ref_len))[q] = r.ref_len;
        ((int64_t *)(img + L.alt_off))[q] = p + r.ref_len;
        ((int32_t *)(img + L.alt_len))[q] = r.alt_len;
        ((int32_t *)(img + L.allele_depth))[q] = r.depth;
        uint8_t *w = img + L.pool + p;
        if (tot <= 8)
          for (int i = 0; i < tot; ++i) w[i] = (uint8_t)(r.allele >> (8 * i));
        else
          for (int i = 0; i < tot; ++i) w[i] = dpool[r.allele + (uint64_t)i];
      }
      at += __shfl(x, 63, 64);
    }
    double *w = (double *)(img + L.ll) + o.g;
    for (int64_t q = lane; q < G; q += 64) w[q] = ll[g.geno_at + q];
  }
}
