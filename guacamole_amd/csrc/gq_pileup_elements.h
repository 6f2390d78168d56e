// gq_pileup_elements.h — pileup-elements (gq_pileup_elements_call): the Pileup itself
// (pileup/Pileup.scala:49-132, pileup/PileupElement.scala) at the listed loci: every element the
// mapq filter keeps, in Pileup.elements order (gq_winorder.h), with its read, alignment kind,
// allele, quality score and CIGAR cursor, and the locus' distinct alleles in Allele order.
// Included by gq_somatic.hip inside its anonymous namespace, after gq_locus_driver.h (the locus
// list, the per-locus prologue, the host loop) and gq_allele_evidence.h (whose ae_entry_u32 reads a
// table column).
//
// The output is variable-length per locus (elements, alleles, allele bytes), so it is made in two
// passes with the sizes scanned in between, all on the device:
//   pileup_elements_size   one wave per listed locus: the cover list in pileup element order, the
//                          reference base (heap-order loci through the AmbItem round trip, as
//                          allele-evidence), variants_only where the list kernel could not decide,
//                          the allele table over every sample (gather_sample), and from it one
//                          PeRec: kept elements, distinct kept alleles, their ref + alt bytes.  The
//                          three totals are added up beside the record counter, so the host sizes
//                          the result block from the counters it reads anyway.
//   (hipcub)               the records by call-order ordinal, pe_counts, three exclusive scans.
//   pileup_elements_fill   one wave per group in output order: cover list and allele table again,
//                          each kept allele's rank and pool offset (Allele order), the allele rows
//                          and bytes at the scanned offsets, then the cover 64 slots at a time:
//                          lanes = elements, each classifies its element, resolves its allele to
//                          the table rank and stores its fields at elem_first + (kept elements of
//                          earlier chunks) + (kept lower lanes): every column's stores of a wave
//                          are contiguous and in element order.
// Fast instantiations: the cover list (kCover) and the initial group's reorder area (kPeTh reads)
// in LDS, 128 alleles; a locus past any of them is handed to the deep instantiations (per-wave HBM
// scratch sized from the deepest handed-over pileup, 1024 alleles), which mark their records so
// each fill instantiation takes its own groups.
#pragma once

constexpr int kPeTh = 512;          // reads of a window's initial group make_cover reorders in the work area
constexpr int kPeWork = 2 * kPeTh;  // words of a wave's work area

// gq_pileup_elements.elem_kind (PileupElement.alignment)
enum { PE_MATCH = 0, PE_MISMATCH = 1, PE_INSERTION = 2, PE_DELETION = 3, PE_MIDDELETION = 4, PE_CLIPPED = 5 };

struct PeRec {     // one listed locus whose filtered pileup is not empty
  uint64_t key;    // the locus' call-order ordinal
  int64_t item;    // its entry of the locus list
  uint32_t depth, n_alleles, pool_bytes;  // kept elements, their distinct alleles, those alleles' ref + alt bytes
  uint8_t refbase;
  uint8_t flags;   // bit0: reference base from heap order, bit1: the deep instantiation's
  uint8_t pad[2];
};
static_assert(sizeof(PeRec) == 32, "PeRec layout");

struct Pe3 {  // per group in output order, three columns: elements, alleles, allele bytes (counts, or scanned offsets)
  int64_t *e, *a, *p;
};

struct PeLayout {  // byte offsets inside the result image
  size_t contig, pos, ref_base, flags, depth, n_alleles, elem_first, allele_first;                  // per group
  size_t ref_off, ref_len, alt_off, alt_len, allele_depth;                                          // per allele
  size_t e_read, e_sample, e_mapq, e_strand, e_kind, e_allele, e_quality, e_rpos, e_cigar, e_within;  // per element
  size_t pool, bytes;
};

template <bool DEEP>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(DEEP ? 1 : 2))) void pileup_elements_size(
    const Tile *__restrict__ tiles, const ComplexItem *__restrict__ items, int64_t n_items, DevReads R,
    gq_pileup_elements_params prm, PeRec *__restrict__ recs, unsigned long long rec_cap, Counters *ctr, SomWin sw,
    AmbItem *__restrict__ amb_out, unsigned long long amb_cap, const AmbItem *__restrict__ amb_in,
    const uint8_t *__restrict__ amb_ref, int64_t n_amb_in, DeepSel dd) {
  constexpr int NS = DEEP ? kDeepNS : kSlots;
  constexpr int FW = DEEP ? 1 : kSomWaves;
  __shared__ uint32_t work[FW][kPeWork];
  __shared__ int32_t cover_a[FW][kCover];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t gwave = wave_id();
  const int64_t nwaves_total = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const GsMem m = locus_mem<DEEP>(dd, cover_a[DEEP ? 0 : wv], nullptr, work[DEEP ? 0 : wv], kPeTh, 0);
  const int min_mapq = prm.min_mapq;
  const int64_t n = locus_count<DEEP>(dd, amb_in, n_amb_in, n_items);
  for (int64_t si = gwave; si < n; si += nwaves_total) {
    LocusItem L = locus_item<DEEP>(si, tiles, items, sw, amb_in, dd);
    Cover ca;
    uint8_t refbase;
    // (the fill pass stores from the list: a cover that is not compact is handed over too; no
    // per-sample pass, so the entry's sample stays 0)
    if (!locus_open<DEEP>(R, L, m, sw, ctr, min_mapq, prm.variants_only, amb_out, amb_cap, amb_in, amb_ref, dd, true, ca,
                          refbase))
      continue;
    const Tile &tt = L.tt;
    const int32_t pos = L.pos;
    const int64_t it = L.it;
    auto hand_over = [&](uint32_t depth) { locus_hand_over<DEEP>(ctr, dd, L, 0, depth); };
    SamplePile<NS> P;
    gather_sample(R, ca, pos, min_mapq, refbase, ctr, P);
    if (P.overflow) {
      hand_over((uint32_t)ca.n);
      continue;
    }
    if (P.depth_f == 0) continue;  // the filtered pileup is empty
    uint32_t na = 0;
    int pb = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const bool live = (s * 64 + lane) < P.nt && P.n_f[s] > 0;
      na += (uint32_t)__popcll(__ballot(live));
      if (live) pb += allele_ref_len(P.desc[s]) + allele_alt_len(P.desc[s]);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) pb += __shfl_xor(pb, d, 64);
    if (lane == 0) {
      const unsigned long long k = atomicAdd(&ctr->n_rec, 1ull);
      atomicAdd(&ctr->n_out, (unsigned long long)P.depth_f);
      atomicAdd(&ctr->out_pool, (unsigned long long)na);
      atomicAdd(&ctr->pool_used, (unsigned long long)pb);
      if (k < rec_cap) {
        PeRec rr;
        rr.key = (uint64_t)(tt.ordinal0 + (pos - tt.L0));
        rr.item = it;
        rr.depth = P.depth_f;
        rr.n_alleles = na;
        rr.pool_bytes = (uint32_t)pb;
        rr.refbase = refbase;
        rr.flags = (uint8_t)((amb_in ? 1 : 0) | (DEEP ? 2 : 0));
        rr.pad[0] = rr.pad[1] = 0;
        recs[k] = rr;
      }
    }
    __builtin_amdgcn_wave_barrier();  // the next locus' cover reorder reuses the work area
  }
}

__global__ void pe_keys(const PeRec *__restrict__ recs, int64_t n, uint64_t *__restrict__ keys,
                        uint32_t *__restrict__ slot) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  keys[k] = recs[k].key;
  slot[k] = (uint32_t)k;
}

__global__ void pe_counts(const PeRec *__restrict__ recs, const uint32_t *__restrict__ order, int64_t n, Pe3 cnt) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const PeRec &g = recs[order[k]];
  cnt.e[k] = (int64_t)g.depth;
  cnt.a[k] = (int64_t)g.n_alleles;
  cnt.p[k] = (int64_t)g.pool_bytes;
}

// Group k of the output (record order[k]), one wave per group.  Every store is bounded by the
// group's own sizes (the size pass saw the same pileup; a disagreement is GQ_E_ASSERT).
template <bool DEEP>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(DEEP ? 1 : 2))) void pileup_elements_fill(
    const Tile *__restrict__ tiles, const ComplexItem *__restrict__ items, DevReads R, int min_mapq,
    const PeRec *__restrict__ recs, const uint32_t *__restrict__ order, int64_t n, Pe3 off, PeLayout L,
    uint8_t *__restrict__ img, Counters *ctr, SomWin sw, DeepSel dd) {
  constexpr int NS = DEEP ? kDeepNS : kSlots;
  constexpr int FW = DEEP ? 1 : kSomWaves;
  __shared__ uint32_t work[FW][kPeWork];
  __shared__ int32_t cover_a[FW][kCover];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  const int64_t gwave = wave_id();
  const int64_t nwaves_total = ((int64_t)gridDim.x * blockDim.x) >> 6;
  GsMem m;
  if constexpr (DEEP) {
    m = gs_deep_mem(dd.scratch + (size_t)gwave * gs_wave_bytes(dd.scap, dd.maxG), dd.scap, dd.maxG);
  } else {
    m = GsMem{cover_a[wv], nullptr, work[wv], nullptr, nullptr, nullptr, kCover, kPeTh, 0};
  }
  for (int64_t k = gwave; k < n; k += nwaves_total) {
    const PeRec rec = recs[order[k]];
    if ((((rec.flags >> 1) & 1) != 0) != DEEP) continue;  // the other instantiation's group
    const ComplexItem item = items[rec.item];
    const Tile tt = tiles[item.tile];
    const int32_t pos = item.pos;
    const int32_t win = sw.range_win[tt.range];
    const int64_t e0 = off.e[k], a0 = off.a[k], p0 = off.p[k];
    if (lane == 0) {
      ((int32_t *)(img + L.contig))[k] = tt.contig;
      ((int64_t *)(img + L.pos))[k] = pos;
      img[L.ref_base + k] = rec.refbase;
      img[L.flags + k] = rec.flags & 1;
      ((int32_t *)(img + L.depth))[k] = (int32_t)rec.depth;
      ((int32_t *)(img + L.n_alleles))[k] = (int32_t)rec.n_alleles;
      ((int64_t *)(img + L.elem_first))[k] = e0;
      ((int64_t *)(img + L.allele_first))[k] = a0;
    }
    const Cover ca = make_cover(R, tt.rb, tt.re, pos, m.cov_a, m.ev, m.cap, m.th, sw.wi[2 * win], sw.init_reads,
                                sw.init_rank, ctr);
    if (ca.deep || !ca.compact) {
      raise_at(ctr, GQ_E_ASSERT, pos);
      continue;
    }
    SamplePile<NS> P;
    gather_sample(R, ca, pos, min_mapq, rec.refbase, ctr, P);
    if (P.overflow || P.depth_f != rec.depth) {
      raise_at(ctr, GQ_E_ASSERT, pos);
      continue;
    }
    // each kept allele's rank among the kept alleles by Allele order (ref, then alt), and the
    // ref + alt bytes of the alleles before it: its row and its place in the group's pool bytes
    int rank[NS];
    uint32_t poff[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      rank[s] = 0;
      poff[s] = 0;
    }
    for (int j = 0; j < P.nt; ++j) {
      if (ae_entry_u32<NS>(P.n_f, j) == 0) continue;
      const AlleleDesc dj = pile_desc(P, j);
      const uint32_t lj = (uint32_t)(allele_ref_len(dj) + allele_alt_len(dj));
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int i = s * 64 + lane;
        if (i < P.nt && i != j && P.n_f[s] > 0 && allele_cmp(R, dj, P.desc[s], pos) < 0) {
          ++rank[s];
          poff[s] += lj;
        }
      }
    }
    // the allele rows, a lane per table entry
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if ((s * 64 + lane) >= P.nt || P.n_f[s] == 0) continue;
      const AlleleDesc al = P.desc[s];
      const int rl = allele_ref_len(al), alt_l = allele_alt_len(al);
      if ((uint32_t)rank[s] >= rec.n_alleles || poff[s] + (uint32_t)(rl + alt_l) > rec.pool_bytes) {
        raise_at(ctr, GQ_E_ASSERT, pos);
        continue;
      }
      const int64_t q = a0 + rank[s], p = p0 + (int64_t)poff[s];
      ((int64_t *)(img + L.ref_off))[q] = p;
      ((int32_t *)(img + L.ref_len))[q] = rl;
      ((int64_t *)(img + L.alt_off))[q] = p + rl;
      ((int32_t *)(img + L.alt_len))[q] = alt_l;
      ((int32_t *)(img + L.allele_depth))[q] = (int32_t)P.n_f[s];
      uint8_t *w = img + L.pool + p;
      for (int i = 0; i < rl; ++i) w[i] = allele_byte(R, al, pos, 0, i);
      for (int i = 0; i < alt_l; ++i) w[rl + i] = allele_byte(R, al, pos, 1, i);
    }
    // the elements: lanes = cover slots, 64 at a time
    uint32_t run = 0;
    for (int64_t k0 = 0; k0 < ca.n; k0 += 64) {
      bool act;
      const int64_t r = ca.read(R, k0 + lane, pos, &act);
      Key128 key{0, 0};
      bool pass = false;
      int mq = 0, q = 0, kind = 0;
      uint32_t fl = 0, smp = 0;
      int32_t cur[3] = {0, 0, 0};
      if (act) {
        mq = (int)R.mapq[r];  // the read's scalars issued with classify's loads
        const int64_t so = R.seq_off[r];
        fl = R.flags[r];
        smp = R.sample[r];
        if (min_mapq <= 0 || mq >= min_mapq) {
          AlleleDesc d;
          int errc = 0;
          if (classify(R, r, pos, rec.refbase, d, &errc, nullptr, cur)) {  // (errors were raised by gather_sample)
            pass = true;
            key = allele_key(R, d, pos, 0);
            q = elem_quality(R, d, so, mq);
            kind = d.kind == K_SNV   ? (d.base == rec.refbase ? PE_MATCH : PE_MISMATCH)
                   : d.kind == K_INS ? PE_INSERTION
                   : d.kind == K_DEL ? PE_DELETION
                   : d.kind == K_MID ? PE_MIDDELETION
                                     : PE_CLIPPED;
          }
        }
      }
      const unsigned long long passb = __ballot(pass);
      if (!passb) continue;
      // each element's allele -> its rank
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
          if (s == (found >> 6)) rr = __shfl(rank[s], found & 63, 64);
        if (match) er = rr;
      }
      const uint32_t at = run + (uint32_t)__popcll(passb & lt_mask);
      if (pass && at < rec.depth) {
        const int64_t e = e0 + at;
        ((int64_t *)(img + L.e_read))[e] = r;
        img[L.e_sample + e] = (uint8_t)smp;
        img[L.e_mapq + e] = (uint8_t)mq;
        img[L.e_strand + e] = (uint8_t)(fl & 1u);
        img[L.e_kind + e] = (uint8_t)kind;
        ((int32_t *)(img + L.e_allele))[e] = er;
        ((int16_t *)(img + L.e_quality))[e] = (int16_t)q;  // (a mapq past 127 for MidDeletion / Clipped)
        ((int32_t *)(img + L.e_rpos))[e] = cur[0];
        ((int32_t *)(img + L.e_cigar))[e] = cur[1];
        ((int32_t *)(img + L.e_within))[e] = cur[2];
      }
      run += (uint32_t)__popcll(passb);
    }
    if (run != rec.depth) raise_at(ctr, GQ_E_ASSERT, pos);
    __builtin_amdgcn_wave_barrier();  // the next group's cover reorder reuses the work area
  }
}
