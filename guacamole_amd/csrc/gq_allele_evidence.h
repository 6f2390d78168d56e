// gq_allele_evidence.h — allele-evidence (gq_allele_evidence): AlleleEvidence.apply
// (variants/AlleleEvidence.scala:58-101) for every distinct allele of every sample's pileup.
// Included by gq_somatic.hip inside its anonymous namespace, after the caller's device helpers
// (make_cover, pileup_ref, gather_sample, pile_desc, DeepSel, GsMem) and gq_locus_driver.h (the
// list kernel, the per-locus prologue, the host loop).
//
// Two kernels:
//   allele_evidence_list<T>   (gq_locus_driver.h)
//                               one workgroup per tile of T loci at a time: the LDS histogram of the
//                             reads the mapq filter keeps (the germline sink), the reference-base
//                             bits of the reads it drops in a second histogram (the pileup's
//                             reference base is the unfiltered pileup's), and per locus "the
//                             filtered pileup is not empty / holds a non-Match element"
//                             (VariantLocus.apply, commands/VAFHistogram.scala:31-37).  The loci
//                             to process are compacted into one list; no wave ever runs for the
//                             others.
//   allele_evidence_call      one wave per listed locus.  Per sample: the cover list in pileup
//                             element order, the allele table (gather_sample), then ONE pass over
//                             the cover that appends each kept element's (mapq, quality,
//                             mismatches) word to its allele's segment of an element buffer
//                             (segment offsets: exclusive scan of the table's counts; position:
//                             the allele's running count + the rank among lower lanes with the
//                             same allele, so a segment is in element order).  From the segments:
//                             Breeze's running mean (a lane per allele), the medians by rank
//                             counting, the forward depths from the pass's ballots.  The cover is
//                             walked a constant number of times whatever the number of alleles.
//                             Fast instantiation: cover lists (kCover) and element buffer (kEvCap)
//                             in LDS, 128 alleles; a locus past any of them goes to the deep
//                             instantiation (per-wave HBM scratch, 1024 alleles).
#pragma once

struct AeRec {  // one row
  uint64_t key;  // locus ordinal << 20 | sample << 12 | rank of the allele among the sample's by (ref, alt)
  int32_t contig, pos;
  uint16_t ref_len, alt_len;
  uint8_t flags, sample, pad[2];
  uint64_t allele;  // ref then alt bytes: inline when they fit 8 bytes, else a pool offset
  gq_evidence ev;
};
static_assert(sizeof(AeRec) == 96, "AeRec layout");

// k-th smallest (0-based) of field `field` (0 mapq, 1 quality (signed), 2 mismatches) of the n
// packed words at ev, by rank counting, lane-parallel over the elements (allele_evidence's scheme).
__device__ __forceinline__ int ae_kth(const uint32_t *ev, uint32_t n, int field, uint32_t k) {
  const int lane = threadIdx.x & 63;
  auto val = [&](uint32_t v) -> int {
    return field == 0 ? (int)(v & 0xFFu) : field == 1 ? (int)(int8_t)((v >> 8) & 0xFFu) : (int)(v >> 16);
  };
  int found = 0x7FFFFFFF;
  for (uint32_t e = lane; e < n; e += 64) {
    const int x = val(ev[e]);
    uint32_t lt = 0, le = 0;
    for (uint32_t f = 0; f < n; ++f) {
      const int y = val(ev[f]);
      lt += y < x;
      le += y <= x;
    }
    if (lt <= k && k < le) found = x;
  }
  for (int d = 1; d < 64; d <<= 1) found = min(found, __shfl_xor(found, d, 64));
  return found;
}

// Entry j of a per-entry register array (entry j: lane j & 63, slot j >> 6), on every lane.
template <int NS>
__device__ __forceinline__ uint32_t ae_entry_u32(const uint32_t (&a)[NS], int j) {
  uint32_t v = 0;
#pragma unroll
  for (int s = 0; s < NS; ++s)
    if (s == (j >> 6)) v = (uint32_t)__shfl((int)a[s], j & 63, 64);
  return v;
}
template <int NS>
__device__ __forceinline__ double ae_entry_f64(const double (&a)[NS], int j) {
  double v = 0.0;
#pragma unroll
  for (int s = 0; s < NS; ++s)
    if (s == (j >> 6)) v = lane_f64(a[s], j & 63);
  return v;
}

template <bool DEEP>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(DEEP ? 1 : 2))) void allele_evidence_call(
    const Tile *__restrict__ tiles, const ComplexItem *__restrict__ items, int64_t n_items, DevReads R,
    gq_allele_evidence_params prm, AeRec *__restrict__ recs, unsigned long long rec_cap, uint8_t *__restrict__ pool,
    unsigned long long pool_cap, Counters *ctr, SomWin sw, AmbItem *__restrict__ amb_out, unsigned long long amb_cap,
    const AmbItem *__restrict__ amb_in, const uint8_t *__restrict__ amb_ref, int64_t n_amb_in, DeepSel dd) {
  constexpr int NS = DEEP ? kDeepNS : kSlots;
  constexpr int FW = DEEP ? 1 : kSomWaves;
  __shared__ uint32_t ev_lds[FW][kEvCap];
  __shared__ int32_t cover_a[FW][kCover], cover_s[FW][kCover];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  const int64_t gwave = wave_id();
  const int64_t nwaves_total = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const GsMem m = locus_mem<DEEP>(dd, cover_a[DEEP ? 0 : wv], cover_s[DEEP ? 0 : wv], ev_lds[DEEP ? 0 : wv], kEvCap / 2, 0);
  const uint32_t evcap = (uint32_t)(DEEP ? 2 * m.cap : kEvCap);
  const int min_mapq = prm.min_mapq;
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
      if (P.depth_f > evcap) {
        hand_over(smp, (uint32_t)max(cs.n, ca.n));  // (the deep pass covers every sample again)
        break;
      }
      // segment of entry j in the element buffer: [seg, seg + n_f) (exclusive scan of the counts)
      uint32_t seg[NS], run[NS], nfw[NS];
      {
        uint32_t carry = 0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const uint32_t v = (s * 64 + lane) < P.nt ? P.n_f[s] : 0u;
          uint32_t x = v;
#pragma unroll
          for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64);
            if (lane >= d) x += y;
          }
          seg[s] = carry + x - v;
          carry += (uint32_t)__shfl((int)x, 63, 64);
          run[s] = nfw[s] = 0;
        }
      }
      // the one pass: each kept element's word into its allele's segment, in element order
      for (int64_t k0 = 0; k0 < cs.n; k0 += 64) {
        bool act;
        const int64_t r = cs.read(R, k0 + lane, pos, &act);
        Key128 key{0, 0};
        bool pass = false, fwd = false;
        uint32_t packed = 0;
        if (act) {
          const int mq = (int)R.mapq[r];
          const int64_t so = R.seq_off[r];  // the read's scalars issued with classify's loads
          const int32_t nmd = R.n_md[r];
          const uint32_t nmm = (uint32_t)R.n_mismatch[r];
          fwd = !(R.flags[r] & 1);
          if (min_mapq <= 0 || mq >= min_mapq) {
            AlleleDesc d;
            int errc = 0;
            if (classify(R, r, pos, refbase, d, &errc)) {  // (errors were raised by gather_sample)
              pass = true;
              key = allele_key(R, d, pos, 0);
              if (nmd < 0) raise_at(ctr, GQ_E_NO_MD, pos);
              packed = (uint32_t)mq | ((uint32_t)(uint8_t)(int8_t)elem_quality(R, d, so, mq) << 8) | (nmm << 16);
            }
          }
        }
        const unsigned long long passb = __ballot(pass), fwdb = __ballot(pass && fwd);
        unsigned long long pending = passb;
        while (pending) {
          const int leader = __ffsll((long long)pending) - 1;
          const uint64_t klo = __shfl(key.lo, leader, 64), khi = __shfl(key.hi, leader, 64);
          const bool match = pass && key.lo == klo && key.hi == khi;
          const unsigned long long mb = __ballot(match);
          pending &= ~mb;
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
          const int owner = found & 63, sl = found >> 6;
          uint32_t base = 0;
#pragma unroll
          for (int s = 0; s < NS; ++s)
            if (s == sl) base = (uint32_t)__shfl((int)(seg[s] + run[s]), owner, 64);
          const uint32_t at = base + (uint32_t)__popcll(mb & lt_mask);
          if (match && at < evcap) m.ev[at] = packed;
#pragma unroll
          for (int s = 0; s < NS; ++s)
            if (s == sl && lane == owner) {
              run[s] += (uint32_t)__popcll(mb);
              nfw[s] += (uint32_t)__popcll(mb & fwdb);
            }
        }
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      // breeze.stats.mean: the running mean in element order, a lane per allele; and the rank of
      // each allele among the sample's (filtered count > 0) by Allele order (ref, then alt)
      double mean_mq[NS], mean_bq[NS];
      uint32_t rank[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const uint32_t cnt = (s * 64 + lane) < P.nt ? P.n_f[s] : 0u;
        double mq = 0.0, bq = 0.0;
        for (uint32_t k = 0; k < cnt && seg[s] + k < evcap; ++k) {
          const uint32_t v = m.ev[seg[s] + k];
          mq += ((double)(v & 0xFFu) - mq) / (double)(k + 1);
          bq += ((double)(int8_t)((v >> 8) & 0xFFu) - bq) / (double)(k + 1);
        }
        mean_mq[s] = mq;
        mean_bq[s] = bq;
        rank[s] = 0;
      }
      for (int k = 0; k < P.nt; ++k) {
        if (ae_entry_u32<NS>(P.n_f, k) == 0) continue;
        const AlleleDesc dk = pile_desc(P, k);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const int j = s * 64 + lane;
          if (j < P.nt && j != k && P.n_f[s] > 0 && allele_cmp(R, dk, P.desc[s], pos) < 0) ++rank[s];
        }
      }
      for (int j = 0; j < P.nt; ++j) {
        const uint32_t cnt = ae_entry_u32<NS>(P.n_f, j);
        if (cnt == 0) continue;  // the allele's elements were all filtered: no row
        const uint32_t off = ae_entry_u32<NS>(seg, j);
        const uint32_t *e = m.ev + off;
        gq_evidence ev;
        ev.likelihood = 0.0;
        ev.read_depth = (int32_t)P.depth_f;
        ev.forward_depth = (int32_t)P.fwd_f;
        ev.allele_read_depth = (int32_t)cnt;
        ev.allele_forward_depth = (int32_t)ae_entry_u32<NS>(nfw, j);
        ev.mean_mq = ae_entry_f64<NS>(mean_mq, j);
        ev.mean_bq = ae_entry_f64<NS>(mean_bq, j);
        if (cnt & 1) {
          ev.median_mq = (double)ae_kth(e, cnt, 0, (cnt - 1) / 2);
          ev.median_bq = (double)ae_kth(e, cnt, 1, (cnt - 1) / 2);
          ev.median_mismatches = (double)ae_kth(e, cnt, 2, (cnt - 1) / 2);
        } else {
          ev.median_mq = ((double)ae_kth(e, cnt, 0, cnt / 2 - 1) + (double)ae_kth(e, cnt, 0, cnt / 2)) / 2.0;
          ev.median_bq = ((double)ae_kth(e, cnt, 1, cnt / 2 - 1) + (double)ae_kth(e, cnt, 1, cnt / 2)) / 2.0;
          ev.median_mismatches = (double)((ae_kth(e, cnt, 2, cnt / 2 - 1) + ae_kth(e, cnt, 2, cnt / 2)) / 2);  // Int median
        }
        const AlleleDesc al = pile_desc(P, j);
        const int rl = allele_ref_len(al), alt_l = allele_alt_len(al);
        AeRec rr;
        rr.key = ((uint64_t)(tt.ordinal0 + (pos - tt.L0)) << 20) | ((uint64_t)smp << 12) |
                 (uint64_t)ae_entry_u32<NS>(rank, j);
        rr.contig = tt.contig;
        rr.pos = pos;
        rr.ref_len = (uint16_t)rl;
        rr.alt_len = (uint16_t)alt_l;
        rr.flags = amb_in ? 1 : 0;
        rr.sample = (uint8_t)smp;
        rr.pad[0] = rr.pad[1] = 0;
        rr.ev = ev;
        if (rl + alt_l <= 8) {
          uint64_t v = 0;
          int q = 0;
          for (int i = 0; i < rl; ++i) v |= (uint64_t)allele_byte(R, al, pos, 0, i) << (8 * q++);
          for (int i = 0; i < alt_l; ++i) v |= (uint64_t)allele_byte(R, al, pos, 1, i) << (8 * q++);
          rr.allele = v;
        } else {
          unsigned long long o = 0;
          if (lane == 0) o = atomicAdd(&ctr->pool_used, (unsigned long long)(rl + alt_l));
          o = __shfl(o, 0, 64);
          if (o + rl + alt_l <= pool_cap)
            for (int i = lane; i < rl + alt_l; i += 64)
              pool[o + i] = i < rl ? allele_byte(R, al, pos, 0, i) : allele_byte(R, al, pos, 1, i - rl);
          rr.allele = o;
        }
        if (lane == 0) {
          const unsigned long long k = atomicAdd(&ctr->n_rec, 1ull);
          if (k < rec_cap) recs[k] = rr;
        }
      }
      __builtin_amdgcn_wave_barrier();  // the next sample's cover reorder reuses the element buffer
    }
  }
}
