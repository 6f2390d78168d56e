// gq_haplik.h — haplotype likelihoods on the device (gqpileup.h: gq_haplik_batch, gq_haplik_windows).
// Included by gq_haplik.hip.  The model, the tables and a pair's / a genotype's last steps are
// gq_haplik_host.h's; this file holds the kernels.
//
// hap_forward_k: one wave per (read, haplotype) pair, kWaves pairs a workgroup.  The cell (s, r)
// needs (s-1, r-1), (s-1, r) and (s, r-1), as the aligner's does, so the wave runs gq_align.h's
// wavefront: lane l owns rpl = ceil(S / 64) consecutive read rows (at most 8) with their M I D and
// their two emission values (match / mismatch prior of the row's quality) in registers; nl =
// ceil(S / rpl) lanes are used.  At step t lane l computes haplotype column r = t - l for its rows,
// top to bottom, and hands its bottom row's M I D and the column's haplotype byte to lane l + 1 with
// a DPP wave shift (wave_shr:1), which computes the same column one step later: R + nl steps a
// pair.  Lane 0 takes its haplotype bytes from a 64-byte register chunk the wave reloads every 64
// steps, and row 0 (M = I = 0, D = INIT / R) as the value the shift leaves in the first lane.  The
// lane that holds row S adds M + I of every column r >= 1 to the sum as it computes them, i.e. in
// column order, and writes the pair's result.  Nothing is kept per cell: no traceback, no scratch.
// The transition table and the two 256-entry emission tables are staged in LDS once a workgroup and
// read from there into registers before the loop; no table is read inside it.
//
// hap_pairs_k makes the pair list of gq_haplik_windows from the device window-read lists,
// hap_genotype_k computes a window's genotypes (a thread each) and hap_best_k picks the best.
#pragma once

namespace gq {
namespace hlk {

constexpr int kLanes = 64;
constexpr int kMaxRows = 8;  // rows per lane at S = kMaxS
constexpr int kWaves = 4;    // pairs per workgroup
static_assert(gq_haplik::kMaxS == kLanes * kMaxRows, "S cap = lanes x rows per lane");

__host__ __device__ __forceinline__ int rows_per_lane(int S) { return (S + kLanes - 1) / kLanes; }
__host__ __device__ __forceinline__ int lanes_used(int S) {
  const int rpl = rows_per_lane(S);
  return rpl ? (S + rpl - 1) / rpl : 0;
}

struct Pairs {  // device pointers; pair p = seq_pool[seq_off[p], + seq_len[p]) x hap_pool[hap_off[p], + hap_len[p])
  const uint8_t *seq_pool;
  const uint8_t *qual_pool;  // same offsets as seq_pool; null: no qualities
  const int64_t *seq_off;
  const int32_t *seq_len;
  const uint8_t *hap_pool;
  const int64_t *hap_off;
  const int32_t *hap_len;
};

__device__ __forceinline__ int shr1(int old, int v) {  // lane l <- lane l - 1; lane 0 <- old
  return __builtin_amdgcn_update_dpp(old, v, 0x138, 0xF, 0xF, false);  // wave_shr:1
}
__device__ __forceinline__ double shr1d(double old, double v) {
  return __hiloint2double(shr1(__double2hiint(old), __double2hiint(v)), shr1(__double2loint(old), __double2loint(v)));
}

// Pairs [0, n) of P, every one within the caps (checked before the launch).  tab: gq_haplik::flat_tables.
__global__ void __launch_bounds__(kLanes *kWaves) hap_forward_k(Pairs P, int64_t n, const double *__restrict__ tab,
                                                                double *__restrict__ scaled,
                                                                double *__restrict__ log_likelihood,
                                                                uint8_t *__restrict__ flags) {
  GQ_NO_CONTRACT
  __shared__ double T[gq_haplik::kTableDoubles];
  for (int i = threadIdx.x; i < gq_haplik::kTableDoubles; i += kLanes * kWaves) T[i] = tab[i];
  __syncthreads();  // the only barrier: a wave may leave after it
  const int lane = threadIdx.x & (kLanes - 1);
  const int64_t p = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (p >= n) return;
  const int S = P.seq_len[p], R = P.hap_len[p];
  if (S <= 0 || R <= 0) {
    if (lane == 0) gq_haplik::finish_empty(scaled + p, log_likelihood + p, flags + p);
    return;
  }
  const uint8_t *seq = P.seq_pool + P.seq_off[p], *hap = P.hap_pool + P.hap_off[p];
  const uint8_t *qual = P.qual_pool ? P.qual_pool + P.seq_off[p] : nullptr;
  const double tMM = T[gq_haplik::kTMM], tMI = T[gq_haplik::kTMI], tMD = T[gq_haplik::kTMD], tII = T[gq_haplik::kTII],
               tDD = T[gq_haplik::kTDD], tIM = T[gq_haplik::kTIM], tDM = T[gq_haplik::kTDM];
  const int rpl = rows_per_lane(S), nl = lanes_used(S);
  const int row0 = lane * rpl;  // this lane's rows: s = row0 + 1 .. row0 + rpl
  double M[kMaxRows], I[kMaxRows], D[kMaxRows];  // cell (row0 + k + 1, r - 1) before a step, (.., r) after
  double em[kMaxRows], ex[kMaxRows];             // the row's prior on a match / on a mismatch
  int sq[kMaxRows];
#pragma unroll
  for (int k = 0; k < kMaxRows; ++k) {
    M[k] = 0.0;
    I[k] = 0.0;
    D[k] = 0.0;
    const int s = row0 + k + 1;
    const bool in = k < rpl && s <= S;
    sq[k] = in ? (int)seq[s - 1] : 0;
    if (in && qual) {
      const int q = qual[s - 1];
      em[k] = T[gq_haplik::kMatchAt + q];
      ex[k] = T[gq_haplik::kMismatchAt + q];
    } else {
      em[k] = in ? T[gq_haplik::kNoQualAt] : 0.0;
      ex[k] = in ? T[gq_haplik::kNoQualAt + 1] : 0.0;
    }
  }
  const double d0 = gq_haplik::init_value() / (double)R;  // row 0's D
  double out_M = 0.0, out_I = 0.0, out_D = 0.0;  // the bottom row's cell of the column just computed, for lane + 1
  int out_b = 0;                                 // that column's haplotype byte
  double dg_M = 0.0, dg_I = 0.0, dg_D = d0;      // what lane - 1 handed over one step ago: cell (row0, r - 1)
  double sum = 0.0;                              // the lane of row S
  const int steps = R + nl;
  for (int t0 = 0; t0 < steps; t0 += 64) {
    const int ci = t0 - 1 + lane;  // lane 0's column r = t needs hap[t - 1]
    const int chunk = (ci >= 0 && ci < R) ? (int)hap[ci] : 0;
    const int jn = steps - t0 < 64 ? steps - t0 : 64;
    for (int jj = 0; jj < jn; ++jj) {
      const int t = t0 + jj;
      const int b0 = __builtin_amdgcn_readlane(chunk, jj);
      const int in_b = shr1(b0, out_b);
      const double in_M = shr1d(0.0, out_M), in_I = shr1d(0.0, out_I), in_D = shr1d(d0, out_D);  // lane 0: row 0
      const int r = t - lane;
      if (lane < nl && r >= 0 && r <= R) {
        double uM = in_M, uI = in_I;               // (s - 1, r)
        double dM = dg_M, dI = dg_I, dD = dg_D;    // (s - 1, r - 1)
        double bD = 0.0;
#pragma unroll
        for (int k = 0; k < kMaxRows; ++k) {
          if (k < rpl) {
            const double lM = M[k], lI = I[k], lD = D[k];  // (s, r - 1)
            const double nI = uM * tMI + uI * tII;
            double nM = 0.0, nD = 0.0;
            if (r > 0) {
              const double prior = sq[k] == in_b ? em[k] : ex[k];
              nM = prior * ((dM * tMM + dI * tIM) + dD * tDM);
              nD = lM * tMD + lD * tDD;
            }
            dM = lM;
            dI = lI;
            dD = lD;
            M[k] = nM;
            I[k] = nI;
            D[k] = nD;
            uM = nM;
            uI = nI;
            bD = nD;
            if (row0 + k + 1 == S && r > 0) sum = sum + (nM + nI);
          }
        }
        out_M = uM;
        out_I = uI;
        out_D = bD;
        out_b = in_b;
      }
      dg_M = in_M;
      dg_I = in_I;
      dg_D = in_D;
    }
  }
  if (lane == nl - 1) gq_haplik::finish(sum, scaled + p, log_likelihood + p, flags + p);
}

// ---- gq_haplik_windows: offsets, the pair list, the genotypes ----

// win_read_off[w] = the first entry of window w's reads in the list, w = 0 .. W
__global__ void __launch_bounds__(256) hap_winoff_k(int64_t W, const int64_t *__restrict__ cand_off,
                                                    const int64_t *__restrict__ fsum, int64_t *__restrict__ win_read_off) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w <= W) win_read_off[w] = fsum[cand_off[w]];
}

// the last w in [0, W) with off[w] <= x (off ascending, x < off[W]): the range that holds x
__device__ __forceinline__ int64_t range_of(const int64_t *off, int64_t W, int64_t x) {
  int64_t lo = 0, hi = W - 1;
  while (lo < hi) {
    const int64_t m = (lo + hi + 1) >> 1;
    if (off[m] <= x) lo = m;
    else hi = m - 1;
  }
  return lo;
}

struct PairOut {
  int64_t *seq_off;
  int32_t *seq_len;
  int64_t *hap_off;
  int32_t *hap_len;
};
// A thread per pair: window w's pair lik_off[w] + n * H_w + h is read n of its list against its
// haplotype h.  bad: the smallest pair whose read is longer than max_s (preset to ~0).
__global__ void __launch_bounds__(256) hap_pairs_k(DevReads R, int64_t W, int64_t n_pairs,
                                                   const int64_t *__restrict__ lik_off,
                                                   const int64_t *__restrict__ win_read_off,
                                                   const int64_t *__restrict__ list_read,
                                                   const int64_t *__restrict__ win_hap_off,
                                                   const int64_t *__restrict__ hap_seq_off, int32_t max_s, PairOut o,
                                                   unsigned long long *bad) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const int64_t w = range_of(lik_off, W, p);
  const int64_t H = win_hap_off[w + 1] - win_hap_off[w], local = p - lik_off[w];
  const int64_t read = list_read[win_read_off[w] + local / H], h = win_hap_off[w] + local % H;
  const int32_t len = R.seq_len[read];
  o.seq_off[p] = R.seq_off[read];
  o.seq_len[p] = len;
  o.hap_off[p] = hap_seq_off[h];
  o.hap_len[p] = (int32_t)(hap_seq_off[h + 1] - hap_seq_off[h]);
  if (len > max_s) atomicMin(bad, (unsigned long long)p);
}

// a thread per (window, genotype)
__global__ void __launch_bounds__(256) hap_genotype_k(int64_t W, int64_t G, const int64_t *__restrict__ gt_off,
                                                      const int64_t *__restrict__ win_read_off,
                                                      const int64_t *__restrict__ win_hap_off,
                                                      const int64_t *__restrict__ lik_off,
                                                      const double *__restrict__ scaled, double *__restrict__ gt_ll) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int64_t w = range_of(gt_off, W, g);
  const int64_t N = win_read_off[w + 1] - win_read_off[w], H = win_hap_off[w + 1] - win_hap_off[w];
  int64_t i, j;
  gq_haplik::genotype_pair(H, g - gt_off[w], &i, &j);
  gt_ll[g] = gq_haplik::genotype_ll(scaled + lik_off[w], N, H, i, j);
}

// a thread per window
__global__ void __launch_bounds__(256) hap_best_k(int64_t W, const int64_t *__restrict__ gt_off,
                                                  const double *__restrict__ gt_ll, int32_t *__restrict__ best) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w < W) best[w] = gq_haplik::first_largest(gt_ll + gt_off[w], gt_off[w + 1] - gt_off[w]);
}

}  // namespace hlk
}  // namespace gq
