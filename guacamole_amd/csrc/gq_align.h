// gq_align.h — affine-gap alignment on the device (gqpileup.h: gq_align_batch, gq_align_reads).
// Included by gq_align.hip.  The recurrence and the table are gq_align_host.h's; this file holds
// the kernels.
//
// align_k: one wave (a 64-thread workgroup) per pair.  The Deletion candidate comes from the same
// row and its cost depends on that neighbour's state, so a row cannot be scanned; the wave runs a
// wavefront instead.  Lane l owns rpl = ceil(S / 64) consecutive sequence rows in registers (FP64
// score and last state each); nl = ceil(S / rpl) lanes are used.  At step t lane l computes
// reference column r = t - l for its rows, top to bottom, and hands its bottom row's score and state
// (and the reference byte of that column) to lane l + 1 with a DPP wave shift (wave_shr:1), which
// computes the same column one step later: R + nl steps for the pair.  Lane 0 takes its reference
// bytes from a 64-byte register chunk the wave reloads every 64 steps (v_readlane by step).
// A cell is, per candidate, one LDS read of the 32-entry table, one FP64 add and one compare.
//
// Traceback: 2 bits a cell (the step taken: I D = X, which is also the path's last state).  A lane
// writes its rpl rows' bits of one column as one byte (rpl <= 4) or halfword, at [t * nl + l]: the
// lanes of a step write consecutive elements.  nl * (R + nl) elements; in LDS when they fit
// kLdsTb bytes, else in the pair's region of the call's global scratch.  Lane 0 then walks the path
// back from (S, ref_end), run-length encodes it into BAM words at the END of the pair's CIGAR
// space ((S + R) words: no path is longer) so they stand in forward order, and cigar_gather_k
// moves every pair's words to their scanned offsets.
#pragma once

namespace gq {
namespace aln {

constexpr int kLanes = 64;
constexpr int kMaxRows = 8;  // rows per lane at S = kMaxS
static_assert(gq_align::kMaxS == kLanes * kMaxRows, "S cap = lanes x rows per lane");
constexpr int kLdsTb = 16128;  // LDS bytes of a pair's traceback (with the table: 16 KiB a workgroup)

__host__ __device__ __forceinline__ int rows_per_lane(int S) { return (S + kLanes - 1) / kLanes; }
__host__ __device__ __forceinline__ int lanes_used(int S) {
  const int rpl = rows_per_lane(S);
  return rpl ? (S + rpl - 1) / rpl : 0;
}
__host__ __device__ __forceinline__ int64_t tb_bytes(int S, int R) {
  const int nl = lanes_used(S);
  return (int64_t)nl * (R + nl) * (rows_per_lane(S) <= 4 ? 1 : 2);
}
// a pair's bytes of global scratch: its traceback when LDS cannot hold it, then (S + R) CIGAR words
__host__ __device__ __forceinline__ int64_t tb_region(int S, int R) {
  const int64_t t = tb_bytes(S, R);
  return t <= kLdsTb ? 0 : (t + 15) & ~(int64_t)15;
}
__host__ __device__ __forceinline__ int64_t scratch_bytes(int S, int R) {
  return tb_region(S, R) + ((4 * ((int64_t)S + R) + 15) & ~(int64_t)15);
}

struct Pairs {  // device pointers; pair i = seq_pool[seq_off[i], + seq_len[i]) x ref_pool[ref_off[i], + ref_len[i])
  const uint8_t *seq_pool;
  const int64_t *seq_off;
  const int32_t *seq_len;
  const uint8_t *ref_pool;
  const int64_t *ref_off;
  const int32_t *ref_len;
};

struct Out {  // per pair of the launch
  int32_t *ref_start, *ref_end;
  double *score;
  int64_t *n_ops;      // CIGAR words
  int64_t *cig_begin;  // index of its first word in the scratch, as words
};

__device__ __forceinline__ int shr1(int old, int v) {  // lane l <- lane l - 1; lane 0 <- old
  return __builtin_amdgcn_update_dpp(old, v, 0x138, 0xF, 0xF, false);  // wave_shr:1
}

// Pairs [first, first + gridDim.x) of P; scr_off[j]: the byte offset of pair first + j's region in
// `scratch` (16-byte aligned, scratch_bytes long).  Every pair is within the caps (checked on the host).
__global__ void __launch_bounds__(kLanes) align_k(Pairs P, int64_t first, const double *__restrict__ table,
                                                  const int64_t *__restrict__ scr_off, uint8_t *__restrict__ scratch,
                                                  Out o) {
  __shared__ double T[32];
  __shared__ __attribute__((aligned(16))) uint8_t tbl[kLdsTb];
  const int lane = threadIdx.x;
  const int64_t j = blockIdx.x, p = first + j;
  if (lane < 32) T[lane] = table[lane];
  __syncthreads();
  const int S = P.seq_len[p], R = P.ref_len[p];
  const uint8_t *seq = P.seq_pool + P.seq_off[p], *ref = P.ref_pool + P.ref_off[p];
  uint8_t *region = scratch + scr_off[j];
  if (S <= 0) {
    if (lane == 0) {
      o.ref_start[j] = 0;
      o.ref_end[j] = 0;
      o.score[j] = 0.0;
      o.n_ops[j] = 0;
      o.cig_begin[j] = scr_off[j] >> 2;
    }
    return;
  }
  const int rpl = rows_per_lane(S), nl = lanes_used(S);
  const bool wide = rpl > 4;
  const bool in_lds = tb_bytes(S, R) <= kLdsTb;
  uint8_t *gtb = region;
  uint32_t *cig = reinterpret_cast<uint32_t *>(region + tb_region(S, R));

  const int row0 = lane * rpl;  // this lane's rows: s = row0 + 1 .. row0 + rpl
  double sc[kMaxRows];          // cell (row0 + k + 1, r - 1) before a step, (.., r) after
  int ls[kMaxRows];             // its last state (gq_align::kLast*)
  int sq[kMaxRows];
#pragma unroll
  for (int k = 0; k < kMaxRows; ++k) {
    sc[k] = 0.0;
    ls[k] = 0;
    const int s = row0 + k + 1;
    sq[k] = (k < rpl && s <= S) ? (int)seq[s - 1] : 0;
  }
  double out_sc = 0.0;  // the bottom row's cell of the column just computed, for lane + 1
  int out_x = 0;        // its last state | that column's reference byte << 8
  double dg_sc = 0.0;   // what lane - 1 handed over one step ago: cell (row0, r - 1)
  int dg_ls = 0;
  double min_sc = 0.0;  // row S (the last used lane): the first strictly smallest score
  int min_r = 0;
  const int steps = R + nl;
  for (int t0 = 0; t0 < steps; t0 += 64) {
    const int ci = t0 - 1 + lane;  // lane 0's column r = t needs ref[t - 1]
    const int chunk = (ci >= 0 && ci < R) ? (int)ref[ci] : 0;
    const int jn = steps - t0 < 64 ? steps - t0 : 64;
    for (int jj = 0; jj < jn; ++jj) {
      const int t = t0 + jj;
      const int b0 = __builtin_amdgcn_readlane(chunk, jj);
      const int in_x = shr1(b0 << 8, out_x);  // lane 0: row 0 has no state
      const double in_sc = __hiloint2double(shr1(0, __double2hiint(out_sc)), shr1(0, __double2loint(out_sc)));
      const int r = t - lane;
      if (lane < nl && r >= 0 && r <= R) {
        const int refb = in_x >> 8;
        double up_sc = in_sc, d_sc = dg_sc;
        int up_ls = in_x & 3, d_ls = dg_ls;
        uint32_t bits = 0;
#pragma unroll
        for (int k = 0; k < kMaxRows; ++k) {
          if (k < rpl) {
            const int s = row0 + k + 1;
            const int e = s == S ? 16 : 0;
            double best = up_sc + T[e + 4 * up_ls + gq_align::kIns];
            int nx = gq_align::kIns;
            if (r > 0) {
              const double dd = sc[k] + T[e + 4 * ls[k] + gq_align::kDel];
              if (dd < best) best = dd, nx = gq_align::kDel;
              const int m = sq[k] == refb ? gq_align::kMatch : gq_align::kMismatch;
              const double g = d_sc + T[e + 4 * d_ls + m];
              if (g < best) best = g, nx = m;
            }
            d_sc = sc[k];
            d_ls = ls[k];
            sc[k] = best;
            ls[k] = nx < gq_align::kMatch ? nx + 1 : gq_align::kLastDiag;
            up_sc = best;
            up_ls = ls[k];
            bits |= (uint32_t)nx << (2 * k);
            if (s == S && (r == 0 || best < min_sc)) min_sc = best, min_r = r;
          }
        }
        out_sc = up_sc;
        out_x = up_ls | (refb << 8);
        const int at = t * nl + lane;  // < (R + nl) * nl
        if (in_lds) {
          if (wide) reinterpret_cast<uint16_t *>(tbl)[at] = (uint16_t)bits;
          else tbl[at] = (uint8_t)bits;
        } else {
          if (wide) reinterpret_cast<uint16_t *>(gtb)[at] = (uint16_t)bits;
          else gtb[at] = (uint8_t)bits;
        }
      }
      dg_sc = in_sc;
      dg_ls = in_x & 3;
    }
  }
  if (!in_lds) __threadfence();  // lane 0 reads what the other lanes stored
  __syncthreads();
  const int end = __builtin_amdgcn_readlane(min_r, nl - 1);
  const double score = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(min_sc), nl - 1),
                                        __builtin_amdgcn_readlane(__double2loint(min_sc), nl - 1));
  if (lane == 0) {
    const int cap = S + R;
    int s = S, r = end, pos = cap, run = 0, op = -1;
    int l = nl - 1, k = S - 1 - l * rpl;  // row s = l * rpl + k + 1
    while (s > 0 && pos > 0) {  // (pos > 0 always holds: a path has at most S + R steps)
      const int at = (r + l) * nl + l;
      uint32_t bits;
      if (in_lds) bits = wide ? (uint32_t) reinterpret_cast<const uint16_t *>(tbl)[at] : (uint32_t)tbl[at];
      else bits = wide ? (uint32_t) reinterpret_cast<const uint16_t *>(gtb)[at] : (uint32_t)gtb[at];
      const int nx = (int)(bits >> (2 * k)) & 3;
      if (nx != op) {
        if (run) cig[--pos] = (uint32_t)run << 4 | (op == 0 ? 1u : op == 1 ? 2u : op == 2 ? 7u : 8u);
        op = nx;
        run = 0;
      }
      ++run;
      if (nx != gq_align::kDel) {
        --s;
        if (--k < 0) k = rpl - 1, --l;
      }
      if (nx != gq_align::kIns && r > 0) --r;  // (r > 0 always holds there: column 0 has only insertions)
    }
    if (run) cig[--pos] = (uint32_t)run << 4 | (op == 0 ? 1u : op == 1 ? 2u : op == 2 ? 7u : 8u);
    o.ref_start[j] = r;
    o.ref_end[j] = end;
    o.score[j] = score;
    o.n_ops[j] = cap - pos;
    o.cig_begin[j] = ((scr_off[j] + tb_region(S, R)) >> 2) + pos;
  }
}

// pair j's CIGAR words from its scratch region to dst[off[j], off[j + 1]); a wave per pair
__global__ void __launch_bounds__(256) cigar_gather_k(int64_t n, const int64_t *__restrict__ n_ops,
                                                      const int64_t *__restrict__ cig_begin,
                                                      const int64_t *__restrict__ off,
                                                      const uint32_t *__restrict__ scratch, uint32_t *__restrict__ dst) {
  const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (j >= n) return;
  const int64_t m = n_ops[j], b = cig_begin[j], a = off[j];
  for (int64_t i = lane; i < m; i += 64) dst[a + i] = scratch[b + i];
}

// ---- gq_align_reads: selection of resident reads and their reference windows ----
struct RefView {
  const uint8_t *bytes;
  const int64_t *off, *len;  // per contig (off -1: absent)
};

__device__ __forceinline__ int read_contig(const DevReads &R, int64_t r) {  // the last contig whose reads begin at or before r
  int lo = 0, hi = R.n_contigs - 1;
  while (lo < hi) {
    const int m = (lo + hi + 1) >> 1;
    if (R.contig_read_begin[m] <= r) lo = m;
    else hi = m - 1;
  }
  return lo;
}

// A lane per read: flag[r] = 1 if selected, with its window [lo[r], hi[r]).  ctr[0] += reads with an N
// or P op; ctr[1] = min over selected reads on a contig the reference lacks (preset to ~0).
__global__ void __launch_bounds__(256) align_select_k(DevReads R, RefView ref, int32_t pad, int32_t all,
                                                      int64_t *__restrict__ flag, int32_t *__restrict__ lo,
                                                      int32_t *__restrict__ hi, unsigned long long *ctr) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > R.n_reads) return;
  if (r == R.n_reads) {  // the scan's total lands here
    flag[r] = 0;
    return;
  }
  const int64_t co = R.cigar_off[r];
  const int32_t nc = R.n_cigar[r];
  bool ids = false, np = false;
  for (int32_t k = 0; k < nc; ++k) {
    const uint32_t op = R.cigar[co + k] & 15;
    ids = ids || op == OP_I || op == OP_D || op == OP_S;
    np = np || op == OP_N || op == OP_P;
  }
  int64_t lead = 0, trail = 0;
  int32_t a = 0, b = nc - 1;
  for (; a < nc; ++a) {
    const uint32_t v = R.cigar[co + a], op = v & 15;
    if (op == OP_S) lead += v >> 4;
    else if (op != OP_H) break;
  }
  for (; b >= a; --b) {
    const uint32_t v = R.cigar[co + b], op = v & 15;
    if (op == OP_S) trail += v >> 4;
    else if (op != OP_H) break;
  }
  bool sel = !np && (all || ids);
  if (np) atomicAdd(ctr, 1ull);
  int32_t wl = 0, wh = 0;
  if (sel) {
    const int c = read_contig(R, r);
    const int64_t L = ref.off[c] < 0 ? -1 : ref.len[c];
    if (L < 0) {
      atomicMin(ctr + 1, (unsigned long long)r);
      sel = false;
    } else {
      int64_t x = (int64_t)R.start[r] - lead - pad, y = (int64_t)R.end[r] + trail + pad;
      x = x < 0 ? 0 : x;
      y = y > L ? L : y;
      x = x > L ? L : x;
      y = y < x ? x : y;
      wl = (int32_t)x;
      wh = (int32_t)y;
    }
  }
  flag[r] = sel ? 1 : 0;
  lo[r] = wl;
  hi[r] = wh;
}

// the selected reads in resident order: pair at[r] = read r
__global__ void __launch_bounds__(256) align_compact_k(DevReads R, RefView ref, const int64_t *__restrict__ flag,
                                                       const int64_t *__restrict__ at, const int32_t *__restrict__ lo,
                                                       const int32_t *__restrict__ hi, int64_t *__restrict__ idx,
                                                       int32_t *__restrict__ sel_lo, int64_t *__restrict__ seq_off,
                                                       int32_t *__restrict__ seq_len, int64_t *__restrict__ ref_off,
                                                       int32_t *__restrict__ ref_len) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R.n_reads || !flag[r]) return;
  const int64_t k = at[r];
  const int c = read_contig(R, r);
  idx[k] = r;
  sel_lo[k] = lo[r];
  seq_off[k] = R.seq_off[r];
  seq_len[k] = R.seq_len[r];
  ref_off[k] = ref.off[c] + lo[r];
  ref_len[k] = hi[r] - lo[r];
}

}  // namespace aln
}  // namespace gq
