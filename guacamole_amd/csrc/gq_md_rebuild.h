// gq_md_rebuild.h — MD events rebuilt on the device from a resident reference
// (gq_reads_rebuild_md).  Included by gq_pileup.hip, which owns gq_dev_reads' arrays and the
// re-derivation (gq_reads_rederive).
//
// The rule is ReferenceGenome.buildMdTag (reference/ReferenceGenome.scala:41-47) followed by
// Read.fromSAMRecord's choice (reads/Read.scala:223-247), as reference.md_from_reference states
// it; only the events the MD string would parse into are produced, never the string:
//   M = X   a position whose read byte differs from the reference byte: an event
//           (reference offset from the read's start) << 8 | reference byte, and a mismatch
//   D       every deleted position: an event, no mismatch
//   I S     advance the read cursor;  H P: nothing;  N: an error
// The event's byte is the reference byte in upper case, as the MD parser reads it (MdTag.apply
// upper-cases the string): the uploaded reference is already unmasked, so this only matters for
// a reference handed over raw.
//
// Kernels (16 lanes per read, as rec_fill; reads' CIGARs differ too much for a lane per read):
//   md_rebuild_count   per read: events, mismatches (saturating at 65535), and the first error
//                      in resident order (min of read << 8 | code, one atomic per wave)
//   (hipcub)           int64 exclusive scan of the event counts: the new md_off
//   md_rebuild_fill    the events at the scanned offsets; a read that keeps its tag has its old
//                      events copied across
// The group's lanes walk the CIGAR together.  In an M run lane g compares the 8-base words
// g, g + 16, ... (unaligned 8-byte loads of read and reference, a byte-difference mask from the
// XOR, a popcount); in the fill pass each round of 16 words is scanned over the group, so lane g
// writes at (events so far) + (events of lanes below it): offset order without a sort.  The
// fill pass recomputes the masks; no per-op counts are kept between the passes.
//
// Past-end loads: the reference's 'N' padding (at least 512 bytes behind every contig) covers an
// 8-byte load at a contig's last base.  A sequence pool the project allocated has kSeqPad bytes
// behind it; a wrapped pool has none (seq_cap = seq_bytes), and the last words of its last read
// are read byte by byte (load8).
#pragma once

namespace gq {
namespace mdr {

constexpr int kLanes = 16;
constexpr int kCountSpread = 64;  // words of the rebuilt-read count (md_rebuild_count)
enum : uint32_t { kNoContig = 1, kBadOp = 2, kPastEnd = 3, kBadBase = 4 };

struct RefDev {
  const uint8_t *bytes;
  const int64_t *off, *len;  // per contig: 512-aligned offset (-1: absent), length
};

// p[at, at + 8) as a little-endian word; bytes at or past `cap` read as zero
__device__ __forceinline__ uint64_t load8(const uint8_t *p, int64_t at, int64_t cap) {
  if (at + 8 <= cap) return *(const gq_u64u *)(p + at);
  uint64_t v = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (at + k < cap) v |= (uint64_t)p[at + k] << (8 * k);
  return v;
}

// 0x80 in every byte of x that is not zero (no carry crosses a byte)
__device__ __forceinline__ uint64_t nonzero_bytes(uint64_t x) {
  const uint64_t lo7 = 0x7F7F7F7F7F7F7F7Full;
  return (((x & lo7) + lo7) | x) & ~lo7;
}

__device__ __forceinline__ uint32_t upper(uint32_t b) { return (b >= 'a' && b <= 'z') ? b - 32 : b; }

template <class T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
  for (int o = kLanes / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, kLanes);
  return v;
}

// the contig of read r: the last one whose reads begin at or before r
__device__ __forceinline__ int contig_of(const DevReads &R, int64_t r) {
  int lo = 0, hi = R.n_contigs - 1;
  while (lo < hi) {
    const int m = (lo + hi + 1) >> 1;
    if (R.contig_read_begin[m] <= r) lo = m;
    else hi = m - 1;
  }
  return lo;
}

// Read r's events by lane g of its group.  FILL: written at out[0, n) in offset order.
// Returns the lane's share of (events, mismatches) in n_ev / n_mm, and the read's error code
// (the same in every lane of the group): the first failing step in CIGAR order.
template <bool FILL>
__device__ __forceinline__ uint32_t walk(const DevReads &R, const RefDev &ref, int64_t r, int g, uint32_t *out,
                                         int32_t &n_ev, int32_t &n_mm) {
  n_ev = n_mm = 0;
  const int c = contig_of(R, r);
  const int64_t roff = ref.off[c], L = ref.len[c];
  if (roff < 0) return kNoContig;
  const int64_t so = R.seq_off[r], co = R.cigar_off[r], st = R.start[r];
  const int32_t sl = R.seq_len[r], nc = R.n_cigar[r];
  const uint8_t *rb = ref.bytes + roff + st;
  int64_t rp = 0, fp = 0;
  int32_t base = 0;              // FILL: events of the ops and rounds before this one
  uint32_t fail = 0;             // the first step that fails, and the op it fails at
  int32_t fail_op = INT32_MAX;
  int32_t bad_op = INT32_MAX;    // the first op where this lane met a byte the MD could not hold
  for (int32_t k = 0; k < nc; ++k) {
    const uint32_t v = R.cigar[co + k], op = v & 15;
    const int64_t ln = v >> 4;
    if (op == 0 || op == 7 || op == 8) {
      if ((ln > 0 && st + fp + ln > L) || rp + ln > sl) {
        fail = kPastEnd, fail_op = k;
        break;
      }
      const int64_t nw = (ln + 7) >> 3;
      for (int64_t w0 = 0; w0 < nw; w0 += kLanes) {
        const int64_t w = w0 + g;
        uint64_t m = 0, fw = 0;
        if (w < nw) {
          const uint64_t a = load8(R.seq, so + rp + 8 * w, R.seq_cap);
          fw = *(const gq_u64u *)(rb + fp + 8 * w);
          m = nonzero_bytes(a ^ fw);
          const int64_t nb = ln - 8 * w;
          if (nb < 8) m &= (1ull << (8 * nb)) - 1;
        }
        const int32_t cnt = __popcll(m);
        uint32_t *dst = nullptr;
        if (FILL) {
          int32_t inc = cnt;  // inclusive scan over the group
#pragma unroll
          for (int o = 1; o < kLanes; o <<= 1) {
            const int32_t x = __shfl_up(inc, o, kLanes);
            if (g >= o) inc += x;
          }
          dst = out + base + inc - cnt;
          base += __shfl(inc, kLanes - 1, kLanes);
        }
        while (m) {
          const int j = __builtin_ctzll(m) >> 3;
          const uint32_t b = upper((uint32_t)(fw >> (8 * j)) & 0xFF);
          if (b < 'A' || b > 'Z') bad_op = min(bad_op, k);
          if (FILL) *dst++ = ((uint32_t)(fp + 8 * w + j) << 8) | b;
          m &= m - 1;
        }
        n_ev += cnt;
        n_mm += cnt;
      }
      rp += ln;
      fp += ln;
    } else if (op == 2) {
      if (ln > 0 && st + fp + ln > L) {
        fail = kPastEnd, fail_op = k;
        break;
      }
      for (int64_t j = g; j < ln; j += kLanes) {
        const uint32_t b = upper(rb[fp + j]);
        if (b < 'A' || b > 'Z') bad_op = min(bad_op, k);
        if (FILL) out[base + j] = ((uint32_t)(fp + j) << 8) | b;
        ++n_ev;
      }
      if (FILL) base += (int32_t)ln;
      fp += ln;
    } else if (op == 3) {
      fail = kBadOp, fail_op = k;
      break;
    } else if (op == 1 || op == 4) {
      rp += ln;
    }
  }
#pragma unroll
  for (int o = kLanes / 2; o >= 1; o >>= 1) bad_op = min(bad_op, __shfl_xor(bad_op, o, kLanes));
  if (bad_op < fail_op) return kBadBase;
  return fail;
}

// err[0]: min over failing reads of (read << 8 | code), preset to ~0; err[1 + k], k < kCountSpread:
// reads rebuilt, spread over the workgroups' low index bits and summed on the host (one word
// would serialise a wave's add per four reads; with recompute_all every read is rebuilt and
// nothing is counted)
__global__ void __launch_bounds__(256) md_rebuild_count(DevReads R, RefDev ref, int recompute_all,
                                                        int64_t *__restrict__ ev_cnt, int32_t *__restrict__ n_md,
                                                        uint16_t *__restrict__ n_mm, unsigned long long *err) {
  const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const int g = threadIdx.x & (kLanes - 1);
  unsigned long long key = ~0ull;
  int rebuilt = 0;
  if (r < R.n_reads) {
    const int32_t old = R.n_md[r];
    if (!recompute_all && old >= 0) {
      if (g == 0) {
        ev_cnt[r] = old;
        n_md[r] = old;
        n_mm[r] = R.n_mismatch[r];
      }
    } else {
      int32_t ev, mm;
      const uint32_t code = walk<false>(R, ref, r, g, nullptr, ev, mm);
      ev = group_sum(ev);
      mm = group_sum(mm);
      if (g == 0) {
        ev_cnt[r] = code ? 0 : ev;
        n_md[r] = code ? 0 : ev;
        n_mm[r] = (uint16_t)min(mm, 65535);
        if (code) key = ((unsigned long long)r << 8) | code;
        rebuilt = 1;
      }
    }
  }
  // one atomic per wave for the error, one for the count (lanes hold increasing r)
  int nr = rebuilt;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long x = __shfl_xor(key, o, 64);
    key = x < key ? x : key;
    nr += __shfl_xor(nr, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (key != ~0ull) atomicMin(err, key);
    if (nr && !recompute_all) atomicAdd(err + 1 + (blockIdx.x & (kCountSpread - 1)), (unsigned long long)nr);
  }
}

__global__ void __launch_bounds__(256) md_rebuild_fill(DevReads R, RefDev ref, int recompute_all,
                                                       const int64_t *__restrict__ new_off,
                                                       uint32_t *__restrict__ new_ev) {
  const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const int g = threadIdx.x & (kLanes - 1);
  if (r >= R.n_reads) return;
  uint32_t *out = new_ev + new_off[r];
  const int32_t old = R.n_md[r];
  if (!recompute_all && old >= 0) {
    const uint32_t *src = R.md_ev + R.md_off[r];
    for (int32_t j = g; j < old; j += kLanes) out[j] = src[j];
    return;
  }
  int32_t ev, mm;
  (void)walk<true>(R, ref, r, g, out, ev, mm);
}

// out[blockIdx.x & (kCountSpread - 1)] += reads of this workgroup without MD events (n_md < 0)
__global__ void __launch_bounds__(256) md_missing_count(const int32_t *__restrict__ n_md, int64_t n,
                                                        unsigned long long *out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int miss = (r < n && n_md[r] < 0) ? 1 : 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) miss += __shfl_xor(miss, o, 64);
  if ((threadIdx.x & 63) == 0 && miss) atomicAdd(out + (blockIdx.x & (kCountSpread - 1)), (unsigned long long)miss);
}

}  // namespace mdr
}  // namespace gq
