// gq_active.h — active regions (gq_active_regions_call) from the staging rows of pileup-counts
// (gq_pileup_counts.h: PcRow rows with a keep word beside each, tiles in call order).  Included by
// gq_somatic.hip inside its anonymous namespace, after gq_pileup_counts.h; the predicate, the key
// and the merge rule are gq_active_host.h's, shared with the host twin.
//
//   active_mark      a lane per staging row: a kept row's evidence and the predicate; the keep word
//                    becomes 1 for an active locus and 0 otherwise.  A row whose keep word is 0 was
//                    never written (or not kept) and is not read.
//   (hipcub)         inclusive scan of the keep words; the total (one word) comes back to the host.
//   active_compact   a lane per staging row: an active row's (key, depth | e) to its scanned place.
//   (hipcub)         radix sort of the pairs by key, unless the call's ranges ascend (then the list
//                    does too; active_heads checks it).
//   active_heads     a lane per active locus: 1 where a region starts (no predecessor, or
//                    same_region says no); raises `disorder` on keys that do not ascend.
//   (hipcub)         inclusive scan of the heads; the total (one word) comes back to the host.
//   active_write     a lane per active locus: its locus columns; a head's lane also walks its run
//                    and writes the region (a segmented reduction, one lane per region).
#pragma once

__global__ __launch_bounds__(kBlock) void active_mark(const PcRow *__restrict__ rows, uint32_t *__restrict__ keep,
                                                      int64_t n_slots, gq_active_params prm) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n_slots || !keep[o]) return;
  const PcRow *r = rows + o;
  const int32_t bc[4] = {r->base_count[0], r->base_count[1], r->base_count[2], r->base_count[3]};
  const int32_t kc[3] = {r->kind_count[0], r->kind_count[1], r->kind_count[2]};
  const int32_t e = gq_active::evidence(r->ref_base, r->ref_depth, bc, kc);
  keep[o] = gq_active::is_active(prm, r->depth, e) ? 1u : 0u;
}

// val = depth << 32 | e (both >= 0)
__global__ __launch_bounds__(kBlock) void active_compact(const PcRow *__restrict__ rows, const uint32_t *__restrict__ keep,
                                                         const uint32_t *__restrict__ inc, int64_t n_slots, int64_t n_act,
                                                         uint64_t *__restrict__ key, uint64_t *__restrict__ val) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n_slots || !keep[o]) return;
  const int64_t k = (int64_t)inc[o] - 1;
  if (k < 0 || k >= n_act) return;  // (the lists were sized from the scan's total)
  const PcRow *r = rows + o;
  const int32_t bc[4] = {r->base_count[0], r->base_count[1], r->base_count[2], r->base_count[3]};
  const int32_t kc[3] = {r->kind_count[0], r->kind_count[1], r->kind_count[2]};
  const int32_t e = gq_active::evidence(r->ref_base, r->ref_depth, bc, kc);
  key[k] = gq_active::key_of(r->contig, r->pos);
  val[k] = (uint64_t)(uint32_t)r->depth << 32 | (uint64_t)(uint32_t)e;
}

__global__ __launch_bounds__(kBlock) void active_heads(const uint64_t *__restrict__ key, int64_t n_act, int32_t pad,
                                                       uint32_t *__restrict__ head, uint32_t *__restrict__ disorder) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_act) return;
  if (i == 0) {
    head[0] = 1u;
    return;
  }
  const uint64_t a = key[i - 1], b = key[i];
  if (a > b) atomicOr(disorder, 1u);  // (equal keys: a locus the call lists twice counts twice)
  head[i] = gq_active::same_region(a, b, pad) ? 0u : 1u;
}

__global__ __launch_bounds__(kBlock) void active_write(const uint64_t *__restrict__ key, const uint64_t *__restrict__ val,
                                                       const uint32_t *__restrict__ head,
                                                       const uint32_t *__restrict__ hinc, int64_t n_act, int64_t n_regions,
                                                       int32_t pad, gq_active::Layout L, uint8_t *__restrict__ img) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_act) return;
  const uint64_t k0 = key[i], v0 = val[i];
  ((int32_t *)(img + L.l_contig))[i] = gq_active::key_contig(k0);
  ((int64_t *)(img + L.l_pos))[i] = gq_active::key_pos(k0);
  ((int32_t *)(img + L.l_depth))[i] = (int32_t)(v0 >> 32);
  ((int32_t *)(img + L.l_evidence))[i] = (int32_t)(uint32_t)v0;
  if (!head[i]) return;
  const int64_t r = (int64_t)hinc[i] - 1;
  if (r < 0 || r >= n_regions) return;  // (the image was sized from the scan's total)
  int64_t sum = (int64_t)(uint32_t)v0, j = i + 1;
  while (j < n_act && !head[j]) {
    sum += (int64_t)(uint32_t)val[j];
    ++j;
  }
  ((int32_t *)(img + L.contig))[r] = gq_active::key_contig(k0);
  ((int64_t *)(img + L.start))[r] = gq_active::region_start(gq_active::key_pos(k0), pad);
  ((int64_t *)(img + L.end))[r] = gq_active::region_end(gq_active::key_pos(key[j - 1]), pad);
  ((int32_t *)(img + L.n_active))[r] = (int32_t)(j - i);
  ((int64_t *)(img + L.evidence))[r] = sum;
}
