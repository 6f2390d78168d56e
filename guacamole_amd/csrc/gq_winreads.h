// gq_winreads.h — the reads of each window of a resident read set, found on the device
// (gq_assemble.h: asm_range_k, asm_test_k, asm_compact_k).  Defined in gq_assemble.hip; shared by
// gq_asm_graphs and gq_haplik_windows, which must select the very same reads in the same order.
#pragma once
#include "gq_host.h"

namespace gq {

struct WindowReads {  // device arrays, released with the object
  DevBuf win;     // int32 contig[W], start[W], end[W]
  DevBuf cnt, coff, ra;  // per window: candidates, their exclusive sum (W + 1), first candidate read
  DevBuf flag, inst, chunks, fsum, isum, csum;  // per candidate (C + 1) and their exclusive sums
  DevBuf list_read, list_chunk;                 // the contributing reads, window after window
  DevBuf tmp;
  int64_t W = 0, C = 0;
  const int32_t *contig() const { return (const int32_t *)win.p; }
  const int32_t *start() const { return (const int32_t *)win.p + W; }
  const int32_t *end() const { return (const int32_t *)win.p + 2 * W; }
  // window w's reads: list_read[fsum[coff[w]], fsum[coff[w + 1]])
  WindowReads() = default;
  WindowReads(const WindowReads &) = delete;
  WindowReads &operator=(const WindowReads &) = delete;
  ~WindowReads() {
    for (DevBuf *b : {&win, &cnt, &coff, &ra, &flag, &inst, &chunks, &fsum, &isum, &csum, &list_read, &list_chunk, &tmp})
      b->release();
  }
};

// W > 0 windows (host arrays, already validated) on the context's stream; synchronises it once (C).
// who: the caller's name, for the message of GQ_E_CAPACITY (2^31 candidates or more).
gq_status find_window_reads(gq_ctx *c, const gq_dev_reads *d, int64_t W, const int32_t *contig, const int32_t *start,
                            const int32_t *end, int32_t k, int32_t min_mapq, const char *who, WindowReads &out);

}  // namespace gq
