/*
 * gqpileup.h — C-ABI drop-in boundary of the MI355X pileup engine.
 *
 * Replaces, for the two callers named by BASELINE.json's north_star, the Spark
 * operator + per-locus callback pair of the reference (paths relative to
 * /root/reference/src/main/scala/org/hammerlab/guacamole/):
 *
 *   DistributedUtil.pileupFlatMap[T](reads, lociPartitions, skipEmpty, function, reference)
 *       DistributedUtil.scala:288-306
 *   DistributedUtil.pileupFlatMapTwoRDDs[T](reads1, reads2, lociPartitions, skipEmpty, function, ref)
 *       DistributedUtil.scala:316-335
 *   GermlineThreshold.Caller.callVariantsAtLocus(pileup, thresholdPercent, emitRef, emitNoCall)
 *       commands/GermlineThresholdCaller.scala:90-179
 *   SomaticStandard.Caller.findPotentialVariantAtLocus(tumor, normal, odds, minMapq, multiAllelic, maxDepth)
 *       commands/SomaticStandardCaller.scala:162-245  (+ driver filters :124-151)
 *
 * A JVM closure cannot cross a C ABI, so operator + callback are fused into
 * fixed-function entry points (gq_germline_threshold, gq_somatic_standard) and
 * a raw per-locus histogram (gq_pileup_counts).  skipEmpty = true is the only
 * mode (both callers pass true: GermlineThresholdCaller.scala:76,
 * SomaticStandardCaller.scala:108).
 *
 * Conventions: plain pointers + sizes, no exceptions across the ABI.  Every
 * function returns a gq_status; gq_last_error() gives the thread-local message.
 * Read sets are uploaded once to HBM (gq_reads_upload) and stay resident; the
 * caller owns host buffers, the library owns device memory and result buffers
 * (released with gq_free_calls / gq_free_somatic / gq_free_counts).
 * One gq_ctx per device; calls on a context are serialized (not re-entrant);
 * contexts on different devices may run concurrently from different threads.
 */
#ifndef GQPILEUP_H
#define GQPILEUP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes mirror the reference's exception classes. */
typedef enum {
  GQ_OK = 0,
  GQ_E_ASSERT = 1,          /* assume/assert failures (AssertionError)                    */
  GQ_E_INVALID_CIGAR = 2,   /* InvalidCigarElementException  PileupElement.scala:277-285   */
  GQ_E_MD = 3,              /* CigarMDTagMismatchException   MappedRead.scala:138-139     */
  GQ_E_NO_MD = 4,           /* ReferenceWithoutMDTagException MappedRead.scala:141        */
  GQ_E_MULTI_REF = 5,       /* "Multiple reference bases found" GermlineThresholdCaller:171 */
  GQ_E_UNSORTED = 6,        /* "Regions must be sorted"       SlidingWindow.scala:55-56   */
  GQ_E_ARG = 7,             /* IllegalArgumentException (bad arguments / loci)             */
  GQ_E_HIP = 8,             /* device runtime error                                       */
  GQ_E_NOMEM = 9,
  GQ_E_CAPACITY = 10,       /* a per-locus table overflowed (distinct alleles > capacity)  */
  /* gq_bam_dev_* (BAM decoded on the device), the host loader's gqi_status classes:          */
  GQ_E_BAM_IO = 11,         /* open / stat / map failed                        (GQI_E_IO)     */
  GQ_E_BAM_FORMAT = 12,     /* not BAM, corrupt BGZF block, truncated record   (GQI_E_FORMAT) */
  GQ_E_BAM_RECORD = 13,     /* ReadLoadError: bad aux type, missing qualities  (GQI_E_RECORD) */
  GQ_E_MD_PARSE = 14,       /* MdTag parse error (ADAM MdTag.apply)            (GQI_E_MD)     */
  GQ_E_NOT_BGZF = 15,       /* a gzip stream without BGZF block sizes: use the host loader    */
  GQ_E_PLAN = 16            /* a region plan (gq_bam_dev_plan) does not hold for this file:   */
                            /* not coordinate-sorted, or a record runs past a planned segment */
                            /* (load the whole file instead)                                  */
} gq_status;

/* CIGAR ops use BAM packing: len << 4 | op, op in M I D N S H P = X -> 0..8. */

/* Read set, structure-of-arrays.  Reads are sorted by (contig, start), ties in
 * input (file) order; contig c owns reads [contig_read_begin[c], contig_read_begin[c+1]).
 * Coordinates are 0-based, contig-relative.  MD tags are pre-parsed into events:
 * md_ev[i] = (offset from read start) << 8 | base, sorted by offset, covering both
 * mismatches (on M/=/X positions) and deleted bases (on D positions).         */
typedef struct {
  int64_t n_reads;
  int32_t n_contigs;
  int32_t n_samples;
  const int64_t *contig_read_begin; /* [n_contigs + 1]                                */
  const int32_t *start;             /* [n_reads] alignment start                       */
  const int32_t *end;               /* [n_reads] start + padded reference length       */
  const int32_t *pmax_end;          /* [n_reads] prefix max of end within the contig   */
  const uint8_t *mapq;              /* [n_reads]                                       */
  const uint8_t *flags;             /* [n_reads] bit0 = reverse strand                 */
  const uint8_t *sample;            /* [n_reads] sample slot                           */
  const int64_t *seq_off;           /* [n_reads] offset into seq / qual pools          */
  const int32_t *seq_len;           /* [n_reads]                                       */
  const int64_t *cigar_off;         /* [n_reads]                                       */
  const int32_t *n_cigar;           /* [n_reads]                                       */
  const int64_t *md_off;            /* [n_reads]                                       */
  const int32_t *n_md;              /* [n_reads] MD events; -1 => read has no MD tag   */
  const uint16_t *n_mismatch;       /* [n_reads] MdTag.countOfMismatches               */
  int64_t seq_bytes;                /* pool sizes                                      */
  int64_t cigar_len;
  int64_t md_len;
  const uint8_t *seq;               /* ASCII bases                                     */
  const uint8_t *qual;              /* phred, same offsets as seq                      */
  const uint32_t *cigar;
  const uint32_t *md_ev;
  /* [n_samples] java.lang.String.hashCode of each slot's sample name (the JVM host passes
   * name.hashCode(); a read without a read group is sample "default", Pileup.scala:58), or
   * NULL.  It orders the per-sample records of a locus as Pileup.bySample's Scala Map iterates
   * (GermlineThresholdCaller.scala:100); NULL keeps slot order.                            */
  const uint32_t *sample_hash;
} gq_reads;

/* LociMap[Long] as flat ranges in partition order (task ascending, contigs
 * lexicographic, start ascending); half-open [start, end).                    */
typedef struct {
  int64_t n_ranges;
  const int32_t *contig;
  const int64_t *start;
  const int64_t *end;
  const int64_t *task;
} gq_loci;

typedef struct {
  int32_t threshold;    /* --threshold (default 8)   */
  int32_t emit_ref;     /* --emit-ref                */
  int32_t emit_no_call; /* --emit-no-call            */
} gq_germline_params;

/* GenotypeAllele codes (bdg-formats): */
enum { GQ_GT_REF = 0, GQ_GT_ALT = 1, GQ_GT_OTHERALT = 2, GQ_GT_NOCALL = 3 };
/* per-call flags (somatic calls: bit0 / bit1 = tumor / normal reference base
 * ambiguous, plus GQ_FLAG_KNIFE_EDGE) */
enum {
  GQ_FLAG_AMBIGUOUS_REF = 1, /* pileup ref base decided by JVM heap order (MD tags disagree) */
  GQ_FLAG_TIE = 2,           /* count tie among passing alleles, ordered as the reference's
                                Scala 2.10 groupBy map iterates (restated, parity unpinned) */
  GQ_FLAG_KNIFE_EDGE = 4     /* somatic: a test or filter decided within FP rounding of its
                                threshold (outcome depends on summation order)              */
};

/* Germline genotype records (Genotype.newBuilder, GermlineThresholdCaller.scala:106-117),
 * in output order (partition order, then sample, then allele rank).          */
typedef struct {
  int64_t n;
  int32_t *contig;
  int64_t *pos;
  uint8_t *sample;
  uint8_t *gt0, *gt1;
  uint8_t *flags;
  int64_t *ref_off;  int32_t *ref_len;   /* into allele_pool */
  int64_t *alt_off;  int32_t *alt_len;
  uint8_t *allele_pool;
  int64_t pool_len;
  /* run counters */
  int64_t visited_loci;   /* loci with depth > 0 (skipEmpty semantics)         */
  int64_t complex_loci;   /* loci routed through the general-allele kernel     */
  int64_t ambiguous_loci; /* loci whose ref base depends on heap order         */
  int64_t tie_loci;
  void *block_;           /* owner of the arrays above (freed by gq_free_calls) */
} gq_calls;

/* The same records left in HBM (gq_germline_threshold_device): `calls` holds DEVICE pointers
 * into one contiguous image owned by the context and valid until its next call (do not pass
 * it to gq_free_calls).  Image layout: int64 pool_len at byte 0, then the arrays of `calls`
 * in the order contig, pos, ref_off, alt_off, ref_len, alt_len, sample, gt0, gt1, flags, pool,
 * each starting on a 64-byte boundary (the first at byte 64); image_bytes covers the pool's
 * used bytes.  One buffer per rank is what the multi-GPU gather moves over xGMI.           */
typedef struct {
  gq_calls calls;
  const void *image;
  int64_t image_bytes;
} gq_calls_device;

typedef struct gq_ctx gq_ctx;
typedef struct gq_dev_reads gq_dev_reads;

/* Per-kernel device times of the last call on this context (HIP events on the
 * context's stream), in milliseconds. */
typedef struct {
  float plan_ms;
  float pileup_ms;   /* dominant kernel: per-tile LDS histogram + on-device decision */
  float complex_ms;
  float finalize_ms; /* sort / compaction of the call records                        */
  float total_ms;    /* first event to last event                                    */
  int64_t pileup_launches;
  int64_t tiles;
  float host_ms;     /* host wall time of the whole call (enqueue + waits + marshalling) */
  float marshal_ms;  /* host time spent building the output arrays                      */
  float walk_ms;     /* germline: the walker kernel over the tiles the column kernel     */
                     /* handed over (pileup_ms is then the column kernel alone)          */
  int64_t walk_tiles;
  int64_t order_loci;  /* germline: loci whose records depend on the restated Scala map order */
  int64_t deep_loci;   /* somatic: candidates the deep caller took (pileup past the fast path) */
  int64_t deep_max;    /* somatic: deepest per-sample pileup among them                     */
  float call_ms;       /* somatic: the fast exact-caller kernel alone (inside complex_ms)    */
  float deep_ms;       /* somatic: the deep caller launches (inside complex_ms)              */
  float front_ms;      /* somatic: the split caller's front kernel (covers + element records, */
                       /* inside call_ms)                                                     */
} gq_timings;

const char *gq_version(void);
const char *gq_last_error(void);

gq_status gq_open(int device, gq_ctx **out);
void gq_close(gq_ctx *ctx);
gq_status gq_get_timings(const gq_ctx *ctx, gq_timings *out);
/* Tile size (loci per workgroup) used by the pileup kernel; 0 => default. */
gq_status gq_set_tile(gq_ctx *ctx, int32_t loci_per_tile);

/* Copy a host read set into HBM (SoA kept resident until gq_reads_free).     */
gq_status gq_reads_upload(gq_ctx *ctx, const gq_reads *host, gq_dev_reads **out);
/* Wrap read arrays that are ALREADY in device memory (e.g. torch tensors);  */
/* the caller keeps them alive.                                              */
gq_status gq_reads_wrap_device(gq_ctx *ctx, const gq_reads *device_ptrs, gq_dev_reads **out);
void gq_reads_free(gq_dev_reads *r);
/* Drop every structure derived from a resident read set (the upload-time derivation, the     */
/* projection, the margin projection) and derive the upload-time part again; the projection  */
/* is derived again by the next call that reads it.  The SoA arrays stay resident and are not */
/* read from the host again; the derived buffers are reused.  A cold pass over reads already  */
/* in HBM: what one MappedRead RDD costs the reference per job, whose pileups are rebuilt by  */
/* every pileupFlatMap (DistributedUtil.scala:288-306; GermlineThresholdCaller.scala:58-88).  */
gq_status gq_reads_rederive(gq_ctx *ctx, gq_dev_reads *r);
/* Sizes of a resident read set and of what the upload derived from it (the germline         */
/* projection pool and its sparse entries): for measurement and capacity planning.             */
typedef struct gq_reads_info {
  int64_t n_reads, seq_bytes, proj_bytes, pev_count, proj_reads;  /* proj_reads: reads the projection takes */
  int64_t n_rows;    /* projection rows (64 bytes each: proj_bytes = 64 n_rows) */
  float h2d_ms;      /* gq_reads_upload: host wall time of the copies (pinned staging, PCIe) */
  float derive_ms;   /* gq_reads_upload / wrap: the upload-time derivation on the device    */
  int64_t cigar_len, md_len;  /* pool sizes (CIGAR ops, MD events) */
  int32_t n_contigs, n_samples;
  float proj_ms;     /* the projection, derived on the first call that reads it (0: not yet) */
  int32_t projected; /* 1 once it is: the proj_* / n_rows / pev_count sizes above are then set */
  float fill_ms;       /* its pool fill kernel(s) (HIP events on the context's stream) */
  float proj_dev_ms;   /* its device span, first kernel to last (HIP events) */
  float derive_dev_ms; /* the upload-time derivation's device span (HIP events) */
} gq_reads_info;
/* A re-derivation and a projection do not wait for their device spans: this call waits for   */
/* them (and reads the projection's taken-read count) the first time it is asked after them;  */
/* the next re-derivation drops figures nobody asked for.                                      */
gq_status gq_reads_get_info(const gq_dev_reads *r, gq_reads_info *out);

/* ---- BAM decoded on the device ----------------------------------------------------------
 * The host loader of gqingest.h (Read.loadReadRDDAndSequenceDictionaryFromBAM and its
 * filters, reads/Read.scala:368-451 / :411-428; Read.fromSAMRecord :217-291;
 * ReadSet.mappedReads ReadSet.scala:47-53; MappedRead.end :87; the MdTag of
 * MappedRead.apply :114-131) with every step after the file read in HBM: the BGZF blocks are
 * inflated on the device (CRC32 and ISIZE checked), record boundaries found there, each record
 * parsed and filtered, MD tags turned into events, and the kept reads laid out as a resident
 * gq_dev_reads.  The compressed file is the only host -> device copy.  Same rules, same
 * arrays as gq_bam_open / gq_bam_scan / gq_bam_fill + gq_md_count / gq_md_fill + upload.
 *   open  -> header (text, reference dictionary) on the host, inflated stream in HBM
 *   scan  -> filters, sizes, the read-group classes' first kept records (the caller maps
 *            read groups to samples, numbered by first appearance: Read.scala:233-237)
 *   reads -> the resident read set (GQ_E_UNSORTED if the kept reads are not in (contig,
 *            start) order: the host loader sorts such files)                               */
typedef struct gq_bam_dev gq_bam_dev;

gq_status gq_bam_dev_open(gq_ctx *ctx, const char *path, gq_bam_dev **out);
/* gq_bam_dev_open in two steps: map (host only: the file, its BGZF block table and the header,
 * inflated on the host; may run while the device context starts) and load (copy, inflate) on
 * a context.  gq_bam_dev_map_ex(populate = 0) maps without faulting the whole file in (for a
 * region-restricted load, which reads only its segments' pages).                            */
gq_status gq_bam_dev_map(const char *path, gq_bam_dev **out);
gq_status gq_bam_dev_map_ex(const char *path, int32_t populate, gq_bam_dev **out);
gq_status gq_bam_dev_load(gq_ctx *ctx, gq_bam_dev *mapped);

/* Region-restricted load (the multi-GPU ingest): one rank reads only the records that can
 * overlap its loci — the reads the reference ships to that rank's tasks
 * (DistributedUtil.scala:584-597; the whole-file read Read.scala:368-451 is what it replaces
 * at world size > 1).  Host only, before gq_bam_dev_load.  Loci: per contig of the BAM's
 * dictionary, sorted disjoint half-open ranges (loci_begin[n_contigs + 1] indexes
 * loci_start / loci_end, as gq_bam_dev_filters).  Each range's records are found
 *   * from the BAI linear index (`bai_path`; NULL or "" for none): the first record that can
 *     overlap the range's first locus (exact for any read length); or, without an index,
 *     by host probes of BGZF blocks (binary search over the blocks' last record keys), from
 *     `halo` loci before the range;
 *   * up to the first BGZF block whose records all start at or past the range's end (probes).
 * Ranges whose blocks meet are merged into one segment.  The next gq_bam_dev_load copies and
 * inflates only the segments' blocks; gq_bam_dev_scan walks each segment's records from its
 * first record.  GQ_E_PLAN: the header does not declare SO:coordinate, or the index does not
 * fit the file (then load the whole file).                                                  */
typedef struct {
  int64_t n_segments;
  int64_t n_blocks;        /* BGZF blocks the load will inflate                                  */
  int64_t comp_bytes;      /* their compressed bytes (the load's host -> device copy)          */
  int64_t bam_bytes;       /* their inflated bytes                                             */
  int64_t probes;          /* host probes: distinct blocks inflated on the host to read record
                            * keys (a block two plan threads reach at once counts once)         */
  int32_t used_index;      /* 1: range starts from the BAI linear index                        */
  int32_t pad;
} gq_bam_dev_plan_info;
gq_status gq_bam_dev_plan(gq_bam_dev *b, const int64_t *loci_begin, const int64_t *loci_start,
                          const int64_t *loci_end, int64_t halo, const char *bai_path,
                          gq_bam_dev_plan_info *info);
/* The planned segments (n_segments entries each): first BGZF block, offset of the first record
 * in that block's inflated bytes, end block (exclusive), and whether records run to the end of
 * the file (else block end - 1 is read only to complete the last record before it).         */
gq_status gq_bam_dev_plan_segments(const gq_bam_dev *b, int64_t *first_block, int64_t *first_offset,
                                   int64_t *end_block, int32_t *to_eof);
void gq_bam_dev_close(gq_bam_dev *b);
const char *gq_bam_dev_header_text(const gq_bam_dev *b); /* SAM text, trailing NULs stripped */
int32_t gq_bam_dev_n_contigs(const gq_bam_dev *b);
const char *gq_bam_dev_contig_name(const gq_bam_dev *b, int32_t i);
int64_t gq_bam_dev_contig_length(const gq_bam_dev *b, int32_t i);

typedef struct {
  int32_t non_duplicate;   /* Read.InputFilters, as gqingest.h gq_bam_filters                   */
  int32_t passed_vendor_quality_checks;
  int32_t is_paired;
  int32_t has_md_tag;
  int32_t use_loci;
  const int64_t *loci_begin; /* [n_contigs + 1] */
  const int64_t *loci_start;
  const int64_t *loci_end;
  int32_t n_rg;            /* the header's @RG IDs: n_rg NUL-terminated strings back to back */
  const char *rg_ids;
} gq_bam_dev_filters;

typedef struct {
  int64_t n_records;       /* alignment records in the file */
  int64_t n_reads;         /* kept                          */
  int64_t seq_bytes, cigar_len, md_events;
  int64_t comp_bytes, bam_bytes; /* compressed file / inflated stream */
  int64_t n_blocks;        /* BGZF blocks                   */
  float map_ms, h2d_ms, inflate_ms, records_ms, parse_ms;  /* open: map + block walk, copy, inflate; scan */
  int64_t max_span;        /* largest reference span (end - start) of a mapped record scanned  */
} gq_bam_dev_sizes;

/* rg_first[k] (k < n_rg): file-order index of the first kept record whose RG tag is header ID
 * k; rg_first[n_rg]: of the first kept record without an RG tag or with an ID the header
 * lacks (both are sample "default"); -1 where none.                                         */
gq_status gq_bam_dev_scan(gq_bam_dev *b, const gq_bam_dev_filters *f, int64_t *rg_first, gq_bam_dev_sizes *sizes);
/* class_sample[k] (k <= n_rg): the sample slot of read-group class k; sample_hash as in
 * gq_reads, may be NULL.  The handle is independent of b (b may be closed after).          */
gq_status gq_bam_dev_reads(gq_bam_dev *b, const uint8_t *class_sample, int32_t n_samples,
                           const uint32_t *sample_hash, gq_dev_reads **out, float *fill_ms);

/* Copies out of a resident read set (host buffers of n_reads / n_contigs + 1 entries).      */
gq_status gq_reads_positions(const gq_dev_reads *r, int32_t *start, int32_t *end);
gq_status gq_reads_contig_begin(const gq_dev_reads *r, int64_t *out);
/* The whole SoA of a resident read set copied into host buffers (dst's pointers, sized from
 * gq_reads_info; a NULL pointer is skipped): the parity tests compare it with the host loader. */
gq_status gq_reads_download(const gq_dev_reads *r, const gq_reads *dst);

/* germline-threshold over the given loci partitions.                         */
gq_status gq_germline_threshold(gq_ctx *ctx, const gq_dev_reads *reads, const gq_loci *loci,
                                const gq_germline_params *params, gq_calls **out);
void gq_free_calls(gq_calls *c);
/* The body of the VCF a germline-threshold run writes (Common.scala:290-293 saveAsVcf of the
 * records' single sample: "CHROM POS . REF ALT . . . GT <gt>" per record, POS 1-based) after
 * `header` (the ## lines and the #CHROM line), to `path`; contig_names[k] names contig id k.
 * GQ_E_ARG on an unwritable path.  The CLI's writer for one-sample output (Python builds the
 * multi-sample layout).                                                                     */
gq_status gq_write_vcf_germline(const char *path, const char *header, int64_t n, const int32_t *contig,
                                const int64_t *pos, const uint8_t *gt0, const uint8_t *gt1, const int64_t *ref_off,
                                const int32_t *ref_len, const int64_t *alt_off, const int32_t *alt_len,
                                const uint8_t *pool, int32_t n_contigs, const char *const *contig_names);
/* gq_germline_threshold with the records left in HBM (no PCIe copy; the multi-GPU driver
 * gathers the images over xGMI).  Same decisions, same record order.                      */
gq_status gq_germline_threshold_device(gq_ctx *ctx, const gq_dev_reads *reads, const gq_loci *loci,
                                       const gq_germline_params *p, gq_calls_device *out);

/* Raw per-locus pileup histogram for every locus of `loci` (dense, in range
 * order).  Categories: Match/Mismatch by sequenced base A,C,G,T,N,other; then
 * insertion, deletion, mid-deletion, clipped; positive-strand depth; the
 * MD-derived reference base (or 'N'); ambiguous-ref flag.                     */
typedef struct {
  int64_t n_loci;
  int32_t *depth;
  int32_t *pos_depth;
  int32_t *base_counts;   /* [n_loci * 6]  A C G T N other              */
  int32_t *indel_counts;  /* [n_loci * 4]  ins del middel clipped       */
  int32_t *ref_depth;     /* Match elements                             */
  uint8_t *ref_base;
  uint8_t *ambiguous;
} gq_counts;
gq_status gq_pileup_counts(gq_ctx *ctx, const gq_dev_reads *reads, const gq_loci *loci, gq_counts **out);
void gq_free_counts(gq_counts *c);

/* somatic-standard.                                                          */
typedef struct {
  int32_t odds;                 /* --odds (20)                          */
  int32_t min_mapq;             /* --min-mapq (1)                       */
  int32_t filter_multi_allelic; /* --filter-multi-allelic               */
  int32_t max_read_depth;       /* caller's maxReadDepth (= --max-tumor-read-depth) */
  int32_t min_tumor_read_depth, max_tumor_read_depth, min_normal_read_depth;
  int32_t min_tumor_alternate_read_depth;
  int32_t min_lod, min_likelihood, min_vaf;
  int32_t min_average_mapping_quality, min_average_base_quality;
  int32_t max_median_mismatches;
  int32_t apply_filters;        /* 0 => raw findPotentialVariantAtLocus output */
} gq_somatic_params;

typedef struct {
  double likelihood;
  int32_t read_depth, allele_read_depth, forward_depth, allele_forward_depth;
  double mean_mq, median_mq, mean_bq, median_bq, median_mismatches;
} gq_evidence;

/* CalledSomaticAllele (variants/CalledSomaticAllele.scala:37-51)            */
typedef struct {
  int64_t n;
  int32_t *contig;
  int64_t *pos;
  uint8_t *sample;
  int64_t *ref_off;  int32_t *ref_len;
  int64_t *alt_off;  int32_t *alt_len;
  uint8_t *allele_pool;
  int64_t pool_len;
  double *log_odds;
  int32_t *gq;               /* phredScaledSomaticLikelihood                 */
  gq_evidence *tumor;        /* tumorVariantEvidence                         */
  gq_evidence *normal;       /* normalReferenceEvidence                      */
  uint8_t *flags;
  int64_t visited_loci;
  int64_t candidate_loci;    /* loci that reached the likelihood kernel      */
  void *block_;              /* owner of the arrays above when non-NULL (freed by gq_free_somatic) */
} gq_somatic_calls;

gq_status gq_somatic_standard(gq_ctx *ctx, const gq_dev_reads *tumor, const gq_dev_reads *normal,
                              const gq_loci *loci, const gq_somatic_params *params, gq_somatic_calls **out);
void gq_free_somatic(gq_somatic_calls *c);

/* variant-support: VariantSupport.pileupToAlleleCounts (commands/VariantSupport.scala:110-118)
 * over pileupFlatMap(reads, partitions, skipEmpty = true, ...) (:93-100).  One row per
 * (visited locus, distinct allele of its pileup): every element counts (no filter).  Rows in
 * call order of the loci, a locus's alleles by (ref, alt) bytes (the reference iterates a Scala
 * HashMap there: order unpinned).  sample = the pileup's head-element read sample
 * (Pileup.scala:51); flags bit0 = reference base from heap order (MD tags disagree), bit1 =
 * the pileup mixes samples (the head element, hence `sample`, is then heap-order dependent). */
typedef struct {
  int64_t n;
  int32_t *contig;
  int64_t *pos;
  int32_t *sample;
  int32_t *count;
  int64_t *ref_off;  int32_t *ref_len;
  int64_t *alt_off;  int32_t *alt_len;
  uint8_t *allele_pool;
  int64_t pool_len;
  uint8_t *flags;
} gq_allele_counts;
gq_status gq_variant_support(gq_ctx *ctx, const gq_dev_reads *reads, const gq_loci *loci, gq_allele_counts **out);
void gq_free_allele_counts(gq_allele_counts *c);

/* germline-standard: GermlineStandard.Caller.callVariantsAtLocus (commands/GermlineStandardCaller
 * .scala:90-124) over pileupFlatMap(reads, partitions, skipEmpty = true) (:63-68), then
 * GenotypeFilter (filters/GenotypeFilter.scala:140-154) when apply_filters.  Results in a
 * gq_somatic_calls: one row per CalledAllele, `sample` its sample slot, `tumor` its
 * AlleleEvidence, `gq` its phredScaledLikelihood, `normal` and `log_odds` zero; flags bit0 =
 * the pileup reference base came from heap order.  A sample's rows follow sample order (the
 * reference iterates a Scala Map there: unpinned for > 1 sample).                          */
typedef struct {
  int32_t min_mapq;                 /* --min-mapq (1): QualityAlignedReadsFilter        */
  int32_t min_read_depth;           /* --min-read-depth (0)                             */
  int32_t max_read_depth;           /* --max-read-depth (Int.MaxValue)                  */
  int32_t min_alternate_read_depth; /* --min-alternate-read-depth (0)                   */
  int32_t min_likelihood;           /* --min-likelihood (0)                             */
  int32_t apply_filters;            /* 0 => raw callVariantsAtLocus output              */
} gq_germline_std_params;
gq_status gq_germline_standard(gq_ctx *ctx, const gq_dev_reads *reads, const gq_loci *loci,
                               const gq_germline_std_params *params, gq_somatic_calls **out);

/* allele-evidence: AlleleEvidence.apply (variants/AlleleEvidence.scala:58-101) for EVERY distinct
 * allele of every sample's pileup, at the loci pileupFlatMap(reads, partitions, skipEmpty = true)
 * visits: what a callback handed to pileupFlatMap could compute itself from the whole pileup.
 * Elements of reads with mapq < min_mapq are dropped first (QualityAlignedReadsFilter,
 * PileupElementsFilter.scala:25-36); the pileup's reference base is the unfiltered pileup's, as in
 * the callers.  With variants_only, only loci whose filtered pileup holds a non-Match element
 * (VariantLocus.apply's depth > referenceDepth, commands/VAFHistogram.scala:31-37) are processed.
 * One row per (locus, sample present in the filtered pileup (Pileup.bySample, Pileup.scala:57-61),
 * distinct allele of that sample's filtered pileup); read_depth / forward_depth are that sample's
 * filtered pileup's, the means run in pileup element order.  Rows: loci in call order, samples
 * ascending, alleles by (ref, alt) bytes.  Loci whose filtered pileup is empty give no row.     */
typedef struct {
  int32_t min_mapq;        /* keep elements with read mapq >= min_mapq; 0 keeps all */
  int32_t variants_only;   /* 1: only loci with a non-Match element after the filter */
} gq_allele_evidence_params;
typedef struct {
  int64_t n;
  int32_t *contig;  int64_t *pos;  int32_t *sample;
  int64_t *ref_off; int32_t *ref_len; int64_t *alt_off; int32_t *alt_len;   /* into allele_pool */
  uint8_t *allele_pool; int64_t pool_len;
  gq_evidence *evidence;   /* likelihood = 0.0; the other nine fields as AlleleEvidence.apply */
  uint8_t *flags;          /* bit0: reference base taken from heap order (MD tags disagree) */
  int64_t visited_loci;    /* loci whose filtered pileup is not empty               */
  int64_t listed_loci;     /* loci handed to the per-locus kernel (variants_only: the variant loci) */
} gq_allele_evidence_rows;
#ifdef __cplusplus
static_assert(sizeof(gq_evidence) == 64, "gq_evidence layout");
static_assert(sizeof(gq_allele_evidence_params) == 8, "gq_allele_evidence_params layout");
static_assert(sizeof(gq_allele_evidence_rows) == 112, "gq_allele_evidence_rows layout");
#endif
gq_status gq_allele_evidence(gq_ctx *ctx, const gq_dev_reads *reads, const gq_loci *loci,
                             const gq_allele_evidence_params *params, gq_allele_evidence_rows **out);
void gq_free_allele_evidence(gq_allele_evidence_rows *rows);

/* genotype-likelihoods: Likelihood.likelihoodsOfAllPossibleGenotypesFromPileup
 * (likelihood/Likelihood.scala:99-201) with logSpace = true and prior 1, for every sample's
 * pileup at the loci pileupFlatMap(reads, partitions, skipEmpty = true) visits: the values the
 * Bayesian callers compute and reduce to one genotype.  The loci, the mapq filter, the reference
 * base and variants_only are gq_allele_evidence's.  One group per (locus, sample present in the
 * filtered pileup) that has an eligible allele: a distinct allele of the filtered pileup whose alt
 * bases are all standard (:106).  A group of n eligible alleles, in Allele order, has the
 * n (n + 1) / 2 genotypes (i <= j) row-major (:107-110); log_likelihood holds, per genotype, the
 * Colt fold + log(1.0) - log(2) * depth (:185-187), less log(sum of exp) over the group's genotypes
 * in that order when normalize is set (:191-193).  Very deep pileups underflow to -inf / NaN as
 * the reference's do.  Groups: loci in call order, samples ascending.  Every array lives in one
 * block (block_), filled by one device-to-host copy.                                          */
typedef struct {
  int32_t min_mapq;           /* keep elements with read mapq >= min_mapq; 0 keeps all */
  int32_t variants_only;      /* 1: only loci with a non-Match element after the filter */
  int32_t include_alignment;  /* 0: probabilityCorrectIgnoringAlignment, 1: ...IncludingAlignment */
  int32_t normalize;          /* 1: normalized log-likelihoods */
} gq_genotype_likelihood_params;
typedef struct {
  int64_t n_groups;            /* (locus, sample) groups                                  */
  int32_t *contig; int64_t *pos; int32_t *sample;
  int32_t *depth;              /* the sample's filtered pileup size                        */
  int32_t *n_alleles;          /* eligible alleles n; the group has n(n+1)/2 genotypes     */
  int64_t *allele_first, *geno_first;   /* into the allele columns / log_likelihood        */
  uint8_t *flags;              /* bit0: reference base from heap order                     */
  int64_t n_alleles_total;
  int64_t *ref_off; int32_t *ref_len; int64_t *alt_off; int32_t *alt_len; int32_t *allele_depth;
  uint8_t *allele_pool; int64_t pool_len;
  int64_t n_genotypes; double *log_likelihood;
  int64_t visited_loci, listed_loci;
  void *block_;
} gq_genotype_likelihoods;
#ifdef __cplusplus
static_assert(sizeof(gq_genotype_likelihood_params) == 16, "gq_genotype_likelihood_params layout");
static_assert(sizeof(gq_genotype_likelihoods) == 176, "gq_genotype_likelihoods layout");
#endif
gq_status gq_genotype_likelihoods_call(gq_ctx *ctx, const gq_dev_reads *reads, const gq_loci *loci,
                                       const gq_genotype_likelihood_params *params, gq_genotype_likelihoods **out);
void gq_free_genotype_likelihoods(gq_genotype_likelihoods *res);

/* pileup-elements: the Pileup itself (pileup/Pileup.scala:49-132, pileup/PileupElement.scala) at
 * the loci pileupFlatMap(reads, partitions, skipEmpty = true) visits: the general case of a
 * per-locus callback, which a host runs over the flat arrays below.  The loci, the mapq filter,
 * the reference base, variants_only and the flag bit are gq_allele_evidence's.  One group per
 * locus whose filtered pileup is not empty, in call order.  A group holds
 *   - its kept elements [elem_first, elem_first + depth) in Pileup.elements order: the task
 *     window's initial-group reads still covering the locus in currentRegions() heap order, then
 *     the other covering reads in read order (the filter removes elements without reordering;
 *     Pileup.bySample is a stable filter on elem_sample);
 *   - its distinct alleles [allele_first, allele_first + n_alleles) over the kept elements, in
 *     Allele order (ref bytes, then alt bytes), with each one's element count.
 * Every array lives in one block (block_), filled by one device-to-host copy.                  */
typedef struct {
  int32_t min_mapq;        /* keep elements with read mapq >= min_mapq; 0 keeps all */
  int32_t variants_only;   /* 1: only loci with a non-Match element after the filter */
} gq_pileup_elements_params;
/* elem_kind: PileupElement.alignment against the pileup's reference base */
enum { GQ_ELEM_MATCH = 0, GQ_ELEM_MISMATCH = 1, GQ_ELEM_INSERTION = 2, GQ_ELEM_DELETION = 3,
       GQ_ELEM_MIDDELETION = 4, GQ_ELEM_CLIPPED = 5 };
typedef struct {
  int64_t n_groups;            /* loci                                                     */
  int32_t *contig; int64_t *pos;
  uint8_t *ref_base;           /* the (unfiltered) pileup's reference base                 */
  uint8_t *flags;              /* bit0: reference base from heap order                     */
  int32_t *depth;              /* kept elements                                            */
  int32_t *n_alleles;          /* distinct alleles of the kept elements                    */
  int64_t *elem_first, *allele_first;   /* into the element / allele columns               */
  int64_t n_alleles_total;
  int64_t *ref_off; int32_t *ref_len; int64_t *alt_off; int32_t *alt_len;   /* into allele_pool */
  int32_t *allele_depth;       /* kept elements with this allele                           */
  uint8_t *allele_pool; int64_t pool_len;
  int64_t n_elements;
  int64_t *elem_read;          /* index into the resident read set (gq_reads_download's numbering) */
  uint8_t *elem_sample;        /* the read's sample slot                                   */
  uint8_t *elem_mapq;
  uint8_t *elem_strand;        /* 1: reverse strand                                        */
  uint8_t *elem_kind;          /* GQ_ELEM_*                                                */
  int32_t *elem_allele;        /* index into the group's alleles (allele_first + ...)      */
  int16_t *elem_quality;       /* PileupElement.qualityScore: the (signed) base quality, the */
                               /* minimum over an insertion's bases, the read's mapq for   */
                               /* MidDeletion / Clipped                                    */
  int32_t *elem_read_position; /* PileupElement.readPosition                               */
  int32_t *elem_cigar_index;   /* PileupElement.cigarElementIndex                          */
  int32_t *elem_index_within;  /* PileupElement.indexWithinCigarElement                    */
  int64_t visited_loci, listed_loci;
  int64_t block_bytes;         /* bytes of block_ (what the device-to-host copy moved)     */
  void *block_;
} gq_pileup_elements;
#ifdef __cplusplus
static_assert(sizeof(gq_pileup_elements_params) == 8, "gq_pileup_elements_params layout");
static_assert(sizeof(gq_pileup_elements) == 256, "gq_pileup_elements layout");
#endif
gq_status gq_pileup_elements_call(gq_ctx *ctx, const gq_dev_reads *reads, const gq_loci *loci,
                                  const gq_pileup_elements_params *params, gq_pileup_elements **out);
void gq_free_pileup_elements(gq_pileup_elements *res);

/* vaf-histogram: VAFHistogram.variantLociFromReads + generateVAFHistogram
 * (commands/VAFHistogram.scala:208-229, 188-196): at every visited locus whose pileup holds a
 * non-Match element (VariantLocus.apply, :31-37), VAF = (depth - referenceDepth).toFloat /
 * depth; kept when depth >= min_read_depth and VAF >= min_vaf / 100.0; binned as
 * pct - pct % (100 / bins) with pct = (int)(VAF * 100).  counts[b] = loci in the bin starting
 * at b.  GQ_E_ASSERT unless 1 <= bins <= 100 (the reference's assume).                      */
typedef struct {
  int32_t bins;            /* --bins (20)          */
  int32_t min_read_depth;  /* --min-read-depth (0) */
  int32_t min_vaf;         /* --min-vaf (0)        */
} gq_vaf_params;
typedef struct {
  int64_t counts[101];
  int64_t variant_loci;  /* loci binned          */
  int64_t visited_loci;  /* non-empty pileups    */
} gq_vaf_hist;
gq_status gq_vaf_histogram(gq_ctx *ctx, const gq_dev_reads *reads, const gq_loci *loci, const gq_vaf_params *params,
                           gq_vaf_hist *out);

/* --reference-fasta (SomaticStandardCaller.scala:57, :75).  A reference genome resident in HBM
 * (replaces ReferenceBroadcast.apply, reference/ReferenceBroadcast.scala:39-55): bases[k] /
 * lengths[k] are the unmasked bases of contig k of the read sets' contig list (bases[k] == NULL
 * for a contig the FASTA lacks).  Bytes are copied; the caller's buffers may be freed after. */
typedef struct gq_reference gq_reference;
gq_status gq_reference_upload(gq_ctx *ctx, int32_t n_contigs, const uint8_t *const *bases, const int64_t *lengths,
                              gq_reference **out);
void gq_reference_free(gq_reference *ref);
/* MD events rebuilt from the reference on the device (ReferenceGenome.buildMdTag,
 * reference/ReferenceGenome.scala:41-47, by Read.fromSAMRecord's choice, reads/Read.scala:
 * 223-247): reads without an MD tag (n_md < 0), or every read with recompute_all, get the events
 * their alignment has against `ref` (a differing base on M/=/X: a mismatch; every base of a D: a
 * deletion).  Any resident read set (gq_reads_upload, gq_reads_wrap_device, gq_bam_dev_reads).
 * The set's md_off / n_md / n_mismatch / md_ev arrays and md_len are replaced, the upload-time
 * structures derived again (gq_reads_rederive) and the projections dropped.  When no read needs
 * a rebuild nothing changes and nothing is re-derived.  `ref` must have the set's number of
 * contigs (GQ_E_ARG).  A failing read leaves the set as it was: info->read is the first one in
 * resident order, info->code its first failing step in CIGAR order:
 *   1 its contig is absent from the reference (ContigNotFound)                     GQ_E_ARG
 *   2 a reference-consuming op other than M/=/X/D (N)                              GQ_E_ARG
 *   3 an M/=/X/D op runs past the contig's end, or M/=/X past the read's sequence  GQ_E_ARG
 *   4 an event's reference byte is not a letter (its MD string would not parse)    GQ_E_MD_PARSE
 * info (may be NULL): read = -1 and code = 0 on success; rebuilt = reads given new events;
 * md_events = the event pool's size afterwards; ms = the device span of count, scan and fill. */
typedef struct { int64_t read; int32_t code; int32_t pad; int64_t rebuilt; int64_t md_events; float ms; } gq_md_rebuild_info;
gq_status gq_reads_rebuild_md(gq_ctx *ctx, gq_dev_reads *r, const gq_reference *ref,
                              int32_t recompute_all, gq_md_rebuild_info *info);
/* Reads of the resident set without MD events (n_md < 0), counted on the device. */
gq_status gq_reads_missing_md(const gq_dev_reads *r, int64_t *out);
/* The last rebuild's spans on this context, HIP events (ms): count, scan, fill; zeros when that
 * call rebuilt nothing or failed. */
gq_status gq_md_rebuild_spans(const gq_ctx *ctx, float *out3);
/* gq_somatic_standard with pileupFlatMapTwoRDDs' referenceGenome argument
 * (DistributedUtil.scala:316-335): every pileup's reference base is the reference's
 * (DistributedUtil.scala:266-268) instead of the reads' MD-derived one.  ref == NULL is
 * gq_somatic_standard.  GQ_E_ARG when a loci range lies on a contig the reference lacks
 * (ContigNotFound, ReferenceBroadcast.scala:26-30) or runs past its end.               */
gq_status gq_somatic_standard_ref(gq_ctx *ctx, const gq_dev_reads *tumor, const gq_dev_reads *normal,
                                  const gq_loci *loci, const gq_reference *ref, const gq_somatic_params *params,
                                  gq_somatic_calls **out);

/* somatic-likelihoods: what SomaticStandard.Caller.findPotentialVariantAtLocus
 * (commands/SomaticStandardCaller.scala:162-245) computes before it keeps one allele per locus and
 * applies --odds, so that a host can apply its own somatic rule.  One group per locus that
 * pileupFlatMapTwoRDDs(tumor, normal, partitions, skipEmpty = true) visits, in call order, where the
 * caller's gate (:184-190) passes after PileupFilter(filter_multi_allelic, min_mapq,
 * minEdgeDistance = 0) on each pileup: both filtered pileups non-empty, both depths <=
 * max_read_depth, tumor referenceDepth != depth, and the tumor has an eligible allele (:200).  Each
 * sample's reference base is its own unfiltered pileup's (MD-derived; no gq_reference here).
 * A sample's alleles are its eligible alleles (Likelihood.scala:106) in Allele order, each with its
 * filtered element count; its n (n + 1) / 2 genotypes (i <= j) row-major hold the normalised
 * log-likelihoods (normalize = true, log space): the tumor's with
 * probabilityCorrectIncludingAlignment, the normal's with probabilityCorrectIgnoringAlignment (the
 * normal's at every group; the reference forces them only when has_variant).  best = the first
 * maximum of exp(tumor log-likelihood) (maxBy, :203); has_variant = that genotype's
 * hasVariantAllele; normal_variant_total = the normal's variant genotypes' likelihoods added in the
 * iteration order of the Map `toMap` builds (:206-217); log_odds = log(exp(tumor_ll[best]) /
 * normal_variant_total) (:218, :236; +inf where the normal has no variant genotype).
 * flags bit0 / bit1: the tumor / normal reference base came from heap order (bit0 as
 * gq_somatic_standard's record flag).  Capacities are gq_somatic_standard's: 1024 distinct alleles
 * per sample, 256 eligible normal alleles (the variant mass ranks every normal genotype), the
 * heap-order replay's limit; past them GQ_E_CAPACITY.  Every array lives in one block (block_),
 * filled by one device-to-host copy.                                                            */
typedef struct {
  int32_t min_mapq;             /* --min-mapq (1)                                   */
  int32_t filter_multi_allelic; /* --filter-multi-allelic                           */
  int32_t max_read_depth;       /* the caller's maxReadDepth (Int.MaxValue)          */
  int32_t reserved;             /* 0                                                */
} gq_somatic_likelihood_params;
typedef struct {
  int64_t n_groups;            /* loci                                                     */
  int32_t *contig; int64_t *pos;
  uint8_t *flags;
  uint8_t *tumor_ref_base, *normal_ref_base;
  int32_t *tumor_depth, *normal_depth;          /* filtered depths                         */
  int32_t *tumor_n_alleles, *normal_n_alleles;  /* eligible alleles n: n(n+1)/2 genotypes  */
  int64_t *tumor_allele_first, *normal_allele_first;  /* into the samples' allele columns  */
  int64_t *tumor_geno_first, *normal_geno_first;      /* into the samples' log-likelihoods */
  int32_t *best;               /* index among the group's tumor genotypes                  */
  uint8_t *has_variant;
  double *normal_variant_total, *log_odds;
  int64_t n_tumor_alleles;
  int64_t *tumor_ref_off; int32_t *tumor_ref_len; int64_t *tumor_alt_off; int32_t *tumor_alt_len;
  int32_t *tumor_allele_depth;
  int64_t n_normal_alleles;
  int64_t *normal_ref_off; int32_t *normal_ref_len; int64_t *normal_alt_off; int32_t *normal_alt_len;
  int32_t *normal_allele_depth;
  uint8_t *allele_pool; int64_t pool_len;       /* both samples' allele bytes              */
  int64_t n_tumor_genotypes; double *tumor_log_likelihood;
  int64_t n_normal_genotypes; double *normal_log_likelihood;
  int64_t visited_loci;        /* loci where either pileup is not empty                    */
  int64_t listed_loci;         /* loci handed to the per-locus kernel                      */
  int64_t block_bytes;         /* bytes of block_ (what the device-to-host copy moved)     */
  void *block_;
} gq_somatic_likelihoods;
#ifdef __cplusplus
static_assert(sizeof(gq_somatic_likelihood_params) == 16, "gq_somatic_likelihood_params layout");
static_assert(sizeof(gq_somatic_likelihoods) == 320, "gq_somatic_likelihoods layout");
#endif
gq_status gq_somatic_likelihoods_call(gq_ctx *ctx, const gq_dev_reads *tumor, const gq_dev_reads *normal,
                                      const gq_loci *loci, const gq_somatic_likelihood_params *params,
                                      gq_somatic_likelihoods **out);
void gq_free_somatic_likelihoods(gq_somatic_likelihoods *res);

/* pileup-counts: the per-locus table of pileupFlatMap(reads, partitions, skipEmpty = true) over
 * one read set, all samples merged: strand-split base counts and element-kind counts.  Elements of
 * reads with mapq < min_mapq are dropped first (QualityAlignedReadsFilter); the reference base is
 * the unfiltered pileup's and the flag bit gq_allele_evidence's.  One row per locus whose filtered
 * pileup has depth >= max(1, min_depth) (and, with variants_only, depth > ref_depth), in call
 * order; unlike gq_pileup_counts (dense, unfiltered, one entry per locus of `loci`) the rows are
 * compacted on the device.  At every row
 *   depth == sum(base_count) + sum(kind_count),
 *   ref_depth == base_count[index of ref_base] (N at index 4),
 *   sum(base_forward) <= forward_depth <= depth.
 * The call stages 96 bytes of device memory per locus of every 512-locus tile of `loci` a read
 * overlaps: a caller whose covered loci need more than the device has makes several calls over
 * whole tasks (a task's first pileup defines its heap order).  Every array lives in one block (block_), filled by one device-to-host copy.
 * (The result struct cannot take the name of the function gq_pileup_counts.)                   */
typedef struct {
  int32_t min_mapq;        /* keep elements with read mapq >= min_mapq; 0 keeps all */
  int32_t min_depth;       /* rows with depth >= max(1, min_depth)                  */
  int32_t variants_only;   /* 1: only rows with depth > ref_depth                   */
  int32_t reserved;        /* 0                                                     */
} gq_pileup_counts_params;
typedef struct {
  int64_t n;                   /* rows                                                     */
  int32_t *contig; int64_t *pos;
  uint8_t *ref_base;           /* the (unfiltered) pileup's reference base: A C G T or N   */
  uint8_t *flags;              /* bit0: reference base from heap order                     */
  int32_t *depth;              /* kept elements                                            */
  int32_t *forward_depth;      /* ... of positive-strand reads                             */
  int32_t *ref_depth;          /* Match elements                                           */
  int32_t *base_count;         /* [n * 6] Match/Mismatch elements by sequenced base: A C G T N other */
  int32_t *base_forward;       /* [n * 6] ... of positive-strand reads                     */
  int32_t *kind_count;         /* [n * 4] Insertion, Deletion, MidDeletion, Clipped elements */
  int64_t visited_loci;        /* loci whose filtered pileup is not empty                  */
  int64_t listed_loci;         /* loci handed to the per-locus kernel                      */
  int64_t block_bytes;         /* bytes of block_ (what the device-to-host copy moved)     */
  void *block_;
} gq_pileup_count_rows;
#ifdef __cplusplus
static_assert(sizeof(gq_pileup_counts_params) == 16, "gq_pileup_counts_params layout");
static_assert(sizeof(gq_pileup_count_rows) == 120, "gq_pileup_count_rows layout");
#endif
gq_status gq_pileup_counts_call(gq_ctx *ctx, const gq_dev_reads *reads, const gq_loci *loci,
                                const gq_pileup_counts_params *params, gq_pileup_count_rows **out);
void gq_free_pileup_counts(gq_pileup_count_rows *res);

/* active-regions: the intervals of `loci` where the pileup shows evidence of a variant, found on the
 * device from the staging rows of pileup-counts (the table never leaves the GPU).  This contract is
 * the project's own; the reference has no such stage.  All arithmetic is integer.
 * Evidence.  At a locus take the pileup-counts row of the min_mapq-filtered pileup (reference base:
 * the unfiltered pileup's, as there).  If ref_base is not one of A C G T, e = 0.  Otherwise
 *   e = base_count[A] + base_count[C] + base_count[G] + base_count[T] - ref_depth
 *       + kind_count[Insertion] + kind_count[Deletion] + kind_count[MidDeletion].
 * Sequenced N, "other" bases and Clipped elements are not evidence.  The locus is active iff
 *   depth >= max(1, min_depth)  and  e >= max(1, min_evidence)  and  100 * e >= min_percent * depth
 * (the products in int64).
 * Regions.  The active loci of the whole call sorted by (contig, pos), whatever the task partition
 * of `loci`.  Consecutive active loci fall in one region iff they share a contig and
 * pos - prev <= 2 * pad + 1 (their intervals dilated by pad overlap or touch).  A region is
 * [max(0, first - pad), last + pad + 1) with n_active, the number of its active loci, and evidence,
 * the int64 sum of their e.  The upper end is not clipped: the library does not know the contig
 * lengths here.
 * Result: one block (block_), filled by one device-to-host copy: the regions, and the active loci
 * in sorted order (few, and they make a wrong region diagnosable).  No active locus: n == 0 and
 * n_loci == 0 with a valid block.  GQ_E_ARG: a null pointer, pad < 0, min_percent
 * outside 0..100.  Capacity limits are gq_pileup_counts_call's.  The host twin takes pileup-count
 * columns (rows in any order; visited_loci and listed_loci are 0 in its block).                  */
typedef struct {
  int32_t min_mapq;      /* 1: as pileup-counts                                         */
  int32_t min_depth;     /* 4: minimum filtered depth; below 1 counts as 1              */
  int32_t min_evidence;  /* 2: minimum e; below 1 counts as 1                           */
  int32_t min_percent;   /* 8: minimum share of the depth e must reach, 0..100          */
  int32_t pad;           /* 75: dilation on each side of an active locus, >= 0          */
  int32_t reserved[3];   /* 0                                                           */
} gq_active_params;
typedef struct {
  int64_t n;                   /* regions, ascending by (contig, start)                    */
  int32_t *contig; int64_t *start; int64_t *end;
  int32_t *n_active;           /* active loci of the region                                */
  int64_t *evidence;           /* sum of their e                                           */
  int64_t n_loci;              /* active loci, ascending by (contig, pos)                  */
  int32_t *locus_contig; int64_t *locus_pos;
  int32_t *locus_depth; int32_t *locus_evidence;
  int64_t visited_loci;        /* loci whose filtered pileup is not empty                  */
  int64_t listed_loci;         /* loci handed to the per-locus kernel                      */
  int64_t block_bytes;         /* bytes of block_ (what the device-to-host copy moved)     */
  void *block_;
} gq_active_regions;
#ifdef __cplusplus
static_assert(sizeof(gq_active_params) == 32, "gq_active_params layout");
static_assert(sizeof(gq_active_regions) == 120, "gq_active_regions layout");
#endif
gq_status gq_active_regions_call(gq_ctx *ctx, const gq_dev_reads *reads, const gq_loci *loci,
                                 const gq_active_params *params, gq_active_regions **out);
gq_status gq_active_regions_host(int64_t n_rows, const int32_t *contig, const int64_t *pos, const uint8_t *ref_base,
                                 const int32_t *depth, const int32_t *ref_depth, const int32_t *base_count,
                                 const int32_t *kind_count, const gq_active_params *params, gq_active_regions **out);
void gq_free_active_regions(gq_active_regions *res);

/* structural-variant: large deletions from discordant read pairs (StructuralVariantCaller.scala).
 * No pileup, MD tag or reference is involved; the input need not be sorted.  With len a record's
 * own l_seq, lo / hi the smaller / larger of its start and its mate's start (0-based):
 *   Min = lo, GapMin = lo + len, GapMax = hi, Max = hi + len, insertSize = hi - lo + len.
 * Stages, each with its own call (tests and hosts with their own reader enter where they like):
 *   pairs        records that are paired, mapped (the loader's isMapped), first in pair, not
 *                duplicates, with a mapped mate and tlen != 0, in file order (resident SoA)
 *   stats        in range: contig == mate_contig, strands differ, tlen < 25000 (raw);
 *                oriented = tlen (forward) or -tlen (reverse); median and MAD over every in-range
 *                pair (exact: even counts give the mean of the two middle values, none gives
 *                0, 0); max_normal = (int)(median + 5 mad), truncated toward zero;
 *                exceptional: in range and raw tlen > max_normal, ordered by (contig, lo), stable
 *   graph        nodes = exceptional pairs in that order; for node i the successors j = i + 1 ...
 *                on its contig up to the first with |GapMin_j - Min_i| > N; edge (i, j, weight
 *                |(GapMax_j - Min_j) - (GapMax_i - Min_i)|) unless the pairs are incompatible
 *   cliques      (host) one greedy clique per connected component with an edge: edges by
 *                (weight, i, j), seeded with the first edge's i                              */
typedef struct gq_sv_pairs gq_sv_pairs; /* resident pairs, and after stats / select the node set */
typedef struct {
  int64_t n_pairs, n_in_range, n_exceptional;
  double median, mad;       /* of the oriented sizes of the in-range pairs                    */
  int32_t max_normal;       /* (int)(median + 5 * mad)                                        */
  int32_t reserved;
  float stats_ms, order_ms; /* device spans: mask + sorts + statistics; compaction + ordering */
} gq_sv_stats;
typedef struct {
  int64_t n_nodes, n_edges;
  int32_t *i, *j;           /* node indexes in (contig, lo) order, i < j; by i then j         */
  int64_t *weight;
  float edge_ms;            /* device span of count + scan + fill                             */
  int32_t reserved;
} gq_sv_graph;
typedef struct {
  int64_t n;                /* cliques, by (contig, start, stop)                               */
  int32_t *contig;
  int64_t *start, *stop;    /* the deletion: max GapMin and min GapMax of the members          */
  int64_t *pairs, *wiggle;  /* members; how far the deletion may shrink and still fit them all */
} gq_sv_cliques;
#ifdef __cplusplus
static_assert(sizeof(gq_sv_stats) == 56, "gq_sv_stats layout");
static_assert(sizeof(gq_sv_graph) == 48, "gq_sv_graph layout");
static_assert(sizeof(gq_sv_cliques) == 48, "gq_sv_cliques layout");
#endif
/* pairs of a loaded file (after gq_bam_dev_load; a scan is not needed); parse_ms: device span  */
gq_status gq_sv_pairs_from_bam(gq_bam_dev *b, gq_sv_pairs **out, float *parse_ms);
/* pairs given as host arrays (already through the pairs stage's filter), strand: bit0 read on the
 * reverse strand, bit1 mate on the reverse strand                                             */
gq_status gq_sv_pairs_from_host(gq_ctx *ctx, int64_t n, const int32_t *contig, const int32_t *start,
                                const int32_t *mate_contig, const int32_t *mate_start, const int32_t *tlen,
                                const int32_t *len, const uint8_t *strand, gq_sv_pairs **out);
int64_t gq_sv_pairs_count(const gq_sv_pairs *p);
gq_status gq_sv_pairs_download(const gq_sv_pairs *p, int32_t *contig, int32_t *start, int32_t *mate_contig,
                               int32_t *mate_start, int32_t *tlen, int32_t *len, uint8_t *strand);
void gq_sv_pairs_free(gq_sv_pairs *p);
/* stats, then the node set: the exceptional pairs in (contig, lo) order                        */
gq_status gq_sv_stats_call(gq_sv_pairs *p, gq_sv_stats *out);
/* the node set for a threshold of the caller's: in-range pairs with raw tlen > threshold       */
gq_status gq_sv_select(gq_sv_pairs *p, int32_t threshold, int64_t *n_nodes);
/* the node set: contig, lo, hi, len and the pair's index in the pairs SoA (null: not wanted)   */
gq_status gq_sv_nodes_download(const gq_sv_pairs *p, int32_t *contig, int32_t *lo, int32_t *hi, int32_t *len,
                               int64_t *pair);
/* edges over the node set with N = max_normal.  GQ_E_CAPACITY when the edge list does not fit
 * in device or host memory (nothing is truncated)                                             */
gq_status gq_sv_graph_call(gq_sv_pairs *p, int32_t max_normal, gq_sv_graph **out);
void gq_sv_free_graph(gq_sv_graph *g);
/* host only: cliques of an edge list over nodes in (contig, lo) order (edges distinct, i < j)  */
gq_status gq_sv_cliques_call(int64_t n_nodes, const int32_t *contig, const int32_t *lo, const int32_t *hi,
                             const int32_t *len, int64_t n_edges, const int32_t *ei, const int32_t *ej,
                             const int64_t *weight, int32_t max_normal, gq_sv_cliques **out);
void gq_sv_free_cliques(gq_sv_cliques *c);
/* stats + graph + cliques in one call; edge_ms / clique_ms (null: not wanted): the edge kernels'
 * device span and the cliques' host time                                                      */
gq_status gq_sv_call(gq_sv_pairs *p, gq_sv_stats *stats, gq_sv_cliques **out, float *edge_ms, float *clique_ms);

/* Affine-gap alignment: AffineGapPenaltyAlignment.align (alignment/AffineGapPenaltyAlignment.scala:
 * 20-141) and ReadAlignment.toCigar (alignment/ReadAlignment.scala:28-61), a batch of independent
 * (sequence, reference) pairs.  Semi-global: the whole sequence against any stretch of the reference.
 * Cell (s, r), s = 1..S, r = 0..R, keeps ONE path: its FP64 score and its last state; row 0 is score 0
 * without a state.  Candidates in this order: Insertion from (s-1, r); Deletion from (s, r-1), r > 0;
 * Match / Mismatch (raw bytes equal / not) from (s-1, r-1), r > 0; the first strictly smallest
 * previous score + step cost wins.  The step cost depends on (last state, next state, s == S) only
 * and comes from a table of 32 doubles built once on the host with the reference's term order:
 *   table[16 * (s == S) + 4 * last + next], last: 0 none, 1 Insertion, 2 Deletion, 3 Match or
 *   Mismatch; next: 0 Insertion, 1 Deletion, 2 Match, 3 Mismatch.
 * ref_end = the first r with the strictly smallest score of row S, ref_start = the column where that
 * path left row 0, score_int = (int)score as Double.toInt (truncated, saturating, NaN 0).  The CIGAR
 * is the run-length encoded path in BAM words len << 4 | op with I 1, D 2, = 7, X 8.  An empty
 * sequence gives no operations, score 0 and ref_start = ref_end = 0.
 * Device caps: S <= 512, R <= 4096 (gq_align_limits); a pair beyond them is GQ_E_CAPACITY naming the
 * pair, nothing is truncated and *out is not written.  The host twin has no caps.            */
typedef struct {
  double mismatch_probability;   /* e^-4     */
  double open_gap_probability;   /* e^-6     */
  double close_gap_probability;  /* 1 - e^-1 */
  double reserved[5];            /* 0        */
} gq_align_params;
typedef struct {
  int64_t n;
  int32_t *ref_start, *ref_end;  /* [n] the aligned stretch [ref_start, ref_end) of the pair's reference */
  double *score;                 /* [n]                                                        */
  int32_t *score_int;            /* [n] ReadAlignment.alignmentScore                            */
  int64_t *cigar_off;            /* [n + 1] into cigar                                          */
  uint32_t *cigar;               /* BAM words                                                   */
  float ms;                      /* device span of the call, copies included (0: host twin)     */
  float kernel_ms;               /* ... of align_k alone, summed over the call's launches       */
  int32_t launches;              /* align_k launches (scratch chunks)                           */
  int32_t reserved;
  void *block_;                  /* owner of the arrays above (gq_free_alignments)              */
} gq_alignments;
/* gq_align_reads: which reads were aligned, and against what */
typedef struct {
  int64_t n_reads;               /* reads of the resident set                                   */
  int64_t n_selected;            /* aligned                                                     */
  int64_t skipped;               /* reads with an N or P op: never selected                     */
  float select_ms;               /* device span of selection + compaction                       */
  int32_t reserved;
} gq_align_reads_info;
#ifdef __cplusplus
static_assert(sizeof(gq_align_params) == 64, "gq_align_params layout");
static_assert(sizeof(gq_alignments) == 80, "gq_alignments layout");
static_assert(sizeof(gq_align_reads_info) == 32, "gq_align_reads_info layout");
#endif
/* The default probabilities. */
void gq_align_default_params(gq_align_params *out);
/* The step-cost table; GQ_E_ARG unless every probability lies strictly inside (0, 1). */
gq_status gq_align_penalties(const gq_align_params *params, double table[32]);
/* out[0..7]: max S, max R, lanes per pair (wave width), max rows per lane, bytes of LDS that hold
 * a pair's traceback, 0, 0, 0.  Rows per lane of a pair = ceil(S / lanes), lanes used nl =
 * ceil(S / rows per lane); its traceback takes nl * (R + nl) * (rows per lane <= 4 ? 1 : 2) bytes
 * and lives in LDS when that fits, else in global scratch.                                   */
void gq_align_limits(int32_t out[8]);
/* Pair i: seq_pool[seq_off[i], + seq_len[i]) against ref_pool[ref_off[i], + ref_len[i]) (host
 * arrays, copied to the device).  n == 0: GQ_OK, an empty block, no launch.  Scratch (global
 * traceback and worst-case CIGAR space, (S + R) words a pair) is limited to a quarter of the free
 * device memory, or to GQ_ALIGN_SCRATCH_BYTES when that environment variable is set (never less than
 * one cap-sized pair needs): a batch that needs more runs as several launches over consecutive
 * pairs, with the same result.                                                              */
gq_status gq_align_batch(gq_ctx *ctx, int64_t n, const uint8_t *seq_pool, const int64_t *seq_off,
                         const int32_t *seq_len, const uint8_t *ref_pool, const int64_t *ref_off,
                         const int32_t *ref_len, const gq_align_params *params, gq_alignments **out);
/* The same on the CPU (plain C++, no device, no caps): the twin the GPU results are compared with. */
gq_status gq_align_host(int64_t n, const uint8_t *seq_pool, const int64_t *seq_off, const int32_t *seq_len,
                        const uint8_t *ref_pool, const int64_t *ref_off, const int32_t *ref_len,
                        const gq_align_params *params, gq_alignments **out);
void gq_free_alignments(gq_alignments *a);
/* Resident reads against windows of a resident reference; nothing is copied to the host but the
 * selected reads' indexes and window bounds.  Selected: reads whose CIGAR holds an I, D or S op
 * (every read with all_reads); a read with an N or P op is never selected and counted in
 * info->skipped.  With lead / trail the summed lengths of the leading / trailing S ops (inside any
 * H), end = the read's resident end, the window is [lo, hi) = [max(0, start - lead - pad),
 * min(contig length, end + trail + pad)) and the sequence all stored bases of the read.  Selected
 * reads keep resident order; (*read_index_out)[k] / (*lo_out)[k] (malloc'd, the caller frees) give
 * pair k's resident index and window start.  GQ_E_ARG when a selected read lies on a contig the
 * reference lacks, or `reference` does not cover the set's contigs.                          */
gq_status gq_align_reads(gq_ctx *ctx, const gq_dev_reads *reads, const gq_reference *reference, int32_t pad,
                         int32_t all_reads, const gq_align_params *params, gq_alignments **out,
                         int64_t **read_index_out, int32_t **lo_out, gq_align_reads_info *info);
void gq_align_free_index(void *p);

/* Local assembly over windows: assembly/DeBruijnGraph.scala restated (DESIGN.md "Local assembly").
 * A window is (contig, [start, end)).  Its reads: every resident read whose [start, end) overlaps it,
 * all stored bases (soft clips included), unless a byte is not one of upper-case A C G T or the read
 * is shorter than k.  count(x) = occurrences of k-mer x over those reads; x is a node iff count >=
 * min_occurrence.  A k-mer is packed 2 bits a base (A 0, C 1, G 2, T 3), first base most significant:
 * key_lo holds its last min(k, 31) bases, key_hi the k - 31 before them (0 for k <= 31).  A window's
 * nodes stand sorted by k-mer, i.e. by (key_hi, key_lo).  child_mask bit b: the node's k - 1 last
 * bases followed by base b is a node; parent_mask bit b: base b followed by its k - 1 first bases is.
 * source / sink: the node index (within the window) of the first / last k bytes of the window's
 * reference, -1 when it is no node.  status, the first that holds: GQ_ASM_SHORT (window shorter than
 * k), GQ_ASM_REF_N (contig absent from the reference, window past its end, or a byte of the source
 * or sink outside A C G T), GQ_ASM_NO_SOURCE, GQ_ASM_NO_SINK, else GQ_ASM_OK.  The graph is built
 * whatever the status.                                                                        */
enum {
  GQ_ASM_OK = 0, GQ_ASM_SHORT = 1, GQ_ASM_REF_N = 2, GQ_ASM_NO_SOURCE = 3, GQ_ASM_NO_SINK = 4,
  /* gq_asm_paths ORs these into an OK window's status when its search met a cap */
  GQ_ASM_PATHS_CAPPED = 16, GQ_ASM_STEPS_CAPPED = 32, GQ_ASM_LENGTH_CAPPED = 64
};
typedef struct {
  int32_t k;                /* 2 .. 62                                                          */
  int32_t min_occurrence;   /* >= 1 (1)                                                         */
  int32_t max_paths;        /* >= 1 (10)                                                        */
  int32_t max_path_length;  /* k-mers of a path; 0: window length - k + 1 + 64                  */
  int64_t max_steps;        /* node visits of a window's search (1,000,000)                     */
  int32_t min_mapq;         /* gq_asm_graphs: only reads of at least this mapping quality (0)   */
  int32_t reserved0;        /* 0                                                                */
  int64_t reserved[4];      /* 0                                                                */
} gq_asm_params;
typedef struct {
  int64_t n_windows, n_nodes;
  int64_t *node_off;                    /* [n_windows + 1] into the node arrays                  */
  uint64_t *key_lo, *key_hi;            /* [n_nodes]                                             */
  int32_t *count;                       /* [n_nodes]                                             */
  uint8_t *child_mask, *parent_mask;    /* [n_nodes]                                             */
  int32_t *source, *sink, *status;      /* [n_windows]                                           */
  int32_t *n_reads;                     /* [n_windows] reads that contributed                    */
  int32_t *win_len;                     /* [n_windows] end - start                               */
  int64_t *n_instances;                 /* [n_windows] k-mer occurrences counted                 */
  int32_t k, min_occurrence;
  float ms;                             /* device span of the call, copies included (0: twin)    */
  float reads_ms;                       /* ... of finding the windows' reads                     */
  float count_ms, edges_ms;             /* ... of asm_window_k, split by its own clock readings into
                                           counting and prune / order / edges                    */
  int32_t launches;                     /* asm_window_k launches                                 */
  int32_t n_global;                     /* windows counted over a table in global scratch        */
  void *block_;                         /* owner of the arrays above (gq_asm_free_graphs)        */
} gq_asm_graph_block;
typedef struct {
  int64_t n_windows, n_haplotypes, n_unitigs;
  int64_t *hap_off;         /* [n_windows + 1] a window's haplotypes, in discovery order          */
  int64_t *hap_seq_off;     /* [n_haplotypes + 1] into bases                                     */
  uint8_t *bases;           /* mergeKmers of each path                                           */
  int32_t *support;         /* [n_haplotypes] smallest count along the path                      */
  int32_t *status;          /* [n_windows] the graph's status | GQ_ASM_*_CAPPED                  */
  int64_t *steps;           /* [n_windows] node visits of the search                             */
  int64_t *unitig_off;      /* [n_windows + 1] a window's unitigs, by first k-mer                */
  int64_t *unitig_seq_off;  /* [n_unitigs + 1] into unitig_bases                                 */
  uint8_t *unitig_bases;
  float ms;                 /* host time of the call                                             */
  int32_t reserved;
  void *block_;
} gq_asm_path_block;
#ifdef __cplusplus
static_assert(sizeof(gq_asm_params) == 64, "gq_asm_params layout");
static_assert(sizeof(gq_asm_graph_block) == 152, "gq_asm_graph_block layout");
static_assert(sizeof(gq_asm_path_block) == 112, "gq_asm_path_block layout");
#endif
void gq_asm_default_params(gq_asm_params *out);
/* out[0..7]: min k, max k, bases per key word, LDS table slots in use (GQ_ASM_LDS_SLOTS applied),
 * LDS table slots compiled in, threads per window, LDS bytes per workgroup, 0                 */
void gq_asm_limits(int32_t out[8]);
/* The graphs of n_windows windows of a resident read set; contig indexes the set's contig list.
 * GQ_E_ARG for k outside 2 .. 62, a contig outside the list, start < 0 or end < start.  n_windows
 * == 0: GQ_OK, an empty block, no launch.  A window is counted over a hash table in LDS; one whose
 * distinct k-mers do not fit is counted again by the same code over a table in global scratch sized
 * from its instance count.  GQ_ASM_LDS_SLOTS (environment, rounded down to a power of two, at least
 * 2) caps the LDS table.  Scratch is limited to a quarter of the free device memory, or to
 * GQ_ASM_SCRATCH_BYTES when set (never less than one window needs): a batch that needs more runs as
 * several launches over consecutive windows, with the same result.                             */
gq_status gq_asm_graphs(gq_ctx *ctx, const gq_dev_reads *reads, const gq_reference *reference, int64_t n_windows,
                        const int32_t *contig, const int32_t *start, const int32_t *end,
                        const gq_asm_params *params, gq_asm_graph_block **out);
/* The same block on the CPU (plain C++, no device), bit for bit.  Read r = seq_pool[seq_off[r], +
 * seq_len[r]); window w lists its overlapping reads win_reads[win_read_off[w] .. win_read_off[w + 1])
 * and has the win_len[w] reference bytes at ref_pool + ref_off[w] (ref_off[w] < 0: none, REF_N).
 * threads: worker threads over the windows (<= 1: the calling thread).                          */
gq_status gq_asm_graphs_host(int64_t n_windows, const uint8_t *seq_pool, const int64_t *seq_off,
                             const int32_t *seq_len, const int64_t *win_read_off, const int64_t *win_reads,
                             const uint8_t *ref_pool, const int64_t *ref_off, const int32_t *win_len,
                             const gq_asm_params *params, int32_t threads, gq_asm_graph_block **out);
void gq_asm_free_graphs(gq_asm_graph_block *g);
/* Host only: haplotypes and unitigs of a graph block (either producer's).  Haplotypes of an OK
 * window: every simple path source .. sink, depth first, children in A C G T order, a node barred
 * only while on the current path; a path that reaches the sink ends there.  Entering a node is a
 * step.  A child that would make the path longer than max_path_length is not entered
 * (LENGTH_CAPPED); the search stops when a step beyond max_steps (STEPS_CAPPED) or a path beyond
 * max_paths (PATHS_CAPPED) is due.  Unitigs of every window: the maximal paths whose steps x -> y
 * have y the only child of x and x the only parent of y (x != y), sorted by first k-mer; an
 * unbranched cycle starts at its smallest k-mer.  params->k and min_occurrence are the block's. */
gq_status gq_asm_paths(const gq_asm_graph_block *graphs, const gq_asm_params *params, gq_asm_path_block **out);
void gq_asm_free_paths(gq_asm_path_block *p);

/* Haplotype likelihoods: every read of a window against every haplotype assembled for it (a pair-HMM
 * forward pass), then Likelihood.likelihoodsOfGenotypes (likelihood/Likelihood.scala) with a uniform
 * prior, in log space, over reads instead of pileup elements and over haplotypes instead of alleles
 * (DESIGN.md "Haplotype likelihoods").
 * Pair: a read of S bases with qualities q[1..S] against a haplotype of R bases.  Cells (s, r),
 * s = 0..S, r = 0..R, three FP64 values M I D each.  With open = open_gap_probability and ext = 1 -
 * close_gap_probability: tMM = 1 - (open + open), tMI = tMD = open, tII = tDD = ext, tIM = tDM = 1 -
 * ext (trans[0..6] in that order of tMM tMI tMD tII tDD tIM tDM, trans[7] = 0).  Emission of read base
 * s against haplotype base r: match[q] when the raw bytes are equal, else mismatch[q], where for qe =
 * min(max(q, quality_floor), 255) match[q] = phredToSuccessProbability(qe) = 1 - 10^(-qe / 10) and
 * mismatch[q] = (1 - match[q]) / 3.  A read without qualities (a null quality pool) has 1 -
 * mismatch_probability and mismatch_probability / 3 for every base; mismatch_probability has no other
 * use.  Every product and sum below is rounded on its own, in the written order (no fused multiply-add):
 *   row 0:     M = I = 0, D(0, r) = INIT / (double)R for r = 0..R, INIT = 2^1000
 *   column 0:  M(s, 0) = D(s, 0) = 0 for s >= 1
 *   M(s, r) = prior(s, r) * ((M(s-1, r-1) * tMM + I(s-1, r-1) * tIM) + D(s-1, r-1) * tDM)      r >= 1
 *   I(s, r) = M(s-1, r) * tMI + I(s-1, r) * tII                                                 r >= 0
 *   D(s, r) = M(s, r-1) * tMD + D(s, r-1) * tDD                                                 r >= 1
 *   sum = 0; for r = 1..R ascending: sum = sum + (M(S, r) + I(S, r))
 * scaled = sum and log_likelihood = log(sum) - log(INIT), the natural logarithm of fdlibm (StrictMath)
 * on both sides.  sum < DBL_MIN (zero or subnormal): log_likelihood = -infinity and the flag
 * GQ_HL_UNDERFLOW; nothing else is done about underflow.  S == 0 or R == 0: scaled 0, -infinity and
 * GQ_HL_EMPTY.  Device caps: S <= 512, R <= 4096 (the aligner's); a pair beyond them is GQ_E_CAPACITY
 * naming the pair, nothing is truncated and *out is not written.  The host twin has no caps.
 * Genotypes of a window with H haplotypes and reads 0..N-1 in list order: g runs over (i, j), i <= j,
 * i-major;  gl(g) = 0; for n ascending: gl = gl + ((log(scaled[n][i] + scaled[n][j]) - log(INIT)) -
 * log(2.0)).  A read whose two sums are both 0 makes the genotype -infinity.  H == 0 or N == 0: the
 * window has no genotypes.                                                                     */
enum { GQ_HL_UNDERFLOW = 1, GQ_HL_EMPTY = 2 };
typedef struct {
  double mismatch_probability;   /* e^-4: only for reads without qualities                      */
  double open_gap_probability;   /* e^-6, below 0.5                                             */
  double close_gap_probability;  /* 1 - e^-1                                                    */
  double quality_floor;          /* 6: a whole number in 0 .. 255                               */
  double reserved[4];            /* 0                                                           */
} gq_haplik_params;
typedef struct {
  int64_t n;
  double *scaled;                /* [n] the sum over row S, scaled by INIT                      */
  double *log_likelihood;        /* [n]                                                         */
  uint8_t *flags;                /* [n] GQ_HL_*                                                 */
  float ms;                      /* device span of the call, copies included (0: host twin)     */
  float kernel_ms;               /* ... of hap_forward_k alone                                  */
  void *block_;                  /* owner of the arrays above (gq_haplik_free_pairs)            */
} gq_haplik_pairs;
typedef struct {
  int64_t n_windows, n_reads, n_pairs, n_genotypes;
  int64_t *win_read_off;         /* [n_windows + 1] into win_reads                              */
  int64_t *win_reads;            /* [n_reads] resident read indexes, list order                 */
  int64_t *lik_off;              /* [n_windows + 1] window w's pairs, read-major: read n of its list
                                    against its haplotype h at lik_off[w] + n * H_w + h         */
  double *scaled, *log_likelihood;  /* [n_pairs]                                                */
  uint8_t *flags;                /* [n_pairs] GQ_HL_*                                           */
  int64_t *gt_off;               /* [n_windows + 1] into gt_log_likelihood                      */
  double *gt_log_likelihood;     /* [n_genotypes] a window's genotypes (i, j), i <= j, i-major   */
  int32_t *best_genotype;        /* [n_windows] index within the window of the first largest
                                    gt_log_likelihood, -1 when the window has none              */
  float ms;                      /* device span of the call, copies included                    */
  float reads_ms;                /* ... of finding the windows' reads                           */
  float kernel_ms;               /* ... of hap_forward_k                                        */
  float genotype_ms;             /* ... of the genotype kernels                                 */
  void *block_;                  /* owner of the arrays above (gq_haplik_free_block)            */
} gq_haplik_block;
#ifdef __cplusplus
static_assert(sizeof(gq_haplik_params) == 64, "gq_haplik_params layout");
static_assert(sizeof(gq_haplik_pairs) == 48, "gq_haplik_pairs layout");
static_assert(sizeof(gq_haplik_block) == 128, "gq_haplik_block layout");
#endif
void gq_haplik_default_params(gq_haplik_params *out);
/* The tables the kernel and the twin read.  GQ_E_ARG unless every probability lies strictly inside
 * (0, 1), open_gap_probability < 0.5 and quality_floor is a whole number in 0 .. 255.            */
gq_status gq_haplik_tables(const gq_haplik_params *params, double trans[8], double match[256], double mismatch[256]);
/* Pair i: seq_pool[seq_off[i], + seq_len[i]) with the qualities at the same offsets of qual_pool
 * (null: no qualities) against hap_pool[hap_off[i], + hap_len[i]) (host arrays, copied to the
 * device).  n == 0: GQ_OK, an empty block, no launch.                                            */
gq_status gq_haplik_batch(gq_ctx *ctx, int64_t n, const uint8_t *seq_pool, const int64_t *seq_off,
                          const int32_t *seq_len, const uint8_t *qual_pool, const uint8_t *hap_pool,
                          const int64_t *hap_off, const int32_t *hap_len, const gq_haplik_params *params,
                          gq_haplik_pairs **out);
/* The same on the CPU (plain C++, no device, no caps), `threads` workers over the pairs (<= 1: the
 * calling thread): the twin the GPU results are compared with.                                   */
gq_status gq_haplik_host(int64_t n, const uint8_t *seq_pool, const int64_t *seq_off, const int32_t *seq_len,
                         const uint8_t *qual_pool, const uint8_t *hap_pool, const int64_t *hap_off,
                         const int32_t *hap_len, const gq_haplik_params *params, int32_t threads,
                         gq_haplik_pairs **out);
void gq_haplik_free_pairs(gq_haplik_pairs *p);
/* The resident reads of each window against the haplotypes `paths` holds for it (hap_off, hap_seq_off
 * and bases of a gq_asm_path_block over the same n_windows windows), and the windows' genotypes.  A
 * window's reads are gq_asm_graphs's, in its list order: overlap, at least asm_params->k bases, every
 * byte one of A C G T, mapping quality >= asm_params->min_mapq (no other field of asm_params is
 * read; null: the defaults).  Pairs, likelihoods and genotypes are made on the device; nothing comes
 * back to the host but the block.  GQ_E_CAPACITY names the first pair over a cap.                */
gq_status gq_haplik_windows(gq_ctx *ctx, const gq_dev_reads *reads, const gq_reference *reference, int64_t n_windows,
                            const int32_t *contig, const int32_t *start, const int32_t *end,
                            const gq_asm_params *asm_params, const gq_asm_path_block *paths,
                            const gq_haplik_params *params, gq_haplik_block **out);
void gq_haplik_free_block(gq_haplik_block *b);
/* Host only: the genotype step.  Window w has the reads win_read_off[w + 1] - win_read_off[w], the
 * haplotypes hap_off[w + 1] - hap_off[w] and its pairs' scaled values at lik_off[w], read-major.
 * gt_off[n_windows + 1] is always written; gt_log_likelihood (room for gt_capacity values) and
 * best_genotype[n_windows] when gt_log_likelihood is not null (null: the offsets alone, to size it).
 * GQ_E_ARG when gt_capacity is less than gt_off[n_windows].                                      */
gq_status gq_haplik_genotypes_host(int64_t n_windows, const int64_t *win_read_off, const int64_t *hap_off,
                                   const int64_t *lik_off, const double *scaled, int64_t *gt_off,
                                   double *gt_log_likelihood, int64_t gt_capacity, int32_t *best_genotype);

/* Variants from assembled haplotypes: the events the aligned haplotypes of a window carry, and per
 * event the likelihoods of the genotypes 0/0, 0/1, 1/1 marginalised over the haplotypes (DESIGN.md
 * "Variants from haplotypes").  This contract is the project's own; the reference has no such stage.
 * Inputs (gq_hapvar_input, host arrays; the device entry uploads them): per window w its contig
 * coordinate win_start[w] and its win_len[w] reference bytes at ref_pool + ref_off[w] (ref_off[w] < 0:
 * none); hap_off, hap_seq_off, bases of a path block; per haplotype hap_align[h], an index into the
 * alignment arrays (ref_start, ref_end, cigar_off, cigar of a gq_alignments over n_align pairs) or -1
 * when the haplotype was not aligned; win_read_off, lik_off, scaled of a likelihood block.
 * Usable haplotypes.  Haplotype h of window w is usable iff hap_align[h] >= 0, the window has reference
 * bytes, ref_start == 0 and ref_end == win_len[w].  Otherwise hap_flags[h] is GQ_HV_HAP_UNALIGNED (no
 * alignment, or no reference bytes) or GQ_HV_HAP_PARTIAL; such a haplotype makes no events and takes no
 * part in any sum or maximum below.  Haplotypes are indexed within their window; a window with more
 * than 64 is GQ_E_CAPACITY naming the window (the carrier sets are 64-bit masks), nothing is truncated
 * and *out is not written.  A usable haplotype's CIGAR must hold only = (7) X (8) I (1) D (2) ops of
 * length >= 1 that consume exactly win_len window bytes and the haplotype's bytes, else GQ_E_ARG.
 * Events of a usable haplotype.  Walk its CIGAR from window offset 0 and haplotype offset 0.  X of
 * length L: L SNV events, one per base, REF the window byte, ALT the haplotype byte.  I of length L at
 * window offset p: left-normalised first: while the base just before the insertion is a matched (=)
 * base of this alignment and equals the insertion's last base, the insertion moves one base to the left
 * (the inserted bytes stay a substring of the haplotype, one to the left); a base under X, I or D stops
 * the shift.  An insertion then at offset 0 has no anchor: it is dropped, the window gets
 * GQ_HV_EDGE_DROPPED and n_edge_dropped counts it.  Otherwise the event stands at offset p - 1 with REF
 * the anchor byte (the window's) and ALT the anchor byte followed by the L inserted bytes.  D of length
 * L: left-normalised the same way, while the preceding matched base equals the last deleted base; the
 * same edge rule; the event stands at p - 1 with REF the L + 1 window bytes from the anchor and ALT the
 * anchor byte.  An event is (window offset, kind, ref_len, alt_len, ALT bytes).
 * Events of a window: the distinct events over its usable haplotypes, sorted by (window offset,
 * ref_len, alt_len, ALT bytes as unsigned bytes); carriers[e] has bit h set iff usable haplotype h made
 * event e; pos[e] = win_start[w] + offset, 0-based.  A window whose raw events (before dedup, dropped
 * ones not counted) exceed the cap gq_hapvar_limits reports gets GQ_HV_TOO_MANY_EVENTS and no events;
 * the host twin has no cap but applies the same flag at the same threshold.
 * Likelihoods of event e of window w with N reads in list order, H haplotypes, usable set U: C =
 * carriers[e], R = U \ C.  For read n alt[n] = the maximum of scaled[lik_off[w] + n * H + h] over h in C
 * and ref[n] the same over h in R, 0.0 when R is empty (the event then has GQ_HV_NO_REF_SIDE).  For the
 * genotypes 0/0, 0/1, 1/1 with (x, y) = (ref, ref), (ref, alt), (alt, alt):  gl = 0; for n ascending:
 * gl = gl + ((log(x + y) - log(INIT)) - log(2.0)), INIT = 2^1000, fdlibm's log, every operation rounded
 * on its own (Likelihood.likelihoodsOfGenotypes with a uniform prior, as the window genotypes above).
 * A read whose two values are both 0 makes the genotype -infinity; N == 0 gives three zeros.  best[e]
 * is the first largest of the three; ad_ref[e] counts reads with ref > alt, ad_alt[e] reads with alt >
 * ref, dp[e] = N.  Two events at one position are scored independently: the other ALT's carriers stand
 * on the REF side.                                                                               */
enum { GQ_HV_SNV = 0, GQ_HV_INS = 1, GQ_HV_DEL = 2 };
enum { GQ_HV_HAP_UNALIGNED = 1, GQ_HV_HAP_PARTIAL = 2 };             /* hap_flags */
enum { GQ_HV_EDGE_DROPPED = 1, GQ_HV_TOO_MANY_EVENTS = 2 };          /* win_flags */
enum { GQ_HV_NO_REF_SIDE = 1 };                                      /* ev_flags  */
typedef struct {
  int64_t n_windows, n_haplotypes, n_align;
  const int32_t *win_start;      /* [n_windows]                                                  */
  const uint8_t *ref_pool;
  const int64_t *ref_off;        /* [n_windows] < 0: the window has no reference bytes           */
  const int32_t *win_len;        /* [n_windows]                                                  */
  const int64_t *hap_off;        /* [n_windows + 1]                                              */
  const int64_t *hap_seq_off;    /* [n_haplotypes + 1] into bases                                */
  const uint8_t *bases;
  const int64_t *hap_align;      /* [n_haplotypes] into the four arrays below, or -1             */
  const int32_t *ref_start, *ref_end;  /* [n_align]                                              */
  const int64_t *cigar_off;      /* [n_align + 1] into cigar                                     */
  const uint32_t *cigar;
  const int64_t *win_read_off;   /* [n_windows + 1]                                              */
  const int64_t *lik_off;        /* [n_windows + 1]                                              */
  const double *scaled;
} gq_hapvar_input;
typedef struct {
  int64_t n_windows, n_events, n_haplotypes, n_alt_bases;
  int64_t *ev_off;               /* [n_windows + 1] a window's events, in the order above        */
  int64_t *pos;                  /* [n_events] 0-based contig coordinate                         */
  uint8_t *kind;                 /* [n_events] GQ_HV_SNV / INS / DEL                             */
  int32_t *ref_len;              /* [n_events] REF = the window's bytes from the event's offset  */
  int64_t *alt_off;              /* [n_events] into alt_bases                                    */
  int32_t *alt_len;              /* [n_events]                                                   */
  uint8_t *alt_bases;            /* [n_alt_bases]                                                */
  uint64_t *carriers;            /* [n_events]                                                   */
  double *gl;                    /* [3 * n_events] 0/0, 0/1, 1/1                                 */
  int32_t *best;                 /* [n_events]                                                   */
  int32_t *ad_ref, *ad_alt, *dp; /* [n_events]                                                   */
  uint8_t *ev_flags;             /* [n_events] GQ_HV_NO_REF_SIDE                                 */
  uint8_t *hap_flags;            /* [n_haplotypes]                                               */
  uint8_t *win_flags;            /* [n_windows]                                                  */
  int64_t n_edge_dropped;
  float ms;                      /* device span of the call, copies included (0: host twin)      */
  float events_ms;               /* ... of the event kernels, the count read-back included       */
  float marginal_ms;             /* ... of hv_marginal_k                                         */
  int32_t reserved;
  void *block_;                  /* owner of the arrays above (gq_hapvar_free_block)             */
} gq_hapvar_block;
#ifdef __cplusplus
static_assert(sizeof(gq_hapvar_input) == 144, "gq_hapvar_input layout");
static_assert(sizeof(gq_hapvar_block) == 192, "gq_hapvar_block layout");
#endif
/* out[0..7]: haplotypes a window may have (64), the raw-event cap of a window, threads per window of
 * the sort kernel, bytes of LDS its sort buffer takes, reads per pass of hv_marginal_k, 0, 0, 0    */
void gq_hapvar_limits(int32_t out[8]);
/* GQ_E_ARG on a null or negative argument, a window with a negative length or counts, a hap_align
 * outside [-1, n_align) or a CIGAR that does not fit (above).  n_windows == 0: an empty block.     */
gq_status gq_hapvar_windows(gq_ctx *ctx, const gq_hapvar_input *in, gq_hapvar_block **out);
/* The same block on the CPU (plain C++, no device), bit for bit; `threads` workers over the windows
 * (<= 1: the calling thread).                                                                      */
gq_status gq_hapvar_host(const gq_hapvar_input *in, int32_t threads, gq_hapvar_block **out);
void gq_hapvar_free_block(gq_hapvar_block *b);

#ifdef __cplusplus
}
#endif
#endif
