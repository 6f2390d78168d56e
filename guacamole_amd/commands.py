"""Caller commands over the GPU engine — the host mirror of the reference's plugin surface.

Reference surface (paths relative to /root/reference/src/main/scala/org/hammerlab/guacamole/):
  * command registry + args       Guacamole.scala:37-77, Command.scala:33-62, Common.scala:48-136
  * germline-threshold            commands/GermlineThresholdCaller.scala:40-88
        --threshold (8), --emit-ref, --emit-no-call, + --reads/--loci/--out/--parallelism/...
  * somatic-standard              commands/SomaticStandardCaller.scala:40-160
        --tumor-reads, --normal-reads, --odds (20), --min-mapq (1), --filter-multi-allelic, ...
  * loci partitioning             DistributedUtil.scala:55-69 (--parallelism, --partition-accuracy)

The per-locus work (pileupFlatMap + callVariantsAtLocus / findPotentialVariantAtLocus)
runs in libgqpileup on the GPU; this module only loads reads, builds LociSets and
partitions, and formats output.

Launched under torch.distributed.run (WORLD_SIZE > 1) the commands run one rank per GPU:
the reference's task partition is split into contiguous blocks of tasks per rank, each rank
uploads the reads overlapping its tasks' loci and calls its share, and rank 0 gathers the
records (over RCCL) and writes the output (distributed.py).
"""
from __future__ import annotations

import argparse
import json
import sys
import weakref
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import native, soa
from .distributed import (all_gather_objects, assign_tasks_to_ranks, device_ingest_ranks, gather_germline,
                          gather_somatic, init_from_env, rank_share, reads_overlapping)
from .loci import (LociSet, LociSetBuilder, flatten_partitions, partition_loci_by_approximate_depth,
                   partition_loci_uniformly)
from .bamdev import DeviceReadSet, load_reads_device, map_bams
from .reads import InputFilters, ReadSet, is_bam, load_reads

def device_reads(ctx: native.Context, rs: ReadSet) -> native.DeviceReads:
    """Upload a ReadSet once per context and keep it resident for as long as the ReadSet lives
    (the HBM copy is held by the ReadSet object itself and freed with it)."""
    cache = rs.__dict__.setdefault("_device", {})
    hit = cache.get(id(ctx))
    if hit is not None and hit[0]() is ctx:
        return hit[1]
    d = ctx.upload(soa.pack(rs))
    cache[id(ctx)] = (weakref.ref(ctx), d)
    return d


LAST_TIMING: Optional[Dict[str, object]] = None  # the last command's stage report in this process


class StageClock:
    """Wall time per stage of a command (GQ_TIMING=1: one JSON line on stderr at the end)."""

    def __init__(self):
        import os
        import time
        self.on = os.environ.get("GQ_TIMING") == "1"
        self.t = time.perf_counter
        self.t0 = self.last = self.t()
        self.stages: Dict[str, float] = {}
        # GQ_T_SPAWN (the launcher's time.time() at spawn): interpreter start + imports before the
        # command, and when the report is written (the rest of the launcher's wall time is exit)
        self.spawn = float(os.environ.get("GQ_T_SPAWN", "0") or 0)
        if self.spawn:
            self.stages["startup_s"] = time.time() - self.spawn

    def note(self, name: str, seconds: float) -> None:
        """A timed sub-step (inside some stage), reported beside the stages."""
        self.stages[name] = self.stages.get(name, 0.0) + seconds

    def mark(self, name: str) -> None:
        now = self.t()
        self.stages[name] = self.stages.get(name, 0.0) + (now - self.last)
        self.last = now

    def report(self, **extra) -> None:
        global LAST_TIMING
        LAST_TIMING = dict(self.stages, total_s=self.t() - self.t0, **extra)
        if self.on:
            import time
            at = {"report_at_s": time.time() - self.spawn} if self.spawn else {}
            print("GQ_TIMING " + json.dumps(dict(self.stages, total_s=self.t() - self.t0, **at, **extra)), file=sys.stderr)


def task_count(parallelism: int, world: int = 1) -> int:
    """`--parallelism` or, at 0, Spark's sc.defaultParallelism (DistributedUtil.scala:59).  The
    default parallelism of a Spark job is the number of its workers' cores; here it is the
    number of ranks (1 for a single process, N under torch.distributed.run with N GPUs).  So, as
    between Spark local[1] and local[N], a run with the default and a different rank count
    cuts the loci into different tasks, and the records at heap-order loci (the first pileup of
    every task) may differ; identical output across rank counts needs
    the same explicit --parallelism."""
    return parallelism if parallelism > 0 else max(1, world)


def partition(loci: LociSet, parallelism: int, accuracy: int, *read_sets: ReadSet, world: int = 1):
    """DistributedUtil.partitionLociAccordingToArgs (DistributedUtil.scala:55-69)."""
    tasks = task_count(parallelism, world)
    if accuracy == 0 or (tasks == 1 and loci.count > 0):
        # one task takes every locus whatever the depths are (the map is the same; the
        # read-region counts are only needed to cut loci between tasks)
        return partition_loci_uniformly(tasks, loci)
    return partition_loci_by_approximate_depth(tasks, loci, accuracy, *[r.regions() for r in read_sets])


def germline_threshold_reads(ctx: native.Context, rs: ReadSet, loci, threshold: int = 8, emit_ref: bool = False,
                             emit_no_call: bool = False) -> List[tuple]:
    """pileupFlatMap(reads, partitions, skipEmpty=true, callVariantsAtLocus) on the GPU.
    `loci` = flatten_partitions(...) arrays.  Rows: (contig, locus, sample, (gt0, gt1), ref, alt, flags)."""
    calls = ctx.germline_threshold(device_reads(ctx, rs), loci, threshold, emit_ref, emit_no_call)
    return calls.tuples(rs.contig_names)


def somatic_standard_reads(ctx: native.Context, tumor: ReadSet, normal: ReadSet, loci, _gather=None,
                           reference=None, _stats=None, _dref=None, **params) -> Optional[List[dict]]:
    """pileupFlatMapTwoRDDs(tumor, normal, partitions, skipEmpty=true, findPotentialVariantAtLocus,
    referenceGenome) + the driver's filters on the GPU.  Rows as the oracle's somatic_standard
    (contig by name).  reference: a reference.ReferenceGenome (--reference-fasta) or None.
    _gather: the gather device of a multi-GPU run (rank 0 gets every rank's rows, others None).
    _dref: that reference already resident for the read sets' contig list (the caller frees it);
    else it is uploaded for the call."""
    if tumor.contig_names != normal.contig_names:
        raise ValueError("tumor and normal reads must share the contig list")
    own = reference is not None and _dref is None
    dref = ctx.upload_reference(reference.for_contigs(tumor.contig_names)) if own else _dref
    try:
        calls = ctx.somatic_standard(device_reads(ctx, tumor), device_reads(ctx, normal), loci, reference=dref,
                                     **params)
    finally:
        if own:
            dref.free()
    if _stats is not None:
        _stats["visited_loci"] = int(calls.visited_loci)
    per_rank = [calls] if _gather is None else gather_somatic(calls, _gather)
    if per_rank is None:
        return None
    rows = []
    for c in per_rank:
        for r in c.rows:
            r = dict(r)
            r["contig"] = tumor.contig_names[r["contig"]]
            rows.append(r)
    return rows


# ---------------------------------------------------------------------------------------------
# CLI
def _common_args(p: argparse.ArgumentParser) -> None:
    """Common.Arguments (Common.scala:48-136): Base, Loci, NoSequenceDictionary,
    ReadLoadingConfigArgs, GenotypeOutput, DistributedUtil.Arguments."""
    p.add_argument("--debug", action="store_true", help="If set, prints a higher level of debug output.")
    p.add_argument("--no-sequence-dictionary", action="store_true",
                   help="If set, get contigs and lengths directly from reads instead of from sequence dictionary.")
    p.add_argument("--recompute-md-tags", action="store_true",
                   help="Use the reference fasta to recompute the MD Tags on all mapped reads")
    p.add_argument("--bam-reader-api", default="best", help="(accepted; the native reader is always used)")
    p.add_argument("--out-chunks", type=int, default=1,
                   help="When writing out to json format, number of chunks to coalesce the genotypes into.")
    p.add_argument("--max-genotypes", type=int, default=0,
                   help="Maximum number of genotypes to output. 0 (default) means output all genotypes.")
    p.add_argument("--loci", default="", help="Loci at which to call variants (e.g. 'all', 'chr1:0-1000,chr2')")
    p.add_argument("--loci-from-file", default="", help="Path to file giving loci")
    p.add_argument("--out", default="",
                   help="Output path: .json (or empty: stdout) Avro-JSON, .vcf a VCF directory, else ADAM Parquet")
    p.add_argument("--parallelism", type=int, default=0, help="Num variant calling tasks (loci partitions)")
    p.add_argument("--partition-accuracy", type=int, default=250,
                   help="Num micro partitions per task in loci partitioning; 0 = uniform")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    # ParquetArgs (bdg-utils cli; Common.scala:50): the options of the ADAM Parquet output
    p.add_argument("-parquet_block_size", type=int, default=128 * 1024 * 1024, help="Parquet block size (default = 128mb)")
    p.add_argument("-parquet_page_size", type=int, default=1 * 1024 * 1024, help="Parquet page size (default = 1mb)")
    p.add_argument("-parquet_compression_codec", default="GZIP", type=str.upper, help="Parquet compression codec")
    p.add_argument("-parquet_disable_dictionary", action="store_true", help="Disable dictionary encoding")
    p.add_argument("-parquet_logging_level", default="SEVERE", help="Parquet logging level (default = severe)")


def _loci_builder(args) -> LociSetBuilder:
    """Common.loci (Common.scala:223-239)."""
    if args.loci and args.loci_from_file:
        raise ValueError("Specify at most one of the 'loci' and 'loci-from-file' arguments")
    if args.loci:
        return LociSet.parse(args.loci)
    if args.loci_from_file:
        with open(args.loci_from_file) as fh:
            return LociSet.parse(fh.read())
    return LociSet.parse("all")


class OutputFormatError(ValueError):
    """An --out path the reference would write in a format this build does not produce."""


def _write_genotypes(path: str, genotypes: List[dict], contig_lengths=None, max_genotypes: int = 0,
                     parquet: Optional[dict] = None) -> None:
    """Common.writeVariantsFromArguments (Common.scala:246-304), by the path's extension
    (lower-cased, after stripMargin):
      * "" or .json: Avro-JSON, serially, to stdout or to the file (overwritten, :254-289);
      * .vcf: toVariantContext.coalesce(1).saveAsVcf (:290-293), a Hadoop output DIRECTORY
        holding one part-r-00000 and the committer's _SUCCESS marker (README.md:49-51); an
        existing path is refused, as Hadoop's checkOutputSpecs refuses it;
      * anything else: adamParquetSave (:294-302): a Hadoop output directory of Parquet part
        files, one per loci task (output.write_parquet_dir).  parquet: ParquetArgs (codec,
        page_size, block_size, dictionary) and the records' task ids (part_of, n_parts).
    --max-genotypes reaches RDD.sample(false, maxGenotypes, 0) as the sampling FRACTION
    (Common.scala:247-249): 1 keeps every genotype, larger values are refused by Spark's
    Bernoulli sampler ("must be on interval [0, 1]"), as here.  --out-chunks only coalesces
    partitions (order-preserving), so it does not change what is written."""
    from .output import write_json, write_parquet_dir, write_vcf_dir
    check_output_path(path)
    if max_genotypes > 1:
        raise ValueError("Sampling fraction (%s) must be on interval [0, 1]" % float(max_genotypes))
    kind = output_kind(path)
    if kind == "vcf":
        write_vcf_dir(path, genotypes, contig_lengths)
    elif kind == "parquet":
        write_parquet_dir(path, genotypes, **(parquet or {}))
    else:
        write_json(path, genotypes)


def output_kind(path: str) -> str:
    """"json", "vcf" or "parquet" (Common.scala:253-302)."""
    low = path.lower()
    if path == "" or low.endswith(".json"):
        return "json"
    return "vcf" if low.endswith(".vcf") else "parquet"


def check_output_path(path: str, codec: str = "GZIP") -> None:
    """Refuse, before any work, an output directory (VCF or Parquet) that already exists, as
    Hadoop's FileOutputFormat.checkOutputSpecs does (Common.scala:290, 294), and a Parquet codec
    this build cannot write."""
    import os
    from .output import PARQUET_CODECS
    kind = output_kind(path)
    if kind == "json":
        return
    if os.path.exists(path):
        raise OutputFormatError("Output directory %s already exists" % path)
    if kind == "parquet" and codec not in PARQUET_CODECS:
        raise OutputFormatError("-parquet_compression_codec %s: this build writes %s" % (codec, ", ".join(
            sorted(PARQUET_CODECS))))


def _all_flat(mine):
    """Every rank's flattened loci ranges (rank order = task order), on every rank."""
    got = all_gather_objects([np.asarray(a) for a in mine])
    return tuple(np.concatenate([g[k] for g in got]) for k in range(4))


def parquet_options(args, flat=None, contig_index=None, rows_contig=None, rows_pos=None) -> dict:
    """ParquetArgs (bdg-utils cli, mixed into Common.Arguments.Base, Common.scala:50) and the part
    file of each record: the loci task whose range holds it (flat = flatten_partitions arrays),
    since the callers' genotypes RDD has one partition per task.

    Divergence (parity unpinned, no fixture covers it): after --dbsnp-vcf the reference's
    keyBy + leftOuterJoin (SomaticStandardCaller.scala:143-144) reshuffles the records under a
    hash partitioner before adamParquetSave, so its record-to-part mapping is the join's, not
    the loci tasks'.  Here the parts stay per loci task in that case too; the records and their
    order within the whole output are the same, only which part file holds a record differs."""
    opts = dict(codec=args.parquet_compression_codec, page_size=args.parquet_page_size,
                block_size=args.parquet_block_size, dictionary=not args.parquet_disable_dictionary)
    if flat is not None and rows_pos is not None:
        contig, start, end, task = (np.asarray(a, np.int64) for a in flat)
        part = np.zeros(len(rows_pos), np.int64)
        if len(rows_pos) and len(task):
            key = contig * (1 << 40) + start  # ranges sorted by (contig, start) within the key space
            o = np.argsort(key, kind="stable")
            rk = np.asarray([contig_index[c] for c in rows_contig], np.int64) * (1 << 40) + np.asarray(rows_pos,
                                                                                                       np.int64)
            i = np.clip(np.searchsorted(key[o], rk, "right") - 1, 0, len(o) - 1)
            part = task[o][i]
        opts.update(part_of=part, n_parts=int(task.max()) + 1 if len(task) else 1)
    return opts


def device_ingest(args, *paths: str) -> bool:
    """Decode these BAMs on the GPU (bamdev.load_reads_device) rather than with the host
    loader: BAM input with contig lengths from the sequence dictionary (GQ_INGEST=host forces
    the host loader).  With --reference-fasta the device load rebuilds MD events from the
    resident reference (Context.rebuild_md), for the reads without a tag or, with
    --recompute-md-tags, for every read; --recompute-md-tags without a FASTA stays with the
    host loader, which refuses it.  Under torch.distributed.run each rank decodes only the part
    of the file its tasks need (distributed.device_ingest_ranks); multi-rank runs with a
    reference keep the host loader (a device ingest with a reference across ranks is not
    built)."""
    import os
    if os.environ.get("GQ_INGEST", "device") == "host":
        return False
    if getattr(args, "no_sequence_dictionary", False):
        return False
    has_ref = bool(getattr(args, "reference_fasta", ""))
    if getattr(args, "recompute_md_tags", False) and not has_ref:
        return False
    if has_ref:
        from .distributed import rank_info
        if rank_info()[1] > 1:
            return False
    return all(is_bam(p) for p in paths)


def load_pair_device(ctx, ctx2, paths, filters, mapped, reference=None, recompute_md=False, drefs=(None, None)):
    """Two BAMs decoded on the device at once: the second on ctx2 (its own stream) on a host
    thread while the first loads on ctx, so one's copy overlaps the other's inflate (ctypes
    releases the GIL).  The second read set is then registered with ctx (device pointers are
    valid across contexts of one device) and keeps ctx2 alive.  reference / recompute_md /
    drefs (each file's resident reference, or None): load_reads_device's."""
    import threading
    import weakref
    box = {}

    def second():
        try:
            box["rs"] = load_reads_device(ctx2, paths[1], filters, mapped[paths[1]], reference=reference,
                                          recompute_md=recompute_md, dref=drefs[1])
        except BaseException as e:  # re-raised below
            box["err"] = e
    th = threading.Thread(target=second)
    th.start()
    try:
        first = load_reads_device(ctx, paths[0], filters, mapped[paths[0]], reference=reference,
                                  recompute_md=recompute_md, dref=drefs[0])
    finally:
        th.join()
    if "err" in box:
        raise box["err"]
    rs = box["rs"]
    if rs is not None:
        rs._device[id(ctx)] = (weakref.ref(ctx), rs.reads)
        rs._ctx2 = ctx2
    return [first, rs]


def resident_references(ctx, reference, mapped, paths):
    """The reference resident once for BAMs that share a contig list: per path the handle
    (Context.upload_reference over that file's header contigs) or None where the file is not
    mapped for the device load; files with equal contig lists share one handle.  Returns
    (handles per path, [(contig names, handle)])."""
    made = []
    out = []
    for path in paths:
        m = mapped.get(path)
        if reference is None or m is None or not m.ok or not m.h:
            out.append(None)
            continue
        names = m.contigs()[0]
        hit = next((h for nm, h in made if nm == names), None)
        if hit is None:
            hit = ctx.upload_reference(reference.for_contigs(names))
            made.append((names, hit))
        out.append(hit)
    return out, made


def load_product_reads(args, filters, *paths):
    """The load block the CSV products share (allele-evidence, genotype-likelihoods,
    pileup-elements, pileup-counts, somatic-likelihoods): the device ingest where it applies
    (two files: load_pair_device), else the host loader.  --reference-fasta supplies MD tags by
    Read.fromSAMRecord's rule (reads without one, or every read with --recompute-md-tags) in
    both loaders; the pileups' reference base stays the MD-derived one.  Returns (the context or
    None if none was opened, the read sets)."""
    reference = None
    if getattr(args, "reference_fasta", ""):
        from .reference import ReferenceGenome
        reference = ReferenceGenome.load_fasta(args.reference_fasta)
    ctx = None
    sets = [None] * len(paths)
    if device_ingest(args, *paths):
        maps = map_bams(list(paths))  # the files mapped on a host thread while the context starts
        ctx = native.Context(args.device)
        ctx2 = native.Context(args.device) if len(paths) == 2 else None  # (the second load's own stream)
        mapped = maps["join"]()
        drefs, made = resident_references(ctx, reference, mapped, paths)
        try:
            if len(paths) == 2:
                sets = load_pair_device(ctx, ctx2, list(paths), filters, mapped, reference, args.recompute_md_tags,
                                        drefs)
            else:
                sets = [load_reads_device(ctx, paths[0], filters, mapped[paths[0]], reference=reference,
                                          recompute_md=args.recompute_md_tags, dref=drefs[0])]
        finally:
            for _, h in made:
                h.free()
    sets = [s if s is not None else load_reads(path, filters, reference=reference, recompute_md=args.recompute_md_tags)
            for s, path in zip(sets, paths)]
    return ctx, sets


def germline_threshold_main(argv: Sequence[str]) -> int:
    p = argparse.ArgumentParser(prog="germline-threshold",
                                description="call variants by thresholding read counts (toy example)")
    p.add_argument("--reads", required=True)
    p.add_argument("--threshold", type=int, default=8, help="Make a call if at least X%% of reads support it")
    p.add_argument("--emit-ref", action="store_true", help="Output homozygous reference calls.")
    p.add_argument("--emit-no-call", action="store_true", help="Output no call calls.")
    _common_args(p)
    args = p.parse_args(argv)
    clock = StageClock()
    check_output_path(args.out, args.parquet_compression_codec)
    rank, world, local, gdev = init_from_env()
    warn_default_parallelism(args, world)
    builder = _loci_builder(args)
    # germline-threshold takes no reference (GermlineThresholdCaller.scala:64-70): with
    # --recompute-md-tags read loading fails (Read.scala:223-225)
    filters = InputFilters.make(overlaps_loci=builder, non_duplicate=True, has_md_tag=True)
    ctx = None
    rs = None
    mine = None  # this rank's loci ranges, when the device ingest planned them
    if device_ingest(args, args.reads):
        if world == 1:
            maps = map_bams([args.reads])  # the file mapped on a host thread while the context starts
            t = clock.t()
            ctx = native.Context(args.device)
            clock.note("ctx_open_s", clock.t() - t)
            rs = load_reads_device(ctx, args.reads, filters, maps["join"]()[args.reads])
        else:
            ctx = native.Context(local)
            got = device_ingest_ranks(ctx, [args.reads], filters, builder, args.parallelism, args.partition_accuracy,
                                      rank, world, gdev)
            if got is not None:
                (rs,), mine, _ = got
    if rs is None:
        rs = load_reads(args.reads, filters, recompute_md=args.recompute_md_tags,
                        contig_lengths_from_dictionary=not args.no_sequence_dictionary)
    clock.mark("load_reads")
    loci = builder.result(rs.contig_lengths_map)
    if mine is None:
        parts = partition(loci, args.parallelism, args.partition_accuracy, rs, world=world)
        flat = flatten_partitions(parts, rs.contig_index())
    clock.mark("partition")
    if ctx is None:
        ctx = native.Context(local if world > 1 else args.device)
    if world == 1:
        device_reads(ctx, rs)
        clock.mark("upload")
    names = rs.sample_names
    sample_name = lambda s: names[s] if s < len(names) else "default"  # noqa: E731
    if world > 1:
        if mine is None:
            rr = assign_tasks_to_ranks(flat, world, [rs], len(rs.contig_names))
            mine_rs, mine = rank_share(rs, flat, rr, rank)
        else:
            mine_rs = rs
        calls = ctx.germline_threshold_device(device_reads(ctx, mine_rs), mine, args.threshold, args.emit_ref,
                                              args.emit_no_call)
        t = clock.t()
        per_rank = gather_germline(calls, gdev)
        clock.note("gather_s", clock.t() - t)
        # each rank numbers its own samples (by first appearance in what it read): names travel
        rank_names = all_gather_objects(list(mine_rs.sample_names))
        flat = _all_flat(mine) if output_kind(args.out) == "parquet" else None
        if per_rank is None:
            clock.mark("call")
            clock.report(rank=rank, reads=int(mine_rs.n), loci=int(sum(np.asarray(mine[2]) - np.asarray(mine[1]))),
                         ingest="device" if isinstance(rs, DeviceReadSet) else "host",
                         device_ingest=getattr(rs, "timings", None))
            return _finish_rank(0)
        rows = [(c, l, nm[s] if s < len(nm) else "default", g, ref, alt, fl)
                for calls_r, nm in zip(per_rank, rank_names) for c, l, s, g, ref, alt, fl in calls_r.tuples(rs.contig_names)]
        sample_name = lambda s: s  # noqa: E731
    else:
        calls = ctx.germline_threshold(device_reads(ctx, rs), flat, args.threshold, args.emit_ref, args.emit_no_call)
        rows = None
    clock.mark("call")
    from .output import germline_genotype, write_vcf_dir_germline, write_vcf_dir_germline_calls
    if args.out.lower().endswith(".vcf") and args.max_genotypes <= 1:
        # the lines _write_genotypes writes for these records, without building the records
        if rows is None:
            write_vcf_dir_germline_calls(args.out, calls, rs.contig_names, sample_name, rs.contig_lengths_map)
        else:
            write_vcf_dir_germline(args.out, rows, sample_name, rs.contig_lengths_map)
    else:
        if rows is None:
            rows = calls.tuples(rs.contig_names)
        out = [germline_genotype(c, l, sample_name(s), gt, ref, alt) for c, l, s, gt, ref, alt, fl in rows]
        pq = None
        if output_kind(args.out) == "parquet":
            pq = parquet_options(args, flat, rs.contig_index(), [r[0] for r in rows], [r[1] for r in rows])
        _write_genotypes(args.out, out, rs.contig_lengths_map, args.max_genotypes, pq)
    clock.mark("write")
    n_out = len(rows) if rows is not None else len(calls)
    print("Called %d genotypes." % n_out, file=sys.stderr)
    clock.report(rank=rank, reads=int(mine_rs.n if world > 1 else rs.n), genotypes=n_out, loci=int(loci.count),
                 ingest="device" if isinstance(rs, DeviceReadSet) else "host",
                 device_ingest=getattr(rs, "timings", None))
    return _finish_rank(0)


def somatic_standard_main(argv: Sequence[str]) -> int:
    """SomaticStandard.Caller.run (commands/SomaticStandardCaller.scala:66-160)."""
    p = argparse.ArgumentParser(prog="somatic-standard",
                                description="call somatic variants using independent callers on tumor and normal")
    p.add_argument("--tumor-reads", required=True, help="Aligned reads: tumor")
    p.add_argument("--normal-reads", required=True, help="Aligned reads: normal")
    p.add_argument("--odds", type=int, default=20, help="Minimum log odds threshold for possible variant candidates")
    p.add_argument("--min-mapq", type=int, default=1, help="Minimum read mapping quality for a read (Phred-scaled)")
    p.add_argument("--filter-multi-allelic", action="store_true", help="Filter any pileups > 2 bases considered")
    p.add_argument("--min-edge-distance", type=int, default=0, help="(accepted and ignored, as in the reference)")
    p.add_argument("--min-likelihood", type=int, default=0)
    p.add_argument("--min-vaf", type=int, default=0)
    p.add_argument("--min-lod", type=int, default=0)
    p.add_argument("--min-average-mapping-quality", type=int, default=0)
    p.add_argument("--min-average-base-quality", type=int, default=0)
    p.add_argument("--min-tumor-read-depth", type=int, default=0)
    p.add_argument("--min-normal-read-depth", type=int, default=0)
    p.add_argument("--max-tumor-read-depth", type=int, default=2 ** 31 - 1)
    p.add_argument("--min-tumor-alternate-read-depth", type=int, default=0)
    p.add_argument("--max-median-mismatches", type=int, default=2 ** 31 - 1)
    p.add_argument("--reference-fasta", default="", help="Local path to a reference FASTA file")
    p.add_argument("--dbsnp-vcf", default="", help="VCF file to identify DBSNP variants")
    _common_args(p)
    args = p.parse_args(argv)
    clock = StageClock()
    check_output_path(args.out, args.parquet_compression_codec)
    rank, world, local, gdev = init_from_env()
    warn_default_parallelism(args, world)
    builder = _loci_builder(args)
    f = InputFilters.make(overlaps_loci=builder, non_duplicate=True, passed_vendor_quality_checks=True,
                          has_md_tag=True)
    reference = None
    if args.reference_fasta:  # SomaticStandardCaller.scala:75
        from .reference import ReferenceGenome
        reference = ReferenceGenome.load_fasta(args.reference_fasta)
    ctx = None
    sets = [None, None]
    made = []  # [(contig names, resident reference)] of the device loads
    mine = None  # this rank's loci ranges, when the device ingest planned them
    try:  # (the resident references are freed whatever the loads or the call raise)
        if device_ingest(args, args.tumor_reads, args.normal_reads):
            if world == 1:
                maps = map_bams([args.tumor_reads, args.normal_reads])
                t = clock.t()
                ctx = native.Context(args.device)
                ctx2 = native.Context(args.device)  # the normal's load: its own stream, alongside the tumor's
                clock.note("ctx_open_s", clock.t() - t)
                mapped = maps["join"]()
                # the reference goes to HBM once: the loads rebuild MD events from it, the call reads it
                drefs, made = resident_references(ctx, reference, mapped, [args.tumor_reads, args.normal_reads])
                sets = load_pair_device(ctx, ctx2, [args.tumor_reads, args.normal_reads], f, mapped, reference,
                                        args.recompute_md_tags, drefs)
            else:
                ctx = native.Context(local)
                got = device_ingest_ranks(ctx, [args.tumor_reads, args.normal_reads], f, builder, args.parallelism,
                                          args.partition_accuracy, rank, world, gdev)
                if got is not None:
                    sets, mine, _ = got
        tumor, normal = [s if s is not None else
                         load_reads(path, f, reference=reference, recompute_md=args.recompute_md_tags,
                                    contig_lengths_from_dictionary=not args.no_sequence_dictionary)
                         for s, path in zip(sets, (args.tumor_reads, args.normal_reads))]
        if tumor.contig_lengths_map != normal.contig_lengths_map:
            raise ValueError("Tumor and normal samples have different sequence dictionaries.")
        clock.mark("load_reads")
        loci = builder.result(normal.contig_lengths_map)
        if mine is None:
            parts = partition(loci, args.parallelism, args.partition_accuracy, tumor, normal, world=world)
            flat = flatten_partitions(parts, tumor.contig_index())
        else:
            flat = mine
        if ctx is None:
            ctx = native.Context(local if world > 1 else args.device)
        sample = tumor.sample_names[0] if tumor.sample_names else "default"
        if world > 1:
            if mine is None:
                rr = assign_tasks_to_ranks(flat, world, [tumor, normal], len(tumor.contig_names))
                tumor, flat = rank_share(tumor, flat, rr, rank)
                normal = normal.subset(reads_overlapping(normal, *flat[:3]))
            else:  # each rank read its own part: the first tumor sample of the lowest rank that has one
                sample = next((n[0] for n in all_gather_objects(list(tumor.sample_names)) if n), "default")
        stats: Dict[str, int] = {}
        all_flat = None
        if output_kind(args.out) == "parquet":  # every rank's tasks: the part file of each record
            all_flat = _all_flat(flat) if world > 1 else flat
        rows = somatic_standard_reads(
            ctx, tumor, normal, flat, odds=args.odds, min_mapq=args.min_mapq,
            filter_multi_allelic=int(args.filter_multi_allelic), max_read_depth=args.max_tumor_read_depth,
            min_tumor_read_depth=args.min_tumor_read_depth, max_tumor_read_depth=args.max_tumor_read_depth,
            min_normal_read_depth=args.min_normal_read_depth,
            min_tumor_alternate_read_depth=args.min_tumor_alternate_read_depth, min_lod=args.min_lod,
            min_likelihood=args.min_likelihood, min_vaf=args.min_vaf,
            min_average_mapping_quality=args.min_average_mapping_quality,
            min_average_base_quality=args.min_average_base_quality, max_median_mismatches=args.max_median_mismatches,
            apply_filters=1, _gather=gdev if world > 1 else None, reference=reference, _stats=stats,
            _dref=next((h for nm, h in made if nm == tumor.contig_names), None))
    finally:
        for _, h in made:
            h.free()
    clock.mark("call")
    report = dict(rank=rank, reads=[int(tumor.n), int(normal.n)], ingest="device" if isinstance(tumor, DeviceReadSet)
                  else "host", device_ingest=[getattr(x, "timings", None) for x in (tumor, normal)], **stats)
    if rows is None:
        clock.report(**report)
        return _finish_rank(0)
    if args.dbsnp_vcf:  # SomaticStandardCaller.scala:139-149
        from .output import dbsnp_join, read_dbsnp_vcf
        rows = dbsnp_join(rows, read_dbsnp_vcf(args.dbsnp_vcf))
    from .output import somatic_genotype
    out = [somatic_genotype(r["contig"], r, sample) for r in rows]
    pq = None
    if all_flat is not None:
        pq = parquet_options(args, all_flat, tumor.contig_index(), [r["contig"] for r in rows],
                             [r["locus"] for r in rows])
    _write_genotypes(args.out, out, tumor.contig_lengths_map, args.max_genotypes, pq)
    clock.mark("write")
    print("Called %d somatic genotypes." % len(out), file=sys.stderr)
    clock.report(genotypes=len(out), **report)
    return _finish_rank(0)


def variant_loci(vcf_path: str) -> LociSet:
    """LociSet.union of the variants' [start, end) (VariantSupport.scala:82-87) over ADAM's VCF
    variants (loadVariants: one Variant per ALT allele, start = POS - 1, end = start + len(REF))."""
    from .output import read_dbsnp_vcf
    b = LociSetBuilder()
    for v in read_dbsnp_vcf(vcf_path):
        b.put(v["contig"], v["start"], v["end"])
    return b.result()


def variant_support_reads(ctx: native.Context, rs: ReadSet, loci) -> List[tuple]:
    """pileupFlatMap(reads, partitions, skipEmpty=true, pileupToAlleleCounts) on the GPU
    (VariantSupport.scala:93-100, 110-118).  Rows (sample name, contig, locus, ref, alt, count,
    flags), in the loci's call order, a locus's alleles by (ref, alt)."""
    rows = ctx.variant_support(device_reads(ctx, rs), loci)
    return [(rs.sample_names[s] if s < len(rs.sample_names) else "default", rs.contig_names[c], l, ref, alt, n, f)
            for s, c, l, ref, alt, n, f in rows]


def variant_support_main(argv: Sequence[str]) -> int:
    """VariantSupport.Caller.run (commands/VariantSupport.scala:62-103): allele counts at each
    variant of --input-variant in every BAM; saveAsTextFile layout (one part file per BAM and
    task, lines "sample, contig, locus, ref, alt, count", AlleleCount.toString :58-60)."""
    import os
    p = argparse.ArgumentParser(prog="variant-support",
                                description="Find number of reads that support each variant across BAMs")
    p.add_argument("-v", "--input-variant", required=True, help="VCF of the variants")
    p.add_argument("-o", "--output", required=True, help="Output path for CSV")
    p.add_argument("bams", nargs="+", help="Retrieve read data from BAMs at each variant position")
    p.add_argument("--parallelism", type=int, default=0, help="Num variant calling tasks")
    p.add_argument("--partition-accuracy", type=int, default=250, help="(accepted; partitioning is uniform)")
    p.add_argument("--bam-reader-api", default="best", help="(accepted; the native reader is always used)")
    p.add_argument("--recompute-md-tags", action="store_true")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    args = p.parse_args(argv)
    single_process_only("variant-support")
    loci = variant_loci(args.input_variant)
    # partitionLociUniformly(args.parallelism, ...) takes the flag as given (VariantSupport.scala:89)
    parts = partition_loci_uniformly(args.parallelism, loci)
    ctx = native.Context(args.device)
    os.makedirs(args.output, exist_ok=False)
    tasks = args.parallelism
    for b, bam in enumerate(args.bams):
        rs = load_reads(bam, InputFilters(), recompute_md=args.recompute_md_tags, contig_lengths_from_dictionary=False)
        idx = rs.contig_index()
        contig, start, end, task = flatten_partitions(parts, {c: idx.get(c, -1) for c in loci.contigs})
        keep = contig >= 0  # contigs without reads hold no pileups
        flat = (contig[keep], start[keep], end[keep], task[keep])
        rows = variant_support_reads(ctx, rs, flat)
        # the task of each row: its loci range's
        by_task: Dict[int, List[str]] = {t: [] for t in range(tasks)}
        r = 0
        for sample, cname, locus, ref, alt, n, _ in rows:
            ci = idx[cname]
            while not (flat[0][r] == ci and flat[1][r] <= locus < flat[2][r]):
                r += 1
            by_task[int(flat[3][r])].append("%s, %s, %d, %s, %s, %d" % (sample, cname, locus, ref, alt, n))
        for t in range(tasks):
            with open(os.path.join(args.output, "part-%05d" % (b * tasks + t)), "w") as fh:
                fh.writelines(line + "\n" for line in by_task[t])
    open(os.path.join(args.output, "_SUCCESS"), "w").close()
    return 0


def germline_standard_reads(ctx: native.Context, rs: ReadSet, loci, **params) -> List[dict]:
    """pileupFlatMap(reads, partitions, skipEmpty=true, callVariantsAtLocus) + GenotypeFilter
    (commands/GermlineStandardCaller.scala:63-72) on the GPU.  Rows as somatic_standard_reads'
    (contig by name; sample = the sample slot; tumor = the allele's evidence)."""
    calls = ctx.germline_standard(device_reads(ctx, rs), loci, **params)
    rows = []
    for r in calls.rows:
        r = dict(r)
        r["contig"] = rs.contig_names[r["contig"]]
        rows.append(r)
    return rows


def germline_standard_main(argv: Sequence[str]) -> int:
    """GermlineStandard.Caller.run (commands/GermlineStandardCaller.scala:48-76).  The truth-set
    concordance report (--truth-genotypes) is outside the pileup path and refused."""
    p = argparse.ArgumentParser(prog="germline-standard",
                                description="call variants using a simple quality-based probability")
    p.add_argument("--reads", required=True)
    p.add_argument("--min-mapq", type=int, default=1, help="Minimum read mapping quality for a read (Phred-scaled)")
    p.add_argument("--min-read-depth", type=int, default=0, help="Minimum number of reads for a genotype call")
    p.add_argument("--max-read-depth", type=int, default=2 ** 31 - 1, help="Maximum number of reads for a genotype call")
    p.add_argument("--min-alternate-read-depth", type=int, default=0)
    p.add_argument("--min-likelihood", type=int, default=0, help="Minimum Phred-scaled likelihood. Default: 0 (off)")
    p.add_argument("--emit-ref", action="store_true", help="(accepted; callVariantsAtLocus is called without it)")
    p.add_argument("--filter-multi-allelic", action="store_true", help="(accepted, unused by this caller)")
    p.add_argument("--min-edge-distance", type=int, default=0, help="(accepted, unused by this caller)")
    p.add_argument("--debug-genotype-filters", action="store_true")
    p.add_argument("--truth-genotypes", default="", help="(concordance report: not supported)")
    _common_args(p)
    args = p.parse_args(argv)
    single_process_only("germline-standard")
    check_output_path(args.out, args.parquet_compression_codec)
    if args.truth_genotypes:
        raise ValueError("--truth-genotypes (concordance report) is not supported")
    builder = _loci_builder(args)
    rs = load_reads(args.reads, InputFilters.make(overlaps_loci=builder, non_duplicate=True, has_md_tag=True),
                    recompute_md=args.recompute_md_tags,
                    contig_lengths_from_dictionary=not args.no_sequence_dictionary)
    loci = builder.result(rs.contig_lengths_map)
    parts = partition(loci, args.parallelism, args.partition_accuracy, rs)
    flat = flatten_partitions(parts, rs.contig_index())
    ctx = native.Context(args.device)
    rows = germline_standard_reads(ctx, rs, flat, min_mapq=args.min_mapq, min_read_depth=args.min_read_depth,
                                   max_read_depth=args.max_read_depth,
                                   min_alternate_read_depth=args.min_alternate_read_depth,
                                   min_likelihood=args.min_likelihood, apply_filters=1)
    from .output import called_allele_genotype
    out = [called_allele_genotype(r["contig"], r, rs.sample_names[r["sample"]] if r["sample"] < len(rs.sample_names)
                                  else "default") for r in rows]
    pq = None
    if output_kind(args.out) == "parquet":
        pq = parquet_options(args, flat, rs.contig_index(), [r["contig"] for r in rows], [r["locus"] for r in rows])
    _write_genotypes(args.out, out, rs.contig_lengths_map, args.max_genotypes, pq)
    print("Called %d genotypes." % len(out), file=sys.stderr)
    return 0


def vaf_histogram_reads(ctx: native.Context, rs: ReadSet, loci, bins: int = 20, min_read_depth: int = 0,
                        min_vaf: int = 0) -> Dict[str, object]:
    """VAFHistogram.variantLociFromReads + generateVAFHistogram (commands/VAFHistogram.scala:
    188-229) on the GPU: {bin start: loci}, variant and visited locus counts."""
    return ctx.vaf_histogram(device_reads(ctx, rs), loci, bins, min_read_depth, min_vaf)


def vaf_histogram_main(argv: Sequence[str]) -> int:
    """VAFHistogram.Caller.run (commands/VAFHistogram.scala:89-184).  The Gaussian mixture fit
    (--cluster, Spark MLlib) is outside the pileup path and refused."""
    import os
    p = argparse.ArgumentParser(prog="vaf-histogram", description="Compute and cluster the variant allele frequencies")
    p.add_argument("bams", nargs="+", help="BAMs")
    p.add_argument("--loci", default="", help="Loci at which to compute VAFs")
    p.add_argument("--loci-from-file", default="", help="Path to file giving loci")
    p.add_argument("--out", default="", help="Path to save the histogram (saveAsTextFile layout)")
    p.add_argument("--local-out", default="", help="Local file path to save the histogram")
    p.add_argument("--bins", type=int, default=20, help="Number of bins (Default: 20)")
    p.add_argument("--cluster", action="store_true", help="(Gaussian mixture model: not supported)")
    p.add_argument("--num-clusters", type=int, default=3)
    p.add_argument("--min-read-depth", type=int, default=0, help="Minimum read depth to include variant allele frequency")
    p.add_argument("--min-vaf", type=int, default=0, help="Minimum variant allele frequency to include")
    p.add_argument("--print-stats", action="store_true", help="(accepted; statistics are not printed)")
    p.add_argument("--sample-percent", type=int, default=25)
    p.add_argument("--parallelism", type=int, default=0, help="Num variant calling tasks (loci partitions)")
    p.add_argument("--partition-accuracy", type=int, default=250)
    p.add_argument("--bam-reader-api", default="best", help="(accepted; the native reader is always used)")
    p.add_argument("--recompute-md-tags", action="store_true")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    args = p.parse_args(argv)
    single_process_only("vaf-histogram")
    if args.out and args.local_out:
        raise ValueError("--out and --local-out are exclusive")
    if args.cluster:
        raise ValueError("--cluster (Gaussian mixture model over Spark MLlib) is not supported")
    builder = _loci_builder(args)
    # ReadSet(..., InputFilters.empty, contigLengthsFromDictionary = true) (:98-109)
    read_sets = [load_reads(b, InputFilters(), recompute_md=args.recompute_md_tags) for b in args.bams]
    rs0 = read_sets[0]
    loci = builder.result(rs0.contig_lengths_map)
    parts = partition(loci, args.parallelism, args.partition_accuracy, rs0)
    ctx = native.Context(args.device)
    bin_size = 100 // args.bins if 1 <= args.bins <= 100 else 1
    lines, plain = [], []
    for path, rs in zip(args.bams, read_sets):
        flat = flatten_partitions(parts, {c: rs.contig_index().get(c, -1) for c in loci.contigs})
        keep = flat[0] >= 0
        flat = tuple(a[keep] for a in flat)
        h = vaf_histogram_reads(ctx, rs, flat, args.bins, args.min_read_depth, args.min_vaf)["histogram"]
        sample = rs.sample_names[int(rs.sample[0])] if rs.n else "default"
        for b in sorted(h):
            row = "%d, %d, %d" % (b, min(b + bin_size, 100), h[b])
            lines.append("%s, %s, %s" % (path, sample, row))
            plain.append(row)
    if args.local_out:
        with open(args.local_out, "w") as fh:
            fh.write("Filename, SampleName, BinStart, BinEnd, Size\n")
            fh.writelines(l + "\n" for l in lines)
    elif args.out:
        os.makedirs(args.out, exist_ok=False)
        with open(os.path.join(args.out, "part-00000"), "w") as fh:
            fh.writelines(l + "\n" for l in lines)
        open(os.path.join(args.out, "_SUCCESS"), "w").close()
    else:
        for row in plain:
            print(row)
    return 0


def allele_evidence_reads(ctx: native.Context, rs: ReadSet, loci, **params) -> List[dict]:
    """AlleleEvidence (variants/AlleleEvidence.scala:58-101) of every distinct allele of every
    sample's pileup at the loci pileupFlatMap(reads, partitions, skipEmpty=true) visits
    (gq_allele_evidence).  params: min_mapq (1), variants_only (True).  Rows dict(contig (name),
    locus, sample (slot), ref, alt, evidence (native.EVIDENCE_FIELDS order), flags), loci in call
    order, samples ascending, a sample's alleles by (ref, alt)."""
    res = ctx.allele_evidence(device_reads(ctx, rs), loci, **params)
    rows = []
    for r in res.rows:
        r = dict(r)
        r["contig"] = rs.contig_names[r["contig"]]
        rows.append(r)
    return rows


ALLELE_EVIDENCE_HEADER = ("contig,locus,sample,ref,alt,readDepth,alleleReadDepth,forwardDepth,alleleForwardDepth,"
                          "meanMappingQuality,medianMappingQuality,meanBaseQuality,medianBaseQuality,"
                          "medianMismatchesPerRead,flags")


def write_allele_evidence_csv(path: str, rows: List[dict], sample_names: Sequence[str]) -> None:
    """The rows of allele_evidence_reads as CSV (ALLELE_EVIDENCE_HEADER): the sample by name, the
    nine evidence fields after the likelihood, doubles as repr() writes them (they read back to the
    same bits), NaN as "NaN".  Refuses an existing path."""
    def num(x) -> str:
        if isinstance(x, float):
            return "NaN" if x != x else repr(x)
        return str(x)
    with open(path, "x") as fh:
        fh.write(ALLELE_EVIDENCE_HEADER + "\n")
        for r in rows:
            s = r["sample"]
            name = sample_names[s] if s < len(sample_names) else "default"
            fh.write(",".join([r["contig"], str(r["locus"]), name, r["ref"], r["alt"]] +
                              [num(x) for x in r["evidence"][1:]] + [str(r["flags"])]) + "\n")


def allele_evidence_main(argv: Sequence[str]) -> int:
    """allele-evidence: the evidence table of every allele at every variant locus (--all-loci: at
    every visited locus) of one BAM, as CSV.  Input filters as germline-standard's
    (GermlineStandardCaller.scala:53-54)."""
    import os
    p = argparse.ArgumentParser(prog="allele-evidence",
                                description="per-allele evidence (depths, strand depths, mapping / base quality, "
                                            "mismatches) at every variant locus")
    p.add_argument("--reads", required=True)
    p.add_argument("--out", required=True, help="Output CSV path (must not exist)")
    p.add_argument("--loci", default="", help="Loci to visit (e.g. 'all', 'chr1:0-1000,chr2')")
    p.add_argument("--loci-from-file", default="", help="Path to file giving loci")
    p.add_argument("--min-mapq", type=int, default=1, help="Minimum read mapping quality for a read (Phred-scaled)")
    p.add_argument("--all-loci", action="store_true", help="Every visited locus, not only those with a non-Match element")
    p.add_argument("--parallelism", type=int, default=0, help="Num tasks (loci partitions)")
    p.add_argument("--partition-accuracy", type=int, default=250,
                   help="Num micro partitions per task in loci partitioning; 0 = uniform")
    p.add_argument("--recompute-md-tags", action="store_true")
    p.add_argument("--reference-fasta", default="",
                   help="Local path to a reference FASTA file: MD tags for reads without one (all reads with "
                        "--recompute-md-tags)")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    args = p.parse_args(argv)
    single_process_only("allele-evidence")
    if os.path.lexists(args.out):
        raise FileExistsError("Output path %s already exists" % args.out)
    builder = _loci_builder(args)
    filters = InputFilters.make(overlaps_loci=builder, mapped=True, non_duplicate=True, has_md_tag=True)
    ctx, (rs,) = load_product_reads(args, filters, args.reads)
    loci = builder.result(rs.contig_lengths_map)
    parts = partition(loci, args.parallelism, args.partition_accuracy, rs)
    flat = flatten_partitions(parts, rs.contig_index())
    if ctx is None:
        ctx = native.Context(args.device)
    rows = allele_evidence_reads(ctx, rs, flat, min_mapq=args.min_mapq, variants_only=not args.all_loci)
    write_allele_evidence_csv(args.out, rows, rs.sample_names)
    print("Wrote %d allele evidence rows." % len(rows), file=sys.stderr)
    return 0


def genotype_likelihoods_reads(ctx: native.Context, rs: ReadSet, loci, **params) -> List[dict]:
    """The log-likelihood of every diploid genotype over the eligible alleles of every sample's
    pileup (Likelihood.likelihoodsOfAllPossibleGenotypesFromPileup, Likelihood.scala:99-201,
    logSpace = true) at the loci pileupFlatMap(reads, partitions, skipEmpty=true) visits
    (gq_genotype_likelihoods_call).  params: min_mapq (1), variants_only (True), include_alignment
    (False), normalize (True).  Groups dict(contig (name), locus, sample (slot), depth, flags,
    alleles=[(ref, alt, depth)], log_likelihoods=[...]), loci in call order, samples ascending."""
    res = ctx.genotype_likelihoods(device_reads(ctx, rs), loci, **params)
    groups = []
    for g in res.groups:
        g = dict(g)
        g["contig"] = rs.contig_names[g["contig"]]
        groups.append(g)
    return groups


GENOTYPE_LIKELIHOODS_HEADER = "contig,locus,sample,ref1,alt1,ref2,alt2,depth,alleleDepth1,alleleDepth2,logLikelihood,flags"


def write_genotype_likelihoods_csv(path: str, groups: List[dict], sample_names: Sequence[str]) -> None:
    """The groups of genotype_likelihoods_reads as CSV (GENOTYPE_LIKELIHOODS_HEADER), one line per
    genotype: the sample by name, the log-likelihood as repr() writes it (it reads back to the same
    bits), NaN as "NaN", the infinities as "Infinity" / "-Infinity".  Refuses an existing path."""
    def num(x: float) -> str:
        if x != x:
            return "NaN"
        if x in (float("inf"), float("-inf")):
            return "Infinity" if x > 0 else "-Infinity"
        return repr(x)
    with open(path, "x") as fh:
        fh.write(GENOTYPE_LIKELIHOODS_HEADER + "\n")
        for g in groups:
            s = g["sample"]
            name = sample_names[s] if s < len(sample_names) else "default"
            al, n = g["alleles"], len(g["alleles"])
            head, tail = [g["contig"], str(g["locus"]), name], str(g["flags"])
            k = 0
            for i in range(n):
                for j in range(i, n):
                    fh.write(",".join(head + [al[i][0], al[i][1], al[j][0], al[j][1], str(g["depth"]), str(al[i][2]),
                                              str(al[j][2]), num(g["log_likelihoods"][k]), tail]) + "\n")
                    k += 1


def genotype_likelihoods_main(argv: Sequence[str]) -> int:
    """genotype-likelihoods: the log-likelihood of every diploid genotype at every variant locus
    (--all-loci: at every visited locus) of one BAM, as CSV.  Input filters as germline-standard's
    (GermlineStandardCaller.scala:53-54)."""
    import os
    p = argparse.ArgumentParser(prog="genotype-likelihoods",
                                description="log-likelihood of every diploid genotype over the alleles at every "
                                            "variant locus")
    p.add_argument("--reads", required=True)
    p.add_argument("--out", required=True, help="Output CSV path (must not exist)")
    p.add_argument("--loci", default="", help="Loci to visit (e.g. 'all', 'chr1:0-1000,chr2')")
    p.add_argument("--loci-from-file", default="", help="Path to file giving loci")
    p.add_argument("--min-mapq", type=int, default=1, help="Minimum read mapping quality for a read (Phred-scaled)")
    p.add_argument("--all-loci", action="store_true", help="Every visited locus, not only those with a non-Match element")
    p.add_argument("--include-alignment", action="store_true",
                   help="Probability correct = base quality x mapping quality (somatic-standard's choice)")
    p.add_argument("--raw", action="store_true", help="Log-likelihoods not normalized over the locus' genotypes")
    p.add_argument("--parallelism", type=int, default=0, help="Num tasks (loci partitions)")
    p.add_argument("--partition-accuracy", type=int, default=250,
                   help="Num micro partitions per task in loci partitioning; 0 = uniform")
    p.add_argument("--recompute-md-tags", action="store_true")
    p.add_argument("--reference-fasta", default="",
                   help="Local path to a reference FASTA file: MD tags for reads without one (all reads with "
                        "--recompute-md-tags)")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    args = p.parse_args(argv)
    single_process_only("genotype-likelihoods")
    if os.path.lexists(args.out):
        raise FileExistsError("Output path %s already exists" % args.out)
    builder = _loci_builder(args)
    filters = InputFilters.make(overlaps_loci=builder, mapped=True, non_duplicate=True, has_md_tag=True)
    ctx, (rs,) = load_product_reads(args, filters, args.reads)
    loci = builder.result(rs.contig_lengths_map)
    parts = partition(loci, args.parallelism, args.partition_accuracy, rs)
    flat = flatten_partitions(parts, rs.contig_index())
    if ctx is None:
        ctx = native.Context(args.device)
    groups = genotype_likelihoods_reads(ctx, rs, flat, min_mapq=args.min_mapq, variants_only=not args.all_loci,
                                        include_alignment=args.include_alignment, normalize=not args.raw)
    write_genotype_likelihoods_csv(args.out, groups, rs.sample_names)
    print("Wrote %d genotype likelihoods of %d (locus, sample) groups." %
          (sum(len(g["log_likelihoods"]) for g in groups), len(groups)), file=sys.stderr)
    return 0


def pileup_elements_reads(ctx: native.Context, rs: ReadSet, loci, **params) -> List[dict]:
    """The pileup itself (pileup/Pileup.scala:49-132) at the loci pileupFlatMap(reads, partitions,
    skipEmpty=true) visits (gq_pileup_elements_call).  params: min_mapq (1), variants_only (True).
    Groups dict(contig (name), locus, ref_base, flags, alleles=[(ref, alt, depth)] in Allele order,
    elements=[dict(read, sample, mapq, reverse, kind, allele, quality, read_position, cigar_index,
    index_within)] in Pileup.elements order), loci in call order; read indexes rs."""
    res = ctx.pileup_elements(device_reads(ctx, rs), loci, **params)
    groups = []
    for g in res.groups:
        g = dict(g)
        g["contig"] = rs.contig_names[g["contig"]]
        groups.append(g)
    return groups


PILEUP_ELEMENTS_HEADER = ("contig,locus,refBase,sample,readIndex,strand,mapq,kind,ref,alt,quality,readPosition,"
                          "cigarElementIndex,indexWithinCigarElement,flags")


def write_pileup_elements_csv(path: str, groups: List[dict], sample_names: Sequence[str]) -> None:
    """The groups of pileup_elements_reads as CSV (PILEUP_ELEMENTS_HEADER), one line per element in
    Pileup.elements order: the sample by name, the strand as + / -, the element's allele as its ref
    and alt bases.  Refuses an existing path."""
    with open(path, "x") as fh:
        fh.write(PILEUP_ELEMENTS_HEADER + "\n")
        for g in groups:
            head, tail, al = [g["contig"], str(g["locus"]), g["ref_base"]], str(g["flags"]), g["alleles"]
            for e in g["elements"]:
                s = e["sample"]
                name = sample_names[s] if s < len(sample_names) else "default"
                a = al[e["allele"]]
                fh.write(",".join(head + [name, str(e["read"]), "-" if e["reverse"] else "+", str(e["mapq"]), e["kind"],
                                          a[0], a[1], str(e["quality"]), str(e["read_position"]), str(e["cigar_index"]),
                                          str(e["index_within"]), tail]) + "\n")


def pileup_elements_main(argv: Sequence[str]) -> int:
    """pileup-elements: every element of the pileup at every variant locus (--all-loci: at every
    visited locus) of one BAM, as CSV.  Input filters as germline-standard's
    (GermlineStandardCaller.scala:53-54)."""
    import os
    p = argparse.ArgumentParser(prog="pileup-elements",
                                description="the pileup itself (read, strand, alignment kind, allele, quality, CIGAR "
                                            "cursor of every element) at every variant locus")
    p.add_argument("--reads", required=True)
    p.add_argument("--out", required=True, help="Output CSV path (must not exist)")
    p.add_argument("--loci", default="", help="Loci to visit (e.g. 'all', 'chr1:0-1000,chr2')")
    p.add_argument("--loci-from-file", default="", help="Path to file giving loci")
    p.add_argument("--min-mapq", type=int, default=1, help="Minimum read mapping quality for a read (Phred-scaled)")
    p.add_argument("--all-loci", action="store_true", help="Every visited locus, not only those with a non-Match element")
    p.add_argument("--parallelism", type=int, default=0, help="Num tasks (loci partitions)")
    p.add_argument("--partition-accuracy", type=int, default=250,
                   help="Num micro partitions per task in loci partitioning; 0 = uniform")
    p.add_argument("--recompute-md-tags", action="store_true")
    p.add_argument("--reference-fasta", default="",
                   help="Local path to a reference FASTA file: MD tags for reads without one (all reads with "
                        "--recompute-md-tags)")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    args = p.parse_args(argv)
    single_process_only("pileup-elements")
    if os.path.lexists(args.out):
        raise FileExistsError("Output path %s already exists" % args.out)
    builder = _loci_builder(args)
    filters = InputFilters.make(overlaps_loci=builder, mapped=True, non_duplicate=True, has_md_tag=True)
    ctx, (rs,) = load_product_reads(args, filters, args.reads)
    loci = builder.result(rs.contig_lengths_map)
    parts = partition(loci, args.parallelism, args.partition_accuracy, rs)
    flat = flatten_partitions(parts, rs.contig_index())
    if ctx is None:
        ctx = native.Context(args.device)
    groups = pileup_elements_reads(ctx, rs, flat, min_mapq=args.min_mapq, variants_only=not args.all_loci)
    write_pileup_elements_csv(args.out, groups, rs.sample_names)
    print("Wrote %d pileup elements of %d loci." % (sum(len(g["elements"]) for g in groups), len(groups)),
          file=sys.stderr)
    return 0


def somatic_likelihoods_reads(ctx: native.Context, tumor: ReadSet, normal: ReadSet, loci, **params) -> List[dict]:
    """What findPotentialVariantAtLocus (SomaticStandardCaller.scala:162-245) computes before it keeps
    one allele and applies --odds, at every locus pileupFlatMapTwoRDDs(tumor, normal, partitions,
    skipEmpty=true) visits where the caller's gate passes (gq_somatic_likelihoods_call).  params:
    min_mapq (1), filter_multi_allelic (False), max_read_depth (2**31 - 1).  Groups as
    native.SomaticLikelihoods.groups with the contig by name, loci in call order."""
    if tumor.contig_names != normal.contig_names:
        raise ValueError("tumor and normal reads must share the contig list")
    res = ctx.somatic_likelihoods(device_reads(ctx, tumor), device_reads(ctx, normal), loci, **params)
    groups = []
    for g in res.groups:
        g = dict(g)
        g["contig"] = tumor.contig_names[g["contig"]]
        groups.append(g)
    return groups


SOMATIC_LIKELIHOODS_HEADER = ("contig,locus,tumorRefBase,normalRefBase,tumorDepth,normalDepth,sample,genotype,ref1,alt1,"
                              "ref2,alt2,alleleDepth1,alleleDepth2,logLikelihood,best,hasVariant,normalVariantTotal,"
                              "logOdds,flags")


def write_somatic_likelihoods_csv(path: str, groups: List[dict]) -> None:
    """The groups of somatic_likelihoods_reads as CSV (SOMATIC_LIKELIHOODS_HEADER), one line per
    genotype: the tumor's genotypes then the normal's (`sample` says which, `genotype` is its index
    among that sample's), the group's best, hasVariant, normalVariantTotal and logOdds repeated on
    each line.  Doubles as repr() writes them (they read back to the same bits), NaN as "NaN", the
    infinities as "Infinity" / "-Infinity".  Refuses an existing path."""
    def num(x: float) -> str:
        if x != x:
            return "NaN"
        if x in (float("inf"), float("-inf")):
            return "Infinity" if x > 0 else "-Infinity"
        return repr(x)
    with open(path, "x") as fh:
        fh.write(SOMATIC_LIKELIHOODS_HEADER + "\n")
        for g in groups:
            head = [g["contig"], str(g["locus"]), g["tumor_ref_base"], g["normal_ref_base"], str(g["tumor_depth"]),
                    str(g["normal_depth"])]
            tail = [str(g["best"]), "1" if g["has_variant"] else "0", num(g["normal_variant_total"]), num(g["log_odds"]),
                    str(g["flags"])]
            for side in ("tumor", "normal"):
                al, ll = g[side + "_alleles"], g[side + "_log_likelihoods"]
                k = 0
                for i in range(len(al)):
                    for j in range(i, len(al)):
                        fh.write(",".join(head + [side, str(k), al[i][0], al[i][1], al[j][0], al[j][1], str(al[i][2]),
                                                  str(al[j][2]), num(ll[k])] + tail) + "\n")
                        k += 1


def somatic_likelihoods_main(argv: Sequence[str]) -> int:
    """somatic-likelihoods: both samples' genotype log-likelihoods, the most likely tumor genotype,
    the normal's variant mass and the somatic log-odds at every locus that passes somatic-standard's
    gate, as CSV.  Input filters as somatic-standard's (SomaticStandardCaller.scala:82-89)."""
    import os
    p = argparse.ArgumentParser(prog="somatic-likelihoods",
                                description="tumor / normal genotype log-likelihoods and somatic log-odds at every "
                                            "locus somatic-standard evaluates")
    p.add_argument("--tumor-reads", required=True, help="Aligned reads: tumor")
    p.add_argument("--normal-reads", required=True, help="Aligned reads: normal")
    p.add_argument("--out", required=True, help="Output CSV path (must not exist)")
    p.add_argument("--loci", default="", help="Loci to visit (e.g. 'all', 'chr1:0-1000,chr2')")
    p.add_argument("--loci-from-file", default="", help="Path to file giving loci")
    p.add_argument("--min-mapq", type=int, default=1, help="Minimum read mapping quality for a read (Phred-scaled)")
    p.add_argument("--filter-multi-allelic", action="store_true", help="Filter any pileups > 2 bases considered")
    p.add_argument("--max-read-depth", type=int, default=2 ** 31 - 1, help="Skip loci with a deeper filtered pileup")
    p.add_argument("--parallelism", type=int, default=0, help="Num tasks (loci partitions)")
    p.add_argument("--partition-accuracy", type=int, default=250,
                   help="Num micro partitions per task in loci partitioning; 0 = uniform")
    p.add_argument("--recompute-md-tags", action="store_true")
    p.add_argument("--reference-fasta", default="",
                   help="Local path to a reference FASTA file: MD tags for reads without one (all reads with "
                        "--recompute-md-tags)")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    args = p.parse_args(argv)
    single_process_only("somatic-likelihoods")
    if os.path.lexists(args.out):
        raise FileExistsError("Output path %s already exists" % args.out)
    builder = _loci_builder(args)
    f = InputFilters.make(overlaps_loci=builder, non_duplicate=True, passed_vendor_quality_checks=True,
                          has_md_tag=True)
    ctx, (tumor, normal) = load_product_reads(args, f, args.tumor_reads, args.normal_reads)
    if tumor.contig_lengths_map != normal.contig_lengths_map:
        raise ValueError("Tumor and normal samples have different sequence dictionaries.")
    loci = builder.result(normal.contig_lengths_map)
    parts = partition(loci, args.parallelism, args.partition_accuracy, tumor, normal)
    flat = flatten_partitions(parts, tumor.contig_index())
    if ctx is None:
        ctx = native.Context(args.device)
    groups = somatic_likelihoods_reads(ctx, tumor, normal, flat, min_mapq=args.min_mapq,
                                       filter_multi_allelic=args.filter_multi_allelic,
                                       max_read_depth=args.max_read_depth)
    write_somatic_likelihoods_csv(args.out, groups)
    print("Wrote %d genotype likelihoods of %d loci." %
          (sum(len(g["tumor_log_likelihoods"]) + len(g["normal_log_likelihoods"]) for g in groups), len(groups)),
          file=sys.stderr)
    return 0


def pileup_counts_reads(ctx: native.Context, rs: ReadSet, loci, chunk_loci: int = 0, **params):
    """The per-locus count table (gq_pileup_counts_call) at the loci pileupFlatMap(reads, partitions,
    skipEmpty=true) visits, all samples merged.  params: min_mapq (1), min_depth (1), variants_only
    (False).  -> native.PileupCounts: numpy columns in call order, ``contig`` indexing its
    ``contig_names`` (its ``rows`` give the name).  chunk_loci > 0: one library call per run of
    whole tasks (plan_count_chunks), the same rows."""
    dr = device_reads(ctx, rs)
    runs = plan_count_chunks(loci[1], loci[2], loci[3], chunk_loci) if chunk_loci > 0 else []
    res = native.PileupCounts.concat([ctx.pileup_counts_call(dr, tuple(a[lo:hi] for a in loci), **params)
                                      for lo, hi in runs or [(0, len(loci[3]))]])
    res.contig_names = list(rs.contig_names)
    return res


def plan_count_chunks(start, end, task, chunk_loci: int) -> List[tuple]:
    """Runs [lo, hi) of the flat loci ranges (flatten_partitions: task ascending), one per library
    call: each run is whole tasks whose loci sum to at most chunk_loci, in order; a task with more
    loci than that is a run of its own.  A task is never split: its first pileup defines its
    heap order, so a split would change the rows at heap-order loci."""
    runs: List[tuple] = []
    n = len(task)
    lo, total, k = 0, 0, 0
    while k < n:
        j, size = k, 0
        while j < n and task[j] == task[k]:
            size += int(end[j]) - int(start[j])
            j += 1
        if k > lo and total + size > chunk_loci:
            runs.append((lo, k))
            lo, total = k, 0
        total += size
        k = j
    if n > lo:
        runs.append((lo, n))
    return runs


PILEUP_COUNTS_HEADER = ("contig,locus,refBase,depth,forwardDepth,refDepth,A,C,G,T,N,other,forwardA,forwardC,forwardG,"
                        "forwardT,forwardN,forwardOther,insertions,deletions,midDeletions,clipped,flags")


def write_pileup_counts_csv(path: str, counts: "native.PileupCounts", contig_names: Optional[Sequence[str]] = None,
                            append: bool = False) -> None:
    """The rows of pileup_counts_reads as CSV (PILEUP_COUNTS_HEADER), formatted a column at a time.
    contig_names: the result's own when None.  Refuses an existing path; append=True adds a later
    call's rows to the file this function made (no header)."""
    c = counts.cols
    contig_names = counts.contig_names if contig_names is None else contig_names
    with open(path, "a" if append else "x") as fh:
        if not append:
            fh.write(PILEUP_COUNTS_HEADER + "\n")
        step = 1 << 20
        for lo in range(0, len(counts), step):
            sl = slice(lo, lo + step)
            names = np.asarray(list(contig_names), dtype=object)[c["contig"][sl]]
            cols = [names, c["pos"][sl].astype(str), c["ref_base"][sl].astype(np.uint8).view("S1").astype(str)]
            cols += [c[k][sl].astype(str) for k in ("depth", "forward_depth", "ref_depth")]
            for k in ("base_count", "base_forward", "kind_count"):
                cols += [c[k][sl, j].astype(str) for j in range(c[k].shape[1])]
            cols.append(c["flags"][sl].astype(str))
            fh.write("".join(",".join(r) + "\n" for r in zip(*cols)))


def pileup_counts_main(argv: Sequence[str]) -> int:
    """pileup-counts: depth, strand-split base counts and element-kind counts at every visited locus
    of one BAM, as CSV.  Input filters as germline-standard's (GermlineStandardCaller.scala:53-54)."""
    import os
    p = argparse.ArgumentParser(prog="pileup-counts",
                                description="per-locus depth, strand-split A/C/G/T/N/other counts and insertion / "
                                            "deletion / mid-deletion / clipped counts")
    p.add_argument("--reads", required=True)
    p.add_argument("--out", required=True, help="Output CSV path (must not exist)")
    p.add_argument("--loci", default="", help="Loci to visit (e.g. 'all', 'chr1:0-1000,chr2')")
    p.add_argument("--loci-from-file", default="", help="Path to file giving loci")
    p.add_argument("--min-mapq", type=int, default=1, help="Minimum read mapping quality for a read (Phred-scaled)")
    p.add_argument("--min-depth", type=int, default=1, help="Only loci with at least this many kept elements")
    p.add_argument("--variants-only", action="store_true", help="Only loci with a non-Match element after the filter")
    p.add_argument("--parallelism", type=int, default=0, help="Num tasks (loci partitions)")
    p.add_argument("--partition-accuracy", type=int, default=250,
                   help="Num micro partitions per task in loci partitioning; 0 = uniform")
    p.add_argument("--recompute-md-tags", action="store_true")
    p.add_argument("--reference-fasta", default="",
                   help="Local path to a reference FASTA file: MD tags for reads without one (all reads with "
                        "--recompute-md-tags)")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    p.add_argument("--chunk-loci", type=int, default=1 << 24,
                   help="Loci per library call (whole tasks; a larger task goes alone)")
    args = p.parse_args(argv)
    single_process_only("pileup-counts")
    if os.path.lexists(args.out):
        raise FileExistsError("Output path %s already exists" % args.out)
    if args.chunk_loci < 1:
        raise ValueError("--chunk-loci must be at least 1")
    builder = _loci_builder(args)
    filters = InputFilters.make(overlaps_loci=builder, mapped=True, non_duplicate=True, has_md_tag=True)
    ctx, (rs,) = load_product_reads(args, filters, args.reads)
    loci = builder.result(rs.contig_lengths_map)
    parts = partition(loci, args.parallelism, args.partition_accuracy, rs)
    flat = flatten_partitions(parts, rs.contig_index())
    if ctx is None:
        ctx = native.Context(args.device)
    dr = device_reads(ctx, rs)
    n_rows, first = 0, True
    for lo, hi in plan_count_chunks(flat[1], flat[2], flat[3], args.chunk_loci) or [(0, len(flat[3]))]:
        res = ctx.pileup_counts_call(dr, tuple(a[lo:hi] for a in flat), min_mapq=args.min_mapq,
                                     min_depth=args.min_depth, variants_only=args.variants_only)
        write_pileup_counts_csv(args.out, res, rs.contig_names, append=not first)
        n_rows, first = n_rows + len(res), False
    print("Wrote %d pileup count rows." % n_rows, file=sys.stderr)
    return 0


ACTIVE_OPTIONS = (("min_mapq", "Minimum read mapping quality for the evidence pileup"),
                  ("min_depth", "Minimum filtered depth of an active locus"),
                  ("min_evidence", "Minimum non-reference A/C/G/T, insertion and deletion elements at an active locus"),
                  ("min_percent", "Minimum share of the depth the evidence must reach, in percent"),
                  ("pad", "Loci added on each side of an active locus"))


def _active_options(p: argparse.ArgumentParser, prefix: str = "") -> None:
    for name, text in ACTIVE_OPTIONS:
        p.add_argument("--%s%s" % (prefix, name.replace("_", "-")), type=int, default=native.ACTIVE_DEFAULTS[name],
                       dest="active_" + name, help=text)


def _active_params(args) -> dict:
    prm = {name: getattr(args, "active_" + name) for name, _ in ACTIVE_OPTIONS}
    if prm["pad"] < 0:
        raise ValueError("the active-region pad must not be negative")
    if not 0 <= prm["min_percent"] <= 100:
        raise ValueError("the active-region percent must lie in 0..100")
    return prm


def active_regions_main(argv: Sequence[str]) -> int:
    """active-regions: the regions of the loci where the pileup shows evidence of a variant
    (gq_active_regions_call), as TSV: contig, start, end, n_active, evidence."""
    import os
    from . import active
    p = argparse.ArgumentParser(prog="active-regions",
                                description="regions around the loci whose pileup shows non-reference evidence")
    p.add_argument("--reads", required=True)
    p.add_argument("--out", required=True, help="Output TSV path of the regions (must not exist)")
    p.add_argument("--out-loci", default="", help="Also write one TSV row per active locus: contig, locus, depth, evidence")
    p.add_argument("--loci", default="all", help="Loci to search (e.g. 'all', 'chr1:0-1000,chr2')")
    p.add_argument("--loci-from-file", default="", help="Path to file giving loci")
    _active_options(p)
    p.add_argument("--parallelism", type=int, default=0, help="Num tasks (loci partitions)")
    p.add_argument("--partition-accuracy", type=int, default=250,
                   help="Num micro partitions per task in loci partitioning; 0 = uniform")
    p.add_argument("--recompute-md-tags", action="store_true")
    p.add_argument("--reference-fasta", default="",
                   help="Local path to a reference FASTA file: MD tags for reads without one (all reads with "
                        "--recompute-md-tags)")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    p.add_argument("--chunk-loci", type=int, default=1 << 24,
                   help="Loci per library call (whole tasks; a larger task goes alone)")
    args = p.parse_args(argv)
    single_process_only("active-regions")
    for path in (args.out, args.out_loci):
        if path and os.path.lexists(path):
            raise FileExistsError("Output path %s already exists" % path)
    if args.chunk_loci < 1:
        raise ValueError("--chunk-loci must be at least 1")
    prm = _active_params(args)
    builder = _loci_builder(args)
    filters = InputFilters.make(overlaps_loci=builder, mapped=True, non_duplicate=True, has_md_tag=True)
    ctx, (rs,) = load_product_reads(args, filters, args.reads)
    loci = builder.result(rs.contig_lengths_map)
    flat = flatten_partitions(partition(loci, args.parallelism, args.partition_accuracy, rs), rs.contig_index())
    if ctx is None:
        ctx = native.Context(args.device)
    found: list = []
    info: dict = {}
    regions = active.find_regions(ctx, device_reads(ctx, rs), flat, chunk_loci=args.chunk_loci, loci_out=found, info=info,
                                  **prm)
    names, lengths = list(rs.contig_names), dict(rs.contig_lengths_map)
    active.write_tsv(args.out, active.named(regions, names), lengths)
    if args.out_loci:
        active.write_loci_tsv(args.out_loci, active.named(found, names))
    print("Wrote %d active regions of %d active loci (%d loci visited)." % (len(regions), len(found), info["visited_loci"]),
          file=sys.stderr)
    return 0


def active_windows(args, ctx, dr, dref, rs, loci: LociSet, clock: "StageClock", info: dict):
    """The windows of an assembly command under --active-regions: the regions found over `loci` (one
    task), cut by active.regions_to_windows in place of the grid.  The evidence pileup needs MD events:
    reads without them get theirs from the resident reference first (Context.rebuild_md)."""
    from . import active
    if ctx.missing_md(dr) > 0:
        ctx.rebuild_md(dr, dref)
    names = list(rs.contig_names)
    flat = flatten_partitions(partition_loci_uniformly(1, loci), rs.contig_index())
    regions = active.find_regions(ctx, dr, flat, info=info, **_active_params(args))
    windows = active.regions_to_windows(active.named(regions, names), dict(rs.contig_lengths_map), args.window_size,
                                        args.window_step or None, args.kmer_size)
    info["regions"] = len(regions)
    clock.mark("active_regions")
    return windows


def _active_report(info: dict) -> dict:
    """What the stage report gains under --active-regions (nothing without it)."""
    if not info:
        return {}
    return dict(regions=info["regions"], active_loci=info["active_loci"], active_ms=info["total_ms"],
                active_staging_ms=info["staging_ms"], active_regions_ms=info["regions_ms"])


def _active_summary(info: dict) -> str:
    """What the summary line gains under --active-regions (nothing without it)."""
    return " The windows cover %d active regions of %d active loci." % (info["regions"], info["active_loci"]) if info else ""


def warn_default_parallelism(args, world: int) -> None:
    """--parallelism 0 means one task per rank (task_count): the records at heap-order loci then
    depend on the rank count, so say so when a multi-rank run takes the default."""
    if world > 1 and args.parallelism == 0:
        import os
        if int(os.environ.get("RANK", "0")) == 0:
            print("warning: --parallelism 0 makes %d tasks (one per rank); the records at heap-order loci (the first "
                  "pileup of each task) can then differ from a run with another rank count. Pass the same explicit "
                  "--parallelism to compare runs." % world, file=sys.stderr)


def single_process_only(command: str) -> None:
    """germline-standard, variant-support, vaf-histogram, allele-evidence, genotype-likelihoods,
    pileup-elements, somatic-likelihoods and pileup-counts run as one process on --device: under torch.distributed.run
    every rank would repeat the whole job and write the same output, so a multi-rank launch is refused."""
    import os
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise RuntimeError("%s runs as a single process (WORLD_SIZE=%s): launch it without torch.distributed.run "
                           "and pick the GPU with --device" % (command, os.environ["WORLD_SIZE"]))


def _finish_rank(rc: int) -> int:
    """Leave the process group (multi-GPU runs) after every rank has finished."""
    import os
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch.distributed as dist
        from . import distributed
        if dist.is_initialized():
            dist.barrier()
            if distributed.OWN_GROUP:
                dist.destroy_process_group()
                distributed.OWN_GROUP = False
    return rc


def structural_variant_main(argv: Sequence[str]) -> int:
    """StructuralVariant.Caller.run (commands/StructuralVariantCaller.scala:273-287): the ranges
    where discordant first-in-pair reads give evidence of a large deletion, one line per contig
    with an exceptional pair (saveAsTextFile layout)."""
    from . import structural
    p = argparse.ArgumentParser(prog="structural-variant", description="Find structural variants, e.g. large deletions.")
    p.add_argument("--reads", required=True, help="Aligned reads (BAM)")
    p.add_argument("--output", required=True, help="Path to output text file (a directory with part-00000)")
    p.add_argument("--filter-contig", default="", help="(accepted and ignored, as the reference's run never reads it)")
    p.add_argument("--out-tsv", default="", help="Also write contig, start, stop, pairs, wiggle per deletion")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    args = p.parse_args(argv)
    single_process_only("structural-variant")
    ctx = native.Context(args.device)
    res = structural.structural_variant(ctx, args.reads)
    s = res["stats"]
    print("insert stats: MedianStats(%r,%r)" % (s["median"], s["mad"]))
    structural.write_output(args.output, structural.text_lines(res["node_contigs"], res["cliques"],
                                                               res["contig_names"]))
    if args.out_tsv:
        with open(args.out_tsv, "w") as fh:
            fh.writelines(l + "\n" for l in structural.tsv_lines(res["cliques"], res["contig_names"]))
    return 0


def realign_reads_main(argv: Sequence[str]) -> int:
    """realign-reads: the reads with an insertion, deletion or soft clip aligned again against their
    reference windows (AffineGapPenaltyAlignment.align, alignment/AffineGapPenaltyAlignment.scala:
    20-46), one TSV line per selected read in resident order."""
    import os
    from . import align
    from .bamdev import download
    from .reference import ReferenceGenome
    p = argparse.ArgumentParser(prog="realign-reads",
                                description="affine-gap re-alignment of reads with indels or soft clips")
    p.add_argument("--reads", required=True, help="Aligned reads")
    p.add_argument("--reference-fasta", required=True, help="Local path to a reference FASTA file")
    p.add_argument("--out", required=True, help="Output TSV path (must not exist)")
    p.add_argument("--pad", type=int, default=32, help="Reference bases on each side of a read's window")
    p.add_argument("--all-reads", action="store_true", help="Align every read, not only those with I, D or S ops")
    p.add_argument("--mismatch-probability", type=float, default=None)
    p.add_argument("--open-gap-probability", type=float, default=None)
    p.add_argument("--close-gap-probability", type=float, default=None)
    p.add_argument("--min-mapq", type=int, default=1, help="Rows only for reads of at least this mapping quality")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    args = p.parse_args(argv)
    single_process_only("realign-reads")
    if os.path.lexists(args.out):
        raise FileExistsError("Output path %s already exists" % args.out)
    clock = StageClock()
    # the reads as stored: no MD tag is needed, so the load gets no reference (it would rebuild tags)
    load_args = argparse.Namespace(reference_fasta="", recompute_md_tags=False, device=args.device)
    ctx, (rs,) = load_product_reads(load_args, InputFilters.make(mapped=True, non_duplicate=True), args.reads)
    if ctx is None:
        ctx = native.Context(args.device)
    dr = device_reads(ctx, rs)
    clock.mark("load_reads")
    dref = ctx.upload_reference(ReferenceGenome.load_fasta(args.reference_fasta).for_contigs(list(rs.contig_names)))
    clock.mark("load_reference")
    try:
        res = align.realign_reads(ctx, dr, dref, pad=args.pad, all_reads=args.all_reads,
                                  mismatch_probability=args.mismatch_probability,
                                  open_gap_probability=args.open_gap_probability,
                                  close_gap_probability=args.close_gap_probability)
    finally:
        dref.free()
    clock.mark("align")
    host = download(dr)
    sel = res["read"]
    contig = np.searchsorted(host["contig_read_begin"], sel, side="right") - 1
    keep = host["mapq"][sel] >= args.min_mapq
    co, nc = host["cigar_off"][sel], host["n_cigar"][sel]
    lines = align.tsv_lines(res, [rs.contig_names[c] for c in contig], host["start"][sel],
                            [align.to_cigar_string(host["cigar"][a:a + k]) for a, k in zip(co, nc)])
    with open(args.out, "w") as fh:
        fh.write(align.TSV_HEADER + "\n")
        fh.writelines(l + "\n" for l, k in zip(lines, keep) if k)
    clock.mark("write")
    print("Aligned %d of %d reads (%d with N or P ops skipped); wrote %d rows." %
          (res["n"], res["n_reads"], res["skipped"], int(keep.sum())), file=sys.stderr)
    clock.report(selected=int(res["n"]), align_ms=res["ms"], kernel_ms=res["kernel_ms"])
    return 0


def assemble_windows_main(argv: Sequence[str]) -> int:
    """assemble-windows: the de Bruijn graph of the reads' k-mers per window (assembly/
    DeBruijnGraph.scala:271-294), its source-to-sink haplotypes and their alignment to the window,
    one TSV line per haplotype."""
    import os
    from . import assemble
    from .reference import ReferenceGenome
    p = argparse.ArgumentParser(prog="assemble-windows", description="local assembly of the reads over windows")
    p.add_argument("--reads", required=True, help="Aligned reads")
    p.add_argument("--reference-fasta", required=True, help="Local path to a reference FASTA file")
    p.add_argument("--loci", default="all", help="Loci to cut into windows (e.g. 'all', 'chr1:0-1000,chr2')")
    p.add_argument("--out", required=True, help="Output TSV path (must not exist)")
    p.add_argument("--kmer-size", type=int, default=25)
    p.add_argument("--min-occurrence", type=int, default=2, help="Occurrences a k-mer needs to be a node")
    p.add_argument("--window-size", type=int, default=200)
    p.add_argument("--window-step", type=int, default=0, help="Distance between window starts (default: the size)")
    p.add_argument("--max-paths", type=int, default=10)
    p.add_argument("--min-mapq", type=int, default=1, help="Only reads of at least this mapping quality")
    p.add_argument("--active-regions", action="store_true",
                   help="Assemble only the active regions found over --loci (the --active-* thresholds), not its grid")
    _active_options(p, "active-")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    args = p.parse_args(argv)
    single_process_only("assemble-windows")
    if os.path.lexists(args.out):
        raise FileExistsError("Output path %s already exists" % args.out)
    clock = StageClock()
    # the reads as stored, as realign-reads loads them
    load_args = argparse.Namespace(reference_fasta="", recompute_md_tags=False, device=args.device)
    ctx, (rs,) = load_product_reads(load_args, InputFilters.make(mapped=True, non_duplicate=True), args.reads)
    if ctx is None:
        ctx = native.Context(args.device)
    dr = device_reads(ctx, rs)
    clock.mark("load_reads")
    names = list(rs.contig_names)
    contigs = ReferenceGenome.load_fasta(args.reference_fasta).for_contigs(names)
    dref = ctx.upload_reference(contigs)
    clock.mark("load_reference")
    loci = LociSet.parse(args.loci).result(rs.contig_lengths_map)
    active_info: dict = {}
    if args.active_regions:
        windows = active_windows(args, ctx, dr, dref, rs, loci, clock, active_info)
    else:
        windows = assemble.cut_windows([r for r in loci.ranges() if r[0] in set(names)], args.window_size,
                                       args.window_step or None, args.kmer_size)
    info: dict = {}
    try:
        rows = assemble.assemble_windows(ctx, dr, dref, windows, names, dict(zip(names, contigs)), k=args.kmer_size,
                                         min_occurrence=args.min_occurrence, max_paths=args.max_paths,
                                         min_mapq=args.min_mapq, info=info)
    finally:
        dref.free()
    clock.mark("assemble")
    with open(args.out, "w") as fh:
        fh.write(assemble.TSV_HEADER + "\n")
        fh.writelines(l + "\n" for l in assemble.tsv_lines(rows))
    clock.mark("write")
    print("Assembled %d windows into %d haplotypes; wrote %d rows.%s" %
          (len(windows), info["n_haplotypes"], len(rows), _active_summary(active_info)), file=sys.stderr)
    clock.report(windows=len(windows), graphs_ms=info["ms"], paths_ms=info["paths_ms"], align_ms=info["align_ms"],
                 global_windows=info["n_global"], **_active_report(active_info))
    return 0


def haplotype_likelihoods_main(argv: Sequence[str]) -> int:
    """haplotype-likelihoods: assemble-windows up to the haplotypes, then every window read against
    every haplotype (a pair-HMM forward pass) and the diploid genotype likelihoods over the window's
    haplotypes (Likelihood.likelihoodsOfGenotypes over reads), one TSV line per genotype."""
    import os
    from . import assemble, haplotypes
    from .reference import ReferenceGenome
    p = argparse.ArgumentParser(prog="haplotype-likelihoods",
                                description="likelihoods of the reads under the assembled haplotypes of each window")
    p.add_argument("--reads", required=True, help="Aligned reads")
    p.add_argument("--reference-fasta", required=True, help="Local path to a reference FASTA file")
    p.add_argument("--loci", default="all", help="Loci to cut into windows (e.g. 'all', 'chr1:0-1000,chr2')")
    p.add_argument("--out", required=True, help="Output TSV path of the genotype rows (must not exist)")
    p.add_argument("--out-reads", default="", help="Also write one row per window read: its log-likelihood per haplotype")
    p.add_argument("--kmer-size", type=int, default=25)
    p.add_argument("--min-occurrence", type=int, default=2, help="Occurrences a k-mer needs to be a node")
    p.add_argument("--window-size", type=int, default=200)
    p.add_argument("--window-step", type=int, default=0, help="Distance between window starts (default: the size)")
    p.add_argument("--max-paths", type=int, default=10)
    p.add_argument("--min-mapq", type=int, default=1, help="Only reads of at least this mapping quality")
    p.add_argument("--active-regions", action="store_true",
                   help="Assemble only the active regions found over --loci (the --active-* thresholds), not its grid")
    _active_options(p, "active-")
    p.add_argument("--quality-floor", type=int, default=None, help="Base qualities below it count as it (6)")
    p.add_argument("--mismatch-probability", type=float, default=None, help="For reads without qualities")
    p.add_argument("--open-gap-probability", type=float, default=None)
    p.add_argument("--close-gap-probability", type=float, default=None)
    p.add_argument("--device", type=int, default=0, help="GPU index")
    args = p.parse_args(argv)
    single_process_only("haplotype-likelihoods")
    for path in (args.out, args.out_reads):
        if path and os.path.lexists(path):
            raise FileExistsError("Output path %s already exists" % path)
    clock = StageClock()
    # the reads as stored, as assemble-windows loads them
    load_args = argparse.Namespace(reference_fasta="", recompute_md_tags=False, device=args.device)
    ctx, (rs,) = load_product_reads(load_args, InputFilters.make(mapped=True, non_duplicate=True), args.reads)
    if ctx is None:
        ctx = native.Context(args.device)
    dr = device_reads(ctx, rs)
    clock.mark("load_reads")
    names = list(rs.contig_names)
    contigs = ReferenceGenome.load_fasta(args.reference_fasta).for_contigs(names)
    dref = ctx.upload_reference(contigs)
    clock.mark("load_reference")
    loci = LociSet.parse(args.loci).result(rs.contig_lengths_map)
    active_info: dict = {}
    if args.active_regions:
        windows = active_windows(args, ctx, dr, dref, rs, loci, clock, active_info)
    else:
        windows = assemble.cut_windows([r for r in loci.ranges() if r[0] in set(names)], args.window_size,
                                       args.window_step or None, args.kmer_size)
    info: dict = {}
    try:
        graphs, paths = assemble.graphs_and_paths(ctx, dr, dref, windows, names, k=args.kmer_size,
                                                  min_occurrence=args.min_occurrence, max_paths=args.max_paths,
                                                  min_mapq=args.min_mapq)
        clock.mark("assemble")
        rows, reads = haplotypes.haplotype_likelihoods(
            ctx, dr, dref, graphs, paths, windows, names, min_mapq=args.min_mapq, with_reads=bool(args.out_reads),
            info=info, quality_floor=args.quality_floor, mismatch_probability=args.mismatch_probability,
            open_gap_probability=args.open_gap_probability, close_gap_probability=args.close_gap_probability)
    finally:
        dref.free()
    clock.mark("likelihoods")
    with open(args.out, "w") as fh:
        fh.write(haplotypes.GENOTYPE_HEADER + "\n")
        fh.writelines(l + "\n" for l in haplotypes.genotype_tsv_lines(rows))
    if args.out_reads:
        with open(args.out_reads, "w") as fh:
            fh.write(haplotypes.READ_HEADER + "\n")
            fh.writelines(l + "\n" for l in haplotypes.read_tsv_lines(reads))
    clock.mark("write")
    print("%d windows, %d read-haplotype pairs (%d underflowed), %d genotypes; wrote %d rows.%s" %
          (len(windows), info["n_pairs"], info["n_underflow"], info["n_genotypes"], len(rows),
           _active_summary(active_info)), file=sys.stderr)
    clock.report(windows=len(windows), graphs_ms=graphs.info["ms"], paths_ms=paths["ms"], haplik_ms=info["haplik_ms"],
                 kernel_ms=info["haplik_kernel_ms"], genotype_ms=info["genotype_ms"], **_active_report(active_info))
    return 0


def germline_assembly_main(argv: Sequence[str]) -> int:
    """germline-assembly: haplotype-likelihoods' pipeline, then the variant events the aligned haplotypes
    carry with their genotype likelihoods marginalised over haplotypes (gq_hapvar_windows), as VCF."""
    import os
    from . import assemble, variants_assembly
    from .reference import ReferenceGenome
    p = argparse.ArgumentParser(prog="germline-assembly",
                                description="germline variant calls from the assembled haplotypes of each window")
    p.add_argument("--reads", required=True, help="Aligned reads")
    p.add_argument("--reference-fasta", required=True, help="Local path to a reference FASTA file")
    p.add_argument("--loci", default="all", help="Loci to cut into windows (e.g. 'all', 'chr1:0-1000,chr2')")
    p.add_argument("--out", required=True, help="Output VCF path (must not exist)")
    p.add_argument("--out-events", default="", help="Also write one TSV row per event of every window")
    p.add_argument("--min-qual", type=float, default=0.0, help="Only calls of at least this QUAL")
    p.add_argument("--emit-all-events", action="store_true", help="Also write events whose best genotype is 0/0")
    p.add_argument("--sample", default="sample", help="Name of the VCF's sample column")
    p.add_argument("--kmer-size", type=int, default=25)
    p.add_argument("--min-occurrence", type=int, default=2, help="Occurrences a k-mer needs to be a node")
    p.add_argument("--window-size", type=int, default=200)
    p.add_argument("--window-step", type=int, default=0, help="Distance between window starts (default: the size)")
    p.add_argument("--max-paths", type=int, default=10)
    p.add_argument("--min-mapq", type=int, default=1, help="Only reads of at least this mapping quality")
    p.add_argument("--active-regions", action="store_true",
                   help="Assemble only the active regions found over --loci (the --active-* thresholds), not its grid")
    _active_options(p, "active-")
    p.add_argument("--quality-floor", type=int, default=None, help="Base qualities below it count as it (6)")
    p.add_argument("--mismatch-probability", type=float, default=None, help="For reads without qualities")
    p.add_argument("--open-gap-probability", type=float, default=None)
    p.add_argument("--close-gap-probability", type=float, default=None)
    p.add_argument("--device", type=int, default=0, help="GPU index")
    args = p.parse_args(argv)
    single_process_only("germline-assembly")
    for path in (args.out, args.out_events):
        if path and os.path.lexists(path):
            raise FileExistsError("Output path %s already exists" % path)
    clock = StageClock()
    # the reads as stored, as assemble-windows loads them
    load_args = argparse.Namespace(reference_fasta="", recompute_md_tags=False, device=args.device)
    ctx, (rs,) = load_product_reads(load_args, InputFilters.make(mapped=True, non_duplicate=True), args.reads)
    if ctx is None:
        ctx = native.Context(args.device)
    dr = device_reads(ctx, rs)
    clock.mark("load_reads")
    names = list(rs.contig_names)
    contigs = ReferenceGenome.load_fasta(args.reference_fasta).for_contigs(names)
    dref = ctx.upload_reference(contigs)
    clock.mark("load_reference")
    loci = LociSet.parse(args.loci).result(rs.contig_lengths_map)
    active_info: dict = {}
    if args.active_regions:
        windows = active_windows(args, ctx, dr, dref, rs, loci, clock, active_info)
    else:
        windows = assemble.cut_windows([r for r in loci.ranges() if r[0] in set(names)], args.window_size,
                                       args.window_step or None, args.kmer_size)
    info: dict = {}
    try:
        rows, _, _ = variants_assembly.call_windows(
            ctx, dr, dref, windows, names, dict(zip(names, contigs)), k=args.kmer_size,
            min_occurrence=args.min_occurrence, max_paths=args.max_paths, min_mapq=args.min_mapq, info=info,
            quality_floor=args.quality_floor, mismatch_probability=args.mismatch_probability,
            open_gap_probability=args.open_gap_probability, close_gap_probability=args.close_gap_probability)
    finally:
        dref.free()
    clock.mark("call")
    calls = variants_assembly.select_calls(rows, names, emit_all=args.emit_all_events, min_qual=args.min_qual)
    with open(args.out, "w") as fh:
        fh.write(variants_assembly.vcf_text(calls, args.sample, dict(rs.contig_lengths_map)))
    if args.out_events:
        with open(args.out_events, "w") as fh:
            fh.write(variants_assembly.EVENT_HEADER + "\n")
            fh.writelines(l + "\n" for l in variants_assembly.event_tsv_lines(rows))
    clock.mark("write")
    print("%d windows, %d haplotypes (%d not usable), %d events (%d indels dropped at a window's edge, %d windows "
          "over the event cap); wrote %d calls.%s" %
          (len(windows), info["n_haplotypes"], info["n_unusable"], info["n_events"], info["n_edge_dropped"],
           info["n_capped_windows"], len(calls), _active_summary(active_info)), file=sys.stderr)
    clock.report(windows=len(windows), graphs_ms=info["graphs_ms"], paths_ms=info["paths_ms"], align_ms=info["align_ms"],
                 haplik_ms=info["haplik_ms"], hapvar_ms=info["hapvar_ms"], events_ms=info["events_ms"],
                 marginal_ms=info["marginal_ms"], **_active_report(active_info))
    return 0


COMMANDS = {"germline-threshold": germline_threshold_main, "somatic-standard": somatic_standard_main,
            "variant-support": variant_support_main, "vaf-histogram": vaf_histogram_main,
            "germline-standard": germline_standard_main, "allele-evidence": allele_evidence_main,
            "genotype-likelihoods": genotype_likelihoods_main, "pileup-elements": pileup_elements_main, "somatic-likelihoods": somatic_likelihoods_main,
            "pileup-counts": pileup_counts_main, "active-regions": active_regions_main, "structural-variant": structural_variant_main,
            "realign-reads": realign_reads_main, "assemble-windows": assemble_windows_main,
            "haplotype-likelihoods": haplotype_likelihoods_main, "germline-assembly": germline_assembly_main}


def main(argv: Optional[Sequence[str]] = None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] not in COMMANDS:
        print("usage: python -m guacamole_amd <command> [args]\ncommands: " + ", ".join(sorted(COMMANDS)),
              file=sys.stderr)
        return 1
    return COMMANDS[argv[0]](argv[1:])
