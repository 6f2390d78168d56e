"""ctypes binding of libgqpileup.so (include/gqpileup.h).

The HIP library is the only compute path: if it is missing or the GPU cannot be
opened, every entry point raises — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libgqpileup.so")
_lib = None

GT_NAMES = {0: "Ref", 1: "Alt", 2: "OtherAlt", 3: "NoCall"}
FLAG_AMBIGUOUS_REF = 1
FLAG_TIE = 2
FLAG_KNIFE_EDGE = 4


class GQError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("gqpileup error %d: %s" % (code, msg))
        self.code = code


class gq_reads(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_contigs", C.c_int32), ("n_samples", C.c_int32)] + [
        (n, C.c_void_p) for n in ("contig_read_begin", "start", "end", "pmax_end", "mapq", "flags", "sample",
                                  "seq_off", "seq_len", "cigar_off", "n_cigar", "md_off", "n_md", "n_mismatch")] + [
        ("seq_bytes", C.c_int64), ("cigar_len", C.c_int64), ("md_len", C.c_int64)] + [
        (n, C.c_void_p) for n in ("seq", "qual", "cigar", "md_ev", "sample_hash")]


class gq_loci(C.Structure):
    _fields_ = [("n_ranges", C.c_int64), ("contig", C.c_void_p), ("start", C.c_void_p), ("end", C.c_void_p),
                ("task", C.c_void_p)]


class gq_germline_params(C.Structure):
    _fields_ = [("threshold", C.c_int32), ("emit_ref", C.c_int32), ("emit_no_call", C.c_int32)]


class gq_calls(C.Structure):
    _fields_ = [("n", C.c_int64), ("contig", C.POINTER(C.c_int32)), ("pos", C.POINTER(C.c_int64)),
                ("sample", C.POINTER(C.c_uint8)), ("gt0", C.POINTER(C.c_uint8)), ("gt1", C.POINTER(C.c_uint8)),
                ("flags", C.POINTER(C.c_uint8)), ("ref_off", C.POINTER(C.c_int64)), ("ref_len", C.POINTER(C.c_int32)),
                ("alt_off", C.POINTER(C.c_int64)), ("alt_len", C.POINTER(C.c_int32)),
                ("allele_pool", C.POINTER(C.c_uint8)), ("pool_len", C.c_int64), ("visited_loci", C.c_int64),
                ("complex_loci", C.c_int64), ("ambiguous_loci", C.c_int64), ("tie_loci", C.c_int64),
                ("block_", C.c_void_p)]


class gq_calls_device(C.Structure):
    _fields_ = [("calls", gq_calls), ("image", C.c_void_p), ("image_bytes", C.c_int64)]


class gq_allele_counts(C.Structure):
    _fields_ = [("n", C.c_int64), ("contig", C.POINTER(C.c_int32)), ("pos", C.POINTER(C.c_int64)),
                ("sample", C.POINTER(C.c_int32)), ("count", C.POINTER(C.c_int32)),
                ("ref_off", C.POINTER(C.c_int64)), ("ref_len", C.POINTER(C.c_int32)),
                ("alt_off", C.POINTER(C.c_int64)), ("alt_len", C.POINTER(C.c_int32)),
                ("allele_pool", C.c_void_p), ("pool_len", C.c_int64), ("flags", C.POINTER(C.c_uint8))]


class gq_germline_std_params(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("min_mapq", "min_read_depth", "max_read_depth", "min_alternate_read_depth",
                                         "min_likelihood", "apply_filters")]


GERMLINE_STD_DEFAULTS = dict(min_mapq=1, min_read_depth=0, max_read_depth=2 ** 31 - 1, min_alternate_read_depth=0,
                             min_likelihood=0, apply_filters=1)


class gq_allele_evidence_params(C.Structure):
    _fields_ = [("min_mapq", C.c_int32), ("variants_only", C.c_int32)]


class gq_genotype_likelihood_params(C.Structure):
    _fields_ = [("min_mapq", C.c_int32), ("variants_only", C.c_int32), ("include_alignment", C.c_int32),
                ("normalize", C.c_int32)]


class gq_vaf_params(C.Structure):
    _fields_ = [("bins", C.c_int32), ("min_read_depth", C.c_int32), ("min_vaf", C.c_int32)]


class gq_vaf_hist(C.Structure):
    _fields_ = [("counts", C.c_int64 * 101), ("variant_loci", C.c_int64), ("visited_loci", C.c_int64)]


class gq_counts(C.Structure):
    _fields_ = [("n_loci", C.c_int64), ("depth", C.POINTER(C.c_int32)), ("pos_depth", C.POINTER(C.c_int32)),
                ("base_counts", C.POINTER(C.c_int32)), ("indel_counts", C.POINTER(C.c_int32)),
                ("ref_depth", C.POINTER(C.c_int32)), ("ref_base", C.POINTER(C.c_uint8)),
                ("ambiguous", C.POINTER(C.c_uint8))]


class gq_timings(C.Structure):
    _fields_ = [("plan_ms", C.c_float), ("pileup_ms", C.c_float), ("complex_ms", C.c_float),
                ("finalize_ms", C.c_float), ("total_ms", C.c_float), ("pileup_launches", C.c_int64),
                ("tiles", C.c_int64), ("host_ms", C.c_float), ("marshal_ms", C.c_float),
                ("walk_ms", C.c_float), ("walk_tiles", C.c_int64), ("order_loci", C.c_int64),
                ("deep_loci", C.c_int64), ("deep_max", C.c_int64), ("call_ms", C.c_float), ("deep_ms", C.c_float),
                ("front_ms", C.c_float)]


class gq_reads_info(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_reads", "seq_bytes", "proj_bytes", "pev_count", "proj_reads", "n_rows")] + [
        ("h2d_ms", C.c_float), ("derive_ms", C.c_float), ("cigar_len", C.c_int64), ("md_len", C.c_int64),
        ("n_contigs", C.c_int32), ("n_samples", C.c_int32), ("proj_ms", C.c_float), ("projected", C.c_int32),
        ("fill_ms", C.c_float), ("proj_dev_ms", C.c_float), ("derive_dev_ms", C.c_float)]


class gq_somatic_params(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "odds", "min_mapq", "filter_multi_allelic", "max_read_depth", "min_tumor_read_depth",
        "max_tumor_read_depth", "min_normal_read_depth", "min_tumor_alternate_read_depth", "min_lod",
        "min_likelihood", "min_vaf", "min_average_mapping_quality", "min_average_base_quality",
        "max_median_mismatches", "apply_filters")]


class gq_evidence(C.Structure):
    _fields_ = [("likelihood", C.c_double), ("read_depth", C.c_int32), ("allele_read_depth", C.c_int32),
                ("forward_depth", C.c_int32), ("allele_forward_depth", C.c_int32), ("mean_mq", C.c_double),
                ("median_mq", C.c_double), ("mean_bq", C.c_double), ("median_bq", C.c_double),
                ("median_mismatches", C.c_double)]


# SomaticStandard.Arguments defaults (commands/SomaticStandardCaller.scala:40-64 and
# filters/SomaticGenotypeFilter.scala:31-56); apply_filters 1 = the driver's filter chain.
SOMATIC_DEFAULTS = dict(odds=20, min_mapq=1, filter_multi_allelic=0, max_read_depth=2 ** 31 - 1,
                        min_tumor_read_depth=0, max_tumor_read_depth=2 ** 31 - 1, min_normal_read_depth=0,
                        min_tumor_alternate_read_depth=0, min_lod=0, min_likelihood=0, min_vaf=0,
                        min_average_mapping_quality=0, min_average_base_quality=0,
                        max_median_mismatches=2 ** 31 - 1, apply_filters=1)

_EVIDENCE_DTYPE = np.dtype([("likelihood", np.float64), ("read_depth", np.int32), ("allele_read_depth", np.int32),
                            ("forward_depth", np.int32), ("allele_forward_depth", np.int32), ("mean_mq", np.float64),
                            ("median_mq", np.float64), ("mean_bq", np.float64), ("median_bq", np.float64),
                            ("median_mismatches", np.float64)])

EVIDENCE_FIELDS = ("likelihood", "read_depth", "allele_read_depth", "forward_depth", "allele_forward_depth",
                   "mean_mq", "median_mq", "mean_bq", "median_bq", "median_mismatches")


class gq_somatic_calls(C.Structure):
    _fields_ = [("n", C.c_int64), ("contig", C.POINTER(C.c_int32)), ("pos", C.POINTER(C.c_int64)),
                ("sample", C.POINTER(C.c_uint8)), ("ref_off", C.POINTER(C.c_int64)), ("ref_len", C.POINTER(C.c_int32)),
                ("alt_off", C.POINTER(C.c_int64)), ("alt_len", C.POINTER(C.c_int32)),
                ("allele_pool", C.POINTER(C.c_uint8)), ("pool_len", C.c_int64), ("log_odds", C.POINTER(C.c_double)),
                ("gq", C.POINTER(C.c_int32)), ("tumor", C.POINTER(gq_evidence)), ("normal", C.POINTER(gq_evidence)),
                ("flags", C.POINTER(C.c_uint8)), ("visited_loci", C.c_int64), ("candidate_loci", C.c_int64),
                ("block_", C.c_void_p)]


class gq_allele_evidence_rows(C.Structure):
    _fields_ = [("n", C.c_int64), ("contig", C.POINTER(C.c_int32)), ("pos", C.POINTER(C.c_int64)),
                ("sample", C.POINTER(C.c_int32)), ("ref_off", C.POINTER(C.c_int64)), ("ref_len", C.POINTER(C.c_int32)),
                ("alt_off", C.POINTER(C.c_int64)), ("alt_len", C.POINTER(C.c_int32)),
                ("allele_pool", C.POINTER(C.c_uint8)), ("pool_len", C.c_int64), ("evidence", C.POINTER(gq_evidence)),
                ("flags", C.POINTER(C.c_uint8)), ("visited_loci", C.c_int64), ("listed_loci", C.c_int64)]


class gq_genotype_likelihoods(C.Structure):
    _fields_ = [("n_groups", C.c_int64), ("contig", C.POINTER(C.c_int32)), ("pos", C.POINTER(C.c_int64)),
                ("sample", C.POINTER(C.c_int32)), ("depth", C.POINTER(C.c_int32)), ("n_alleles", C.POINTER(C.c_int32)),
                ("allele_first", C.POINTER(C.c_int64)), ("geno_first", C.POINTER(C.c_int64)),
                ("flags", C.POINTER(C.c_uint8)), ("n_alleles_total", C.c_int64), ("ref_off", C.POINTER(C.c_int64)),
                ("ref_len", C.POINTER(C.c_int32)), ("alt_off", C.POINTER(C.c_int64)), ("alt_len", C.POINTER(C.c_int32)),
                ("allele_depth", C.POINTER(C.c_int32)), ("allele_pool", C.POINTER(C.c_uint8)), ("pool_len", C.c_int64),
                ("n_genotypes", C.c_int64), ("log_likelihood", C.POINTER(C.c_double)), ("visited_loci", C.c_int64),
                ("listed_loci", C.c_int64), ("block_", C.c_void_p)]


class gq_pileup_elements_params(C.Structure):
    _fields_ = [("min_mapq", C.c_int32), ("variants_only", C.c_int32)]


class gq_pileup_elements(C.Structure):
    _fields_ = [("n_groups", C.c_int64), ("contig", C.POINTER(C.c_int32)), ("pos", C.POINTER(C.c_int64)),
                ("ref_base", C.POINTER(C.c_uint8)), ("flags", C.POINTER(C.c_uint8)), ("depth", C.POINTER(C.c_int32)),
                ("n_alleles", C.POINTER(C.c_int32)), ("elem_first", C.POINTER(C.c_int64)),
                ("allele_first", C.POINTER(C.c_int64)), ("n_alleles_total", C.c_int64),
                ("ref_off", C.POINTER(C.c_int64)), ("ref_len", C.POINTER(C.c_int32)), ("alt_off", C.POINTER(C.c_int64)),
                ("alt_len", C.POINTER(C.c_int32)), ("allele_depth", C.POINTER(C.c_int32)),
                ("allele_pool", C.POINTER(C.c_uint8)), ("pool_len", C.c_int64), ("n_elements", C.c_int64),
                ("elem_read", C.POINTER(C.c_int64)), ("elem_sample", C.POINTER(C.c_uint8)),
                ("elem_mapq", C.POINTER(C.c_uint8)), ("elem_strand", C.POINTER(C.c_uint8)),
                ("elem_kind", C.POINTER(C.c_uint8)), ("elem_allele", C.POINTER(C.c_int32)),
                ("elem_quality", C.POINTER(C.c_int16)), ("elem_read_position", C.POINTER(C.c_int32)),
                ("elem_cigar_index", C.POINTER(C.c_int32)), ("elem_index_within", C.POINTER(C.c_int32)),
                ("visited_loci", C.c_int64), ("listed_loci", C.c_int64), ("block_bytes", C.c_int64),
                ("block_", C.c_void_p)]


class gq_somatic_likelihood_params(C.Structure):
    _fields_ = [("min_mapq", C.c_int32), ("filter_multi_allelic", C.c_int32), ("max_read_depth", C.c_int32),
                ("reserved", C.c_int32)]


def _sample_allele_fields(s: str):
    return [(s + "_ref_off", C.POINTER(C.c_int64)), (s + "_ref_len", C.POINTER(C.c_int32)),
            (s + "_alt_off", C.POINTER(C.c_int64)), (s + "_alt_len", C.POINTER(C.c_int32)),
            (s + "_allele_depth", C.POINTER(C.c_int32))]


class gq_somatic_likelihoods(C.Structure):
    _fields_ = ([("n_groups", C.c_int64), ("contig", C.POINTER(C.c_int32)), ("pos", C.POINTER(C.c_int64)),
                 ("flags", C.POINTER(C.c_uint8)), ("tumor_ref_base", C.POINTER(C.c_uint8)),
                 ("normal_ref_base", C.POINTER(C.c_uint8)), ("tumor_depth", C.POINTER(C.c_int32)),
                 ("normal_depth", C.POINTER(C.c_int32)), ("tumor_n_alleles", C.POINTER(C.c_int32)),
                 ("normal_n_alleles", C.POINTER(C.c_int32)), ("tumor_allele_first", C.POINTER(C.c_int64)),
                 ("normal_allele_first", C.POINTER(C.c_int64)), ("tumor_geno_first", C.POINTER(C.c_int64)),
                 ("normal_geno_first", C.POINTER(C.c_int64)), ("best", C.POINTER(C.c_int32)),
                 ("has_variant", C.POINTER(C.c_uint8)), ("normal_variant_total", C.POINTER(C.c_double)),
                 ("log_odds", C.POINTER(C.c_double)), ("n_tumor_alleles", C.c_int64)] + _sample_allele_fields("tumor") +
                [("n_normal_alleles", C.c_int64)] + _sample_allele_fields("normal") +
                [("allele_pool", C.POINTER(C.c_uint8)), ("pool_len", C.c_int64), ("n_tumor_genotypes", C.c_int64),
                 ("tumor_log_likelihood", C.POINTER(C.c_double)), ("n_normal_genotypes", C.c_int64),
                 ("normal_log_likelihood", C.POINTER(C.c_double)), ("visited_loci", C.c_int64),
                 ("listed_loci", C.c_int64), ("block_bytes", C.c_int64), ("block_", C.c_void_p)])


class gq_pileup_counts_params(C.Structure):
    _fields_ = [("min_mapq", C.c_int32), ("min_depth", C.c_int32), ("variants_only", C.c_int32),
                ("reserved", C.c_int32)]


class gq_pileup_count_rows(C.Structure):
    _fields_ = [("n", C.c_int64), ("contig", C.POINTER(C.c_int32)), ("pos", C.POINTER(C.c_int64)),
                ("ref_base", C.POINTER(C.c_uint8)), ("flags", C.POINTER(C.c_uint8)), ("depth", C.POINTER(C.c_int32)),
                ("forward_depth", C.POINTER(C.c_int32)), ("ref_depth", C.POINTER(C.c_int32)),
                ("base_count", C.POINTER(C.c_int32)), ("base_forward", C.POINTER(C.c_int32)),
                ("kind_count", C.POINTER(C.c_int32)), ("visited_loci", C.c_int64), ("listed_loci", C.c_int64),
                ("block_bytes", C.c_int64), ("block_", C.c_void_p)]


class gq_active_params(C.Structure):
    _fields_ = [("min_mapq", C.c_int32), ("min_depth", C.c_int32), ("min_evidence", C.c_int32),
                ("min_percent", C.c_int32), ("pad", C.c_int32), ("reserved", C.c_int32 * 3)]


class gq_active_regions(C.Structure):
    _fields_ = [("n", C.c_int64), ("contig", C.POINTER(C.c_int32)), ("start", C.POINTER(C.c_int64)),
                ("end", C.POINTER(C.c_int64)), ("n_active", C.POINTER(C.c_int32)), ("evidence", C.POINTER(C.c_int64)),
                ("n_loci", C.c_int64), ("locus_contig", C.POINTER(C.c_int32)), ("locus_pos", C.POINTER(C.c_int64)),
                ("locus_depth", C.POINTER(C.c_int32)), ("locus_evidence", C.POINTER(C.c_int32)),
                ("visited_loci", C.c_int64), ("listed_loci", C.c_int64), ("block_bytes", C.c_int64),
                ("block_", C.c_void_p)]


class gq_md_rebuild_info(C.Structure):
    _fields_ = [("read", C.c_int64), ("code", C.c_int32), ("pad", C.c_int32), ("rebuilt", C.c_int64),
                ("md_events", C.c_int64), ("ms", C.c_float)]


class gq_sv_stats(C.Structure):
    _fields_ = [("n_pairs", C.c_int64), ("n_in_range", C.c_int64), ("n_exceptional", C.c_int64),
                ("median", C.c_double), ("mad", C.c_double), ("max_normal", C.c_int32), ("reserved", C.c_int32),
                ("stats_ms", C.c_float), ("order_ms", C.c_float)]


class gq_sv_graph(C.Structure):
    _fields_ = [("n_nodes", C.c_int64), ("n_edges", C.c_int64), ("i", C.POINTER(C.c_int32)),
                ("j", C.POINTER(C.c_int32)), ("weight", C.POINTER(C.c_int64)), ("edge_ms", C.c_float),
                ("reserved", C.c_int32)]


class gq_sv_cliques(C.Structure):
    _fields_ = [("n", C.c_int64), ("contig", C.POINTER(C.c_int32)), ("start", C.POINTER(C.c_int64)),
                ("stop", C.POINTER(C.c_int64)), ("pairs", C.POINTER(C.c_int64)), ("wiggle", C.POINTER(C.c_int64))]


class gq_align_params(C.Structure):
    _fields_ = [("mismatch_probability", C.c_double), ("open_gap_probability", C.c_double),
                ("close_gap_probability", C.c_double), ("reserved", C.c_double * 5)]


class gq_alignments(C.Structure):
    _fields_ = [("n", C.c_int64), ("ref_start", C.POINTER(C.c_int32)), ("ref_end", C.POINTER(C.c_int32)),
                ("score", C.POINTER(C.c_double)), ("score_int", C.POINTER(C.c_int32)),
                ("cigar_off", C.POINTER(C.c_int64)), ("cigar", C.POINTER(C.c_uint32)), ("ms", C.c_float),
                ("kernel_ms", C.c_float), ("launches", C.c_int32), ("reserved", C.c_int32), ("block_", C.c_void_p)]


class gq_align_reads_info(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_selected", C.c_int64), ("skipped", C.c_int64), ("select_ms", C.c_float),
                ("reserved", C.c_int32)]


class gq_asm_params(C.Structure):
    _fields_ = [("k", C.c_int32), ("min_occurrence", C.c_int32), ("max_paths", C.c_int32),
                ("max_path_length", C.c_int32), ("max_steps", C.c_int64), ("min_mapq", C.c_int32), ("reserved0", C.c_int32),
                ("reserved", C.c_int64 * 4)]


class gq_asm_graph_block(C.Structure):
    _fields_ = [("n_windows", C.c_int64), ("n_nodes", C.c_int64), ("node_off", C.POINTER(C.c_int64)),
                ("key_lo", C.POINTER(C.c_uint64)), ("key_hi", C.POINTER(C.c_uint64)), ("count", C.POINTER(C.c_int32)),
                ("child_mask", C.POINTER(C.c_uint8)), ("parent_mask", C.POINTER(C.c_uint8)),
                ("source", C.POINTER(C.c_int32)), ("sink", C.POINTER(C.c_int32)), ("status", C.POINTER(C.c_int32)),
                ("n_reads", C.POINTER(C.c_int32)), ("win_len", C.POINTER(C.c_int32)),
                ("n_instances", C.POINTER(C.c_int64)), ("k", C.c_int32), ("min_occurrence", C.c_int32),
                ("ms", C.c_float), ("reads_ms", C.c_float), ("count_ms", C.c_float), ("edges_ms", C.c_float),
                ("launches", C.c_int32), ("n_global", C.c_int32), ("block_", C.c_void_p)]


class gq_asm_path_block(C.Structure):
    _fields_ = [("n_windows", C.c_int64), ("n_haplotypes", C.c_int64), ("n_unitigs", C.c_int64),
                ("hap_off", C.POINTER(C.c_int64)), ("hap_seq_off", C.POINTER(C.c_int64)),
                ("bases", C.POINTER(C.c_uint8)), ("support", C.POINTER(C.c_int32)), ("status", C.POINTER(C.c_int32)),
                ("steps", C.POINTER(C.c_int64)), ("unitig_off", C.POINTER(C.c_int64)),
                ("unitig_seq_off", C.POINTER(C.c_int64)), ("unitig_bases", C.POINTER(C.c_uint8)), ("ms", C.c_float),
                ("reserved", C.c_int32), ("block_", C.c_void_p)]


class gq_haplik_params(C.Structure):
    _fields_ = [("mismatch_probability", C.c_double), ("open_gap_probability", C.c_double),
                ("close_gap_probability", C.c_double), ("quality_floor", C.c_double), ("reserved", C.c_double * 4)]


class gq_haplik_pairs(C.Structure):
    _fields_ = [("n", C.c_int64), ("scaled", C.POINTER(C.c_double)), ("log_likelihood", C.POINTER(C.c_double)),
                ("flags", C.POINTER(C.c_uint8)), ("ms", C.c_float), ("kernel_ms", C.c_float), ("block_", C.c_void_p)]


class gq_haplik_block(C.Structure):
    _fields_ = [("n_windows", C.c_int64), ("n_reads", C.c_int64), ("n_pairs", C.c_int64), ("n_genotypes", C.c_int64),
                ("win_read_off", C.POINTER(C.c_int64)), ("win_reads", C.POINTER(C.c_int64)),
                ("lik_off", C.POINTER(C.c_int64)), ("scaled", C.POINTER(C.c_double)),
                ("log_likelihood", C.POINTER(C.c_double)), ("flags", C.POINTER(C.c_uint8)),
                ("gt_off", C.POINTER(C.c_int64)), ("gt_log_likelihood", C.POINTER(C.c_double)),
                ("best_genotype", C.POINTER(C.c_int32)), ("ms", C.c_float), ("reads_ms", C.c_float),
                ("kernel_ms", C.c_float), ("genotype_ms", C.c_float), ("block_", C.c_void_p)]


class gq_hapvar_input(C.Structure):
    _fields_ = [("n_windows", C.c_int64), ("n_haplotypes", C.c_int64), ("n_align", C.c_int64)] + [
        (n, C.c_void_p) for n in ("win_start", "ref_pool", "ref_off", "win_len", "hap_off", "hap_seq_off", "bases",
                                  "hap_align", "ref_start", "ref_end", "cigar_off", "cigar", "win_read_off", "lik_off",
                                  "scaled")]


class gq_hapvar_block(C.Structure):
    _fields_ = [("n_windows", C.c_int64), ("n_events", C.c_int64), ("n_haplotypes", C.c_int64),
                ("n_alt_bases", C.c_int64), ("ev_off", C.POINTER(C.c_int64)), ("pos", C.POINTER(C.c_int64)),
                ("kind", C.POINTER(C.c_uint8)), ("ref_len", C.POINTER(C.c_int32)), ("alt_off", C.POINTER(C.c_int64)),
                ("alt_len", C.POINTER(C.c_int32)), ("alt_bases", C.POINTER(C.c_uint8)),
                ("carriers", C.POINTER(C.c_uint64)), ("gl", C.POINTER(C.c_double)), ("best", C.POINTER(C.c_int32)),
                ("ad_ref", C.POINTER(C.c_int32)), ("ad_alt", C.POINTER(C.c_int32)), ("dp", C.POINTER(C.c_int32)),
                ("ev_flags", C.POINTER(C.c_uint8)), ("hap_flags", C.POINTER(C.c_uint8)),
                ("win_flags", C.POINTER(C.c_uint8)), ("n_edge_dropped", C.c_int64), ("ms", C.c_float),
                ("events_ms", C.c_float), ("marginal_ms", C.c_float), ("reserved", C.c_int32), ("block_", C.c_void_p)]


# gq_pileup_elements.elem_kind (PileupElement.alignment)
ELEMENT_KINDS = ("Match", "Mismatch", "Insertion", "Deletion", "MidDeletion", "Clipped")

EXPORTED = ("gq_version", "gq_last_error", "gq_open", "gq_close", "gq_get_timings", "gq_set_tile", "gq_reads_upload",
            "gq_reads_wrap_device", "gq_reads_free", "gq_reads_rederive", "gq_germline_threshold", "gq_germline_threshold_device",
            "gq_free_calls", "gq_pileup_counts",
            "gq_free_counts", "gq_somatic_standard", "gq_free_somatic", "gq_reads_get_info", "gq_reference_upload",
            "gq_reference_free", "gq_somatic_standard_ref", "gq_variant_support", "gq_free_allele_counts",
            "gq_vaf_histogram", "gq_germline_standard", "gq_bam_dev_open", "gq_bam_dev_close", "gq_bam_dev_header_text",
            "gq_bam_dev_n_contigs", "gq_bam_dev_contig_name", "gq_bam_dev_contig_length", "gq_bam_dev_scan",
            "gq_bam_dev_reads", "gq_reads_positions", "gq_reads_contig_begin", "gq_reads_download", "gq_bam_dev_map",
            "gq_bam_dev_load", "gq_bam_dev_map_ex", "gq_bam_dev_plan", "gq_bam_dev_plan_segments",
            "gq_write_vcf_germline", "gq_allele_evidence", "gq_free_allele_evidence", "gq_genotype_likelihoods_call",
            "gq_free_genotype_likelihoods", "gq_pileup_elements_call", "gq_free_pileup_elements",
            "gq_somatic_likelihoods_call", "gq_free_somatic_likelihoods", "gq_pileup_counts_call",
            "gq_free_pileup_counts", "gq_reads_rebuild_md", "gq_md_rebuild_spans", "gq_reads_missing_md",
            "gq_sv_pairs_from_bam", "gq_sv_pairs_from_host", "gq_sv_pairs_count", "gq_sv_pairs_download",
            "gq_sv_pairs_free", "gq_sv_stats_call", "gq_sv_select", "gq_sv_nodes_download", "gq_sv_graph_call",
            "gq_sv_free_graph", "gq_sv_cliques_call", "gq_sv_free_cliques", "gq_sv_call",
            "gq_align_default_params", "gq_align_penalties", "gq_align_limits", "gq_align_batch", "gq_align_host",
            "gq_free_alignments", "gq_align_reads", "gq_align_free_index",
            "gq_asm_default_params", "gq_asm_limits", "gq_asm_graphs", "gq_asm_graphs_host", "gq_asm_free_graphs",
            "gq_asm_paths", "gq_asm_free_paths",
            "gq_haplik_default_params", "gq_haplik_tables", "gq_haplik_batch", "gq_haplik_host", "gq_haplik_free_pairs",
            "gq_haplik_windows", "gq_haplik_free_block", "gq_haplik_genotypes_host",
            "gq_hapvar_limits", "gq_hapvar_windows", "gq_hapvar_host", "gq_hapvar_free_block",
            "gq_active_regions_call", "gq_active_regions_host", "gq_free_active_regions")


def lib():
    """Load the HIP library (raises if it has not been built)."""
    global _lib
    if _lib is None:
        # GQ_LIB: an alternative in-tree build of the same library (kernel A/B experiments)
        path = os.environ.get("GQ_LIB", LIB_PATH)
        if not os.path.exists(path):
            raise RuntimeError("libgqpileup.so not built (%s); run __graft_entry__.build()" % path)
        L = C.CDLL(path)
        L.gq_version.restype = C.c_char_p
        L.gq_last_error.restype = C.c_char_p
        for f in ("gq_open", "gq_get_timings", "gq_set_tile", "gq_reads_upload", "gq_reads_wrap_device", "gq_reads_get_info",
                  "gq_reads_rederive", "gq_reads_rebuild_md", "gq_md_rebuild_spans", "gq_reads_missing_md",
                  "gq_germline_threshold", "gq_germline_threshold_device", "gq_pileup_counts", "gq_somatic_standard",
                  "gq_reference_upload", "gq_somatic_standard_ref", "gq_variant_support", "gq_vaf_histogram",
                  "gq_germline_standard", "gq_allele_evidence", "gq_genotype_likelihoods_call",
                  "gq_pileup_elements_call", "gq_somatic_likelihoods_call", "gq_pileup_counts_call"):
            getattr(L, f).restype = C.c_int
        L.gq_germline_threshold.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(gq_loci), C.POINTER(gq_germline_params),
                                            C.POINTER(C.POINTER(gq_calls))]
        L.gq_germline_threshold_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(gq_loci),
                                                   C.POINTER(gq_germline_params), C.POINTER(gq_calls_device)]
        L.gq_pileup_counts.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(gq_loci), C.POINTER(C.POINTER(gq_counts))]
        L.gq_somatic_standard.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(gq_loci),
                                          C.POINTER(gq_somatic_params), C.POINTER(C.POINTER(gq_somatic_calls))]
        L.gq_somatic_standard_ref.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(gq_loci), C.c_void_p,
                                              C.POINTER(gq_somatic_params), C.POINTER(C.POINTER(gq_somatic_calls))]
        L.gq_reference_upload.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.c_void_p,
                                          C.POINTER(C.c_void_p)]
        L.gq_reference_free.argtypes = [C.c_void_p]
        L.gq_variant_support.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(gq_loci),
                                         C.POINTER(C.POINTER(gq_allele_counts))]
        L.gq_free_allele_counts.argtypes = [C.POINTER(gq_allele_counts)]
        L.gq_germline_standard.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(gq_loci), C.POINTER(gq_germline_std_params),
                                           C.POINTER(C.POINTER(gq_somatic_calls))]
        L.gq_allele_evidence.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(gq_loci), C.POINTER(gq_allele_evidence_params),
                                         C.POINTER(C.POINTER(gq_allele_evidence_rows))]
        L.gq_free_allele_evidence.argtypes = [C.POINTER(gq_allele_evidence_rows)]
        L.gq_free_allele_evidence.restype = None
        L.gq_genotype_likelihoods_call.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(gq_loci),
                                                   C.POINTER(gq_genotype_likelihood_params),
                                                   C.POINTER(C.POINTER(gq_genotype_likelihoods))]
        L.gq_free_genotype_likelihoods.argtypes = [C.POINTER(gq_genotype_likelihoods)]
        L.gq_free_genotype_likelihoods.restype = None
        L.gq_pileup_elements_call.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(gq_loci),
                                              C.POINTER(gq_pileup_elements_params),
                                              C.POINTER(C.POINTER(gq_pileup_elements))]
        L.gq_free_pileup_elements.argtypes = [C.POINTER(gq_pileup_elements)]
        L.gq_free_pileup_elements.restype = None
        L.gq_somatic_likelihoods_call.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(gq_loci),
                                                  C.POINTER(gq_somatic_likelihood_params),
                                                  C.POINTER(C.POINTER(gq_somatic_likelihoods))]
        L.gq_free_somatic_likelihoods.argtypes = [C.POINTER(gq_somatic_likelihoods)]
        L.gq_free_somatic_likelihoods.restype = None
        L.gq_pileup_counts_call.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(gq_loci),
                                            C.POINTER(gq_pileup_counts_params),
                                            C.POINTER(C.POINTER(gq_pileup_count_rows))]
        L.gq_free_pileup_counts.argtypes = [C.POINTER(gq_pileup_count_rows)]
        L.gq_free_pileup_counts.restype = None
        L.gq_active_regions_call.restype = C.c_int
        L.gq_active_regions_call.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(gq_loci), C.POINTER(gq_active_params),
                                             C.POINTER(C.POINTER(gq_active_regions))]
        L.gq_active_regions_host.restype = C.c_int
        L.gq_active_regions_host.argtypes = [C.c_int64] + [C.c_void_p] * 7 + [C.POINTER(gq_active_params),
                                                                              C.POINTER(C.POINTER(gq_active_regions))]
        L.gq_free_active_regions.argtypes = [C.POINTER(gq_active_regions)]
        L.gq_free_active_regions.restype = None
        L.gq_vaf_histogram.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(gq_loci), C.POINTER(gq_vaf_params),
                                       C.POINTER(gq_vaf_hist)]
        L.gq_free_calls.argtypes = [C.POINTER(gq_calls)]
        L.gq_free_counts.argtypes = [C.POINTER(gq_counts)]
        L.gq_free_somatic.argtypes = [C.POINTER(gq_somatic_calls)]
        L.gq_reads_free.argtypes = [C.c_void_p]
        L.gq_reads_rederive.argtypes = [C.c_void_p, C.c_void_p]
        L.gq_reads_rebuild_md.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                          C.POINTER(gq_md_rebuild_info)]
        L.gq_md_rebuild_spans.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.gq_reads_missing_md.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.gq_close.argtypes = [C.c_void_p]
        vp = C.c_void_p
        for f in ("gq_bam_dev_open", "gq_bam_dev_scan", "gq_bam_dev_reads", "gq_reads_positions", "gq_reads_contig_begin",
                  "gq_reads_download"):
            getattr(L, f).restype = C.c_int
        L.gq_bam_dev_open.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
        L.gq_bam_dev_map.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.gq_bam_dev_map.restype = C.c_int
        L.gq_bam_dev_map_ex.argtypes = [C.c_char_p, C.c_int32, C.POINTER(vp)]
        L.gq_bam_dev_map_ex.restype = C.c_int
        L.gq_bam_dev_plan.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_char_p, vp]
        L.gq_bam_dev_plan.restype = C.c_int
        L.gq_bam_dev_plan_segments.argtypes = [vp, vp, vp, vp, vp]
        L.gq_bam_dev_plan_segments.restype = C.c_int
        L.gq_write_vcf_germline.argtypes = [C.c_char_p, C.c_char_p, C.c_int64] + [vp] * 9 + [C.c_int32,
                                                                                           C.POINTER(C.c_char_p)]
        L.gq_write_vcf_germline.restype = C.c_int
        L.gq_bam_dev_load.argtypes = [vp, vp]
        L.gq_bam_dev_load.restype = C.c_int
        L.gq_bam_dev_close.argtypes = [vp]
        L.gq_bam_dev_close.restype = None
        L.gq_bam_dev_header_text.argtypes = [vp]
        L.gq_bam_dev_header_text.restype = C.c_char_p
        L.gq_bam_dev_n_contigs.argtypes = [vp]
        L.gq_bam_dev_n_contigs.restype = C.c_int32
        L.gq_bam_dev_contig_name.argtypes = [vp, C.c_int32]
        L.gq_bam_dev_contig_name.restype = C.c_char_p
        L.gq_bam_dev_contig_length.argtypes = [vp, C.c_int32]
        L.gq_bam_dev_contig_length.restype = C.c_int64
        L.gq_bam_dev_scan.argtypes = [vp, vp, vp, vp]
        L.gq_bam_dev_reads.argtypes = [vp, vp, C.c_int32, vp, C.POINTER(vp), C.POINTER(C.c_float)]
        L.gq_reads_positions.argtypes = [vp, vp, vp]
        L.gq_reads_contig_begin.argtypes = [vp, vp]
        L.gq_reads_download.argtypes = [vp, C.POINTER(gq_reads)]
        for f in ("gq_sv_pairs_from_bam", "gq_sv_pairs_from_host", "gq_sv_pairs_download", "gq_sv_stats_call",
                  "gq_sv_select", "gq_sv_nodes_download", "gq_sv_graph_call", "gq_sv_cliques_call", "gq_sv_call"):
            getattr(L, f).restype = C.c_int
        L.gq_sv_pairs_from_bam.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_float)]
        L.gq_sv_pairs_from_host.argtypes = [vp, C.c_int64] + [vp] * 7 + [C.POINTER(vp)]
        L.gq_sv_pairs_count.argtypes = [vp]
        L.gq_sv_pairs_count.restype = C.c_int64
        L.gq_sv_pairs_download.argtypes = [vp] * 8
        L.gq_sv_pairs_free.argtypes = [vp]
        L.gq_sv_pairs_free.restype = None
        L.gq_sv_stats_call.argtypes = [vp, C.POINTER(gq_sv_stats)]
        L.gq_sv_select.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64)]
        L.gq_sv_nodes_download.argtypes = [vp] * 6
        L.gq_sv_graph_call.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(gq_sv_graph))]
        L.gq_sv_free_graph.argtypes = [C.POINTER(gq_sv_graph)]
        L.gq_sv_free_graph.restype = None
        L.gq_sv_cliques_call.argtypes = [C.c_int64, vp, vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int32,
                                         C.POINTER(C.POINTER(gq_sv_cliques))]
        L.gq_sv_free_cliques.argtypes = [C.POINTER(gq_sv_cliques)]
        L.gq_sv_free_cliques.restype = None
        L.gq_sv_call.argtypes = [vp, C.POINTER(gq_sv_stats), C.POINTER(C.POINTER(gq_sv_cliques)),
                                 C.POINTER(C.c_float), C.POINTER(C.c_float)]
        for f in ("gq_align_penalties", "gq_align_batch", "gq_align_host", "gq_align_reads"):
            getattr(L, f).restype = C.c_int
        L.gq_align_default_params.argtypes = [C.POINTER(gq_align_params)]
        L.gq_align_default_params.restype = None
        L.gq_align_penalties.argtypes = [C.POINTER(gq_align_params), C.POINTER(C.c_double)]
        L.gq_align_limits.argtypes = [C.POINTER(C.c_int32)]
        L.gq_align_limits.restype = None
        L.gq_align_host.argtypes = [C.c_int64] + [vp] * 6 + [C.POINTER(gq_align_params),
                                                             C.POINTER(C.POINTER(gq_alignments))]
        L.gq_align_batch.argtypes = [vp] + L.gq_align_host.argtypes
        L.gq_free_alignments.argtypes = [C.POINTER(gq_alignments)]
        L.gq_free_alignments.restype = None
        L.gq_align_reads.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, C.POINTER(gq_align_params),
                                     C.POINTER(C.POINTER(gq_alignments)), C.POINTER(C.POINTER(C.c_int64)),
                                     C.POINTER(C.POINTER(C.c_int32)), C.POINTER(gq_align_reads_info)]
        L.gq_align_free_index.argtypes = [vp]
        L.gq_align_free_index.restype = None
        for f in ("gq_asm_graphs", "gq_asm_graphs_host", "gq_asm_paths"):
            getattr(L, f).restype = C.c_int
        L.gq_asm_default_params.argtypes = [C.POINTER(gq_asm_params)]
        L.gq_asm_default_params.restype = None
        L.gq_asm_limits.argtypes = [C.POINTER(C.c_int32)]
        L.gq_asm_limits.restype = None
        L.gq_asm_graphs.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, C.POINTER(gq_asm_params),
                                    C.POINTER(C.POINTER(gq_asm_graph_block))]
        L.gq_asm_graphs_host.argtypes = [C.c_int64] + [vp] * 8 + [C.POINTER(gq_asm_params), C.c_int32,
                                                                  C.POINTER(C.POINTER(gq_asm_graph_block))]
        L.gq_asm_free_graphs.argtypes = [C.POINTER(gq_asm_graph_block)]
        L.gq_asm_free_graphs.restype = None
        L.gq_asm_paths.argtypes = [C.POINTER(gq_asm_graph_block), C.POINTER(gq_asm_params),
                                   C.POINTER(C.POINTER(gq_asm_path_block))]
        L.gq_asm_free_paths.argtypes = [C.POINTER(gq_asm_path_block)]
        L.gq_asm_free_paths.restype = None
        for f in ("gq_haplik_tables", "gq_haplik_batch", "gq_haplik_host", "gq_haplik_windows",
                  "gq_haplik_genotypes_host"):
            getattr(L, f).restype = C.c_int
        L.gq_haplik_default_params.argtypes = [C.POINTER(gq_haplik_params)]
        L.gq_haplik_default_params.restype = None
        L.gq_haplik_tables.argtypes = [C.POINTER(gq_haplik_params)] + [C.POINTER(C.c_double)] * 3
        L.gq_haplik_batch.argtypes = [vp, C.c_int64] + [vp] * 7 + [C.POINTER(gq_haplik_params),
                                                                   C.POINTER(C.POINTER(gq_haplik_pairs))]
        L.gq_haplik_host.argtypes = [C.c_int64] + [vp] * 7 + [C.POINTER(gq_haplik_params), C.c_int32,
                                                              C.POINTER(C.POINTER(gq_haplik_pairs))]
        L.gq_haplik_free_pairs.argtypes = [C.POINTER(gq_haplik_pairs)]
        L.gq_haplik_free_pairs.restype = None
        L.gq_haplik_windows.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, C.POINTER(gq_asm_params),
                                        C.POINTER(gq_asm_path_block), C.POINTER(gq_haplik_params),
                                        C.POINTER(C.POINTER(gq_haplik_block))]
        L.gq_haplik_free_block.argtypes = [C.POINTER(gq_haplik_block)]
        L.gq_haplik_free_block.restype = None
        L.gq_haplik_genotypes_host.argtypes = [C.c_int64] + [vp] * 6 + [C.c_int64, vp]
        L.gq_hapvar_limits.argtypes = [C.POINTER(C.c_int32)]
        L.gq_hapvar_limits.restype = None
        L.gq_hapvar_windows.argtypes = [vp, C.POINTER(gq_hapvar_input), C.POINTER(C.POINTER(gq_hapvar_block))]
        L.gq_hapvar_windows.restype = C.c_int
        L.gq_hapvar_host.argtypes = [C.POINTER(gq_hapvar_input), C.c_int32, C.POINTER(C.POINTER(gq_hapvar_block))]
        L.gq_hapvar_host.restype = C.c_int
        L.gq_hapvar_free_block.argtypes = [C.POINTER(gq_hapvar_block)]
        L.gq_hapvar_free_block.restype = None
        _lib = L
    return _lib


def write_vcf_germline(path: str, header: str, calls: "GermlineCalls", contig_names: Sequence[str]) -> None:
    """gq_write_vcf_germline: the header, then one line per record of `calls` (one sample)."""
    a = calls.a
    n = len(calls)
    cols = {k: np.ascontiguousarray(a[k]) for k in ("contig", "pos", "gt0", "gt1", "ref_off", "ref_len", "alt_off",
                                                   "alt_len")}
    names = (C.c_char_p * max(1, len(contig_names)))(*[x.encode() for x in contig_names])
    pool = np.frombuffer(calls.pool, np.uint8) if calls.pool else np.zeros(1, np.uint8)
    _check(lib().gq_write_vcf_germline(path.encode(), header.encode(), n, *[_ptr(cols[k]) or None for k in cols],
                                       pool.ctypes.data, len(contig_names), names))


def _check(rc: int) -> None:
    if rc != 0:
        raise GQError(rc, lib().gq_last_error().decode())


# ---- affine-gap alignment (gq_align_*) ----
E_ARG, E_CAPACITY = 7, 10


def align_params(mismatch_probability: Optional[float] = None, open_gap_probability: Optional[float] = None,
                 close_gap_probability: Optional[float] = None) -> gq_align_params:
    """gq_align_params: the library's defaults (e^-4, e^-6, 1 - e^-1) where None."""
    p = gq_align_params()
    lib().gq_align_default_params(C.byref(p))
    if mismatch_probability is not None:
        p.mismatch_probability = float(mismatch_probability)
    if open_gap_probability is not None:
        p.open_gap_probability = float(open_gap_probability)
    if close_gap_probability is not None:
        p.close_gap_probability = float(close_gap_probability)
    return p


def align_penalties(**probabilities) -> np.ndarray:
    """gq_align_penalties: the 32 step costs, [16 * (s == S) + 4 * last + next]."""
    p = align_params(**probabilities)
    t = np.zeros(32, np.float64)
    _check(lib().gq_align_penalties(C.byref(p), t.ctypes.data_as(C.POINTER(C.c_double))))
    return t


def align_limits() -> Dict[str, int]:
    """gq_align_limits: the device caps and the constants the traceback's placement depends on."""
    v = (C.c_int32 * 8)()
    lib().gq_align_limits(v)
    return dict(max_s=v[0], max_r=v[1], lanes=v[2], max_rows=v[3], lds_bytes=v[4])


def pack_pairs(sequences: Sequence[bytes], references: Sequence[bytes]):
    """Host pools and offsets of (sequence, reference) pairs, as gq_align_batch takes them."""
    if len(sequences) != len(references):
        raise ValueError("%d sequences, %d references" % (len(sequences), len(references)))

    def pool(items):
        ln = np.array([len(x) for x in items], np.int32)
        off = np.zeros(len(items), np.int64)
        if len(items) > 1:
            off[1:] = np.cumsum(ln[:-1], dtype=np.int64)
        data = np.frombuffer(b"".join(bytes(x) for x in items) or b"\0", np.uint8)
        return data, off, ln
    return pool(sequences) + pool(references)


def _alignments(out) -> Dict[str, object]:
    """A gq_alignments block copied into numpy arrays (and freed)."""
    try:
        a = out.contents
        n = int(a.n)
        take = lambda p, k, dt: np.ctypeslib.as_array(p, (k,)).astype(dt, copy=True) if k else np.zeros(0, dt)
        off = np.ctypeslib.as_array(a.cigar_off, (n + 1,)).astype(np.int64, copy=True)
        return dict(n=n, ref_start=take(a.ref_start, n, np.int32), ref_end=take(a.ref_end, n, np.int32),
                    score=take(a.score, n, np.float64), score_int=take(a.score_int, n, np.int32), cigar_off=off,
                    cigar=take(a.cigar, int(off[n]), np.uint32), ms=float(a.ms), kernel_ms=float(a.kernel_ms),
                    launches=int(a.launches))
    finally:
        lib().gq_free_alignments(out)


def _pair_args(packed):
    seq, so, sl, ref, ro, rl = packed
    return [len(sl), seq.ctypes.data, so.ctypes.data, sl.ctypes.data, ref.ctypes.data, ro.ctypes.data, rl.ctypes.data]


def align_host(packed, **probabilities) -> Dict[str, object]:
    """gq_align_host over pack_pairs' arrays: the CPU twin of Context.align_batch."""
    p = align_params(**probabilities)
    out = C.POINTER(gq_alignments)()
    _check(lib().gq_align_host(*_pair_args(packed), C.byref(p), C.byref(out)))
    return _alignments(out)


# ---- local assembly (gq_asm_*) ----
ASM_STATUS = {0: "OK", 1: "SHORT", 2: "REF_N", 3: "NO_SOURCE", 4: "NO_SINK"}
ASM_CAPS = ((16, "PATHS_CAPPED"), (32, "STEPS_CAPPED"), (64, "LENGTH_CAPPED"))


def asm_status_name(status: int) -> str:
    """A gq_asm_paths status as text: the graph's status, then the caps its search met."""
    return "|".join([ASM_STATUS[status & 15]] + [n for b, n in ASM_CAPS if status & b])


def asm_params(k: Optional[int] = None, min_occurrence: Optional[int] = None, max_paths: Optional[int] = None,
               max_path_length: Optional[int] = None, max_steps: Optional[int] = None,
               min_mapq: Optional[int] = None) -> gq_asm_params:
    """gq_asm_params: the library's defaults (k 25, 1, 10, window length - k + 65, 1,000,000) where None."""
    p = gq_asm_params()
    lib().gq_asm_default_params(C.byref(p))
    for name, v in (("k", k), ("min_occurrence", min_occurrence), ("max_paths", max_paths),
                    ("max_path_length", max_path_length), ("max_steps", max_steps), ("min_mapq", min_mapq)):
        if v is not None:
            setattr(p, name, int(v))
    return p


def asm_limits() -> Dict[str, int]:
    """gq_asm_limits: the k range and the shape of the device table."""
    v = (C.c_int32 * 8)()
    lib().gq_asm_limits(v)
    return dict(min_k=v[0], max_k=v[1], word_bases=v[2], lds_slots=v[3], lds_slots_max=v[4], threads=v[5],
                lds_bytes=v[6])


GRAPH_ARRAYS = ("node_off", "key_lo", "key_hi", "count", "child_mask", "parent_mask", "source", "sink", "status",
                "n_reads", "win_len", "n_instances")


class AsmGraphs:
    """A gq_asm_graph_block (the device's or the twin's): `a` holds numpy copies of its arrays, the
    block itself lives until this object goes, for paths()."""

    def __init__(self, ptr):
        self.ptr = ptr
        g = ptr.contents
        w, n = int(g.n_windows), int(g.n_nodes)
        take = lambda p, k: np.ctypeslib.as_array(p, (k,)).copy() if k else np.zeros(0, p._type_)
        self.n_windows, self.n_nodes, self.k, self.min_occurrence = w, n, int(g.k), int(g.min_occurrence)
        self.a = {name: take(getattr(g, name), w + 1 if name == "node_off" else n if name in GRAPH_ARRAYS[1:6] else w)
                  for name in GRAPH_ARRAYS}
        self.info = dict(ms=float(g.ms), reads_ms=float(g.reads_ms), count_ms=float(g.count_ms),
                         edges_ms=float(g.edges_ms), launches=int(g.launches), n_global=int(g.n_global))

    def __del__(self):
        if getattr(self, "ptr", None):
            lib().gq_asm_free_graphs(self.ptr)
            self.ptr = None

    def paths(self, max_paths: Optional[int] = None, max_path_length: Optional[int] = None,
              max_steps: Optional[int] = None) -> Dict[str, object]:
        """gq_asm_paths: haplotypes (offsets, bases, support), status and steps per window, unitigs."""
        p = asm_params(self.k, self.min_occurrence, max_paths, max_path_length, max_steps)
        out = C.POINTER(gq_asm_path_block)()
        _check(lib().gq_asm_paths(self.ptr, C.byref(p), C.byref(out)))
        try:
            b = out.contents
            w, nh, nu = int(b.n_windows), int(b.n_haplotypes), int(b.n_unitigs)
            take = lambda p, k: np.ctypeslib.as_array(p, (k,)).copy() if k else np.zeros(0, p._type_)
            so, uo = take(b.hap_seq_off, nh + 1), take(b.unitig_seq_off, nu + 1)
            return dict(hap_off=take(b.hap_off, w + 1), hap_seq_off=so, bases=take(b.bases, int(so[nh])).tobytes(),
                        support=take(b.support, nh), status=take(b.status, w), steps=take(b.steps, w),
                        unitig_off=take(b.unitig_off, w + 1), unitig_seq_off=uo,
                        unitig_bases=take(b.unitig_bases, int(uo[nu])).tobytes(), ms=float(b.ms))
        finally:
            lib().gq_asm_free_paths(out)


def asm_graphs_host(sequences: Sequence[bytes], window_reads: Sequence[Sequence[int]],
                    window_refs: Sequence[Optional[bytes]], window_lens: Optional[Sequence[int]] = None,
                    threads: int = 1, **params) -> AsmGraphs:
    """gq_asm_graphs_host: window w has the reads window_reads[w] (indexes into `sequences`) and the
    reference bytes window_refs[w] (None: no reference, its length then from window_lens)."""
    return asm_graphs_host_packed(asm_pack_host(sequences, window_reads, window_refs, window_lens), threads, **params)


def asm_pack_host(sequences: Sequence[bytes], window_reads: Sequence[Sequence[int]],
                  window_refs: Sequence[Optional[bytes]], window_lens: Optional[Sequence[int]] = None):
    """asm_graphs_host's arguments as gq_asm_graphs_host's arrays, for asm_graphs_host_packed."""
    seq, so, sl = pack_pairs(sequences, sequences)[:3]
    cnt = np.array([len(x) for x in window_reads], np.int64)
    roff = np.zeros(len(window_reads) + 1, np.int64)
    roff[1:] = np.cumsum(cnt)
    reads = np.array([r for x in window_reads for r in x] or [0], np.int64)
    refs = [b"" if x is None else bytes(x) for x in window_refs]
    wl = np.array([len(r) if x is not None else int(window_lens[i])
                   for i, (x, r) in enumerate(zip(window_refs, refs))] or [0], np.int32)
    ro = np.zeros(max(1, len(refs)), np.int64)
    at = 0
    for i, (x, r) in enumerate(zip(window_refs, refs)):
        ro[i] = -1 if x is None else at
        at += len(r)
    pool = np.frombuffer(b"".join(refs) or b"\0", np.uint8)
    return (len(window_reads), seq, so, sl, roff, reads, pool, ro, wl)


def asm_graphs_host_call(packed, threads: int = 1, **params):
    """The gq_asm_graphs_host call alone over asm_pack_host's arrays: the block's pointer (AsmGraphs
    takes it over)."""
    p = asm_params(**params)
    out = C.POINTER(gq_asm_graph_block)()
    _check(lib().gq_asm_graphs_host(packed[0], *[a.ctypes.data for a in packed[1:]], C.byref(p), int(threads),
                                    C.byref(out)))
    return out


def asm_graphs_host_packed(packed, threads: int = 1, **params) -> AsmGraphs:
    return AsmGraphs(asm_graphs_host_call(packed, threads, **params))


# ---- haplotype likelihoods (gq_haplik_*) ----
HL_UNDERFLOW, HL_EMPTY = 1, 2


def haplik_params(mismatch_probability: Optional[float] = None, open_gap_probability: Optional[float] = None,
                  close_gap_probability: Optional[float] = None, quality_floor: Optional[float] = None) -> gq_haplik_params:
    """gq_haplik_params: the library's defaults (e^-4, e^-6, 1 - e^-1, 6) where None."""
    p = gq_haplik_params()
    lib().gq_haplik_default_params(C.byref(p))
    for name, v in (("mismatch_probability", mismatch_probability), ("open_gap_probability", open_gap_probability),
                    ("close_gap_probability", close_gap_probability), ("quality_floor", quality_floor)):
        if v is not None:
            setattr(p, name, float(v))
    return p


def haplik_tables(**params) -> Dict[str, np.ndarray]:
    """gq_haplik_tables: trans (tMM tMI tMD tII tDD tIM tDM 0), match[256] and mismatch[256] by raw quality."""
    p = haplik_params(**params)
    t, m, x = np.zeros(8, np.float64), np.zeros(256, np.float64), np.zeros(256, np.float64)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    _check(lib().gq_haplik_tables(C.byref(p), dp(t), dp(m), dp(x)))
    return dict(trans=t, match=m, mismatch=x)


def haplik_pack(reads: Sequence[bytes], quals: Optional[Sequence[bytes]], haplotypes: Sequence[bytes]):
    """Host pools and offsets of (read, qualities, haplotype) pairs, as gq_haplik_batch takes them; quals None:
    no qualities."""
    seq, so, sl, hap, ho, hl = pack_pairs(reads, haplotypes)
    qual = None
    if quals is not None:
        if [len(q) for q in quals] != [len(r) for r in reads]:
            raise ValueError("qualities and reads differ in length")
        qual = np.frombuffer(b"".join(bytes(x) for x in quals) or b"\0", np.uint8)
    return seq, so, sl, qual, hap, ho, hl


def _haplik_args(packed):
    seq, so, sl, qual, hap, ho, hl = packed
    return [len(sl), seq.ctypes.data, so.ctypes.data, sl.ctypes.data, qual.ctypes.data if qual is not None else None,
            hap.ctypes.data, ho.ctypes.data, hl.ctypes.data]


def _haplik_pairs(out) -> Dict[str, object]:
    """A gq_haplik_pairs block copied into numpy arrays (and freed)."""
    try:
        a = out.contents
        n = int(a.n)
        take = lambda p, dt: np.ctypeslib.as_array(p, (n,)).astype(dt, copy=True) if n else np.zeros(0, dt)  # noqa: E731
        return dict(n=n, scaled=take(a.scaled, np.float64), log_likelihood=take(a.log_likelihood, np.float64),
                    flags=take(a.flags, np.uint8), ms=float(a.ms), kernel_ms=float(a.kernel_ms))
    finally:
        lib().gq_haplik_free_pairs(out)


def haplik_host(packed, threads: int = 1, **params) -> Dict[str, object]:
    """gq_haplik_host over haplik_pack's arrays: the CPU twin of Context.haplik_batch."""
    p = haplik_params(**params)
    out = C.POINTER(gq_haplik_pairs)()
    _check(lib().gq_haplik_host(*_haplik_args(packed), C.byref(p), int(threads), C.byref(out)))
    return _haplik_pairs(out)


def haplik_genotypes_host(win_read_off, hap_off, lik_off, scaled) -> Dict[str, np.ndarray]:
    """gq_haplik_genotypes_host: gt_off, gt_log_likelihood and best_genotype of the windows."""
    wro, ho, lo = (np.ascontiguousarray(x, np.int64) for x in (win_read_off, hap_off, lik_off))
    sc = np.ascontiguousarray(scaled, np.float64)
    w = len(wro) - 1
    if w < 0 or len(ho) != w + 1 or len(lo) != w + 1:
        raise ValueError("offset arrays of different lengths")
    gt_off = np.zeros(w + 1, np.int64)
    args = [w, wro.ctypes.data, ho.ctypes.data, lo.ctypes.data, sc.ctypes.data if sc.size else None, gt_off.ctypes.data]
    _check(lib().gq_haplik_genotypes_host(*args, None, 0, None))
    g = int(gt_off[w])
    gl, best = np.zeros(max(g, 1), np.float64), np.zeros(max(w, 1), np.int32)
    _check(lib().gq_haplik_genotypes_host(*args, gl.ctypes.data, g, best.ctypes.data))
    return dict(gt_off=gt_off, gt_log_likelihood=gl[:g], best_genotype=best[:w])


HAPLIK_BLOCK_ARRAYS = (("win_read_off", "w1"), ("win_reads", "n_reads"), ("lik_off", "w1"), ("scaled", "n_pairs"),
                       ("log_likelihood", "n_pairs"), ("flags", "n_pairs"), ("gt_off", "w1"),
                       ("gt_log_likelihood", "n_genotypes"), ("best_genotype", "n_windows"))


def _haplik_block(out) -> Dict[str, object]:
    """A gq_haplik_block copied into numpy arrays (and freed)."""
    try:
        b = out.contents
        size = dict(n_windows=int(b.n_windows), n_reads=int(b.n_reads), n_pairs=int(b.n_pairs),
                    n_genotypes=int(b.n_genotypes), w1=int(b.n_windows) + 1)
        take = lambda p, k: np.ctypeslib.as_array(p, (k,)).copy() if k else np.zeros(0, p._type_)  # noqa: E731
        res = {name: take(getattr(b, name), size[k]) for name, k in HAPLIK_BLOCK_ARRAYS}
        res.update(n_windows=size["n_windows"], ms=float(b.ms), reads_ms=float(b.reads_ms), kernel_ms=float(b.kernel_ms),
                   genotype_ms=float(b.genotype_ms))
        return res
    finally:
        lib().gq_haplik_free_block(out)


# ---- variants from assembled haplotypes (gq_hapvar_*) ----
HV_SNV, HV_INS, HV_DEL = 0, 1, 2
HV_KINDS = ("SNV", "INS", "DEL")
HV_HAP_UNALIGNED, HV_HAP_PARTIAL = 1, 2
HV_EDGE_DROPPED, HV_TOO_MANY_EVENTS = 1, 2
HV_NO_REF_SIDE = 1
HAPVAR_INPUT_ARRAYS = (("win_start", np.int32), ("ref_pool", np.uint8), ("ref_off", np.int64), ("win_len", np.int32),
                       ("hap_off", np.int64), ("hap_seq_off", np.int64), ("bases", np.uint8), ("hap_align", np.int64),
                       ("ref_start", np.int32), ("ref_end", np.int32), ("cigar_off", np.int64), ("cigar", np.uint32),
                       ("win_read_off", np.int64), ("lik_off", np.int64), ("scaled", np.float64))
HAPVAR_BLOCK_ARRAYS = (("ev_off", "w1"), ("pos", "e"), ("kind", "e"), ("ref_len", "e"), ("alt_off", "e"), ("alt_len", "e"),
                       ("alt_bases", "a"), ("carriers", "e"), ("gl", "e3"), ("best", "e"), ("ad_ref", "e"), ("ad_alt", "e"),
                       ("dp", "e"), ("ev_flags", "e"), ("hap_flags", "h"), ("win_flags", "w"))


def hapvar_limits() -> Dict[str, int]:
    """gq_hapvar_limits: the haplotypes a window may have, the raw-event cap and the kernels' constants."""
    v = (C.c_int32 * 8)()
    lib().gq_hapvar_limits(v)
    return dict(max_haplotypes=v[0], max_raw_events=v[1], sort_threads=v[2], lds_bytes=v[3], reads_per_pass=v[4])


def hapvar_pack(win_start, window_refs, paths: Dict[str, object], hap_align, alignments: Optional[Dict[str, object]],
                lik: Dict[str, object]) -> Dict[str, np.ndarray]:
    """The arrays of a gq_hapvar_input.  window_refs: the windows' reference bytes (None: none); paths: hap_off,
    hap_seq_off, bases; hap_align: per haplotype an index into `alignments` (ref_start, ref_end, cigar_off,
    cigar; None: no alignments) or -1; lik: win_read_off, lik_off, scaled."""
    ref_off, win_len, at = [], [], 0
    for r in window_refs:
        ref_off.append(-1 if r is None else at)
        win_len.append(0 if r is None else len(r))
        at += 0 if r is None else len(r)
    al = alignments or dict(ref_start=[], ref_end=[], cigar_off=[0], cigar=[])
    raw = dict(win_start=win_start, ref_pool=np.frombuffer(b"".join(bytes(r) for r in window_refs if r is not None), np.uint8),
               ref_off=ref_off, win_len=win_len, hap_off=paths["hap_off"], hap_seq_off=paths["hap_seq_off"],
               bases=np.frombuffer(bytes(paths["bases"]), np.uint8), hap_align=hap_align, ref_start=al["ref_start"],
               ref_end=al["ref_end"], cigar_off=al["cigar_off"], cigar=al["cigar"], win_read_off=lik["win_read_off"],
               lik_off=lik["lik_off"], scaled=lik["scaled"])
    return {n: np.ascontiguousarray(raw[n], dt) for n, dt in HAPVAR_INPUT_ARRAYS}


def hapvar_input(packed: Dict[str, np.ndarray]) -> gq_hapvar_input:
    """The struct over hapvar_pack's arrays (which the caller keeps alive)."""
    s = gq_hapvar_input(len(packed["win_start"]), len(packed["hap_seq_off"]) - 1, len(packed["ref_start"]))
    for n, _ in HAPVAR_INPUT_ARRAYS:
        setattr(s, n, packed[n].ctypes.data if packed[n].size else None)
    return s


def _hapvar_block(out) -> Dict[str, object]:
    """A gq_hapvar_block copied into numpy arrays (and freed)."""
    try:
        b = out.contents
        size = dict(w=int(b.n_windows), w1=int(b.n_windows) + 1, e=int(b.n_events), e3=3 * int(b.n_events),
                    h=int(b.n_haplotypes), a=int(b.n_alt_bases))
        take = lambda p, k: np.ctypeslib.as_array(p, (k,)).copy() if k else np.zeros(0, p._type_)  # noqa: E731
        res = {name: take(getattr(b, name), size[k]) for name, k in HAPVAR_BLOCK_ARRAYS}
        res.update(n_windows=size["w"], n_edge_dropped=int(b.n_edge_dropped), ms=float(b.ms),
                   events_ms=float(b.events_ms), marginal_ms=float(b.marginal_ms))
        return res
    finally:
        lib().gq_hapvar_free_block(out)


def hapvar_host(packed: Dict[str, np.ndarray], threads: int = 1) -> Dict[str, object]:
    """gq_hapvar_host over hapvar_pack's arrays: the CPU twin of Context.hapvar_windows."""
    out = C.POINTER(gq_hapvar_block)()
    _check(lib().gq_hapvar_host(C.byref(hapvar_input(packed)), int(threads), C.byref(out)))
    return _hapvar_block(out)


ACTIVE_DEFAULTS = dict(min_mapq=1, min_depth=4, min_evidence=2, min_percent=8, pad=75)


def active_params(**params) -> gq_active_params:
    """gq_active_params from keywords (ACTIVE_DEFAULTS where one is missing or None)."""
    unknown = set(params) - set(ACTIVE_DEFAULTS)
    if unknown:
        raise TypeError("unknown active-regions parameters: %s" % ", ".join(sorted(unknown)))
    v = {k: d if params.get(k) is None else int(params[k]) for k, d in ACTIVE_DEFAULTS.items()}
    return gq_active_params(v["min_mapq"], v["min_depth"], v["min_evidence"], v["min_percent"], v["pad"])


class ActiveRegions:
    """A gq_active_regions block as numpy columns copied out of it: the regions (``contig``, ``start``,
    ``end``, ``n_active``, ``evidence``) ascending by (contig, start), and the active loci in sorted order
    (``locus_contig``, ``locus_pos``, ``locus_depth``, ``locus_evidence``).  ``contig`` indexes the read
    set's contigs; ``end`` is not clipped to the contig's length."""

    REGION_COLUMNS = ("contig", "start", "end", "n_active", "evidence")
    LOCUS_COLUMNS = ("locus_contig", "locus_pos", "locus_depth", "locus_evidence")

    def __init__(self, cols: Dict[str, np.ndarray], visited: int = 0, listed: int = 0, block_bytes: int = 0):
        self.cols, self.visited_loci, self.listed_loci, self.block_bytes = cols, visited, listed, block_bytes

    @staticmethod
    def from_struct(c: gq_active_regions) -> "ActiveRegions":
        def col(name: str, n: int) -> np.ndarray:
            p = getattr(c, name)
            return np.ctypeslib.as_array(p, (n,)).copy() if n else np.zeros(0, p._type_)
        cols = {k: col(k, int(c.n)) for k in ActiveRegions.REGION_COLUMNS}
        cols.update({k: col(k, int(c.n_loci)) for k in ActiveRegions.LOCUS_COLUMNS})
        return ActiveRegions(cols, int(c.visited_loci), int(c.listed_loci), int(c.block_bytes))

    def __len__(self) -> int:
        return int(self.cols["start"].shape[0])

    @property
    def regions(self) -> List[tuple]:
        """(contig index, start, end, n_active, evidence) per region."""
        return list(zip(*[self.cols[k].tolist() for k in self.REGION_COLUMNS]))

    @property
    def loci(self) -> List[tuple]:
        """(contig index, pos, depth, evidence) per active locus."""
        return list(zip(*[self.cols[k].tolist() for k in self.LOCUS_COLUMNS]))


def active_regions_host(contig, pos, ref_base, depth, ref_depth, base_count, kind_count, **params) -> ActiveRegions:
    """gq_active_regions_host over pileup-count columns (PileupCounts.cols' names; rows in any order): the
    CPU twin of Context.active_regions."""
    a = [np.ascontiguousarray(x, dt) for x, dt in ((contig, np.int32), (pos, np.int64), (ref_base, np.uint8),
                                                   (depth, np.int32), (ref_depth, np.int32),
                                                   (np.asarray(base_count, np.int32).reshape(-1, 6), np.int32),
                                                   (np.asarray(kind_count, np.int32).reshape(-1, 4), np.int32))]
    n = len(a[0])
    if any(len(x) != n for x in a):
        raise ValueError("active_regions_host: columns of different lengths")
    prm = active_params(**params)
    out = C.POINTER(gq_active_regions)()
    _check(lib().gq_active_regions_host(n, *[x.ctypes.data if n else None for x in a], C.byref(prm), C.byref(out)))
    try:
        return ActiveRegions.from_struct(out.contents)
    finally:
        lib().gq_free_active_regions(out)


def _ptr(a) -> int:
    if isinstance(a, np.ndarray):
        return a.ctypes.data if a.size else 0
    return int(a.data_ptr())  # torch tensor already in device memory


def make_gq_reads(arrs: Dict[str, object]) -> Tuple[gq_reads, list]:
    """gq_reads over numpy (host) or torch (device) arrays from soa.pack/assemble."""
    keep = [arrs[k] for k in arrs]
    n = int(arrs["start"].shape[0])
    s = gq_reads(n, int(arrs["n_contigs"]), int(arrs["n_samples"]),
                 *[_ptr(arrs[k]) for k in ("contig_read_begin", "start", "end", "pmax_end", "mapq", "flags",
                                           "sample", "seq_off", "seq_len", "cigar_off", "n_cigar", "md_off", "n_md",
                                           "n_mismatch")],
                 int(arrs["seq"].shape[0]), int(arrs["cigar"].shape[0]), int(arrs["md_ev"].shape[0]),
                 *[_ptr(arrs[k]) for k in ("seq", "qual", "cigar", "md_ev")],
                 _ptr(arrs["sample_hash"]) if "sample_hash" in arrs else None)
    return s, keep


def make_gq_loci(contig, start, end, task) -> Tuple[gq_loci, list]:
    keep = [np.ascontiguousarray(contig, np.int32), np.ascontiguousarray(start, np.int64),
            np.ascontiguousarray(end, np.int64), np.ascontiguousarray(task, np.int64)]
    return gq_loci(len(keep[0]), *[_ptr(a) for a in keep]), keep


class Context:
    """One gq_ctx per GPU (gq_open / gq_close)."""

    def __init__(self, device: int = 0):
        from . import _early
        h = _early.take(device)  # the CLI's context, opened while the interpreter imported
        self.h = C.c_void_p()
        if h is not None and h.value:
            lib()
            self.h = h
        else:
            _check(lib().gq_open(int(device), C.byref(self.h)))
        self.device = device
        # germline calls reuse the context's result image: a DeviceCalls is valid until the
        # next germline call on this context (gqpileup.h, gq_calls_device)
        self.image_epoch = 0

    def close(self) -> None:
        if self.h:
            lib().gq_close(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tile(self, t: int) -> None:
        _check(lib().gq_set_tile(self.h, int(t)))

    def timings(self) -> Dict[str, float]:
        t = gq_timings()
        _check(lib().gq_get_timings(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in gq_timings._fields_}

    def proj_stats(self, reads: "DeviceReads") -> Dict[str, int]:
        """Sizes of a resident read set and of its upload-time projection (gq_reads_get_info)."""
        info = gq_reads_info()
        _check(lib().gq_reads_get_info(reads.h, C.byref(info)))
        return {k: (float if t is C.c_float else int)(getattr(info, k)) for k, t in gq_reads_info._fields_}

    def upload(self, arrs: Dict[str, object]) -> "DeviceReads":
        s, keep = make_gq_reads(arrs)
        h = C.c_void_p()
        _check(lib().gq_reads_upload(self.h, C.byref(s), C.byref(h)))
        return DeviceReads(self, h, None)

    def rederive(self, reads: "DeviceReads") -> None:
        """gq_reads_rederive: every derived structure of the resident read set dropped and the
        upload-time part derived again (the projection on the next call that reads it)."""
        _check(lib().gq_reads_rederive(self.h, reads.h))

    def rebuild_md(self, reads: "DeviceReads", dref: "DeviceReference", recompute_all: bool = False) -> Dict[str, object]:
        """gq_reads_rebuild_md: the resident read set's MD events rebuilt from the resident
        reference, for the reads without a tag or (recompute_all) for every read, by
        Read.fromSAMRecord's rule; the set is then derived again.  Raises what the host path
        (reference.rebuild_md_tags, then the MD parse) raises, naming the read's index:
        reference.ContigNotFound, ValueError (an N op), IndexError (an alignment past the contig's
        or the read's end), soa.MdParseError (a reference byte no MD tag can hold); the read set
        is then unchanged.  Returns rebuilt (reads), md_events (the new pool), ms (count + scan +
        fill on the device) and the three spans."""
        info = gq_md_rebuild_info()
        rc = lib().gq_reads_rebuild_md(self.h, reads.h, dref.h, int(bool(recompute_all)), C.byref(info))
        if rc != 0 and info.code:
            msg = lib().gq_last_error().decode()
            if info.code == 1:
                from .reference import ContigNotFound
                e = ContigNotFound("of read %d" % info.read, [])
                e.msg = msg
                e.args = (msg,)
                raise e
            if info.code == 2:
                raise ValueError(msg)
            if info.code == 3:
                raise IndexError(msg)
            from .soa import MdParseError
            raise MdParseError(msg)
        _check(rc)
        spans = (C.c_float * 3)()
        _check(lib().gq_md_rebuild_spans(self.h, spans))
        return dict(rebuilt=int(info.rebuilt), md_events=int(info.md_events), ms=float(info.ms),
                    count_ms=float(spans[0]), scan_ms=float(spans[1]), fill_ms=float(spans[2]))

    def align_batch(self, packed, **probabilities) -> Dict[str, object]:
        """gq_align_batch over pack_pairs' arrays: ref_start, ref_end, score, score_int, cigar_off, cigar
        (BAM words) per pair, the call's and the kernel's device spans (ms) and its launches."""
        p = align_params(**probabilities)
        out = C.POINTER(gq_alignments)()
        _check(lib().gq_align_batch(self.h, *_pair_args(packed), C.byref(p), C.byref(out)))
        return _alignments(out)

    def asm_graphs(self, reads: "DeviceReads", dref: "DeviceReference", contig, start, end, **params) -> AsmGraphs:
        """gq_asm_graphs: the de Bruijn graphs of the windows (contig index, [start, end)) of the
        resident reads, with source and sink from the resident reference."""
        c, s, e = (np.ascontiguousarray(x, np.int32) for x in (contig, start, end))
        p = asm_params(**params)
        out = C.POINTER(gq_asm_graph_block)()
        _check(lib().gq_asm_graphs(self.h, reads.h, dref.h, len(c), c.ctypes.data, s.ctypes.data, e.ctypes.data,
                                   C.byref(p), C.byref(out)))
        return AsmGraphs(out)

    def haplik_batch(self, packed, **params) -> Dict[str, object]:
        """gq_haplik_batch over haplik_pack's arrays: scaled, log_likelihood and flags per pair, the call's and
        the kernel's device spans (ms)."""
        p = haplik_params(**params)
        out = C.POINTER(gq_haplik_pairs)()
        _check(lib().gq_haplik_batch(self.h, *_haplik_args(packed), C.byref(p), C.byref(out)))
        return _haplik_pairs(out)

    def haplik_windows(self, reads: "DeviceReads", dref: "DeviceReference", contig, start, end, paths: Dict[str, object],
                       k: Optional[int] = None, min_mapq: Optional[int] = None, **params) -> Dict[str, object]:
        """gq_haplik_windows: the resident reads of the windows (gq_asm_graphs's selection for k and min_mapq)
        against the haplotypes of `paths` (AsmGraphs.paths() over the same windows), and the windows' genotypes:
        the block's arrays, and its spans."""
        c, s, e = (np.ascontiguousarray(x, np.int32) for x in (contig, start, end))
        ho, so = (np.ascontiguousarray(paths[n], np.int64) for n in ("hap_off", "hap_seq_off"))
        bases = np.frombuffer(bytes(paths["bases"]) or b"\0", np.uint8)
        if len(ho) != len(c) + 1:
            raise ValueError("%d windows, paths over %d" % (len(c), len(ho) - 1))
        pb = gq_asm_path_block()
        pb.n_windows, pb.n_haplotypes = len(c), len(so) - 1
        pb.hap_off = ho.ctypes.data_as(C.POINTER(C.c_int64))
        pb.hap_seq_off = so.ctypes.data_as(C.POINTER(C.c_int64))
        pb.bases = bases.ctypes.data_as(C.POINTER(C.c_uint8))
        ap = asm_params(k=k, min_mapq=min_mapq)
        p = haplik_params(**params)
        out = C.POINTER(gq_haplik_block)()
        _check(lib().gq_haplik_windows(self.h, reads.h, dref.h, len(c), c.ctypes.data, s.ctypes.data, e.ctypes.data,
                                       C.byref(ap), C.byref(pb), C.byref(p), C.byref(out)))
        return _haplik_block(out)

    def hapvar_windows(self, packed: Dict[str, np.ndarray]) -> Dict[str, object]:
        """gq_hapvar_windows over hapvar_pack's arrays: the windows' events, their carriers and genotype
        likelihoods, the haplotype and window flags and the call's spans."""
        out = C.POINTER(gq_hapvar_block)()
        _check(lib().gq_hapvar_windows(self.h, C.byref(hapvar_input(packed)), C.byref(out)))
        return _hapvar_block(out)

    def align_reads(self, reads: "DeviceReads", dref: "DeviceReference", pad: int = 32, all_reads: bool = False,
                    **probabilities) -> Dict[str, object]:
        """gq_align_reads: the resident reads with an I, D or S op (all_reads: every read; never one
        with an N or P op) against their windows of the resident reference.  align_batch's arrays,
        plus read (resident indexes), lo (window starts), n_reads, skipped and select_ms."""
        p = align_params(**probabilities)
        out = C.POINTER(gq_alignments)()
        idx, lo = C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)()
        info = gq_align_reads_info()
        _check(lib().gq_align_reads(self.h, reads.h, dref.h, int(pad), int(bool(all_reads)), C.byref(p), C.byref(out),
                                    C.byref(idx), C.byref(lo), C.byref(info)))
        try:
            k = int(info.n_selected)
            res = dict(read=np.ctypeslib.as_array(idx, (k,)).astype(np.int64, copy=True) if k else np.zeros(0, np.int64),
                       lo=np.ctypeslib.as_array(lo, (k,)).astype(np.int32, copy=True) if k else np.zeros(0, np.int32),
                       n_reads=int(info.n_reads), skipped=int(info.skipped), select_ms=float(info.select_ms))
        finally:
            lib().gq_align_free_index(idx)
            lib().gq_align_free_index(lo)
        res.update(_alignments(out))
        return res

    def missing_md(self, reads: "DeviceReads") -> int:
        """gq_reads_missing_md: reads of the resident set without MD events, counted on the device."""
        out = C.c_int64()
        _check(lib().gq_reads_missing_md(reads.h, C.byref(out)))
        return int(out.value)

    def wrap_device(self, arrs: Dict[str, object]) -> "DeviceReads":
        s, keep = make_gq_reads(arrs)
        h = C.c_void_p()
        _check(lib().gq_reads_wrap_device(self.h, C.byref(s), C.byref(h)))
        return DeviceReads(self, h, keep)

    def germline_threshold(self, reads: "DeviceReads", loci, threshold: int = 8, emit_ref: bool = False,
                           emit_no_call: bool = False) -> "GermlineCalls":
        L, keep = make_gq_loci(*loci)
        p = gq_germline_params(int(threshold), int(bool(emit_ref)), int(bool(emit_no_call)))
        out = C.POINTER(gq_calls)()
        self.image_epoch += 1
        _check(lib().gq_germline_threshold(self.h, reads.h, C.byref(L), C.byref(p), C.byref(out)))
        return GermlineCalls.from_result(out)

    def germline_threshold_device(self, reads: "DeviceReads", loci, threshold: int = 8, emit_ref: bool = False,
                                  emit_no_call: bool = False) -> "DeviceCalls":
        """gq_germline_threshold_device: the records stay in HBM (valid until the next call)."""
        L, keep = make_gq_loci(*loci)
        p = gq_germline_params(int(threshold), int(bool(emit_ref)), int(bool(emit_no_call)))
        out = gq_calls_device()
        self.image_epoch += 1
        _check(lib().gq_germline_threshold_device(self.h, reads.h, C.byref(L), C.byref(p), C.byref(out)))
        return DeviceCalls(out, self)

    def upload_reference(self, contigs: List[Optional[np.ndarray]]) -> "DeviceReference":
        """A reference genome in HBM (gq_reference_upload): contigs[k] = the unmasked bases of
        contig k of the read sets' contig list (None where the reference lacks it)."""
        keep = [None if a is None else np.ascontiguousarray(a, np.uint8) for a in contigs]
        n = len(keep)
        ptrs = (C.c_void_p * max(n, 1))(*[None if a is None else a.ctypes.data for a in keep])
        lens = np.array([-1 if a is None else len(a) for a in keep] or [0], np.int64)
        h = C.c_void_p()
        _check(lib().gq_reference_upload(self.h, n, C.cast(ptrs, C.POINTER(C.c_void_p)), lens.ctypes.data,
                                         C.byref(h)))
        return DeviceReference(h)

    def somatic_standard(self, tumor: "DeviceReads", normal: "DeviceReads", loci, reference=None,
                         **params) -> "SomaticCalls":
        """somatic-standard over the loci ranges (gq_somatic_standard, or gq_somatic_standard_ref
        with a DeviceReference).  params: the gq_somatic_params fields; defaults SOMATIC_DEFAULTS
        (the CLI defaults)."""
        L, keep = make_gq_loci(*loci)
        p = dict(SOMATIC_DEFAULTS)
        p.update(params)
        ps = gq_somatic_params(**{k: int(v) for k, v in p.items()})
        out = C.POINTER(gq_somatic_calls)()
        if reference is None:
            _check(lib().gq_somatic_standard(self.h, tumor.h, normal.h, C.byref(L), C.byref(ps), C.byref(out)))
        else:
            _check(lib().gq_somatic_standard_ref(self.h, tumor.h, normal.h, C.byref(L), reference.h, C.byref(ps),
                                                 C.byref(out)))
        return SomaticCalls.from_result(out)

    def variant_support(self, reads: "DeviceReads", loci) -> List[tuple]:
        """gq_variant_support: rows (sample index, contig index, locus, ref, alt, count, flags)."""
        L, keep = make_gq_loci(*loci)
        out = C.POINTER(gq_allele_counts)()
        _check(lib().gq_variant_support(self.h, reads.h, C.byref(L), C.byref(out)))
        try:
            c = out.contents
            n = c.n
            if n == 0:
                return []
            arr = lambda p: np.ctypeslib.as_array(p, shape=(n,)).copy()
            pool = C.string_at(c.allele_pool, c.pool_len) if c.pool_len else b""
            contig, pos, smp, cnt = arr(c.contig), arr(c.pos), arr(c.sample), arr(c.count)
            ro, rl, ao, al, fl = arr(c.ref_off), arr(c.ref_len), arr(c.alt_off), arr(c.alt_len), arr(c.flags)
            return [(int(smp[i]), int(contig[i]), int(pos[i]), pool[ro[i]:ro[i] + rl[i]].decode("latin-1"),
                     pool[ao[i]:ao[i] + al[i]].decode("latin-1"), int(cnt[i]), int(fl[i])) for i in range(n)]
        finally:
            lib().gq_free_allele_counts(out)

    def germline_standard(self, reads: "DeviceReads", loci, **params) -> "SomaticCalls":
        """germline-standard (gq_germline_standard): CalledAllele rows in the SomaticCalls layout
        (tumor = the allele's evidence, sample = its sample slot).  params: the
        gq_germline_std_params fields; defaults GERMLINE_STD_DEFAULTS (the CLI defaults)."""
        L, keep = make_gq_loci(*loci)
        p = dict(GERMLINE_STD_DEFAULTS)
        p.update(params)
        ps = gq_germline_std_params(**{k: int(v) for k, v in p.items()})
        out = C.POINTER(gq_somatic_calls)()
        _check(lib().gq_germline_standard(self.h, reads.h, C.byref(L), C.byref(ps), C.byref(out)))
        return SomaticCalls.from_result(out)

    def allele_evidence(self, reads: "DeviceReads", loci, min_mapq: int = 1,
                        variants_only: bool = True) -> "AlleleEvidenceRows":
        """gq_allele_evidence: AlleleEvidence for every distinct allele of every sample at the visited
        loci (variants_only: at the loci whose filtered pileup holds a non-Match element)."""
        L, keep = make_gq_loci(*loci)
        prm = gq_allele_evidence_params(int(min_mapq), int(bool(variants_only)))
        out = C.POINTER(gq_allele_evidence_rows)()
        _check(lib().gq_allele_evidence(self.h, reads.h, C.byref(L), C.byref(prm), C.byref(out)))
        try:
            return AlleleEvidenceRows.from_struct(out.contents)
        finally:
            lib().gq_free_allele_evidence(out)

    def genotype_likelihoods(self, reads: "DeviceReads", loci, min_mapq: int = 1, variants_only: bool = True,
                             include_alignment: bool = False, normalize: bool = True) -> "GenotypeLikelihoods":
        """gq_genotype_likelihoods_call: the log-likelihood of every diploid genotype over the eligible
        alleles of every sample at the visited loci (variants_only: at the loci whose filtered
        pileup holds a non-Match element)."""
        L, keep = make_gq_loci(*loci)
        prm = gq_genotype_likelihood_params(int(min_mapq), int(bool(variants_only)), int(bool(include_alignment)),
                                            int(bool(normalize)))
        out = C.POINTER(gq_genotype_likelihoods)()
        _check(lib().gq_genotype_likelihoods_call(self.h, reads.h, C.byref(L), C.byref(prm), C.byref(out)))
        try:
            return GenotypeLikelihoods.from_struct(out.contents)
        finally:
            lib().gq_free_genotype_likelihoods(out)

    def pileup_elements(self, reads: "DeviceReads", loci, min_mapq: int = 1,
                        variants_only: bool = True) -> "PileupElements":
        """gq_pileup_elements_call: every kept element of every visited locus' pileup in
        Pileup.elements order, with the locus' distinct alleles (variants_only: at the loci whose
        filtered pileup holds a non-Match element)."""
        L, keep = make_gq_loci(*loci)
        prm = gq_pileup_elements_params(int(min_mapq), int(bool(variants_only)))
        out = C.POINTER(gq_pileup_elements)()
        _check(lib().gq_pileup_elements_call(self.h, reads.h, C.byref(L), C.byref(prm), C.byref(out)))
        try:
            return PileupElements.from_struct(out.contents)
        finally:
            lib().gq_free_pileup_elements(out)

    def somatic_likelihoods(self, tumor: "DeviceReads", normal: "DeviceReads", loci, min_mapq: int = 1,
                            filter_multi_allelic: bool = False,
                            max_read_depth: int = 2 ** 31 - 1) -> "SomaticLikelihoods":
        """gq_somatic_likelihoods_call: both samples' normalised genotype log-likelihoods, the most
        likely tumor genotype, the normal's variant mass and the somatic log-odds at every locus that
        passes somatic-standard's gate (before it keeps one allele and applies --odds)."""
        L, keep = make_gq_loci(*loci)
        prm = gq_somatic_likelihood_params(int(min_mapq), int(bool(filter_multi_allelic)), int(max_read_depth), 0)
        out = C.POINTER(gq_somatic_likelihoods)()
        _check(lib().gq_somatic_likelihoods_call(self.h, tumor.h, normal.h, C.byref(L), C.byref(prm), C.byref(out)))
        try:
            return SomaticLikelihoods.from_struct(out.contents)
        finally:
            lib().gq_free_somatic_likelihoods(out)

    def pileup_counts_call(self, reads: "DeviceReads", loci, min_mapq: int = 1, min_depth: int = 1,
                           variants_only: bool = False) -> "PileupCounts":
        """gq_pileup_counts_call: one row per locus whose filtered pileup has depth >= max(1,
        min_depth) (variants_only: and depth > ref_depth), in call order: depth, strand-split base
        counts and element-kind counts.  (``pileup_counts`` is the dense, unfiltered histogram.)"""
        L, keep = make_gq_loci(*loci)
        prm = gq_pileup_counts_params(int(min_mapq), int(min_depth), int(bool(variants_only)), 0)
        out = C.POINTER(gq_pileup_count_rows)()
        _check(lib().gq_pileup_counts_call(self.h, reads.h, C.byref(L), C.byref(prm), C.byref(out)))
        try:
            return PileupCounts.from_struct(out.contents)
        finally:
            lib().gq_free_pileup_counts(out)

    def active_regions(self, reads: "DeviceReads", loci, **params) -> "ActiveRegions":
        """gq_active_regions_call: the regions of `loci` where the pileup shows evidence of a variant
        (gqpileup.h "active-regions").  params: active_params'."""
        L, _keep = make_gq_loci(*loci)
        prm = active_params(**params)
        out = C.POINTER(gq_active_regions)()
        _check(lib().gq_active_regions_call(self.h, reads.h, C.byref(L), C.byref(prm), C.byref(out)))
        try:
            return ActiveRegions.from_struct(out.contents)
        finally:
            lib().gq_free_active_regions(out)

    def vaf_histogram(self, reads: "DeviceReads", loci, bins: int = 20, min_read_depth: int = 0,
                      min_vaf: int = 0) -> Dict[str, object]:
        """gq_vaf_histogram: {bin start: loci} (non-empty bins), plus variant / visited locus counts."""
        L, keep = make_gq_loci(*loci)
        prm = gq_vaf_params(int(bins), int(min_read_depth), int(min_vaf))
        h = gq_vaf_hist()
        _check(lib().gq_vaf_histogram(self.h, reads.h, C.byref(L), C.byref(prm), C.byref(h)))
        return dict(histogram={b: int(h.counts[b]) for b in range(101) if h.counts[b]},
                    variant_loci=int(h.variant_loci), visited_loci=int(h.visited_loci))

    def pileup_counts(self, reads: "DeviceReads", loci) -> Dict[str, np.ndarray]:
        L, keep = make_gq_loci(*loci)
        out = C.POINTER(gq_counts)()
        _check(lib().gq_pileup_counts(self.h, reads.h, C.byref(L), C.byref(out)))
        try:
            c = out.contents
            n = c.n_loci

            def arr(p, k=1):
                return np.ctypeslib.as_array(p, shape=(n * k,)).copy() if n else np.zeros(0)

            return dict(depth=arr(c.depth), pos_depth=arr(c.pos_depth), base_counts=arr(c.base_counts, 6).reshape(-1, 6),
                        indel_counts=arr(c.indel_counts, 4).reshape(-1, 4), ref_depth=arr(c.ref_depth),
                        ref_base=arr(c.ref_base), ambiguous=arr(c.ambiguous))
        finally:
            lib().gq_free_counts(out)


class DeviceReference:
    """A gq_reference handle (freed with the object)."""

    def __init__(self, h):
        self.h = h

    def free(self) -> None:
        if self.h:
            lib().gq_reference_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceReads:
    def __init__(self, ctx: Context, h, keep):
        self.ctx, self.h, self.keep = ctx, h, keep

    def free(self) -> None:
        if self.h:
            lib().gq_reads_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceCalls:
    """Germline records left in HBM by gq_germline_threshold_device: one contiguous device image
    (``image`` address, ``image_bytes``), its array offsets, and the run counters."""

    NAMES = ("contig", "pos", "sample", "gt0", "gt1", "flags", "ref_off", "ref_len", "alt_off", "alt_len")

    def __init__(self, d: gq_calls_device, ctx: Optional["Context"] = None):
        self.ctx, self.epoch = ctx, (ctx.image_epoch if ctx is not None else None)
        c = d.calls
        self.n, self.image, self.image_bytes = int(c.n), int(d.image or 0), int(d.image_bytes)
        self.pool_len = int(c.pool_len)
        self.visited_loci, self.complex_loci = int(c.visited_loci), int(c.complex_loci)
        self.ambiguous_loci, self.tie_loci = int(c.ambiguous_loci), int(c.tie_loci)
        base = self.image
        self.offsets = {k: (C.cast(getattr(c, k), C.c_void_p).value or base) - base for k in self.NAMES}
        self.offsets["pool"] = (C.cast(c.allele_pool, C.c_void_p).value or base) - base
        self._types = {k: np.dtype(getattr(c, k)._type_) for k in self.NAMES}

    def __len__(self) -> int:
        return self.n

    def check_current(self) -> None:
        """Raise if a later germline call on the context has replaced the image."""
        if self.ctx is not None and self.ctx.image_epoch != self.epoch:
            raise GQError(7, "DeviceCalls used after a later germline call on its context (the result image "
                             "is reused; copy it first with to_host())")

    def to_host(self) -> "GermlineCalls":
        """Copy the image over PCIe (hipMemcpy) and view it as GermlineCalls (test / export)."""
        self.check_current()
        host = np.zeros(max(self.image_bytes, 1), np.uint8)
        if self.image_bytes:
            hip = C.CDLL("libamdhip64.so.7")  # by SONAME: the HIP runtime already loaded in this process
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            rc = hip.hipMemcpy(host.ctypes.data, C.c_void_p(self.image), self.image_bytes, 2)  # DeviceToHost
            if rc != 0:
                raise GQError(8, "hipMemcpy of the result image failed (%d)" % rc)
        a = {k: host[self.offsets[k]:self.offsets[k] + self.n * self._types[k].itemsize].view(self._types[k])
             for k in self.NAMES}
        pool = host[self.offsets["pool"]:self.offsets["pool"] + self.pool_len].tobytes()
        return GermlineCalls(a, pool, self.visited_loci, self.complex_loci, self.ambiguous_loci, self.tie_loci)


class GermlineCalls:
    """Germline genotype records in output order (numpy arrays; allele strings on demand)."""

    def __init__(self, arrays: Dict[str, np.ndarray], pool: bytes, visited, complex_loci, ambiguous, ties):
        self.a = arrays
        self.pool = pool
        self.visited_loci, self.complex_loci, self.ambiguous_loci, self.tie_loci = visited, complex_loci, ambiguous, ties

    @staticmethod
    def from_result(ptr) -> "GermlineCalls":
        """Zero-copy numpy views over the result block (gq_calls.block_).  The views keep
        a ctypes buffer object alive whose finalizer calls gq_free_calls."""
        import weakref

        c = ptr.contents
        n = c.n
        pool = C.string_at(c.allele_pool, c.pool_len) if c.pool_len else b""
        names = ("contig", "pos", "sample", "gt0", "gt1", "flags", "ref_off", "ref_len", "alt_off", "alt_len")
        if n == 0 or not c.block_:
            a = {k: np.zeros(0, np.dtype(getattr(c, k)._type_)) for k in names}
            out = GermlineCalls(a, pool, c.visited_loci, c.complex_loci, c.ambiguous_loci, c.tie_loci)
            lib().gq_free_calls(ptr)
            return out
        ends = [C.cast(getattr(c, k), C.c_void_p).value + n * C.sizeof(getattr(c, k)._type_) for k in names]
        size = max(ends) - c.block_
        buf = (C.c_uint8 * size).from_address(c.block_)
        weakref.finalize(buf, lib().gq_free_calls, ptr)
        a = {}
        for k in names:
            t = getattr(c, k)._type_
            a[k] = np.frombuffer(buf, dtype=np.dtype(t), count=n, offset=C.cast(getattr(c, k), C.c_void_p).value - c.block_)
        return GermlineCalls(a, pool, c.visited_loci, c.complex_loci, c.ambiguous_loci, c.tie_loci)

    IMAGE_FIELDS = (("contig", np.int32), ("pos", np.int64), ("ref_off", np.int64), ("alt_off", np.int64),
                    ("ref_len", np.int32), ("alt_len", np.int32), ("sample", np.uint8), ("gt0", np.uint8),
                    ("gt1", np.uint8), ("flags", np.uint8))

    @staticmethod
    def from_image(img: np.ndarray, n: int, visited=0, complex_loci=0, ambiguous=0, ties=0) -> "GermlineCalls":
        """Decode a result image of n records (gqpileup.h, gq_calls_device: int64 pool_len at byte
        0, then the arrays in IMAGE_FIELDS order and the pool, each on a 64-byte boundary from 64)."""
        img = np.asarray(img, np.uint8)
        al = lambda x: (x + 63) & ~63
        off, a = 64, {}
        for k, dt in GermlineCalls.IMAGE_FIELDS:
            nb = n * np.dtype(dt).itemsize
            a[k] = img[off:off + nb].view(dt).copy() if n else np.zeros(0, dt)
            off = al(off + nb)
        pool_len = int(img[:8].view(np.int64)[0]) if n else 0
        return GermlineCalls(a, img[off:off + pool_len].tobytes(), visited, complex_loci, ambiguous, ties)

    def __len__(self) -> int:
        return int(self.a["pos"].shape[0])

    def ref(self, i: int) -> str:
        o = int(self.a["ref_off"][i])
        return self.pool[o:o + int(self.a["ref_len"][i])].decode("latin-1")

    def alt(self, i: int) -> str:
        o = int(self.a["alt_off"][i])
        return self.pool[o:o + int(self.a["alt_len"][i])].decode("latin-1")

    def tuples(self, contig_names: Sequence[str]) -> List[tuple]:
        """(contig, locus, sample, (gt0, gt1), ref, alt, flags) — same shape as the oracle's rows."""
        a = self.a
        pool = self.pool
        cols = [a[k].tolist() for k in ("contig", "pos", "sample", "gt0", "gt1", "ref_off", "ref_len", "alt_off",
                                         "alt_len", "flags")]
        return [(contig_names[c], p, s, (GT_NAMES[g0], GT_NAMES[g1]), pool[ro:ro + rl].decode("latin-1"),
                 pool[ao:ao + al].decode("latin-1"), f) for c, p, s, g0, g1, ro, rl, ao, al, f in zip(*cols)]


class SomaticCalls:
    """CalledSomaticAllele records in output order: numpy columns copied out of the library's
    result (one copy per column), row dicts built on first use of ``rows``."""

    def __init__(self, cols: Dict[str, np.ndarray], pool: bytes, visited: int, candidates: int):
        self.cols, self.pool, self.visited_loci, self.candidate_loci = cols, pool, visited, candidates
        self._rows: Optional[List[dict]] = None

    COLUMNS = ("contig", "pos", "sample", "ref_off", "ref_len", "alt_off", "alt_len", "log_odds", "gq", "tumor",
               "normal", "flags")

    @staticmethod
    def from_result(ptr) -> "SomaticCalls":
        """Zero-copy numpy views over the result block (gq_somatic_calls.block_), kept alive by a
        ctypes buffer whose finalizer calls gq_free_somatic; results without a block are copied
        and freed at once."""
        import weakref

        c = ptr.contents
        n = int(c.n)
        pool = C.string_at(c.allele_pool, c.pool_len) if c.pool_len else b""
        if n == 0 or not c.block_:
            try:
                return SomaticCalls.from_struct(c, pool)
            finally:
                lib().gq_free_somatic(ptr)
        types = {k: getattr(c, k)._type_ for k in SomaticCalls.COLUMNS}
        ends = [C.cast(getattr(c, k), C.c_void_p).value + n * C.sizeof(types[k]) for k in SomaticCalls.COLUMNS]
        buf = (C.c_uint8 * (max(ends) - c.block_)).from_address(c.block_)
        weakref.finalize(buf, lib().gq_free_somatic, ptr)
        cols = {}
        for k in SomaticCalls.COLUMNS:
            dt = np.dtype(_EVIDENCE_DTYPE) if types[k] is gq_evidence else np.dtype(types[k])
            cols[k] = np.frombuffer(buf, dtype=dt, count=n, offset=C.cast(getattr(c, k), C.c_void_p).value - c.block_)
        return SomaticCalls(cols, pool, int(c.visited_loci), int(c.candidate_loci))

    @staticmethod
    def from_struct(c: gq_somatic_calls, pool: bytes) -> "SomaticCalls":
        n = int(c.n)

        def col(ptr):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0)
        cols = {k: col(getattr(c, k)) for k in SomaticCalls.COLUMNS}
        return SomaticCalls(cols, pool, int(c.visited_loci), int(c.candidate_loci))

    @property
    def rows(self) -> List[dict]:
        if self._rows is None:
            c, pool = self.cols, self.pool
            # columns to Python lists once (per-element numpy indexing cost ~25 us a row)
            L = {k: c[k].tolist() for k in ("contig", "pos", "sample", "ref_off", "ref_len", "alt_off", "alt_len",
                                            "log_odds", "gq", "flags")}
            ev = {s: list(zip(*[c[s][k].tolist() for k in EVIDENCE_FIELDS])) if len(self) else [] for s in ("tumor", "normal")}
            self._rows = [dict(contig=ct, locus=ps, sample=sm, ref=pool[ro:ro + rl].decode("latin-1"),
                               alt=pool[ao:ao + al].decode("latin-1"), log_odds=lo, gq=g, tumor=te, normal=ne, flags=fl)
                          for ct, ps, sm, ro, rl, ao, al, lo, g, fl, te, ne in
                          zip(L["contig"], L["pos"], L["sample"], L["ref_off"], L["ref_len"], L["alt_off"], L["alt_len"],
                              L["log_odds"], L["gq"], L["flags"], ev["tumor"], ev["normal"])]
        return self._rows

    def __len__(self) -> int:
        return int(self.cols["pos"].shape[0])

    COLS = ("contig", "pos", "sample", "ref_off", "ref_len", "alt_off", "alt_len", "log_odds", "gq", "tumor", "normal",
            "flags")

    def pack(self) -> np.ndarray:
        """One uint8 buffer (n, pool length, visited, candidates, the columns' raw bytes, the
        pool) for the multi-GPU gather."""
        head = np.array([len(self), len(self.pool), self.visited_loci, self.candidate_loci], np.int64)
        parts = [head.view(np.uint8)] + [np.ascontiguousarray(self.cols[k]).view(np.uint8).ravel() for k in self.COLS]
        parts.append(np.frombuffer(self.pool, np.uint8))
        return np.concatenate(parts)

    @staticmethod
    def unpack(buf: np.ndarray) -> "SomaticCalls":
        buf = np.asarray(buf, np.uint8)
        n, pl, visited, cands = (int(x) for x in buf[:32].view(np.int64))
        dts = dict(contig=np.int32, pos=np.int64, sample=np.uint8, ref_off=np.int64, ref_len=np.int32,
                   alt_off=np.int64, alt_len=np.int32, log_odds=np.float64, gq=np.int32, tumor=_EVIDENCE_DTYPE,
                   normal=_EVIDENCE_DTYPE, flags=np.uint8)
        off, cols = 32, {}
        for k in SomaticCalls.COLS:
            dt = np.dtype(dts[k])
            nb = n * dt.itemsize
            cols[k] = buf[off:off + nb].copy().view(dt)
            off += nb
        return SomaticCalls(cols, buf[off:off + pl].tobytes(), visited, cands)



class AlleleEvidenceRows:
    """gq_allele_evidence's rows in output order: numpy columns copied out of the library's
    result, row dicts built on first use of ``rows``."""

    COLUMNS = ("contig", "pos", "sample", "ref_off", "ref_len", "alt_off", "alt_len", "evidence", "flags")

    def __init__(self, cols: Dict[str, np.ndarray], pool: bytes, visited: int, listed: int):
        self.cols, self.pool, self.visited_loci, self.listed_loci = cols, pool, visited, listed
        self._rows: Optional[List[dict]] = None

    @staticmethod
    def from_struct(c: gq_allele_evidence_rows) -> "AlleleEvidenceRows":
        n = int(c.n)
        pool = C.string_at(c.allele_pool, c.pool_len) if c.pool_len else b""
        cols = {}
        for k in AlleleEvidenceRows.COLUMNS:
            t = getattr(c, k)._type_
            dt = np.dtype(_EVIDENCE_DTYPE) if t is gq_evidence else np.dtype(t)
            if n:
                buf = (C.c_uint8 * (n * dt.itemsize)).from_address(C.cast(getattr(c, k), C.c_void_p).value)
                cols[k] = np.frombuffer(buf, dtype=dt, count=n).copy()
            else:
                cols[k] = np.zeros(0, dt)
        return AlleleEvidenceRows(cols, pool, int(c.visited_loci), int(c.listed_loci))

    def __len__(self) -> int:
        return int(self.cols["pos"].shape[0])

    @property
    def rows(self) -> List[dict]:
        """dict(contig (index), locus, sample (slot), ref, alt, evidence (EVIDENCE_FIELDS order), flags)."""
        if self._rows is None:
            c, pool = self.cols, self.pool
            # columns to Python lists once, as SomaticCalls.rows
            L = {k: c[k].tolist() for k in ("contig", "pos", "sample", "ref_off", "ref_len", "alt_off", "alt_len",
                                            "flags")}
            ev = list(zip(*[c["evidence"][k].tolist() for k in EVIDENCE_FIELDS])) if len(self) else []
            self._rows = [dict(contig=ct, locus=ps, sample=sm, ref=pool[ro:ro + rl].decode("latin-1"),
                               alt=pool[ao:ao + al].decode("latin-1"), evidence=e, flags=fl)
                          for ct, ps, sm, ro, rl, ao, al, fl, e in
                          zip(L["contig"], L["pos"], L["sample"], L["ref_off"], L["ref_len"], L["alt_off"],
                              L["alt_len"], L["flags"], ev)]
        return self._rows


class GenotypeLikelihoods:
    """gq_genotype_likelihoods_call's result in output order: numpy columns copied out of the
    library's block (per group, per allele, per genotype), dicts built on first use of ``groups``
    / ``rows``."""

    GROUP_COLUMNS = ("contig", "pos", "sample", "depth", "n_alleles", "allele_first", "geno_first", "flags")
    ALLELE_COLUMNS = ("ref_off", "ref_len", "alt_off", "alt_len", "allele_depth")

    def __init__(self, cols: Dict[str, np.ndarray], pool: bytes, visited: int, listed: int):
        self.cols, self.pool, self.visited_loci, self.listed_loci = cols, pool, visited, listed
        self._groups: Optional[List[dict]] = None
        self._rows: Optional[List[dict]] = None

    @staticmethod
    def from_struct(c: gq_genotype_likelihoods) -> "GenotypeLikelihoods":
        def col(name: str, n: int) -> np.ndarray:
            dt = np.dtype(getattr(c, name)._type_)
            if not n:
                return np.zeros(0, dt)
            buf = (C.c_uint8 * (n * dt.itemsize)).from_address(C.cast(getattr(c, name), C.c_void_p).value)
            return np.frombuffer(buf, dtype=dt, count=n).copy()
        cols = {k: col(k, int(c.n_groups)) for k in GenotypeLikelihoods.GROUP_COLUMNS}
        cols.update({k: col(k, int(c.n_alleles_total)) for k in GenotypeLikelihoods.ALLELE_COLUMNS})
        cols["log_likelihood"] = col("log_likelihood", int(c.n_genotypes))
        pool = C.string_at(c.allele_pool, c.pool_len) if c.pool_len else b""
        return GenotypeLikelihoods(cols, pool, int(c.visited_loci), int(c.listed_loci))

    def __len__(self) -> int:
        return int(self.cols["pos"].shape[0])

    @property
    def n_alleles_total(self) -> int:
        return int(self.cols["ref_off"].shape[0])

    @property
    def n_genotypes(self) -> int:
        return int(self.cols["log_likelihood"].shape[0])

    @property
    def groups(self) -> List[dict]:
        """dict(contig (index), locus, sample (slot), depth, flags, alleles=[(ref, alt, depth)] in
        Allele order, log_likelihoods=[...] row-major over the allele pairs i <= j)."""
        if self._groups is None:
            c, pool = self.cols, self.pool
            L = {k: c[k].tolist() for k in self.GROUP_COLUMNS + self.ALLELE_COLUMNS}
            ll = c["log_likelihood"].tolist()
            al = [(pool[ro:ro + rl].decode("latin-1"), pool[ao:ao + an].decode("latin-1"), d)
                  for ro, rl, ao, an, d in zip(L["ref_off"], L["ref_len"], L["alt_off"], L["alt_len"], L["allele_depth"])]
            self._groups = [dict(contig=ct, locus=ps, sample=sm, depth=dp, flags=fl, alleles=al[af:af + n],
                                 log_likelihoods=ll[gf:gf + n * (n + 1) // 2])
                            for ct, ps, sm, dp, n, af, gf, fl in
                            zip(L["contig"], L["pos"], L["sample"], L["depth"], L["n_alleles"], L["allele_first"],
                                L["geno_first"], L["flags"])]
        return self._groups

    @property
    def rows(self) -> List[dict]:
        """One dict per genotype: contig (index), locus, sample (slot), allele1 / allele2 = (ref,
        alt, depth), depth, log_likelihood, flags."""
        if self._rows is None:
            rows = []
            for g in self.groups:
                al, n = g["alleles"], len(g["alleles"])
                pairs = [(i, j) for i in range(n) for j in range(i, n)]
                rows.extend(dict(contig=g["contig"], locus=g["locus"], sample=g["sample"], allele1=al[i], allele2=al[j],
                                 depth=g["depth"], log_likelihood=v, flags=g["flags"])
                            for (i, j), v in zip(pairs, g["log_likelihoods"]))
            self._rows = rows
        return self._rows


class SomaticLikelihoods:
    """gq_somatic_likelihoods_call's result in output order: numpy columns copied out of the
    library's block (per group = locus, per tumor / normal allele, per tumor / normal genotype),
    dicts built on first use of ``groups``."""

    GROUP_COLUMNS = ("contig", "pos", "flags", "tumor_ref_base", "normal_ref_base", "tumor_depth", "normal_depth",
                     "tumor_n_alleles", "normal_n_alleles", "tumor_allele_first", "normal_allele_first",
                     "tumor_geno_first", "normal_geno_first", "best", "has_variant", "normal_variant_total", "log_odds")
    ALLELE_COLUMNS = ("ref_off", "ref_len", "alt_off", "alt_len", "allele_depth")

    def __init__(self, cols: Dict[str, np.ndarray], pool: bytes, visited: int, listed: int, block_bytes: int = 0):
        self.cols, self.pool, self.visited_loci, self.listed_loci = cols, pool, visited, listed
        self.block_bytes = block_bytes
        self._groups: Optional[List[dict]] = None

    @staticmethod
    def from_struct(c: gq_somatic_likelihoods) -> "SomaticLikelihoods":
        def col(name: str, n: int) -> np.ndarray:
            dt = np.dtype(getattr(c, name)._type_)
            if not n:
                return np.zeros(0, dt)
            buf = (C.c_uint8 * (n * dt.itemsize)).from_address(C.cast(getattr(c, name), C.c_void_p).value)
            return np.frombuffer(buf, dtype=dt, count=n).copy()
        cols = {k: col(k, int(c.n_groups)) for k in SomaticLikelihoods.GROUP_COLUMNS}
        for s, na, ng in (("tumor", c.n_tumor_alleles, c.n_tumor_genotypes),
                          ("normal", c.n_normal_alleles, c.n_normal_genotypes)):
            cols.update({s + "_" + k: col(s + "_" + k, int(na)) for k in SomaticLikelihoods.ALLELE_COLUMNS})
            cols[s + "_log_likelihood"] = col(s + "_log_likelihood", int(ng))
        pool = C.string_at(c.allele_pool, c.pool_len) if c.pool_len else b""
        return SomaticLikelihoods(cols, pool, int(c.visited_loci), int(c.listed_loci), int(c.block_bytes))

    def __len__(self) -> int:
        return int(self.cols["pos"].shape[0])

    @property
    def n_genotypes(self) -> int:
        return int(self.cols["tumor_log_likelihood"].shape[0] + self.cols["normal_log_likelihood"].shape[0])

    @property
    def groups(self) -> List[dict]:
        """dict(contig (index), locus, flags, tumor_ref_base, normal_ref_base, tumor_depth,
        normal_depth, tumor_alleles / normal_alleles = [(ref, alt, depth)] in Allele order,
        tumor_log_likelihoods / normal_log_likelihoods = [...] row-major over the allele pairs
        i <= j, best (index into tumor_log_likelihoods), has_variant, normal_variant_total,
        log_odds)."""
        if self._groups is None:
            c, pool = self.cols, self.pool
            G = {k: c[k].tolist() for k in self.GROUP_COLUMNS}
            side = {}
            for s in ("tumor", "normal"):
                A = {k: c[s + "_" + k].tolist() for k in self.ALLELE_COLUMNS}
                al = [(pool[ro:ro + rl].decode("latin-1"), pool[ao:ao + an].decode("latin-1"), d)
                      for ro, rl, ao, an, d in zip(A["ref_off"], A["ref_len"], A["alt_off"], A["alt_len"],
                                                   A["allele_depth"])]
                side[s] = (al, c[s + "_log_likelihood"].tolist())
            (ta, tl), (na, nl) = side["tumor"], side["normal"]
            self._groups = [
                dict(contig=G["contig"][k], locus=G["pos"][k], flags=G["flags"][k],
                     tumor_ref_base=chr(G["tumor_ref_base"][k]), normal_ref_base=chr(G["normal_ref_base"][k]),
                     tumor_depth=G["tumor_depth"][k], normal_depth=G["normal_depth"][k],
                     tumor_alleles=ta[taf:taf + tn], normal_alleles=na[naf:naf + nn],
                     tumor_log_likelihoods=tl[tgf:tgf + tn * (tn + 1) // 2],
                     normal_log_likelihoods=nl[ngf:ngf + nn * (nn + 1) // 2],
                     best=G["best"][k], has_variant=bool(G["has_variant"][k]),
                     normal_variant_total=G["normal_variant_total"][k], log_odds=G["log_odds"][k])
                for k, (tn, nn, taf, naf, tgf, ngf) in enumerate(zip(
                    G["tumor_n_alleles"], G["normal_n_alleles"], G["tumor_allele_first"], G["normal_allele_first"],
                    G["tumor_geno_first"], G["normal_geno_first"]))]
        return self._groups


class PileupElements:
    """gq_pileup_elements_call's result in output order: numpy columns copied out of the library's
    block (per group = locus, per allele, per element), dicts built on first use of ``groups``."""

    GROUP_COLUMNS = ("contig", "pos", "ref_base", "flags", "depth", "n_alleles", "elem_first", "allele_first")
    ALLELE_COLUMNS = ("ref_off", "ref_len", "alt_off", "alt_len", "allele_depth")
    ELEMENT_COLUMNS = ("elem_read", "elem_sample", "elem_mapq", "elem_strand", "elem_kind", "elem_allele",
                       "elem_quality", "elem_read_position", "elem_cigar_index", "elem_index_within")

    def __init__(self, cols: Dict[str, np.ndarray], pool: bytes, visited: int, listed: int, block_bytes: int = 0):
        self.cols, self.pool, self.visited_loci, self.listed_loci = cols, pool, visited, listed
        self.block_bytes = block_bytes
        self._groups: Optional[List[dict]] = None

    @staticmethod
    def from_struct(c: gq_pileup_elements) -> "PileupElements":
        def col(name: str, n: int) -> np.ndarray:
            dt = np.dtype(getattr(c, name)._type_)
            if not n:
                return np.zeros(0, dt)
            buf = (C.c_uint8 * (n * dt.itemsize)).from_address(C.cast(getattr(c, name), C.c_void_p).value)
            return np.frombuffer(buf, dtype=dt, count=n).copy()
        cols = {k: col(k, int(c.n_groups)) for k in PileupElements.GROUP_COLUMNS}
        cols.update({k: col(k, int(c.n_alleles_total)) for k in PileupElements.ALLELE_COLUMNS})
        cols.update({k: col(k, int(c.n_elements)) for k in PileupElements.ELEMENT_COLUMNS})
        pool = C.string_at(c.allele_pool, c.pool_len) if c.pool_len else b""
        return PileupElements(cols, pool, int(c.visited_loci), int(c.listed_loci), int(c.block_bytes))

    def __len__(self) -> int:
        return int(self.cols["pos"].shape[0])

    @property
    def n_loci(self) -> int:
        return len(self)

    @property
    def n_alleles_total(self) -> int:
        return int(self.cols["ref_off"].shape[0])

    @property
    def n_elements(self) -> int:
        return int(self.cols["elem_read"].shape[0])

    @property
    def groups(self) -> List[dict]:
        """dict(contig (index), locus, ref_base, flags, alleles=[(ref, alt, depth)] in Allele order,
        elements=[dict(read, sample, mapq, reverse, kind, allele, quality, read_position, cigar_index,
        index_within)] in Pileup.elements order; kind is one of ELEMENT_KINDS, allele indexes alleles."""
        if self._groups is None:
            c, pool = self.cols, self.pool
            L = {k: c[k].tolist() for k in self.GROUP_COLUMNS + self.ALLELE_COLUMNS + self.ELEMENT_COLUMNS}
            al = [(pool[ro:ro + rl].decode("latin-1"), pool[ao:ao + an].decode("latin-1"), d)
                  for ro, rl, ao, an, d in zip(L["ref_off"], L["ref_len"], L["alt_off"], L["alt_len"], L["allele_depth"])]
            el = [dict(read=rd, sample=sm, mapq=mq, reverse=bool(st), kind=ELEMENT_KINDS[kd], allele=a, quality=q,
                       read_position=rp, cigar_index=ci, index_within=iw)
                  for rd, sm, mq, st, kd, a, q, rp, ci, iw in
                  zip(L["elem_read"], L["elem_sample"], L["elem_mapq"], L["elem_strand"], L["elem_kind"],
                      L["elem_allele"], L["elem_quality"], L["elem_read_position"], L["elem_cigar_index"],
                      L["elem_index_within"])]
            self._groups = [dict(contig=ct, locus=ps, ref_base=chr(rb), flags=fl, alleles=al[af:af + na],
                                 elements=el[ef:ef + dp])
                            for ct, ps, rb, fl, dp, na, ef, af in
                            zip(L["contig"], L["pos"], L["ref_base"], L["flags"], L["depth"], L["n_alleles"],
                                L["elem_first"], L["allele_first"])]
        return self._groups


class PileupCounts:
    """gq_pileup_counts_call's result in call order: numpy columns copied out of the library's block
    (``base_count`` / ``base_forward`` n x 6 in the order BASES, ``kind_count`` n x 4 in the order
    KINDS).  No per-row objects are made unless ``rows`` is asked for (small results)."""

    COLUMNS = ("contig", "pos", "ref_base", "flags", "depth", "forward_depth", "ref_depth", "base_count",
               "base_forward", "kind_count")
    WIDTH = dict(base_count=6, base_forward=6, kind_count=4)
    BASES = ("A", "C", "G", "T", "N", "other")
    KINDS = ("insertions", "deletions", "mid_deletions", "clipped")

    def __init__(self, cols: Dict[str, np.ndarray], visited: int, listed: int, block_bytes: int = 0):
        self.cols, self.visited_loci, self.listed_loci, self.block_bytes = cols, visited, listed, block_bytes
        self.contig_names: Optional[List[str]] = None  # set by commands.pileup_counts_reads

    @staticmethod
    def from_struct(c: gq_pileup_count_rows) -> "PileupCounts":
        n = int(c.n)

        def col(name: str) -> np.ndarray:
            dt, w = np.dtype(getattr(c, name)._type_), PileupCounts.WIDTH.get(name, 1)
            if not n:
                a = np.zeros(0, dt)
            else:
                buf = (C.c_uint8 * (n * w * dt.itemsize)).from_address(C.cast(getattr(c, name), C.c_void_p).value)
                a = np.frombuffer(buf, dtype=dt, count=n * w).copy()
            return a.reshape(-1, w) if w > 1 else a
        return PileupCounts({k: col(k) for k in PileupCounts.COLUMNS}, int(c.visited_loci), int(c.listed_loci),
                            int(c.block_bytes))

    @staticmethod
    def concat(parts: Sequence["PileupCounts"]) -> "PileupCounts":
        """The results of consecutive calls (runs of whole tasks, in call order) as one."""
        if len(parts) == 1:
            return parts[0]
        cols = {k: np.concatenate([p.cols[k] for p in parts]) for k in PileupCounts.COLUMNS}
        return PileupCounts(cols, sum(p.visited_loci for p in parts), sum(p.listed_loci for p in parts),
                            sum(p.block_bytes for p in parts))

    def __len__(self) -> int:
        return int(self.cols["pos"].shape[0])

    @property
    def rows(self) -> List[dict]:
        """dict(contig (its name where contig_names is set, else its index), locus, ref_base, flags,
        depth, forward_depth, ref_depth, base_count, base_forward (tuples in the order BASES),
        kind_count (tuple in the order KINDS))."""
        L = {k: self.cols[k].tolist() for k in self.COLUMNS}
        if self.contig_names is not None:
            L["contig"] = [self.contig_names[ct] for ct in L["contig"]]
        return [dict(contig=ct, locus=ps, ref_base=chr(rb), flags=fl, depth=d, forward_depth=fd, ref_depth=rd,
                     base_count=tuple(bc), base_forward=tuple(bf), kind_count=tuple(kc))
                for ct, ps, rb, fl, d, fd, rd, bc, bf, kc in zip(*[L[k] for k in self.COLUMNS])]
