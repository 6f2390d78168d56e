"""The cases test_gpu_proj_paths runs through the projection kernels (germline_proj, somatic_proj
and the fills and row assigners beneath them), each with what is expected of it, in one place
for proj_path_runner (the child that runs them under GQ_GERM=proj GQ_SOM=proj) and for the
parent test.  Not a test module.

A germline case is a dict  name, kind "germline", rs, loci, threshold, walk_tiles (expected),
                           tiles (expected, or None);
a somatic case             name, kind "somatic", t, n, loci, held, min_mapq, reference, forced,
                           walk_tiles, candidates (an exact count, or None: the model's bracket).
Every germline case is run with emit_ref and emit_no_call on, so every visited locus is a record.

What the expectations rest on (gq_kernels.h, gq_host.h, gq_pileup.hip, gq_germline_proj.h):
* a slice (128 loci) holds at most kSliceRowsMax = 2048 rows.  slice_rows_fifo hands slices of
  more than kRowsLdsPieces = 1024 pieces to slice_assign_rows, so both assigners meet 2048 in the
  first-fit code: a piece whose row would be 2048 sets `over`, 2048 rows themselves fit; row_count
  marks the slice pbad only on -1, and germline_proj sends a tile away on `nrows > kMaxRows`.  So
  2048 stacked reads stay on germline_proj under either assigner and 2049 go to the walker.
* pbad is per slice, but a tile is a 512-locus block and germline_proj / somatic_proj test the
  four slices' bytes at once (pbad4): one bad slice sends its whole tile, and only that tile.
* a window of more than kCell3Win = 255 reads is filled by proj_fill_deep, no walker involved.
* proj_ok refuses a read col_base_ok refuses: a byte other than A C G T N (clean = 0), no MD
  tag, 32768 loci or more.  The smallest is a 1M read whose base is R.
* the none byte of the margin projection: mproj_fill_rw marks the SLICE (mnb[slot]), somatic_proj
  reads the four marks of its block as one word (`nb`): the bound is off per tile, as in
  somatic_direct.
"""
import numpy as np

import direct_cases as dc

T = dc.T
SLICE_ROWS_MAX = 2048  # kSliceRowsMax
WIDTHS = (12, 13, 15, 16, 17, 240, 241, 255, 256, 257, 480, 481, 2047, 2048, 2049)


def _germline(name, reads, loci, threshold, n_blocks, walk_tiles=0, tiles=None):
    return dict(name=name, kind="germline", rs=reads.build(T * (n_blocks + 2)), loci=dc.ranges(loci),
                threshold=threshold, walk_tiles=walk_tiles, tiles=tiles)


def _tiles_of(loci):
    """Tiles of a list of [a, b) ranges: a tile per 512-locus block a range touches."""
    return sum((b - 1) // T - a // T + 1 for a, b in loci)


# ---------------------------------------------------------------------------------------------
# counter widths: nibbles folded every 12 rows, bytes widened every 240, the cell / deep fill
# switch at a window of 255 / 256 reads, the slice bound at 2048 / 2049 rows
# ---------------------------------------------------------------------------------------------
def width_case(n):
    """test_stack_on_the_percent_knife_edge's stacks: every base at every place, alt reads (the
    percent test passes exactly) and alt - 1 reads (it fails)."""
    threshold, alt = dc.ISSUE_PAIRS.get(n) or dc.knife_edge(n)
    assert alt * 100 >= (threshold + 1) * n > (alt - 1) * 100
    reads, loci = dc.Reads(), []
    k = 0
    for base in "ACTG":
        for place in dc.PLACES:
            for a in (alt, alt - 1):
                dc.stack(reads, loci, 2 * T * (k + 1), place, base, n, a)
                k += 1
    # one read past kSliceRowsMax: every slice of a stack is pbad, so every tile of the call walks
    # (the stacks at place T reach into the next block: two tiles each)
    walk = _tiles_of(loci) if n > SLICE_ROWS_MAX else 0
    return _germline("stack_%d" % n, reads, loci, threshold, 2 * (k + 1), walk, _tiles_of(loci))


def all_255_cases():
    """test_all_255_reads_carry_the_event's stacks: event count == count == 255."""
    reads, loci = dc.Reads(), []
    for k, base in enumerate("ACTG"):
        for v, place in enumerate((96, 103)):
            dc.stack(reads, loci, 2 * T * (2 * k + v + 1), place, base, 255, 255)
    for threshold in (8, 99):
        yield _germline("all_255_events_t%d" % threshold, reads, loci, threshold, 20)


def widths():
    for n in WIDTHS:
        yield width_case(n)
    yield from all_255_cases()


# ---------------------------------------------------------------------------------------------
# rows by interval partitioning
# ---------------------------------------------------------------------------------------------
def staggered_case():
    """64 reads of 8 bases at each of the starts s .. s + 15 in one slice (read k at s + k % 16,
    k < 64 * 16), s a multiple of 8: the reads at s fill the slice's column c alone, those at
    s + 1 .. s + 7 columns c and c + 1, so the 64 reads at s + 8 (column c + 1 alone) are the
    only ones that find freed rows.  The locus s + 11 holds the 512 reads starting at s + 4 ..
    s + 11; 128 of them carry the event (threshold 24: exactly a quarter): all 64 at s + 8, the
    last of which is the last read placed in a reused row, and 64 (63 in the second copy) at s + 9."""
    reads, loci = dc.Reads(), []
    for v, alt in enumerate((128, 127)):
        s = 2 * T * (v + 1) + 128 + 40
        lx = s + 11
        base = dc.ref_base(lx + 1)
        for j in range(16):
            ev = 64 if j == 8 else alt - 64 if j == 9 else 0
            if 64 - ev:
                reads.plain(s + j, 8, 64 - ev)
            if ev:
                reads.snv(s + j, 8, lx, base, ev)
        loci.append((s - 1, s + 24))
    assert 128 * 100 == 25 * 512
    return _germline("staggered_1024_reads", reads, loci, 24, 6)


def ladder_case():
    """One read of 8 bases per locus from block offset 370 to 520: depth 8, pieces crossing the
    slice boundary at 384 and the block boundary at 512.  Two of the eight reads over locus 385
    and two over locus 513 carry an event there (threshold 24: a quarter); both start before the
    boundary, so a piece cut at the slice's edge loses the event.  The second copy carries one."""
    reads, loci = dc.Reads(), []
    for v, alt in enumerate((2, 1)):
        B = 2 * T * (v + 1)
        carry = {}
        for edge in (384, 512):
            for j in range(alt):
                carry[B + edge - 4 + j] = B + edge + 1
        for st in range(B + 370, B + 521):
            if st in carry:
                reads.snv(st, 8, carry[st], dc.ref_base(carry[st] + 1))
            else:
                reads.plain(st, 8)
        loci.append((B + 369, B + 530))
    assert 2 * 100 == 25 * 8
    return _germline("ladder_across_slice_and_block", reads, loci, 24, 6, tiles=4)


def rows():
    yield staggered_case()
    yield ladder_case()


# ---------------------------------------------------------------------------------------------
# sparse entries past kEnt = 6 per lane
# ---------------------------------------------------------------------------------------------
def sparse_field_case():
    """500 reads of 8 bases, one per start, each with two MD mismatches (1000 entries in one
    tile: 384 ride with the records, the loop takes the rest).  The read at x - 3 and the read at
    x - 4 both read locus x as the same other base, so every inner locus holds 2 events in 8
    elements: threshold 24 passes with both and fails with one lost."""
    reads, loci = dc.Reads(), []
    B = 2 * T
    for st in range(B + 2, B + 502):
        s = dc.ref_seq(st, st + 8)
        a, b = dc.ref_base(st + 4), dc.ref_base(st + 5)  # what loci st + 3 and st + 4 are read as
        reads.add(st, s[:3] + a + b + s[5:], "8M", "3%s0%s3" % (s[3], s[4]))
    loci.append((B + 1, B + 511))
    return _germline("sparse_500_reads_1000_entries", reads, loci, 24, 4, tiles=1)


def sparse_column_case():
    """One 8-locus column with 7 entries and one with 13, mismatches and N read bases mixed.
    Threshold 19: 4 events of 20 reads and 8 of 40 pass exactly, 3 and 7 (second copies) fail;
    the N bases (3 and 5; 4 and 6 in the copies) sit on another locus of the same column."""
    reads, loci = dc.Reads(), []
    k = 0
    for n, ev, nn in ((20, 4, 3), (40, 8, 5), (20, 3, 4), (40, 7, 6)):
        k += 1
        s = 2 * T * k + 96  # a column's first locus
        lx = s + 2
        seq = dc.ref_seq(s, s + 8)
        reads.snv(s, 8, lx, dc.ref_base(lx + 1), ev)
        reads.add(s, seq[:5] + "N" + seq[6:], "8M", "8", nn)
        reads.plain(s, 8, n - ev - nn)
        loci.append((s - 1, s + 9))
    assert 4 * 100 == 20 * 20 and 8 * 100 == 20 * 40
    return _germline("sparse_columns_7_and_13", reads, loci, 19, 2 * k + 2)


def sparse():
    yield sparse_field_case()
    yield sparse_column_case()


# ---------------------------------------------------------------------------------------------
# general CIGARs, and a read the projection refuses
# ---------------------------------------------------------------------------------------------
def cigar_cases():
    reads, loci = dc.Reads(), []
    B = 2 * T
    s = B + 60
    ref = dc.ref_seq(s, s + 50)
    alt = dc.ref_base(s + 21)
    body = ref[:20] + alt + ref[21:]
    md = "20%s29" % ref[20]
    reads.add(s, "GGG" + ref, "3S50M", "50", 3)  # a leading clip
    reads.add(s, "GGG" + body, "3S50M", md, 1)
    reads.add(s, ref[:10] + "TT" + ref[10:], "10M2I40M", "50", 3)  # the locus in the second segment
    reads.add(s, body[:10] + "TT" + body[10:], "10M2I40M", md, 1)
    dc.segmented(reads, s + 5, 3, 4)  # 1M1D1M1D1M1D1M
    loci.append((s - 1, s + 51))
    for threshold in (8, 24):  # 2 events of 8 + ... elements: some pass at 8, none at 24 but the deletions
        yield _germline("general_cigars_t%d" % threshold, reads, loci, threshold, 4, tiles=1)

    # an R base (col_base_ok: clean = 0) in a 1M read on the last locus of block B: slice 3 of that
    # block is pbad, so the block's tile walks; the reads around it cross into block B + T, whose
    # tile has no bad slice and stays on germline_proj
    reads, loci = dc.Reads(), []
    x = B + T - 1
    reads.plain(x - 4, 10, 6)
    reads.snv(x - 4, 10, x + 1, dc.ref_base(x + 2), 2)  # (2 of 8 at the next block's first locus)
    reads.add(x, "R", "1M", "0%s0" % dc.ref_base(x), 1)
    reads.plain(B + 40, 10, 4)  # slice 0 of the same block: walks with it
    loci.append((B + 30, x + 8))
    yield _germline("unprojectable_1M_read", reads, loci, 24, 6, walk_tiles=1, tiles=2)


def cigars():
    yield from cigar_cases()


# ---------------------------------------------------------------------------------------------
# the tile loop: germline_proj splits the tiles statically, workgroup b taking n_tiles / gridDim.x
# consecutive ones and wave w of it every fourth.  germline_grid gives min(ceil(tiles / 4),
# resident workgroups, kPartsCols = 2048) workgroups, so a wave takes a second tile only once the
# grid is capped, and 8 * 2048 = 16384 tiles is the smallest count that gives every wave of every
# workgroup two tiles whatever the occupancy query answers (8192 where it answers 4 per CU on 256
# CUs; the count must not depend on that answer).
# ---------------------------------------------------------------------------------------------
def tile_loop():
    kinds = dc.tile_kinds()
    rs, loci = dc.germline_tiles(kinds)
    # kind b holds a byte other than A C G T N: its tile walks.  Kind g's read without MD lies in
    # the uncalled block behind its tile, whose slices no tile reads.
    yield dict(name="16384_tiles", kind="germline", rs=rs, loci=loci, threshold=8, walk_tiles=kinds.count("b"),
               tiles=dc.N_TILES)


def panel():
    """test_deep_panel_500x_germline's read set (12 kb at 500x: blocks of ~550 projection rows)."""
    from guacamole_amd.synthetic import generate
    rs = generate(12_000, 500.0, seed=5, indel_rate=3e-4).to_read_set()
    loci = (np.array([0], np.int32), np.array([0], np.int64), np.array([rs.contig_lengths[0]], np.int64),
            np.array([0], np.int64))
    for t in (2, 8):
        yield dict(name="panel_500x_t%d" % t, kind="germline", rs=rs, loci=loci, threshold=t, walk_tiles=0, tiles=None)


# ---------------------------------------------------------------------------------------------
# somatic: the bound grid over the margin projection
# ---------------------------------------------------------------------------------------------
SOMATIC_ARRANGEMENTS = ("plain", "lead_3S", "second_segment", "column_last", "block_last", "block_first",
                        "min_mapq_20")


def _somatic(name, t, n, loci, held, min_mapq=1, reference=None, forced=0, walk_tiles=0, candidates=None):
    return dict(name=name, kind="somatic", t=t, n=n, loci=loci, held=held, min_mapq=min_mapq, reference=reference,
                forced=forced, walk_tiles=walk_tiles, candidates=candidates)


def grid_limits(cases):
    """The deepest pileup of the grid as the projection sees it (rows of a slice, reads of a
    window): min_mapq_20 doubles every case's reads."""
    return 2 * max(len(c) for c in cases)


def somatic():
    """walk_tiles 0 throughout: the grid's deepest case is 600 reads (1200 with the mapq-5 reads of
    min_mapq_20), under kSliceRowsMax; its reads are M, 3S..M and 10M2I40M, all of which proj_ok
    takes; the windows past kCell3Win (241, 300, 600 reads) are the deep fill's, and the slices
    past kRowsLdsPieces (min_mapq_20 at 600) first-fit's: neither is a walker."""
    cases = dc.grid_cases()
    assert grid_limits(cases) <= SLICE_ROWS_MAX
    for name in SOMATIC_ARRANGEMENTS:
        arr = dc.ARRANGEMENTS[name]
        t, n, loci, where, held = dc.bound_sets(cases, **arr)
        yield _somatic(name, t, n, loci, held, min_mapq=20 if arr.get("low_mapq") else 1)
    # test_bound_with_reference_fasta on plain: the reference disagrees at the odd cases
    t, n, loci, where, held = dc.bound_sets(cases)
    ref = dc.ref_array(t.contig_lengths[0])
    odd = np.array(where[1::2])
    ref[odd] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), ref[odd])]
    yield _somatic("plain_reference_fasta", t, n, loci, held[0::2], reference=ref, forced=len(odd))
    # test_none_element_turns_off_its_tile_only: the mark is per slice, the test per block (= tile)
    t, n, loci, expect = dc.none_tiles(64)
    assert expect == 3 * 22
    yield _somatic("none_element_64_tiles", t, n, loci, None, candidates=expect)


GROUPS = {"widths": widths, "rows": rows, "sparse": sparse, "cigars": cigars, "tile_loop": tile_loop, "panel": panel,
          "somatic": somatic}
