"""genotype-likelihoods without a GPU: the library's exports and struct layouts, the CSV writer, the
CLI's refusals, and the oracle's self-consistency that the GPU tests
(test_gpu_genotype_likelihoods.py) lean on: a germline-standard row's likelihood is exp of the
first maximum of likelihoods_at (log space, normalized) over the reads the mapq filter keeps."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

from conftest import ROOT, fixture
from guacamole_amd import native
from guacamole_amd.commands import COMMANDS, GENOTYPE_LIKELIHOODS_HEADER, main, write_genotype_likelihoods_csv
from guacamole_amd.reads import load_reads
from oracle import oracle as O

from test_allele_evidence import FILTERS, first_pileup_zone, in_zone, kept, loci_of


def covering(rs, contig, locus, sample=None):
    """The reads of rs covering the locus (of one sample), input order kept: what Pileup.apply takes."""
    m = ((np.asarray(rs.contig) == rs.contig_index()[contig]) & (np.asarray(rs.start) <= locus) &
         (np.asarray(rs.end) > locus))
    if sample is not None:
        m &= np.asarray(rs.sample) == sample
    return rs.subset(np.nonzero(m)[0])


def strict_exp(x):
    """java.lang.StrictMath.exp (fdlibm e_exp.c) for -745 < x < 2**-28: the exp the reference takes of
    the chosen log-likelihood.  math.exp is the C library's, which differs from it in the last bit
    at about one argument in a hundred."""
    ln2hi, ln2lo, invln2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00
    p1, p2, p3, p4, p5 = (1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05,
                          -1.65339022054652515390e-06, 4.13813679705723846039e-08)
    assert -745.0 < x < 2.0 ** -28
    hx = (struct.unpack("<Q", struct.pack("<d", x))[0] >> 32) & 0x7FFFFFFF
    hi = lo = 0.0
    k = 0
    if hx > 0x3FD62E42:  # |x| > 0.5 ln2
        if hx < 0x3FF0A2B2:  # and |x| < 1.5 ln2
            hi, lo, k = x + ln2hi, -ln2lo, -1
        else:
            k = int(invln2 * x - 0.5)
            hi, lo = x - k * ln2hi, k * ln2lo
        x = hi - lo
    elif hx < 0x3E300000:  # |x| < 2**-28
        return 1.0 + x
    t = x * x
    c = x - t * (p1 + t * (p2 + t * (p3 + t * (p4 + t * p5))))
    if k == 0:
        return 1.0 - ((x * c) / (c - 2.0) - x)
    y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi)
    return math.ldexp(y, k) if k >= -1021 else math.ldexp(y, k + 1000) * 9.33263618503218878990e-302


def test_library_exports_genotype_likelihoods():
    L = native.lib()
    names = {"gq_genotype_likelihoods_call", "gq_free_genotype_likelihoods"}
    assert all(hasattr(L, n) for n in names) and names <= set(native.EXPORTED)


def test_struct_sizes_equal_the_headers_static_asserts():
    hdr = open(os.path.join(ROOT, "include", "gqpileup.h")).read()
    sizes = {m.group(1): int(m.group(2)) for m in re.finditer(r"static_assert\(sizeof\((\w+)\) == (\d+)", hdr)}
    assert sizes["gq_genotype_likelihood_params"] == 16 and sizes["gq_genotype_likelihoods"] == 176
    for name in ("gq_genotype_likelihood_params", "gq_genotype_likelihoods"):
        assert C.sizeof(getattr(native, name)) == sizes[name], name


def test_csv_writer(tmp_path):
    nan, inf = float("nan"), float("inf")
    groups = [dict(contig="chr1", locus=7, sample=0, depth=10, flags=0, alleles=[("A", "A", 7), ("A", "C", 3)],
                   log_likelihoods=[-12.5, -0.1 - 0.2, -inf]),
              dict(contig="chr1", locus=7, sample=1, depth=4, flags=1, alleles=[("A", "ACGT", 4)], log_likelihoods=[nan]),
              dict(contig="2", locus=2 ** 31 + 5, sample=5, depth=2, flags=0, alleles=[("AT", "A", 1), ("T", "", 1)],
                   log_likelihoods=[inf, 0.0, -1e-300])]
    out = tmp_path / "rows.csv"
    write_genotype_likelihoods_csv(str(out), groups, ["s0", "s1"])
    lines = out.read_text().splitlines()
    assert lines[0] == GENOTYPE_LIKELIHOODS_HEADER and len(GENOTYPE_LIKELIHOODS_HEADER.split(",")) == 12
    assert lines[1:] == ["chr1,7,s0,A,A,A,A,10,7,7,-12.5,0",
                         "chr1,7,s0,A,A,A,C,10,7,3,-0.30000000000000004,0",
                         "chr1,7,s0,A,C,A,C,10,3,3,-Infinity,0",
                         "chr1,7,s1,A,ACGT,A,ACGT,4,4,4,NaN,1",
                         "2,2147483653,default,AT,A,AT,A,2,1,1,Infinity,0",
                         "2,2147483653,default,AT,A,T,,2,1,1,0.0,0",
                         "2,2147483653,default,T,,T,,2,1,1,-1e-300,0"]
    assert float(lines[2].split(",")[10]) == -0.1 - 0.2  # doubles read back to the same bits
    with pytest.raises(FileExistsError):
        write_genotype_likelihoods_csv(str(out), groups, ["s0", "s1"])


def test_cli_refuses_existing_out_and_multi_rank(tmp_path, monkeypatch):
    assert "genotype-likelihoods" in COMMANDS
    out = tmp_path / "rows.csv"
    out.write_text("keep me\n")
    with pytest.raises(FileExistsError):
        main(["genotype-likelihoods", "--reads", fixture("chrM.sorted.bam"), "--out", str(out)])
    assert out.read_text() == "keep me\n"
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="single process"):
        main(["genotype-likelihoods", "--reads", fixture("chrM.sorted.bam"), "--out", str(tmp_path / "new.csv")])
    assert not (tmp_path / "new.csv").exists()


def test_oracle_called_likelihood_is_the_first_maximum_of_likelihoods_at():
    """chrM, 3 tasks, min_mapq 1: at every germline-standard locus past its task's first-pileup zone
    whose reference base is not heap-order dependent, exp(max(likelihoods_at(kept reads covering
    the locus, log space, normalized))) equals the row's likelihood within 1e-12 (the reference's
    LikelihoodSuite tolerance), and bit for bit at 95 % of them or more."""
    min_mapq = 1
    rs = load_reads(fixture("chrM.sorted.bam"), FILTERS)
    loci = loci_of(rs, "chrM:0-16571", 3)
    rows = O.germline_standard(rs, loci, apply_filters=0, min_mapq=min_mapq)
    zones = first_pileup_zone(rs, loci)
    sub = kept(rs, min_mapq)
    idx = rs.contig_index()
    done, equal, excluded = set(), 0, 0
    for r in rows:
        if (r["flags"] & 1) or in_zone(zones, idx[r["contig"]], r["locus"]):
            excluded += 1
            continue
        if (r["contig"], r["locus"]) in done:  # (a hom-alt or two-allele call gives two rows)
            assert r["tumor"][0] == last
            continue
        done.add((r["contig"], r["locus"]))
        ll = O.likelihoods_at(covering(sub, r["contig"], r["locus"]), r["contig"], r["locus"], log_space=True,
                              normalize=True)
        want = math.exp(max(v for _, v in ll))
        last = r["tumor"][0]
        assert abs(want - last) <= 1e-12, (r["contig"], r["locus"], want, last)
        equal += want == last
    assert len(done) > 100 and equal >= 0.95 * len(done), (len(done), equal, excluded)


def test_strict_exp_is_the_oracles_exp():
    """The port above against the oracle's own exp: likelihoods_at returns exp(x) of the values it
    returns in log space, so strict_exp of each log value must give the plain value's bits (the C
    library's exp, math.exp, does not at every value); and strict_exp of the first maximum is a
    germline-standard row's likelihood bit for bit at every compared locus."""
    rs = load_reads(fixture("chrM.sorted.bam"), FILTERS)
    n = libm_differs = 0
    for locus in range(3000, 3300):
        sub = covering(rs, "chrM", locus)
        for normalize in (True, False):
            logs = O.likelihoods_at(sub, "chrM", locus, log_space=True, normalize=normalize)
            plain = O.likelihoods_at(sub, "chrM", locus, log_space=False, normalize=normalize)
            for (_, x), (_, y) in zip(logs, plain):
                if -745.0 < x < 2.0 ** -28:
                    assert strict_exp(x) == y, (locus, x, strict_exp(x), y)
                    n += 1
                    libm_differs += math.exp(x) != y
    assert n > 500 and libm_differs > 0, (n, libm_differs)
    loci = loci_of(rs, "chrM:0-16571", 3)
    zones = first_pileup_zone(rs, loci)
    sub = kept(rs, 1)
    checked = 0
    for r in O.germline_standard(rs, loci, apply_filters=0, min_mapq=1):
        if (r["flags"] & 1) or in_zone(zones, 0, r["locus"]):
            continue
        ll = O.likelihoods_at(covering(sub, r["contig"], r["locus"]), r["contig"], r["locus"], log_space=True,
                              normalize=True)
        assert strict_exp(max(v for _, v in ll)) == r["tumor"][0], (r["locus"], r["tumor"][0])
        checked += 1
    assert checked > 100
