"""Variants from assembled haplotypes on the CPU: the host twin (gq_hapvar_host) against the restatement
(hapvar_restatement.py) field for field and gl bit for bit on the hand-built cases, each builder's
precondition from the twin alone, the comparison's power to discriminate, the ABI, and the VCF / TSV
writers on a fixed block.  (test_gpu_hapvar.py compares the device with the twin.)"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import hapvar_cases as HV
import hapvar_restatement as V
from conftest import ROOT
from guacamole_amd import native, variants_assembly as VA


@pytest.fixture(scope="module")
def cases():
    return HV.all_cases()


@pytest.fixture(scope="module")
def twin(cases):
    return {name: native.hapvar_host(HV.pack(ws)) for name, ws in cases.items()}


def test_twin_equals_the_restatement(cases, twin):
    assert native.hapvar_limits()["max_raw_events"] == HV.CAP and native.hapvar_limits()["max_haplotypes"] == 64
    for name, ws in cases.items():
        HV.same_block(twin[name], V.block(ws, HV.CAP))
    batch = HV.shuffled_batch(cases)
    one = native.hapvar_host(HV.pack(batch), threads=1)
    HV.same_block(one, V.block(batch, HV.CAP))
    HV.same_block(native.hapvar_host(HV.pack(batch), threads=3), one)


def test_case_preconditions(cases, twin):
    keys = lambda name, w: HV.event_keys(twin[name], w)  # noqa: E731
    snv = cases["snv"]
    assert keys("snv", 0) == [(17, 0, 1, bytes([HV.other(snv[0]["ref"][17])]))]
    assert [k[0] for k in keys("snv", 1)] == [1010, 1011, 1012]          # an X run of 3: three events
    assert [k[0] for k in keys("snv", 2)] == [0, 39]                     # the first and the last offset
    assert list(twin["snv"]["carriers"][6:8]) == [0b110, 0b100]          # a shared event: two carrier bits
    same = keys("snv", 4)
    assert [k[0] for k in same] == [5, 5] and same[0][3] < same[1][3]     # one offset, two ALTs, in byte order
    assert keys("snv", 5) == [] and twin["snv"]["ev_off"][5] == twin["snv"]["ev_off"][6]
    # every indel normalises to the repeat's start, whatever its CIGAR said: the case that is meant to shift does
    indel = twin["indel"]
    assert len(cases["indel"]) == 16 and len(indel["pos"]) == 16
    for w in range(16):
        first, unit = (7, b"C") if w < 8 else (6, b"GA")
        ref = cases["indel"][w]["ref"]
        (pos, kind, ref_len, alt), = keys("indel", w)
        cigar_at = cases["indel"][w]["aligns"][1][2][0] >> 4
        assert pos == first - 1 and cigar_at == first + (0, 1, 2 * len(unit), 3 * len(unit))[w % 8 // 2]
        if w % 2 == 0:
            assert (kind, ref_len, alt) == (native.HV_INS, 1, ref[first - 1:first] + unit)
        else:
            assert (kind, ref_len, alt) == (native.HV_DEL, 1 + len(unit), ref[first - 1:first])
    stopped = twin["stopped"]
    assert keys("stopped", 0) == [(8, 0, 1, b"G"), (8, 1, 1, b"CC")]      # the X base stops the shift and anchors it
    assert keys("stopped", 1) == [(7, 2, 2, b"T"), (10, 1, 1, b"CCC")]    # the deletion stops the insertion behind it
    assert keys("stopped", 2) == [] and keys("stopped", 3) == []
    assert stopped["n_edge_dropped"] == 4 and list(stopped["win_flags"]) == [0, 0, 1, 1]
    order = twin["order"]
    assert [(k[0], k[1]) for k in keys("order", 0)] == [(13, 0), (13, 1), (13, 2)]  # SNV, INS, DEL at one anchor
    assert list(order["carriers"][:3]) == [0b100, 0b010, 0b001]
    a, b = keys("order", 1)
    assert a[:3] == b[:3] and a[3][:-1] == b[3][:-1] and a[3][-1] < b[3][-1]
    assert list(order["carriers"][3:]) == [0b0100, 0b1001]
    usable = twin["usable"]
    assert list(usable["hap_flags"]) == [1, 0, 2, 0, 1, 0, 0, 1, 0, 2, 0]
    assert list(usable["carriers"]) == [0b10, 0b100000, 0b100000, 0b101, 0b1]
    assert list(usable["ev_flags"]) == [0, 0, 0, 1, 1] and list(usable["gl"][9::3][:2]) == [-math.inf] * 2
    empty = twin["empty"]
    assert list(np.diff(empty["ev_off"])) == [0, 1, 0, 0] and list(empty["gl"]) == [0.0] * 3 and empty["best"][0] == 0
    assert list(empty["hap_flags"]) == [0, 0, 1, 1] and twin["nothing_but_empty"]["pos"].size == 0
    assert [len(w["haps"]) for w in cases["hap_counts"]] == [1, 2, 10, 63, 64]
    assert twin["hap_counts"]["carriers"][-1] == 1 << 63 and list(twin["hap_counts"]["ev_flags"][:1]) == [1]
    assert list(twin["read_counts"]["dp"][::2]) == [1, 63, 64, 65, 128, 129, 200]
    values = twin["values"]
    assert list(values["ad_ref"]) == [3, 3] and list(values["ad_alt"]) == [2, 2] and list(values["dp"]) == [6, 7]  # the tie counts for neither
    # a read with a 0 on one side puts that homozygote at -infinity; a read with both sides 0 all three
    assert list(np.isfinite(values["gl"][:3])) == [False, True, False] and list(values["gl"][3:]) == [-math.inf] * 3
    raw = lambda name: sum(bin(int(c)).count("1") for c in twin[name]["carriers"])  # noqa: E731
    assert (raw("below_cap"), raw("at_cap"), raw("over_cap")) == (HV.CAP - 1, HV.CAP, 0)
    assert [list(twin[n]["win_flags"]) for n in ("below_cap", "at_cap", "over_cap")] == [[0], [0], [2]]
    many = twin["many"]
    assert len(cases["many"]) == 300 and 1300 < many["pos"].size < 1700 and set(many["kind"]) == {0, 1, 2}


def test_comparison_discriminates(twin):
    def fails(want, change):
        bad = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in want.items()}
        change(bad)
        with pytest.raises(AssertionError):
            HV.same_block(bad, want)

    want = twin["order"]
    HV.same_block({k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in want.items()}, want)

    def swap_events(b):
        for name in ("kind", "ref_len", "alt_len", "carriers"):
            b[name][[1, 2]] = b[name][[2, 1]]

    def flip_bit(b):
        b["carriers"][0] ^= 2

    def one_ulp(b):
        b["gl"][4] = np.nextafter(b["gl"][4], 0.0)

    def shift_ev_off(b):
        b["ev_off"][1] += 1

    for change in (swap_events, flip_bit, one_ulp, shift_ev_off):
        fails(want, change)


def test_abi_and_argument_errors(cases):
    assert C.sizeof(native.gq_hapvar_input) == 144 and C.sizeof(native.gq_hapvar_block) == 192
    names = {"gq_hapvar_limits", "gq_hapvar_windows", "gq_hapvar_host", "gq_hapvar_free_block"}
    assert all(hasattr(native.lib(), n) for n in names) and names <= set(native.EXPORTED)
    lim = native.hapvar_limits()
    assert lim["lds_bytes"] == 16 * lim["max_raw_events"] <= 64 * 1024 and lim["reads_per_pass"] == 64

    def rejected(change, code=native.E_ARG):
        packed = HV.pack(cases["snv"])
        change(packed)
        with pytest.raises(native.GQError) as e:
            native.hapvar_host(packed)
        assert e.value.code == code
        return str(e.value)

    def set_at(name, i, v):
        def change(p):
            p[name][i] = v
        return change

    rejected(set_at("win_len", 0, -1))
    rejected(set_at("hap_align", 1, 99))
    rejected(set_at("hap_align", 1, -2))
    rejected(set_at("hap_seq_off", 1, 90))     # a haplotype of negative length behind it
    assert "CIGAR of haplotype 1" in rejected(set_at("cigar", 1, 16 << 4 | 7))  # one base short of the window
    rejected(set_at("cigar", 1, 17 << 4 | 3))  # an N op
    packed = HV.pack(HV.too_many_haplotypes(HV.rng(5)))
    out = C.POINTER(native.gq_hapvar_block)()
    rc = native.lib().gq_hapvar_host(C.byref(native.hapvar_input(packed)), 1, C.byref(out))
    assert rc == native.E_CAPACITY and not out and "window 0" in native.lib().gq_last_error().decode()
    none = native.hapvar_host(HV.pack([]))
    assert none["n_windows"] == 0 and list(none["ev_off"]) == [0] and none["pos"].size == 0


def test_command_is_registered():
    from guacamole_amd import commands
    assert "germline-assembly" in commands.COMMANDS
    with pytest.raises(SystemExit):
        commands.COMMANDS["germline-assembly"](["--help"])


# ---- the writers on a fixed block ----
def fixed_rows():
    """Two overlapping windows of chrB and one of chrA (the contig list puts chrA first)."""
    windows = [("chrB", 0, 20), ("chrB", 10, 30), ("chrA", 0, 20)]
    refs = [b"ACGTACGTACGTACGTACGT", b"GTACGTACGTACGTACGTAC", b"TTTTTTTTTTGGGGGGGGGG"]
    ln10 = math.log(10)
    block = dict(
        ev_off=[0, 2, 4, 6], pos=[12, 14, 12, 15, 3, 10], kind=[0, 2, 0, 1, 0, 0], ref_len=[1, 3, 1, 1, 1, 1],
        alt_off=[0, 1, 2, 3, 6, 7], alt_len=[1, 1, 1, 3, 1, 1], alt_bases=b"TGTTCCAC",
        carriers=[1, 6, 1, 2, 1, 3],
        gl=[-30.0, -2.0, -25.0,   -10.0 * ln10, -1.0 * ln10, 0.0,   -31.0, -3.0, -26.0,   -5.0, -40.0, -50.0,
            -math.inf, -7.0, -1.5,   -math.inf, -math.inf, -math.inf],
        best=[1, 2, 1, 0, 2, 0], ad_ref=[4, 0, 5, 9, 0, 0], ad_alt=[5, 8, 4, 0, 6, 0], dp=[9, 8, 9, 9, 6, 2],
        ev_flags=[0, 0, 0, 0, 1, 1])
    block = {k: (v if isinstance(v, bytes) else np.array(v)) for k, v in block.items()}
    block["alt_bases"] = np.frombuffer(block["alt_bases"], np.uint8)
    return VA.event_rows(block, windows, refs), windows


def test_writers_on_a_fixed_block():
    rows, windows = fixed_rows()
    assert [(r["ref"], r["alt"]) for r in rows] == [("A", "T"), ("GTA", "G"), ("A", "T"), ("T", "TCC"), ("T", "A"), ("G", "C")]
    lines = VA.event_tsv_lines(rows)
    assert lines[0] == "chrB\t0\t20\t12\tSNV\tA\tT\t0\t-30.0\t-2.0\t-25.0\t0/1\t4\t5\t9\t0"
    assert lines[1].split("\t")[7] == "1,2" and lines[4].split("\t")[8:11] == ["-inf", "-7.0", "-1.5"]
    assert VA.EVENT_HEADER.count("\t") == lines[0].count("\t")
    calls = VA.select_calls(rows, ["chrA", "chrB"])
    # chrA first (the contig list's order); chrB:12 A>T once, from window 0 (|12 - 10| = 2 < |12 - 20| = 8); the 0/0
    # insertion is left out; the all -infinity event is 0/0
    assert [(r["contig"], r["pos"], r["window"]) for r in calls] == [("chrA", 3, 2), ("chrB", 12, 0), ("chrB", 14, 0)]
    assert VA.vcf_line(calls[1]) == "chrB\t13\t.\tA\tT\t121.60\t.\tNH=1;WS=0\tGT:AD:DP:GQ:PL\t0/1:4,5:9:99:122,0,100"
    assert VA.vcf_line(calls[2]) == "chrB\t15\t.\tGTA\tG\t100.00\t.\tNH=2;WS=0\tGT:AD:DP:GQ:PL\t1/1:0,8:8:10:100,10,0"
    assert VA.vcf_line(calls[0]) == "chrA\t4\t.\tT\tA\t.\t.\tNH=1;WS=0\tGT:AD:DP:GQ:PL\t1/1:0,6:6:24:2147483647,24,0"
    for r in rows:
        pl, gq, qual = V.pl_gq_qual(r["gl"], r["best"])
        fields = VA.vcf_line(r).split("\t")
        assert fields[9].split(":")[3:] == [str(gq), ",".join(map(str, pl))]
        assert fields[5] == ("." if qual is None else "%.2f" % qual)
    every = VA.select_calls(rows, ["chrA", "chrB"], emit_all=True)
    assert [(r["contig"], r["pos"], r["alt"]) for r in every] == [("chrA", 3, "A"), ("chrA", 10, "C"), ("chrB", 12, "T"),
                                                                  ("chrB", 14, "G"), ("chrB", 15, "TCC")]
    assert VA.vcf_line(every[1]).split("\t")[5] == "." and VA.vcf_line(every[4]).split("\t")[5] == "0.00"
    assert [r["pos"] for r in VA.select_calls(rows, ["chrA", "chrB"], min_qual=110)] == [3, 12]  # an infinite QUAL passes
    # the tie: an event as far from both centres comes from the first window
    tie = [dict(rows[0], pos=15, window=0), dict(rows[2], pos=15, window=1)]
    assert [r["window"] for r in VA.select_calls(tie, ["chrB"])] == [0]
    text = VA.vcf_text(calls, "s1", {"chrA": 20, "chrB": 30})
    head = [l for l in text.splitlines() if l.startswith("#")]
    assert head[0] == "##fileformat=VCFv4.1" and head[-1].endswith("FORMAT\ts1") and len(text.splitlines()) == len(head) + 3
    for tag in ("##FORMAT=<ID=GT", "##FORMAT=<ID=AD", "##FORMAT=<ID=DP", "##FORMAT=<ID=GQ", "##FORMAT=<ID=PL", "##INFO=<ID=NH",
                "##INFO=<ID=WS", "##contig=<ID=chrB,length=30>"):
        assert any(l.startswith(tag) for l in head), tag


def test_stand_alone_program(tmp_path):
    """tests/native/hapvar_check.cpp over the host twin, built with g++ (a sanitizer build of the same file is
    run by hand, see its head)."""
    exe = str(tmp_path / "hapvar_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "hapvar_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
