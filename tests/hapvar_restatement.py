"""Variants from assembled haplotypes restated from the contract (include/gqpileup.h, "Variants from
assembled haplotypes") in plain Python: the CIGAR as alignment columns, left-normalisation by moving an
indel's columns, the sort, the dedup, the carrier masks, the maxima and the genotype sums with
hap_restatement.strict_log.  A case is a list of windows, each a dict: start, ref (bytes or None), haps
(bytes each), aligns (per haplotype None or (ref_start, ref_end, CIGAR words)), scaled (N rows of H)."""
import math

from hap_restatement import INIT, strict_log

SNV, INS, DEL = 0, 1, 2
HAP_UNALIGNED, HAP_PARTIAL = 1, 2
EDGE_DROPPED, TOO_MANY_EVENTS = 1, 2
NO_REF_SIDE = 1
OPS = {7: "=", 8: "X", 1: "I", 2: "D"}


def columns(words):
    """One alignment column per base: (op, window offset or None, haplotype offset or None)."""
    cols, p, q = [], 0, 0
    for word in words:
        op = OPS[int(word) & 15]
        for _ in range(int(word) >> 4):
            cols.append((op, None if op == "I" else p, None if op == "D" else q))
            p += op != "I"
            q += op != "D"
    return cols


def haplotype_events(words, ref, hap):
    """([(offset, ref_len, alt_len, ALT bytes)], dropped) of a usable haplotype."""
    cols = columns(words)
    events, dropped, i = [], 0, 0
    while i < len(cols):
        op, p, q = cols[i]
        if op == "=":
            i += 1
        elif op == "X":
            events.append((p, 1, 1, hap[q:q + 1]))
            i += 1
        else:
            j = i
            while j < len(cols) and cols[j][0] == op:  # (two ops of one kind never touch in a run-length CIGAR)
                j += 1
            length = j - i
            seq = (lambda c: hap[c[2]]) if op == "I" else (lambda c: ref[c[1]])
            block = [seq(c) for c in cols[i:j]]
            at = i  # the block's first column; a matched column before it that equals its last base swaps sides
            while at > 0 and cols[at - 1][0] == "=" and ref[cols[at - 1][1]] == block[-1]:
                block = [block[-1]] + block[:-1]
                at -= 1
            before = sum(1 for c in cols[:at] if c[0] != "I")  # window bases in front of the indel
            if before == 0:
                dropped += 1
            elif op == "I":
                events.append((before - 1, 1, length + 1, ref[before - 1:before] + bytes(block)))
            else:
                events.append((before - 1, length + 1, 1, ref[before - 1:before]))
            i = j
    return events, dropped


def kind_of(ref_len, alt_len):
    return SNV if (ref_len, alt_len) == (1, 1) else INS if ref_len == 1 else DEL


def event_likelihoods(scaled, n_haps, carriers, rest):
    """(gl[3], best, ad_ref, ad_alt) over the rows of scaled."""
    log_init, log_two = strict_log(INIT), strict_log(2.0)
    gl, ad_ref, ad_alt = [0.0, 0.0, 0.0], 0, 0
    for row in scaled:
        alt = max(row[h] for h in range(n_haps) if carriers >> h & 1)
        ref = max([row[h] for h in range(n_haps) if rest >> h & 1], default=0.0)
        for g, (x, y) in enumerate(((ref, ref), (ref, alt), (alt, alt))):
            gl[g] = gl[g] + ((strict_log(x + y) - log_init) - log_two)
        ad_ref += ref > alt
        ad_alt += alt > ref
    best = 0
    for g in (1, 2):
        if gl[g] > gl[best]:
            best = g
    return gl, best, ad_ref, ad_alt


def block(windows, cap):
    """The whole output block as lists, keyed as native._hapvar_block's arrays."""
    out = {k: [] for k in ("pos", "kind", "ref_len", "alt_off", "alt_len", "carriers", "gl", "best", "ad_ref", "ad_alt",
                           "dp", "ev_flags", "hap_flags", "win_flags")}
    out["ev_off"], out["alt_bases"], out["n_edge_dropped"] = [0], b"", 0
    for win in windows:
        ref, haps, n_haps = win["ref"], win["haps"], len(win["haps"])
        usable, found, raw, flags = 0, {}, 0, 0
        for h, (hap, al) in enumerate(zip(haps, win["aligns"])):
            if al is None or ref is None:
                out["hap_flags"].append(HAP_UNALIGNED)
                continue
            if al[0] != 0 or al[1] != len(ref):
                out["hap_flags"].append(HAP_PARTIAL)
                continue
            out["hap_flags"].append(0)
            usable |= 1 << h
            events, dropped = haplotype_events(al[2], ref, hap)
            out["n_edge_dropped"] += dropped
            flags |= EDGE_DROPPED if dropped else 0
            raw += len(events)
            for ev in events:
                found[ev] = found.get(ev, 0) | 1 << h
        if raw > cap:
            flags |= TOO_MANY_EVENTS
            found = {}
        out["win_flags"].append(flags)
        for ev in sorted(found):  # (offset, ref_len, alt_len, bytes): bytes compare as unsigned
            off, ref_len, alt_len, alt = ev
            carriers = found[ev]
            rest = usable & ~carriers
            gl, best, ad_ref, ad_alt = event_likelihoods(win["scaled"], n_haps, carriers, rest)
            out["pos"].append(win["start"] + off)
            out["kind"].append(kind_of(ref_len, alt_len))
            out["ref_len"].append(ref_len)
            out["alt_off"].append(len(out["alt_bases"]))
            out["alt_len"].append(alt_len)
            out["alt_bases"] += alt
            out["carriers"].append(carriers)
            out["gl"] += gl
            out["best"].append(best)
            out["ad_ref"].append(ad_ref)
            out["ad_alt"].append(ad_alt)
            out["dp"].append(len(win["scaled"]))
            out["ev_flags"].append(0 if rest else NO_REF_SIDE)
        out["ev_off"].append(len(out["pos"]))
    return out


def pl_gq_qual(gl, best):
    """(PL[3], GQ, QUAL or None when infinite) as the VCF writer states them."""
    top = max(gl)
    pl = [2 ** 31 - 1 if g == -math.inf else min(2 ** 31 - 1, int(round(10 * (top - g) / math.log(10)))) for g in gl]
    gq = min(99, sorted(pl)[1])
    qual = 10 * (gl[best] - gl[0]) / math.log(10)
    return pl, gq, None if math.isinf(qual) or math.isnan(qual) else qual
