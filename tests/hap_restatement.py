"""The haplotype-likelihood model restated from its specification (include/gqpileup.h, "Haplotype
likelihoods"): the forward pass and the genotype sums in plain Python floats, one rounding an
operation in the written order, the tables taken from gq_haplik_tables; a brute-force enumerator
over all alignment paths in exact fractions; and fdlibm's log (e_log.c, the published algorithm
behind java.lang.StrictMath.log), which the genotype sums take."""
import math
import struct
from fractions import Fraction

INIT = math.ldexp(1.0, 1000)
DBL_MIN = 2.2250738585072014e-308
UNDERFLOW, EMPTY = 1, 2
TMM, TMI, TMD, TII, TDD, TIM, TDM = range(7)


def priors(seq, qual, tables, mismatch_probability=None):
    """(prior on a match, prior on a mismatch) per read base; qual None: from the mismatch probability."""
    if qual is None:
        e = float(mismatch_probability)
        return [(1 - e, e / 3.0)] * len(seq)
    return [(float(tables["match"][q]), float(tables["mismatch"][q])) for q in qual]


def forward(seq, qual, hap, tables, mismatch_probability=None):
    """(scaled, flags) of one pair."""
    S, R = len(seq), len(hap)
    if S == 0 or R == 0:
        return 0.0, EMPTY
    t = [float(x) for x in tables["trans"]]
    tMM, tMI, tMD, tII, tDD, tIM, tDM = t[:7]
    pri = priors(seq, qual, tables, mismatch_probability)
    d0 = INIT / float(R)
    pm, pi, pd = [0.0] * (R + 1), [0.0] * (R + 1), [d0] * (R + 1)
    for s in range(1, S + 1):
        b = seq[s - 1]
        e_match, e_mismatch = pri[s - 1]
        cm, ci, cd = [0.0] * (R + 1), [0.0] * (R + 1), [0.0] * (R + 1)
        ci[0] = pm[0] * tMI + pi[0] * tII
        m_left = d_left = 0.0
        for r in range(1, R + 1):
            prior = e_match if b == hap[r - 1] else e_mismatch
            m = prior * ((pm[r - 1] * tMM + pi[r - 1] * tIM) + pd[r - 1] * tDM)
            ci[r] = pm[r] * tMI + pi[r] * tII
            d_left = m_left * tMD + d_left * tDD
            m_left = m
            cm[r] = m
            cd[r] = d_left
        pm, pi, pd = cm, ci, cd
    total = 0.0
    for r in range(1, R + 1):
        total = total + (pm[r] + pi[r])
    return total, (UNDERFLOW if total < DBL_MIN else 0)


def log_likelihood(scaled):
    """With the platform's log: within a few ulps of the engine's (fdlibm)."""
    return -math.inf if scaled < DBL_MIN else math.log(scaled) - 1000 * math.log(2)


def brute_force(seq, qual, hap, tables, mismatch_probability=None):
    """The sum over every alignment path, exactly: a path starts in state D at (0, r0), any r0 in 0 .. R,
    with weight INIT / R (row 0 is given, not a recurrence), steps to M at (s+1, r+1) from any state, to I
    at (s+1, r) from M or I, to D at (s, r+1) from M or D in a row s >= 1, and ends in M or I in row S at a
    column r >= 1."""
    S, R = len(seq), len(hap)
    if S == 0 or R == 0:
        return Fraction(0)
    t = [Fraction(float(x)) for x in tables["trans"]]
    to_m = {"M": t[TMM], "I": t[TIM], "D": t[TDM]}
    to_i = {"M": t[TMI], "I": t[TII]}
    to_d = {"M": t[TMD], "D": t[TDD]}
    pri = [(Fraction(a), Fraction(b)) for a, b in priors(seq, qual, tables, mismatch_probability)]
    total = Fraction(0)

    def walk(state, s, r, w):
        nonlocal total
        if s == S and state != "D" and r >= 1:
            total += w
        if s < S and r < R:
            e = pri[s][0] if seq[s] == hap[r] else pri[s][1]
            walk("M", s + 1, r + 1, w * to_m[state] * e)
        if s < S and state in to_i:
            walk("I", s + 1, r, w * to_i[state])
        if r < R and s >= 1 and state in to_d:
            walk("D", s, r + 1, w * to_d[state])

    for r0 in range(R + 1):
        walk("D", 0, r0, Fraction(INIT) / R)
    return total


# ---- fdlibm e_log.c ----
def _hi(x):
    return struct.unpack("<q", struct.pack("<d", x))[0] >> 32


def _lo(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0] & 0xFFFFFFFF


def _with_hi(x, hi):
    return struct.unpack("<d", struct.pack("<Q", (_lo(x)) | ((hi & 0xFFFFFFFF) << 32)))[0]


def strict_log(x):
    ln2_hi, ln2_lo, two54 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.80143985094819840000e+16
    Lg1, Lg2, Lg3, Lg4 = 6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01
    Lg5, Lg6, Lg7 = 1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01
    hx, lx, k = _hi(x), _lo(x), 0
    if hx < 0x00100000:
        if ((hx & 0x7fffffff) | lx) == 0:
            return -math.inf
        if hx < 0:
            return math.nan
        k -= 54
        x *= two54
        hx = _hi(x)
    if hx >= 0x7ff00000:
        return x + x
    k += (hx >> 20) - 1023
    hx &= 0x000fffff
    i0 = (hx + 0x95f64) & 0x100000
    x = _with_hi(x, hx | (i0 ^ 0x3ff00000))
    k += i0 >> 20
    f = x - 1.0
    if (0x000fffff & (2 + hx)) < 3:
        if f == 0.0:
            if k == 0:
                return 0.0
            dk = float(k)
            return dk * ln2_hi + dk * ln2_lo
        R = f * f * (0.5 - 0.33333333333333333 * f)
        if k == 0:
            return f - R
        dk = float(k)
        return dk * ln2_hi - ((R - dk * ln2_lo) - f)
    s = f / (2.0 + f)
    dk = float(k)
    z = s * s
    i = hx - 0x6147a
    w = z * z
    j = 0x6b851 - hx
    t1 = w * (Lg2 + w * (Lg4 + w * Lg6))
    t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)))
    i |= j
    R = t2 + t1
    if i > 0:
        hfsq = 0.5 * f * f
        if k == 0:
            return f - (hfsq - s * (hfsq + R))
        return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f)
    if k == 0:
        return f - s * (f - R)
    return dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f)


def genotypes(scaled, n_reads, n_haps):
    """A window's genotype log-likelihoods, (i, j) with i <= j in i-major order, and the index of the first
    largest (-1: none).  scaled: read-major, [n * H + h]."""
    if n_reads == 0 or n_haps == 0:
        return [], -1
    log_init, log_two = strict_log(INIT), strict_log(2.0)
    out = []
    for i in range(n_haps):
        for j in range(i, n_haps):
            gl = 0.0
            for n in range(n_reads):
                gl = gl + ((strict_log(scaled[n * n_haps + i] + scaled[n * n_haps + j]) - log_init) - log_two)
            out.append(gl)
    best = 0
    for g, x in enumerate(out):
        if x > out[best]:
            best = g
    return out, best
