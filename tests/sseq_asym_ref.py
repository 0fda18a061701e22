"""High-precision reference of the asymptotic (beta) branch of the sSeq test (dist.rs:226-257), the checker of
`special::betainc`, `special::betaincinv` and `special::nb_asymptotic` (scan-rs_amd/csrc/special.hpp).

I_x(a, b) comes from the all-positive series

    I_x(a, b) = x^a (1-x)^b / (a B(a, b)) * sum_n prod_{j<n} (a+b+j) x / (a+1+j)

on the side x (a+b+2) < a+1 and from 1 - I_{1-x}(b, a) on the other, with 1 - x formed exactly. ln B is mpmath.loggamma's,
the prefactor is evaluated at PREC bits. The sum has no cancellation, so it is accumulated in fixed point (python integers,
FIXED bits below the leading term 1): a, b and x enter as the exact rationals their doubles are, a + b is exact, and every
term loses at most one unit of 2^-FIXED to truncation. The sum stops when the rigorous bound of the remaining tail,
term * r / (1 - r) with r = max(term ratio, x) < 1, is below 2^-150 (< 1e-45) of the sum; at TermCapExceeded it gives no value.

`mpmath.betainc` is not used: it does not converge at these parameters. scipy is used only for the starting point of the
median's Newton iteration, which then runs on the series.
"""
from __future__ import annotations

import math

import mpmath
import numpy as np
from mpmath import mpf

PREC = 320  # bits of the mpmath context
FIXED = 256  # fixed-point bits of the series' sum
XBITS = 128  # a non-double x (the median's iterates) is rounded to this many bits
SCALE = 64  # a, b >= 2^-11 are integers after * 2^SCALE
TERM_CAP = 2_000_000
STOP_BITS = 150  # 2^-150 = 7e-46
TIE_DISTANCE = 1e-12


class TermCapExceeded(ArithmeticError):
    """The series needs more terms than the cap allows: no value."""


def _fixed(v: float) -> int:
    s = v * 2.0 ** SCALE
    i = int(s)
    if not (v > 0.0 and math.isfinite(v) and float(i) == s and i / 2.0 ** SCALE == v):
        raise ValueError(f"{v!r} is not a positive double that * 2^{SCALE} makes an integer")
    return i


def _series(a: float, b: float, x, cap: int):
    """sum_n prod_{j<n} (a+b+j) x / (a+1+j) as an mpf, and the number of terms. x: mpf in (0, 1) with x (a+b+2) < a+1."""
    A, B, one = _fixed(a), _fixed(b), 1 << SCALE
    _, man, exp, _ = x._mpf_
    man, exp = int(man), int(exp)
    if exp >= 0:
        raise ValueError("x must be below 1")
    sh = -exp
    # a cheap proof that the cap cannot be enough: term_cap >= min(r_0, x)^cap, sum <= 1 / (1 - max(r_0, x))
    xf = float(x)
    r0 = (a + b) * xf / (a + 1.0)
    rmin, rmax = min(r0, xf), max(r0, xf)
    if rmax < 1.0 and rmin > 0.0 and cap * math.log(rmin) + math.log1p(-rmax) > -45.0 * math.log(10.0) + 1.0:
        raise TermCapExceeded(f"a={a!r} b={b!r} x={xf!r}: more than {cap} terms")
    xfix = (man << FIXED) >> sh  # x in FIXED bits, rounded down
    num, den = (A + B) * man, A + one
    step_n, step_d = one * man, one
    T = 1 << FIXED
    s = T
    n = 0
    while True:
        Tn = (T * num // den) >> sh
        num += step_n
        den += step_d
        n += 1
        s += Tn
        if Tn < T and (Tn << STOP_BITS) < s:
            # ratio r_n = Tn / T < 1; the later ratios lie between r_n and x
            r = max((Tn << FIXED) // T + 1, xfix + 1)
            if r < (1 << FIXED) and ((Tn * r // ((1 << FIXED) - r)) << STOP_BITS) < s:
                break
        T = Tn
        if Tn == 0:
            break
        if n >= cap:
            raise TermCapExceeded(f"a={a!r} b={b!r} x={xf!r}: more than {cap} terms")
    return mpf(s) / mpf(2) ** FIXED, n


def _as_mpf(x):
    """x as an mpf: a float exactly, an mpf rounded to XBITS."""
    if isinstance(x, (float, np.floating)):
        return mpf(float(x))
    with mpmath.workprec(XBITS):
        return +mpf(x)


def _log_prefactor(a, b, x):
    """ln[x^a (1-x)^b / B(a, b)]"""
    a, b = mpf(a), mpf(b)
    return a * mpmath.log(x) + b * mpmath.log1p(-x) - (mpmath.loggamma(a) + mpmath.loggamma(b) - mpmath.loggamma(a + b))


def betainc_terms(a: float, b: float, x, cap: int = TERM_CAP):
    """(I_x(a, b) as an mpf, number of series terms). a, b: doubles; x: a double (taken exactly) or an mpf."""
    with mpmath.workprec(PREC):
        x = _as_mpf(x)
        if not 0 < x < 1:
            raise ValueError("x must lie in (0, 1)")
        lp = _log_prefactor(a, b, x)
        if x * (mpf(a) + mpf(b) + 2) < mpf(a) + 1:
            s, n = _series(a, b, x, cap)
            return mpmath.exp(lp) * s / mpf(a), n
        # here x >= (a+1)/(a+b+2) >= 2^-25: the lowest bit of x is far above 2^-PREC, so 1 - x is formed without rounding
        if -int(x._mpf_[2]) > PREC - 2:
            raise ValueError("1 - x is not exact at this precision")
        y = 1 - x
        s, n = _series(b, a, y, cap)
        return 1 - mpmath.exp(lp) * s / mpf(b), n


def betainc(a: float, b: float, x, cap: int = TERM_CAP):
    return betainc_terms(a, b, x, cap)[0]


def beta_density(a: float, b: float, x):
    """x^(a-1) (1-x)^(b-1) / B(a, b)"""
    with mpmath.workprec(PREC):
        x = _as_mpf(x)
        return mpmath.exp(_log_prefactor(a, b, x)) / (x * (1 - x))


def beta_median(a: float, b: float, cap: int = TERM_CAP):
    """x with I_x(a, b) = 1/2 to about XBITS bits: Newton on the series from scipy's betaincinv."""
    from scipy.special import betaincinv

    with mpmath.workprec(PREC):
        x = mpf(float(betaincinv(a, b, 0.5)))
        if not 0 < x < 1:
            raise ValueError("no starting point")
        for _ in range(12):
            x = _as_mpf(x)
            step = (betainc(a, b, x, cap) - mpf(1) / 2) / beta_density(a, b, x)
            xn = x - step
            if not 0 < xn < 1:
                raise ArithmeticError(f"the median's Newton step left (0, 1): a={a!r} b={b!r}")
            x = xn
            if abs(step) < mpf(2) ** -(XBITS - 12) * x:
                return _as_mpf(x)
        raise ArithmeticError(f"the median's Newton iteration did not settle: a={a!r} b={b!r}")


def alpha_beta(sf_a: float, sf_b: float, mu: float, phi: float):
    """alpha and beta in double, as special.hpp and tests/sseq_ref.py round them"""
    alpha = sf_a * mu / (1.0 + phi * mu)
    beta = (sf_b / sf_a) * alpha
    return alpha, beta


def nb_asymptotic(count_a: int, count_b: int, sf_a: float, sf_b: float, mu: float, phi: float, median=None, cap: int = TERM_CAP):
    """dist.rs:226-257 on the series. Returns a dict: p (mpf), p_lower = 2 I_qa(alpha, beta) and p_upper = 2 I_qb(beta, alpha) (the
    p-value on either side of the `qa < median` decision), median (mpf) and distance = |qa - median| / median."""
    alpha, beta = alpha_beta(sf_a, sf_b, mu, phi)
    xa, xb = float(count_a), float(count_b)
    if int(xa) != count_a or int(xb) != count_b:
        raise ValueError("the counts must be exact in double")
    qa = (xa + 0.5) / (xa + xb)
    qb = (xb + 0.5) / (xa + xb)
    with mpmath.workprec(PREC):
        if median is None:
            median = beta_median(alpha, beta, cap)

        def cdf(a, b, q):
            return mpf(0) if q < 0 else mpf(1) if q > 1 else betainc(a, b, q, cap)

        p_lower, p_upper = 2 * cdf(alpha, beta, qa), 2 * cdf(beta, alpha, qb)
        return dict(p=p_lower if mpf(qa) < median else p_upper, p_lower=p_lower, p_upper=p_upper, median=median,
                    distance=abs(mpf(qa) - median) / median, alpha=alpha, beta=beta, qa=qa, qb=qb)


# ---- the continued fraction's loop, restated for its iteration count ---------------------------------------------------------------
BETACF_CAP = 200000


def beta_excess(a, b, x):
    """special.hpp's beta_excess, x (a+b) - a, correctly rounded (the library's differs by its last bit at most)"""
    from fractions import Fraction

    return np.array([float(Fraction(float(xi)) * (Fraction(float(ai)) + Fraction(float(bi))) - Fraction(float(ai))) for ai, bi, xi in zip(a, b, x)])


def betacf_iterations(a, b, x, n=None):
    """special.hpp's betacf, line for line, over arrays: (f, iterations). An entry that reaches BETACF_CAP did not converge."""
    a, b, x = (np.atleast_1d(np.asarray(v, dtype=np.float64)).copy() for v in (a, b, x))
    n = beta_excess(a, b, x) if n is None else np.atleast_1d(np.asarray(n, dtype=np.float64)).copy()
    tiny, eps = 1e-300, 1e-16
    idx = np.arange(len(a))
    f_out, it_out = np.zeros(len(a)), np.zeros(len(a), dtype=np.int64)

    def floor_tiny(v):
        return np.where(np.abs(v) < tiny, tiny, v)

    with np.errstate(all="ignore"):
        f = floor_tiny(a * (1.0 - n) / (a + 1.0))
        c, d = f.copy(), np.zeros(len(a))
        for m in range(1, BETACF_CAP + 1):
            den = a + 2.0 * m - 1.0
            am = (a + m - 1.0) * (a + b + m - 1.0) * m * (b - m) * x * x / (den * den)
            bm = m + m * (b - m) * x / den + (a + m) * (1.0 - n + m * (2.0 - x)) / (den + 2.0)
            d = 1.0 / floor_tiny(bm + am * d)
            c = floor_tiny(bm + am / c)
            dl = c * d
            f = f * dl
            done = np.abs(dl - 1.0) < eps
            if m == BETACF_CAP:
                done[:] = True
            if done.any():
                f_out[idx[done]], it_out[idx[done]] = f[done], m
                keep = ~done
                if not keep.any():
                    break
                idx, a, b, x, n, c, d, f = (v[keep] for v in (idx, a, b, x, n, c, d, f))
    return f_out, it_out


def betainc_cf_iterations(a, b, x):
    """the iterations of the one betacf call that special.hpp's betainc(a, b, x) makes (0 where it makes none)"""
    a, b, x = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (a, b, x))
    inside = (x > 0.0) & (x < 1.0)
    low = x * (a + b + 2.0) < a + 1.0
    n = beta_excess(a, b, x)
    aa, bb, xx, nn = np.where(low, a, b), np.where(low, b, a), np.where(low, x, 1.0 - x), np.where(low, n, -n)
    it = np.zeros(len(a), dtype=np.int64)
    if inside.any():
        it[inside] = betacf_iterations(aa[inside], bb[inside], xx[inside], nn[inside])[1]
    return it


def regime(a: float, b: float) -> str:
    """which branch of special.hpp's log_beta_pf serves (a, b), and the size of a + b, with which every rounding of x or of a + b
    itself weighs on ln of the prefactor (S: below 1e4, M: below 1e6, L: from 1e6)"""
    lo, hi = min(a, b), max(a, b)
    if hi < 15.0:
        return "small"
    return ("mixed" if lo < 15.0 else "stirling") + ("-S" if a + b < 1e4 else "-M" if a + b < 1e6 else "-L")
