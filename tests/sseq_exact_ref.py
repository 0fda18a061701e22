"""High-precision reference of the exact branch of the sSeq test (nb_exact_test, dist.rs:74-118 and 259-310), the checker of
`special::nb_term` / `special::nb_add_total` and of both exact backends (scan-rs_amd/csrc/special.hpp, sseq.hip, sseq_ratio.inc,
sseq_host.cpp). It looks at nothing of the library.

The conditional distribution of x_a given x_a + x_b = n has the terms

    T(k) ~ Γ(sar + k) Γ(sbr + n - k) / (k! (n - k)!),   k = 0 .. n,   r = 1 / phi, sar = sf_a r, sbr = sf_b r

(mu enters every term through one common factor and leaves p). The doubles sf_a, sf_b and phi are taken exactly, r, sar and sbr are
formed at PREC bits, and the n + 1 terms are taken relative to T(0) by the step

    T(k+1) / T(k) = (sar + k) (n - k) / ((k + 1) (sbr + n - k - 1)),

n steps of four multiplications and a division, each rounded at PREC = 320 bits: the terms carry more than 90 digits at n = 1e5. p is the
sum of the terms <= the observed one over the sum of all. With sf_a == sf_b the terms k and n - k are equal in exact arithmetic; the
mirror term n - x_a is then put into the extreme set by construction and not by a comparison of rounded numbers.

More than `cap` terms raise TermCapExceeded: no value.
"""
from __future__ import annotations

import math

import mpmath
import numpy as np
from mpmath import mpf

PREC = 320  # bits of the mpmath context, as in tests/sseq_asym_ref.py
TERM_CAP = 200_000
TIE_DISTANCE = 1e-12  # |ln(T(k) / T(x_a))| below which the side of `<=` is decided by rounding in double precision
_PREFILTER = 1e-6  # double-precision screen before the distance is taken at PREC bits

_cache: dict = {}


class TermCapExceeded(ArithmeticError):
    """The test has more terms than the cap allows: no value."""


def degenerate(x_a, x_b, sf_a, sf_b, phi):
    """the three guards of dist.rs:76-86"""
    return x_a + x_b == 0 or phi == 0.0 or sf_a == 0.0 or sf_b == 0.0


def shape(sf_a: float, sf_b: float, phi: float):
    """(r, sar, sbr) at PREC bits from the doubles"""
    with mpmath.workprec(PREC):
        r = 1 / mpf(float(phi))
        return r, mpf(float(sf_a)) * r, mpf(float(sf_b)) * r


def terms(n: int, sf_a: float, sf_b: float, phi: float, cap: int = TERM_CAP):
    """[T(k) / T(0) for k = 0 .. n] as mpf (the last call's list is kept)"""
    n = int(n)
    if n + 1 > cap:
        raise TermCapExceeded(f"n = {n}: more than {cap} terms")
    key = (n, float(sf_a), float(sf_b), float(phi))
    if key not in _cache:
        _cache.clear()
        with mpmath.workprec(PREC):
            _, sar, sbr = shape(sf_a, sf_b, phi)
            t = [mpf(1)]
            for k in range(n):
                t.append(t[-1] * ((sar + k) * (n - k)) / ((k + 1) * (sbr + (n - k - 1))))
        _cache[key] = t
    return _cache[key]


def _float_logs(t):
    """ln of every term in double (absolute error ~1e-16 |ln T|): the screen for near ties"""
    out = np.empty(len(t))
    for i, v in enumerate(t):
        _, man, exp, bc = v._mpf_
        man = int(man)
        sh = max(bc - 64, 0)
        out[i] = math.log(man >> sh) + (exp + sh) * math.log(2.0)
    return out


def log_span(n: int, sf_a: float, sf_b: float, mu: float, phi: float) -> float:
    """S: the largest over k of |lnΓ(sar+k) - lnΓ(sar)| + |lnΓ(sbr+n-k) - lnΓ(sbr)| + lnΓ(k+1) + lnΓ(n-k+1), plus |n ln(mu/(r+mu))| +
    |(sf_a+sf_b) ln(r/(r+mu))|: the sizes of the six doubles a log-space term is made of. A size, not a value: double precision serves
    (the ln Γ differences are running sums of logarithms, which do not cancel)."""
    n = int(n)
    r = 1.0 / phi
    sar, sbr = sf_a * r, sf_b * r
    j = np.arange(n, dtype=np.float64)
    with np.errstate(all="ignore"):
        ga = np.concatenate([[0.0], np.cumsum(np.log(sar + j))])
        gb = np.concatenate([[0.0], np.cumsum(np.log(sbr + j))])
        lf = np.concatenate([[0.0], np.cumsum(np.log(j + 1.0))])
        per_k = np.abs(ga) + np.abs(gb[::-1]) + lf + lf[::-1]
        const = abs(n * math.log(mu / (r + mu))) + abs((sf_a + sf_b) * math.log(r / (r + mu)))
    return float(per_k.max() + const)


def nb_exact(x_a: int, x_b: int, sf_a: float, sf_b: float, mu: float, phi: float, cap: int = TERM_CAP):
    """dist.rs:74-118 at PREC bits. Returns a dict: p (mpf; terms <= the observed one over all terms), p_lower / p_upper (without / with every
    k != x_a whose term lies within TIE_DISTANCE of the observed one), distance (min over k != x_a of |ln(T(k) / T(x_a))|), log_span and
    mirror (sf_a == sf_b and n - x_a != x_a: the mirror term is in p by construction)."""
    x_a, x_b = int(x_a), int(x_b)
    if degenerate(x_a, x_b, sf_a, sf_b, phi):
        return dict(p=mpf(1), p_lower=mpf(1), p_upper=mpf(1), distance=math.inf, log_span=0.0, mirror=False)
    n = x_a + x_b
    t = terms(n, sf_a, sf_b, phi, cap)
    mirror = float(sf_a) == float(sf_b) and n - x_a != x_a
    with mpmath.workprec(PREC):
        obs = t[x_a]
        ext = [v <= obs for v in t]
        if mirror:
            ext[n - x_a] = True
        lf = _float_logs(t)
        d = np.abs(lf - lf[x_a])
        d[x_a] = np.inf
        near = [int(k) for k in np.flatnonzero(d < _PREFILTER + 1e-13 * np.abs(lf[x_a]))]
        exact = {k: float(abs(mpmath.log(t[k] / obs))) for k in near}
        distance = min(exact.values()) if exact else float(d.min())
        tie = [k for k, v in exact.items() if v < TIE_DISTANCE]
        total = mpmath.fsum(t)
        s_ext = mpmath.fsum(v for v, e in zip(t, ext) if e)
        s_lo = s_ext - mpmath.fsum(t[k] for k in tie if ext[k])
        s_hi = s_ext + mpmath.fsum(t[k] for k in tie if not ext[k])
        return dict(p=s_ext / total, p_lower=s_lo / total, p_upper=s_hi / total, distance=distance,
                    log_span=log_span(n, sf_a, sf_b, mu, phi), mirror=mirror)


def log_terms(x_a: int, n: int, sf_a: float, sf_b: float, phi: float, cap: int = TERM_CAP):
    """ln T(k) - ln T(x_a) for k = 0 .. n as doubles, each rounded from its PREC-bit value"""
    t = terms(n, sf_a, sf_b, phi, cap)
    with mpmath.workprec(PREC):
        obs = t[int(x_a)]
        return np.array([float(mpmath.log(v / obs)) for v in t])


def binomial_p(x_a: int, n: int, q):
    """the two-sided p-value of Binomial(n, q) at x_a by the same rule (terms <= the observed one), at PREC bits: the limit of the
    conditional distribution as r grows with sf_a / (sf_a + sf_b) = q"""
    with mpmath.workprec(PREC):
        q = mpf(q)
        t = [mpmath.binomial(n, k) * q ** k * (1 - q) ** (n - k) for k in range(n + 1)]
        return mpmath.fsum(v for v in t if v <= t[x_a]) / mpmath.fsum(t)
