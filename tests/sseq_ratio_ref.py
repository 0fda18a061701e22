"""CPU restatement of the Ratio backend of the exact NB test (nb_exact_test_ratio, diff-exp/src/dist.rs:116-215), the checker
of the library's Ratio kernels.

`nb_exact_test_ratio_loop` is the reference's f64 loop written out in pure Python, operation by operation. `ratio_terms` /
`nb_exact_test_ratio` give the same bits with numpy's sequential accumulations (`multiply.accumulate`, `divide.accumulate` and
`add.accumulate` run strictly left to right, and adding 0.0 to a partial sum leaves it unchanged); tests/test_sseq_ratio_cpu.py
asserts that the two agree bit for bit, so that the GPU battery can afford n = 1e6.

One rule is the library's and not the reference's: when sf_a / phi == sf_b / phi bit for bit, the terms k and n - k are equal in exact
arithmetic, and the mirror term n - x_a belongs to the extreme set whatever the rounding of the two sweeps made of it. The reference leaves
that to `<=` on the rounded terms and drops the mirror in some cases (p 3 to 38 % low; tests/test_sseq_exact_cpu.py has the measured rows).
"""
from __future__ import annotations

import math

import numpy as np

import sseq_ref

MIN_OBS = 2.0 ** -970  # below it the library's device path hands a test to the LogSpace kernels (include/scanrs_amd.h)


def ratio_step(k, n, sa_r, sb_r):
    """dist.rs:124-126."""
    return (sa_r + k) * (n - k) / ((k + 1.0) * (sb_r + n - k - 1.0))


def nb_exact_test_ratio_loop(x_a, x_b, sf_a, sf_b, mu, phi):
    """dist.rs:155-215 as a pure-Python loop in the reference's order of operations."""
    if x_a + x_b == 0:
        return 1.0
    if phi == 0.0:
        return 1.0
    if sf_a == 0.0 or sf_b == 0.0:
        return 1.0
    n = int(x_a + x_b)
    nn = float(n)
    r = 1.0 / phi
    sa_r = sf_a * r
    sb_r = sf_b * r
    mode = n
    for k in range(n):
        if ratio_step(float(k), nn, sa_r, sb_r) < 1.0:
            mode = k
            break
    u = [0.0] * (n + 1)
    u[mode] = 1.0
    for k in range(mode, n):
        u[k + 1] = u[k] * ratio_step(float(k), nn, sa_r, sb_r)
    for k in range(mode - 1, -1, -1):
        u[k] = u[k + 1] / ratio_step(float(k), nn, sa_r, sb_r)
    u_obs = u[int(x_a)]
    if u_obs == 0.0 or not math.isfinite(u_obs):
        return sseq_ref.nb_exact_test(x_a, x_b, sf_a, sf_b, mu, phi)
    sum_all = 0.0
    sum_ext = 0.0
    mirror = n - int(x_a) if sa_r == sb_r else -1  # the library's rule for the exact tie (see the module docstring)
    for k, v in enumerate(u):
        sum_all += v
        if v <= u_obs or k == mirror:
            sum_ext += v
    return sum_ext / sum_all


def ratio_terms(n, sf_a, sf_b, phi):
    """(anchor, U[0..n]) of dist.rs:168-195: the bits of the loop above."""
    n = int(n)
    nn = float(n)
    r = 1.0 / phi
    sa_r = sf_a * r
    sb_r = sf_b * r
    k = np.arange(n, dtype=np.float64)
    with np.errstate(all="ignore"):
        steps = (sa_r + k) * (nn - k) / ((k + 1.0) * (sb_r + nn - k - 1.0))
        below = np.flatnonzero(steps < 1.0)
        mode = int(below[0]) if below.size else n
        u = np.zeros(n + 1)
        u[mode:] = np.multiply.accumulate(np.concatenate([[1.0], steps[mode:]]))
        u[:mode + 1] = np.divide.accumulate(np.concatenate([[1.0], steps[:mode][::-1]]))[::-1]
    return mode, u


def degenerate(x_a, x_b, sf_a, sf_b, phi):
    return x_a + x_b == 0 or phi == 0.0 or sf_a == 0.0 or sf_b == 0.0


def u_obs(x_a, x_b, sf_a, sf_b, mu, phi):
    """The observed term U[x_a] of the serial sweep (anchor term = 1)."""
    return float(ratio_terms(x_a + x_b, sf_a, sf_b, phi)[1][int(x_a)])


def in_ratio_partition(x_a, x_b, sf_a, sf_b, mu, phi):
    """The library's device path partitions a test with Ratio when U[x_a] is finite and at least 2^-970; otherwise the test goes
    to LogSpace (the reference: only when U[x_a] is 0 or not finite)."""
    o = u_obs(x_a, x_b, sf_a, sf_b, mu, phi)
    return math.isfinite(o) and o >= MIN_OBS


def nb_exact_test_ratio(x_a, x_b, sf_a, sf_b, mu, phi):
    """dist.rs:155-215; the bits of nb_exact_test_ratio_loop, fast enough for n = 1e6."""
    if degenerate(x_a, x_b, sf_a, sf_b, phi):
        return 1.0
    _, u = ratio_terms(x_a + x_b, sf_a, sf_b, phi)
    o = u[int(x_a)]
    if o == 0.0 or not math.isfinite(o):
        return sseq_ref.nb_exact_test(x_a, x_b, sf_a, sf_b, mu, phi)
    sum_all = np.add.accumulate(u)[-1]
    ext = u <= o
    r = 1.0 / phi
    if sf_a * r == sf_b * r:
        ext[int(x_b)] = True  # the mirror term n - x_a
    sum_ext = np.add.accumulate(np.where(ext, u, 0.0))[-1]
    return float(sum_ext / sum_all)


def nb_exact_test_ratio_tie_bounds(x_a, x_b, sf_a, sf_b, mu, phi, rtol=1e-12):
    """(p without, p with) the terms at k != x_a that tie with the observed one to rtol, like sseq_ref.nb_exact_test_tie_bounds:
    the sum of the terms below U[x_a] (1 - rtol) plus the observed term, and the sum of the terms up to U[x_a] (1 + rtol), each
    over the sum of all terms. Which side of `<=` a tying term falls on is decided by rounding, in the reference too."""
    _, u = ratio_terms(x_a + x_b, sf_a, sf_b, phi)
    o = u[int(x_a)]
    sum_all = math.fsum(u)
    lo = u < o * (1.0 - rtol)
    lo[int(x_a)] = True
    hi = u <= o * (1.0 + rtol)
    return math.fsum(u[lo]) / sum_all, math.fsum(u[hi]) / sum_all
