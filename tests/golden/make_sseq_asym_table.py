"""Writes sseq_asym_table.json: the cases of the asymptotic-branch batteries (tests/test_sseq_asym_cpu.py, tests/test_gpu_sseq.py) with
their high-precision values from tests/sseq_asym_ref.py and scipy's double-precision values beside them as the yardstick.

    python tests/golden/make_sseq_asym_table.py [processes]

Takes a few minutes on 8 processes. Doubles are stored as JSON numbers (python's repr round-trips them), high-precision values as
decimal strings. Nothing here looks at the library under test.

  betainc     a, b, x, tag, ref (I_x(a, b), 30 digits), scipy, terms (of the series)
  median      a, b, ref (the median, 40 digits), density (at the median), dlogdens (d ln density / dx there), scipy, scipy_forward
              (|I(scipy's x) - 1/2| / (1/2) on the series)
  nb          x_a, x_b, sf_a, sf_b, mu, phi, group, p, p_lower, p_upper (30 digits), distance (|qa - median| / median), scipy
  left_out    what was generated and has no row, with the reason
"""
import json
import multiprocessing
import os
import sys

import mpmath
import numpy as np
from scipy.special import betainc as sp_betainc
from scipy.special import betaincinv as sp_betaincinv

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sseq_asym_ref as ref  # noqa: E402
import sseq_ref  # noqa: E402

CAP = 100_000_000  # series terms per value here (about a minute); the helper's own default is smaller
QUANTILES = (1e-250, 1e-100, 1e-30, 1e-10, 1e-3, 0.3, 0.5, 0.7, 0.999)
EDGE = (14.999, 15.0, 15.001)
MAX_TIE_SHARE = 0.02

# nb cases: (sf_a, sf_b) groups with sf_b / sf_a from 1e-3 to 1e3, and the alphas reached inside each through mu and phi
NB_GROUPS = (
    (1234567.875, 1234.5625, (650.0, 1.1e4, 3.3e5, 9.9e6)),
    (2200013.5, 73211.25, (20.5, 3.1e3, 2.2e5, 9.5e6)),
    (1900021.75, 2300417.5, (0.62, 14.2, 803.0, 4.1e4, 1.5e6, 8.0e6)),
    (60017.375, 1900021.75, (0.71, 40.3, 5.2e3, 3.0e5)),
    (9700.4375, 9700437.5, (0.55, 30.7, 2.1e3, 9.9e3)),
)
NB_QUANTILES = (1e-200, 1e-40, 1e-8, 1e-3, 0.2)
NB_TOTALS = (3001, 1_000_003, 2 ** 31 + 11, 2 ** 40 - 5)


def s(v, digits=30):
    return mpmath.nstr(v, digits, min_fixed=0, max_fixed=0)


def ab_pairs():
    grid = [float(v) for v in np.geomspace(0.5, 1e7, 8)]
    pairs = [(a, b) for a in grid for b in grid]
    others = (2.5,) + EDGE + (700.25, 1.0e6)
    for t in EDGE:
        for o in others:
            for p in ((t, o), (o, t)):
                if p not in pairs:
                    pairs.append(p)
    return pairs


def betainc_points(a, b):
    pts = []
    with np.errstate(all="ignore"):
        for q in QUANTILES:
            pts.append((float(sp_betaincinv(a, b, q)), f"q={q:g}"))
    xs = (a + 1.0) / (a + b + 2.0)
    pts.append((float(np.nextafter(xs, 0.0)), "switch-"))
    pts.append((float(np.nextafter(xs, 1.0)), "switch+"))
    return pts


def do_pair(ab):
    a, b = ab
    rows, left = [], []
    with mpmath.workprec(ref.PREC):
        for x, tag in betainc_points(a, b):
            if not 0.0 < x < 1.0:
                left.append(dict(kind="betainc", a=a, b=b, tag=tag, reason="x outside (0, 1) in double"))
                continue
            try:
                v, n = ref.betainc_terms(a, b, x, CAP)
            except ref.TermCapExceeded:
                left.append(dict(kind="betainc", a=a, b=b, x=x, tag=tag, reason="series term cap"))
                continue
            if v < mpmath.mpf("1e-300"):
                left.append(dict(kind="betainc", a=a, b=b, x=x, tag=tag, reason="value below 1e-300"))
                continue
            rows.append(dict(a=a, b=b, x=x, tag=tag, ref=s(v), scipy=float(sp_betainc(a, b, x)), terms=n))
        med = None
        try:
            m = ref.beta_median(a, b, CAP)
            sx = float(sp_betaincinv(a, b, 0.5))
            fwd = abs(ref.betainc(a, b, sx, CAP) - mpmath.mpf(1) / 2) * 2
            med = dict(a=a, b=b, ref=s(m, 40), density=s(ref.beta_density(a, b, m)), dlogdens=s((mpmath.mpf(a) - 1) / m - (mpmath.mpf(b) - 1) / (1 - m)),
                       scipy=sx, scipy_forward=float(fwd))
        except ref.TermCapExceeded:
            left.append(dict(kind="median", a=a, b=b, reason="series term cap"))
    return rows, med, left


def nb_params(sf_a, alpha, k):
    """mu and phi with sf_a mu / (1 + phi mu) near alpha; phi runs over a few decades with k"""
    m = alpha / sf_a
    phi = min((0.011, 0.13, 0.9, 2.3)[k % 4], 0.8 / m)
    return m / (1.0 - phi * m), phi


def nb_counts(alpha, beta):
    """(x_a, x_b, tag) of one (alpha, beta): fractions from the deep lower to the deep upper tail, and counts around the median"""
    out, seen = [], set()
    with np.errstate(all="ignore"):
        fr = [(float(sp_betaincinv(alpha, beta, q)), f"lower q={q:g}") for q in NB_QUANTILES]
        fr += [(1.0 - float(sp_betaincinv(beta, alpha, q)), f"upper q={q:g}") for q in NB_QUANTILES]
        med = float(sp_betaincinv(alpha, beta, 0.5))
    for i, (x, tag) in enumerate(fr):
        n = NB_TOTALS[i % len(NB_TOTALS)]
        xa = min(max(int(round(n * x - 0.5)), 1), n - 1)
        if (xa, n - xa) not in seen:
            seen.add((xa, n - xa))
            out.append((xa, n - xa, tag))
    for n, d in ((2 ** 40 - 5, 0), (2 ** 40 - 5, -2), (1_000_003, 1), (3001, 0)):
        xa = min(max(int(n * med) + d, 1), n - 1)
        if (xa, n - xa) not in seen:
            seen.add((xa, n - xa))
            out.append((xa, n - xa, f"median{d:+d} of {n}"))
    return out


def nb_row(xa, xb, sf_a, sf_b, mu, phi, group, tag, median):
    r = ref.nb_asymptotic(xa, xb, sf_a, sf_b, mu, phi, median, CAP)
    return dict(x_a=xa, x_b=xb, sf_a=sf_a, sf_b=sf_b, mu=mu, phi=phi, group=group, tag=tag, alpha=r["alpha"], beta=r["beta"], p=s(r["p"]),
                p_lower=s(r["p_lower"]), p_upper=s(r["p_upper"]), distance=float(r["distance"]),
                scipy=float(sseq_ref.nb_asymptotic_test(xa, xb, sf_a, sf_b, mu, phi)))


def do_nb(task):
    group, k = task
    sf_a, sf_b, alphas = NB_GROUPS[group]
    mu, phi = nb_params(sf_a, alphas[k], k + group)
    alpha, beta = ref.alpha_beta(sf_a, sf_b, mu, phi)
    assert 0.5 <= alpha <= 1e7 and 0.5 <= beta <= 1e7, (alpha, beta)
    rows, left = [], []
    with mpmath.workprec(ref.PREC):
        median = ref.beta_median(alpha, beta, CAP)
        for xa, xb, tag in nb_counts(alpha, beta):
            try:
                row = nb_row(xa, xb, sf_a, sf_b, mu, phi, group, tag, median)
            except ref.TermCapExceeded:
                left.append(dict(kind="nb", x_a=xa, x_b=xb, sf_a=sf_a, sf_b=sf_b, mu=mu, phi=phi, reason="series term cap"))
                continue
            if mpmath.mpf(row["p"]) < mpmath.mpf("1e-300"):
                left.append(dict(kind="nb", x_a=xa, x_b=xb, sf_a=sf_a, sf_b=sf_b, mu=mu, phi=phi, reason="value below 1e-300"))
                continue
            rows.append(row)
    return rows, left


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    out = dict(betainc=[], median=[], nb=[], left_out=[])
    with multiprocessing.Pool(procs) as pool:
        nb_tasks = [(g, k) for g in range(len(NB_GROUPS)) for k in range(len(NB_GROUPS[g][2]))]
        nb_async = pool.map_async(do_nb, nb_tasks, chunksize=1)
        for rows, med, left in pool.imap(do_pair, ab_pairs(), chunksize=1):
            out["betainc"] += rows
            if med:
                out["median"].append(med)
            out["left_out"] += left
        for rows, left in nb_async.get():
            out["nb"] += rows
            out["left_out"] += left
    # the tie route's share, on the reference alone: cases beyond the cap are moved away from the median
    ties = [r for r in out["nb"] if r["distance"] < ref.TIE_DISTANCE]
    allowed = int(MAX_TIE_SHARE * len(out["nb"]))
    with mpmath.workprec(ref.PREC):
        for r in ties[allowed:]:
            new = nb_row(r["x_a"] + 5, r["x_b"] - 5, r["sf_a"], r["sf_b"], r["mu"], r["phi"], r["group"], r["tag"] + " moved", None)
            assert new["distance"] >= ref.TIE_DISTANCE
            out["nb"][out["nb"].index(r)] = new
    ties = sum(r["distance"] < ref.TIE_DISTANCE for r in out["nb"])
    assert ties <= MAX_TIE_SHARE * len(out["nb"])
    out["summary"] = dict(betainc=len(out["betainc"]), median=len(out["median"]), nb=len(out["nb"]), nb_ties=ties,
                          left_out={k: sum(1 for e in out["left_out"] if e["reason"] == k) for k in sorted({e["reason"] for e in out["left_out"]})})
    with open(os.path.join(HERE, "sseq_asym_table.json"), "w") as f:
        f.write("{\n")
        for key in ("betainc", "median", "nb", "left_out"):  # one row per line
            f.write(f'"{key}": [\n' + ",\n".join(json.dumps(r) for r in out[key]) + "\n],\n")
        f.write('"summary": ' + json.dumps(out["summary"]) + "\n}\n")
    print(json.dumps(out["summary"]))


if __name__ == "__main__":
    main()
