"""The cases of the asymptotic-branch batteries (tests/golden/sseq_asym_table.json), their regimes and bounds, shared by the host battery
(tests/test_sseq_asym_cpu.py) and the device battery (tests/test_gpu_sseq.py).

The bound of a regime is MARGIN x the worst relative error of scipy (double precision, the yardstick) against the high-precision
reference in that regime, never below FLOOR. A regime is `sseq_asym_ref.regime(a, b)` and whether the value lies in the body (>= TAIL)
or the tail (below, down to 1e-300), where the rounding of the prefactor's logarithm alone costs |ln I| ulp."""
import json
import os

import mpmath

from sseq_asym_ref import TIE_DISTANCE, regime

TESTS = os.path.dirname(os.path.abspath(__file__))
FLOOR = 1e-13
MARGIN = 4.0
TAIL = 1e-20


def load_table():
    with open(os.path.join(TESTS, "golden", "sseq_asym_table.json")) as f:
        return json.load(f)


def rel_err(got, ref):
    """|got - ref| / ref with ref a decimal string of the reference"""
    with mpmath.workprec(200):
        r = mpmath.mpf(ref)
        return float(abs(mpmath.mpf(float(got)) - r) / r)


def regime_of(a, b, ref):
    return regime(a, b) + ("/tail" if mpmath.mpf(ref) < TAIL else "/body")


def worst_by_regime(keys, errs):
    out = {}
    for k, e in zip(keys, errs):
        out[k] = max(out.get(k, 0.0), e)
    return out


def bounds_from(yardstick):
    return {k: max(MARGIN * v, FLOOR) for k, v in yardstick.items()}


def nb_errors(rows, got):
    """relative error of every p-value against the reference; a case closer to the median than TIE_DISTANCE may match either side"""
    errs, tie_route = [], 0
    for r, g in zip(rows, got):
        e = rel_err(g, r["p"])
        if r["distance"] < TIE_DISTANCE:
            other = min(rel_err(g, r["p_lower"]), rel_err(g, r["p_upper"]))
            if other < e:
                e, tie_route = other, tie_route + 1
        errs.append(e)
    return errs, tie_route


def nb_keys(rows):
    return [regime_of(r["alpha"], r["beta"], r["p"]) for r in rows]


def nb_bounds(rows):
    return bounds_from(worst_by_regime(nb_keys(rows), nb_errors(rows, [r["scipy"] for r in rows])[0]))


def report(title, keys, lib, yard):
    wl, wy = worst_by_regime(keys, lib), worst_by_regime(keys, yard)
    print(f"\n{title}: worst relative error per regime (cases, library, scipy, bound)")
    for k in sorted(wl):
        print(f"  {k:14s} {keys.count(k):5d}  {wl[k]:.2e}  {wy[k]:.2e}  {max(MARGIN * wy[k], FLOOR):.2e}")
    return wl, bounds_from(wy)


def median_forward_error(m, x):
    """|I_x(a, b) - 1/2| / (1/2) at an x next to the reference median, from the density there (the second-order term is checked small)"""
    with mpmath.workprec(200):
        dx = mpmath.mpf(float(x)) - mpmath.mpf(m["ref"])
        assert abs(dx * mpmath.mpf(m["dlogdens"])) < 1e-6 and abs(dx) < 1e-6 * mpmath.mpf(m["ref"]), (m, x)
        return float(2 * abs(dx) * mpmath.mpf(m["density"]))
