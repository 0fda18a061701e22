"""The cases of the exact-branch batteries (tests/golden/sseq_exact_table.json), their regimes and bounds, shared by the host battery
(tests/test_sseq_exact_cpu.py) and the device battery (tests/test_gpu_sseq_exact.py).

A regime is the size class of max(sar, sbr) (`<15`, `<1e4`, `<1e6`, `>=1e6`; sar = sf_a / phi, sbr = sf_b / phi as the library rounds them),
whether min(sar, sbr) is below 15 (`lo`: the raised-argument product serves that side; `hi`: Stirling's series serves both), and whether
p lies in the body (>= TAIL) or the tail (below, down to 1e-300). `<15/hi` cannot exist; the other fourteen are all in the table. The few
rows with n >= WIDE (the one-vs-rest shape, n near 1e5) form regimes of their own (`/wide`): their log_span is that of sixteen times as many
terms and would loosen the LogSpace bound of every row it shared a regime with. A finer split only lowers bounds.

Bounds on the relative error of p against the reference's p:

  Ratio     max(MARGIN x the worst error of the double-precision loop tests/sseq_ratio_ref.py in the regime, FLOOR), over the rows the Ratio
            backend partitions itself (`in_ratio`); the rows it hands to LogSpace are held to the LogSpace bound, for both backends.
  LogSpace  max(MARGIN x 2^-53 x S, FLOOR), S the largest `log_span` of the regime. A log-space term is made of six doubles (two ln Γ
            differences, two ln k!, n ln(mu/(r+mu)), (sf_a+sf_b) ln(r/(r+mu))), each carrying a rounding or two of its own size; log_span
            is the sum of those sizes at the k where it is largest, 2^-53 S half an ulp of it, and a relative error e of one term's
            logarithm moves p by at most 2 e.

A row closer than TIE_DISTANCE to a tie with another term (and not a mirror row) may match p_lower or p_upper instead; the share of such rows
is capped by the generator and by a test. A mirror row (sf_a == sf_b, n - x_a != x_a) is held to p, which includes the mirror term.
"""
import json
import os

import mpmath

from sseq_exact_ref import TIE_DISTANCE

TESTS = os.path.dirname(os.path.abspath(__file__))
FLOOR = 1e-13
MARGIN = 4.0
TAIL = 1e-20
MAX_TIE_SHARE = 0.02
WIDE = 50000
SIZES = ((15.0, "<15"), (1e4, "<1e4"), (1e6, "<1e6"))
REGIMES = tuple(f"{s}/{m}/{t}" for s in ("<15", "<1e4", "<1e6", ">=1e6") for m in ("lo", "hi") for t in ("body", "tail") if (s, m) != ("<15", "hi"))


def load_table():
    with open(os.path.join(TESTS, "golden", "sseq_exact_table.json")) as f:
        return json.load(f)


def rel_err(got, ref):
    """|got - ref| / ref with ref a decimal string of the reference"""
    with mpmath.workprec(200):
        r = mpmath.mpf(ref)
        return float(abs(mpmath.mpf(float(got)) - r) / r)


def regime(sar, sbr, p, n=0):
    hi, lo = max(sar, sbr), min(sar, sbr)
    size = next((name for lim, name in SIZES if hi < lim), ">=1e6")
    return f"{size}/{'lo' if lo < 15.0 else 'hi'}/{'tail' if mpmath.mpf(p) < TAIL else 'body'}" + ("/wide" if n >= WIDE else "")


def keys(rows):
    return [regime(r["sar"], r["sbr"], r["p"], r["x_a"] + r["x_b"]) for r in rows]


def near_tie(r):
    return r["distance"] < TIE_DISTANCE and not r["mirror"]


def errors(rows, got):
    """relative error of every p-value against the reference's p, and the number of rows that took the tie route: a near-tie row may match
    p_lower or p_upper instead"""
    errs, tie_route = [], 0
    for r, g in zip(rows, got):
        e = rel_err(g, r["p"])
        if near_tie(r):
            other = min(rel_err(g, r["p_lower"]), rel_err(g, r["p_upper"]))
            if other < e:
                e, tie_route = other, tie_route + 1
        errs.append(e)
    return errs, tie_route


def worst_by_regime(ks, errs):
    out = {}
    for k, e in zip(ks, errs):
        out[k] = max(out.get(k, 0.0), e)
    return out


def logspace_bounds(rows):
    span = worst_by_regime(keys(rows), [r["log_span"] for r in rows])
    return {k: max(MARGIN * 2.0 ** -53 * s, FLOOR) for k, s in span.items()}


def ratio_bounds(rows):
    part = [r for r in rows if r["in_ratio"]]
    yard = worst_by_regime(keys(part), errors(part, [r["f64_ratio"] for r in part])[0])
    return {k: max(MARGIN * yard.get(k, 0.0), FLOOR) for k in set(keys(rows))}


def row_bounds(rows, backend):
    """the bound of every row for backend "logspace" or "ratio": a row outside the Ratio partition carries the LogSpace bound in both"""
    ks, ls = keys(rows), logspace_bounds(rows)
    if backend == "logspace":
        return [ls[k] for k in ks]
    rt = ratio_bounds(rows)
    return [rt[k] if r["in_ratio"] else ls[k] for r, k in zip(rows, ks)]


def report(title, rows, lib, backend):
    """prints, per regime: cases, the library's worst error, both double-precision yardsticks' and the bound; returns the library's worst"""
    ks = keys(rows)
    own = [r["in_ratio"] or backend == "logspace" for r in rows]
    sel = lambda v: [x for x, o in zip(v, own) if o]  # noqa: E731
    wl = worst_by_regime(sel(ks), sel(lib))
    yl = worst_by_regime(ks, errors(rows, [r["f64_logspace"] for r in rows])[0])
    yr = worst_by_regime(sel(ks), errors(sel(rows), [r["f64_ratio"] for r in sel(rows)])[0])
    bound = ratio_bounds(rows) if backend == "ratio" else logspace_bounds(rows)
    print(f"\n{title}: worst relative error per regime (cases, library, f64_logspace, f64_ratio, bound)")
    for k in sorted(wl, key=lambda k: (REGIMES.index(k[:-5]) + 0.5 if k.endswith("/wide") else REGIMES.index(k))):
        print(f"  {k:16s} {sel(ks).count(k):5d}  {wl[k]:.2e}  {yl[k]:.2e}  {yr.get(k, float('nan')):.2e}  {bound[k]:.2e}")
    if backend == "ratio" and not all(own):
        out = [e for e, o in zip(lib, own) if not o]
        print(f"  handed to LogSpace {len(out):4d}  {max(out):.2e}  (held to the LogSpace bound of their regime)")
    return wl


def failures(rows, lib, backend):
    return [(k, e, b, r) for k, e, b, r in zip(keys(rows), lib, row_bounds(rows, backend), rows) if not e <= b]


def groups(rows):
    """row indices per `group`: the rows of a group share (sf_a, sf_b), so one sseq_de_from_sums call serves them"""
    return [[i for i, r in enumerate(rows) if r["group"] == g] for g in sorted({r["group"] for r in rows})]
