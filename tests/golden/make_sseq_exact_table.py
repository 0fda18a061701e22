"""Writes sseq_exact_table.json: the cases of the exact-branch batteries (tests/test_sseq_exact_cpu.py, tests/test_gpu_sseq_exact.py) with
their high-precision values from tests/sseq_exact_ref.py and two double-precision yardsticks beside them.

    python tests/golden/make_sseq_exact_table.py [processes]

Takes under a minute on 8 processes. Doubles are stored as JSON numbers (python's repr round-trips them), high-precision values as decimal
strings. Nothing here looks at the library under test.

  rows        x_a, x_b, sf_a, sf_b, mu, phi, group (rows of a group share sf_a and sf_b), tag, sar, sbr (sf / phi as doubles round them), mode
              (of the terms), p, p_lower, p_upper (30 digits), distance, log_span, mirror (tests/sseq_exact_ref.py), in_ratio
              (sseq_ratio_ref.in_ratio_partition), f64_logspace (sseq_ref.nb_exact_test with direct=True: gammaln of every argument, the formula as
              the reference writes it), f64_ratio (sseq_ratio_ref.nb_exact_test_ratio)
  left_out    what was generated and has no row, with the reason
  summary     counts; near_ties is the number of rows with distance < TIE_DISTANCE that are no mirror rows

The shape of the terms is set by (sar, sbr, n) alone: mu multiplies every term by one factor. The mode therefore sits at 0, at n or inside
(0, n) through the size-factor pair, phi and n; mu runs over three decades (capped by pick_mu) and moves only the constant of the log-space
terms.
"""
import json
import math
import multiprocessing
import os
import sys

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sseq_exact_ref as ref  # noqa: E402
import sseq_ratio_ref  # noqa: E402
import sseq_ref  # noqa: E402

MAX_TIE_SHARE = 0.02
PHIS = (0.005, 0.011, 0.13, 0.9, 2.3, 27.0)
MUS = (1e-3, 0.8, 20.0)
CONST_CAP = 5e4
SMALL_N = (1, 2, 10, 100)
LARGE_N = (2047, 2048, 2049, 4097, 6145)  # SSEQ_CHUNK = 2048: these end and open chunks
CHUNK = 2048
TAILS = (1e-8, 1e-40, 1e-200, 1e-296)  # the last: an observed term below 2^-970 of the anchor's, which the Ratio backend hands to LogSpace
PIN = (6, 3, 885.7432862994995, 2023.055530268548, 0.0029272959469517066, 27.024221110009037)  # dist.rs:420-429: 0.03254
# (sf_a, sf_b): sf_b / sf_a from 1e-3 to 1e3, magnitudes from 0.3 to 2e6. The last pair lies beyond that ratio: a cluster of a few cells
# against a million, the only way to max(sar, sbr) >= 1e6 beside min(sar, sbr) < 15.
GROUPS = (
    (1200.0, 1.0e6),
    (2.0e6, 2000.0),
    (2.0e5, 8.0e5),
    (0.3, 300.0),
    (40.5, 0.7),
    (1900021.75, 2300417.5),
    (3.25, 7.5),
    (1.5, 1500.0),
    (2.0, 2.0e6),
)
# n near 1e5 with x_a <= 900: what the exact branch gets from a one-vs-rest call (group, phi, n, x_a's)
ONE_VS_REST = ((0, 0.13, 100003, (0, 5, 118, 900)), (7, 0.9, 99991, (0, 3, 97, 899)))
# sf_a == sf_b, x_a != n - x_a: the mirror term ties with the observed one in exact arithmetic (with their x_a <-> x_b swaps)
SYMMETRIC = ((30, 2000, 50.0, 50.0, 20.0, 0.5), (450, 440, 5e5, 5e5, 1e-3, 0.13), (120, 80, 7.0, 7.0, 10.0, 0.3), (3, 6142, 0.4, 0.4, 0.8, 0.9),
             (1000, 1049, 2.0e6, 2.0e6, 0.8, 0.011))


def s(v, digits=30):
    return mpmath.nstr(v, digits, min_fixed=0, max_fixed=0)


def x_candidates(n, sf_a, sf_b, phi):
    """[(x_a, tag)]: the ends, the mode and its neighbours, the chunk ends, and the x_a at which either tail's mass passes each of TAILS"""
    t = ref.terms(n, sf_a, sf_b, phi)
    lf = ref._float_logs(t)
    mode = int(np.argmax(lf))
    out = [(0, "x_a=0"), (n, "x_a=n"), (mode, "mode"), (mode - 1, "mode-1"), (mode + 1, "mode+1")]
    if n > CHUNK:
        anchor = sseq_ratio_ref.ratio_terms(n, sf_a, sf_b, phi)[0]
        out += [(CHUNK - 1, "chunk end 2047"), (CHUNK, "chunk end 2048"), (anchor - CHUNK, "anchor-2048"), (anchor + CHUNK, "anchor+2048")]
    lf = lf - np.logaddexp.reduce(lf)
    lower = np.logaddexp.accumulate(lf) / np.log(10.0)
    upper = (np.logaddexp.accumulate(lf[::-1]) / np.log(10.0))[::-1]
    for q in TAILS:
        k = np.flatnonzero(lower[:mode] <= np.log10(q))
        if k.size:
            out.append((int(k[-1]), f"lower tail {q:g}"))
        k = np.flatnonzero(upper[mode + 1:] <= np.log10(q))
        if k.size:
            out.append((int(k[0]) + mode + 1, f"upper tail {q:g}"))
    seen, uniq = set(), []
    for x, tag in out:
        if 0 <= x <= n and x not in seen:
            seen.add(x)
            uniq.append((x, tag))
    return mode, uniq


def pick_mu(j, sf_a, sf_b, phi):
    """MUS[j], lowered where the constant (sf_a + sf_b) ln(r / (r + mu)) = -(sf_a + sf_b) log1p(mu phi) would pass CONST_CAP: every term is rounded
    at the size of that constant, and a regime's bound follows its largest log_span"""
    x = CONST_CAP / (sf_a + sf_b)
    return min(MUS[j % len(MUS)], math.expm1(x) / phi if x < 700.0 else math.inf)


def make_row(x_a, x_b, sf_a, sf_b, mu, phi, group, tag, mode=None):
    v = ref.nb_exact(x_a, x_b, sf_a, sf_b, mu, phi)
    if mode is None:
        mode = int(np.argmax(ref._float_logs(ref.terms(x_a + x_b, sf_a, sf_b, phi))))
    r = 1.0 / phi
    with np.errstate(all="ignore"):
        return dict(x_a=x_a, x_b=x_b, sf_a=sf_a, sf_b=sf_b, mu=mu, phi=phi, group=group, tag=tag, sar=sf_a * r, sbr=sf_b * r, mode=mode, p=s(v["p"]),
                    p_lower=s(v["p_lower"]), p_upper=s(v["p_upper"]), distance=v["distance"], log_span=v["log_span"], mirror=v["mirror"],
                    in_ratio=bool(sseq_ratio_ref.in_ratio_partition(x_a, x_b, sf_a, sf_b, mu, phi)),
                    f64_logspace=float(sseq_ref.nb_exact_test(x_a, x_b, sf_a, sf_b, mu, phi, direct=True)),
                    f64_ratio=float(sseq_ratio_ref.nb_exact_test_ratio(x_a, x_b, sf_a, sf_b, mu, phi)))


def keep(row, rows, left):
    if mpmath.mpf(row["p"]) < mpmath.mpf("1e-300"):
        left.append(dict(x_a=row["x_a"], x_b=row["x_b"], sf_a=row["sf_a"], sf_b=row["sf_b"], mu=row["mu"], phi=row["phi"], tag=row["tag"],
                         reason="value below 1e-300"))
    else:
        rows.append(row)


def do_task(task):
    kind, arg = task
    rows, left = [], []
    if kind == "grid":
        g, pi = arg
        sf_a, sf_b = GROUPS[g]
        phi = PHIS[pi]
        i = g * len(PHIS) + pi
        for n, full in ((SMALL_N[i % len(SMALL_N)], False), (LARGE_N[i % len(LARGE_N)], True)):
            mode, cands = x_candidates(n, sf_a, sf_b, phi)
            if not full:
                cands = cands[:3]
            for j, (x, tag) in enumerate(cands):
                keep(make_row(x, n - x, sf_a, sf_b, pick_mu(i + j, sf_a, sf_b, phi), phi, g, f"n={n} {tag}", mode), rows, left)
    elif kind == "one_vs_rest":
        g, phi, n, xs = arg
        sf_a, sf_b = GROUPS[g]
        for j, x in enumerate(xs):
            keep(make_row(x, n - x, sf_a, sf_b, pick_mu(j, sf_a, sf_b, phi), phi, g, f"one-vs-rest n={n}"), rows, left)
    elif kind == "symmetric":
        k, (x_a, x_b, sf_a, sf_b, mu, phi) = arg
        for a, b in ((x_a, x_b), (x_b, x_a)):
            keep(make_row(a, b, sf_a, sf_b, mu, phi, len(GROUPS) + 1 + k, "symmetric"), rows, left)
    else:
        keep(make_row(*PIN, len(GROUPS), "pin dist.rs:420-429"), rows, left)
    return rows, left


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    tasks = [("one_vs_rest", a) for a in ONE_VS_REST] + [("grid", (g, pi)) for g in range(len(GROUPS)) for pi in range(len(PHIS))]
    tasks += [("pin", None)] + [("symmetric", (k, c)) for k, c in enumerate(SYMMETRIC)]
    out = dict(rows=[], left_out=[])
    with multiprocessing.Pool(procs) as pool:
        for rows, left in pool.imap(do_task, tasks, chunksize=1):
            out["rows"] += rows
            out["left_out"] += left
    # the tie route's share, on the reference alone: near ties beyond the cap are moved off the tie
    ties = [r for r in out["rows"] if r["distance"] < ref.TIE_DISTANCE and not r["mirror"]]
    allowed = int(MAX_TIE_SHARE * len(out["rows"]))
    for r in ties[allowed:]:
        x = r["x_a"] + 1 if r["x_b"] > 0 else r["x_a"] - 1
        new = make_row(x, r["x_a"] + r["x_b"] - x, r["sf_a"], r["sf_b"], r["mu"], r["phi"], r["group"], r["tag"] + " moved")
        assert new["distance"] >= ref.TIE_DISTANCE
        out["rows"][out["rows"].index(r)] = new
    out["rows"].sort(key=lambda r: r["group"])
    ties = sum(r["distance"] < ref.TIE_DISTANCE and not r["mirror"] for r in out["rows"])
    assert ties <= MAX_TIE_SHARE * len(out["rows"])
    out["summary"] = dict(rows=len(out["rows"]), groups=len({r["group"] for r in out["rows"]}), near_ties=ties,
                          near_tie_share=ties / len(out["rows"]), mirror_rows=sum(r["mirror"] for r in out["rows"]),
                          outside_ratio_partition=sum(not r["in_ratio"] for r in out["rows"]),
                          left_out={k: sum(1 for e in out["left_out"] if e["reason"] == k) for k in sorted({e["reason"] for e in out["left_out"]})})
    with open(os.path.join(HERE, "sseq_exact_table.json"), "w") as f:
        f.write("{\n")
        for key in ("rows", "left_out"):  # one row per line
            f.write(f'"{key}": [\n' + ",\n".join(json.dumps(r) for r in out[key]) + "\n],\n")
        f.write('"summary": ' + json.dumps(out["summary"]) + "\n}\n")
    print(json.dumps(out["summary"]))


if __name__ == "__main__":
    main()
