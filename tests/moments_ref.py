"""Reference side of the column-moment tests (tests/test_moments_cpu.py, tests/test_gpu_moments.py). No GPU, no library.

A case is a sparse count matrix held "summed-over-major": `indptr` over the positions that are summed over (the cells),
`indices` the slice (gene) of every nonzero, `values` its u32 count, and `links`, the map as the handle holds it: a list whose
entries are a float64 vector with one factor per cell (ScaleAxis) or one of LN_1P / LOG2_1P / LOG10_1P.

  exact_moments        per slice S1 = sum f, S2 = sum f^2, the number of terms, mean = S1/m and var = S2/m - (S1/m)^2, the map
                       evaluated in mpmath at 100 bits from the f64 inputs (log(1 + x) as the function it is)
  f64_terms            the terms as the device evaluates them: f64, `x + 1.0` rounded before the logarithm
  fixed_point_moments  col_moments_kernel's accumulation restated: rint(v 2^e1), rint(v v 2^e2) as Python integers, summed
                       exactly, divided by 2^e
  legacy_x / legacy_plan  the rule this project used before scanrs_host_col_moments_plan (quantum = 2^-30 of the LARGEST possible
                       value or finer): data for the tests, which use it to prove that their grid is adversarial
  contract_ratios      the contract every route is held to, as error / bound per quantity
  grid_cases           the cases

The map's own definition limits what ANY route can agree with the exact function: `x + 1.0` is rounded to f64 before the
logarithm (as the reference defines the map), which moves a term f by up to 2^-53 / f relative. The cases keep that below the
contract: their smallest terms are near 1e-4 where the factors differ from cell to cell, and where one tiny factor is shared
by many cells it is a power of two, so that 1 + x is exact. test_moments_cpu.py checks that plain f64 summation of f64_terms
meets the contract on every case with a margin of two."""
import functools
import math

import mpmath
import numpy as np

LN_1P, LOG2_1P, LOG10_1P = 2, 3, 4  # the library's FN_* / OP_* codes
MP = mpmath.mp.clone()
MP.prec = 100

TOL_SUM = 1e-12  # |sum - S1| <= TOL_SUM S1, the same for the mean
TOL_VAR = 1e-10  # |var - var_ref| <= TOL_VAR S2 / m


def _is_log(l):
    return isinstance(l, (int, np.integer))


def _mp_log(kind, x):
    y = MP.log1p(x)
    if kind == LOG2_1P:
        return y / MP.ln2
    if kind == LOG10_1P:
        return y / MP.ln10
    return y


def _cell_of(indptr):
    indptr = np.asarray(indptr, dtype=np.int64)
    return np.repeat(np.arange(indptr.shape[0] - 1), np.diff(indptr))


def exact_terms(indptr, indices, values, links):
    """The exact value of the map at every nonzero (list of mpf), evaluated once per (count, cell) pair."""
    cell = _cell_of(indptr)
    values = np.asarray(values)
    cache, out = {}, []
    for c, v in zip(cell.tolist(), values.tolist()):
        key = (c, v)
        f = cache.get(key)
        if f is None:
            f = MP.mpf(v)
            for l in links:
                f = _mp_log(int(l), f) if _is_log(l) else f * MP.mpf(float(l[c]))
            cache[key] = f
        out.append(f)
    return out


def exact_moments(indptr, indices, values, links, axis_extent, n_inner=None):
    """dict of per-slice lists: S1, S2 (mpf), n_terms (int), mean, var (mpf); axis_extent = m, the divisor of mean and variance."""
    indices = np.asarray(indices, dtype=np.int64)
    n_inner = int(n_inner if n_inner is not None else (indices.max() + 1 if indices.size else 0))
    s1, s2, n = [MP.mpf(0)] * n_inner, [MP.mpf(0)] * n_inner, [0] * n_inner
    for g, f in zip(indices.tolist(), exact_terms(indptr, indices, values, links)):
        s1[g] += f
        s2[g] += f * f
        n[g] += 1
    m = MP.mpf(axis_extent)
    mean = [a / m for a in s1]
    var = [b / m - (a / m) ** 2 for a, b in zip(s1, s2)]
    return {"S1": s1, "S2": s2, "n_terms": n, "mean": mean, "var": var, "m": m}


def f64_terms(indptr, indices, values, links):
    """The terms in f64 as eval_map computes them (numpy's logarithms stand in for the device's, which are within 2 ulp)."""
    cell = _cell_of(indptr)
    x = np.asarray(values, dtype=np.float64)
    for l in links:
        if _is_log(l):
            x = {LN_1P: np.log, LOG2_1P: np.log2, LOG10_1P: np.log10}[int(l)](x + 1.0)
        else:
            x = np.asarray(l, dtype=np.float64)[cell] * x
    return x


def _moments_from(s1, s2, axis_extent):
    m = MP.mpf(axis_extent)
    return {"sum": s1, "mean": [a / m for a in s1], "var": [b / m - (a / m) ** 2 for a, b in zip(s1, s2)]}


def fixed_point_moments(indptr, indices, values, links, axis_extent, n_inner, e1, e2):
    """{"sum", "mean", "var"} per slice (mpf) from integer accumulation of rint(v 2^e1) and rint(v v 2^e2)."""
    v = f64_terms(indptr, indices, values, links)
    t1 = np.rint(np.ldexp(v, e1))
    t2 = np.rint(np.ldexp(v * v, e2))
    a1, a2 = [0] * n_inner, [0] * n_inner
    for g, p, q in zip(np.asarray(indices).tolist(), t1.tolist(), t2.tolist()):
        a1[g] += int(p)
        a2[g] += int(q)
    s1 = [MP.ldexp(MP.mpf(a), -e1) for a in a1]
    s2 = [MP.ldexp(MP.mpf(a), -e2) for a in a2]
    return _moments_from(s1, s2, axis_extent)


def plain_f64_moments(indptr, indices, values, links, axis_extent, n_inner):
    """The ordinary pass's arithmetic: f64 terms added in f64 (in storage order)."""
    v = f64_terms(indptr, indices, values, links)
    s1 = np.zeros(n_inner)
    s2 = np.zeros(n_inner)
    np.add.at(s1, np.asarray(indices, dtype=np.int64), v)
    np.add.at(s2, np.asarray(indices, dtype=np.int64), v * v)
    return _moments_from([MP.mpf(float(a)) for a in s1], [MP.mpf(float(a)) for a in s2], axis_extent)


def legacy_x(max_count, links):
    """The old plan's bound of the largest mapped value: the chain at the largest count under every link's largest factor."""
    x = float(max_count)
    for l in links:
        if _is_log(l):
            x = {LN_1P: math.log1p(x), LOG2_1P: math.log2(1.0 + x), LOG10_1P: math.log10(1.0 + x)}[int(l)]
        else:
            x *= float(np.max(l))
    return x


def legacy_plan(x, n_outer, n_wg, mode):
    """(accept, e1, e2) by the rule of the parent of scanrs_host_col_moments_plan, as it was written."""
    cells = math.ceil(n_outer / n_wg)
    x1, x2 = max(x, 1e-300), max(x * x, 1e-300)
    b1, b2 = x1 * cells * 1.0001, x2 * cells * 1.0001
    e1 = min(62 - math.ceil(math.log2(b1)), 50 - math.ceil(math.log2(x1 * 1.0001)))
    e2 = min(62 - math.ceil(math.log2(b2)), 50 - math.ceil(math.log2(x2 * 1.0001)))
    refuse = e1 > 1000 or e2 > 1000 or e1 + math.log2(x1) < 30.0 or (mode == 2 and e2 + math.log2(x2) < 30.0)
    return (not refuse), e1, e2


def n_workgroups(n_outer, n_cu=256):
    return max(1, min(n_cu, (n_outer + 63) // 64))


def _hi_lo(v):
    """A list of mpf (or an array of f64) as two f64 arrays whose sum is the value to ~106 bits."""
    if isinstance(v, np.ndarray):
        return np.asarray(v, dtype=np.float64), np.zeros(v.shape[0])
    hi = np.array([float(x) for x in v], dtype=np.float64)
    lo = np.array([float(MP.mpf(x) - MP.mpf(h)) for x, h in zip(v, hi.tolist())], dtype=np.float64)
    return hi, lo


def _ref_arrays(ref):
    if "_np" not in ref:
        ref["_np"] = {k: _hi_lo(ref[k]) for k in ("S1", "S2", "mean", "var")}
        ref["_np"]["empty"] = np.array(ref["n_terms"]) == 0
        ref["_np"]["m"] = float(ref["m"])
    return ref["_np"]


def contract_ratios(got_sum, got_mean, got_var, ref):
    """Worst error / bound over the slices for (sum, mean, var): the bounds are TOL_SUM S1, TOL_SUM mean and TOL_VAR S2 / m, no
    absolute term; a slice without terms must give exactly 0 and 0 (else inf). `got_*`: arrays of f64 or lists of mpf; got_sum may be
    None. (result - reference) is formed from the leading f64 parts, whose difference is exact wherever it matters, plus the
    difference of the remainders."""
    r = _ref_arrays(ref)
    empty, worst = r["empty"], []
    for got, key, bound in ((got_sum, "S1", TOL_SUM * r["S1"][0]), (got_mean, "mean", TOL_SUM * r["mean"][0]),
                            (got_var, "var", TOL_VAR * r["S2"][0] / r["m"])):
        if got is None:
            worst.append(0.0)
            continue
        ghi, glo = _hi_lo(got if isinstance(got, list) else np.asarray(got, dtype=np.float64))
        if np.any(ghi[empty] != 0.0) or np.any(glo[empty] != 0.0) or not np.all(np.isfinite(ghi)):
            worst.append(math.inf)
            continue
        err = np.abs((ghi - r[key][0]) + (glo - r[key][1]))[~empty]
        worst.append(float(np.max(err / bound[~empty])) if err.size else 0.0)
    return worst


def plan_links(links):
    """The links as `scanrs_amd.host_col_moments_plan` takes them: what the device reduces from the factor vectors."""
    out = []
    for l in links:
        if _is_log(l):
            out.append((int(l),))
        else:
            a = np.asarray(l, dtype=np.float64)
            bad = (not np.all(np.isfinite(a))) or bool(np.any(a < 0))
            pos = a[a > 0]
            out.append(("scale", float(pos.min()) if pos.size else 0.0, float("nan") if bad else float(a.max())))
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, n_outer, n_inner, indptr, indices, values, links, adversarial):
        self.name, self.n_outer, self.n_inner = name, int(n_outer), int(n_inner)
        self.indptr = np.asarray(indptr, dtype=np.uint64)
        self.indices = np.asarray(indices, dtype=np.uint32)
        self.values = np.asarray(values, dtype=np.uint32)
        self.links, self.adversarial = links, adversarial
        per = np.bincount(self.indices.astype(np.int64), minlength=self.n_inner)
        assert self.indices.shape[0] <= 60000 and per.max() <= 4000, (name, self.indices.shape[0], int(per.max()))

    @functools.cached_property
    def ref(self):
        return exact_moments(self.indptr, self.indices, self.values, self.links, self.n_outer, self.n_inner)

    @property
    def max_count(self):
        return int(self.values.max())

    def args(self):
        return self.indptr, self.indices, self.values, self.links


def _from_cells(name, n_genes, cells, links, adversarial):
    """cells: per cell a dict gene -> count"""
    indptr, idx, val = [0], [], []
    for d in cells:
        for g in sorted(d):
            idx.append(g)
            val.append(d[g])
        indptr.append(len(idx))
    return Case(name, len(cells), n_genes, indptr, idx, val, links, adversarial)


def _random_cells(rng, n_cells, n_genes, per_cell, cmax, g0=0, empty=0.1):
    cells = []
    for _ in range(n_cells):
        if rng.random() < empty:
            cells.append({})
            continue
        k = max(1, int(rng.poisson(per_cell)))
        genes = rng.choice(np.arange(g0, n_genes), size=min(k, n_genes - g0), replace=False)
        cells.append({int(g): int(c) for g, c in zip(genes, rng.integers(1, cmax + 1, size=genes.shape[0]))})
    return cells


def raw_profile_cells(rng, n_cells=3000, n_genes=500, n_big=30, reserved=50):
    """An unfiltered profile: nearly every barcode holds ONE molecule (median total 1), a few are cells of 5 000 - 30 000
    molecules; genes 0 .. reserved-1 are seen in those cells only. No empty barcode, no empty gene."""
    big = set(rng.choice(n_cells, size=n_big, replace=False).tolist())
    cells = []
    for c in range(n_cells):
        if c not in big:
            cells.append({int(rng.integers(reserved, n_genes)): 1})
            continue
        d = {int(g): int(rng.geometric(1.0 / 45.0)) for g in rng.choice(np.arange(reserved, n_genes), size=320, replace=False)}
        for g in range(reserved):
            if rng.random() < 0.7:
                d[g] = int(rng.integers(1, 4))
        cells.append(d)
    for g in range(reserved):  # every reserved gene is seen at least once
        if not any(g in cells[c] for c in big):
            cells[min(big)][g] = 1
    return cells


@functools.lru_cache(maxsize=None)
def grid_cases():
    rng = np.random.default_rng(20261019)
    out = []
    # 1. raw unfiltered profile, log2, factor = target / total with target = the median total = 1
    cells = raw_profile_cells(rng)
    tot = np.array([sum(d.values()) for d in cells], dtype=np.float64)
    assert np.median(tot) == 1.0 and 5000 <= tot.max() <= 30000
    out.append(_from_cells("raw_profile", 500, cells, [1.0 / tot, LOG2_1P], True))
    # 2. totals exp(N(7, 2)) clipped to [1, 3e5]; gene 0 has count 1 in the 5 largest cells only; log10; two ranges of slices
    n = 6000
    tot = np.clip(np.rint(np.exp(rng.normal(7.0, 2.0, size=n))), 1.0, 3e5)
    cells = _random_cells(rng, n, 8200, 4.0, 6, g0=1)
    for c in np.argsort(tot)[-5:]:
        cells[int(c)][0] = 1
    out.append(_from_cells("lognormal_totals", 8200, cells, [np.median(tot) / tot, LOG10_1P], True))
    # 3. one count of 2^32 - 1 in one cell, everything else count 1, every factor 0.01, ln
    n = 2000
    cells = _random_cells(rng, n, 300, 6.0, 1, empty=0.05)
    cells[17] = {5: 2**32 - 1}
    out.append(_from_cells("one_huge_count", 300, cells, [np.full(n, 0.01), LN_1P], True))
    # 4. two scale links in front of the logarithm whose maxima sit on different cells (2^10 ~ 1e3 there, 2^-10 ~ 1e-3 elsewhere:
    #    powers of two, so that 1 + x is exact where 2^-20 is shared by all other cells)
    n = 1500
    cells = _random_cells(rng, n, 400, 8.0, 5, g0=2)
    cells[0], cells[1] = {0: 3, 7: 1}, {1: 2, 9: 4}
    a, b = np.full(n, 2.0**-10), np.full(n, 2.0**-10)
    a[0], b[1] = 2.0**10, 2.0**10
    out.append(_from_cells("two_links_two_maxima", 400, cells, [a, b, LOG2_1P], True))
    # 5. / 6. one scale link BEHIND the logarithm with a factor of 1e5 (1e9) on one cell
    for name, big, fn in (("outer_link_1e5", 1e5, LN_1P), ("outer_link_1e9", 1e9, LOG10_1P)):
        n = 900
        cells = _random_cells(rng, n, 350, 10.0, 9)
        cells[11] = {3: 2, 8: 1}
        pre, post = 0.5 + rng.random(n), np.ones(n)
        post[11] = big
        out.append(_from_cells(name, 350, cells, [pre, int(fn), post], True))
    # benign: factors within a factor of four, counts far above the table, empty cells and genes, two ranges of slices
    n = 400
    cells = _random_cells(rng, n, 8200, 60.0, 6)
    for c in rng.choice(n, size=40, replace=False):
        if cells[int(c)]:
            cells[int(c)][int(rng.integers(0, 8200))] = int(rng.integers(9, 70000))
    out.append(_from_cells("benign_wide", 8200, cells, [0.5 + 1.5 * rng.random(n), 0.9 + 0.2 * rng.random(n), LOG10_1P], False))
    # benign: the accumulator's worst case, one slice in which EVERY cell holds the largest count under the largest factor
    n = 3000
    cells = _random_cells(rng, n, 300, 8.0, 37, g0=1, empty=0.0)
    for d in cells:
        d[0] = 37
    out.append(_from_cells("dense_column", 300, cells, [np.full(n, 1.75), LOG2_1P], False))
    return {c.name: c for c in out}
