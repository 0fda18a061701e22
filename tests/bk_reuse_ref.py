"""Cases, model and references for svd_bk's reused projection (tests/test_bk_reuse_cpu.py, tests/test_gpu_bk_reuse.py).

svd_bk does not compute the projection T = op(A) Q with a sparse product: it keeps the half-products H = op(A) K of its iterations
and forms T' = H C, C the coefficient matrix with Q = K C tracked through every CholeskyQR and block Gram-Schmidt step (solver.cpp,
BkRun; the decisions in bk_plan.hpp). T' carries the rounding of H amplified by |C|, so every column whose coefficient column reaches
"reuse_cmax" is recomputed by a direct sparse product. This module restates that scheme in f64 numpy (`model`), with the same
decisions — flagged columns, the raise of the bound, last_direct, the full-direct fallback — and holds the bounds the library is
tested against:

  B1 projection   residual_i = max_r |(op(A) x_i)_r - s_i y_{i,r}| <= sqrt(q) L u s_1, x = the Q-side factor, y = the T-side one,
                  L = max(bound used, 1), u = 2**-53. The residual is formed in np.longdouble (64-bit significand) from the f64
                  entries; its own error (n + 1) 2**-64 sum |a||x| is returned with it and must stay below 2**-8 of the bound.
  B2 Q side       max |X^T X - I| < 1e-12
  B3 T side       |(Y^T Y - I)_ij| <= KAPPA_U sqrt(q) u s_1**2 / (s_i s_j)  (the Gram route squares the condition number)
  B4 subspace     s_i <= sigma_i (1 + 1e-12)  and  s_i >= so_i - (1e-8 s_1 + max(sigma_i - so_i, 0) / 4),
                  sigma = dense f64 SVD, so = the oracle's svd_bk on the same start panel.

The start panel is always scanrs_oracle.omega_panel of the view's orientation, given to the library, the oracle and the model,
so all three build the same Krylov space.

KAPPA_U = 4 x the worst ratio |(Y^T Y - I)_ij| s_i s_j / (sqrt(q) u s_1**2) of the model over VIEWS x settings, rounded up to a
tenth: the worst is 1.88 (`PYTHONPATH=oracle python tests/bk_reuse_ref.py` prints the ratios against KAPPA_U: cellranger at reuse_cmax 1e-300,
k = 8, q = 80; then odd_block 1.69, three_iterations 1.44), so KAPPA_U = 7.6. It may not exceed 8.

Thresholds: a case that needs its own reuse_cmax takes the geometric middle of a gap of at least a factor 4, below 1e7, in the
model's sorted coefficient maxima of the older blocks (`pick_threshold`): coefficients beyond 1e7 are not reproducible between two
correct f64 orthonormalisations, and a threshold inside a gap makes the flagged set the same for the model, the host path and the
device path. At the default 1e5 no gap is asked for: there a branch-1 case may differ from the model in the columns whose maximum
lies within a factor 2 of the bound (`flagged_range`).

Teeth: with reuse_cmax 1e300 nothing is flagged. deep_8_iterations then leaves B1's bound for L = 1e5 by a factor 9e8 (residual
0.12 s_1) and wide_pass by 1e5 in the model. The 800 x 2000 counts are benign by comparison — their largest coefficient is 2.9e5,
so without the guard they stay INSIDE the bound for L = 1e5 (ratio 0.003); what the guard buys there shows against the bound of the
direct product, L = 1: a factor 336.

The cellranger case takes the oracle's dense normalized matrix as A. The oracle evaluates the map chain in f64: by the term budget
of tests/spmm_exact_ref.py (32 half-ulps per term on the longest route) an entry of A is within 16 u of the exact map, which moves a
residual by at most 16 u max_r sum |a||x| (`map_error`): 16 / (sqrt(q) L) of B1's bound at most, 3e-5 of it at L = 1e5."""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import scanrs_oracle as so

U = 2.0 ** -53
LD = np.longdouble
DEFAULT_CMAX = 1e5
ALL_DIRECT = 1e-300  # every column flagged: the control
NO_GUARD = 1e300     # no column flagged: the teeth
KAPPA_U = 7.6        # see the module docstring
MAX_PASS = 104       # widest repair pass the raise rule aims for (bk_plan.hpp, BK_PASS_MAX)


# ---- matrices ------------------------------------------------------------------------------------------------------------------
def counts(rng, m, n, dens, vmax):
    d = np.zeros((m, n), dtype=np.uint32)
    mask = rng.random((m, n)) < dens
    d[mask] = rng.integers(1, vmax + 1, size=int(mask.sum()))
    return d


def planted(rng, m, n, strengths, dens=0.05, vmax=3):
    """Sparse noise plus one dense programme per strength on m/8 rows x n/8 columns: a few dominant singular values over a floor,
    the spectrum on which the Krylov blocks become numerically dependent."""
    d = counts(rng, m, n, dens, vmax)
    for s in strengths:
        rows = rng.choice(m, m // 8, replace=False)
        cols = rng.choice(n, n // 8, replace=False)
        d[np.ix_(rows, cols)] += np.uint32(s)
    return d


@dataclass(frozen=True)
class Case:
    name: str
    kind: str               # "counts" | "planted"
    shape: Tuple[int, int]
    arg: tuple              # (dens, vmax) | strengths
    seed: int
    k: int
    mult: float
    n_iter: int
    branch: int             # bk_limit_branch expected at the case's own reuse_cmax
    target: Optional[float] = None  # the case's reuse_cmax is the gap middle nearest to this (None: the default 1e5)
    normalized: bool = False


CASES = {c.name: c for c in (
    Case("benign_none", "counts", (400, 900), (0.08, 30), 3, 12, 2.0, 5, 0),
    Case("fits_wide_view", "planted", (300, 700), (3, 2, 1), 3, 8, 2.0, 5, 1),
    Case("fits_tall", "planted", (700, 300), (8, 4, 2), 3, 8, 2.0, 5, 1),
    Case("deep_8_iterations", "planted", (300, 700), (8, 4, 2), 3, 8, 2.0, 8, 1),
    Case("wide_pass", "planted", (400, 900), (20, 10, 5, 2), 3, 26, 2.0, 5, 4),
    # the two raises need a threshold inside a factor-4 gap with MORE flagged columns above it than the pass has room for, all
    # (raised to the top) or all but `room` of them (raised to `need`) within two decades. On these counts the maxima of blocks 2
    # and 3 form one continuum from 19 to 3e5 with no such gap, so five iterations reach only branch 4. With four iterations the
    # gaps are 3.8 -> 19 (101 columns above it, the fifth largest 454 < 852: raised to `need`) and 565 -> 2.4e3 (ONE column above
    # it: more than the room only for b = 104, room 0: raised to the top)
    Case("b104_raised_top", "counts", (800, 2000), (0.08, 30), 3, 52, 2.0, 4, 2, target=1.2e3),
    Case("b100_raised_need", "counts", (800, 2000), (0.08, 30), 3, 50, 2.0, 4, 3, target=8.5),
    Case("b100_default", "counts", (800, 2000), (0.08, 30), 3, 50, 2.0, 5, 1),
    Case("two_iterations", "planted", (300, 700), (8, 4, 2), 3, 8, 2.0, 2, 0),
    Case("three_iterations", "planted", (300, 700), (8, 4, 2), 3, 8, 2.0, 3, 0),
    Case("odd_block", "planted", (300, 700), (8, 4, 2), 3, 7, 1.0, 5, 0),
    Case("cellranger", "planted", (300, 700), (3, 2, 1), 3, 8, 2.0, 5, 0, normalized=True),  # the normalisation flattens the programmes: older maxima to 1.8e3
)}


TRANSPOSED = ("fits_wide_view", "fits_tall")   # also run through the transposed view g.t() (the other orientation of the same counts)
BOTH_STORAGES = ("fits_wide_view", "fits_tall")  # also built as CSR (every case is built as CSC)
VIEWS = tuple((name, False) for name in CASES) + tuple((name, True) for name in TRANSPOSED)
TEETH = ("deep_8_iterations", "wide_pass")       # without the guard these leave B1 at L = 1e5 by more than a factor 100


def settings(p):
    """The reuse_cmax values a view is run at: its own (the default for most), the all-direct control, the default."""
    out = [p.cmax, ALL_DIRECT]
    return out if p.cmax == DEFAULT_CMAX else out + [DEFAULT_CMAX]


@functools.lru_cache(maxsize=None)
def case_counts(name):
    c = CASES[name]
    rng = np.random.default_rng(c.seed)
    d = counts(rng, *c.shape, *c.arg) if c.kind == "counts" else planted(rng, *c.shape, c.arg)
    d.setflags(write=False)
    return d


def panel_for(shape, b):
    """omega_panel in the orientation svd_bk reads it: (n, b) for m >= n, (b, m) otherwise (bk_svd.rs:91,119)."""
    m, n = shape
    return so.omega_panel((n, b), 0) if m >= n else so.omega_panel((b, m), 0)


def block_width(shape, k, mult):
    return min(int(np.ceil(k * mult)), min(shape))


# ---- the model -----------------------------------------------------------------------------------------------------------------
class ModelFailure(Exception):
    """The model met a Cholesky failure: the library would shift or complete the panel, which voids the bookkeeping: change the case."""


def _cholqr(P, coef=None):
    """Iterated CholeskyQR as orth_cholqr runs it: stop at the first Gram matrix after a pass that is I to 5e-14 sqrt(n)."""
    n = P.shape[1]
    for it in range(8):
        g = P.T @ P
        if it >= 1 and np.max(np.abs(g - np.eye(n))) < 5e-14 * np.sqrt(n):
            return P, coef
        try:
            r = np.linalg.cholesky(g).T
        except np.linalg.LinAlgError as e:
            raise ModelFailure(str(e))
        rinv = np.linalg.inv(r)
        P = P @ rinv
        if coef is not None:
            coef = coef @ rinv
    raise ModelFailure("CholeskyQR did not converge in 8 passes")


@dataclass
class ModelResult:
    b: int
    q: int
    reuse: bool
    colmax: np.ndarray
    flagged_older: int      # before any raise
    branch: int
    limit: float            # the bound finally used
    direct: tuple           # columns recomputed by the sparse product, after the last_direct merge
    last_direct: bool
    full_direct: bool
    early_projections: int
    cmax_dense: float
    u: np.ndarray
    s: np.ndarray
    v: np.ndarray


def limit_rule(colmax_older, b, n_iter, reuse_cmax):
    """The raise rule of bk_plan.hpp (bk_plan): (flagged count before the raise, branch, bound used)."""
    flagged = sorted((x for x in colmax_older if not x < reuse_cmax), reverse=True)
    limit, branch = reuse_cmax, (4 if flagged else 0)
    if n_iter >= 2 and b <= MAX_PASS:
        room = MAX_PASS - b
        if len(flagged) > room:
            need = flagged[room]
            if flagged[0] < 100.0 * limit:
                limit, branch = float(np.nextafter(flagged[0], np.inf)), 2
            elif need < 100.0 * limit and (room == 0 or flagged[room - 1] > need):
                limit, branch = float(np.nextafter(need, np.inf)), 3
        elif flagged:
            branch = 1
    return len(flagged), branch, limit


def plan_rule(colmax, b, n_iter, reuse_cmax, coef_valid=True):
    """The projection plan of bk_plan.hpp (bk_plan) from max |C| per column of Q: the fields `scanrs_amd.host_bk_plan` returns.
    `direct`: the columns recomputed by the sparse product, after the last_direct merge. The cost comparison behind last_direct is
    kept as it was first written; bk_plan.hpp states why it reduces to n_iter >= 2."""
    q, last_lo = b * n_iter, (n_iter - 1) * b
    reuse = b % 2 == 0
    flagged_older, branch, limit, bad, last_direct = 0, 0, float(reuse_cmax), [], False
    if reuse and not coef_valid:
        bad = list(range(q))  # rank-deficient panels were completed on the host: Q = K C no longer holds
    if reuse and coef_valid:
        flagged_older, branch, limit = limit_rule(colmax[:last_lo], b, n_iter, float(reuse_cmax))
        bad = [j for j in range(q) if not colmax[j] < limit]
        bad_other = sum(j < last_lo for j in bad)
        chunks = lambda x: (x + 127) // 128
        last_direct = chunks(b + bad_other) <= chunks(b) + chunks(len(bad)) and n_iter >= 2
        if last_direct:
            bad = [j for j in bad if j < last_lo] + list(range(last_lo, q))
    full_direct = not (reuse and (len(bad) * 2 < q or last_direct))
    cmax_dense = 0.0
    if not full_direct:
        dense_cols = sorted(set(range(q)) - set(bad))
        cmax_dense = float(np.max(np.asarray(colmax)[dense_cols])) if dense_cols else 0.0
    n_early = n_iter - 2 if (reuse and n_iter >= 3) else 0
    return dict(reuse=reuse, flagged_older=flagged_older, limit_branch=branch, limit=limit, direct=tuple(bad), last_direct=last_direct,
                full_direct=full_direct, n_early=n_early, cmax_dense=cmax_dense)


def model(dense, omega, k, mult, n_iter, reuse_cmax=DEFAULT_CMAX):
    """BkRun (solver.cpp) in f64 numpy, host-path form (rounds of project + CholeskyQR until the projection is at rounding level)."""
    A = np.asarray(dense, dtype=np.float64)
    m, n = A.shape
    rows_ge = m >= n
    op = (lambda X: A @ X) if rows_ge else (lambda X: A.T @ X)    # S -> T
    opT = (lambda Y: A.T @ Y) if rows_ge else (lambda Y: A @ Y)   # T -> S
    ds, dt = (n, m) if rows_ge else (m, n)
    b = block_width((m, n), k, mult)
    q = b * n_iter
    assert b >= k and q <= ds, "the identity-panel branch of svd_bk is not modelled"
    reuse = b % 2 == 0
    P = np.array(omega, dtype=np.float64).reshape((n, b) if rows_ge else (b, m))
    P = P if rows_ge else P.T.copy()
    K, H = np.zeros((ds, q)), np.zeros((dt, q))
    for i in range(n_iter):
        Y = op(P)
        if i >= 1:
            H[:, (i - 1) * b:i * b] = Y  # the half-product of iteration i is op(A) K_{i-1}
        P, _ = _cholqr(opT(Y))
        K[:, i * b:(i + 1) * b] = P
    Klast = P
    # Q = qr(K).Q block by block, Q = K C
    Q, C = K.copy(), np.eye(q)
    for i in range(1, n_iter):
        sl, nprev = slice(i * b, (i + 1) * b), i * b
        Bj, coef = Q[:, sl].copy(), C[:, sl].copy()
        for rnd in range(4):
            h = Q[:, :nprev].T @ Bj
            if rnd >= 1 and np.max(np.abs(h)) < 1e-14:
                break
            Bj = Bj - Q[:, :nprev] @ h
            coef = coef - C[:, :nprev] @ h
            Bj, coef = _cholqr(Bj, coef)
        Q[:, sl], C[:, sl] = Bj, coef
    colmax = np.max(np.abs(C), axis=0)
    last_lo = q - b
    pl = plan_rule(colmax, b, n_iter, reuse_cmax)
    bad, last_direct = list(pl["direct"]), pl["last_direct"]
    if reuse and not last_direct:
        H[:, last_lo:] = op(Klast)
    if pl["full_direct"]:
        T = op(Q)
    else:
        T = np.zeros((dt, q))
        T[:, :b] = H[:, :b]
        for j in range(1, n_iter - (1 if last_direct else 0)):
            nr = (j + 1) * b
            T[:, j * b:nr] = H[:, :nr] @ C[:nr, j * b:nr]
        if bad:
            T[:, bad] = op(Q[:, bad])
    G = T.T @ T
    G = 0.5 * (G + G.T)
    w, Z = np.linalg.eigh(G)
    idx = np.argsort(w)[::-1][:k]
    s = np.sqrt(np.maximum(w[idx], 0.0))
    E = Z[:, idx]
    side_s, side_t = Q @ E, (T @ E) / s
    u, v = (side_t, side_s) if rows_ge else (side_s, side_t)
    return ModelResult(b, q, reuse, colmax, pl["flagged_older"], pl["limit_branch"], pl["limit"], pl["direct"], last_direct, pl["full_direct"],
                       pl["n_early"], pl["cmax_dense"], u, s, v)


def pick_threshold(colmax_older, target):
    """Geometric middle of the gap (factor >= 4, wholly below 1e7) in the sorted maxima nearest to `target`; None without one."""
    x = np.sort(np.asarray(colmax_older, dtype=np.float64))
    best = None
    for lo, hi in zip(x[:-1], x[1:]):
        if hi >= 4.0 * lo and hi < 1e7 and lo > 0.0:
            mid = float(np.sqrt(lo * hi))
            if best is None or abs(np.log(mid / target)) < abs(np.log(best / target)):
                best = mid
    return best


# ---- references ----------------------------------------------------------------------------------------------------------------
def sides(shape, u, v):
    """(Q-side factor, T-side factor): V and U for m >= n, U and V otherwise."""
    return (v, u) if shape[0] >= shape[1] else (u, v)


def residual(dense_f, u, s, v):
    """(res, self_err): res_i = max_r |(op(A) x_i)_r - s_i y_{i,r}| formed in np.longdouble from f64 entries, self_err_i the bound
    (n + 1) 2**-64 max_r sum |a||x_i| of that computation's own error (n terms summed, the subtraction)."""
    assert np.finfo(LD).nmant >= 63, "np.longdouble has no 64-bit significand on this host"
    A = np.asarray(dense_f, dtype=np.float64)
    x, y = sides(A.shape, u, v)
    Aop, Al = _op_longdouble(A)
    prod = Al @ np.asarray(x, dtype=np.float64).astype(LD)
    mag = (np.abs(Aop) @ np.abs(x)) * (1.0 + 1e-9)  # (an f64 sum of positive terms: far more accurate than the bound needs)
    res = np.max(np.abs(prod - (np.asarray(y, dtype=np.float64) * np.asarray(s, dtype=np.float64)).astype(LD)), axis=0)
    self_err = (Aop.shape[1] + 1) * 2.0 ** -64 * np.max(mag, axis=0)
    return res.astype(np.float64), self_err


_LD_CACHE = {}


def _op_longdouble(A):
    """(op(A) in f64, the same in np.longdouble), kept for the matrices of `prepared` (their buffers are read-only and live on)."""
    key = (A.__array_interface__["data"][0], A.shape) if not A.flags.writeable else None
    if key in _LD_CACHE:
        return _LD_CACHE[key]
    Aop = A if A.shape[0] >= A.shape[1] else A.T
    out = (Aop, Aop.astype(LD))
    if key is not None:
        _LD_CACHE[key] = out
    return out


def map_error(dense_f, u, s, v):
    """16 u max_r sum |a||x_i|: how far the oracle's f64 map chain can move a residual (module docstring)."""
    A = np.asarray(dense_f, dtype=np.float64)
    x, _ = sides(A.shape, u, v)
    Aop = A if A.shape[0] >= A.shape[1] else A.T
    return 16.0 * U * np.max(np.abs(Aop) @ np.abs(x), axis=0)


def used_limit(limit, all_direct):
    return 1.0 if all_direct else max(float(limit), 1.0)


def ratios(dense_f, q, L, u, s, v, sigma, s_oracle):
    """The four bounds as ratios (<= 1 passes): dict b1, b2, b3, b4_upper, b4_lower, and self (B1's reference error over its bound)."""
    k = len(s)
    x, y = sides(np.shape(dense_f), u, v)
    res, self_err = residual(dense_f, u, s, v)
    bound1 = np.sqrt(q) * L * U * s[0]
    gx = np.abs(x.T @ x - np.eye(k))
    gy = np.abs(y.T @ y - np.eye(k))
    bound3 = KAPPA_U * np.sqrt(q) * U * s[0] ** 2 / np.outer(s, s)
    shortfall = np.maximum(sigma[:k] - s_oracle[:k], 0.0)
    return {
        "b1": float(np.max(res) / bound1),
        "self": float(np.max(self_err) / bound1),
        "b2": float(np.max(gx) / 1e-12),
        "b3": float(np.max(gy / bound3)),
        "b4_upper": float(np.max(s / (sigma[:k] * (1.0 + 1e-12)))),
        "b4_lower": float(np.max((s_oracle[:k] - s) / (1e-8 * s[0] + 0.25 * shortfall))),
    }


@dataclass
class Prepared:
    case: Case
    transposed: bool
    counts: np.ndarray      # uint32, as the handle is built (before .t())
    dense_f: np.ndarray     # f64, the matrix svd_bk sees (view applied, normalized when the case says so)
    omega: np.ndarray
    b: int
    q: int
    sigma: np.ndarray       # dense SVD
    s_oracle: np.ndarray    # the oracle's svd_bk on omega
    cmax: float             # the case's own reuse_cmax

    def model(self, reuse_cmax=None):
        return _model_cached(self.case.name, self.transposed, self.cmax if reuse_cmax is None else float(reuse_cmax))


@functools.lru_cache(maxsize=None)
def prepared(name, transposed=False):
    c = CASES[name]
    cnt = case_counts(name)
    o = so.AdaptiveMat.from_dense(cnt, so.CSC)
    if c.normalized:
        o = so.normalize(o, "cellranger")
    if transposed:
        o = o.t()
    dense_f = np.ascontiguousarray(np.asarray(o.to_dense(), dtype=np.float64))
    dense_f.setflags(write=False)
    b = block_width(dense_f.shape, c.k, c.mult)
    omega = panel_for(dense_f.shape, b)
    sigma = np.linalg.svd(dense_f, compute_uv=False)
    s_oracle = so.BkSvd(c.mult, c.n_iter).run_pca(o, c.k, omega=omega)[1]
    p = Prepared(c, transposed, cnt, dense_f, omega, b, b * c.n_iter, sigma, s_oracle, DEFAULT_CMAX)
    if c.target is not None:
        base = model(dense_f, omega, c.k, c.mult, c.n_iter, DEFAULT_CMAX)
        thr = pick_threshold(base.colmax[:p.q - b], c.target)
        assert thr is not None, f"{name}: no gap of a factor 4 below 1e7 in the coefficient maxima"
        p.cmax = thr
    return p


@functools.lru_cache(maxsize=None)
def _model_cached(name, transposed, reuse_cmax):
    p = prepared(name, transposed)
    return model(p.dense_f, p.omega, p.case.k, p.case.mult, p.case.n_iter, reuse_cmax)


def model_ratios(p, reuse_cmax=None):
    r = p.model(reuse_cmax)
    cm = p.cmax if reuse_cmax is None else reuse_cmax
    L = used_limit(r.limit, cm == ALL_DIRECT or r.full_direct)
    return r, ratios(p.dense_f, r.q, L, r.u, r.s, r.v, p.sigma, p.s_oracle)


def flagged_range(p, reuse_cmax):
    """(fewest, most) older columns a correct run may flag at `reuse_cmax`: those at or above twice the bound, those above half."""
    older = p.model(reuse_cmax).colmax[:p.q - p.b]
    return int(np.sum(older >= 2.0 * reuse_cmax)), int(np.sum(older >= 0.5 * reuse_cmax))


def b1_ratio(dense_f, q, L, u, s, v):
    res, self_err = residual(dense_f, u, s, v)
    bound = np.sqrt(q) * L * U * s[0]
    return float(np.max(res) / bound), float(np.max(self_err) / bound)


def threshold_gap(p):
    """(largest older maximum below the case's threshold, smallest at or above it)."""
    older = p.model().colmax[:p.q - p.b]
    below, above = older[older < p.cmax], older[older >= p.cmax]
    return (float(below.max()) if below.size else 0.0), (float(above.min()) if above.size else np.inf)


if __name__ == "__main__":  # the table the docstrings quote
    for name, tr in VIEWS:
        if True:
            p = prepared(name, tr)
            for cm in settings(p) + [NO_GUARD]:
                r, ra = model_ratios(p, cm)
                older = r.colmax[:r.q - r.b]
                print("%-18s t=%d cmax %-8.3g b %3d q %3d branch %d flagged %3d limit %.3g direct %3d last_direct %d full %d older max %.2e | "
                      "b1 %.3f (self %.1e) b2 %.3f b3 %.3f b4 %.3f / %.3f" % (
                          name, tr, cm, r.b, r.q, r.branch, r.flagged_older, r.limit, len(r.direct), r.last_direct,
                          r.full_direct, older.max() if older.size else 0.0, ra["b1"], ra["self"], ra["b2"], ra["b3"], ra["b4_upper"], ra["b4_lower"]), flush=True)
