"""TEST INFRASTRUCTURE: a plain numpy model of the kNN filter of knn.hip and the seeded inputs that attack its error margin.

Two things live here, shared by tests/test_knn_filter_cpu.py (no device) and tests/test_gpu_knn_filter.py:

* the exact side: squared distances as the device's f64 kernels form them (a chain of fused multiply-adds over the coordinates,
  s = fma(t, t, s), emulated exactly with error-free transformations), ranked with ties by index;
* the filter's test value as knn.hip states it: coordinates rounded f64 -> f32 -> bf16 (round to nearest even), an f32 dot
  product, A_q and N_p with the margin gamma split into three bf16 pieces, the (1 +- 4e-7) shaves, the absolute slack and the
  clamp of A. Only the order of the f32 summation is not the matrix cores' (it is numpy's): pairs within f32 rounding of zero
  may fall on the other side, which is 4 orders of magnitude below the margin the tests are about.

The builders produce data on which bf16 rounding does NOT cancel: few dimensions, away from the origin, coordinates placed just
under half a bf16 ulp from their rounded value."""
import numpy as np

OLD_GAMMA = 0.0021  # the margin knn.hip used before it was re-derived from u = 2^-8: half of what rounding alone needs
UMAX = np.iinfo(np.uint32).max


# ---- number formats ---------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """float32 array -> the nearest bf16 value (ties to even), returned as float32"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16
    return (b & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def bf16_ulp(b):
    """spacing of the bf16 grid at the (nonzero, bf16-valued) float64 array b"""
    _, e = np.frexp(np.abs(b))  # |b| = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, e - 8)


def split3(v):
    """float32 v -> three bf16 pieces (as float32) with v = h + m + l up to 2^-24 |v|, as knn.hip's split3"""
    v = np.asarray(v, dtype=np.float32)
    h = bf16_rne(v)
    r1 = (v - h).astype(np.float32)
    m = bf16_rne(r1)
    lo = bf16_rne((r1 - m).astype(np.float32))
    return h, m, lo


def worst_rounding(x, f):
    """every coordinate moved to its bf16 value plus f bf16-ulps AWAY from zero (f < 0: towards zero). |f| < 0.5 keeps the bf16
    value, so the rounding error of every coordinate is the same large fraction of the worst case and has the sign of -f x."""
    b = bf16_rne(np.asarray(x, dtype=np.float32)).astype(np.float64)
    return b + np.sign(b) * f * bf16_ulp(b)


# ---- exact side -------------------------------------------------------------------------------------------------------------
def _fma_sq_acc(t, s):
    """fma(t, t, s) elementwise in float64: t*t = p + e exactly (Dekker), p + s = h + l exactly (Knuth), result h + (l + e).
    Differs from the correctly rounded value only when l + e is itself inexact AND lands within 2^-106 of a rounding boundary."""
    c = 134217729.0 * t
    hi = c - (c - t)
    lo = t - hi
    p = t * t
    e = ((hi * hi - p) + 2.0 * hi * lo) + lo * lo
    h = p + s
    z = h - p
    l = (p - (h - z)) + (s - z)
    return h + (l + e)


def exact_d2(q, p, chunk=512):
    """n_q x n_p squared distances, bit for bit what knn_exhaustive_kernel / knn_rerank_kernel compute under knn.hip's Euclid: s = fma(p_j - q_j, p_j - q_j, s), j ascending"""
    q, p = np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64)
    out = np.empty((q.shape[0], p.shape[0]))
    for a in range(0, q.shape[0], chunk):
        qq = q[a:a + chunk]
        s = np.zeros((qq.shape[0], p.shape[0]))
        for j in range(q.shape[1]):
            s = _fma_sq_acc(p[None, :, j] - qq[:, j, None], s)
        out[a:a + chunk] = s
    return out


def rank(d2, k, drop_self=False):
    """the k nearest per row of d2 (ties by index), UINT32_MAX padded; drop_self removes column i from row i"""
    n_q, n_p = d2.shape
    if drop_self:
        d2 = d2.copy()
        i = np.arange(min(n_q, n_p))
        d2[i, i] = np.inf  # sorts last: no builder has an infinite distance
    kk = min(k, n_p)
    order = np.argsort(d2, axis=1, kind="stable")[:, :kk].astype(np.int64)
    order[np.take_along_axis(d2, order, axis=1) == np.inf] = UMAX
    out = np.full((n_q, k), UMAX, dtype=np.int64)
    out[:, :kk] = order
    return out


def kth_d2(d2, k):
    """per row the k-th smallest entry (+inf when the row has fewer than k)"""
    if d2.shape[1] < k:
        return np.full(d2.shape[0], np.inf)
    return np.partition(d2, k - 1, axis=1)[:, k - 1]


# ---- the filter's test value ------------------------------------------------------------------------------------------------
def filter_pass(q, p, tau, gamma, a_pass=9e29, with_slack=True):
    """boolean n_q x n_p: the pairs one pass of the filter lets through (thresholds tau, margin gamma)"""
    q, p = np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64)
    qb, pb = bf16_rne(q.astype(np.float32)), bf16_rne(p.astype(np.float32))
    m = max(np.max(np.abs(q)), np.max(np.abs(p)))
    slack = 2.0 ** -117 * (m + 1.0) if with_slack else 1e-300
    qn, pn = np.sum(q * q, axis=1), np.sum(p * p, axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        n32 = (pn * (0.5 - gamma) * (1.0 - 4e-7)).astype(np.float32)
        a = 0.5 * np.asarray(tau, dtype=np.float64) - qn * (0.5 - gamma)
        a = a + np.abs(a) * 4e-7 + slack
        a32 = np.where(a > a_pass, np.float32(a_pass), a.astype(np.float32)).astype(np.float32)
        a32 = np.where(np.isnan(a32), np.float32(a_pass), a32).astype(np.float32)
        t = qb @ pb.T  # f32 products of bf16 values are exact; the sum is f32
        for piece in split3(a32):
            t = (t + piece[:, None]).astype(np.float32)
        for piece in split3(-n32):
            t = (t + piece[None, :]).astype(np.float32)
    return t >= 0


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------
def _pca_like(rng, n, d):
    centres = rng.standard_normal((12, d)) * 3.0
    v = centres[rng.integers(0, 12, size=n)] + rng.standard_normal((n, d))
    v *= np.linspace(1.0, 0.3, d)  # decaying spectrum, as PCA scores have (the case of tests/test_knn.py)
    v[17] = v[5]
    v[n - 1] = v[5]  # three exactly coincident points
    return v


def _worst(rng, n, d, f, signed=False):
    x = rng.uniform(0.5, 4.0, size=(n, d))
    if signed:
        x *= rng.choice([-1.0, 1.0], size=(n, d))
    return worst_rounding(x, f)


def _circle(rng, n):
    t = rng.uniform(0.0, 2.0 * np.pi, size=n)
    return np.stack([np.cos(t), np.sin(t)], axis=1)


# name -> (seed, builder). SELECTIVE: cases whose lists must not overflow (a test that passes because everything overflowed has
# tested the exhaustive fallback, not the filter)
_BUILDERS = {
    "u12_2d": (1, lambda r: r.uniform(1.0, 2.0, size=(2048, 2))),
    "circle": (2, lambda r: _circle(r, 4096)),
    "worst_2d": (3, lambda r: _worst(r, 4096, 2, 0.47)),
    "worst_3d": (4, lambda r: _worst(r, 4096, 3, 0.47)),
    "worst_5d": (5, lambda r: _worst(r, 4096, 5, 0.47)),
    "worst_2d_towards_zero": (6, lambda r: _worst(r, 2048, 2, -0.47)),
    "worst_2d_signed": (7, lambda r: _worst(r, 2048, 2, 0.47, signed=True)),
    "worst_2d_up40": (8, lambda r: _worst(r, 2048, 2, 0.47) * 2.0 ** 40),
    "worst_2d_down40": (8, lambda r: _worst(r, 2048, 2, 0.47) * 2.0 ** -40),
    "box_one_bf16_cell": (9, lambda r: 1.0 + 2.0 ** -8 * r.uniform(0.6, 0.99, size=(2048, 2))),  # every point rounds to (1, 1)
    "u12_1d": (10, lambda r: r.uniform(1.0, 2.0, size=(4096, 1))),
    "gauss_50d": (11, lambda r: r.standard_normal((1280, 50))),
    "gauss_2d": (12, lambda r: r.standard_normal((4096, 2))),
    "pca_like": (13, lambda r: _pca_like(r, 1536, 20)),
}
CASES = tuple(_BUILDERS)
SELECTIVE = ("u12_2d", "circle", "worst_2d", "worst_3d", "worst_5d", "worst_2d_up40", "worst_2d_down40", "gauss_50d", "gauss_2d", "pca_like")
OLD_MARGIN_FAILS = ("u12_2d", "worst_2d", "worst_2d_signed", "worst_2d_up40", "worst_2d_down40", "box_one_bf16_cell")  # the old margin drops true neighbours here

_cache = {}


def points(name):
    seed, fn = _BUILDERS[name]
    return fn(np.random.default_rng(seed))


def case(name):
    """(points, exact n x n squared distances of the set against itself); the last two cases are kept (134 MB each at n = 4096)"""
    if name not in _cache:
        while len(_cache) >= 2:
            _cache.pop(next(iter(_cache)))
        v = points(name)
        d2 = exact_d2(v, v)
        d2.setflags(write=False)
        _cache[name] = (v, d2)
    return _cache[name]


def search_strides(n_p, ratio=4, cap=1024):
    """(stride of the subset ranked exactly first, strides of the filter rounds) as knn_filtered chooses them"""
    st0 = 1
    while (n_p + st0 - 1) // st0 > cap:
        st0 *= 2
    strides, st = [], st0
    while st > 1:
        st = max(st // ratio, 1)
        strides.append(st)
    return st0, strides


def model_search(v, d2, k, gamma, drop_self=True, ratio=4, cap=1024):
    """The rounds of knn_filtered on the set against itself, every round with the exact k-th distance of the previous subset as its
    threshold (what a complete filter, or the exhaustive fallback, leaves behind). Per round: (stride, candidate counts[n],
    true neighbours of the round the model drops from lists that did not overflow)."""
    n = v.shape[0]
    work = d2
    if drop_self:
        work = d2.copy()
        work[np.arange(n), np.arange(n)] = np.inf
    st0, strides = search_strides(n, ratio, cap)
    tau = kth_d2(work[:, ::st0], k)
    rounds = []
    for st in strides:
        passed = filter_pass(v, v[::st], tau, gamma)
        cnt = passed.sum(axis=1)
        sub = work[:, ::st]
        new_tau = kth_d2(sub, k)
        lost = ((sub <= new_tau[:, None]) & ~passed & (cnt <= cap)[:, None]).sum(axis=1)
        rounds.append((st, cnt, lost))
        tau = new_tau
    return rounds
