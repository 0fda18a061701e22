"""nearest_neighbors of umap-rs (umap-rs/src/knn.rs:112-166) under pearson and cosine distance (dist.rs:19-34, 73-124), restated
with plain Python floats: IEEE doubles, every operation separate (Python never fuses), math.sqrt correctly rounded. The search
selects by (key, index) - the tie rule of the library. Not imported by the library; the tests hold the host twin
to it bit for bit."""
import math

INF = float("inf")
NAN = float("nan")


def _mul(a: float, b: float) -> float:
    return a * b  # Python float multiplication overflows to inf silently, as IEEE does


def _div(a: float, b: float) -> float:
    """IEEE division: Python raises on a zero divisor."""
    if b != 0.0 or b != b:
        return a / b
    if a != a or a == 0.0:
        return NAN
    return math.copysign(INF, a) * math.copysign(1.0, b)


def _sqrt(a: float) -> float:
    if a != a:
        return NAN
    return math.sqrt(a) if a >= 0.0 else NAN


def _rust_max0(v: float) -> float:
    """f64::max(v, 0.0): a NaN operand loses."""
    return v if v > 0.0 else 0.0


def prepare(kind: str, x):
    """(c, s_xx): what depends on one row only (dist.rs:74-76 / 107-115)."""
    x = [float(t) for t in x]
    if kind == "pearson":
        mu = 0.0
        for t in x:
            mu = mu + t
        mu = mu / float(len(x))
        c = [t - mu for t in x]
    else:
        c = x
    s = 0.0
    for t in c:
        s = s + _mul(t, t)
    return c, s


def pair_value(s_xx: float, s_yy: float, s_xy: float) -> float:
    """dist.rs:77-83 / 117-123."""
    if s_xx == 0.0 and s_yy == 0.0:
        return 0.0
    if s_xy == 0.0:
        return 1.0
    return _rust_max0(1.0 - _div(s_xy, _sqrt(_mul(s_xx, s_yy))))


def fold_xy(cx, cy) -> float:
    s = 0.0
    for a, b in zip(cx, cy):
        s = s + _mul(a, b)
    return s


def value(kind: str, x, y) -> float:
    """D(x, y): distance_functions::cosine / ::pearson."""
    cx, sx = prepare(kind, x)
    cy, sy = prepare(kind, y)
    return pair_value(sx, sy, fold_xy(cx, cy))


def distance(kind: str, x, y):
    """(key, dist): the metric the tree orders by and metric2dist of it (dist.rs:19-34)."""
    key = _sqrt(value(kind, x, y))
    return key, _mul(key, key)


def nearest_neighbors(data, k: int, kind: str):
    """(indices, distances) as lists of rows of width min(k, n - 1); ordered by (key, index), the row itself excluded."""
    rows = [prepare(kind, r) for r in data]
    n = len(rows)
    k_eff = min(k, max(n - 1, 0))
    idx, dist = [], []
    for q in range(n):
        cq, sq = rows[q]
        keys = []
        for p in range(n):
            if p == q:
                continue
            cp, sp = rows[p]
            keys.append((_sqrt(pair_value(sq, sp, fold_xy(cq, cp))), p))
        keys.sort()
        idx.append([p for _, p in keys[:k_eff]])
        dist.append([_mul(key, key) for key, _ in keys[:k_eff]])
    return idx, dist
