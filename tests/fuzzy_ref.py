"""umap-rs/src/fuzzy.rs:30-181 and embedding.rs:38-53, 75-85 restated in plain Python floats, loops in the reference's order
(DESIGN.md §7r). The exponential is a parameter, `exp_many(list) -> list` (one call per fold, so that the library's own exponential
can be passed without a foreign call per element); the folds themselves run here, in column order. Where the reference would panic
(an index past the end of non_zero_dist) `Refused(row)` is raised. Besides the results, every row reports whether it is MARGINAL:
in some bisection step |psum - target| lies within k * 2^-50 of 1e-5, or within k * 2^-50 of 0 where the step goes on to compare
psum with target: the two comparisons a different (1 ulp) exponential could decide the other way (k * 2^-50 bounds what two
exponentials within 1 ulp of the truth each can move a sum of k terms <= 1). A step that breaks with |psum - target| far below 1e-5
never compares psum with target, so a sum that merely lands on the target is not marginal."""
import math
import sys

F64_MAX = sys.float_info.max
NO_INDEX = 0xFFFFFFFF
BANDWIDTH, NITER, SMOOTH_K_TOLERANCE, MIN_K_DIST_SCALE = 1.0, 64, 1e-5, 1e-3
TREE = 256


class Refused(Exception):
    def __init__(self, row):
        super().__init__(f"row {row}")
        self.row = row


def math_exp_many(xs):
    return [math.exp(x) for x in xs]


def fmax(a, b):
    """f64::max: the other operand where one is NaN"""
    if a != a:
        return b
    if b != b:
        return a
    return b if a < b else a


def rho_of_row(row, local_connectivity):
    """fuzzy.rs:79-99; IndexError where the reference panics"""
    non_zero_dist = [d for d in row if d > 0.0]
    rho = 0.0
    if len(non_zero_dist) >= int(local_connectivity):  # `as usize` truncates
        index = math.floor(local_connectivity)
        interpolation = local_connectivity - index
        if index > 0.0:
            index = int(index)
            rho = non_zero_dist[index - 1]
            if interpolation > SMOOTH_K_TOLERANCE:
                rho += interpolation * (non_zero_dist[index] - non_zero_dist[index - 1])
        else:
            rho = interpolation * non_zero_dist[0]
    elif non_zero_dist:
        rho = -F64_MAX
        for b in non_zero_dist:
            rho = fmax(rho, b)
    return rho


def smooth_knn_dist(distances, rho, k, bandwidth, n_iter, exp_many=math_exp_many, repaired=False):
    """fuzzy.rs:117-145 -> (sigma, iterations, marginal). repaired=True folds v - rho where the reference folds v (tests only)."""
    target = math.log2(float(k)) * bandwidth
    lo, mid, hi = 0.0, 1.0, F64_MAX
    margin = k * 2.0 ** -50
    iterations, marginal = 0, False
    for _ in range(n_iter):
        iterations += 1
        args = [-(fmax(fmax((v - rho) if repaired else v, -rho), 0.0) / mid) for v in distances]
        psum = 0.0
        for e in exp_many(args):
            psum = psum + e
        gap = abs(psum - target)
        if abs(gap - SMOOTH_K_TOLERANCE) <= margin:  # the break could go the other way
            marginal = True
        if gap < SMOOTH_K_TOLERANCE:
            break
        if gap <= margin:  # `psum > target` is reached and could go the other way (never while k * 2^-50 < 1e-5: it broke above)
            marginal = True
        if psum > target:
            hi = mid
            mid = lo + (hi - lo) / 2.0
        else:
            lo = mid
            if hi == F64_MAX:
                mid *= 2.0
            else:
                mid = lo + (hi - lo) / 2.0
    return mid, iterations, marginal


def tree_total(folds):
    """the library's fixed tree over the row folds (the stated deviation from the sequential global mean)"""
    cur = list(folds)
    while True:
        nxt = []
        for b in range(0, len(cur), TREE):
            a = cur[b:b + TREE] + [0.0] * (TREE - len(cur[b:b + TREE]))
            s = TREE // 2
            while s >= 1:
                for t in range(s):
                    a[t] = a[t] + a[t + s]
                s //= 2
            nxt.append(a[0])
        cur = nxt
        if len(cur) == 1:
            return cur[0]


def smooth_knn_distances(dist, local_connectivity, n_iter, bandwidth, exp_many=math_exp_many, total="sequential"):
    """fuzzy.rs:65-114 -> (sigmas, rhos, iterations, marginal). total: "sequential" = the reference's fold over all n * k distances,
    "tree" = the library's tree over the row folds."""
    n, k = len(dist), len(dist[0])
    rhos = []
    for i in range(n):
        try:
            rhos.append(rho_of_row(dist[i], local_connectivity))
        except IndexError:
            raise Refused(i)
    folds = []
    for i in range(n):
        acc = 0.0
        for v in dist[i]:
            acc = acc + v
        folds.append(acc)
    if total == "sequential":
        acc = 0.0
        for i in range(n):
            for v in dist[i]:
                acc = acc + v
    else:
        acc = tree_total(folds)
    global_mean_distance = acc / (float(n) * float(k))
    sigmas, iters, marg, raw = [], [], [], []
    for i in range(n):
        s, it, m = smooth_knn_dist(dist[i], rhos[i], k, bandwidth, n_iter, exp_many)
        raw.append(s)
        if rhos[i] > 0.0:
            mean_ith_distances = folds[i] / float(k)
            if s < MIN_K_DIST_SCALE * mean_ith_distances:
                s = MIN_K_DIST_SCALE * mean_ith_distances
        elif s < MIN_K_DIST_SCALE * global_mean_distance:
            s = MIN_K_DIST_SCALE * global_mean_distance
        sigmas.append(s)
        iters.append(it)
        marg.append(m)
    smooth_knn_distances.last_raw = raw  # sigma before the floor, for the tests that compare the two global means
    return sigmas, rhos, iters, marg


def sequential_global_floor(dist, raw_sigma):
    """sigma of a row whose rho is not > 0 under the reference's sequential global mean (fuzzy.rs:76, 109-111)"""
    n, k = len(dist), len(dist[0])
    acc = 0.0
    for i in range(n):
        for v in dist[i]:
            acc = acc + v
    m = MIN_K_DIST_SCALE * (acc / (float(n) * float(k)))
    return [m if s < m else s for s in raw_sigma]


def compute_membership_strengths(idx, dist, sigmas, rhos, exp_many=math_exp_many):
    """fuzzy.rs:148-181 -> (rows, cols, values)"""
    rows, cols, values = [], [], []
    where, args = [], []  # the exponentials are element-wise: formed in one call behind the loop
    for i in range(len(idx)):
        for j in range(len(idx[i])):
            if idx[i][j] == NO_INDEX:
                continue
            if j == idx[i][j]:  # the column position against the index, as the reference writes it
                val = 0.0
            elif dist[i][j] - rhos[i] <= 0.0 or sigmas[i] == 0.0:
                val = 1.0
            else:
                val = None
                where.append(len(values))
                args.append(-((dist[i][j] - rhos[i]) / sigmas[i]))
            cols.append(i)
            rows.append(idx[i][j])
            values.append(val)
    for p, e in zip(where, exp_many(args) if args else []):
        values[p] = e
    return rows, cols, values


def fuzzy_simplicial_set(idx, dist, local_connectivity=1.0, set_operation_ratio=1.0, apply_fuzzy_combine=True, n_iter=None, bandwidth=None,
                         exp_many=math_exp_many, total="sequential"):
    """fuzzy.rs:30-62 -> dict(indptr, indices, values, sigmas, rhos, iterations, marginal). The lists must not name a row twice."""
    n = len(idx)
    n_iter = NITER if not n_iter else n_iter
    bandwidth = BANDWIDTH if not bandwidth else bandwidth
    sigmas, rhos, iters, marg = smooth_knn_distances(dist, local_connectivity, n_iter, bandwidth, exp_many, total)
    rows, cols, values = compute_membership_strengths(idx, dist, sigmas, rhos, exp_many)
    r = {}
    for a, b, v in zip(rows, cols, values):
        assert (a, b) not in r, "a repeated index: TriMat would add, the library refuses"
        r[a, b] = v
    if apply_fuzzy_combine:
        out = {}
        for (a, b) in set(r) | {(b, a) for (a, b) in r}:
            x, t = r.get((a, b), 0.0), r.get((b, a), 0.0)
            sum_ = x + t
            prod = x * t
            lhs = (sum_ - prod) * set_operation_ratio
            rhs = prod * (1.0 - set_operation_ratio)
            out[a, b] = lhs + rhs
    else:
        out = r
    indptr, indices, vals = [0] * (n + 1), [], []
    for (a, b) in sorted(out):
        indptr[a + 1] += 1
        indices.append(b)
        vals.append(out[a, b])
    for a in range(n):
        indptr[a + 1] += indptr[a]
    return dict(indptr=indptr, indices=indices, values=vals, sigmas=sigmas, rhos=rhos, iterations=iters, marginal=marg,
                raw_sigmas=smooth_knn_distances.last_raw)


def union_pattern_scipy(idx, n):
    """the structure a second way: the pattern of R + R^T - R.multiply(R^T) with scipy.sparse, every stored entry counted (ones as
    values, so that nothing cancels): (indptr, indices) of the union, (indptr, indices) of R alone"""
    import numpy as np
    import scipy.sparse as sp

    rows = [c for row in idx for c in row if c != NO_INDEX]
    cols = [i for i, row in enumerate(idx) for c in row if c != NO_INDEX]
    r = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    rt = sp.csr_matrix(r.T)
    u = sp.csr_matrix(r + rt - 0.5 * r.multiply(rt))
    u.sort_indices()
    r.sort_indices()
    assert u.nnz == (r + rt).nnz
    return (u.indptr.tolist(), u.indices.tolist()), (r.indptr.tolist(), r.indices.tolist())


def edges(indptr, indices, values, n_epochs):
    """embedding.rs:38-53 without the shuffle, and make_epochs_per_sample (75-85): (head, tail, weights, epochs_per_sample)"""
    graph_max = 0.0
    for v in values:
        graph_max = fmax(graph_max, v)
    pruned = [0.0 if v < graph_max / n_epochs else v for v in values]
    head, tail, weights = [], [], []
    for row in range(len(indptr) - 1):
        for e in range(indptr[row], indptr[row + 1]):
            if pruned[e] != 0.0:
                weights.append(pruned[e])
                tail.append(row)
                head.append(indices[e])
    mx = -F64_MAX
    for w in weights:
        mx = fmax(mx, w)
    eps = []
    for w in weights:
        nn = (w / mx) * n_epochs
        eps.append(n_epochs / nn if nn > 0.0 else -1.0)
    return head, tail, weights, eps
