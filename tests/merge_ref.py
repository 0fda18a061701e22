"""CPU restatement of the reference's merge_clusters (scan-rs/src/merge_clusters.rs), complete linkage (linkage.rs) and
median_mut (stats.rs:13-39), line for line, over the sSeq restatement tests/sseq_ref.py. The checker of the library's
cluster.py. Matrices are scipy.sparse, genes x cells."""
from __future__ import annotations

import math

import numpy as np

import sseq_ref as ref

ADJUSTED_P_VALUE_THRESHOLD = 0.05


# ---- stats.rs ---------------------------------------------------------------------------------------------------------------
def median_mut(xs):
    """stats.rs:13-39: a full sort; xs[n / 2] for an odd n, (xs[n / 2] + xs[n / 2 - 1]) / 2 for an even one."""
    if len(xs) == 0:
        raise ValueError("EmptyInput")
    s = sorted(xs)
    n = len(s)
    if n % 2 == 0:
        a, b = s[n // 2], s[n // 2 - 1]
        if isinstance(a, (int, np.integer)):
            return (a + b) // 2  # T::from_u64(2) division of an integer type
        return (a + b) / 2
    return s[n // 2]


# ---- linkage.rs -------------------------------------------------------------------------------------------------------------
def euclidean(x, y):
    d = 0.0
    for i in range(len(x)):
        k = float(x[i]) - float(y[i])
        d += k * k
    return math.sqrt(d)


def pdist(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.shape[0]
    d = np.zeros(m * (m - 1) // 2)
    k = 0
    for i in range(m):
        for j in range(i + 1, m):
            d[k] = euclidean(x[i], x[j])
            k += 1
    return d


def utidx(m, a, b):
    if a < b:
        return m * a - (a * (a + 1) // 2) + b - a - 1
    return m * b - (b * (b + 1) // 2) + a - b - 1


def sort_by_column(z, col):
    order = sorted(range(z.shape[0]), key=lambda i: (z[i, col], i))
    return z[order].copy()


def relabel(z, m):
    parents = list(range(2 * m - 1))
    sizes = [1] * (2 * m - 1)
    nxt = m

    def find(i):
        p = i
        while parents[i] != i:
            i = parents[i]
        while parents[p] != i:
            p = parents[p]
            parents[p] = i
        return i

    for i in range(m - 1):
        a, b = int(z[i, 0]), int(z[i, 1])
        pa, pb = find(a), find(b)
        z[i, 0], z[i, 1] = (pa, pb) if pa < pb else (pb, pa)
        parents[pa] = nxt
        parents[pb] = nxt
        sizes[nxt] = sizes[pa] + sizes[pb]
        z[i, 3] = sizes[nxt]
        nxt += 1


def nn_chain(d, m):
    d = np.array(d, dtype=np.float64)
    z = np.zeros((m - 1, 4))
    sizes = [1] * m
    chain = [0] * m
    chain_length = 0
    b = 0
    for i in range(m - 1):
        if chain_length == 0:
            chain_length = 1
            for j in range(m):
                if sizes[j] > 0:
                    chain[0] = j
                    break
        while True:
            a = chain[chain_length - 1]
            if chain_length > 1:
                b = chain[chain_length - 2]
                curr_min = d[utidx(m, a, b)]
            else:
                curr_min = math.inf
            for c in range(m):
                if sizes[c] == 0 or a == c:
                    continue
                acdist = d[utidx(m, a, c)]
                if acdist < curr_min:
                    curr_min = acdist
                    b = c
            if chain_length > 1 and b == chain[chain_length - 2]:
                break
            chain[chain_length] = b
            chain_length += 1
        chain_length -= 2
        if a > b:
            a, b = b, a
        asz, bsz = sizes[a], sizes[b]
        z[i] = (a, b, curr_min, asz + bsz)
        sizes[a] = 0
        sizes[b] = asz + bsz
        for j in range(m):
            if sizes[j] == 0 or j == b:
                continue
            d[utidx(m, j, b)] = max(d[utidx(m, j, a)], d[utidx(m, j, b)])
    z = sort_by_column(z, 2)
    relabel(z, m)
    return z


def linkage(x):
    x = np.asarray(x, dtype=np.float64)
    return nn_chain(pdist(x), x.shape[0])


# ---- merge_clusters.rs ------------------------------------------------------------------------------------------------------
def bincount(values):
    res = {}
    for v in values:
        res[int(v)] = res.get(int(v), 0) + 1
    return dict(sorted(res.items()))


def medioids(pca, labels, bins):
    pca = np.asarray(pca, dtype=np.float64)
    labels = np.asarray(labels)
    res = np.zeros((len(bins), pca.shape[1]))
    for i, label in enumerate(bins):
        rows = pca[labels == label]
        for c in range(pca.shape[1]):
            res[i, c] = median_mut(list(rows[:, c]))
    return res


def relabel_by_size(labels):
    hist = list(bincount(labels).items())
    hist.sort(key=lambda t: -t[1])  # stable
    mp = {lab: i for i, (lab, _) in enumerate(hist)}
    return np.array([mp[int(x)] for x in labels], dtype=np.int16)


def merge_clusters(mat, pca, labels):
    """Returns (labels, trace): trace entries (leaf0, leaf1, n_de, smallest adjusted p) in evaluation order, and the
    totals (candidates, rounds, merges)."""
    labels = np.array(labels, dtype=np.int16)
    m = len(labels)
    trace = []
    rounds = merges = 0
    if m == 0:
        return np.zeros(0, dtype=np.int16), dict(entries=trace, n_candidates=0, n_rounds=0, n_merges=0)
    seen_pairs = set()
    while True:
        rounds += 1
        bins = bincount(labels)
        centers = medioids(pca, labels, bins)
        z = linkage(centers)
        max_label = float(labels.max())
        any_merged = False
        for i in range(z.shape[0]):
            if z[i, 0] <= max_label and z[i, 1] <= max_label:
                leaf0, leaf1 = int(z[i, 0]), int(z[i, 1])
                group0 = np.flatnonzero(labels == leaf0)
                group1 = np.flatnonzero(labels == leaf1)
                key = (tuple(group0), tuple(group1))
                if key in seen_pairs:
                    continue
                seen_pairs.add(key)
                cell_indices = np.sort(np.concatenate([group0, group1]))
                params = ref.compute_sseq_params(mat, cell_indices=cell_indices)
                de = ref.differential_expression(mat, group0, group1, params)
                padj = de["adjusted_p_values"]
                n_de = int(np.sum(padj < ADJUSTED_P_VALUE_THRESHOLD))
                ok = padj[~np.isnan(padj)]
                trace.append((leaf0, leaf1, n_de, float(ok.min()) if ok.size else math.nan))
                if n_de == 0:
                    labels = np.where(labels == leaf1, leaf0, np.where(labels > leaf1, labels - 1, labels)).astype(np.int16)
                    merges += 1
                    any_merged = True
                    break
        if not any_merged:
            break
    return relabel_by_size(labels), dict(entries=trace, n_candidates=len(trace), n_rounds=rounds, n_merges=merges)
