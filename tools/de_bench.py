"""sSeq one-vs-rest differential expression on the device-generated 1 M x 33 k matrix (synth_counts_torch, genes x cells,
cell-major): ms for the parameters, the group pass and the tests, the exact-branch term count and the split between the
branches, and the group pass's one-pass bytes (8 nnz + 2 cells) against HBM. One JSON line.

    python tools/de_bench.py [--cells 1000000] [--genes 33000] [--groups 20] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scanrs_amd as sa  # noqa: E402
from scanrs_amd.synth import synth_counts_torch  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--genes", type=int, default=33_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    ip, ix, vv = synth_counts_torch(a.cells, a.genes, a.density, 0, dev)
    torch.cuda.synchronize()
    nnz = int(ix.numel())
    m = sa.AdaptiveMat.from_device(a.genes, a.cells, sa.CSC, ip.data_ptr(), ix.data_ptr(), vv.data_ptr())
    labels = np.random.default_rng(0).integers(0, a.groups, a.cells).astype(np.int16)

    def timed(f):
        best, out = float("inf"), None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = f()
            best = min(best, (time.perf_counter() - t0) * 1e3)
        return best, out

    t_params, params = timed(lambda: sa.compute_sseq_params(m))
    t_pass, (sums, cnt) = timed(lambda: sa.group_sums(m, labels, a.groups))
    allsum = sums.sum(axis=1)
    sf_a = np.array([params.size_factors[labels == j].sum() for j in range(a.groups)])
    sf_b = params.size_factors.sum() - sf_a
    rest = allsum[:, None] - sums
    t_tests, _ = timed(lambda: sa.sseq_de_from_sums(sums, rest, sf_a, sf_b, params))
    big = 900
    use = params.use_genes[:, None]
    asym = use & (sums > big) & (rest > big)
    trivial = ((sums + rest) == 0) | (params.gene_phi[:, None] == 0) | (sf_a[None, :] == 0) | (sf_b[None, :] == 0)
    exact = ~asym & ~trivial
    terms = int(((sums + rest + 1) * exact).sum())
    one_pass = 8.0 * nnz + 2.0 * a.cells
    print(json.dumps({
        "cells": a.cells, "genes": a.genes, "nnz": nnz, "groups": a.groups,
        "params_ms": round(t_params, 2), "group_pass_ms": round(t_pass, 2), "tests_ms": round(t_tests, 2),
        "tests": int(a.genes * a.groups), "exact_tests": int(exact.sum()), "asymptotic_tests": int(asym.sum()), "early_return_tests": int((trivial & ~asym).sum()),
        "exact_terms": terms,
        "group_pass_bytes": one_pass, "group_pass_hbm_floor_ms": round(one_pass / HBM_BYTES_PER_S * 1e3, 3),
    }))


if __name__ == "__main__":
    main()
