"""sSeq one-vs-rest differential expression on the device-generated 1 M x 33 k matrix (synth_counts_torch, genes x cells,
cell-major): ms for the parameters, the group pass and the tests, the exact-branch term count and the split between the
branches, and the group pass's one-pass bytes (8 nnz + 2 cells) against HBM. One JSON line.

    python tools/de_bench.py [--cells 1000000] [--genes 33000] [--groups 20] [--reps 3] [--backend {logspace,ratio}]
                             [--shards N [--devices a,b,...]]

The line carries `one_vs_rest_call_ms`, every repeat of the whole sseq_de_one_vs_rest call on the single handle. With --shards N a
second JSON line follows: the same matrix cut over N shards of a MultiMat (`--devices`: one id per shard, default all on device
0, which measures the overhead of the scheme, not a speed-up), the repeats of its sseq_de_one_vs_rest call, its grouped pass
(group_sums), the rest of the call (the test stage: the split tests, the gather of the p-values and the replicated host steps),
the tests each shard launched, the exchange steps and bytes per shard from scanrs_comm_info, and whether every field equals the
single handle's bit for bit.

With --control-conditions N the labels are a shared control instead: group 0 holds half the cells, the other half is spread
over N conditions, and every condition is tested against the control (mode 2, sseq_de_vs_control). The line then carries the
exact tests, their terms, the tests Ratio hands to LogSpace, and the ms of the tests and of the whole call for the backend.
With --per-pair-params that leg also times the same tests with the parameters of each pair's own union: `pairs_call_ms` for one
sseq_de_each_vs_control call (its "de_pairs_passes" / "de_pairs_literal" counters beside it), and `literal_loop_ms` for the calls it
replaces, compute_sseq_params(cell_indices = union) + sseq_differential_expression per pair, timed once on the first
`literal_loop_pairs` (at most 20) conditions. With --shards N as well, a second JSON line follows: the sseq_de_each_vs_control call over
N shards of a MultiMat, the tests each shard launched, the exchange steps, the communicator's calls and bytes per call
(scanrs_multi_comm_info), and whether every field of the results and of the per-pair parameters equals the single handle's bit for bit.
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
    ap.add_argument("--backend", choices=("logspace", "ratio"), default="logspace")
    ap.add_argument("--control-conditions", type=int, default=0)
    ap.add_argument("--per-pair-params", action="store_true", help="with --control-conditions: also time sseq_de_pairs and the per-pair literal calls")
    ap.add_argument("--no-literal-loop", action="store_true", help="with --per-pair-params: skip the loop of literal calls")
    ap.add_argument("--shards", type=int, default=0, help="also run one-vs-rest DE (with --control-conditions --per-pair-params: sseq_de_each_vs_control) over this many shards of a MultiMat")
    ap.add_argument("--devices", type=str, default="", help="with --shards: comma-separated device id per shard (default: all on device 0)")
    a = ap.parse_args()
    backend = sa.NB_EXACT_RATIO if a.backend == "ratio" else sa.NB_EXACT_LOGSPACE
    import torch

    dev = torch.device("cuda", 0)
    ip, ix, vv = synth_counts_torch(a.cells, a.genes, a.density, 0, dev)
    torch.cuda.synchronize()
    nnz = int(ix.numel())
    m = sa.AdaptiveMat.from_device(a.genes, a.cells, sa.CSC, ip.data_ptr(), ix.data_ptr(), vv.data_ptr())
    labels = np.random.default_rng(0).integers(0, a.groups, a.cells).astype(np.int16)
    if a.control_conditions:
        labels = np.zeros(a.cells, dtype=np.int16)
        other = np.random.default_rng(0).permutation(a.cells)[: a.cells // 2]
        labels[other] = 1 + np.random.default_rng(1).integers(0, a.control_conditions, len(other))

    def timed(f):
        best, out = float("inf"), None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = f()
            best = min(best, (time.perf_counter() - t0) * 1e3)
        return best, out

    t_params, params = timed(lambda: sa.compute_sseq_params(m))
    if a.control_conditions:
        return control_leg(a, m, labels, params, t_params, backend, timed, nnz, (ip, ix, vv))
    t_pass, (sums, cnt) = timed(lambda: sa.group_sums(m, labels, a.groups))
    allsum = sums.sum(axis=1)
    sf_a = np.array([params.size_factors[labels == j].sum() for j in range(a.groups)])
    sf_b = params.size_factors.sum() - sf_a
    rest = allsum[:, None] - sums
    t_tests, _ = timed(lambda: sa.sseq_de_from_sums(sums, rest, sf_a, sf_b, params, backend=backend))
    calls, whole = [], None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        whole = sa.sseq_de_one_vs_rest(m, labels, params, n_groups=a.groups, backend=backend)
        calls.append(round((time.perf_counter() - t0) * 1e3, 2))
    big = 900
    use = params.use_genes[:, None]
    asym = use & (sums > big) & (rest > big)
    trivial = ((sums + rest) == 0) | (params.gene_phi[:, None] == 0) | (sf_a[None, :] == 0) | (sf_b[None, :] == 0)
    exact = ~asym & ~trivial
    terms = int(((sums + rest + 1) * exact).sum())
    one_pass = 8.0 * nnz + 2.0 * a.cells
    extra = {} if backend == sa.NB_EXACT_LOGSPACE else {"backend": a.backend, "ratio_fallback_tests": ratio_fallbacks(sums, rest, sf_a, sf_b, params, exact)}
    print(json.dumps({
        "cells": a.cells, "genes": a.genes, "nnz": nnz, "groups": a.groups, **extra,
        "params_ms": round(t_params, 2), "group_pass_ms": round(t_pass, 2), "tests_ms": round(t_tests, 2), "one_vs_rest_call_ms": calls,
        "tests": int(a.genes * a.groups), "exact_tests": int(exact.sum()), "asymptotic_tests": int(asym.sum()), "early_return_tests": int((trivial & ~asym).sum()),
        "exact_terms": terms,
        "group_pass_bytes": one_pass, "group_pass_hbm_floor_ms": round(one_pass / HBM_BYTES_PER_S * 1e3, 3),
    }), flush=True)
    if a.shards:
        sharded_leg(a, (ip, ix, vv), labels, params, whole, backend, timed)


def sharded_leg(a, triplet, labels, params, whole, backend, timed):
    devices = [int(d) for d in a.devices.split(",")] if a.devices else [0] * a.shards
    if len(devices) != a.shards:
        raise SystemExit("--devices needs one id per shard")
    ip, ix, vv = (t.cpu().numpy() for t in triplet)  # MultiMat takes the whole matrix from the host once
    t0 = time.perf_counter()
    mm = sa.MultiMat(a.genes, a.cells, sa.CSC, ip, ix, vv, a.shards, devices=devices)
    t_create = (time.perf_counter() - t0) * 1e3
    t_params, p2 = timed(lambda: sa.compute_sseq_params(mm))
    t_pass, _ = timed(lambda: sa.group_sums(mm, labels, a.groups))
    before = [mm.comm_info(i) for i in range(a.shards)]
    calls, res = [], None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = sa.sseq_de_one_vs_rest(mm, labels, params, n_groups=a.groups, backend=backend)
        calls.append(round((time.perf_counter() - t0) * 1e3, 2))
    after = [mm.comm_info(i) for i in range(a.shards)]
    fields = ("sums_in", "sums_out", "p_values", "adjusted_p_values", "log2_fold_change", "normalized_mean_in", "normalized_mean_out")
    same = all(np.array_equal(getattr(r, f), getattr(w, f), equal_nan=f not in ("sums_in", "sums_out")) for r, w in zip(res, whole) for f in fields)
    same = same and all(np.array_equal(getattr(p2, f), getattr(params, f), equal_nan=True)
                        for f in ("size_factors", "gene_means", "gene_variances", "gene_moment_phi", "gene_phi"))
    print(json.dumps({
        "shards": a.shards, "devices": devices, "cells_per_shard": [hi - lo for _, lo, hi in mm.shard_ranges()], "create_ms": round(t_create, 2),
        "sharded_params_ms": round(t_params, 2), "sharded_group_pass_ms": round(t_pass, 2), "sharded_call_ms": calls,
        "sharded_test_stage_ms": round(min(calls) - t_pass, 2),
        "de_shard_tests": [mm.counter("de_shard_tests", i) for i in range(a.shards)],
        "de_shard_allreduces": [mm.counter("de_shard_allreduces", i) for i in range(a.shards)],
        "exchange_bytes_per_call": [(y["allreduce_bytes"] - x["allreduce_bytes"]) // a.reps for x, y in zip(before, after)],
        "equals_single_handle_bits": bool(same),
    }), flush=True)
    mm.close()


def ratio_fallbacks(xa, xb, sf_a, sf_b, params, exact):
    """The exact tests whose observed term lies below 2^-970 of the anchor's, which the Ratio backend hands to LogSpace: counted
    here from the closed form of the terms in log space (a test within rounding of the threshold may be counted either way)."""
    from scipy.special import gammaln

    n_fall = 0
    for j in range(xa.shape[1]):  # test by test: a few arrays of one value per gene at a time
        e = np.flatnonzero(exact[:, j])
        if not e.size:
            continue
        k, n = xa[e, j].astype(np.float64), (xa[e, j] + xb[e, j]).astype(np.float64)
        sar, sbr = sf_a[j] / params.gene_phi[e], sf_b[j] / params.gene_phi[e]
        # the anchor: the first k with step(k) < 1, n (sar - 1) - (sbr - 1) < k (sar + sbr - 2), else n
        aa, bb = n * (sar - 1.0) - (sbr - 1.0), sar + sbr - 2.0
        with np.errstate(all="ignore"):
            anchor = np.where(bb > 0, np.clip(np.floor(aa / bb) + 1.0, 0.0, n), np.where(aa < 0, 0.0, n))

        def ln_term(kk):
            return gammaln(sar + kk) + gammaln(sbr + n - kk) - gammaln(kk + 1.0) - gammaln(n - kk + 1.0)

        n_fall += int(np.count_nonzero(ln_term(k) - ln_term(anchor) < -970.0 * np.log(2.0)))
    return n_fall


PAIR_RESULT_FIELDS = ("sums_in", "sums_out", "p_values", "adjusted_p_values", "log2_fold_change", "normalized_mean_in", "normalized_mean_out")
PAIR_PARAM_FIELDS = ("gene_means", "gene_variances", "gene_moment_phi", "gene_phi", "use_genes", "zeta_hat", "delta", "size_factor_a", "size_factor_b",
                     "median_total", "sum_size_factors", "num_cells_a", "num_cells_b", "literal")


def sharded_pairs_leg(a, triplet, labels, groups, backend, single):
    devices = [int(d) for d in a.devices.split(",")] if a.devices else [0] * a.shards
    if len(devices) != a.shards:
        raise SystemExit("--devices needs one id per shard")
    ip, ix, vv = (t.cpu().numpy() for t in triplet)  # MultiMat takes the whole matrix from the host once
    t0 = time.perf_counter()
    mm = sa.MultiMat(a.genes, a.cells, sa.CSC, ip, ix, vv, a.shards, devices=devices)
    t_create = (time.perf_counter() - t0) * 1e3
    before = [mm.comm_info(i) for i in range(a.shards)]
    calls, got = [], None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        got = sa.sseq_de_each_vs_control(mm, labels, control=0, n_groups=groups, backend=backend)
        calls.append(round((time.perf_counter() - t0) * 1e3, 2))
    after = [mm.comm_info(i) for i in range(a.shards)]
    same = all(np.array_equal(np.asarray(getattr(r, f)), np.asarray(getattr(w, f)), equal_nan=True)
               for fields, i in ((PAIR_RESULT_FIELDS, 0), (PAIR_PARAM_FIELDS, 1)) for r, w in zip(got[i], single[i]) for f in fields)
    print(json.dumps({
        "shards": a.shards, "devices": devices, "cells_per_shard": [hi - lo for _, lo, hi in mm.shard_ranges()], "create_ms": round(t_create, 2),
        "sharded_pairs_call_ms": calls,
        "de_shard_tests": [mm.counter("de_shard_tests", i) for i in range(a.shards)],
        "de_shard_allreduces": [mm.counter("de_shard_allreduces", i) for i in range(a.shards)],
        "comm_calls_per_call": [(y["allreduce_calls"] - x["allreduce_calls"]) // a.reps for x, y in zip(before, after)],
        "comm_bytes_per_call": [(y["allreduce_bytes"] - x["allreduce_bytes"]) // a.reps for x, y in zip(before, after)],
        "equals_single_handle_bits": bool(same),
    }), flush=True)
    mm.close()


def control_leg(a, m, labels, params, t_params, backend, timed, nnz, triplet):
    groups = a.control_conditions + 1
    t_pass, (sums, cnt) = timed(lambda: sa.group_sums(m, labels, groups))
    sf = np.bincount(labels, weights=params.size_factors, minlength=groups)
    xa, xb = np.ascontiguousarray(sums[:, 1:]), np.repeat(sums[:, :1], groups - 1, axis=1)
    sf_a, sf_b = sf[1:], np.full(groups - 1, sf[0])
    t_tests, _ = timed(lambda: sa.sseq_de_from_sums(xa, xb, sf_a, sf_b, params, backend=backend))
    t_call, _ = timed(lambda: sa.sseq_de_vs_control(m, labels, params, n_groups=groups, backend=backend))
    use = params.use_genes[:, None]
    asym = use & (xa > 900) & (xb > 900)
    trivial = ((xa + xb) == 0) | (params.gene_phi[:, None] == 0) | (sf_a[None, :] == 0) | (sf_b[None, :] == 0)
    exact = ~asym & ~trivial
    pairs, single = {}, None
    if a.per_pair_params:
        t_pairs, single = timed(lambda: sa.sseq_de_each_vs_control(m, labels, control=0, n_groups=groups, backend=backend))
        n_lit = 0 if a.no_literal_loop else min(20, groups - 1)
        control = np.flatnonzero(labels == 0)
        t0 = time.perf_counter()
        for g in range(1, n_lit + 1):
            cond = np.flatnonzero(labels == g)
            pp = sa.compute_sseq_params(m, cell_indices=np.sort(np.concatenate([cond, control])))
            sa.sseq_differential_expression(m, cond, control, pp, backend=backend)
        pairs = {"pairs_call_ms": round(t_pairs, 2), "de_pairs_passes": m.counter("de_pairs_passes"), "de_pairs_literal": m.counter("de_pairs_literal"),
                 "literal_loop_ms": round((time.perf_counter() - t0) * 1e3, 2), "literal_loop_pairs": n_lit}
    print(json.dumps({
        **pairs,
        "cells": a.cells, "genes": a.genes, "nnz": nnz, "control_conditions": a.control_conditions, "control_cells": int(cnt[0]),
        "backend": a.backend, "params_ms": round(t_params, 2), "group_pass_ms": round(t_pass, 2),
        "tests_ms": round(t_tests, 2), "vs_control_call_ms": round(t_call, 2),
        "tests": int(a.genes * (groups - 1)), "exact_tests": int(exact.sum()), "asymptotic_tests": int(asym.sum()),
        "early_return_tests": int((trivial & ~asym).sum()), "exact_terms": int(((xa + xb + 1) * exact).sum()),
        "ratio_fallback_tests": ratio_fallbacks(xa, xb, sf_a, sf_b, params, exact) if backend == sa.NB_EXACT_RATIO else 0,
    }), flush=True)
    if a.shards and a.per_pair_params:
        sharded_pairs_leg(a, triplet, labels, groups, backend, single)


if __name__ == "__main__":
    main()
