"""select_rows / select_cols / partition_on_thresholds at the benchmark size: the device-generated 1 M cells x 33 k genes matrix of
bench.py (synth_counts_torch, seed 0, 3 %), genes x cells, held cell-major (CSC) and gene-major (CSR). Per call: the median device
time of `--reps` runs after one warm-up (every call returns synchronised), the bytes it must read and write computed from the
shapes, GB/s and the share of the MI355X HBM peak, and beside it the host route that was the only way before these calls existed
(scipy slicing of the same matrix + AdaptiveMat.from_csmat), timed once in the same process. One JSON line per storage.

    python tools/select_bench.py [--cells 1000000] [--genes 33000] [--storages csc,csr] [--reps 5] [--no-host] [--shards N]

--shards N: the partition rows and the select rows of the table through a MultiMat of N shards, all on device 0 (on
one device this measures the overhead of the scheme, not a speed-up), with the rounds, the exchange steps and the bytes that went
through shard 0's communicator per call, and a check that the concatenated results equal the single handle's arrays.
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

HBM_BYTES_PER_S = 8.0e12  # MI355X peak (6.3e12 is what a streaming copy reaches)


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        del out
    return float(np.median(ts))


def entry(ms, nbytes, host_ms=None, **extra):
    gbs = nbytes / (ms * 1e-3) / 1e9
    e = {"ms": round(ms, 3), "GB": round(nbytes / 1e9, 3), "GB_per_s": round(gbs, 1), "share_of_hbm_peak": round(gbs * 1e9 / HBM_BYTES_PER_S, 4)}
    if host_ms is not None:
        e["host_route_ms"] = round(host_ms, 1)
        e["faster_than_host_route"] = bool(ms < host_ms)
    e.update(extra)
    return e


def same_arrays(a, b):
    return bool(all(np.array_equal(x, y) for x, y in zip(a, b)))


def sharded_cases(m, mm, storage, a, row_q, col_q, lists):
    """The rows of the table through the MultiMat mm, each against the same call on the single handle m."""
    out = {}

    def comm_delta(fn):
        before = mm.comm_info(0)
        r = fn()
        after = mm.comm_info(0)
        return r, after["allreduce_calls"] - before["allreduce_calls"], after["allreduce_bytes"] - before["allreduce_bytes"]

    for name, (row_t, col_t) in (("partition_quantile_0.1", (row_q, col_q)), ("partition_on_threshold_3", (3.0, 3.0))):
        t_rounds = timed(lambda: mm.partition_on_thresholds(row_t, col_t, filtered=False, residual=False), a.reps)
        alloc0 = (m.counter("t_alloc_us"), m.counter("alloc_calls"))  # process-wide: what the calls below spend in hipMalloc
        t_all = timed(lambda: mm.partition_on_thresholds(row_t, col_t), a.reps)
        alloc_ms, alloc_calls = (m.counter("t_alloc_us") - alloc0[0]) / 1e3 / (a.reps + 1), (m.counter("alloc_calls") - alloc0[1]) / (a.reps + 1)
        (f, r, sr, sc), calls, nbytes = comm_delta(lambda: mm.partition_on_thresholds(row_t, col_t))
        sf, sr_, ssr, ssc = m.partition_on_thresholds(row_t, col_t)
        same = bool(np.array_equal(sr, ssr) and np.array_equal(sc, ssc)) and same_arrays(f.to_csmat(), sf.to_csmat()) and same_arrays(r.to_csmat(), sr_.to_csmat())
        out[name] = {
            "ms": round(t_all, 3), "rounds_only_ms": round(t_rounds, 3), "hipmalloc_ms_per_call": round(alloc_ms, 3),
            "hipmalloc_calls_per_call": round(alloc_calls, 1), "rounds": mm.counter("partition_rounds"),
            "rounds_single_handle": m.counter("partition_rounds"), "exchange_steps": mm.counter("partition_allreduces"),
            "comm_calls": int(calls), "comm_bytes": int(nbytes), "result_shard_ranges": [[lo, hi] for _, lo, hi in f.shard_ranges()],
            "equals_single_handle": same,
        }
        f.close()
        r.close()
        del sf, sr_
    rows_outer = storage == sa.CSR
    for name, fn_m, fn_s, idx, on_sharded_axis in (
            ("select_rows_2000_ascending", mm.select_rows, m.select_rows, lists[0], rows_outer),
            ("select_rows_2000_shuffled", mm.select_rows, m.select_rows, lists[1], rows_outer),
            ("select_cols_every_second", mm.select_cols, m.select_cols, lists[2], not rows_outer)):
        if on_sharded_axis and np.any(np.diff(idx) < 0):
            out[name] = {"refused": "a list along the sharded dimension must not descend"}
            continue
        ms = timed(lambda: fn_m(idx), a.reps)
        got, calls, nbytes = comm_delta(lambda: fn_m(idx))
        want = fn_s(idx)
        out[name] = {"ms": round(ms, 3), "comm_calls": int(calls), "comm_bytes": int(nbytes), "equals_single_handle": same_arrays(got.to_csmat(), want.to_csmat())}
        got.close()
        del want
    return out


def host_upload(m, storage):
    m.sort_indices()
    return sa.AdaptiveMat.from_csmat(m.shape[0], m.shape[1], storage, m.indptr, m.indices, m.data)


def host_partition(m, mt, row_t, col_t, storage):
    """The loop on the host (m and its other orientation mt given), scipy slices, two uploads."""
    t0 = time.perf_counter()
    csr, csc = (m, mt) if storage == sa.CSR else (mt, m)
    ex_r, ex_c = np.zeros(m.shape[0], dtype=bool), np.zeros(m.shape[1], dtype=bool)
    while True:
        s = np.asarray(csc.T @ (~ex_r).astype(np.int64)).ravel()
        new_c = (s < col_t) & ~ex_c
        ex_c |= new_c
        s = np.asarray(csr @ (~ex_c).astype(np.int64)).ravel()
        new_r = (s < row_t) & ~ex_r
        ex_r |= new_r
        if not new_c.any() and not new_r.any():
            break
    kept = csr[np.flatnonzero(~ex_r)]
    f, r = kept[:, np.flatnonzero(~ex_c)], kept[:, np.flatnonzero(ex_c)]
    if storage == sa.CSC:
        f, r = f.tocsc(), r.tocsc()
    hf, hr = host_upload(f, storage), host_upload(r, storage)
    del hf, hr
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--genes", type=int, default=33_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--storages", default="csc,csr")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--select-genes", type=int, default=2000)
    ap.add_argument("--no-host", action="store_true", help="skip the host routes (device numbers only)")
    ap.add_argument("--shards", type=int, default=0, help="run the table through a MultiMat of this many shards, all on device 0")
    a = ap.parse_args()
    import scipy.sparse as sp
    import torch

    dev = torch.device("cuda", 0)
    sa.init()
    ip, ix, vv = synth_counts_torch(a.cells, a.genes, a.density, a.seed, dev)
    torch.cuda.synchronize()
    base = sa.AdaptiveMat.from_device(a.genes, a.cells, sa.CSC, ip.data_ptr(), ix.data_ptr(), vv.data_ptr())
    del ip, ix, vv
    torch.cuda.empty_cache()
    # the same matrix on the host, both orientations (the host route slices it; the gene-major handle is uploaded from it)
    indptr, indices, data = base.to_csmat()
    csc = sp.csc_matrix((data, indices.astype(np.int32), indptr.astype(np.int64)), shape=(a.genes, a.cells))
    csc.has_sorted_indices = True
    del indptr, indices, data
    nnz = int(csc.nnz)
    csr = None  # the gene-major orientation on the host: for the CSR handle and for the host routes
    if "csr" in a.storages.split(",") or not (a.no_host or a.shards):
        csr = csc.tocsr()
        csr.sort_indices()
    row_sums = np.bincount(csc.indices, weights=csc.data, minlength=a.genes)  # (exact: every sum is far below 2^53)
    col_sums = np.asarray(csc.sum(axis=0)).ravel()
    row_q, col_q = (float(np.quantile(s.astype(np.float64), 0.1, method="midpoint")) for s in (row_sums, col_sums))
    rng = np.random.default_rng(a.seed)
    genes_sorted = np.sort(rng.choice(a.genes, min(a.select_genes, a.genes), replace=False))
    genes_shuffled = rng.permutation(genes_sorted)
    every_second = np.arange(0, a.cells, 2)

    for name in a.storages.split(","):
        storage = sa.CSR if name == "csr" else sa.CSC
        host, other = (csr, csc) if storage == sa.CSR else (csc, csr)
        m = base if storage == sa.CSC else host_upload(csr, sa.CSR)
        out = {"storage": name, "cells": a.cells, "genes": a.genes, "nnz": nnz, "hbm_peak_GB_per_s": HBM_BYTES_PER_S / 1e9, "reps": a.reps}
        if a.shards:
            mm = sa.MultiMat(a.genes, a.cells, storage, host.indptr, host.indices, host.data, a.shards, devices=[0] * a.shards)
            out["shards"] = a.shards
            out["shard_ranges"] = [[lo, hi] for _, lo, hi in mm.shard_ranges()]
            out.update(sharded_cases(m, mm, storage, a, row_q, col_q, (genes_sorted, genes_shuffled, every_second)))
            mm.close()
            print(json.dumps(out), flush=True)
            if m is not base:
                del m
            continue

        def partition_case(row_t, col_t):
            t_rounds = timed(lambda: m.partition_on_thresholds(row_t, col_t, filtered=False, residual=False), a.reps)
            rounds = m.counter("partition_rounds")
            t_all = timed(lambda: m.partition_on_thresholds(row_t, col_t), a.reps)
            f, r, sr, sc = m.partition_on_thresholds(row_t, col_t)
            out_nnz = f.nnz() + r.nnz()
            del f, r
            # rounds: one masked pass over indices + counts per round for the outer sums, one for the first inner sums (+ 8 B of
            # atomics per nonzero); outputs: a count walk over the indices, a fill walk over both, both matrices written
            b_rounds = (rounds + 1) * nnz * 8 + nnz * 8
            b_out = nnz * 4 + nnz * 8 + out_nnz * 8
            h_ms = None if a.no_host else host_partition(host, other, row_t, col_t, storage)
            return {
                "rounds": int(rounds), "rows_excluded": int(a.genes - len(sr)), "cols_excluded": int(a.cells - len(sc)),
                "total": entry(t_all, b_rounds + b_out, h_ms),
                "rounds_only": entry(t_rounds, b_rounds, ms_per_round=round(t_rounds / rounds, 3)),
                "two_output_matrices": entry(max(t_all - t_rounds, 1e-3), b_out),
            }

        out["partition_quantile_0.1"] = partition_case(row_q, col_q)
        out["partition_on_threshold_3"] = partition_case(3.0, 3.0)

        def select_case(fn, host_fn, bytes_fn):
            ms = timed(fn, a.reps)
            r = fn()
            nbytes = bytes_fn(r.nnz())
            del r
            h_ms = None
            if not a.no_host:
                t0 = time.perf_counter()
                h = host_upload(host_fn(), storage)
                h_ms = (time.perf_counter() - t0) * 1e3
                del h
            return entry(ms, nbytes, h_ms)

        rows_outer = storage == sa.CSR
        gather_bytes = lambda n: n * 16  # the picked vectors read and written  # noqa: E731
        expand_bytes = lambda n: nnz * 4 + nnz * 8 + n * 8  # count walk, fill walk, the result written  # noqa: E731
        out["select_rows_2000_ascending"] = select_case(lambda: m.select_rows(genes_sorted), lambda: host[genes_sorted], gather_bytes if rows_outer else expand_bytes)
        out["select_rows_2000_shuffled"] = select_case(lambda: m.select_rows(genes_shuffled), lambda: host[genes_shuffled], gather_bytes if rows_outer else expand_bytes)
        out["select_cols_every_second"] = select_case(lambda: m.select_cols(every_second), lambda: host[:, every_second], expand_bytes if rows_outer else gather_bytes)
        print(json.dumps(out), flush=True)
        if m is not base:
            del m


if __name__ == "__main__":
    main()
