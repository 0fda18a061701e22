"""sum_rows_dual / mean_var_rows / sum_cols at the benchmark size: the device-generated 1 M cells x 33 k genes matrix of bench.py
(synth_counts_torch, seed 0, 3 %), genes x cells, held cell-major (CSC) and gene-major (CSR, transposed on the device with a torch
sort). Per call: the median wall time of `--reps` runs after two warm-ups (every call returns synchronised, lists and results travel
through the host as a caller's would), and beside it the two ways a caller had before these calls existed: `group_sums` with a label
per cell (disjoint lists only, u64) and `dot` with a two-column indicator panel (f64 only, no squares, walks every nonzero).
`--shards 1,2,4` adds the same calls through a MultiMat with that many shards on the one device: times, exchange
steps, communicator bytes per call, the share of the fixed-point form's pre-pass, and the bit comparison between the shard counts.
One JSON line.

    python tools/subset_bench.py [--cells 1000000] [--genes 33000] [--reps 5] [--shards 1,2,4]
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


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        del out
    return round(float(np.median(ts)), 3)


def once(fn):
    t0 = time.perf_counter()
    fn()
    return round((time.perf_counter() - t0) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--genes", type=int, default=33_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--list-share", type=float, default=0.25, help="share of the cells in each of the two lists")
    ap.add_argument("--sum-cols", type=int, default=10_000)
    ap.add_argument("--shards", type=str, default="",
                    help="comma-separated shard counts: the same calls through a MultiMat with that many shards, all on device 0")
    a = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    sa.init()
    ip, ix, vv = synth_counts_torch(a.cells, a.genes, a.density, a.seed, dev)
    nnz = int(ix.shape[0])
    shard_counts = [int(s) for s in a.shards.split(",") if s]
    host = tuple(t.cpu().numpy() for t in (ip, ix, vv)) if shard_counts else None  # a MultiMat is made from host arrays
    cm = sa.AdaptiveMat.from_device(a.genes, a.cells, sa.CSC, ip.data_ptr(), ix.data_ptr(), vv.data_ptr())
    # the same matrix gene-major: sort the nonzeros by (gene, cell)
    cell = torch.repeat_interleave(torch.arange(a.cells, device=dev, dtype=torch.int64), ip[1:] - ip[:-1])
    key, perm = torch.sort(ix.to(torch.int64) * a.cells + cell)
    del cell
    g_ip = torch.zeros(a.genes + 1, device=dev, dtype=torch.int64)
    g_ip[1:] = torch.cumsum(torch.bincount(ix.to(torch.int64), minlength=a.genes), 0)
    g_ix = (key % a.cells).to(torch.int32)
    g_vv = vv[perm].contiguous()
    del key, perm
    torch.cuda.synchronize()
    gm = sa.AdaptiveMat.from_device(a.genes, a.cells, sa.CSR, g_ip.data_ptr(), g_ix.data_ptr(), g_vv.data_ptr())
    del ip, ix, vv, g_ip, g_ix, g_vv
    torch.cuda.empty_cache()
    for h in (cm, gm):
        h.set_option("side_build", 0)  # nothing is built that a call does not ask for

    rng = np.random.default_rng(a.seed)
    n_list = int(a.cells * a.list_share)
    perm = rng.permutation(a.cells)
    la, lb = np.sort(perm[:n_list]), np.sort(perm[n_list: 2 * n_list])           # disjoint
    lc = np.sort(np.concatenate([la[: n_list // 2], perm[2 * n_list: 2 * n_list + n_list - n_list // 2]]))  # shares half of la
    few = np.sort(rng.choice(a.cells, min(a.sum_cols, a.cells), replace=False))
    labels = np.full(a.cells, -1, dtype=np.int16)
    labels[la], labels[lb] = 0, 1
    panel = np.zeros((a.cells, 2))
    panel[la, 0], panel[lb, 1] = 1.0, 1.0

    out = {"cells": a.cells, "genes": a.genes, "nnz": nnz, "cells_per_list": n_list, "reps": a.reps, "ms": {}}
    ms = out["ms"]
    check = {}
    for name, h in (("gene_major", gm), ("cell_major", cm)):
        e = ms[name] = {}
        before = (h.counter("subset_masked_passes"), h.counter("subset_scatter_passes"))
        e["sum_rows_dual_u64_disjoint"] = timed(lambda: h.sum_rows_dual(la, lb, np.uint64), a.reps)
        e["sum_rows_dual_u64_half_overlap"] = timed(lambda: h.sum_rows_dual(la, lc, np.uint64), a.reps)
        e["sum_rows_u64_one_list"] = timed(lambda: h.sum_rows(la, np.uint64), a.reps)
        after = (h.counter("subset_masked_passes"), h.counter("subset_scatter_passes"))
        e["sum_rows_route"] = "scatter" if after[1] > before[1] else "masked walk"
        before = after
        e[f"sum_cols_u64_{len(few)}"] = timed(lambda: h.sum_cols(few, np.uint64), a.reps)
        after = (h.counter("subset_masked_passes"), h.counter("subset_scatter_passes"))
        e["sum_cols_route"] = "scatter" if after[1] > before[1] else "listed vectors"
        e["existing_group_sums_disjoint"] = timed(lambda: sa.group_sums(h, labels, 2), a.reps)
        s1, s2 = h.sum_rows_dual(la, lb, np.uint64)
        gs = sa.group_sums(h, labels, 2)[0]
        assert np.array_equal(gs[:, 0], s1) and np.array_equal(gs[:, 1], s2)
        check[name] = (s1, s2, h.sum_cols(few, np.uint64))
    assert all(np.array_equal(x, y) for x, y in zip(check["gene_major"], check["cell_major"]))

    # f64 results need the copy whose outer dimension is the result axis
    e = ms["gene_major"]
    e["sum_rows_dual_f64_disjoint"] = timed(lambda: gm.sum_rows_dual(la, lb), a.reps)
    e["existing_dot_indicator_panel_f64"] = timed(lambda: gm.dot(panel), a.reps)
    e = ms["cell_major"]
    e[f"sum_cols_f64_{len(few)}"] = timed(lambda: cm.sum_cols(few), a.reps)

    # the map of normalize(CellRanger): per-cell scale (8 MB at 10^6 cells, indexed by the INNER position of the gene-major walk),
    # log2, per-gene 1/sigma
    v = gm.view()
    v.set_option("side_build", 0)
    sa.normalize(v, sa.Normalization.CellRanger)
    e = ms["gene_major_normalized"] = {}
    e["mean_var_rows_one_list"] = timed(lambda: v.mean_var_rows(la), a.reps)
    e["sum_rows_dual_f64_disjoint"] = timed(lambda: v.sum_rows_dual(la, lb), a.reps)
    e["existing_mean_var_axis_all_cells"] = timed(lambda: v.mean_var_axis(1), a.reps)
    del v

    # "subset_scatter" 0 on the cell-major handle: the first call builds the gene-major copy, later ones walk it
    cm.set_option("subset_scatter", 0)
    e = ms["cell_major_scatter_off"] = {}
    e["first_call_builds_the_other_copy"] = once(lambda: cm.sum_rows_dual(la, lb, np.uint64))
    e["sum_rows_dual_u64_disjoint"] = timed(lambda: cm.sum_rows_dual(la, lb, np.uint64), a.reps)
    if shard_counts:
        sharded(a, out, shard_counts, host, gm, check["gene_major"], la, lb, few)
    print(json.dumps(out), flush=True)


def sharded(a, out, shard_counts, host, gm, u64_unsharded, la, lb, few):
    """The calls through a MultiMat of the same matrix (genes x cells, CSC: the cells are sharded, so the sum_rows family crosses the
    shards and sum_cols runs along them), all shards on device 0. Per shard count and call: the median time, the exchange steps
    ("subset_allreduces") and the bytes a rank's communicator carried per call (scanrs_multi_comm_info); for the f64 calls the
    share of the device time that the pre-pass of the quantum takes (kernel classes "subset_fx_bound" / "subset_fx_walk" of
    shard 0); and whether the results hold the same bits at every shard count (the u64 ones also against the unsharded handle)."""
    # the unsharded f64 calls of the same lists, raw and under log_normalize (a map without a cross-shard floating-point sum)
    w = gm.view()
    w.set_option("side_build", 0)
    sa.log_normalize_with_size_factor(w, None, sa.FN_LOG2_1P)
    u = out["ms"]["gene_major_unsharded_f64"] = {}
    u["sum_rows_dual_f64_disjoint"] = timed(lambda: gm.sum_rows_dual(la, lb), a.reps)
    u["mean_var_rows_one_list"] = timed(lambda: gm.mean_var_rows(la), a.reps)
    u["mean_var_rows_one_list_log_normalized"] = timed(lambda: w.mean_var_rows(la), a.reps)
    f64_unsharded = (gm.sum_rows_dual(la, lb)[0], gm.mean_var_rows(la)[1], w.mean_var_rows(la)[1])
    del w
    out["sharded"], first = {}, None
    for n in shard_counts:
        mm = sa.MultiMat(a.genes, a.cells, sa.CSC, *host, n, devices=[0] * n)
        mm.set_option("side_build", 0)
        e = out["sharded"][str(n)] = {"ms": {}, "exchange_steps": {}, "comm_bytes_per_call": {}}

        def measure(name, fn):
            fn()  # (the first f64 call builds the gene-major copy of every shard)
            b0 = mm.comm_info(0)["allreduce_bytes"]
            e["ms"][name] = timed(fn, a.reps, warm=1)
            e["comm_bytes_per_call"][name] = (mm.comm_info(0)["allreduce_bytes"] - b0) // (a.reps + 1)
            e["exchange_steps"][name] = mm.counter("subset_allreduces")

        measure("sum_rows_dual_u64_disjoint", lambda: mm.sum_rows_dual(la, lb, np.uint64))
        measure("sum_rows_u64_one_list", lambda: mm.sum_rows(la, np.uint64))
        measure(f"sum_cols_u64_{len(few)}", lambda: mm.sum_cols(few, np.uint64))
        e["ms"]["first_f64_call_builds_the_other_copy"] = once(lambda: mm.sum_rows(la))
        measure("sum_rows_dual_f64_disjoint", lambda: mm.sum_rows_dual(la, lb))
        measure("mean_var_rows_one_list", lambda: mm.mean_var_rows(la))
        measure(f"sum_cols_f64_{len(few)}", lambda: mm.sum_cols(few))
        got = [*mm.sum_rows_dual(la, lb, np.uint64), mm.sum_cols(few, np.uint64), mm.sum_rows_dual(la, lb)[0], mm.mean_var_rows(la)[1]]
        mm.profile_enable(True)
        mm.mean_var_rows(la)
        prof = mm.profile_get(0)
        mm.profile_enable(False)
        bound, walk = (prof.get(k, {}).get("total_ms", 0.0) for k in ("subset_fx_bound", "subset_fx_walk"))
        e["mean_var_rows_device_ms_shard0"] = {"bound_pre_pass": round(bound, 3), "fixed_point_walk": round(walk, 3),
                                               "pre_pass_share": round(bound / (bound + walk), 3) if bound + walk else None}
        mm.log_normalize(None, sa.FN_LOG2_1P)
        measure("mean_var_rows_one_list_log_normalized", lambda: mm.mean_var_rows(la))
        got.append(mm.mean_var_rows(la)[1])
        mm.close()
        e["u64_equal_the_unsharded_handle"] = all(np.array_equal(x, y) for x, y in zip(got[:3], u64_unsharded))
        e["f64_max_rel_diff_to_unsharded"] = [float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300))) for x, y in zip(got[3:], f64_unsharded)]
        if first is None:
            first = got
        e["bits_equal_the_first_shard_count"] = all(x.tobytes() == y.tobytes() for x, y in zip(got, first))
        print(f"{n} shard(s) measured", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
