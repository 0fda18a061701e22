"""merge_clusters on the device-generated 1 M x 33 k matrix (synth_counts_torch, genes x cells, cell-major) with its planted
clustering (the generator's 20 clusters) over-split into 40 labels, scores on the device: total ms of the fused route and of
the literal one (handle option merge_fused), passes over the nonzeros, candidates, rounds, merges, ms per candidate, the
medoids' ms, and the fused pass's bytes against HBM peak. One JSON line.

    python tools/merge_bench.py [--cells 1000000] [--genes 33000] [--splits 2] [--no-literal] [--shards N [--devices a,b,...]]

With --shards N a second JSON line follows: the same matrix cut over N shards of a MultiMat (`--devices`: one id per shard, default
all on device 0, which measures the overhead of the scheme, not a speed-up), scores as a host array over all cells: ms of the fused
merge_clusters call and of cluster_medoids, the exchange steps of each, the medoids' ms per radix round, the communicator's calls and
bytes per call (scanrs_multi_comm_info), the tests each shard launched, and whether labels and trace equal the single handle's bit
for bit.
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


def planted_clusters(n_cells, n_clusters, seed, device, chunk=4096):
    """The cluster of every cell as synth_counts_torch draws it (the first draw of each chunk's generator)."""
    import torch

    out = []
    for ci in range((n_cells + chunk - 1) // chunk):
        c0, c1 = ci * chunk, min(n_cells, (ci + 1) * chunk)
        g = torch.Generator(device=device)
        g.manual_seed(seed * 1000003 + 17 * ci + 1)
        out.append(torch.randint(0, n_clusters, (c1 - c0,), device=device, generator=g))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--genes", type=int, default=33_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--splits", type=int, default=2, help="labels per planted cluster")
    ap.add_argument("--dims", type=int, default=10)
    ap.add_argument("--no-literal", action="store_true")
    ap.add_argument("--shards", type=int, default=0, help="also run the fused route over this many shards of a MultiMat")
    ap.add_argument("--devices", type=str, default="", help="with --shards: comma-separated device id per shard (default: all on device 0)")
    a = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    ip, ix, vv = synth_counts_torch(a.cells, a.genes, a.density, 0, dev)
    clusters = planted_clusters(a.cells, 20, 0, dev)
    torch.cuda.synchronize()
    nnz = int(ix.numel())
    m = sa.AdaptiveMat.from_device(a.genes, a.cells, sa.CSC, ip.data_ptr(), ix.data_ptr(), vv.data_ptr())
    # scores: a centre per planted cluster plus noise; the labels cut every cluster into `splits` random parts
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    centres = torch.randn((20, a.dims), device=dev, dtype=torch.float64, generator=g) * 6.0
    scores = (centres[clusters] + torch.randn((a.cells, a.dims), device=dev, dtype=torch.float64, generator=g)).contiguous()
    part = torch.randint(0, a.splits, (a.cells,), device=dev, generator=g)
    labels = (clusters * a.splits + part).to(torch.int16).cpu().numpy()
    torch.cuda.synchronize()
    pca = sa.PcaResultDevice(0, 0, scores.data_ptr(), a.dims, a.dims, 0, a.cells)

    t0 = time.perf_counter()
    sa.medioids(pca, labels)
    t_med = (time.perf_counter() - t0) * 1e3

    def run(fused):
        m.set_option("merge_fused", 1 if fused else 0)
        t0 = time.perf_counter()
        out, tr = sa.merge_clusters(m, pca, labels, trace=True)
        return (time.perf_counter() - t0) * 1e3, out, tr

    run(True)  # warm: code objects, scratch
    t_f, out_f, tr_f = run(True)
    res = {
        "cells": a.cells, "genes": a.genes, "nnz": nnz, "labels": int(labels.max()) + 1,
        "fused_ms": round(t_f, 1), "fused_passes": tr_f.n_passes, "candidates": tr_f.n_candidates, "rounds": tr_f.n_rounds,
        "merges": tr_f.n_merges, "fused_ms_per_candidate": round(t_f / max(1, tr_f.n_candidates), 2),
        "medoids_ms": round(t_med, 2),
    }
    # the grouped pass walks the cell-major copy once: indices + values per nonzero, a label and a total per cell, and the
    # clusters x genes x 40 B accumulators it scatters into
    fused_pass_bytes = 8.0 * nnz + 10.0 * a.cells + 40.0 * (int(labels.max()) + 1) * a.genes
    res["fused_pass_bytes"] = fused_pass_bytes
    res["fused_pass_hbm_floor_ms"] = round(fused_pass_bytes / HBM_BYTES_PER_S * 1e3, 3)
    if not a.no_literal:
        t_l, out_l, tr_l = run(False)
        res.update({
            "literal_ms": round(t_l, 1), "literal_passes": tr_l.n_passes,
            "literal_ms_per_candidate": round(t_l / max(1, tr_l.n_candidates), 2),
            "same_labels": bool(np.array_equal(out_f, out_l)),
            "same_de_counts": [e[:3] for e in tr_f.entries] == [e[:3] for e in tr_l.entries],
            "max_rel_diff_min_p": float(np.nanmax(np.abs(tr_f.min_p_adj - tr_l.min_p_adj) / np.maximum(tr_l.min_p_adj, 1e-300)))
            if tr_f.n_candidates == tr_l.n_candidates and tr_f.n_candidates else None,
        })
    print(json.dumps(res), flush=True)
    if a.shards:
        m.set_option("merge_fused", 1)
        sharded_leg(a, (ip, ix, vv), scores.cpu().numpy(), labels, out_f, tr_f)


def sharded_leg(a, triplet, scores, labels, out_single, tr_single):
    devices = [int(d) for d in a.devices.split(",")] if a.devices else [0] * a.shards
    if len(devices) != a.shards:
        raise SystemExit("--devices needs one id per shard")
    ip, ix, vv = (t.cpu().numpy() for t in triplet)  # MultiMat takes the whole matrix from the host once
    t0 = time.perf_counter()
    mm = sa.MultiMat(a.genes, a.cells, sa.CSC, ip, ix, vv, a.shards, devices=devices)
    t_create = (time.perf_counter() - t0) * 1e3
    sa.cluster_medoids(mm, scores, labels)  # warm
    t0 = time.perf_counter()
    sa.cluster_medoids(mm, scores, labels)
    t_med = (time.perf_counter() - t0) * 1e3
    med_steps = mm.counter("de_shard_allreduces", 0)
    sa.merge_clusters(mm, scores, labels)  # warm
    before = [mm.comm_info(i) for i in range(a.shards)]
    t0 = time.perf_counter()
    out, tr = sa.merge_clusters(mm, scores, labels, trace=True)
    t_merge = (time.perf_counter() - t0) * 1e3
    after = [mm.comm_info(i) for i in range(a.shards)]
    same = bool(np.array_equal(out, out_single)) and all(
        getattr(tr, f).tobytes() == getattr(tr_single, f).tobytes() for f in ("leaf0", "leaf1", "n_de", "min_p_adj")) and (
        tr.n_candidates, tr.n_rounds, tr.n_merges, tr.n_passes) == (tr_single.n_candidates, tr_single.n_rounds, tr_single.n_merges, tr_single.n_passes)
    print(json.dumps({
        "shards": a.shards, "devices": devices, "cells_per_shard": [hi - lo for _, lo, hi in mm.shard_ranges()], "create_ms": round(t_create, 2),
        "sharded_fused_ms": round(t_merge, 1), "candidates": tr.n_candidates, "rounds": tr.n_rounds, "merges": tr.n_merges,
        "sharded_medoids_ms": round(t_med, 2), "medoid_exchange_steps": med_steps,
        "medoid_ms_per_radix_round": round(t_med / max(1, med_steps - 1), 3),
        "de_shard_tests": [mm.counter("de_shard_tests", i) for i in range(a.shards)],
        "de_shard_allreduces": [mm.counter("de_shard_allreduces", i) for i in range(a.shards)],
        "comm_calls_per_call": [y["allreduce_calls"] - x["allreduce_calls"] for x, y in zip(before, after)],
        "comm_bytes_per_call": [y["allreduce_bytes"] - x["allreduce_bytes"] for x, y in zip(before, after)],
        "equals_single_handle_bits": same,
    }), flush=True)
    mm.close()


if __name__ == "__main__":
    main()
