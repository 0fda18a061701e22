"""merge_clusters on the device-generated 1 M x 33 k matrix (synth_counts_torch, genes x cells, cell-major) with its planted
clustering (the generator's 20 clusters) over-split into 40 labels, scores on the device: total ms of the fused route and of
the literal one (handle option merge_fused), passes over the nonzeros, candidates, rounds, merges, ms per candidate, the
medoids' ms, and the fused pass's bytes against HBM peak. One JSON line.

    python tools/merge_bench.py [--cells 1000000] [--genes 33000] [--splits 2] [--no-literal]
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
    print(json.dumps(res))


if __name__ == "__main__":
    main()
