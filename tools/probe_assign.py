"""Cost of the nearest-centroid assignment: python tools/probe_assign.py [N ...] [--K 16 64 256 1024] [--rounds 5] [--batch 16] [--kmeans-k 64]

The setting of tools/probe_term_sums.py: for each corpus size N (default: a synthetic 1 M-doc x 768-nnz fp32 index with 29 523 columns) and each
K, the centroids are K stored rows (read through queries_from_rows), the metric is the dot product (no bias).
  assign:    DeviceIndex.assign(centroids) -- one vs_index_assign call: the prep kernel, the assign kernel, the slab's allocation and release.
  baseline:  what a caller can do without it, written out below, in the same process: vs_index_scores for the centroids in batches of --batch
             (it accepts a DEVICE output buffer, so no [K, N] matrix crosses to the host: a [batch, N] fp32 block stays on the GPU), followed by
             a running torch.max over the batches (value, then the lower centroid index among equals).
Both label vectors are compared; they must be equal wherever the baseline's fp32 scores separate the best two centroids (the two sides round
differently: assign sums in fp64 in stored order, the scan in its own order) -- the share of differing labels is printed, not asserted.
Device events on torch's current stream around one call; the two sides alternate round by round after one warm-up.  Prints one JSON line per (N,
K) with the median, the minimum and the spread (max - min) of both sides, their ratio, the plan and the verdict of the criterion fixed before
the run: assign counts as faster where its median is below the baseline's median by more than the baseline's own spread.
Recorded next to it: the slab's bytes and the cache traffic the cost model predicts (cells x Kp x 4 bytes), and one kmeans(K = --kmeans-k, iters
= 5) wall time split into assign and update (host timers around synchronised calls)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat
from vsearch_amd import device_index as di
from vsearch_amd.device_index import DeviceIndex, assign_plan, current_stream

V, NNZ_DOC, INDEX_SEED = 29523, 768, 0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def baseline(idx, cen, block, batch):
    """vs_index_scores into a device block [batch, N], a running max over the batches -> (labels int32 [N], values float32 [N])"""
    K, n = int(cen.shape[0]), int(block.shape[1])
    best = torch.full((n,), -float("inf"), dtype=torch.float32, device=cen.device)
    arg = torch.zeros(n, dtype=torch.int32, device=cen.device)
    for j0 in range(0, K, batch):
        b = min(batch, K - j0)
        q = cen[j0:j0 + b]
        nat.check(nat.lib().vs_index_scores(idx._h, C.c_void_p(q.data_ptr()), nat.VS_F32, V, b, C.c_void_p(block.data_ptr()), current_stream(0)))
        val, pos = block[:b].max(dim=0)                                                  # (the first of equal maxima: the lower index)
        better = val > best
        best = torch.where(better, val, best)
        arg = torch.where(better, (pos + j0).to(torch.int32), arg)
    return arg, best


def probe(N, Ks, rounds, batch, kmeans_k):
    dev = torch.device("cuda", 0)
    idx = DeviceIndex.synthetic(INDEX_SEED, 0, N, V, NNZ_DOC, 0, 0, nat.VS_F32, 0)
    idx.set_option("blocked_postings", 0)
    rng = np.random.default_rng(1)
    cells = int(idx.info().nnz)
    block = torch.empty((batch, N), dtype=torch.float32, device=dev)
    for K in Ks:
        rows = torch.from_numpy(rng.choice(N, size=K, replace=False).astype(np.int64)).to(dev)
        cen = idx.queries_from_rows(rows.unsqueeze(1).contiguous()).contiguous()
        sides = {"assign": lambda: idx.assign(cen), "baseline": lambda: baseline(idx, cen, block, batch)}
        got = {name: fn() for name, fn in sides.items()}                                 # warm-up
        torch.cuda.synchronize()
        differ = float((got["assign"][0] != got["baseline"][0]).float().mean().item())
        del got
        times = {name: [] for name in sides}
        for _ in range(rounds):
            for name, fn in sides.items():
                times[name].append(timed(fn)[0])
        w, slices, chunks, rpc, slab = assign_plan(N, K, V)
        out = {"probe": "assign", "docs": N, "K": K, "rounds": rounds, "n_cols": V, "cells": cells, "slice_w": w, "slices": slices, "chunks": chunks,
               "rows_per_chunk": rpc, "slab_bytes": slab, "model_cache_bytes": cells * w * slices * 4, "baseline_batch": batch,
               "baseline_output": "device", "labels_differ_share": differ, "device": torch.cuda.get_device_name(0)}
        for name, t in times.items():
            out[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(np.min(t)), 3),
                         "spread_ms": round(float(np.max(t) - np.min(t)), 3)}
        am, bm = float(np.median(times["assign"])), float(np.median(times["baseline"]))
        out["ratio_to_baseline"] = round(am / bm, 4)
        out["model_cache_TBps"] = round(out["model_cache_bytes"] / (am * 1e-3) / 1e12, 2)
        out["faster"] = bool(am < bm - float(np.max(times["baseline"]) - np.min(times["baseline"])))
        print(json.dumps(out), flush=True)
    if kmeans_k:
        rows = torch.from_numpy(rng.choice(N, size=kmeans_k, replace=False).astype(np.int64)).to(dev)
        start = idx.queries_from_rows(rows.unsqueeze(1).contiguous())
        spent = {"assign": 0.0, "update": 0.0}
        real_assign, real_sums = idx.assign, idx.term_sums

        def clocked(name, fn):
            def run(*args, **kw):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = fn(*args, **kw)
                torch.cuda.synchronize()
                spent[name] += time.perf_counter() - t0
                return res
            return run
        idx.assign, idx.term_sums = clocked("assign", real_assign), clocked("update", real_sums)
        di.kmeans_loop(idx, start, 1, "l2", None)                                        # warm-up
        spent = {"assign": 0.0, "update": 0.0}
        idx.assign, idx.term_sums = clocked("assign", real_assign), clocked("update", real_sums)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, _, n_iter, changed = di.kmeans_loop(idx, start, 5, "l2", None)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        print(json.dumps({"probe": "kmeans", "docs": N, "K": kmeans_k, "iters": n_iter, "changed": changed, "wall_ms": round(wall * 1e3, 1),
                          "assign_ms": round(spent["assign"] * 1e3, 1), "update_term_sums_ms": round(spent["update"] * 1e3, 1),
                          "rest_ms": round((wall - spent["assign"] - spent["update"]) * 1e3, 1)}), flush=True)
    idx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000])
    ap.add_argument("--K", nargs="*", type=int, default=[16, 64, 256, 1024])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--kmeans-k", type=int, default=64)
    a = ap.parse_args()
    for n in a.sizes:
        probe(n, a.K, a.rounds, a.batch, a.kmeans_k)


if __name__ == "__main__":
    main()
