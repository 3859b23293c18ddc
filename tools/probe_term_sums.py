"""Cost of term sums: python tools/probe_term_sums.py [N ...] [--B 64] [--rounds 5] [--batch-rows 131072] [--tile-cols 9216 ...]

The setting of tools/probe_term_agg.py: for each corpus size N (default: a synthetic 1 M-doc x 768-nnz fp32 index with 29 523 columns) and
B = 64 queries of bench.py's first batch, per-query match bitmaps from match_filter at two thresholds -- the 100th score of the plain search
(a sparse set) and -inf (the full set).
  term_sums:    DeviceIndex.term_sums(filter=bitmaps) -- one vs_index_term_sums call, automatic plan.
  baseline:     what a caller does without it, written out below, in the same process: per query, unpack the bitmap to row ids on the GPU,
                pull the rows with get_rows in batches of --batch-rows rows, compute the fixed-point image of the values in torch
                (clamp, x 2^24 in fp64, round half to even, NaN -> 0) and index_add_ it into an int64 row.
Both results are compared (they must be equal).  Device events on torch's current stream around one call; the two sides alternate round by
round after one warm-up.  Prints one JSON line per (N, set) row with the median, the minimum and the spread (max - min) of both sides, their
ratio, the plan and the verdict of the criterion fixed before the run: term_sums is not slower than the baseline by more than the baseline's
own spread plus 5 %.
Recorded next to it, as information and not as a criterion: term_counts of the same sets in the same rounds (two column tiles read the column
ids twice); term_sums under each --tile-cols given (a smaller tile lets two workgroups share a CU); and the 64-bit LDS atomic adds per second
the automatic plan achieves (every non-zero cell of a set row is one add in exactly one tile's workgroup)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, term_sum_plan

V, NNZ_DOC, NNZ_Q, INDEX_SEED, QUERY_SEED = 29523, 768, 776, 0, 1
CLAMP, SCALE = float(1 << nat.TERM_FX_CLAMP_LOG2), float(1 << nat.TERM_FX_SHIFT)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def baseline(idx, words, n, batch_rows):
    """bitmap -> ids -> get_rows -> fx in torch -> one index_add_ per query (and per batch of a query's ids) -> sums [B, V] int64"""
    shifts = torch.arange(32, device=words.device, dtype=torch.int32)
    out = torch.zeros((words.shape[0], V), dtype=torch.int64, device=words.device)
    for b in range(words.shape[0]):
        mask = (((words[b, :, None] >> shifts) & 1) != 0).reshape(-1)[:n]
        ids = torch.nonzero(mask).reshape(-1)
        for i0 in range(0, int(ids.shape[0]), batch_rows):
            _, indices, values = idx.get_rows(ids[i0:i0 + batch_rows].contiguous())
            fx = torch.nan_to_num(torch.round(torch.clamp(values, -CLAMP, CLAMP).double() * SCALE), nan=0.0).to(torch.int64)
            out[b].index_add_(0, indices.long(), fx)
    return out


def probe(N, B, rounds, batch_rows, tile_cols):
    dev = torch.device("cuda", 0)
    idx = DeviceIndex.synthetic(INDEX_SEED, 0, N, V, NNZ_DOC, 0, 0, nat.VS_F32, 0)
    idx.set_option("blocked_postings", 0)
    gen = DeviceIndex.synthetic(QUERY_SEED, 0, B, V, NNZ_Q, 0, 0, 0, 0)             # bench.py's first query batch
    ip, ix, d = gen.export_csr()
    gen.close()
    q = torch.zeros((B, V), dtype=torch.float32, device=dev)
    q[torch.from_numpy(np.repeat(np.arange(B), np.diff(ip))).to(dev), torch.from_numpy(ix).to(dev)] = torch.from_numpy(d).to(dev)
    _, sc = idx.search(q, 100)
    sets = {"sparse": idx.match_filter(q, sc[:, 99].cpu().numpy().astype(np.float32)),
            "full": idx.match_filter(q, np.full(B, -np.inf, dtype=np.float32))}
    for set_name, f in sets.items():
        sides = {"term_sums": lambda: idx.term_sums(filter=f).sums, "baseline": lambda: baseline(idx, f.words, N, batch_rows),
                 "term_counts": lambda: idx.term_counts(filter=f).counts}
        for tc in tile_cols:
            sides[f"term_sums_tile_{tc}"] = (lambda tc: lambda: idx.term_sums(filter=f, tile_cols=tc).sums)(tc)
        got = {name: fn() for name, fn in sides.items()}                                 # warm-up, and the results agree
        torch.cuda.synchronize()
        assert torch.equal(got["term_sums"], got["baseline"]), set_name
        for tc in tile_cols:
            assert torch.equal(got["term_sums"], got[f"term_sums_tile_{tc}"]), (set_name, tc)
        cells = int(got["term_counts"].sum().item())                                     # the non-zero cells of the sets' rows
        total = idx.term_sums(filter=f).total
        del got
        times = {name: [] for name in sides}
        for _ in range(rounds):
            for name, fn in sides.items():
                times[name].append(timed(fn)[0])
        tiles, tcols, chunks, rpc = term_sum_plan(N, B, V, True)
        out = {"probe": "term_sums", "docs": N, "B": B, "rounds": rounds, "set": set_name, "matches_per_query_median": int(total.float().median().item()),
               "n_cols": V, "tiles": tiles, "tile_cols": tcols, "chunks": chunks, "rows_per_chunk": rpc, "baseline_batch_rows": batch_rows,
               "cells": cells, "device": torch.cuda.get_device_name(0)}
        for name, t in times.items():
            out[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(np.min(t)), 3),
                         "spread_ms": round(float(np.max(t) - np.min(t)), 3)}
        tm, bm = float(np.median(times["term_sums"])), float(np.median(times["baseline"]))
        margin = float(np.max(times["baseline"]) - np.min(times["baseline"])) + 0.05 * bm
        out["ratio_to_baseline"] = round(tm / bm, 4)
        out["ratio_to_term_counts"] = round(tm / float(np.median(times["term_counts"])), 3)
        out["lds_adds_per_s"] = round(cells / (tm * 1e-3), 0)
        out["not_slower"] = bool(tm <= bm + margin)
        print(json.dumps(out), flush=True)
    idx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000])
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch-rows", type=int, default=131072)
    ap.add_argument("--tile-cols", nargs="*", type=int, default=[9216])
    a = ap.parse_args()
    for n in a.sizes:
        probe(n, a.B, a.rounds, a.batch_rows, a.tile_cols)


if __name__ == "__main__":
    main()
