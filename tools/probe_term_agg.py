"""Cost of term counts: python tools/probe_term_agg.py [N ...] [--B 64] [--rounds 5] [--batch-rows 131072]

For each corpus size N (default: a synthetic 1 M-doc x 768-nnz fp32 index) and B = 64 queries of bench.py's first batch: per-query match
bitmaps from match_filter at two thresholds -- the 100th score of the plain search (a sparse set) and -inf (the full set).
  term_counts:  DeviceIndex.term_counts(filter=bitmaps) -- one vs_index_term_counts call.
  baseline:     what a caller does without it, written out below, in the same process: per query, unpack the bitmap to row ids on the GPU,
                pull the rows with get_rows and torch.bincount(indices[values != 0], minlength=n_cols).  get_rows materialises the rows, so a
                query's ids go through it in batches of --batch-rows rows (the full set does not fit in one piece: 1 M rows are 6 GB of
                cells); the batch size is part of every output line.
Both results are compared (they must be equal).  Device events on torch's current stream around one call; the two sides alternate round by
round after one warm-up.  Prints one JSON line per (N, set) row with the median, the minimum and the spread (max - min) of both sides, their
ratio, the plan (regime, chunks) and the verdict of the criterion fixed before the run: term_counts is not slower than the baseline by more
than the baseline's own spread plus 5 %.  bytes_model: the cost model of DESIGN.md 3.1k for the row -- bitmap bits + 2 B a cell of column ids
+ the value bytes of the store, over the set's rows."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, term_plan

V, NNZ_DOC, NNZ_Q, INDEX_SEED, QUERY_SEED = 29523, 768, 776, 0, 1


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def baseline(idx, words, n, batch_rows):
    """bitmap -> ids -> get_rows -> one bincount per query (and per batch of a query's ids) -> counts [B, V]"""
    shifts = torch.arange(32, device=words.device, dtype=torch.int32)
    out = torch.zeros((words.shape[0], V), dtype=torch.int64, device=words.device)
    for b in range(words.shape[0]):
        mask = (((words[b, :, None] >> shifts) & 1) != 0).reshape(-1)[:n]
        ids = torch.nonzero(mask).reshape(-1)
        for i0 in range(0, int(ids.shape[0]), batch_rows):
            _, indices, values = idx.get_rows(ids[i0:i0 + batch_rows].contiguous())
            out[b] += torch.bincount(indices[values != 0].long(), minlength=V)
    return out


def probe(N, B, rounds, batch_rows):
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
    info = idx.info()
    for set_name, f in sets.items():
        sides = {"term_counts": lambda: idx.term_counts(filter=f).counts, "baseline": lambda: baseline(idx, f.words, N, batch_rows)}
        got = {name: fn() for name, fn in sides.items()}                                 # warm-up, and the two results agree
        torch.cuda.synchronize()
        assert torch.equal(got["term_counts"], got["baseline"]), set_name
        total = idx.term_counts(filter=f).total
        del got
        times = {name: [] for name in sides}
        for _ in range(rounds):
            for name, fn in sides.items():
                times[name].append(timed(fn)[0])
        regime, chunks, rpc = term_plan(N, B, V, True)
        rows = int(total.sum().item())
        cells = rows * (info.n_packets * 8 / max(info.n_rows, 1))
        out = {"probe": "term_agg", "docs": N, "B": B, "rounds": rounds, "set": set_name, "matches_per_query_median": int(total.float().median().item()),
               "n_cols": V, "regime": "global" if regime else "lds", "chunks": chunks, "rows_per_chunk": rpc, "baseline_batch_rows": batch_rows,
               "bytes_model": int(B * N / 8 + cells * (2 + 4) + rows * 8), "device": torch.cuda.get_device_name(0)}
        for name, t in times.items():
            out[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(np.min(t)), 3),
                         "spread_ms": round(float(np.max(t) - np.min(t)), 3)}
        tm, bm = float(np.median(times["term_counts"])), float(np.median(times["baseline"]))
        margin = float(np.max(times["baseline"]) - np.min(times["baseline"])) + 0.05 * bm
        out["ratio_to_baseline"] = round(tm / bm, 4)
        out["not_slower"] = bool(tm <= bm + margin)
        print(json.dumps(out), flush=True)
    idx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000])
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch-rows", type=int, default=131072)
    a = ap.parse_args()
    for n in a.sizes:
        probe(n, a.B, a.rounds, a.batch_rows)


if __name__ == "__main__":
    main()
