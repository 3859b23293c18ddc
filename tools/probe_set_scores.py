"""Cost of the scores of a document set: python tools/probe_set_scores.py [N ...] [--B 1 8] [--rounds 5] [--chunks 0 ...]

For each corpus size N (default: a synthetic 1 M-doc x 768-nnz fp32 index), each batch size B of bench.py's first queries and the sets "every"
(NULL bitmap), "p1" (1 % of the rows at random, per query) and "runs" (1 % of the rows in runs of 512, per query), on ONE handle:
  set_scores            the raw vs_index_set_scores call into a preallocated [B, N] block (rows_per_chunk automatic, and each --chunks value);
  range_one_query       baseline (a): vs_index_search_range(max_hits = 0) with queries_per_pass = 1 -- the same arithmetic over every row
                        without the [B, N] write (thresholds that about 100 rows pass);
  scores_then_torch     baseline (b), what a caller writes without the call for a 64-bin score histogram: vs_index_scores into a device block
                        (the one-query scan's fp32 chain: other numerics), then bucketize + bincount under the set's mask, per query;
  histogram_score       end to end: set_scores + one vs_index_value_histogram of 64 bins a query over its row and its bitmap.
Device events on torch's current stream around one call; the variants alternate round by round after a warm-up.  One JSON line per (N, B): the
median, the minimum and the spread (max - min) of every variant, each set's ratio to the every-row time, and the every-row parity with (a) by
DESIGN.md 3.1h's rule: met when the median is within (a)'s own spread plus 5 % of (a)'s median."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, current_stream, set_score_plan
from vsearch_amd.doc_filter import DocFilter

V, NNZ_DOC, NNZ_Q, INDEX_SEED, QUERY_SEED, BINS = 29523, 768, 776, 0, 1, 64


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def queries(B, dev):
    gen = DeviceIndex.synthetic(QUERY_SEED, 0, B, V, NNZ_Q, 0, 0, 0, 0)                 # bench.py's first query batch
    ip, ix, d = gen.export_csr()
    gen.close()
    q = torch.zeros((B, V), dtype=torch.float32, device=dev)
    q[torch.from_numpy(np.repeat(np.arange(B), np.diff(ip))).to(dev), torch.from_numpy(ix).to(dev)] = torch.from_numpy(d).to(dev)
    return q


def masks(N, B, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    p1 = torch.rand((B, N), device=dev, generator=g) < 0.01
    runs = (torch.rand((B, (N + 511) // 512), device=dev, generator=g) < 0.01).repeat_interleave(512, dim=1)[:, :N].contiguous()
    return {"every": None, "p1": p1, "runs": runs}


def probe(idx, N, B, rounds, chunks):
    dev = torch.device("cuda", 0)
    q = queries(B, dev)
    _, sc = idx.search(q, 100)
    thr = sc[:, 99].cpu().numpy().astype(np.float32)
    out = torch.empty((B, N), dtype=torch.float32, device=dev)
    block = torch.empty((B, N), dtype=torch.float32, device=dev)
    sets = masks(N, B, dev)
    filters = {k: (None if m is None else DocFilter.from_mask(m)) for k, m in sets.items()}
    lib, h = nat.lib(), idx._h
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def set_scores(f, rpc=0):
        nat.check(lib.vs_index_set_scores(h, ptr(q), nat.VS_F32, V, B, ptr(f.words) if f is not None else None, 0, f.ld if f is not None else 0, rpc,
                                          ptr(out), N, current_stream(0)))

    thr_dev = torch.from_numpy(thr).to(dev)
    counts = torch.empty(B, dtype=torch.int64, device=dev)

    def range_one_query():
        idx.set_queries_per_pass(1)
        try:
            nat.check(lib.vs_index_search_range(h, ptr(q), nat.VS_F32, V, B, ptr(thr_dev), 0, None, 0, 0, 0, None, None, ptr(counts), None, 0,
                                                current_stream(0)))
        finally:
            idx.set_queries_per_pass(0)

    lo = float(sc.min()) * 0.25
    hi = float(sc.max()) * 1.01
    edges = torch.linspace(lo, hi, BINS + 1, device=dev)

    def scores_then_torch(m):
        nat.check(lib.vs_index_scores(h, ptr(q), nat.VS_F32, V, B, ptr(block), current_stream(0)))
        for b in range(B):
            s = block[b] if m is None else block[b][m[b]]
            torch.bincount(torch.bucketize(s, edges, right=True), minlength=BINS + 2)

    def histogram_score(f):
        set_scores(f)
        for b in range(B):
            fb = None if f is None else DocFilter(f.words[b], N)
            idx._value_hist_call(out[b], nat.VAL_F32, edges, fb, 0, 0)

    variants = {"range_one_query": range_one_query}
    for name, f in filters.items():
        variants[f"set_scores_{name}"] = (lambda f=f: set_scores(f))
        variants[f"scores_then_torch_{name}"] = (lambda m=sets[name]: scores_then_torch(m))
        variants[f"histogram_score_{name}"] = (lambda f=f: histogram_score(f))
        for rpc in chunks:
            if rpc:
                variants[f"set_scores_{name}_rpc{rpc}"] = (lambda f=f, rpc=rpc: set_scores(f, rpc))
    for fn in variants.values():                                                         # warm-up
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    info = idx.info()
    rec = {"probe": "set_scores", "docs": N, "B": B, "rounds": rounds, "plan_chunks_rows": set_score_plan(N, B, V),
           "set_rows": {k: (N * B if m is None else int(m.sum())) for k, m in sets.items()}, "bytes_per_pass": int(info.bytes_per_pass),
           "device": torch.cuda.get_device_name(0)}
    med = {name: float(np.median(t)) for name, t in times.items()}
    for name, t in times.items():
        r = {"median_ms": round(med[name], 4), "min_ms": round(float(np.min(t)), 4), "spread_ms": round(float(np.max(t) - np.min(t)), 4)}
        if name.startswith("set_scores_"):
            r["ratio_to_every"] = round(med[name] / med["set_scores_every"], 4)
        if name.startswith("histogram_score_"):
            r["ratio_to_scores_then_torch"] = round(med[name] / med["scores_then_torch_" + name[len("histogram_score_"):]], 4)
        rec[name] = r
    a = times["range_one_query"]
    allowed = (max(a) - min(a)) + 0.05 * med["range_one_query"]
    rec["every_row_parity"] = {"ratio_to_range_one_query": round(med["set_scores_every"] / med["range_one_query"], 4),
                               "allowed_excess_ms": round(allowed, 4), "excess_ms": round(med["set_scores_every"] - med["range_one_query"], 4),
                               "met": bool(med["set_scores_every"] - med["range_one_query"] <= allowed)}
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000])
    ap.add_argument("--B", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunks", type=int, nargs="*", default=[], help="explicit rows_per_chunk values to time beside the automatic one")
    a = ap.parse_args()
    nat.require_device()
    for n in a.sizes:
        idx = DeviceIndex.synthetic(INDEX_SEED, 0, n, V, NNZ_DOC, 0, 0, nat.VS_F32, 0)
        idx.set_option("blocked_postings", 0)                                            # the baselines stream the same packets
        for B in a.B:
            probe(idx, n, B, a.rounds, a.chunks)
        idx.close()


if __name__ == "__main__":
    main()
