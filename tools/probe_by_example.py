"""Cost of query by example: python tools/probe_by_example.py [N ...] [--B 1024] [--k 100] [--rounds 7]

For each corpus size N (default: a synthetic 1 M-doc index and BASELINE.json's 21 015 324 docs x 768 nnz, fp32) and B = 1024 queries:
get_rows of B x 10 ids, queries_from_rows at m = 1 and 10, the exclusion (vs_topk_exclude of a [B, k + 10] list), and search_by_example at
m = 1, at m = 10 and at m = 10 with a = 768, next to a plain search of bench.py's first query batch.  Device events on torch's current
stream around one call; the variants alternate round by round after a warm-up.  Prints one JSON line per N: median / min ms per variant,
each one's share of the plain search, and the mean non-zeros of the m = 10 queries with and without the top-768 cut."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, resparsify, topk_exclude

V, NNZ_DOC, NNZ_Q, INDEX_SEED, QUERY_SEED = 29523, 768, 776, 0, 1


def timed(fn, rounds):
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def probe(N, B, K, rounds):
    dev = torch.device("cuda", 0)
    idx = DeviceIndex.synthetic(INDEX_SEED, 0, N, V, NNZ_DOC, 0, 0, nat.VS_F32, 0).prepare()
    gen = DeviceIndex.synthetic(QUERY_SEED, 0, B, V, NNZ_Q, 0, 0, 0, 0)             # bench.py's first query batch
    ip, ix, d = gen.export_csr()
    gen.close()
    q = torch.zeros((B, V), dtype=torch.float32, device=dev)
    q[torch.from_numpy(np.repeat(np.arange(B), np.diff(ip))).to(dev), torch.from_numpy(ix).to(dev)] = torch.from_numpy(d).to(dev)
    rng = np.random.default_rng(5)
    ids10 = torch.from_numpy(rng.integers(0, N, (B, 10))).to(dev)
    ids1 = ids10[:, :1].contiguous()
    flat = ids10.reshape(-1).contiguous()
    top_ids, top_sc = idx.search(idx.queries_from_rows(ids10), K + 10)
    torch.cuda.synchronize()
    q10 = idx.queries_from_rows(ids10)
    nnz10 = float((q10 != 0).sum(1).float().mean())
    nnz10a = float((resparsify(q10, 768, 0) != 0).sum(1).float().mean())
    variants = {
        "search": lambda: idx.search(q, K),
        "get_rows_Bx10": lambda: idx.get_rows(flat),
        "queries_from_rows_m1": lambda: idx.queries_from_rows(ids1),
        "queries_from_rows_m10": lambda: idx.queries_from_rows(ids10),
        "exclude_m10": lambda: topk_exclude(top_ids, top_sc, ids10, K, 0),
        "search_by_example_m1": lambda: idx.search_by_example(ids1, K),
        "search_by_example_m10": lambda: idx.search_by_example(ids10, K),
        "search_by_example_m10_a768": lambda: idx.search_by_example(ids10, K, a=768),
    }
    for fn in variants.values():                                                     # warm-up
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name] += timed(fn, 1)
    base = float(np.median(times["search"]))
    out = {"probe": "by_example", "docs": N, "B": B, "k": K, "rounds": rounds, "q_nnz_m10": round(nnz10, 1), "q_nnz_m10_a768": round(nnz10a, 1),
           "device": torch.cuda.get_device_name(0)}
    for name, t in times.items():
        med = float(np.median(t))
        rec = {"median_ms": round(med, 3), "min_ms": round(float(np.min(t)), 3)}
        if name != "search":
            rec["share_of_search"] = round(med / base, 4)
        out[name] = rec
    print(json.dumps(out), flush=True)
    idx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000, 21_015_324])
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    for n in a.sizes:
        probe(n, a.B, a.k, a.rounds)


if __name__ == "__main__":
    main()
