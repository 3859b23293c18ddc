"""Cost of range search: python tools/probe_range.py [N ...] [--B 64] [--rounds 5]

For each corpus size N (default: a synthetic 1 M-doc x 768-nnz fp32 index) and B = 64 queries of bench.py's first batch, on ONE handle with
option blocked_postings = 0 (range search never takes the postings; the baseline must stream the same packets):
  search_range at max_hits in {0, 100, 512}, at per-query thresholds that about 100 rows pass (the 100th score of the plain search), and the
  same at thr = -inf (every row matches: the worst case of the match counter and of the candidate buffers);
  for comparison the unchanged top-k tile scan, search(k = max_hits), and the one-query range scan (queries_per_pass = 1) at max_hits = 100.
Device events on torch's current stream around one call; the variants alternate round by round after a warm-up.  Prints one JSON line per N
with the median, the minimum and the spread (max - min) of every variant, and the range scans' ratio to their baseline."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex

V, NNZ_DOC, NNZ_Q, INDEX_SEED, QUERY_SEED = 29523, 768, 776, 0, 1


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def probe(N, B, rounds):
    dev = torch.device("cuda", 0)
    idx = DeviceIndex.synthetic(INDEX_SEED, 0, N, V, NNZ_DOC, 0, 0, nat.VS_F32, 0)
    idx.set_option("blocked_postings", 0)
    gen = DeviceIndex.synthetic(QUERY_SEED, 0, B, V, NNZ_Q, 0, 0, 0, 0)             # bench.py's first query batch
    ip, ix, d = gen.export_csr()
    gen.close()
    q = torch.zeros((B, V), dtype=torch.float32, device=dev)
    q[torch.from_numpy(np.repeat(np.arange(B), np.diff(ip))).to(dev), torch.from_numpy(ix).to(dev)] = torch.from_numpy(d).to(dev)
    _, sc = idx.search(q, 100)
    assert idx.info().last_path == 1, "the baseline is the tile scan"
    thr = sc[:, 99].cpu().numpy().astype(np.float32)                                 # the tile scan's own (exact) scores: >= 100 rows pass
    counts = idx.count_matches(q, thr).cpu().numpy()
    lo = np.full(B, -np.inf, dtype=np.float32)

    def one_query():
        idx.set_queries_per_pass(1)
        try:
            idx.search_range(q, thr, max_hits=100)
        finally:
            idx.set_queries_per_pass(0)
    variants = {"search_k100": lambda: idx.search(q, 100), "search_k512": lambda: idx.search(q, 512)}
    for name, t in (("thr", thr), ("all", lo)):
        for mh in (0, 100, 512):
            variants[f"range_{name}_h{mh}"] = (lambda t=t, mh=mh: idx.search_range(q, t, max_hits=mh))
    variants["range_thr_h100_one_query"] = one_query
    for fn in variants.values():                                                     # warm-up
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    info = idx.info()
    out = {"probe": "range", "docs": N, "B": B, "rounds": rounds, "matches_per_query_median": float(np.median(counts)),
           "bytes_per_pass": int(info.bytes_per_pass), "device": torch.cuda.get_device_name(0)}
    med = {name: float(np.median(t)) for name, t in times.items()}
    for name, t in times.items():
        rec = {"median_ms": round(med[name], 3), "min_ms": round(float(np.min(t)), 3), "spread_ms": round(float(np.max(t) - np.min(t)), 3)}
        if name.startswith("range_") and not name.endswith("one_query"):
            base = "search_k512" if name.endswith("h512") else "search_k100"
            rec["ratio_to_" + base] = round(med[name] / med[base], 4)
        out[name] = rec
    print(json.dumps(out), flush=True)
    idx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000])
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    for n in a.sizes:
        probe(n, a.B, a.rounds)


if __name__ == "__main__":
    main()
