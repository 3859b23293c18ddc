"""Cost of explaining a search's hits: python tools/probe_explain.py [N ...] [--B 1024] [--k 100] [--rounds 7]

For each corpus size N (default: a synthetic 1 M-doc index and BASELINE.json's 21 015 324 docs x 768 nnz, fp32) and B = 1024 queries:
the search's top k, then DeviceIndex.explain of those (query, id) pairs at topn = 0, 10 and 100.  Device events on torch's current
stream around one call; the variants alternate round by round after a warm-up.  GB/s counts the bytes of the explained rows (packets +
values) once per pair.  Prints one JSON line per N: median / min ms per variant and explain's share of the search."""
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
    ids, _ = idx.search(q, K)
    torch.cuda.synchronize()
    info = idx.info()
    row_bytes = (info.n_packets * 48) / max(1, info.n_rows)                          # 16 B of columns + 32 B of fp32 values a packet
    variants = {"search": lambda: idx.search(q, K)}
    for topn in (0, 10, 100):
        variants[f"explain_top{topn}"] = (lambda t: (lambda: idx.explain(q, ids, topn=t)))(topn)
    for fn in variants.values():                                                     # warm-up
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name] += timed(fn, 1)
    base = float(np.median(times["search"]))
    out = {"probe": "explain", "docs": N, "B": B, "k": K, "rounds": rounds, "row_bytes": round(row_bytes, 1), "device": torch.cuda.get_device_name(0)}
    for name, t in times.items():
        med = float(np.median(t))
        rec = {"median_ms": round(med, 3), "min_ms": round(float(np.min(t)), 3)}
        if name != "search":
            rec["GBps"] = round(B * K * row_bytes / (med * 1e-3) / 1e9, 1)
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
