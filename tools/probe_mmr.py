"""Cost of diversified search: python tools/probe_mmr.py [N] [--B 1024] [--rounds 5] [--cases 10:64,100:400,100:1024]

For a synthetic index of N documents (default 1 M) and B = 1024 queries of bench.py's first batch, per (k, depth) case: plain search at k
and at depth, get_rows of the depth candidates of every query, the selection kernel alone over those rows (vs_mmr_select_csr, lam 0.5,
cosine), and search_diverse end to end (which chunks the rows under its default max_row_bytes) -- each also as a share of the plain search
at k.  The comparison that matters is get_rows and the kernel against the plain search at depth.  Device events on torch's current stream
around one call; medians over `rounds` after a warm-up, the variants alternating round by round.  Prints one JSON line per case."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, _search_diverse, mmr_select

V, NNZ_DOC, NNZ_Q, INDEX_SEED, QUERY_SEED = 29523, 768, 776, 0, 1


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def probe(N, B, cases, rounds):
    dev = torch.device("cuda", 0)
    idx = DeviceIndex.synthetic(INDEX_SEED, 0, N, V, NNZ_DOC, 0, 0, nat.VS_F32, 0).prepare()
    gen = DeviceIndex.synthetic(QUERY_SEED, 0, B, V, NNZ_Q, 0, 0, 0, 0)             # bench.py's first query batch
    ip, ix, d = gen.export_csr()
    gen.close()
    q = torch.zeros((B, V), dtype=torch.float32, device=dev)
    q[torch.from_numpy(np.repeat(np.arange(B), np.diff(ip))).to(dev), torch.from_numpy(ix).to(dev)] = torch.from_numpy(d).to(dev)
    for k, depth in cases:
        ids, sc = idx.search(q, depth)
        flat = ids.reshape(-1)
        rows = idx.get_rows(flat)
        chunks = []
        variants = {
            "search_k": lambda: idx.search(q, k),
            "search_depth": lambda: idx.search(q, depth),
            "get_rows": lambda: idx.get_rows(flat),
            "mmr_kernel": lambda: mmr_select(*rows, ids, sc, k, 0.5, "cosine", V, 0),
            "search_diverse": lambda: _search_diverse(idx, q, k, 0.5, depth, "cosine", None, None, chunks),
        }
        for fn in variants.values():                                                 # warm-up
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(rounds):
            for name, fn in variants.items():
                times[name].append(timed(fn))
        base = float(np.median(times["search_k"]))
        out = {"probe": "mmr", "docs": N, "B": B, "k": k, "depth": depth, "rounds": rounds, "row_bytes": int(rows[0][-1]) * 8,
               "chunks": chunks[-1], "device": torch.cuda.get_device_name(0)}
        for name, t in times.items():
            med = float(np.median(t))
            rec = {"median_ms": round(med, 3), "min_ms": round(float(np.min(t)), 3)}
            if name != "search_k":
                rec["share_of_search_k"] = round(med / base, 4)
            out[name] = rec
        print(json.dumps(out), flush=True)
        del rows
    idx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("size", nargs="?", type=int, default=1_000_000)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default="10:64,100:400,100:1024")
    a = ap.parse_args()
    probe(a.size, a.B, [tuple(int(x) for x in c.split(":")) for c in a.cases.split(",")], a.rounds)


if __name__ == "__main__":
    main()
