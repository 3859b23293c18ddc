"""Cost of grouped search: python tools/probe_grouped.py [N ...] [--B 1024] [--k 100] [--rounds 5]

For each corpus size N (default: a synthetic 1 M-doc index; add 21015324 for BASELINE.json's corpus when the per-query bitmaps of a later
round fit beside it) and B = 1024 queries of bench.py's first batch, under two group laws -- `row // 8`, and a skewed one (group sizes ~ 1 / rank,
the largest holding a tenth of the rows): plain search at depth k and at depth kk_1 = 2 k m, search_grouped at m = 1 and m = 3, the collapse
kernel alone over the depth-kk_1 list, the filter kernel alone for the queries round 1 leaves incomplete, and the histogram of rounds a
grouped search takes.  Device events on torch's current stream around one call; the variants alternate round by round after a warm-up.
Prints one JSON line per (N, law)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, GroupState, _search_grouped, group_filter, topk_collapse

V, NNZ_DOC, NNZ_Q, INDEX_SEED, QUERY_SEED = 29523, 768, 776, 0, 1


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def group_law(name, N):
    if name == "div8":
        return (np.arange(N) // 8).astype(np.int32)
    rng = np.random.default_rng(9)                                   # skewed: group of a row ~ Zipf over N / 8 groups, the head holds ~ 10 %
    n_groups = max(N // 8, 2)
    w = 1.0 / np.arange(1, n_groups + 1)
    return rng.choice(n_groups, N, p=w / w.sum()).astype(np.int32)


def probe(N, B, K, rounds, laws):
    dev = torch.device("cuda", 0)
    idx = DeviceIndex.synthetic(INDEX_SEED, 0, N, V, NNZ_DOC, 0, 0, nat.VS_F32, 0).prepare()
    gen = DeviceIndex.synthetic(QUERY_SEED, 0, B, V, NNZ_Q, 0, 0, 0, 0)             # bench.py's first query batch
    ip, ix, d = gen.export_csr()
    gen.close()
    q = torch.zeros((B, V), dtype=torch.float32, device=dev)
    q[torch.from_numpy(np.repeat(np.arange(B), np.diff(ip))).to(dev), torch.from_numpy(ix).to(dev)] = torch.from_numpy(d).to(dev)
    for law in laws:
        g = torch.from_numpy(group_law(law, N)).to(dev)
        kk1 = {m: min(N, 2 * K * m) for m in (1, 3)}
        lists = {m: idx.search(q, kk1[m]) for m in (1, 3)}
        states, qmaps = {}, {}
        for m in (1, 3):                                                             # the state round 1 leaves: what the filter kernel reads
            st = GroupState(B, K, m, 0)
            topk_collapse(st, lists[m][0], lists[m][1], g, init=True, exhausted_hint=kk1[m] >= N)
            states[m] = st
            qmaps[m] = (st.status == 0).nonzero().flatten().to(torch.int32)
        scratch = {m: GroupState(B, K, m, 0) for m in (1, 3)}
        variants = {
            "search_k": lambda: idx.search(q, K),
            "search_kk1_m1": lambda: idx.search(q, kk1[1]),
            "search_kk1_m3": lambda: idx.search(q, kk1[3]),
            "search_grouped_m1": lambda: idx.search_grouped(q, K, g, per_group=1),
            "search_grouped_m3": lambda: idx.search_grouped(q, K, g, per_group=3),
            "collapse_m1": lambda: topk_collapse(scratch[1], lists[1][0], lists[1][1], g, init=True),
            "collapse_m3": lambda: topk_collapse(scratch[3], lists[3][0], lists[3][1], g, init=True),
        }
        for m in (1, 3):
            if qmaps[m].numel():
                variants[f"group_filter_m{m}"] = (lambda m=m: group_filter(states[m], g, qmaps[m]))
        for fn in variants.values():                                                 # warm-up
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(rounds):
            for name, fn in variants.items():
                times[name].append(timed(fn))
        hist = {}
        for m in (1, 3):
            left = []
            _search_grouped(idx, q, K, m, g, None, None, left_out=left)
            before = [B] + left[:-1]
            hist[f"m{m}"] = {str(r + 1): before[r] - left[r] for r in range(len(left))}       # queries complete after round r
        base = float(np.median(times["search_k"]))
        out = {"probe": "grouped", "docs": N, "law": law, "groups": int(g.max()) + 1, "B": B, "k": K, "kk1": kk1, "rounds": rounds,
               "queries_done_in_round": hist, "device": torch.cuda.get_device_name(0)}
        for name, t in times.items():
            med = float(np.median(t))
            rec = {"median_ms": round(med, 3), "min_ms": round(float(np.min(t)), 3)}
            if name != "search_k":
                rec["share_of_search_k"] = round(med / base, 4)
            out[name] = rec
        print(json.dumps(out), flush=True)
    idx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000])
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--laws", default="div8,skewed")
    a = ap.parse_args()
    for n in a.sizes:
        probe(n, a.B, a.k, a.rounds, a.laws.split(","))


if __name__ == "__main__":
    main()
