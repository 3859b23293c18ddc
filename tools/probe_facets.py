"""Cost of facet counts: python tools/probe_facets.py [N ...] [--B 64] [--rounds 5]

For each corpus size N (default: a synthetic 1 M-doc x 768-nnz fp32 index) and B = 64 queries of bench.py's first batch: per-query match
bitmaps from match_filter at two thresholds -- the 100th score of the plain search (a sparse set) and -inf (the full set) -- counted over
labels uniform over 256, 16 384 and 1 000 000 values, and over one label for every row (the most contended case).
  facet_counts:  DeviceIndex.facet_counts(labels, n_labels, filter=bitmaps) -- one vs_index_facet_counts call.
  baseline:      what a caller does without it, in the same process: unpack the [B, W] bitmap to [B, N] bools on the GPU, then
                 torch.bincount(labels[mask[b]], minlength=n_labels) once per query.
Both results are compared (they must be equal).  Device events on torch's current stream around one call; the two sides alternate round by
round after one warm-up.  Prints one JSON line per (N, set, labels) row with the median, the minimum and the spread (max - min) of both
sides, their ratio, and the verdict of the criterion fixed before the run: facet_counts is not slower than the baseline by more than the
baseline's own spread plus 5 %."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, facet_plan

V, NNZ_DOC, NNZ_Q, INDEX_SEED, QUERY_SEED = 29523, 768, 776, 0, 1
LABEL_SETS = (("uniform_256", 256), ("uniform_16384", 16384), ("uniform_1000000", 1_000_000), ("one_label", 1))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def baseline(words, n, labels64, n_labels):
    """unpack to bools, then one bincount per query -> counts [B, n_labels]"""
    shifts = torch.arange(32, device=words.device, dtype=torch.int32)
    mask = (((words[:, :, None] >> shifts) & 1) != 0).reshape(words.shape[0], -1)[:, :n]
    return torch.stack([torch.bincount(labels64[mask[b]], minlength=n_labels) for b in range(words.shape[0])])


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
    sets = {"sparse": idx.match_filter(q, sc[:, 99].cpu().numpy().astype(np.float32)),
            "full": idx.match_filter(q, np.full(B, -np.inf, dtype=np.float32))}
    gen_t = torch.Generator(device=dev).manual_seed(7)
    for set_name, f in sets.items():
        matches = int(idx.facet_counts(torch.zeros(N, dtype=torch.int32, device=dev), 1, filter=f).total.float().median().item())
        for lab_name, L in LABEL_SETS:
            labels = torch.randint(0, L, (N,), generator=gen_t, device=dev, dtype=torch.int32) if L > 1 else torch.zeros(N, dtype=torch.int32, device=dev)
            labels64 = labels.long()
            sides = {"facet_counts": lambda: idx.facet_counts(labels, L, filter=f).counts, "baseline": lambda: baseline(f.words, N, labels64, L)}
            got = {name: fn() for name, fn in sides.items()}                             # warm-up, and the two results agree
            torch.cuda.synchronize()
            assert torch.equal(got["facet_counts"], got["baseline"]), (set_name, lab_name)
            del got
            times = {name: [] for name in sides}
            for _ in range(rounds):
                for name, fn in sides.items():
                    times[name].append(timed(fn)[0])
            regime, qt, chunks, rpc = facet_plan(N, B, L, True)
            out = {"probe": "facets", "docs": N, "B": B, "rounds": rounds, "set": set_name, "matches_per_query_median": matches, "labels": lab_name,
                   "n_labels": L, "regime": "global" if regime else "lds", "qt": qt, "chunks": chunks, "rows_per_chunk": rpc,
                   "device": torch.cuda.get_device_name(0)}
            for name, t in times.items():
                out[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(np.min(t)), 3),
                             "spread_ms": round(float(np.max(t) - np.min(t)), 3)}
            fm, bm = float(np.median(times["facet_counts"])), float(np.median(times["baseline"]))
            margin = float(np.max(times["baseline"]) - np.min(times["baseline"])) + 0.05 * bm
            out["ratio_to_baseline"] = round(fm / bm, 4)
            out["not_slower"] = bool(fm <= bm + margin)
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
