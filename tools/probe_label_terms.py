"""Cost of the per-label term sums: python tools/probe_label_terms.py [N ...] [--K 12 64 256 1024 4096] [--rounds 5] [--items 0 512 2048 8192]
[--kmeans-k 64] [--no-counts] [--order 64 4096 16384 16385 65536]

The setting of tools/probe_term_sums.py and tools/probe_assign.py: a synthetic N-doc x 768-nnz fp32 index with 29 523 columns (default 1 M
docs), on one GPU, one process.  For every K, two label arrays -- random labels, and labels in runs of 512 rows -- and two sets -- every row,
and a random 1 % of the rows:
  label_term_sums:  DeviceIndex.label_term_sums(labels, K, filter) -- one vs_index_label_term_sums call (label order, item table, segmented sums).
  baseline:         the composition it replaces, on the same build: DocFilter.from_labels(labels, batch of 64) [& filter] and one term_sums call a
                    batch.  Beyond 256 labels the baseline runs TWO batches (128 labels) and the time is scaled by K / 128: "extrapolated": true.
  (+ the same pair for the counts: label_term_counts against from_labels + term_counts, unless --no-counts.)
Both sides must be EQUAL before anything is timed (beyond 256 labels: the rows of the two batches that ran).  Device events on torch's current
stream around one side; the two sides alternate round by round after one warm-up.  One JSON line per case with the median, the minimum and the
spread (max - min) of both sides, their ratio, the plan and the verdict of the criterion fixed before the run (the project's parity rule):
faster where the median is below the baseline's median by more than the baseline's max - min spread plus 5 %.
--items: the sums again under explicit rows_per_item values (0 = the automatic rule) at K = 64 and K = 1024, random labels, every row -- what
the automatic rule of label_term_check.h is judged by.  --kmeans-k: kmeans(K, iters = 5) from the start rows of `tools/probe_assign.py --K --kmeans-k K`, one whole
run to warm up and three timed ones, each wall time split into assign and update (host timers around synchronised calls).
--order: vs_label_order on its own (count pass, scan, place pass; device buffers, no read-back) for these label counts, random labels, every
row and the 1 % set -- the LDS regime up to 16 384 labels, whose chunk grows with the labels (label_order_chunk), and the global regime above."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat
from vsearch_amd import device_index as di
from vsearch_amd.device_index import DeviceIndex, label_term_plan
from vsearch_amd.doc_filter import DocFilter

V, NNZ_DOC, INDEX_SEED = 29523, 768, 0
BATCH = di.KMEANS_UPDATE_BATCH


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def composition(idx, lab, K, flt, call, batches=None):
    """from_labels + call (term_sums | term_counts) in batches of 64 -> the batches' (matrix, total); batches: run only the first so many"""
    out = []
    for i, b0 in enumerate(range(0, K, BATCH)):
        if batches is not None and i >= batches:
            break
        sets = DocFilter.from_labels(lab, np.arange(b0, min(K, b0 + BATCH), dtype=np.int32), device=lab.device)
        if flt is not None:
            sets = sets & flt
        out.append(tuple(call(filter=sets)))
    return out


def stats(t):
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(np.min(t)), 3), "spread_ms": round(float(np.max(t) - np.min(t)), 3)}


def case(idx, N, K, kind, lab, set_name, flt, rounds, what, rows_per_item=0):
    new_call = idx.label_term_sums if what == "sums" else idx.label_term_counts
    old_call = idx.term_sums if what == "sums" else idx.term_counts
    extrapolated = K > 256
    batches = 2 if extrapolated else None
    sides = {"new": lambda: new_call(lab, K, filter=flt, rows_per_item=rows_per_item), "baseline": lambda: composition(idx, lab, K, flt, old_call, batches)}
    got = {name: fn() for name, fn in sides.items()}                                     # warm-up, and the two sides are equal
    torch.cuda.synchronize()
    ran = sum(int(m.shape[0]) for m, _ in got["baseline"])
    equal = bool(torch.equal(got["new"][0][:ran], torch.cat([m for m, _ in got["baseline"]])) and
                 torch.equal(got["new"][1][:ran], torch.cat([t for _, t in got["baseline"]])))
    set_rows = int(got["new"][1].sum()) + int(got["new"][2][0])
    del got
    if not equal:
        print(json.dumps({"probe": "label_terms", "what": what, "K": K, "labels": kind, "set": set_name, "equal": False}), flush=True)
        raise SystemExit("the two sides differ: nothing is timed")
    times = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            times[name].append(timed(fn)[0])
    scale = K / (BATCH * 2) if extrapolated else 1.0
    base = [t * scale for t in times["baseline"]]
    tiles, tc, rpi, max_items = label_term_plan(N, K, V, rows_per_item)
    nm, bm = float(np.median(times["new"])), float(np.median(base))
    out = {"probe": "label_terms", "what": what, "docs": N, "K": K, "labels": kind, "set": set_name, "set_rows": set_rows, "rounds": rounds,
           "tiles": tiles, "tile_cols": tc, "rows_per_item": rpi, "max_items": max_items, "equal": True, "extrapolated": extrapolated,
           "new": stats(times["new"]), "baseline": stats(base), "ratio_to_baseline": round(nm / bm, 4),
           "faster": bool(nm < bm - float(np.max(base) - np.min(base)) - 0.05 * bm), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out), flush=True)


def order_case(idx, N, L, set_name, flt, rounds, rng):
    lab = torch.from_numpy(rng.integers(0, L, size=N).astype(np.int32)).to(torch.device("cuda", 0))
    call = lambda: idx._label_order_call(lab, L, flt, 0)
    ptr, _, other = call()                                                             # warm-up
    listed = int(ptr[-1]) + int(other[0])
    t = [timed(call)[0] for _ in range(rounds)]
    print(json.dumps({"probe": "label_order", "docs": N, "n_labels": L, "regime": "lds" if L <= nat.FACET_LDS_BINS else "global", "set": set_name,
                      "set_rows": listed, "rounds": rounds, **stats(t)}), flush=True)


def kmeans_split(idx, N, K):
    dev = torch.device("cuda", 0)
    rows = np.random.default_rng(1).choice(N, size=K, replace=False)                    # (the start of `tools/probe_assign.py --K --kmeans-k K`)
    rows = torch.from_numpy(rows.astype(np.int64)).to(dev)
    start = idx.queries_from_rows(rows.unsqueeze(1).contiguous())
    spent = {}
    real = {"assign": idx.assign, "update": idx.label_term_sums}

    def clocked(name, fn):
        def run(*args, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn(*args, **kw)
            torch.cuda.synchronize()
            spent[name] += time.perf_counter() - t0
            return res
        return run
    for run in range(4):                                                               # one whole run to warm up, then three timed ones
        spent.update(assign=0.0, update=0.0)
        idx.assign, idx.label_term_sums = clocked("assign", real["assign"]), clocked("update", real["update"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, _, n_iter, changed = di.kmeans_loop(idx, start, 5, "l2", None)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        if run:
            print(json.dumps({"probe": "kmeans", "docs": N, "K": K, "iters": n_iter, "changed": changed, "wall_ms": round(wall * 1e3, 1),
                              "assign_ms": round(spent["assign"] * 1e3, 1), "update_label_term_sums_ms": round(spent["update"] * 1e3, 1),
                              "rest_ms": round((wall - spent["assign"] - spent["update"]) * 1e3, 1)}), flush=True)


def probe(N, Ks, rounds, items, kmeans_k, counts, order=()):
    dev = torch.device("cuda", 0)
    idx = DeviceIndex.synthetic(INDEX_SEED, 0, N, V, NNZ_DOC, 0, 0, nat.VS_F32, 0)
    idx.set_option("blocked_postings", 0)
    rng = np.random.default_rng(1)
    sparse = DocFilter.from_mask(torch.from_numpy(rng.random(N) < 0.01), device=dev)
    for K in Ks:
        labels = {"random": rng.integers(0, K, size=N), "runs512": (np.arange(N) // 512 * 2654435761 % (1 << 32)) % K}
        for kind, lab in labels.items():
            lab = torch.from_numpy(lab.astype(np.int32)).to(dev)
            for set_name, flt in (("all", None), ("1%", sparse)):
                case(idx, N, K, kind, lab, set_name, flt, rounds, "sums")
                if counts and kind == "random":
                    case(idx, N, K, kind, lab, set_name, flt, rounds, "counts")
    for K in (64, 1024):
        if items and K in Ks:
            lab = torch.from_numpy(rng.integers(0, K, size=N).astype(np.int32)).to(dev)
            for rpi in items:
                case(idx, N, K, "random", lab, "all", None, rounds, "sums", rows_per_item=rpi)
    for L in order:
        for set_name, flt in (("all", None), ("1%", sparse)):
            order_case(idx, N, L, set_name, flt, rounds, rng)
    if kmeans_k:
        kmeans_split(idx, N, kmeans_k)
    idx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000])
    ap.add_argument("--K", nargs="*", type=int, default=[12, 64, 256, 1024, 4096])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--items", nargs="*", type=int, default=[0, 512, 2048, 8192])
    ap.add_argument("--kmeans-k", type=int, default=64)
    ap.add_argument("--no-counts", action="store_true")
    ap.add_argument("--order", nargs="*", type=int, default=[64, 4096, 16384, 16385, 65536])
    a = ap.parse_args()
    for n in a.sizes:
        probe(n, a.K, a.rounds, a.items, a.kmeans_k, not a.no_counts, a.order)


if __name__ == "__main__":
    main()
