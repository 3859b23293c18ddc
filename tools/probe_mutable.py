"""Cost of the mutable index: python tools/probe_mutable.py [N ...] [--B 1024] [--k 100] [--rounds 7]

For each corpus size N (default: a synthetic 1 M-doc index and BASELINE.json's 21 015 324 docs x 768 nnz, fp32) and B = 1024 queries of
bench.py's first batch: a plain search; the search with 0.1 % and 10 % of the rows deleted (tombstones in the handle) next to the same
search on an untouched handle under the explicit deny DocFilter (what a caller had to do before: the two launch the same FL = 1 kernels);
the tombstoned search with a shared and with a per-query user filter on top, and the AND kernel on its own (filtered search minus the
same filtered search on the untouched handle with the pre-ANDed mask); delete_rows of 1 k and 1 M device ids; compact at 10 % deleted with
the GB/s of index bytes moved (read + written) against the HBM peak bench.py uses.  Device events on torch's current stream around one
call, the variants alternate round by round after a warm-up.  Prints one JSON line per N: median / min / max ms per variant."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex
from vsearch_amd.doc_filter import DocFilter

V, NNZ_DOC, NNZ_Q, INDEX_SEED, QUERY_SEED = 29523, 768, 776, 0, 1
HBM_PEAK_GBS = 8000.0        # bench.py's HBM_PEAK_GBS


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def probe(N, B, K, rounds, per_query):
    dev = torch.device("cuda", 0)
    idx = DeviceIndex.synthetic(INDEX_SEED, 0, N, V, NNZ_DOC, 0, 0, nat.VS_F32, 0).prepare()
    gen = DeviceIndex.synthetic(QUERY_SEED, 0, B, V, NNZ_Q, 0, 0, 0, 0)             # bench.py's first query batch
    ip, ix, d = gen.export_csr()
    gen.close()
    q = torch.zeros((B, V), dtype=torch.float32, device=dev)
    q[torch.from_numpy(np.repeat(np.arange(B), np.diff(ip))).to(dev), torch.from_numpy(ix).to(dev)] = torch.from_numpy(d).to(dev)
    g = torch.Generator(device="cuda").manual_seed(3)
    r = torch.rand(N, device=dev, generator=g)
    dead = {"0.1pct": r < 0.001, "10pct": r < 0.1}
    ids = {name: torch.nonzero(m).flatten() for name, m in dead.items()}
    deny = {name: DocFilter.from_mask(~m) for name, m in dead.items()}
    user = torch.rand(N, device=dev, generator=g) < 0.5
    f_user, f_both = DocFilter.from_mask(user), DocFilter.from_mask(user & ~dead["10pct"])
    variants = {}
    state = {"dead": None}

    def with_dead(name, fn):
        def run():
            if state["dead"] != name:                                                # (outside the timed region of the next call: see below)
                idx.restore_rows()
                idx.delete_rows(ids[name])
                state["dead"] = name
                torch.cuda.synchronize()
            return fn()
        return run

    def plain(fn):
        def run():
            if state["dead"] is not None:
                idx.restore_rows()
                state["dead"] = None
                torch.cuda.synchronize()
            return fn()
        return run

    variants["search"] = plain(lambda: idx.search(q, K))
    for name in dead:
        variants[f"deny_filter_{name}"] = plain(lambda name=name: idx.search(q, K, filter=deny[name]))
        variants[f"tombstones_{name}"] = with_dead(name, lambda: idx.search(q, K))
    variants["filter_shared_pre_anded"] = plain(lambda: idx.search(q, K, filter=f_both))
    variants["tombstones_10pct_and_shared_filter"] = with_dead("10pct", lambda: idx.search(q, K, filter=f_user))
    if per_query:
        pq = torch.rand((B, N), device=dev, generator=g) < 0.5
        f_pq = DocFilter.from_mask(pq)
        f_pq_both = DocFilter.from_mask(pq & ~dead["10pct"][None, :])
        del pq
        variants["filter_per_query_pre_anded"] = plain(lambda: idx.search(q, K, filter=f_pq_both))
        variants["tombstones_10pct_and_per_query_filter"] = with_dead("10pct", lambda: idx.search(q, K, filter=f_pq))
    ids_1k = torch.randint(0, N, (1000,), device=dev, generator=g)
    ids_1m = torch.randint(0, N, (1_000_000,), device=dev, generator=g)
    def deleting(x):
        def run():
            idx.delete_rows(x)
            state["dead"] = "random"                                                 # (the next search variant restores first)
        return run

    variants["delete_rows_1k"] = deleting(ids_1k)
    variants["delete_rows_1M"] = deleting(ids_1m)
    times = {name: [] for name in variants}
    # the state switch (restore + delete) happens inside run() but before fn(): time fn() alone by switching first
    for name, fn in variants.items():                                                # warm-up (builds the bitmap, sizes the scratch)
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in variants.items():
            if not name.startswith("delete_rows"):
                fn()                                                                 # (puts the handle into the variant's state, untimed)
            times[name].append(timed(fn))
    # compaction at 10 % deleted: blocking call, wall clock around it
    idx.restore_rows()
    idx.delete_rows(ids["10pct"])
    torch.cuda.synchronize()
    info = idx.info()
    comp = []
    moved = 0
    for _ in range(3):
        t0 = time.perf_counter()
        new, old = idx.compact()
        comp.append((time.perf_counter() - t0) * 1e3)
        moved = int(info.device_bytes) + int(new.info().device_bytes)                # source read once, result written once
        new.close()
    out = {"probe": "mutable", "docs": N, "B": B, "k": K, "rounds": rounds, "device": torch.cuda.get_device_name(0), "n_live_10pct": int(old.size)}
    for name, t in times.items():
        out[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(np.min(t)), 3), "max_ms": round(float(np.max(t)), 3)}
    out["and_kernel_shared_ms"] = round(out["tombstones_10pct_and_shared_filter"]["median_ms"] - out["filter_shared_pre_anded"]["median_ms"], 3)
    if per_query:
        out["and_kernel_per_query_ms"] = round(out["tombstones_10pct_and_per_query_filter"]["median_ms"] - out["filter_per_query_pre_anded"]["median_ms"], 3)
    best = float(np.min(comp))
    out["compact_10pct"] = {"median_ms": round(float(np.median(comp)), 3), "min_ms": round(best, 3), "bytes_moved": moved,
                            "GBps": round(moved / best / 1e6, 1), "frac_of_hbm_peak": round(moved / best / 1e6 / HBM_PEAK_GBS, 4)}
    print(json.dumps(out), flush=True)
    idx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000, 21_015_324])
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-per-query", action="store_true", help="skip the per-query filter legs (B x N / 8 bytes of bitmap, twice)")
    a = ap.parse_args()
    for n in a.sizes:
        probe(n, a.B, a.k, a.rounds, not a.no_per_query)


if __name__ == "__main__":
    main()
