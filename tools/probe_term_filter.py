"""Measure the term-filter scan (vs_index_term_bitmaps) and DocFilter.from_terms on one MI355X against (a) a plain device read of the same
column-id bytes and (c) what a caller had to do before: export_csr to the host and a torch mask.  Prints one JSON line per figure and a
markdown table; needs a GPU (no fallback).

    python tools/probe_term_filter.py [--rows 1000000] [--nnz 768] [--reps 20] [--no-baseline] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, reps, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--nnz", type=int, default=768)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-baseline", action="store_true", help="skip (c), the export_csr + torch mask a caller needed before")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from vsearch_amd import _native as nat
    from vsearch_amd.device_index import DeviceIndex
    from vsearch_amd.doc_filter import DocFilter
    nat.require_device()
    V = 29523
    idx = DeviceIndex.synthetic(1, 0, args.rows, V, args.nnz)
    info = idx.info()
    col_bytes = int(info.n_packets) * 16
    rows = []

    def report(name, ms, lo, hi, **kw):
        rec = dict(name=name, median_ms=round(ms, 4), min_ms=round(lo, 4), max_ms=round(hi, 4), **kw)
        rows.append(rec)
        print(json.dumps(rec), flush=True)

    # (a) the floor: the same bytes read once -- a device-to-device copy (reads and writes them: halved) and a sum over them
    src = torch.empty(col_bytes // 8, dtype=torch.int64, device="cuda").random_()
    dst = torch.empty_like(src)
    ms, lo, hi = median_ms(lambda: dst.copy_(src), args.reps)
    report("floor: d2d copy of the column ids, halved", ms / 2, lo / 2, hi / 2, bytes=col_bytes, GBps=round(col_bytes / (ms / 2) / 1e6, 1))
    floor = ms / 2
    ms, lo, hi = median_ms(lambda: src.sum(), args.reps)
    report("floor: torch sum over the column ids", ms, lo, hi, bytes=col_bytes, GBps=round(col_bytes / ms / 1e6, 1))
    del src, dst

    # (b) the scan
    rng = np.random.default_rng(0)
    for T in (1, 16, 256):
        cols = rng.choice(V, T, replace=False)
        ms, lo, hi = median_ms(lambda: idx.term_bitmaps(cols), args.reps)
        passes = -(-T // nat.TERM_FILTER_SLOTS)
        report(f"term_bitmaps T={T}", ms, lo, hi, passes=passes, bytes=col_bytes * passes, GBps=round(col_bytes * passes / ms / 1e6, 1),
               x_floor=round(ms / passes / floor, 2))
    thr = {int(c): 0.5 for c in cols}
    ms, lo, hi = median_ms(lambda: idx.term_bitmaps(cols, thr=thr), args.reps)
    report("term_bitmaps T=256 with thresholds", ms, lo, hi, passes=2, x_floor=round(ms / 2 / floor, 2))
    for B in (1, 256):
        def lists(n):
            return [rng.choice(V, n, replace=False).tolist() for _ in range(B)] if B > 1 else rng.choice(V, n, replace=False).tolist()
        kw = dict(must=lists(2), must_not=lists(1), should=lists(5), min_should=2)
        ms, lo, hi = median_ms(lambda: DocFilter.from_terms(idx, **kw), max(args.reps // 4, 3))
        report(f"from_terms B={B} (2 must, 1 must_not, 2 of 5 should)", ms, lo, hi)

    # (c) before: the CSR to the host, then a torch mask on the same GPU
    if not args.no_baseline:
        try:
            t0 = time.perf_counter()
            ip, ix, _ = idx.export_csr()
            t_export = time.perf_counter() - t0
            t0 = time.perf_counter()
            col = int(cols[0])
            ixd = torch.from_numpy(ix).cuda()
            ipd = torch.from_numpy(ip).cuda()
            hit = (ixd == col).nonzero().flatten()
            mask = torch.zeros(args.rows, dtype=torch.bool, device="cuda")
            mask[torch.searchsorted(ipd, hit, right=True) - 1] = True
            torch.cuda.synchronize()
            t_mask = time.perf_counter() - t0
            got = DocFilter.from_terms(idx, must=[col])
            same = bool((DocFilter.from_mask(mask).words == got.words).all())
            report("before: export_csr to the host", t_export * 1e3, t_export * 1e3, t_export * 1e3, host_bytes=int(ix.nbytes + ip.nbytes) + int(ix.shape[0]) * 4)
            report("before: torch mask of ONE term from the exported CSR (upload + compare + scatter)", t_mask * 1e3, t_mask * 1e3, t_mask * 1e3, equal=same)
        except Exception as e:                       # noqa: BLE001  (reported, not hidden: the figure is "does not fit")
            print(json.dumps(dict(name="before: export_csr + torch mask", error=f"{type(e).__name__}: {e}")), flush=True)
    print("\n| what | median ms | min | max | notes |\n|---|---|---|---|---|")
    for r in rows:
        notes = ", ".join(f"{k}={v}" for k, v in r.items() if k not in ("name", "median_ms", "min_ms", "max_ms"))
        print(f"| {r['name']} | {r['median_ms']} | {r['min_ms']} | {r['max_ms']} | {notes} |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(dict(rows=args.rows, nnz=args.nnz, device=torch.cuda.get_device_name(0), results=rows), fh, indent=1)


if __name__ == "__main__":
    main()
