"""Cost and payoff of the reweighted index: python tools/probe_rescale.py [N] [--rounds 5] [--host-rounds 5] [--parts a b c] [--B 64] [--k 100]

On one MI355X, synthetic indexes of N rows (default 1 M) x 768 cells.  Medians of --rounds after a warm-up, device events around the calls (every
call here blocks, so the wall clock is printed next to them), and both sides compared for equality before anything is timed.
 (a) DeviceIndex.rescale (vs_index_rescale) in eight shapes -- fp32 -> fp32 with no scale, a row scale, a column scale, both; fp32 -> fp16;
     fp16 -> fp32; binary -> fp32 with column scales -- and row_stats, each with the fraction of the HBM time of the bytes it moves
     (6.29 TB/s, the measured copy rate), against
       - select_rows(arange(N)) of the same source on the same build, which moves the bytes of the fp32 -> fp32 shapes.  Parity iff the
         rescale's median is within the baseline's own max - min spread plus 5 % of its median (the rule of DESIGN.md 3.1h, fixed before
         the run);
       - "get_rows": get_rows into device arrays, a torch multiply, from_csr;
       - "host": export_csr, numpy, from_csr -- in the both-scales shape only, timed --host-rounds times and AFTER the GPU routes (timed first,
         the host route left outliers of 0.5 s in the calls behind it: tools/probe_select.py).
 (b) search (B queries, top k, after prepare()) on the fp16 result against the fp32 source.
 (c) search on the normalised index against the source.
Prints one JSON line per measurement."""
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

V, NNZ_DOC, NNZ_Q, INDEX_SEED, QUERY_SEED = 29523, 768, 776, 0, 1
CHUNK = 1 << 16              # rows of a block when two indexes are compared on the device
HBM_BYTES_PER_MS = 6.29e9    # the measured float4 copy rate of the MI355X
VALUE_BYTES = {nat.VS_F32: 4, nat.VS_F16: 2, nat.VS_NONE: 0}


def timed(fn):
    """-> (device ms between two events on the current stream, wall ms, the call's result)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, out


def stats(t):
    return {"median": round(float(np.median(t)), 3), "min": round(float(np.min(t)), 3), "max": round(float(np.max(t)), 3), "n": len(t)}


def measure(fn, rounds, close=True):
    """a warm-up, then `rounds` timed calls -> (event stats, wall stats); an index a call returns is closed"""
    ev, wall = [], []
    for i in range(rounds + 1):
        e, w, out = timed(fn)
        if close:
            for x in (out if isinstance(out, tuple) else (out,)):
                if isinstance(x, DeviceIndex):
                    x.close()
        if i:
            ev.append(e)
            wall.append(w)
    return stats(ev), stats(wall)


def same_index(a, b, dev):
    """row pointers, columns and value bits of two indexes, block by block on the device"""
    if a.n_rows != b.n_rows or a.info().n_packets != b.info().n_packets or a.info().nnz != b.info().nnz or a.info().store_dtype != b.info().store_dtype:
        return False
    for r0 in range(0, a.n_rows, CHUNK):
        ids = torch.arange(r0, min(a.n_rows, r0 + CHUNK), dtype=torch.int64, device=dev)
        x, y = a.get_rows(ids), b.get_rows(ids)
        if not all(torch.equal(p, q) for p, q in zip(x, y)):
            return False
    return True


def via_get_rows(idx, everything, rs, cs, store):
    """the device route without the feature: the rows as 32-bit CSR arrays, a torch multiply in float64 rounded once, from_csr"""
    ip, ix, d = idx.get_rows(everything)
    x = d.to(torch.float64)
    if rs is not None:
        x = x * torch.repeat_interleave(rs.to(torch.float64), ip[1:] - ip[:-1])
    if cs is not None:
        x = x * cs.to(torch.float64)[ix.to(torch.int64)]
    return DeviceIndex.from_csr(ip, ix, x.to(torch.float32), V, store_dtype=store)


def via_host(idx, rs, cs, store):
    ip, ix, d = idx.export_csr()
    x = d.astype(np.float64)
    if rs is not None:
        x *= np.repeat(rs.astype(np.float64), np.diff(ip))
    if cs is not None:
        x *= cs.astype(np.float64)[ix]
    return DeviceIndex.from_csr(ip, ix, x.astype(np.float32), V, store_dtype=store)


def queries(B, dev):
    gen = DeviceIndex.synthetic(QUERY_SEED, 0, B, V, NNZ_Q, 0, 0, 0, 0)             # bench.py's first query batch
    qp, qx, qd = gen.export_csr()
    gen.close()
    q = torch.zeros((B, V), dtype=torch.float32, device=dev)
    q[torch.from_numpy(np.repeat(np.arange(B), np.diff(qp))).to(dev), torch.from_numpy(qx).to(dev)] = torch.from_numpy(qd).to(dev)
    return q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("N", nargs="?", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=5)
    ap.add_argument("--parts", nargs="*", default=["a", "b", "c"])
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--k", type=int, default=100)
    a = ap.parse_args()
    N, dev = a.N, torch.device("cuda", 0)
    base = {"probe": "rescale", "docs": N, "cells": NNZ_DOC, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(0)
    rs_h, cs_h = (rng.random(N) + 0.5).astype(np.float32), (rng.random(V) + 0.5).astype(np.float32)
    rs, cs = torch.from_numpy(rs_h).to(dev), torch.from_numpy(cs_h).to(dev)
    everything = torch.arange(N, dtype=torch.int64, device=dev)
    F32, F16, BIN = nat.VS_F32, nat.VS_F16, nat.VS_NONE
    shapes = [("fp32 -> fp32, no scale", F32, F32, None, None), ("fp32 -> fp32, row scale", F32, F32, rs, None),
              ("fp32 -> fp32, column scale", F32, F32, None, cs), ("fp32 -> fp32, both scales", F32, F32, rs, cs),
              ("fp32 -> fp16, no scale", F32, F16, None, None), ("fp16 -> fp32, no scale", F16, F32, None, None),
              ("binary -> fp32, column scale", BIN, F32, None, cs)]

    if "a" in a.parts:
        for src_dtype in (F32, F16, BIN):
            idx = DeviceIndex.synthetic(INDEX_SEED, 0, N, V, NNZ_DOC, 0, 0, src_dtype, 0)
            info = idx.info()
            packets = int(info.n_packets)
            read_bytes = packets * (16 + 8 * VALUE_BYTES[src_dtype]) + 4 * (N + 1)
            base_ev = None
            if src_dtype == F32:                                               # the baseline that moves the same bytes, timed first
                base_ev, base_wall = measure(lambda: idx.select_rows(everything), a.rounds)
            for name, sd, od, r, c in shapes:
                if sd != src_dtype:
                    continue
                out = dict(base, part="a", shape=name, route=idx.rescale_plan(r, c, od)[2])
                new = idx.rescale(r, c, od)
                try:
                    other = via_get_rows(idx, everything, r, c, od)
                    out["equal_get_rows"] = same_index(new, other, dev)
                    other.close()
                    have_get_rows = True
                except (MemoryError, ValueError, NotImplementedError, RuntimeError) as e:
                    out["get_rows_ms"], have_get_rows = f"failed: {type(e).__name__}: {e}"[:200], False
                host = name == "fp32 -> fp32, both scales" and a.host_rounds > 0
                if host:
                    other = via_host(idx, rs_h, cs_h, od)
                    out["equal_host"] = same_index(new, other, dev)
                    other.close()
                new.close()
                out["rescale_ms"], out["rescale_wall_ms"] = measure(lambda: idx.rescale(r, c, od), a.rounds)
                moved = read_bytes + packets * (16 + 8 * VALUE_BYTES[od]) + 4 * (N + 1) + (4 * N if r is not None else 0)
                out["bytes_moved"], out["hbm_fraction"] = moved, round(moved / HBM_BYTES_PER_MS / out["rescale_ms"]["median"], 3)
                if base_ev is not None and od == F32:
                    allowed = (base_ev["max"] - base_ev["min"]) + 0.05 * base_ev["median"]
                    gap = out["rescale_ms"]["median"] - base_ev["median"]
                    out.update(select_all_ms=base_ev, allowed_gap_ms=round(allowed, 3), gap_ms=round(gap, 3), parity=bool(gap <= allowed))
                if have_get_rows:
                    out["get_rows_ms"], out["get_rows_wall_ms"] = measure(lambda: via_get_rows(idx, everything, r, c, od), a.rounds)
                if host:
                    out["host_ms"], out["host_wall_ms"] = measure(lambda: via_host(idx, rs_h, cs_h, od), a.host_rounds)
                print(json.dumps(out), flush=True)
            if src_dtype == F32:
                out = dict(base, part="a", shape="row_stats")
                out["row_stats_ms"], out["row_stats_wall_ms"] = measure(lambda: idx.row_stats(), a.rounds, close=False)
                out["bytes_moved"], out["hbm_fraction"] = read_bytes + 28 * N, round((read_bytes + 28 * N) / HBM_BYTES_PER_MS / out["row_stats_ms"]["median"], 3)
                print(json.dumps(out), flush=True)
            idx.close()

    if "b" in a.parts or "c" in a.parts:
        q = queries(a.B, dev)
        idx = DeviceIndex.synthetic(INDEX_SEED, 0, N, V, NNZ_DOC, 0, 0, F32, 0).prepare()
        src_ev, _ = measure(lambda: idx.search(q, a.k), a.rounds, close=False)
        if "b" in a.parts:
            half = idx.rescale(dtype="fp16").prepare()
            out = dict(base, part="b", what="search: the fp16 result against the fp32 source", B=a.B, k=a.k, source_ms=src_ev)
            out["fp16_ms"], _ = measure(lambda: half.search(q, a.k), a.rounds, close=False)
            out["source_path"], out["fp16_path"] = int(idx.info().last_path), int(half.info().last_path)
            print(json.dumps(out), flush=True)
            half.close()
        if "c" in a.parts:
            st = idx.row_stats()
            unit = idx.rescale((1.0 / torch.sqrt(st.sumsq)).to(torch.float32)).prepare()
            out = dict(base, part="c", what="search: the normalised index against the source", B=a.B, k=a.k, source_ms=src_ev)
            out["normalised_ms"], _ = measure(lambda: unit.search(q, a.k), a.rounds, close=False)
            out["source_path"], out["normalised_path"] = int(idx.info().last_path), int(unit.info().last_path)
            print(json.dumps(out), flush=True)
            unit.close()
        idx.close()


if __name__ == "__main__":
    main()
