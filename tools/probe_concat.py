"""Cost of the joined index: python tools/probe_concat.py [N] [--rounds 5] [--host-rounds 5] [--sources 2 8 256] [--host-sources 8] [--modes fp32 fp16 mixed]

On one MI355X, synthetic indexes of N rows (default 1 M) x 768 cells, cut into S equal row ranges that are joined again.  Medians of --rounds
after a warm-up, device events around the calls (every call here blocks, so the wall clock is printed next to them), and both sides compared
for equality before anything is timed.  Modes: all-fp32 -> fp32, all-fp16 -> fp16, and mixed -- fp32, fp16 and bag-of-token sources in turn
-> fp16.
 (a) DeviceIndex.concat (vs_index_concat) against select_rows(arange(N)) of the unsplit source of the result's store, which moves the same
     bytes.  Parity iff concat's median is within select's own max - min spread plus 5 % of select's median (the rule of DESIGN.md 3.1h, fixed
     before the run); judged for the same-dtype joins.
 (b) what a caller writes without it: get_rows of every source into device arrays, torch.cat, from_csr ("get_rows").  It takes seconds, so it
     is timed --host-rounds times for the source counts of --host-sources only, and after the GPU routes.
Every line carries the bytes the join reads and writes and the rate that makes of the median, and the 256-source line the ratio to the
2-source join -- the cost of the table search.  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat
from vsearch_amd import synth
from vsearch_amd.device_index import DeviceIndex

V, NNZ_DOC = 29523, 768
CHUNK = 1 << 16              # rows of a block when two indexes are compared on the device
VALUE_BYTES = {nat.VS_F32: 32, nat.VS_F16: 16, nat.VS_NONE: 0}


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


def measure(fn, rounds):
    """a warm-up, then `rounds` timed calls -> (event stats, wall stats); the index a call returns is closed"""
    ev, wall = [], []
    for i in range(rounds + 1):
        e, w, out = timed(fn)
        out.close()
        if i:
            ev.append(e)
            wall.append(w)
    return stats(ev), stats(wall)


def rows_equal(new, row0, src, dev, round_f16):
    """rows [row0, row0 + src.n_rows) of `new` against the rows of `src`, block by block on the device: row lengths, columns, and the values
    (src's rounded to float16 first where the result stores float16 and the source does not)"""
    for r0 in range(0, src.n_rows, CHUNK):
        n = min(src.n_rows, r0 + CHUNK) - r0
        x = new.get_rows(torch.arange(row0 + r0, row0 + r0 + n, dtype=torch.int64, device=dev))
        y = src.get_rows(torch.arange(r0, r0 + n, dtype=torch.int64, device=dev))
        vals = y[2].to(torch.float16).to(torch.float32) if round_f16 else y[2]
        if not (torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2], vals)):
            return False
    return True


def joined_equals(new, srcs, dev, out_dtype):
    if new.n_rows != sum(s.n_rows for s in srcs) or new.info().n_packets != sum(s.info().n_packets for s in srcs) or new.info().nnz != sum(s.info().nnz for s in srcs):
        return False
    row0 = 0
    for s in srcs:
        if not rows_equal(new, row0, s, dev, out_dtype == nat.VS_F16 and s.info().store_dtype == nat.VS_F32):
            return False
        row0 += s.n_rows
    return True


def via_get_rows(srcs, dev, out_dtype):
    """the caller's route: every source's rows into device arrays, one concatenation, one build"""
    parts = [s.get_rows(torch.arange(s.n_rows, dtype=torch.int64, device=dev)) for s in srcs]
    lengths = torch.cat([p[0][1:] - p[0][:-1] for p in parts])
    ip = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lengths, 0)])
    return DeviceIndex.from_csr(ip, torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]), V, store_dtype=out_dtype)


def cuts_of(n, s):
    return [n * i // s for i in range(s + 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("N", nargs="?", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=5)
    ap.add_argument("--sources", nargs="*", type=int, default=[2, 8, 256])
    ap.add_argument("--host-sources", nargs="*", type=int, default=[8])
    ap.add_argument("--modes", nargs="*", default=["fp32", "fp16", "mixed"])
    a = ap.parse_args()
    N, dev = a.N, torch.device("cuda", 0)
    base = {"probe": "concat", "docs": N, "cells": NNZ_DOC, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    whole = {nat.VS_F32: DeviceIndex.synthetic(0, 0, N, V, NNZ_DOC, 0, 0, nat.VS_F32, 0), nat.VS_F16: DeviceIndex.synthetic(0, 0, N, V, NNZ_DOC, 0, 0, nat.VS_F16, 0)}
    if "mixed" in a.modes:
        whole[nat.VS_NONE] = DeviceIndex.synthetic(3, 0, N, V, NNZ_DOC, synth.KIND_BOT, 0, nat.VS_NONE, 0)
    everything = torch.arange(N, dtype=torch.int64, device=dev)
    for mode in a.modes:
        out_dtype = nat.VS_F32 if mode == "fp32" else nat.VS_F16
        turn = {"fp32": [nat.VS_F32], "fp16": [nat.VS_F16], "mixed": [nat.VS_F32, nat.VS_F16, nat.VS_NONE]}[mode]
        # (a)'s baseline: the unsplit source of the result's store through select_rows -- the same bytes written, and for a same-dtype join read
        s_ev, s_wall = measure(lambda: whole[out_dtype].select_rows(everything), a.rounds)
        allowed = (s_ev["max"] - s_ev["min"]) + 0.05 * s_ev["median"]
        first = None
        for S in a.sources:
            cuts = cuts_of(N, S)
            srcs = [whole[turn[i % len(turn)]].slice_rows(cuts[i], cuts[i + 1] - cuts[i]) for i in range(S)]
            new = srcs[0].concat(srcs[1:], dtype=out_dtype)
            out = dict(base, mode=mode, sources=S, equal=joined_equals(new, srcs, dev, out_dtype))
            if mode != "mixed":
                out["equal_unsplit"] = rows_equal(new, 0, whole[out_dtype], dev, False)
            packets = int(new.info().n_packets)
            new.close()
            moved = sum(int(s.info().n_packets) * (16 + VALUE_BYTES[int(s.info().store_dtype)]) for s in srcs) + packets * (16 + VALUE_BYTES[out_dtype]) + 8 * N
            c_ev, c_wall = measure(lambda: srcs[0].concat(srcs[1:], dtype=out_dtype), a.rounds)
            out.update(concat_ms=c_ev, concat_wall_ms=c_wall, bytes_moved=moved, GBps=round(moved / c_ev["median"] / 1e6, 1), select_all_ms=s_ev,
                       select_all_wall_ms=s_wall, allowed_gap_ms=round(allowed, 3), gap_ms=round(c_ev["median"] - s_ev["median"], 3))
            if mode != "mixed":
                out["parity"] = bool(c_ev["median"] - s_ev["median"] <= allowed)
            if first is None:
                first = c_ev["median"]
            else:
                out["ratio_to_first_source_count"] = round(c_ev["median"] / first, 3)
            if S in a.host_sources and a.host_rounds > 0:
                try:
                    other = via_get_rows(srcs, dev, out_dtype)
                    out["equal_get_rows"] = joined_equals(other, srcs, dev, out_dtype)
                    other.close()
                    out["get_rows_ms"], out["get_rows_wall_ms"] = measure(lambda: via_get_rows(srcs, dev, out_dtype), a.host_rounds)
                    out["speedup_over_get_rows"] = round(out["get_rows_wall_ms"]["median"] / c_wall["median"], 1)
                except (MemoryError, ValueError, NotImplementedError, RuntimeError) as e:
                    out["get_rows_ms"] = f"failed: {type(e).__name__}: {e}"[:200]
            print(json.dumps(out), flush=True)
            for s in srcs:
                s.close()
    for w in whole.values():
        w.close()


if __name__ == "__main__":
    main()
