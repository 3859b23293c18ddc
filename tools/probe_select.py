"""Cost and payoff of the sub-index: python tools/probe_select.py [N] [--rounds 5] [--host-rounds 5] [--parts a b c] [--B 64] [--k 100] [--labels 256]

On one MI355X, a synthetic fp32 index of N rows (default 1 M) x 768 cells.  Medians of --rounds after a warm-up, device events around the calls
(every call here blocks, so the wall clock is printed next to them), and both sides compared for equality before anything is timed.
 (a) DeviceIndex.select_rows (vs_index_select_rows) against what a caller writes without it: export_csr to the host, slicing there, from_csr
     ("host"); and get_rows with device ids and outputs, then from_csr ("get_rows").  Shapes: every row as a permutation, and 1 % of the rows
     ascending and random.  The host route moves the whole CSR (12 bytes a cell) over the host and takes seconds: it is timed --host-rounds
     times, and in every shape after the GPU routes (timed first, it left outliers of 0.5 s in the calls behind it).
 (b) select_rows(arange(N)) against compact() of the same source without tombstones: both move the same bytes.  Parity iff select's median is
     within compact's own max - min spread plus 5 % of compact's median (the rule of DESIGN.md 3.1h, fixed before the run).
 (c) the payoffs: search (B queries, top k) on the 1 % sub-index after prepare() against search(filter=) on the source; facet_value_stats and
     label_term_sums with --labels random labels on the source against the same calls on the source put into label order.
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd.device_index import DeviceIndex
from vsearch_amd.doc_filter import DocFilter

V, NNZ_DOC, NNZ_Q, INDEX_SEED, QUERY_SEED = 29523, 768, 776, 0, 1
CHUNK = 1 << 16              # rows of a block when two indexes are compared on the device


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
    if a.n_rows != b.n_rows or a.info().n_packets != b.info().n_packets or a.info().nnz != b.info().nnz:
        return False
    for r0 in range(0, a.n_rows, CHUNK):
        ids = torch.arange(r0, min(a.n_rows, r0 + CHUNK), dtype=torch.int64, device=dev)
        x, y = a.get_rows(ids), b.get_rows(ids)
        if not all(torch.equal(p, q) for p, q in zip(x, y)):
            return False
    return True


def via_host(idx, ids):
    ip, ix, d = idx.export_csr()
    lengths = ip[ids + 1] - ip[ids]
    new_ip = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    take = np.repeat(ip[ids] - new_ip[:-1], lengths) + np.arange(new_ip[-1], dtype=np.int64)
    return DeviceIndex.from_csr(new_ip, ix[take], d[take], V)


def via_get_rows(idx, ids_dev):
    ip, ix, d = idx.get_rows(ids_dev)
    return DeviceIndex.from_csr(ip, ix, d, V)


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
    ap.add_argument("--labels", type=int, default=256)
    a = ap.parse_args()
    N, dev = a.N, torch.device("cuda", 0)
    base = {"probe": "select", "docs": N, "cells": NNZ_DOC, "store": "fp32", "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    idx = DeviceIndex.synthetic(INDEX_SEED, 0, N, V, NNZ_DOC, 0, 0, 0, 0)
    rng = np.random.default_rng(0)
    one_pct = np.sort(rng.permutation(N)[:max(N // 100, 1)])
    shapes = {"permutation of every row": rng.permutation(N), "1 % ascending": one_pct, "1 % random": rng.permutation(one_pct)}

    if "a" in a.parts:
        for name, ids in shapes.items():
            ids_dev = torch.from_numpy(ids).to(dev)
            out = dict(base, part="a", shape=name, rows=len(ids))
            new = idx.select_rows(ids_dev)
            others = {}
            for route, fn in (("host", lambda: via_host(idx, ids)), ("get_rows", lambda: via_get_rows(idx, ids_dev))):
                try:
                    other = fn()
                    out[f"equal_{route}"] = same_index(new, other, dev)
                    other.close()
                    others[route] = fn
                except (MemoryError, ValueError, NotImplementedError, RuntimeError) as e:
                    out[f"{route}_ms"] = f"failed: {type(e).__name__}: {e}"[:200]
            new.close()
            # the GPU routes first, the host route (which moves the whole CSR through host memory every time) last
            out["select_device_ids_ms"], out["select_device_ids_wall_ms"] = measure(lambda: idx.select_rows(ids_dev), a.rounds)
            out["select_host_ids_ms"], out["select_host_ids_wall_ms"] = measure(lambda: idx.select_rows(ids), a.rounds)
            if "get_rows" in others:
                out["get_rows_ms"], out["get_rows_wall_ms"] = measure(others["get_rows"], a.rounds)
            if "host" in others and a.host_rounds > 0:
                out["host_ms"], out["host_wall_ms"] = measure(others["host"], a.host_rounds)
            print(json.dumps(out), flush=True)

    if "b" in a.parts:
        everything = torch.arange(N, dtype=torch.int64, device=dev)
        new, (packed, _) = idx.select_rows(everything), idx.compact()
        out = dict(base, part="b", equal=same_index(new, packed, dev))
        new.close()
        packed.close()
        c_ev, c_wall = measure(lambda: idx.compact(), a.rounds)
        s_ev, s_wall = measure(lambda: idx.select_rows(everything), a.rounds)
        allowed = (c_ev["max"] - c_ev["min"]) + 0.05 * c_ev["median"]
        out.update(compact_ms=c_ev, compact_wall_ms=c_wall, select_ms=s_ev, select_wall_ms=s_wall, allowed_gap_ms=round(allowed, 3),
                   gap_ms=round(s_ev["median"] - c_ev["median"], 3), parity=bool(s_ev["median"] - c_ev["median"] <= allowed))
        print(json.dumps(out), flush=True)

    if "c" in a.parts:
        q = queries(a.B, dev)
        idx.prepare()
        f = DocFilter.from_ids(one_pct, N)
        sub = idx.select_rows(one_pct).prepare()
        want_ids, want_sc = idx.search(q, a.k, filter=f)
        got_ids, got_sc = sub.search(q, a.k)
        ids_dev = torch.from_numpy(one_pct).to(dev)
        out = dict(base, part="c", what="search", B=a.B, k=a.k, rows=len(one_pct),
                   equal=bool(torch.equal(ids_dev[got_ids], want_ids) and torch.equal(got_sc, want_sc)))
        out["filtered_source_ms"], _ = measure(lambda: idx.search(q, a.k, filter=f), a.rounds, close=False)
        out["sub_index_ms"], _ = measure(lambda: sub.search(q, a.k), a.rounds, close=False)
        out["source_path"], out["sub_index_path"], out["sub_index_postings_bytes"] = int(idx.info().last_path), int(sub.info().last_path), int(sub.info().aux_bytes)
        print(json.dumps(out), flush=True)
        sub.close()

        labels = torch.from_numpy(rng.integers(0, a.labels, size=N).astype(np.int32)).to(dev)
        values = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).to(dev)
        order = torch.argsort(labels.to(torch.int64), stable=True)
        t_sort = measure(lambda: idx.select_rows(order), a.rounds)[0]
        srt = idx.select_rows(order).prepare()
        l2, v2 = labels[order].contiguous(), values[order].contiguous()
        x, y = idx.facet_value_stats(labels, a.labels, values), srt.facet_value_stats(l2, a.labels, v2)
        out = dict(base, part="c", what="facet_value_stats", labels=a.labels, sort_ms=t_sort,
                   equal=bool(all(torch.equal(p, r) for p, r in zip(x[:4], y[:4]))))      # counts, missing, min, max: exact in any order
        out["random_labels_ms"], _ = measure(lambda: idx.facet_value_stats(labels, a.labels, values), a.rounds, close=False)
        out["sorted_ms"], _ = measure(lambda: srt.facet_value_stats(l2, a.labels, v2), a.rounds, close=False)
        print(json.dumps(out), flush=True)
        x, y = idx.label_term_sums(labels, a.labels), srt.label_term_sums(l2, a.labels)
        out = dict(base, part="c", what="label_term_sums", labels=a.labels, equal=bool(all(torch.equal(p, r) for p, r in zip(x, y))))
        out["random_labels_ms"], _ = measure(lambda: idx.label_term_sums(labels, a.labels), a.rounds, close=False)
        out["sorted_ms"], _ = measure(lambda: srt.label_term_sums(l2, a.labels), a.rounds, close=False)
        print(json.dumps(out), flush=True)
        srt.close()
    idx.close()


if __name__ == "__main__":
    main()
