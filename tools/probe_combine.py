"""Cost and payoff of the combined index: python tools/probe_combine.py [N] [--rounds 5] [--parts a b] [--B 64] [--k 100]

On one MI355X, synthetic indexes of N rows (default 1 M): A = 768 fp32 cells a row.  Medians of --rounds after a warm-up, device events around
the calls (every call here blocks, so the wall clock is printed next to them), and both sides compared for equality -- row pointers, columns,
value bits -- before anything is timed.  The GPU routes are timed before any host route (there is none here: the device route without the
feature is the baseline).
 (a) DeviceIndex.combine (vs_index_combine) of A with
       - "bot":  B = ~86 binary cells a row (the bag-of-token shape), weights 1 and 0.3;
       - "half": B = 768 fp32 cells a row sharing half of A's columns (A's rows with 384 cells replaced), weights 1 and 0.5;
     each with the bytes it moves over the measured copy rate (6.29 TB/s), against
       - "torch": what a caller writes today -- get_rows of both into device CSR, a torch sparse add (COO, float64, coalesce), from_csr;
       - select_rows(arange(N)) of A on the same build: it moves fewer bytes (one source, no union), a reference point and no parity claim.
     The comparison rule (fixed before the run): a loss iff the call's median exceeds the baseline's median by more than the
     baseline's own max - min spread plus 5 % of its median.
 (b) search (B queries, top k, after prepare()) on the combined index against Index.search_hybrid(method="raw", missing="score") over the
     two sources, and the share of the exact top k that search_hybrid(missing="zero") at its default depth finds.
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
from vsearch_amd import synth
from vsearch_amd.device_index import DeviceIndex

V, NNZ_DOC, NNZ_BOT, NNZ_Q, INDEX_SEED, BOT_SEED, HALF_SEED, QUERY_SEED = 29523, 768, 86, 776, 0, 3, 7, 1
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
        if close and isinstance(out, DeviceIndex):
            out.close()
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
        if not all(torch.equal(p.view(torch.int32) if p.is_floating_point() else p, q.view(torch.int32) if q.is_floating_point() else q) for p, q in zip(x, y)):
            return False
    return True


def via_torch(a, b, everything, wa, wb):
    """the device route without the feature: both indexes as CSR arrays, the weighted cells side by side as COO in float64, coalesce (equal
    coordinates are summed, zeros are kept), from_csr"""
    n = a.n_rows
    parts_r, parts_c, parts_v = [], [], []
    for idx, w in ((a, wa), (b, wb)):
        ip, ix, d = idx.get_rows(everything)
        parts_r.append(torch.repeat_interleave(torch.arange(n, device=ip.device), ip[1:] - ip[:-1]))
        parts_c.append(ix.to(torch.int64))
        parts_v.append(d.to(torch.float64) * float(np.float32(w)))
    coo = torch.sparse_coo_tensor(torch.stack([torch.cat(parts_r), torch.cat(parts_c)]), torch.cat(parts_v), size=(n, V)).coalesce()
    rows, cols = coo.indices()
    ip = torch.zeros(n + 1, dtype=torch.int64, device=rows.device)
    ip[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    return DeviceIndex.from_csr(ip, cols.to(torch.int32), coo.values().to(torch.float32), V, store_dtype=nat.VS_F32)


def half_shared(a, everything, dev):
    """A's rows with every second stored cell moved to another column: 768 cells a row, 384 of them on A's columns"""
    ip, ix, d = a.get_rows(everything)
    ix = ix.to(torch.int64)
    pos = torch.arange(ix.numel(), device=dev)
    moved = (pos & 1) == 1
    # an odd cell goes halfway to the next stored column (columns ascend inside a row): a column the row does not store, or the cell stays
    nxt = torch.roll(ix, -1)
    mid = (ix + nxt) // 2
    ok = moved & (nxt > ix + 1)
    ix = torch.where(ok, mid, ix)
    gen = torch.Generator(device=dev).manual_seed(HALF_SEED)
    vals = torch.rand(d.shape, generator=gen, device=dev, dtype=torch.float32) + 0.01
    return DeviceIndex.from_csr(ip, ix.to(torch.int32), vals, V, store_dtype=nat.VS_F32), float(ok.sum()) / max(1, ix.numel())


def queries(B, dev):
    gen = DeviceIndex.synthetic(QUERY_SEED, 0, B, V, NNZ_Q, 0, 0, 0, 0)             # bench.py's first query batch
    qp, qx, qd = gen.export_csr()
    gen.close()
    q = torch.zeros((B, V), dtype=torch.float32, device=dev)
    q[torch.from_numpy(np.repeat(np.arange(B), np.diff(qp))).to(dev), torch.from_numpy(qx).to(dev)] = torch.from_numpy(qd).to(dev)
    return q


def index_bytes(idx):
    info = idx.info()
    return int(info.n_packets) * (16 + 8 * VALUE_BYTES[int(info.store_dtype)]) + 4 * (int(info.n_rows) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("N", nargs="?", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", nargs="*", default=["a", "b"])
    ap.add_argument("--shapes", nargs="*", default=["bot", "half"])
    ap.add_argument("--no-torch", action="store_true", help="skip the torch baseline (it holds tens of GB at 1 M rows)")
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--k", type=int, default=100)
    a = ap.parse_args()
    N, dev = a.N, torch.device("cuda", 0)
    base = {"probe": "combine", "docs": N, "cells": NNZ_DOC, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    everything = torch.arange(N, dtype=torch.int64, device=dev)
    A = DeviceIndex.synthetic(INDEX_SEED, 0, N, V, NNZ_DOC, 0, 0, nat.VS_F32, 0)
    bot = DeviceIndex.synthetic(BOT_SEED, 0, N, V, NNZ_BOT, synth.KIND_BOT, 0, nat.VS_NONE, 0)

    if "a" in a.parts:
        sel_ev, sel_wall = measure(lambda: A.select_rows(everything), a.rounds)            # the reference point, timed first
        for shape in a.shapes:
            if shape == "bot":
                B_idx, wa, wb, shared = bot, 1.0, 0.3, None
            else:
                B_idx, shared = half_shared(A, everything, dev)
                wa, wb = 1.0, 0.5
            out = dict(base, part="a", shape=shape, cells_b=round(int(B_idx.info().nnz) / N, 1), plan=A.combine_plan(B_idx)._asdict())
            if shared is not None:
                out["moved_share_of_b"] = round(shared, 3)
            new = A.combine(B_idx, wa, wb)
            out["cells_out"] = round(int(new.info().nnz) / N, 1)
            have_torch = not a.no_torch
            if have_torch:
                try:
                    other = via_torch(A, B_idx, everything, wa, wb)
                    out["equal_torch"] = same_index(new, other, dev)
                    other.close()
                except (MemoryError, ValueError, NotImplementedError, RuntimeError) as e:
                    out["torch_ms"], have_torch = f"failed: {type(e).__name__}: {e}"[:200], False
            # the bytes that have to move: both sources read once, the result written once, the union counts written and read
            moved = index_bytes(A) + index_bytes(B_idx) + index_bytes(new) + 8 * N
            out["packets"] = {"a": int(A.info().n_packets), "b": int(B_idx.info().n_packets), "out": int(new.info().n_packets)}
            new.close()
            torch.cuda.empty_cache()               # what the torch route cached goes back to the device before the library's own allocations are timed
            out["combine_ms"], out["combine_wall_ms"] = measure(lambda: A.combine(B_idx, wa, wb), a.rounds)
            # (the kernels walk the sources' ids again for every pass -- count three times, fill four -- out of the caches or not: not in this figure)
            out["bytes_moved"], out["hbm_fraction"] = moved, round(moved / HBM_BYTES_PER_MS / out["combine_ms"]["median"], 3)
            out["select_all_ms"] = sel_ev
            out["times_select_all"] = round(out["combine_ms"]["median"] / sel_ev["median"], 2)
            if have_torch:
                t_ev, t_wall = measure(lambda: via_torch(A, B_idx, everything, wa, wb), a.rounds)
                allowed = (t_ev["max"] - t_ev["min"]) + 0.05 * t_ev["median"]
                gap = out["combine_ms"]["median"] - t_ev["median"]
                out.update(torch_ms=t_ev, torch_wall_ms=t_wall, allowed_gap_ms=round(allowed, 3), gap_ms=round(gap, 3), loss=bool(gap > allowed),
                           speedup=round(t_ev["median"] / out["combine_ms"]["median"], 1))
            print(json.dumps(out), flush=True)
            if B_idx is not bot:
                B_idx.close()

    if "b" in a.parts:
        from vsearch_amd.ir import BoTIndex, SparseIndex
        q = queries(a.B, dev)
        wa, wb = 1.0, 0.3
        new = A.combine(bot, wa, wb).prepare()
        out = dict(base, part="b", what="search on the combined index against search_hybrid over the two sources", B=a.B, k=a.k, weights=[wa, wb])
        ids, scores = new.search(q, a.k)
        out["combined_ms"], _ = measure(lambda: new.search(q, a.k), a.rounds, close=False)
        out["combined_path"] = int(new.info().last_path)
        sp, bt = SparseIndex(device="cuda:0", fp16=False), BoTIndex(device="cuda:0", fp16=False)
        sp.adopt_device_index(A)
        bt.adopt_device_index(bot)
        hybrid = lambda missing: sp.search_hybrid(q, [(bt, None)], a.k, method="raw", weights=[wa, wb], missing=missing)
        zero, full = hybrid("zero"), hybrid("score")
        found = lambda res: float(np.mean([len(np.intersect1d(res.ids[b].cpu().numpy(), ids[b].cpu().numpy())) / a.k for b in range(a.B)]))
        out["exact_top_k_found_by_missing_zero"], out["exact_top_k_found_by_missing_score"] = round(found(zero), 4), round(found(full), 4)
        out["hybrid_score_ms"], _ = measure(lambda: hybrid("score"), a.rounds, close=False)
        out["hybrid_zero_ms"], _ = measure(lambda: hybrid("zero"), a.rounds, close=False)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
