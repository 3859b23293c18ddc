"""Cost of list fusion: python tools/probe_fuse.py [--B 1024] [--L 2] [--kk 1000] [--k 100] [--rounds 20] [--warmup 3]

Reciprocal rank fusion of L hit lists of depth kk per query, about half of a list's documents shared with the next list, on device buffers:
vs_fuse_topk (one kernel) against the torch formulation of the same fusion -- concatenate the lists, sort every row by id, mark the first
entry of every id, scatter-add the contributions into one slot per id, topk.  Both produce the same fused values (checked); torch leaves the
order of ties to its sort.  Device events on torch's current stream around one call; the median of `rounds` calls after `warmup`, the two
variants alternating call by call.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd.device_index import fuse_topk


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def make_lists(B, L, kk, dev):
    """ids int64 / scores float32 [L, B, kk]: list l holds documents [l * kk / 2, l * kk / 2 + kk) of a per-query shuffle, in an order of its own"""
    g = torch.Generator(device=dev).manual_seed(0)
    n = kk + (L - 1) * (kk // 2)
    docs = torch.rand((B, n), generator=g, device=dev).argsort(dim=1) * 6661 + 13          # distinct ids in a row
    ids = torch.stack([docs[:, l * (kk // 2):l * (kk // 2) + kk][:, torch.randperm(kk, generator=g, device=dev)] for l in range(L)])
    scores = torch.rand((L, B, kk), generator=g, device=dev).sort(dim=2, descending=True).values
    return ids.contiguous(), scores.contiguous()


def torch_rrf(ids, k, c=60.0):
    """the same fusion with torch operators -> (ids [B, k], fused [B, k])"""
    L, B, kk = ids.shape
    cat = ids.permute(1, 0, 2).reshape(B, L * kk)
    contrib = (1.0 / (c + torch.arange(1, kk + 1, device=ids.device, dtype=torch.float32))).repeat(L).expand(B, L * kk)
    sorted_ids, perm = cat.sort(dim=1)
    head = torch.ones_like(sorted_ids, dtype=torch.bool)
    head[:, 1:] = sorted_ids[:, 1:] != sorted_ids[:, :-1]
    slot = head.cumsum(dim=1) - 1
    fused = torch.zeros((B, L * kk), dtype=torch.float32, device=ids.device).scatter_add_(1, slot, contrib.gather(1, perm))
    uid = torch.full((B, L * kk), -1, dtype=torch.int64, device=ids.device).scatter_(1, slot, sorted_ids)
    top = fused.masked_fill(uid < 0, float("-inf")).topk(k, dim=1)
    return uid.gather(1, top.indices), top.values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--L", type=int, default=2)
    ap.add_argument("--kk", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ids, scores = make_lists(a.B, a.L, a.kk, dev)
    out = tuple(torch.empty(shape, dtype=dt, device=dev) for shape, dt in
                (((a.B, a.k), torch.int64), ((a.B, a.k), torch.float32), ((a.B, a.k, a.L), torch.int32), ((a.B, a.k, a.L), torch.float32),
                 ((a.B,), torch.int32)))
    variants = {"vs_fuse_topk": lambda: fuse_topk(ids, scores, a.k, "rrf", out=out), "torch": lambda: torch_rrf(ids, a.k)}
    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    res, (t_ids, t_fused) = variants["vs_fuse_topk"](), variants["torch"]()
    torch.cuda.synchronize()
    same_values = bool(torch.equal(res.fused, t_fused))
    untied = torch.ones_like(t_fused, dtype=torch.bool)
    untied[:, 1:] &= t_fused[:, 1:] != t_fused[:, :-1]
    untied[:, :-1] &= t_fused[:, :-1] != t_fused[:, 1:]
    same_ids = bool((res.ids[untied] == t_ids[untied]).all())
    times = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    med = {name: float(np.median(t)) for name, t in times.items()}
    print(json.dumps({"probe": "fuse", "B": a.B, "L": a.L, "kk": a.kk, "k": a.k, "rounds": a.rounds, "warmup": a.warmup,
                      "union_mean": round(float(res.n.float().mean()), 1), "same_fused_values": same_values, "same_untied_ids": same_ids,
                      "vs_fuse_topk_ms": round(med["vs_fuse_topk"], 4), "vs_fuse_topk_min_ms": round(float(np.min(times["vs_fuse_topk"])), 4),
                      "torch_ms": round(med["torch"], 4), "torch_min_ms": round(float(np.min(times["torch"])), 4),
                      "torch_over_kernel": round(med["torch"] / med["vs_fuse_topk"], 2), "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
