"""Cost of the numeric-field calls: python tools/probe_values.py [N ...] [--rounds 5] [--bins 64] [--k 10]

For each row count N (default: 1 M and the 21 015 324 rows of BASELINE) a float32 value column with 5 % missing rows, B in {1, 8} queries and
two kinds of sets -- selective (about 1 % of the rows, random) and full (every row) -- the raw entry points on device buffers against what a
caller writes in torch on the same GPU without them:
  range filter   vs_value_range_bitmaps            against  DocFilter.from_mask((v >= lo) & (v <= hi))        (ranges about 1 % wide / open)
  histogram      vs_value_histogram, `bins` bins   against  torch.bucketize + torch.bincount per query over the bool mask
  top-k          vs_value_topk, k                  against  torch.where(mask, v, -inf).topk(k)
  stats          vs_value_stats                    (no torch counterpart is timed)
Device events on torch's current stream around one call, five rounds after a warm-up, the variants alternating round by round.  Prints one
JSON line per (N, B, set) with the median, the minimum and the spread (max - min) of every variant, the bytes a kernel must move (B * N / 8
of bitmap plus 4 bytes per row of a non-empty span: every row here) with the rate that gives, and the verdict of the criterion of DESIGN.md
3.1h: parity iff median <= the baseline's median + its own spread + 5 % of its median."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import current_stream, value_range_bitmaps
from vsearch_amd.doc_filter import DocFilter


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def probe(N, B, kind, rounds, bins, k):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(N + B)
    v = torch.randn(N, device=dev, generator=g) * 20 + 1990
    v[torch.rand(N, device=dev, generator=g) < 0.05] = float("nan")
    mask = torch.rand((B, N), device=dev, generator=g) < 0.01 if kind == "selective" else torch.ones((B, N), dtype=torch.bool, device=dev)
    has, ninf = ~torch.isnan(v), torch.tensor(-float("inf"), device=dev)           # (kept by the caller: not timed)
    f = DocFilter.from_mask(mask)
    words, ld = f.words, f.ld
    edges = torch.linspace(1930, 2050, bins + 1, device=dev)
    if kind == "selective":                                                          # B ranges about 1 % of the rows wide
        lo = 1990 + torch.arange(B, device=dev, dtype=torch.float32)
        hi = lo + 0.5
    else:
        lo = torch.full((B,), -float("inf"), device=dev)
        hi = torch.full((B,), float("inf"), device=dev)
    lo_h, hi_h = lo.cpu().numpy(), hi.cpu().numpy()
    s = current_stream(0)
    L = nat.lib()
    o64 = [torch.empty(B, dtype=torch.int64, device=dev) for _ in range(4)]
    o32 = [torch.empty(B, dtype=torch.float32, device=dev) for _ in range(2)]
    counts = torch.empty((B, bins), dtype=torch.int64, device=dev)
    ids, vals = torch.empty((B, k), dtype=torch.int64, device=dev), torch.empty((B, k), dtype=torch.float32, device=dev)

    def ours_hist():
        nat.check(L.vs_value_histogram(_p(words), 0, ld, None, B, _p(v), nat.VAL_F32, N, _p(edges), bins + 1, 0, _p(counts), bins, _p(o64[0]), _p(o64[1]),
                                       _p(o64[2]), 0, s))

    def torch_hist():
        return torch.stack([torch.bincount(torch.bucketize(v[mask[b] & has], edges, right=True), minlength=bins + 2) for b in range(B)])

    def ours_topk():
        nat.check(L.vs_value_topk(_p(words), 0, ld, None, B, _p(v), nat.VAL_F32, N, k, 1, 0, 0, _p(ids), _p(vals), 0, s))

    def torch_topk():
        return torch.where(mask & has[None, :], v[None, :], ninf).topk(k)

    def ours_stats():
        nat.check(L.vs_value_stats(_p(words), 0, ld, None, B, _p(v), nat.VAL_F32, N, 0, _p(o64[0]), _p(o64[1]), _p(o32[0]), _p(o32[1]), _p(o64[3]), 0, s))

    variants = {"range_ours": lambda: value_range_bitmaps(v, lo_h, hi_h), "range_torch": lambda: DocFilter.from_mask((v >= lo[:, None]) & (v <= hi[:, None])),
                "hist_ours": ours_hist, "hist_torch": torch_hist, "topk_ours": ours_topk, "topk_torch": torch_topk, "stats_ours": ours_stats}
    # the two sides agree before anything is timed
    assert (value_range_bitmaps(v, lo_h, hi_h) == DocFilter.from_mask((v >= lo[:, None]) & (v <= hi[:, None])).words.reshape(B, -1)).all()
    ours_hist()
    th = torch_hist()
    assert (counts == th[:, 1:bins + 1]).all() and (o64[0] == th[:, 0]).all() and (o64[1] == th[:, bins + 1]).all()
    ours_topk()
    assert (vals == torch_topk().values).all() or kind == "selective"                # (a selective set may hold fewer than k rows: -inf against NaN)
    for fn in variants.values():                                                     # warm-up
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    must = B * N // 8 + 4 * N
    out = {"probe": "values", "rows": N, "B": B, "set": kind, "rounds": rounds, "bins": bins, "k": k, "bytes_min": must,
           "device": torch.cuda.get_device_name(0)}
    med = {name: float(np.median(t)) for name, t in times.items()}
    for name, t in times.items():
        rec = {"median_ms": round(med[name], 4), "min_ms": round(float(np.min(t)), 4), "spread_ms": round(float(np.max(t) - np.min(t)), 4)}
        if name.endswith("_ours"):
            rec["GBps"] = round(must / med[name] / 1e6, 1)
            base = name.replace("_ours", "_torch")
            if base in times:
                bound = med[base] + float(np.max(times[base]) - np.min(times[base])) + 0.05 * med[base]
                rec["ratio_to_torch"] = round(med[name] / med[base], 4)
                rec["parity"] = bool(med[name] <= bound)
        out[name] = rec
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000, 21_015_324])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    a = ap.parse_args()
    for n in a.sizes:
        for B in (1, 8):
            for kind in ("selective", "full"):
                probe(n, B, kind, a.rounds, a.bins, a.k)


if __name__ == "__main__":
    main()
