"""Cost of the breakdowns: python tools/probe_facet_values.py [N ...] [--rounds 5] [--bins 8] [--labels 12 256 2048 65536] [--batches 2] [--density 0.01] [--ours-only]

For each row count N (default: 1 M and the 21 015 324 rows of BASELINE) a float32 value column with 5 % missing rows, B in {1, 8} queries, two
kinds of sets -- selective (about 1 % of the rows, random) and full (every row) --, L labels and two label layouts -- random, and runs (labels
ascending along the rows: a compacted corpus, sorted clusters) -- the raw entry points on device buffers against two baselines on the same GPU:
  (a) today's composition: vs_label_bitmaps of 64 labels, ANDed with the B set bitmaps, vs_value_stats (vs_value_histogram) over the B x 64
      sets -- once per batch of 64 labels.  At most `--batches` batches are timed; where L needs more, the time is scaled by ceil(L / 64) /
      batches and the record says "extrapolated": the batches do the same work, and timing all 1024 of 65 536 labels would take minutes a round.
  (b) what a caller writes in torch over a [B, N] bool mask: bincount(labels[m], weights=v[m]) and scatter_reduce(amin / amax) for the stats,
      bucketize + a bincount of label x (bins + 2) + slot for the cross-tab, per query.
Device events on torch's current stream around one call, `rounds` rounds after a warm-up, the variants alternating round by round.  Prints one
JSON line per (N, B, set, L, layout) with the median, the minimum and the spread (max - min: the noise) of every variant and the ratio of the
baselines' medians to the call's; "loses_to" lists the baselines whose median is below the call's."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import current_stream, label_bitmaps
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


def probe(N, B, kind, L, layout, rounds, bins, max_batches, density=0.01, ours_only=False):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(N + B + L)
    v = torch.randn(N, device=dev, generator=g) * 20 + 1990
    v[torch.rand(N, device=dev, generator=g) < 0.05] = float("nan")
    if layout == "random":
        labels = torch.randint(0, L, (N,), device=dev, generator=g, dtype=torch.int32)
    else:
        labels = (torch.arange(N, device=dev, dtype=torch.int64) * L // N).to(torch.int32)
    mask = torch.rand((B, N), device=dev, generator=g) < density if kind == "selective" else torch.ones((B, N), dtype=torch.bool, device=dev)
    has = ~torch.isnan(v)                                                            # (kept by the caller: not timed)
    lab64 = labels.to(torch.int64)
    f = DocFilter.from_mask(mask)
    words = f.words.reshape(B, -1)
    ld = words.shape[1]
    edges = torch.linspace(1930, 2050, bins + 1, device=dev)
    E = bins + 1
    s = current_stream(0)
    lib = nat.lib()
    i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
    cnt, mis, sm, tot, oth = i64(B, L), i64(B, L), i64(B, L), i64(B), i64(B)
    lo, hi = torch.empty((B, L), device=dev), torch.empty((B, L), device=dev)
    hc, hb, ha, hm = i64(B, L, bins), i64(B, L), i64(B, L), i64(B, L)

    def stats_ours():
        nat.check(lib.vs_facet_value_stats(_p(words), 0, ld, None, B, _p(labels), L, _p(v), nat.VAL_F32, N, 0, _p(cnt), _p(mis), _p(lo), _p(hi), _p(sm), L,
                                           _p(tot), _p(oth), 0, s))

    def hist_ours():
        nat.check(lib.vs_facet_value_histogram(_p(words), 0, ld, None, B, _p(labels), L, _p(v), nat.VAL_F32, N, _p(edges), E, 0, _p(hc), bins, _p(hb),
                                               _p(ha), _p(hm), _p(tot), _p(oth), 0, s))

    n_batches = -(-L // 64)
    timed_batches = min(n_batches, max_batches)
    scale = n_batches / timed_batches
    BQ = B * 64
    c64, m64, s64 = i64(BQ), i64(BQ), i64(BQ)
    lo64, hi64 = torch.empty(BQ, device=dev), torch.empty(BQ, device=dev)
    h64, hb64, ha64 = i64(BQ, bins), i64(BQ), i64(BQ)

    def batch_sets(k):                                                               # from_labels of 64 labels & the B sets: B x 64 bitmaps
        lb = label_bitmaps(labels, np.arange(64 * k, 64 * k + 64, dtype=np.int32))
        return (words[:, None, :] & lb[None, :, :]).reshape(BQ, -1).contiguous()

    def stats_composed():
        for k in range(timed_batches):
            w = batch_sets(k)
            nat.check(lib.vs_value_stats(_p(w), 0, w.shape[1], None, BQ, _p(v), nat.VAL_F32, N, 0, _p(c64), _p(m64), _p(lo64), _p(hi64), _p(s64), 0, s))

    def hist_composed():
        for k in range(timed_batches):
            w = batch_sets(k)
            nat.check(lib.vs_value_histogram(_p(w), 0, w.shape[1], None, BQ, _p(v), nat.VAL_F32, N, _p(edges), E, 0, _p(h64), bins, _p(hb64), _p(ha64),
                                             _p(m64), 0, s))

    def stats_torch():
        out = []
        for b in range(B):
            m = mask[b] & has
            l, x = lab64[m], v[m]
            c = torch.bincount(l, minlength=L)
            t = torch.bincount(l, weights=x.double(), minlength=L)
            mn = torch.full((L,), float("inf"), device=dev).scatter_reduce(0, l, x, "amin")
            mx = torch.full((L,), -float("inf"), device=dev).scatter_reduce(0, l, x, "amax")
            out.append((c, torch.bincount(lab64[mask[b] & ~has], minlength=L), mn, mx, t))
        return out

    def hist_torch():
        out = []
        for b in range(B):
            m = mask[b] & has
            out.append(torch.bincount(lab64[m] * (bins + 2) + torch.bucketize(v[m], edges, right=True), minlength=L * (bins + 2)).view(L, bins + 2))
        return out

    variants = {"stats_ours": stats_ours, "stats_composed": stats_composed, "stats_torch": stats_torch, "hist_ours": hist_ours,
                "hist_composed": hist_composed, "hist_torch": hist_torch}
    # the sides agree before anything is timed
    stats_ours()
    st = stats_torch()
    assert all((cnt[b] == st[b][0]).all() and (mis[b] == st[b][1]).all() for b in range(B))
    assert all((lo[b][cnt[b] > 0] == st[b][2][cnt[b] > 0]).all() and (hi[b][cnt[b] > 0] == st[b][3][cnt[b] > 0]).all() for b in range(B))
    hist_ours()
    th = hist_torch()
    assert all((hc[b] == th[b][:, 1:bins + 1]).all() and (hb[b] == th[b][:, 0]).all() and (ha[b] == th[b][:, bins + 1]).all() for b in range(B))
    stats_composed()
    k0 = 64 * (timed_batches - 1)                                                    # (the outputs hold the last batch timed)
    assert (c64.view(B, 64)[:, :min(64, L - k0)] == cnt[:, k0:k0 + min(64, L - k0)]).all()
    if ours_only:                                                                    # (A/B runs of two builds of the library)
        variants = {k: fn for k, fn in variants.items() if k.endswith("_ours")}
    for fn in variants.values():                                                     # warm-up
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    out = {"probe": "facet_values", "rows": N, "B": B, "set": kind, "density": density if kind == "selective" else 1.0, "labels": L, "layout": layout, "rounds": rounds, "bins": bins,
           "composed_batches_timed": timed_batches, "composed_batches": n_batches, "extrapolated": bool(scale > 1),
           "device": torch.cuda.get_device_name(0)}
    med = {}
    for name, t in times.items():
        k = scale if name.endswith("_composed") else 1.0
        med[name] = float(np.median(t)) * k
        out[name] = {"median_ms": round(med[name], 4), "min_ms": round(float(np.min(t)) * k, 4), "spread_ms": round(float(np.max(t) - np.min(t)) * k, 4)}
    for call in () if ours_only else ("stats", "hist"):
        ours = med[call + "_ours"]
        out[call + "_ours"]["composed_over_ours"] = round(med[call + "_composed"] / ours, 3)
        out[call + "_ours"]["torch_over_ours"] = round(med[call + "_torch"] / ours, 3)
        out[call + "_ours"]["loses_to"] = [b for b in ("composed", "torch") if med[call + "_" + b] < ours]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000, 21_015_324])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bins", type=int, default=8)
    ap.add_argument("--labels", nargs="*", type=int, default=[12, 256, 2048, 65536])
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--density", type=float, default=0.01, help="the share of the rows in a selective set")
    ap.add_argument("--ours-only", action="store_true", help="time the two calls alone (A/B runs of two builds)")
    a = ap.parse_args()
    for n in a.sizes:
        for B in (1, 8):
            for kind in ("selective", "full"):
                for L in a.labels:
                    for layout in ("random", "runs"):
                        probe(n, B, kind, L, layout, a.rounds, a.bins, a.batches, a.density, a.ours_only)


if __name__ == "__main__":
    main()
