"""Cost of boosted search: python tools/probe_boost.py [N ...] [--B 64] [--rounds 5] [--lib PATH --range-only]

For each corpus size N (default: a synthetic 1 M-doc x 768-nnz fp32 index) and B = 64 queries of bench.py's first batch, on ONE handle with
option blocked_postings = 0 (the exact scans never take the postings):
  (1) search_range(thr = -inf) at max_hits in {100, 512} on the tile scan and on the one-query scan (queries_per_pass = 1): the baseline;
      search_boosted with F = 1 and F = 4 float32 fields ("add", no floor) at the same four shapes.  Parity rule (fixed before
      the run): a boosted call is at parity if its median is within the baseline's own run-to-run spread plus 5 %.
  (2) --lib PATH --range-only: the same range-search shapes on another build of the library (the parent commit's), for "no regression of
      search_range itself"; run it in the same session on the same machine and compare the two JSON lines.
  (3) what a caller writes today: (a) set_scores + torch.topk(s + w * p) -- exact, needs a [B, N] block; (b) search(depth = 1024) + a torch
      rescore, with its recall of the exact boosted top 100 at weights that move about 10 %, 50 % and 90 % of the top 100.
Device events on torch's current stream around one call; the variants alternate round by round after a warm-up.  Prints one JSON line per N
with the median, the minimum and the spread (max - min) of every variant."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat

V, NNZ_DOC, NNZ_Q, INDEX_SEED, QUERY_SEED = 29523, 768, 776, 0, 1
SHAPES = ((100, 0), (512, 0), (100, 1), (512, 1))                                    # (max_hits, queries_per_pass option)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def with_qpp(idx, qpp, fn):
    def run():
        idx.set_queries_per_pass(qpp)
        try:
            return fn()
        finally:
            idx.set_queries_per_pass(0)
    return run


def moved_weight(idx, q, field, want):
    """a weight under which about `want` of the exact boosted top 100 are not in the plain top 100 (bisection over the weight)"""
    plain = idx.search(q, 100)[0]
    moved = lambda w: float((~(idx.search_boosted(q, [field], [w], max_hits=100).ids[:, :, None] == plain[:, None, :]).any(dim=2)).float().mean())
    lo, hi = 0.0, 1.0
    while moved(hi) < want and hi < 1e6:
        hi *= 4
    for _ in range(12):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if moved(mid) < want else (lo, mid)
    return hi, moved(hi)


def probe(N, B, rounds, range_only):
    from vsearch_amd.device_index import DeviceIndex
    dev = torch.device("cuda", 0)
    idx = DeviceIndex.synthetic(INDEX_SEED, 0, N, V, NNZ_DOC, 0, 0, nat.VS_F32, 0)
    idx.set_option("blocked_postings", 0)
    gen = DeviceIndex.synthetic(QUERY_SEED, 0, B, V, NNZ_Q, 0, 0, 0, 0)             # bench.py's first query batch
    ip, ix, d = gen.export_csr()
    gen.close()
    q = torch.zeros((B, V), dtype=torch.float32, device=dev)
    q[torch.from_numpy(np.repeat(np.arange(B), np.diff(ip))).to(dev), torch.from_numpy(ix).to(dev)] = torch.from_numpy(d).to(dev)
    lo = np.full(B, -np.inf, dtype=np.float32)
    g = torch.Generator(device=dev).manual_seed(7)
    fields = [torch.rand(N, device=dev, generator=g) * 10 for _ in range(4)]
    w1 = torch.full((B, 1), 0.05, device=dev)
    w4 = torch.tensor([[0.05, 0.25, -0.05, 0.01]], device=dev).repeat(B, 1).contiguous()

    variants = {}
    for mh, qpp in SHAPES:
        tag = f"h{mh}_{'one_query' if qpp else 'tiles'}"
        variants[f"range_{tag}"] = with_qpp(idx, qpp, lambda mh=mh: idx.search_range(q, lo, max_hits=mh))
        if not range_only:
            variants[f"boost_f1_{tag}"] = with_qpp(idx, qpp, lambda mh=mh: idx.search_boosted(q, fields[:1], w1, max_hits=mh))
            variants[f"boost_f4_{tag}"] = with_qpp(idx, qpp, lambda mh=mh: idx.search_boosted(q, fields, w4, max_hits=mh))
    extra = {}
    if not range_only:
        def today_exact():                                                           # (a) the [B, N] block of exact scores, then torch
            s = idx.set_scores(q)
            return torch.topk(s + 0.05 * fields[0][None, :], 100, dim=1)

        def today_window(w=0.05):                                                    # (b) a rescore window of 1024
            ids, sc = idx.search(q, 1024)
            top = torch.topk(sc + w * fields[0][ids], 100, dim=1)
            return torch.gather(ids, 1, top.indices)
        variants["today_set_scores_topk"] = today_exact
        variants["today_search1024_rescore"] = today_window
        exact = idx.search_boosted(q, fields[:1], w1, max_hits=100)
        # (fl32(S) + fl32(w * p) rounds twice where search_boosted rounds once: the two lists may differ at ties and last bits)
        extra["today_set_scores_topk_same_ids"] = round(float((today_exact().indices[:, :, None] == exact.ids[:, None, :]).any(dim=2).float().mean()), 4)
        for want in (0.1, 0.5, 0.9):
            w, got = moved_weight(idx, q, fields[0], want)
            ex = idx.search_boosted(q, fields[:1], [w], max_hits=100).ids
            win = today_window(w)
            recall = float((ex[:, :, None] == win[:, None, :]).any(dim=2).float().mean())
            extra[f"window1024_moved_{int(want * 100)}"] = {"weight": round(w, 5), "moved": round(got, 3), "recall_of_exact_top100": round(recall, 4)}
    for fn in variants.values():                                                     # warm-up
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    info = idx.info()
    out = {"probe": "boost", "lib": os.path.basename(nat.LIB_PATH), "docs": N, "B": B, "rounds": rounds, "bytes_per_pass": int(info.bytes_per_pass),
           "device": torch.cuda.get_device_name(0)}
    med = {name: float(np.median(t)) for name, t in times.items()}
    for name, t in times.items():
        rec = {"median_ms": round(med[name], 3), "min_ms": round(float(np.min(t)), 3), "spread_ms": round(float(np.max(t) - np.min(t)), 3)}
        if name.startswith("boost_"):
            base = "range_" + name.split("_", 2)[2]
            spread = float(np.max(times[base]) - np.min(times[base]))
            rec["ratio_to_range"] = round(med[name] / med[base], 4)
            rec["parity"] = bool(med[name] <= med[base] + spread + 0.05 * med[base])
        out[name] = rec
    out.update(extra)
    print(json.dumps(out), flush=True)
    idx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000])
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib", default=None, help="load this build of libvsearch_hip.so instead (a baseline build of another commit)")
    ap.add_argument("--range-only", action="store_true", help="only the range-search shapes (a build without vs_index_search_boosted)")
    a = ap.parse_args()
    if a.lib:
        nat.LIB_PATH = os.path.abspath(a.lib)
        if a.range_only:
            nat._SIGNATURES.pop("vs_index_search_boosted", None)
    for n in a.sizes:
        probe(n, a.B, a.rounds, a.range_only)


if __name__ == "__main__":
    main()
