"""Cost of the per-label percentiles: python tools/probe_facet_quantiles.py [N ...] [--rounds 5] [--labels 12 256 4096] [--batches 2] [--density 0.01]
                                       [--fields uniform years] [--B 1 8] [--R 1 7] [--ours-only] [--lib PATH]

For each row count N (default: 1 M and the 21 015 324 rows of BASELINE), a field -- "uniform": float32 in [0, 1000) with 5 % missing rows;
"years": int32 in 1900..2029 with 5 % missing, every row in one bin at radix levels 0 and 1 --, B in {1, 8} queries, two kinds of sets --
selective (about 1 % of the rows, random) and full --, R in {1, 7} quantiles, L labels and two label layouts -- random, and runs (labels
ascending along the rows) -- vs_facet_value_quantiles on device buffers against two baselines on the same GPU:
  (a) today's composition: vs_label_bitmaps of 64 labels, ANDed with the B set bitmaps, vs_value_quantiles over the B x 64 sets -- once per
      batch of 64 labels.  At most `--batches` batches are timed; where L needs more, the time is scaled by ceil(L / 64) / batches and the
      record says "extrapolated": the batches do the same work.
  (b) what a caller writes in torch per query: gather labels and order keys under the mask, sort the composite (label << 32 | key) 64-bit
      key, index at the segment starts (a bincount's cumsum) plus the ranks.
Where B x L x R x 2048 counts pass the 2^27 rule of a call, the ranks are served in passes of min(16, 65536 // (B x L)), as the facade does
("rank_passes").  All sides must agree on every value before anything is timed.  Device events on torch's current stream around one call, `rounds` rounds after
a warm-up, the variants alternating round by round.  Prints one JSON line per shape with the median, the minimum and the spread (max - min:
the noise) of every variant, the plan of each level (regime, qt, tile_labels, label_tiles), the ratio of the baselines' medians to the call's,
and "loses_to": the baselines whose median is below the call's.  --lib PATH loads another build of the library (A/B runs of the regimes:
make EXTRA=-DVS_FQ_MAX_LABEL_TILES=0 / =65535)."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def probe(N, B, kind, L, layout, field, R, rounds, max_batches, density=0.01, ours_only=False):
    from vsearch_amd.device_index import _value_keys, current_stream, facet_value_quantile_plan, label_bitmaps
    from vsearch_amd.doc_filter import DocFilter
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(N + B + L)
    if field == "uniform":
        v = torch.rand(N, device=dev, generator=g) * 1000
        v[torch.rand(N, device=dev, generator=g) < 0.05] = float("nan")
        dt, tdt = nat.VAL_F32, torch.float32
    else:
        v = torch.randint(1900, 2030, (N,), device=dev, generator=g, dtype=torch.int32)
        v[torch.rand(N, device=dev, generator=g) < 0.05] = -(1 << 31)
        dt, tdt = nat.VAL_I32, torch.int32
    if layout == "random":
        labels = torch.randint(0, L, (N,), device=dev, generator=g, dtype=torch.int32)
    else:
        labels = (torch.arange(N, device=dev, dtype=torch.int64) * L // N).to(torch.int32)
    mask = torch.rand((B, N), device=dev, generator=g) < density if kind == "selective" else torch.ones((B, N), dtype=torch.bool, device=dev)
    keys = _value_keys(v)                                                            # (kept by the caller: not timed)
    comp = (labels.to(torch.int64) << 32) | keys
    has = keys != 0
    f = DocFilter.from_mask(mask)
    words = f.words.reshape(B, -1)
    ld = words.shape[1]
    q = torch.linspace(0.1, 0.9, R, dtype=torch.float64, device=dev) if R > 1 else torch.tensor([0.5], dtype=torch.float64, device=dev)
    s = current_stream(0)
    lib = nat.lib()
    i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
    cnt, mis, tot, oth = i64(B, L), i64(B, L), i64(B), i64(B)
    rp = max(1, min(16, 65536 // (B * L)))                                           # ranks a pass: B x L x ranks x 2048 counts <= 2^27, as the facade splits
    passes = [(j, min(R, j + rp)) for j in range(0, R, rp)]
    outs = [(q[j0:j1].contiguous(), torch.empty((B, L, j1 - j0), dtype=tdt, device=dev), i64(B, L, j1 - j0)) for j0, j1 in passes]

    def ours():
        for qj, vj, rj in outs:
            nat.check(lib.vs_facet_value_quantiles(_p(words), 0, ld, None, B, _p(labels), L, _p(v), dt, N, _p(qj), nat.QUANTILE_LOWER, None,
                                                   int(qj.shape[0]), 0, _p(vj), _p(rj), _p(cnt), _p(mis), _p(tot), _p(oth), 0, s))

    n_batches = -(-L // 64)
    timed_batches = min(n_batches, max_batches)
    scale = n_batches / timed_batches
    BQ = B * 64
    v64, r64, c64, m64 = torch.empty((BQ, R), dtype=tdt, device=dev), i64(BQ, R), i64(BQ), i64(BQ)

    def composed():
        for k in range(timed_batches):
            lb = label_bitmaps(labels, np.arange(64 * k, 64 * k + 64, dtype=np.int32))
            w = (words[:, None, :] & lb[None, :, :]).reshape(BQ, -1).contiguous()
            nat.check(lib.vs_value_quantiles(_p(w), 0, w.shape[1], None, BQ, _p(v), dt, N, _p(q), nat.QUANTILE_LOWER, None, R, 0, _p(v64), _p(r64),
                                             _p(c64), _p(m64), 0, s))

    def in_torch():
        out = []
        for b in range(B):
            c = comp[mask[b] & has].sort().values
            n = torch.bincount(c >> 32, minlength=L)
            start = n.cumsum(0) - n
            r = torch.floor(q[None, :] * (n.to(torch.float64) - 1.0)[:, None]).to(torch.int64)
            at = (start[:, None] + r).clamp(0, max(int(c.shape[0]) - 1, 0))
            k = c[at] & 0xFFFFFFFF if c.shape[0] else torch.zeros_like(at)
            out.append((torch.where(n[:, None] > 0, k, torch.zeros_like(k)), n))
        return out

    ours()
    tk = in_torch()
    ok = _value_keys(torch.cat([o[1] for o in outs], dim=2).reshape(-1)).reshape(B, L, R)
    assert all((ok[b] == tk[b][0]).all() and (cnt[b] == tk[b][1]).all() for b in range(B)), "the call and the torch expression differ"
    if not ours_only:
        composed()
        k0 = 64 * (timed_batches - 1)                                                # (the outputs hold the last batch timed)
        m = min(64, L - k0)
        assert (c64.view(B, 64)[:, :m] == cnt[:, k0:k0 + m]).all() and (_value_keys(v64.reshape(-1)).view(B, 64, R)[:, :m] == ok[:, k0:k0 + m]).all()
    variants = {"ours": ours} if ours_only else {"ours": ours, "composed": composed, "torch": in_torch}
    for fn in variants.values():                                                     # warm-up
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    out = {"probe": "facet_quantiles", "rows": N, "field": field, "B": B, "R": R, "set": kind, "labels": L, "layout": layout, "rounds": rounds,
           "plans": [list(facet_value_quantile_plan(N, B, L, passes[0][1], level, True)[:4]) for level in range(3)],     # (of the first rank pass)
           "rank_passes": len(passes), "composed_batches_timed": timed_batches, "composed_batches": n_batches, "extrapolated": bool(scale > 1)}
    med = {}
    for name, t in times.items():
        k = scale if name == "composed" else 1.0
        med[name] = float(np.median(t)) * k
        out[name] = {"median_ms": round(med[name], 4), "min_ms": round(float(np.min(t)) * k, 4), "spread_ms": round(float(np.max(t) - np.min(t)) * k, 4)}
    if not ours_only:
        out["ours"]["composed_over_ours"] = round(med["composed"] / med["ours"], 3)
        out["ours"]["torch_over_ours"] = round(med["torch"] / med["ours"], 3)
        out["ours"]["loses_to"] = [b for b in ("composed", "torch") if med[b] < med["ours"]]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000, 21_015_324])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--labels", nargs="*", type=int, default=[12, 256, 4096])
    ap.add_argument("--fields", nargs="*", default=["uniform", "years"])
    ap.add_argument("--sets", nargs="*", default=["selective", "full"])
    ap.add_argument("--layouts", nargs="*", default=["random", "runs"])
    ap.add_argument("--B", nargs="*", type=int, default=[1, 8])
    ap.add_argument("--R", nargs="*", type=int, default=[1, 7])
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--density", type=float, default=0.01, help="the share of the rows in a selective set")
    ap.add_argument("--ours-only", action="store_true", help="time the call alone (A/B runs of two builds)")
    ap.add_argument("--lib", default=None, help="another build of libvsearch_hip.so")
    a = ap.parse_args()
    if a.lib:
        nat.LIB_PATH = os.path.abspath(a.lib)
    for n in a.sizes:
        for field in a.fields:
            for B in a.B:
                for R in a.R:
                    for kind in a.sets:
                        for L in a.labels:
                            for layout in a.layouts:
                                probe(n, B, kind, L, layout, field, R, a.rounds, a.batches, a.density, a.ours_only)


if __name__ == "__main__":
    main()
