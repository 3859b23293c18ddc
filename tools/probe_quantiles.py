"""Cost of the percentile calls: python tools/probe_quantiles.py [N ...] [--rounds 5]

For each row count N (default: 1 M and the 21 015 324 rows of BASELINE), two fields -- float32 uniform in [0, 1) and int32 years 1900..2029
(every row in one bin at levels 0 and 1: three full passes, every LDS atomic on one bin), 5 % missing rows each -- B in {1, 8} queries, R in
{1, 7} quantiles and two kinds of sets -- selective (about 1 % of the rows, random) and full (every row) -- the raw vs_value_quantiles call on
device buffers (method nearest) against what a caller writes in torch on the same GPU without it:
  sort       per query  v[mask[b] & has].sort().values  indexed at the ranks
  kthvalue   per query and rank  torch.kthvalue(v[mask[b] & has], rank + 1)
The three agree on every value before anything is timed.  Device events on torch's current stream around one call (the torch variants end in
the same gather of R values), `rounds` rounds after a warm-up, the variants alternating round by round; every configuration draws fresh
inputs.  Prints one JSON line per configuration with the median, the minimum and the spread (max - min) of every variant, the bytes the three
passes must move (3 x (B * N / 8 of bitmap + 4 bytes a row of a non-empty span: every row here)) with the rate that gives, the ratios to the
torch variants, and the verdict of the criterion of DESIGN.md 3.1h: parity iff median <= the baseline's median + its spread + 5 % of it."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import current_stream
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


def probe(N, B, R, kind, field, rounds):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(N + 131 * B + 7 * R + (field == "years"))
    if field == "years":
        v = torch.randint(1900, 2030, (N,), device=dev, generator=g, dtype=torch.int32)
        v[torch.rand(N, device=dev, generator=g) < 0.05] = -0x80000000
        has, dt = v != -0x80000000, nat.VAL_I32
    else:
        v = torch.rand(N, device=dev, generator=g)
        v[torch.rand(N, device=dev, generator=g) < 0.05] = float("nan")
        has, dt = ~torch.isnan(v), nat.VAL_F32
    mask = torch.rand((B, N), device=dev, generator=g) < 0.01 if kind == "selective" else torch.ones((B, N), dtype=torch.bool, device=dev)
    f = DocFilter.from_mask(mask)
    words, ld = f.words, f.ld
    q = torch.linspace(0.05, 0.95, R, dtype=torch.float64, device=dev) if R > 1 else torch.tensor([0.5], dtype=torch.float64, device=dev)
    s, L = current_stream(0), nat.lib()
    vals = torch.empty((B, R), dtype=v.dtype, device=dev)
    ranks, count, missing = (torch.empty(shape, dtype=torch.int64, device=dev) for shape in ((B, R), (B,), (B,)))

    def ours():
        nat.check(L.vs_value_quantiles(_p(words), 0, ld, None, B, _p(v), dt, N, _p(q), nat.QUANTILE_NEAREST, None, R, 0, _p(vals), _p(ranks), _p(count),
                                       _p(missing), 0, s))

    ours()
    rk = ranks.clone()                                                               # (the ranks are given to the torch variants: not timed)
    assert (rk >= 0).all()

    def torch_sort():
        return torch.stack([v[mask[b] & has].sort().values[rk[b]] for b in range(B)])

    rk_host = rk.cpu().tolist()

    def torch_kth():
        out = []
        for b in range(B):
            x = v[mask[b] & has]
            out.append(torch.stack([torch.kthvalue(x, r + 1).values for r in rk_host[b]]))
        return torch.stack(out)

    variants = {"ours": ours, "torch_sort": torch_sort, "torch_kthvalue": torch_kth}
    assert (torch_sort() == vals).all() and (torch_kth() == vals).all()               # the three agree before anything is timed
    for fn in variants.values():                                                     # warm-up
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    must = 3 * (B * N // 8 + 4 * N)
    out = {"probe": "quantiles", "rows": N, "B": B, "R": R, "set": kind, "field": field, "rounds": rounds, "bytes_min": must,
           "device": torch.cuda.get_device_name(0)}
    med = {name: float(np.median(t)) for name, t in times.items()}
    for name, t in times.items():
        rec = {"median_ms": round(med[name], 4), "min_ms": round(float(np.min(t)), 4), "spread_ms": round(float(np.max(t) - np.min(t)), 4)}
        if name != "ours":
            bound = med[name] + float(np.max(t) - np.min(t)) + 0.05 * med[name]
            rec["ours_over_this"] = round(med["ours"] / med[name], 4)
            rec["ours_at_parity_or_faster"] = bool(med["ours"] <= bound)
        else:
            rec["GBps"] = round(must / med[name] / 1e6, 1)
        out[name] = rec
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000, 21_015_324])
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    nat.require_device()
    for n in a.sizes:
        for field in ("uniform", "years"):
            for kind in ("selective", "full"):
                for B in (1, 8):
                    for R in (1, 7):
                        probe(n, B, R, kind, field, a.rounds)


if __name__ == "__main__":
    main()
