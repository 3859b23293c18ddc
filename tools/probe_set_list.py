"""Cost of the set egress: python tools/probe_set_list.py [N ...] [--rounds 5]

For each row count N (default: 1 M and the 21 015 324 rows of BASELINE), three kinds of sets -- every row, 1 % of the rows at random, 1 % of the
rows in runs of 512 -- and B in {1, 8} queries, the raw calls on device buffers against what a caller writes in torch on the same GPU without
them:
  list    vs_set_ids, the whole list (in pages of 2^27 / B ids where B x count is more)  |  shifts over the words to a [B, N] bool, then
          nonzero per query
  page    vs_set_ids, 1024 ids at offset count / 2                                       |  the same unpack and nonzero, sliced
  sample  vs_set_sample, n in {32, 1024}                                                 |  torch.rand(N) under the unpacked mask into topk
                                                                                            per query; and torch.rand(N) through vs_value_topk
Both sides agree on every id before anything is timed: the lists and pages with each other; the sample with a restatement of the pinned hash
in torch int64 arithmetic and a sort by (h, id) -- the random baselines draw other numbers, so of them every id is checked to be a member.
Device events on torch's current stream around one call, `rounds` rounds after a warm-up, the sides alternating round by round.  Prints one
JSON line per configuration with the median, the minimum and the spread (max - min) of every side, the ratio, and the verdict of the criterion
of DESIGN.md 3.1h, fixed beforehand: parity iff ours' median <= the baseline's median + its spread + 5 % of it."""
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

GOLDEN = -0x61C8864680B583EB                                                          # 0x9E3779B97F4A7C15 as an int64


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _shr(z, k):
    """a logical right shift of int64 bit patterns"""
    return (z >> k) & ((1 << (64 - k)) - 1)


def _mix(z):
    z = z ^ _shr(z, 30)
    z = z * -0x40A7B892E31B1A47                                                       # 0xBF58476D1CE4E5B9
    z = z ^ _shr(z, 27)
    z = z * -0x6B2FB644ECCEEE15                                                       # 0x94D049BB133111EB
    return z ^ _shr(z, 31)


def torch_hash(seed, ids):
    """the pinned hash of vs_set_sample restated in torch: int64 arithmetic wraps modulo 2^64"""
    k = _mix(torch.tensor([seed], dtype=torch.int64, device=ids.device) + GOLDEN)
    return _shr(_mix(k ^ ((ids + 1) * GOLDEN)), 32)


def make_masks(N, B, kind, g, dev):
    if kind == "every":
        return torch.ones((B, N), dtype=torch.bool, device=dev)
    if kind == "random":
        return torch.rand((B, N), device=dev, generator=g) < 0.01
    blocks = (N + 511) // 512
    on = torch.rand((B, blocks), device=dev, generator=g) < 0.01
    return on.repeat_interleave(512, dim=1)[:, :N].contiguous()


def report(out, times, ours="ours"):
    med = {name: float(np.median(t)) for name, t in times.items()}
    for name, t in times.items():
        rec = {"median_ms": round(med[name], 4), "min_ms": round(float(np.min(t)), 4), "spread_ms": round(float(np.max(t) - np.min(t)), 4)}
        if name != ours:
            bound = med[name] + float(np.max(t) - np.min(t)) + 0.05 * med[name]
            rec["ours_over_this"] = round(med[ours] / med[name], 4)
            rec["ours_at_parity_or_faster"] = bool(med[ours] <= bound)
        out[name] = rec
    print(json.dumps(out), flush=True)


def run_sides(variants, rounds):
    for fn in variants.values():                                                     # warm-up
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    return times


def probe(N, B, kind, rounds):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(N + 131 * B + len(kind))
    mask = make_masks(N, B, kind, g, dev)
    f = DocFilter.from_mask(mask)
    words, ld = f.words, f.ld
    s, L = current_stream(0), nat.lib()
    counts = torch.empty(B, dtype=torch.int64, device=dev)
    nat.check(L.vs_set_count(_p(words), 0, ld, None, B, N, 0, _p(counts), 0, s))
    assert (counts == mask.sum(1)).all()
    top = int(counts.max())
    shifts = torch.arange(32, device=dev, dtype=torch.int32)
    base = {"probe": "set_list", "rows": N, "B": B, "set": kind, "count_max": top, "rounds": rounds, "device": torch.cuda.get_device_name(0)}

    def unpack():
        return ((words[:, :, None] >> shifts) & 1).to(torch.bool).reshape(B, -1)[:, :N]

    def torch_list():
        m = unpack()
        return [m[b].nonzero().squeeze(1) for b in range(B)]

    # ---- the whole list ------------------------------------------------------------------------------------------------------------------------
    page = max(1, min(top, nat.SET_MAX_OUT_IDS // B))
    ids = torch.empty((B, page), dtype=torch.int64, device=dev)
    offs = torch.zeros(B, dtype=torch.int64, device=dev)

    def ours_list(check=None):
        for o in range(0, top, page):
            offs.fill_(o)
            nat.check(L.vs_set_ids(_p(words), 0, ld, None, B, N, _p(offs), page, 0, 0, _p(ids), _p(counts), 0, s))
            if check is not None:
                for b in range(B):
                    want = check[b][o:o + page]
                    assert (ids[b, :want.shape[0]] == want).all() and (ids[b, want.shape[0]:] == -1).all()

    want = torch_list()
    ours_list(check=want)                                                            # both sides agree on every id
    report(dict(base, what="list", pages=-(-top // page)), run_sides({"ours": ours_list, "torch_unpack_nonzero": torch_list}, rounds))

    # ---- a page of 1024 ids at offset count / 2 -------------------------------------------------------------------------------------------------
    half = counts // 2
    pids = torch.empty((B, 1024), dtype=torch.int64, device=dev)

    def ours_page():
        nat.check(L.vs_set_ids(_p(words), 0, ld, None, B, N, _p(half), 1024, 0, 0, _p(pids), _p(counts), 0, s))

    half_host = half.tolist()

    def torch_page():
        return [x[o:o + 1024] for x, o in zip(torch_list(), half_host)]

    ours_page()
    for b, w in enumerate(torch_page()):
        assert (pids[b, :w.shape[0]] == w).all() and (pids[b, w.shape[0]:] == -1).all()
    del want
    report(dict(base, what="page"), run_sides({"ours": ours_page, "torch_unpack_nonzero_slice": torch_page}, rounds))

    # ---- a sample ----------------------------------------------------------------------------------------------------------------------------------
    seeds = torch.arange(7, 7 + B, dtype=torch.int64, device=dev)
    for n in (32, 1024):
        sids = torch.empty((B, n), dtype=torch.int64, device=dev)
        hs = torch.empty((B, n), dtype=torch.int32, device=dev)
        vids = torch.empty((1, n), dtype=torch.int64, device=dev)
        vvals = torch.empty((1, n), dtype=torch.float32, device=dev)

        def ours_sample():
            nat.check(L.vs_set_sample(_p(words), 0, ld, None, B, N, _p(seeds), n, 0, 0, _p(sids), _p(hs), _p(counts), 0, s))

        def torch_rand_topk():
            m = unpack()
            out = []
            for b in range(B):
                r = torch.rand(N, device=dev).masked_fill_(~m[b], 2.0)
                v, i = r.topk(min(n, N), largest=False)
                out.append(torch.where(v < 2.0, i, torch.full_like(i, -1)))
            return out

        def rand_value_topk():
            out = []
            for b in range(B):
                r = torch.rand(N, device=dev)
                nat.check(L.vs_value_topk(_p(words[b]), 0, 0, None, 1, _p(r), nat.VAL_F32, N, n, 0, 0, 0, _p(vids), _p(vvals), 0, s))
                out.append(vids.clone())
            return out

        ours_sample()
        m = unpack()
        for b in range(B):                                                           # ours against the hash restated in torch, id by id
            members = m[b].nonzero().squeeze(1)
            h = torch_hash(7 + b, members)
            order = h.argsort(stable=True)[:n]                                         # (the members ascend: ties go to the smaller id)
            k = int(order.shape[0])
            assert (sids[b, :k] == members[order]).all() and (sids[b, k:] == -1).all() and ((hs[b, :k].to(torch.int64) & 0xFFFFFFFF) == h[order]).all()
            for side in (torch_rand_topk()[b], rand_value_topk()[b].reshape(-1)):    # the random baselines: every id is a member
                real = side[side >= 0]
                assert int(real.shape[0]) == min(n, int(members.shape[0])) and m[b][real].all()
        del m
        report(dict(base, what="sample", n=n), run_sides({"ours": ours_sample, "torch_rand_topk": torch_rand_topk, "rand_vs_value_topk": rand_value_topk},
                                                         rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000, 21_015_324])
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    nat.require_device()
    for n in a.sizes:
        for kind in ("every", "random", "runs"):
            for B in (1, 8):
                probe(n, B, kind, a.rounds)


if __name__ == "__main__":
    main()
