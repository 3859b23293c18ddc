"""Cost and payoff of index pruning: python tools/probe_prune.py [N ...] [--m 512 256 128] [--stores fp32 fp16] [--rounds 5] [--baseline-max N]
                                                                 [--baseline-m M ...] [--baseline-rounds 2]

For each corpus size N (default: synthetic 1 M and 21 015 324 docs x 768 cells), store and m, with and without a protect index (a synthetic
bag-of-token index of the same rows, 86 cells a row):
 (i)  DeviceIndex.prune (vs_index_prune, a blocking call: wall clock around it) against what a caller writes today -- export_csr to the host, a
      dense top-m in blocks of rows on the GPU in torch (plus the protect mask), from_csr -- in the same run, alternating, after the two outputs
      were compared for equality.  The baseline holds the CSR on the host (12 bytes a cell) and takes seconds: it runs only up to
      --baseline-max rows, for the m of --baseline-m, --baseline-rounds times (the run that is compared is one of them).  The call's time is also
      given as a share of the HBM time of the bytes its three steps move, computed from the shapes: the source's packets read twice (select,
      pack), a keep byte a source packet written and read, the kept packets written once.
 (ii) the payoff: search queries/s at B = 1024, k = 100 on the pruned index against the source (median, min, max of the repeats), the device
      bytes of both, and recall@100 of the pruned index's hits against the source's.  Recall on synthetic rows says little about a corpus.
Prints one JSON line per (N, store, m, protect)."""
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

V, NNZ_DOC, NNZ_BOT, NNZ_Q, INDEX_SEED, BOT_SEED, QUERY_SEED = 29523, 768, 86, 776, 0, 3, 1
HBM_PEAK_GBS = 8000.0        # bench.py's HBM_PEAK_GBS
STORES = {"fp32": nat.VS_F32, "fp16": nat.VS_F16}
BLOCK_ROWS = 4096            # rows of a dense block of the baseline: 4096 x 29523 fp32 = 484 MB


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(t):
    return {"median": round(float(np.median(t)), 3), "min": round(float(np.min(t)), 3), "max": round(float(np.max(t)), 3)}


def baseline(idx, m, store, protect_csr, dev):
    """what a caller writes today: the CSR to the host, a dense top-m per block of rows on the GPU, the kept cells back through from_csr"""
    ip, ix, d = idx.export_csr()
    n = len(ip) - 1
    keep = np.zeros(len(ix), dtype=bool)
    for r0 in range(0, n, BLOCK_ROWS):
        r1 = min(n, r0 + BLOCK_ROWS)
        a, b = int(ip[r0]), int(ip[r1])
        rows = torch.from_numpy(np.repeat(np.arange(r1 - r0), np.diff(ip[r0:r1 + 1]))).to(dev)
        cols = torch.from_numpy(ix[a:b]).to(dev)
        dense = torch.full((r1 - r0, V), float("-inf"), dtype=torch.float32, device=dev)
        dense[rows, cols] = torch.from_numpy(d[a:b]).to(dev)
        mask = torch.zeros((r1 - r0, V), dtype=torch.bool, device=dev)
        mask.scatter_(1, dense.topk(m, dim=1).indices, True)
        if protect_csr is not None:
            pip, pix = protect_csr
            pa, pb = int(pip[r0]), int(pip[r1])
            mask[torch.from_numpy(np.repeat(np.arange(r1 - r0), np.diff(pip[r0:r1 + 1]))).to(dev), torch.from_numpy(pix[pa:pb]).to(dev)] = True
        keep[a:b] = mask[rows, cols].cpu().numpy()
    kept = np.add.reduceat(keep, ip[:-1]) * (np.diff(ip) > 0) if len(ix) else np.zeros(n, dtype=np.int64)
    new_ip = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    return DeviceIndex.from_csr(new_ip, ix[keep], d[keep], V, store_dtype=store)


def probe(N, store_name, ms, rounds, baseline_max, baseline_ms, baseline_rounds, B, K):
    dev = torch.device("cuda", 0)
    store = STORES[store_name]
    idx = DeviceIndex.synthetic(INDEX_SEED, 0, N, V, NNZ_DOC, 0, 0, store, 0).prepare()
    bot = DeviceIndex.synthetic(BOT_SEED, 0, N, V, NNZ_BOT, synth.KIND_BOT, 0, nat.VS_NONE, 0)
    gen = DeviceIndex.synthetic(QUERY_SEED, 0, B, V, NNZ_Q, 0, 0, 0, 0)             # bench.py's first query batch
    qp, qx, qd = gen.export_csr()
    gen.close()
    q = torch.zeros((B, V), dtype=torch.float32, device=dev)
    q[torch.from_numpy(np.repeat(np.arange(B), np.diff(qp))).to(dev), torch.from_numpy(qx).to(dev)] = torch.from_numpy(qd).to(dev)
    info = idx.info()
    vb = 32 if store == nat.VS_F32 else 16
    for _ in range(2):
        idx.search(q, K)
    src_ids, _ = idx.search(q, K)
    src_ms = [timed(lambda: idx.search(q, K)) for _ in range(rounds)]
    src_aux = int(idx.info().aux_bytes)
    idx.set_option("blocked_postings", 0)              # the source's postings copy is released (as DeviceIndex.prune's retry does): at 21 M rows
    idx.set_option("blocked_postings", -1)             # the source's packets, its copy and the pruned index with its own copy do not fit one GPU
    protect_csr = bot.export_csr()[:2] if N <= baseline_max else None
    for m in ms:
        do_base = N <= baseline_max and m in baseline_ms
        for with_protect in (False, True):
            prot = bot if with_protect else None
            out = {"probe": "prune", "docs": N, "store": store_name, "m": m, "protect": with_protect, "rounds": rounds,
                   "device": torch.cuda.get_device_name(0)}
            new, kept = idx.prune(topk=m, protect=prot)                                # warm-up, and the output both sides are compared on
            ninfo = new.info()
            t_call, t_base = [], []
            if do_base:
                t, base = wall_ms(lambda: baseline(idx, m, store, protect_csr if with_protect else None, dev))
                t_base.append(t)
                a, b = new.export_csr(), base.export_csr()
                out["equal_output"] = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)))
                base.close()
                del a, b
            for i in range(rounds):                                                     # alternating
                t, x = wall_ms(lambda: idx.prune(topk=m, protect=prot))
                x[0].close()
                t_call.append(t)
                if do_base and i + 1 < baseline_rounds:
                    t, x = wall_ms(lambda: baseline(idx, m, store, protect_csr if with_protect else None, dev))
                    x.close()
                    t_base.append(t)
            moved = int(info.n_packets) * (2 * (16 + vb) + 2) + int(ninfo.n_packets) * (16 + vb) + 4 * N
            out["prune_ms"] = stats(t_call)
            out["baseline_ms"] = stats(t_base) if do_base else "not measured (the baseline holds the CSR on the host)"
            out["bytes_moved"] = moved
            out["hbm_ms"] = round(moved / HBM_PEAK_GBS / 1e6, 3)
            out["hbm_share_of_call"] = round(moved / HBM_PEAK_GBS / 1e6 / float(np.min(t_call)), 4)
            out["kept_mean"] = round(float(kept.mean()), 2)
            # (ii) the payoff
            new.prepare()
            for _ in range(2):
                new.search(q, K)
            ids, _ = new.search(q, K)
            new_ms = [timed(lambda: new.search(q, K)) for _ in range(rounds)]
            hit = (ids[:, :, None] == src_ids[:, None, :]).any(dim=2).float().mean().item()
            out["search_qps_source"] = stats([B / v * 1e3 for v in src_ms])
            out["search_qps_pruned"] = stats([B / v * 1e3 for v in new_ms])
            pinfo = new.info()
            out["pruned_search_path"] = int(pinfo.last_path)
            out["packet_bytes_source"], out["postings_bytes_source"] = int(info.device_bytes), src_aux
            out["packet_bytes_pruned"], out["postings_bytes_pruned"] = int(pinfo.device_bytes), int(pinfo.aux_bytes)
            out["recall_at_k_vs_source"] = round(hit, 4)
            print(json.dumps(out), flush=True)
            new.close()
    idx.close()
    bot.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000, 21_015_324])
    ap.add_argument("--m", nargs="*", type=int, default=[512, 256, 128])
    ap.add_argument("--stores", nargs="*", default=["fp32", "fp16"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--baseline-max", type=int, default=1_000_000, help="largest corpus the host-side baseline is run on")
    ap.add_argument("--baseline-m", nargs="*", type=int, default=None, help="the m the baseline is run for (default: every m)")
    ap.add_argument("--baseline-rounds", type=int, default=2)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    a = ap.parse_args()
    for n in a.sizes:
        for s in a.stores:
            probe(n, s, a.m, a.rounds, a.baseline_max, a.m if a.baseline_m is None else a.baseline_m, a.baseline_rounds, a.B, a.k)


if __name__ == "__main__":
    main()
