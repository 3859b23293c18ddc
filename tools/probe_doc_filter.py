"""Cost of the document filter on the headline workload: python tools/probe_doc_filter.py [N] [B] [k] [rounds]

BASELINE.json's headline (21 015 324 synthetic docs x 768 nnz, fp32, B = 1024, k = 100): the unfiltered search against filtered ones --
an all-ones shared filter, 50 % and 1 % shared filters, per-query 50 % filters.  One process; every round times each variant once (device
events on torch's current stream around one search), the variants alternate round by round, after a warm-up.  Prints one JSON line:
median / min / max ms per variant and the median's overhead over the unfiltered search."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, current_stream
from vsearch_amd.doc_filter import DocFilter

N = int(sys.argv[1]) if len(sys.argv) > 1 else 21_015_324
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
K = int(sys.argv[3]) if len(sys.argv) > 3 else 100
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 7
V, NNZ_DOC, NNZ_Q, INDEX_SEED, QUERY_SEED = 29523, 768, 776, 0, 1


def main():
    dev = torch.device("cuda", 0)
    idx = DeviceIndex.synthetic(INDEX_SEED, 0, N, V, NNZ_DOC, 0, 0, nat.VS_F32, 0).prepare()
    gen = DeviceIndex.synthetic(QUERY_SEED, 0, B, V, NNZ_Q, 0, 0, 0, 0)             # bench.py's first query batch
    ip, ix, d = gen.export_csr()
    gen.close()
    q = torch.zeros((B, V), dtype=torch.float32, device=dev)
    q[torch.from_numpy(np.repeat(np.arange(B), np.diff(ip))).to(dev), torch.from_numpy(ix).to(dev)] = torch.from_numpy(d).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    variants = {
        "unfiltered": None,
        "all_ones": DocFilter.from_mask(torch.ones(N, dtype=torch.bool, device=dev)),
        "shared_50": DocFilter.from_mask(torch.rand(N, device=dev, generator=g) < 0.5),
        "shared_1": DocFilter.from_mask(torch.rand(N, device=dev, generator=g) < 0.01),
    }
    nw = (N + 31) // 32
    words = torch.empty((B, nw), dtype=torch.int32, device=dev)
    for b0 in range(0, B, 64):                                                   # (packed in slices of queries: the [B, N] mask would be 21 GB)
        m = (torch.rand((min(64, B - b0), N), device=dev, generator=g) < 0.5).to(torch.uint8)
        nat.check(nat.lib().vs_filter_pack(C.c_void_p(m.data_ptr()), int(m.shape[0]), N, N, C.c_void_p(words[b0].data_ptr()), nw, 0,
                                           current_stream(0)))
    variants["per_query_50"] = DocFilter(words, N)
    torch.cuda.synchronize()
    paths = {}
    for name, f in variants.items():                                             # warm-up, and the path each variant takes
        for _ in range(2):
            idx.search(q, K, filter=f)
        info = idx.info()
        paths[name] = (int(info.last_path), int(info.postings_walk), int(info.last_fallbacks))
    times = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, f in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            idx.search(q, K, filter=f)
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    base = float(np.median(times["unfiltered"]))
    out = {"probe": "doc_filter", "docs": N, "B": B, "k": K, "rounds": ROUNDS, "device": torch.cuda.get_device_name(0)}
    for name, t in times.items():
        med = float(np.median(t))
        out[name] = {"median_ms": round(med, 3), "min_ms": round(float(np.min(t)), 3), "max_ms": round(float(np.max(t)), 3),
                     "overhead": round(med / base - 1.0, 4), "path": paths[name][0], "walk": paths[name][1], "fallbacks": paths[name][2]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
