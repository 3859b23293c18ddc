"""The quad walk's prefetch of the next block (bp_quad.h, behind the walk's barrier) -- run on MI355X.

The prefetched dword is never read, so no result may depend on it: every case below is searched with the default prefetch (cooperative
where the XCD's workgroups share a block range, per wave elsewhere), with VS_BP_KNOB=1024 (per wave always) and VS_BP_KNOB=512 (none),
and all three must equal each other and the CSR scan bit for bit.  What the cases are for is the cooperative path's ADDRESS GUARD
(a lane asks for line L = rank + ranks x slot of the next block's main area only while b + 1 < b1 and L < 2 V): they are the smallest
shapes at which it could go wrong -- a main area of fewer lines than one wave has lanes, a short last block, a chunk range of two blocks
(one boundary a work item, so every range's last block is reached right behind a prefetching one), the conditions of the fallback to the per-wave prefetch, a filtered search (the
filter words are waited for before the prefetch is issued) and a tile without entries.

The library reads its knobs once, so each setting is one fresh process that runs all cases and leaves its results in a file; a fourth
process runs the default with VS_BP_TIMING=1, whose "quad walk" line on stderr ends in the prefetch that ran: coop, wave or none.

What these tests can and cannot see: a result that differs, a fault, and WHICH arm ran ("coop" = at least one workgroup took the
cooperative arm across at least one block boundary).  A wrong address that is still mapped changes no result, and the word does not
show that a range's last block issued nothing: that is the guard's `b + 1 < b1`, argued in the comment above the load in bp_quad.h."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the prefetch the default build must take there
CASES = {
    "a_main_area_below_one_wave": "coop",         # V = 40: 80 lines, 3 blocks + 5 rows, 16 tiles x 1 chunk: 2 workgroups an XCD
    "b_short_last_block": "coop",                 # V = 300, 6 blocks (the last: 37 rows), 8 tiles x 2 chunks
    "c_two_blocks_an_item": "coop",               # V = 29 523, 4 blocks in 2 chunks: one boundary a work item
    "d_items_below_workgroups": "wave",           # 8 queries on 40 blocks: one tile, a chunk count that does not divide the XCDs
    "d_eight_chunks": "coop",                     # 256 queries on 64 blocks in 8 chunks: 32 workgroups an XCD
    "e_shared_filter": "coop",                    # shape b, filtered
    "e_per_query_filter": "coop",
    "f_empty_tile": "coop",                       # shape b, the second tile's queries all zero: its table has no steps
}

WORKER = r"""
import sys
import numpy as np, torch
sys.path.insert(0, %(repo)r)
import oracle
from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex

out = {}

def run(name, idx, q, k, chunks, filt=None):
    print("CASE " + name, file=sys.stderr, flush=True)
    qd = torch.from_numpy(q).cuda()
    idx.set_option("blocked_postings", 1)
    idx.set_option("postings_walk", 4)
    idx.set_option("postings_head", 0)              # (columns this dense would become dense strips, which belong to the list walk)
    idx.set_option("postings_chunks", chunks)
    ids, sc = idx.search(qd, k, filter=filt)
    torch.cuda.synchronize()
    info = idx.info()
    assert info.last_path == 3 and info.postings_walk == 4, (name, info.last_path, info.postings_walk)
    out[name + "/ids"], out[name + "/scores"] = ids.cpu().numpy(), sc.cpu().numpy()
    print("CASE ref", file=sys.stderr, flush=True)
    idx.set_option("blocked_postings", 0)
    ids, sc = idx.search(qd, k, filter=filt)
    torch.cuda.synchronize()
    assert idx.info().last_path == 1, name
    out[name + "/ref_ids"], out[name + "/ref_scores"] = ids.cpu().numpy(), sc.cpu().numpy()

idx = DeviceIndex.synthetic(3, 0, 3 * 2048 + 5, 40, 8)
run("a_main_area_below_one_wave", idx, oracle.synth_queries(1, 128, 40, 20), 10, 1)

n_b = 5 * 2048 + 37
idx = DeviceIndex.synthetic(4, 0, n_b, 300, 64)
q = oracle.synth_queries(2, 64, 300, 150)
run("b_short_last_block", idx, q, 10, 2)
g = torch.Generator().manual_seed(5)
run("e_shared_filter", idx, q, 10, 2, (torch.rand(n_b, generator=g) < 0.5).cuda())
run("e_per_query_filter", idx, q, 10, 2, (torch.rand(64, n_b, generator=g) < 0.5).cuda())
q0 = q.copy()
q0[8:16] = 0.0
run("f_empty_tile", idx, q0, 10, 2)

idx = DeviceIndex.synthetic(5, 0, 4 * 2048, 29523, 768)
run("c_two_blocks_an_item", idx, oracle.synth_queries(3, 128), 100, 2)

idx = DeviceIndex.synthetic(6, 0, 40 * 2048, 29523, 256)
run("d_items_below_workgroups", idx, oracle.synth_queries(4, 8), 100, 0)
del idx
idx = DeviceIndex.synthetic(7, 0, 64 * 2048, 29523, 256)
run("d_eight_chunks", idx, oracle.synth_queries(5, 256), 100, 8)

np.savez(sys.argv[1], **out)
print("OK")
"""

MODES = {"default": {}, "per_wave": {"VS_BP_KNOB": "1024"}, "none": {"VS_BP_KNOB": "512"}, "default_clocked": {"VS_BP_TIMING": "1"}}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """mode -> (arrays of every case, stderr): one process a mode, one after the other."""
    d = tmp_path_factory.mktemp("quad_prefetch")
    res = {}
    for mode, env in MODES.items():
        path = str(d / (mode + ".npz"))
        base = {k: v for k, v in os.environ.items() if k not in ("VS_BP_KNOB", "VS_BP_TIMING", "VS_BP_PF_LINES", "VS_BP_CHUNKS")}
        r = subprocess.run([sys.executable, "-c", WORKER % {"repo": REPO}, path], capture_output=True, text=True, timeout=600, env=dict(base, **env))
        assert r.returncode == 0 and "OK" in r.stdout, (mode, r.stdout[-500:], r.stderr[-3000:])
        res[mode] = (dict(np.load(path)), r.stderr)
    return res


@pytest.mark.parametrize("case", list(CASES))
def test_results_do_not_depend_on_the_prefetch(runs, case):
    ref_ids, ref_sc = runs["default"][0][case + "/ref_ids"], runs["default"][0][case + "/ref_scores"]
    assert ref_ids.size > 0
    for mode, (arr, _) in runs.items():
        # (scores as bit patterns: -inf pads of a filtered search, and no -0.0 == 0.0)
        assert (arr[case + "/ref_ids"] == ref_ids).all() and (arr[case + "/ref_scores"].view(np.uint32) == ref_sc.view(np.uint32)).all(), mode
        assert (arr[case + "/ids"] == ref_ids).all(), f"{mode}: ids differ from the CSR scan"
        assert (arr[case + "/scores"].view(np.uint32) == ref_sc.view(np.uint32)).all(), f"{mode}: scores differ from the CSR scan"


@pytest.mark.parametrize("case", list(CASES))
def test_the_expected_prefetch_ran(runs, case):
    stderr = runs["default_clocked"][1]
    part = stderr.split("CASE " + case + "\n", 1)[1].split("CASE ", 1)[0]
    words = set(re.findall(r"quad walk, cycles per block and wave:.*; prefetch (\w+)", part))
    assert words == {CASES[case]}, (words, part[-1500:])
