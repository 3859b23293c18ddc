"""The quad walk's epilogue (bp_quad.h): ONE pass a block -- a thread harvests both of its documents (tid and tid + 1024), one test a
wave, pushes that find no room in a slot's 2048-key buffer stay pending in their thread until the buffer is cut -- run on MI355X.

Every case is compared BIT FOR BIT (ids and scores) with the CSR scan of the same index ("blocked_postings" = 0); the walk is forced
("postings_walk" = 4: the indexes are far too small for the quad policy's size gate) and sweeps all blocks of an index as ONE work item
a tile ("postings_chunks" = 1), so a candidate buffer lives across block boundaries.  The block size is SET ("postings_rows"; info()
does not report it): 2048, where a thread owns two documents of every full block, and 1920, the headline index's, where
k = 100 (128 keys kept by a cut) + a block's 1920 candidates fill a buffer exactly and k = 200 (250 kept) overflows it.

What the shapes are for:
 * row counts around the two-document ownership (1, 1023, 1024, 1025, rows - 1, rows, rows + 1, 2 rows + 1) with 1 - 8 queries: a tile
   with empty slots (threshold 0x7FFFFFFF), short last blocks, a block whose second halves are partly or wholly missing;
 * the ramp: scores strictly increasing with the row id over 3.x blocks, so EVERY document of every block beats the threshold -- from
   the second block on the pushes of a block do not fit behind the keys a cut kept and must go pending and come back;
 * ties: 600 documents with equal sums across a block boundary -- keys order by row;
 * filtered (the FL = 1 instantiation): a shared and a per-query filter, one that allows second-half documents (rows >= 1024 of a
   block) only;
 * one wave reading the counters late (VS_BP_KNOB = 128 + 4096 n, a fresh process each: the knob is read once);
 * an fp16-store index on the ramp."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 512


def _walk_and_scan(idx, q, k, rows, filt=None):
    """(ids, scores) of the quad walk and of the CSR scan, as numpy"""
    qd = torch.from_numpy(q).cuda()
    idx.set_option("postings_rows", rows)
    idx.set_option("postings_walk", 4)
    idx.set_option("postings_head", 0)
    idx.set_option("postings_chunks", 1)
    idx.set_option("blocked_postings", 1)
    ids, sc = idx.search(qd, k, filter=filt)
    info = idx.info()
    assert info.last_path == 3 and info.postings_walk == 4, (info.last_path, info.postings_walk)
    got = ids.cpu().numpy(), sc.cpu().numpy()
    idx.set_option("blocked_postings", 0)
    ids, sc = idx.search(qd, k, filter=filt)
    assert idx.info().last_path == 1
    return got, (ids.cpu().numpy(), sc.cpu().numpy())


def _assert_same(got, want, what):
    assert want[0].size > 0
    assert (got[0] == want[0]).all(), f"{what}: ids differ from the CSR scan ({int((got[0] != want[0]).sum())} places)"
    # (bit patterns: -inf pads of a filtered search, and no -0.0 == 0.0)
    assert (got[1].view(np.uint32) == want[1].view(np.uint32)).all(), f"{what}: scores differ from the CSR scan"


def _random_queries(seed, b, nnz=48):
    g = np.random.default_rng(seed)
    q = np.zeros((b, V), dtype=np.float32)
    for i in range(b):
        q[i, g.choice(V, nnz, replace=False)] = g.integers(1, 256, nnz).astype(np.float32) / 64.0
    return q


def ramp_csr(n, tie=None):
    """n documents x 8 non-zeros whose score for a query on columns 0 and 1 with EQUAL weights is w (i + 1) / 8192: strictly increasing
    with the row id, every value exact in fp16 (column 0: 1 + (i // 64) / 128, column 1: (i % 64 + 1) / 8192; n <= 8192).
    tie = (lo, hi): those rows hold 1.5 in column 0 and nothing in column 1 -- equal sums -- and every other row HALF its ramp value.
    Columns 8 .. V - 1: six more non-zeros a row that no ramp query asks for."""
    assert n <= 8192
    g = np.random.default_rng(7)
    i = np.arange(n)
    cols = np.empty((n, 8), dtype=np.int32)
    vals = np.empty((n, 8), dtype=np.float32)
    cols[:, 0], cols[:, 1] = 0, 1
    vals[:, 0] = 1.0 + (i // 64) / 128.0
    vals[:, 1] = (i % 64 + 1) / 8192.0
    if tie is not None:
        vals[:, :2] *= 0.5
        vals[tie[0]:tie[1], 0] = 1.5
        vals[tie[0]:tie[1], 1] = 0.0
    noise = 8 + np.argsort(g.random((n, V - 8)), axis=1)[:, :6]
    cols[:, 2:] = np.sort(noise, axis=1)
    vals[:, 2:] = g.integers(1, 256, (n, 6)) / 64.0
    return np.arange(0, 8 * n + 1, 8, dtype=np.int64), cols.reshape(-1), vals.reshape(-1)


def ramp_queries(b=8):
    q = np.zeros((b, V), dtype=np.float32)
    for j in range(b):
        q[j, 0] = q[j, 1] = 2.0 ** (j - 3)
    return q


_cache = {}


def ramp_index(rows, store=None):
    """3.x blocks of `rows` documents on the ramp (one index a block size and store: shared by the cases, never changed)"""
    key = (rows, store)
    if key not in _cache:
        n = 4 * rows - 7
        ip, ix, d = ramp_csr(n)
        _cache[key] = (DeviceIndex.from_csr(ip, ix, d, V, store_dtype=store), n)
    return _cache[key]


def random_index(n):
    if ("random", n) not in _cache:
        _cache[("random", n)] = DeviceIndex.synthetic(11, 0, n, V, 64)
    return _cache[("random", n)]


def _row_counts(rows):
    return [1, 1023, 1024, 1025, rows - 1, rows, rows + 1, 2 * rows + 1]


@pytest.mark.parametrize("rows", [2048, 1280])
@pytest.mark.parametrize("case", range(8))
def test_row_counts_around_the_two_document_ownership(rows, case):
    n = _row_counts(rows)[case]
    b = 1 + (case * 3 + 4) % 8                      # 5 8 3 6 1 4 7 2 queries: tiles with empty slots, and a full one
    got, want = _walk_and_scan(random_index(n), _random_queries(100 + case, b), min(10, n), rows)
    _assert_same(got, want, f"{n} rows in blocks of {rows}, {b} queries")


@pytest.mark.parametrize("rows", [1920, 2048])
@pytest.mark.parametrize("k", [200, 100])
def test_every_document_a_candidate_pending_pushes_come_back(rows, k):
    idx, n = ramp_index(rows)
    got, want = _walk_and_scan(idx, ramp_queries(), k, rows)
    _assert_same(got, want, f"ramp, blocks of {rows}, k = {k}")
    assert (got[0] == np.arange(n - 1, n - 1 - k, -1)[None, :]).all()          # the last k rows, best first


@pytest.mark.parametrize("k", [100, 700])
def test_ties_across_a_block_boundary_order_by_row(k):
    rows, n = 2048, 2 * 2048
    if "tie" not in _cache:
        ip, ix, d = ramp_csr(n, tie=(rows - 300, rows + 300))
        _cache["tie"] = DeviceIndex.from_csr(ip, ix, d, V)
    got, want = _walk_and_scan(_cache["tie"], ramp_queries(), k, rows)
    _assert_same(got, want, f"ties, k = {k}")
    m = min(k, 600)
    assert (got[0][:, :m] == np.arange(rows - 300, rows - 300 + m)[None, :]).all()      # equal scores: the lower row first


def _filters(n, b, rows, kind):
    g = torch.Generator().manual_seed(5)
    if kind == "shared":
        return (torch.rand(n, generator=g) < 0.5).cuda()
    if kind == "per_query":
        return (torch.rand(b, n, generator=g) < 0.5).cuda()
    return ((torch.arange(n) % rows) >= 1024).cuda()                      # second halves only: the documents tid + 1024


@pytest.mark.parametrize("kind", ["shared", "per_query", "second_half"])
@pytest.mark.parametrize("case", [3, 6, 7])
def test_filtered_row_counts(kind, case):
    rows = 2048
    n = _row_counts(rows)[case]
    b = 1 + (case * 3 + 4) % 8
    got, want = _walk_and_scan(random_index(n), _random_queries(100 + case, b), 10, rows, _filters(n, b, rows, kind))
    _assert_same(got, want, f"{kind} filter, {n} rows, {b} queries")


@pytest.mark.parametrize("kind", ["shared", "per_query", "second_half"])
@pytest.mark.parametrize("rows,k", [(1920, 200), (1920, 100), (2048, 200)])
def test_filtered_ramp(kind, rows, k):
    idx, n = ramp_index(rows)
    got, want = _walk_and_scan(idx, ramp_queries(), k, rows, _filters(n, 8, rows, kind))
    _assert_same(got, want, f"{kind} filter on the ramp, blocks of {rows}, k = {k}")


def test_fp16_store_on_the_ramp():
    idx, n = ramp_index(1920, nat.VS_F16)
    for k in (200, 100):
        got, want = _walk_and_scan(idx, ramp_queries(), k, 1920)
        _assert_same(got, want, f"fp16 store, k = {k}")
        assert (got[0] == np.arange(n - 1, n - 1 - k, -1)[None, :]).all()


LATE_WAVE = r"""
import sys
import numpy as np
sys.path.insert(0, %(repo)r)
sys.path.insert(0, %(tests)r)
import test_gpu_quad_epilogue as t
for rows, k in ((1920, 200), (1920, 100), (2048, 200)):
    idx, n = t.ramp_index(rows)
    got, want = t._walk_and_scan(idx, t.ramp_queries(), k, rows)
    t._assert_same(got, want, "late wave, blocks of %%d, k = %%d" %% (rows, k))
    assert (got[0] == np.arange(n - 1, n - 1 - k, -1)[None, :]).all()
print("OK")
"""


@pytest.mark.parametrize("n", [1, 4, 16])
def test_a_wave_that_reads_the_counters_late(n):
    """VS_BP_KNOB = 128 + 4096 n: wave 5 of every workgroup sleeps n x 512 cycles between the block's barrier and its read of the counters."""
    code = LATE_WAVE % {"repo": REPO, "tests": os.path.join(REPO, "tests")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, VS_BP_KNOB=str(128 + 4096 * n)))
    assert r.returncode == 0 and "OK" in r.stdout, (n, r.stdout[-500:], r.stderr[-2000:])
