"""GPU tests of range search (vs_index_search_range; DeviceIndex / ShardGroup / Index .search_range / .count_matches / .match_filter,
Retriever.retrieve_range) -- run on MI355X.

The contract is tests/_range_ref.py.  Everything compares BITS -- ids, counts, bitmap words and scores.view(uint32): the
CSR kinds' numerics (fp32 products, one fp64 sum) do not depend on the order of the adds, so the numpy reference is exact on generic random
values; the dense matrix kind gets values m / 256 with small m, whose fp32 sums are exact in any order as well.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, RangeResults, ShardGroup
from vsearch_amd.doc_filter import DocFilter
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

import _range_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
VR = 2000                     # columns of the CSR cases
B_MAX = 9                     # a full tile of 8 queries plus one
ALL_HITS = (0, 1, 128, 129, 512, 513, 2048)
STORES = {"fp32": nat.VS_F32, "fp16": nat.VS_F16, "bin": nat.VS_NONE}


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


_cases = {}


def _case(n_rows, store="fp32", max_nnz=40):
    """-> (DeviceIndex, queries [B_MAX, VR], reference scores [B_MAX, n_rows]); built once, never changed by a test"""
    key = (n_rows, store, max_nnz)
    if key not in _cases:
        ip, ix, va = ref.csr_case(n_rows, VR, seed=n_rows + max_nnz, max_nnz=max_nnz)
        q = ref.sparse_queries(B_MAX, VR, seed=n_rows + 1)
        data = None if store == "bin" else (va.astype(np.float16) if store == "fp16" else va)
        dev = DeviceIndex.from_csr(ip, ix, data, VR, store_dtype=STORES[store])
        _cases[key] = (dev, q, ref.scores(q, ip, ix, va, store))
    return _cases[key]


def _call(dev, q, thr, max_hits, on_dev, flt=None, want_words=True, id_offset=0):
    """vs_index_search_range into junk-filled outputs, host or device buffers throughout -> dict of numpy arrays"""
    info = dev.info()
    n, B, K = int(info.n_rows), q.shape[0], max_hits
    W = (n + 31) // 32
    thr = ref.thresholds(thr, B)
    outs = dict(ids=np.full((B, K), 77, np.int64), scores=np.full((B, K), 1.5, F32), counts=np.full(B, -5, np.int64),
                words=np.full((B, W), 0xA5A5A5A5, np.uint32).view(np.int32))
    ins = dict(q=np.ascontiguousarray(q), thr=thr)
    fld = 0
    if flt is not None:
        ins["flt"] = _np(flt.words)
        fld = flt.ld
    if on_dev:
        outs = {k: torch.from_numpy(v).cuda() for k, v in outs.items()}
        ins = {k: torch.from_numpy(v).cuda() for k, v in ins.items()}
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
        torch.cuda.synchronize()
    else:
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
    dt = nat.VS_F16 if q.dtype == np.float16 else nat.VS_F32
    nat.check(nat.lib().vs_index_search_range(dev._h, ptr(ins["q"]), dt, q.shape[1], B, ptr(ins["thr"]), K, ptr(ins["flt"]) if flt is not None else None,
                                              0, fld, id_offset, ptr(outs["ids"]), ptr(outs["scores"]), ptr(outs["counts"]),
                                              ptr(outs["words"]) if want_words else None, W, None))
    return {k: _np(v) for k, v in outs.items()}


def _check(dev, q, S, thr, max_hits, allowed=None, flt=None, what=None):
    want = ref.search(S, thr, max_hits, allowed)
    for on_dev in (False, True):
        ref.assert_equal_bits(_call(dev, q, thr, max_hits, on_dev, flt), want, (what, max_hits, on_dev))
    return want


def _mid_thresholds(S, B, want_hits):
    """per-query thresholds that about `want_hits` rows pass (at least one, where the index has rows)"""
    n = S.shape[1]
    return np.array([np.sort(S[b])[::-1][min(n - 1, max(0, want_hits - 1 + 3 * b))] for b in range(B)], dtype=F32)


# ---- rows x batch x max_hits: every slot of junk-filled host and device buffers ------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 1000, 20000])
def test_equals_the_reference_across_rows_batches_and_hits(n_rows):
    dev, q, S = _case(n_rows)
    assert (S == 0).all(axis=0).any() or n_rows < 9                 # rows with no packets (every 9th) score +0.0 under every query
    if n_rows >= 1000:                                              # the long cases: every max_hits and every B, not every pair
        pairs = [(0, 1), (1, 9), (128, 8), (129, 1), (512, 9), (513, 9), (513, 8), (2048, 1)]
    else:
        pairs = [(mh, B) for mh in ALL_HITS for B in (1, 8, 9)]
    assert {mh for mh, _ in pairs} == set(ALL_HITS) and {B for _, B in pairs} == {1, 8, 9}
    for i, (max_hits, B) in enumerate(pairs):
        thr = _mid_thresholds(S, B, (5, 140, 600)[i % 3])
        want = _check(dev, q[:B], S[:B], thr, max_hits, what=(n_rows, B))
        assert (want["counts"] >= 1).all()
        info = dev.info()
        assert info.queries_per_pass == (8 if max_hits <= 512 else 1) and info.last_path == (1 if max_hits <= 512 else 0)
        if n_rows == 20000:
            # 20 000 rows: the plan the library took for this call has several chunks, and a ragged last one -- on the tile scan's one
            # tile (B <= 8) and two tiles (B = 9) and on the one-query scan's one query and nine (eight queries there may divide the rows evenly)
            nchunk, rpc = dev.last_range_plan()
            assert nchunk > 1 and (nchunk - 1) * rpc < n_rows <= nchunk * rpc, (max_hits, B, nchunk, rpc)
            assert n_rows % rpc != 0 or (max_hits, B) == (513, 8), (max_hits, B, nchunk, rpc)
    want = _check(dev, q, S, -np.inf, 16, what="all rows")          # every row matches; the list is the top 16
    assert (want["counts"] == n_rows).all()
    got = _call(dev, q, 0.25, 3, on_dev=False, want_words=False)    # no bitmap asked for: the junk stays
    assert (got["words"].view(np.uint32) == 0xA5A5A5A5).all()
    ref.assert_equal_bits(got, ref.search(S, 0.25, 3), "no words", ("ids", "scores", "counts"))


# ---- thresholds -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qpp", [0, 1])
def test_thresholds(qpp):
    dev, q, S = _case(1000)
    n = 1000
    dev.set_queries_per_pass(qpp)
    try:
        B = 8
        qs, Ss = q[:B], S[:B]
        empty = np.flatnonzero((Ss == 0).all(axis=0))
        assert empty.size > 50                                      # rows with no packets score +0.0 under every query
        want = _check(dev, qs, Ss, -np.inf, 129, what="-inf")
        assert (want["counts"] == n).all() and (want["words"][:, -1] == (1 << (n & 31)) - 1).all()
        want = _check(dev, qs, Ss, np.inf, 129, what="+inf")
        assert (want["counts"] == 0).all() and (want["ids"] == -1).all() and np.isneginf(want["scores"]).all()
        for zero in (0.0, -0.0):                                    # thr = 0: the empty rows match, the negative rows do not
            want = _check(dev, qs, Ss, zero, 2048, what="zero")
            assert (want["counts"] < n).all() and np.isin(empty, want["ids"][0]).all()
        tie, shared = ref.tie_threshold(Ss, 2)                      # exactly a score several rows share: >= keeps them all, ids ascending
        assert shared >= 2
        want = _check(dev, qs, Ss, tie, 2048, what="tie")
        last = want["ids"][2, want["counts"][2] - shared:want["counts"][2]]
        assert (Ss[2, last] == tie).all() and (np.diff(last) > 0).all()
        half, above = ref.halfway(Ss, 4, 30)                        # halfway between two adjacent scores
        want = _check(dev, qs, Ss, half, 513, what="halfway")
        assert want["counts"][4] == above
        per_q = np.array([-np.inf, np.inf, 0.0, tie, half, 1.0, -1.0, Ss[7].max()], dtype=F32)
        want = _check(dev, qs, Ss, per_q, 128, what="per query")
        assert want["counts"][0] == n and want["counts"][1] == 0 and want["counts"][7] >= 1
        assert dev.info().queries_per_pass == (8 if qpp == 0 else 1)
        # a NaN threshold: VS_EINVAL for a host array; on the device it matches no row (the other queries are served)
        nan_q = per_q.copy()
        nan_q[3] = np.nan
        with pytest.raises(ValueError, match="NaN"):
            _call(dev, qs, nan_q, 5, on_dev=False)
        got = _call(dev, qs, nan_q, 5, on_dev=True)
        want = ref.search(Ss, nan_q, 5)
        assert want["counts"][3] == 0 and (want["words"][3] == 0).all()
        ref.assert_equal_bits(got, want, "NaN on the device")
    finally:
        dev.set_queries_per_pass(0)


def test_tile_scan_and_one_query_scan_agree_at_512():
    dev, q, S = _case(20000)
    thr = _mid_thresholds(S, B_MAX, 700)                            # more matches than max_hits: the lists are cut
    got = {}
    for qpp in (0, 1):
        dev.set_queries_per_pass(qpp)
        try:
            got[qpp] = _call(dev, q, thr, 512, on_dev=True)
            assert dev.info().queries_per_pass == (8 if qpp == 0 else 1)
        finally:
            dev.set_queries_per_pass(0)
    ref.assert_equal_bits(got[0], got[1], "tile == one query")
    want = ref.search(S, thr, 512)
    assert (want["counts"] > 512).all()
    ref.assert_equal_bits(got[0], want, "512")
    ref.assert_equal_bits(_call(dev, q, thr, 513, on_dev=True), ref.search(S, thr, 513), "513")       # across the threshold between the scans
    assert dev.info().queries_per_pass == 1


# ---- overflow: more matches in a chunk than the candidate buffers hold, so the prune runs with the floor active --------------------------------
def test_overflow_with_pruning():
    n, B = 20000, 128
    ip, ix, va = ref.csr_case(n, VR, seed=3, max_nnz=12)
    q = ref.sparse_queries(B, VR, seed=4, nnz=24)
    S = ref.scores(q, ip, ix, va)
    dev = DeviceIndex.from_csr(ip, ix, va, VR)
    want = ref.search(S, -np.inf, 16)
    assert (want["counts"] == n).all()                              # every row passes the floor ...
    for qpp in (0, 1):
        dev.set_queries_per_pass(qpp)
        got = _call(dev, q, -np.inf, 16, on_dev=True)
        assert dev.info().queries_per_pass == (8 if qpp == 0 else 1)
        # ... and the chunks of the plan this call took overfill the scan's buffer: a prune happens with the floor active
        assert dev.last_range_plan()[1] > (2 * ref.K_MQ_SUPER if qpp == 0 else ref.K_WG_CAP), (qpp, dev.last_range_plan())
        ref.assert_equal_bits(got, want, ("overflow", qpp))
    dev.set_queries_per_pass(0)
    thr = _mid_thresholds(S, B, 5000)                               # a finite floor with thousands above it
    want = ref.search(S, thr, 16)
    assert (want["counts"] > ref.K_WG_CAP).all()
    ref.assert_equal_bits(_call(dev, q, thr, 16, on_dev=True), want, "finite floor")
    ref.assert_equal_bits(_call(dev, q, thr, 0, on_dev=True), ref.search(S, thr, 0), "count only")
    dev.close()


# ---- stores -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["fp16", "bin"])
def test_fp16_and_binary_stores(store):
    dev, q, S = _case(1000, store)
    for qpp in (0, 1):
        dev.set_queries_per_pass(qpp)
        try:
            thr = _mid_thresholds(S, B_MAX, 60)
            want = _check(dev, q, S, thr, 129, what=(store, qpp))
            assert (want["counts"] >= 60).all()
            if store == "bin":                                      # integer scores: ties everywhere, the id order decides inside them
                assert (np.diff(want["ids"][0, :want["counts"][0]][want["scores"][0, :want["counts"][0]] == want["scores"][0, 0]]) > 0).all()
            if store == "fp16":                                     # fp16 queries are widened, fp32 ones rounded to the index dtype
                got = _call(dev, q.astype(np.float16), thr, 129, on_dev=True)
                ref.assert_equal_bits(got, want, "fp16 queries")
        finally:
            dev.set_queries_per_pass(0)


def test_long_rows_take_the_wider_lane_groups():
    dev, q, S = _case(1000, "fp32", max_nnz=700)
    assert dev.info().lanes_per_row >= 16
    for max_hits in (64, 600):
        want = _check(dev, q, S, _mid_thresholds(S, B_MAX, 100), max_hits, what="long rows")
        assert (want["counts"] >= 100).all()


def test_dense_matrix_index_and_dense_stored_as_packets():
    n, V, B = 1500, 96, 9
    mat, q = ref.dense_case(n, V, B, seed=2)
    S = ref.scores(q, *ref.dense_to_csr(mat))
    assert (S == (q.astype(np.float64) @ mat.astype(np.float64).T).astype(F32)).all()                  # sums of m / 65536: exact in fp32 and fp64 alike
    dense = DeviceIndex.from_dense(mat)
    packets = DeviceIndex.from_dense(mat, max_density=0.9)
    assert dense.info().kind == nat.VS_KIND_DENSE and dense.info().n_packets == 0 and packets.info().n_packets > 0
    allowed = np.random.default_rng(1).random((B, n)) < 0.6
    flt = DocFilter.from_mask(torch.from_numpy(allowed))
    for dev in (dense, packets):
        for max_hits in (0, 1, 129, 2048):
            for thr in (-np.inf, np.inf, ref.tie_threshold(S, 1)[0], _mid_thresholds(S, B, 40)):
                _check(dev, q, S, thr, max_hits, what="dense")
        want = _check(dev, q, S, _mid_thresholds(S, B, 300), 129, allowed, flt, what="dense, filtered")
        assert (want["counts"] > 129).all()
        dev.delete_rows(np.arange(0, n, 3))
        live = np.ones(n, dtype=bool)
        live[::3] = False
        _check(dev, q, S, _mid_thresholds(S, B, 300), 513, allowed & live, flt, what="dense, filtered, deleted")
        want = _check(dev, q, S, -np.inf, 5, live, what="dense, deleted")
        assert (want["counts"] == live.sum()).all()
        dev.close()


def test_a_csr_index_wider_than_the_query_image_is_unsupported():
    V = 40000
    ip, ix, va = ref.csr_case(64, V, seed=1)
    dev = DeviceIndex.from_csr(ip, ix, va, V)
    with pytest.raises(NotImplementedError, match="too wide"):
        dev.search_range(ref.sparse_queries(2, V, seed=2), 0.5)
    dev.close()


# ---- filters and deletions ---------------------------------------------------------------------------------------------------------------------
def test_filters_deletions_and_restore():
    n = 1000
    ip, ix, va = ref.csr_case(n, VR, seed=n + 40)
    dev, (_, q, S) = DeviceIndex.from_csr(ip, ix, va, VR), _case(n)
    rng = np.random.default_rng(9)
    shared, per_q = rng.random(n) < 0.5, rng.random((B_MAX, n)) < 0.5
    thr = _mid_thresholds(S, B_MAX, 200)
    for qpp in (0, 1):
        dev.set_queries_per_pass(qpp)
        for allowed in (shared, per_q):
            flt = DocFilter.from_mask(torch.from_numpy(allowed))
            for max_hits in (0, 64, 600):
                _check(dev, q, S, thr, max_hits, allowed, flt, what=("filter", qpp))
            want = _check(dev, q, S, -np.inf, 7, allowed, flt, what="filter, -inf")
            assert (want["counts"] == np.broadcast_to(allowed, (B_MAX, n)).sum(axis=1)).all()          # the popcount of the filter
    dead = rng.choice(n, size=300, replace=False)
    dev.delete_rows(dead)
    live = np.ones(n, dtype=bool)
    live[dead] = False
    for qpp in (0, 1):
        dev.set_queries_per_pass(qpp)
        want = _check(dev, q, S, -np.inf, 7, live, what="deleted, -inf")
        assert (want["counts"] == n - 300).all() and dev.n_live == n - 300
        _check(dev, q, S, thr, 600, live, what="deleted")
        for allowed in (shared, per_q):                             # both together
            flt = DocFilter.from_mask(torch.from_numpy(allowed))
            _check(dev, q, S, thr, 129, allowed & live, flt, what="deleted and filtered")
    dev.restore_rows()
    dev.set_queries_per_pass(0)
    want = _check(dev, q, S, -np.inf, 7, what="restored")
    assert (want["counts"] == n).all()
    dev.close()


def test_host_bitmap_rows_longer_than_the_bitmap_keep_their_tail():
    dev, q, S = _case(65)
    W, ld, B = 3, 5, 4
    words = np.full((B, ld), 0x5A5A5A5A, np.uint32)
    counts = np.zeros(B, np.int64)
    thr = np.zeros(B, F32)
    nat.check(nat.lib().vs_index_search_range(dev._h, C.c_void_p(q.ctypes.data), nat.VS_F32, VR, B, C.c_void_p(thr.ctypes.data), 0, None, 0, 0, 0, None, None,
                                              C.c_void_p(counts.ctypes.data), C.c_void_p(words.ctypes.data), ld, None))
    want = ref.search(S[:B], 0.0, 0)
    assert (words[:, :W] == want["words"]).all() and (words[:, W:] == 0x5A5A5A5A).all() and (counts == want["counts"]).all()
    with pytest.raises(ValueError, match="ld_words"):
        nat.check(nat.lib().vs_index_search_range(dev._h, C.c_void_p(q.ctypes.data), nat.VS_F32, VR, B, C.c_void_p(thr.ctypes.data), 0, None, 0, 0, 0, None,
                                                  None, None, C.c_void_p(words.ctypes.data), 2, None))
    with pytest.raises(ValueError, match="max_hits"):
        nat.check(nat.lib().vs_index_search_range(dev._h, C.c_void_p(q.ctypes.data), nat.VS_F32, VR, B, C.c_void_p(thr.ctypes.data), 2049, None, 0, 0, 0, None,
                                                  None, C.c_void_p(counts.ctypes.data), None, 0, None))
    dthr = torch.from_numpy(thr).cuda()                             # host and device pointers do not mix
    with pytest.raises(ValueError, match="all be host or all device"):
        nat.check(nat.lib().vs_index_search_range(dev._h, C.c_void_p(q.ctypes.data), nat.VS_F32, VR, B, C.c_void_p(dthr.data_ptr()), 0, None, 0, 0, 0, None,
                                                  None, C.c_void_p(counts.ctypes.data), None, 0, None))


# ---- the Python methods: bitmap consistency, explain, shards --------------------------------------------------------------------------------------
def test_methods_and_bitmap_consistency():
    dev, q, S = _case(1000)
    thr = _mid_thresholds(S, B_MAX, 150)
    want = ref.search(S, thr, 100)
    for qq in (q, torch.from_numpy(q), torch.from_numpy(q).cuda()):
        res = dev.search_range(qq, thr, id_offset=0)                # max_hits defaults to 100
        assert isinstance(res, RangeResults) and type(res.ids) is type(qq) and (not isinstance(qq, torch.Tensor) or res.ids.device == qq.device)
        ref.assert_equal_bits(dict(ids=_np(res.ids), scores=_np(res.scores), counts=_np(res.counts)), want, "search_range", ("ids", "scores", "counts"))
        assert (_np(dev.count_matches(qq, thr)) == want["counts"]).all()
    assert (_np(dev.search_range(q, thr, max_hits=5, id_offset=1000).ids) == want["ids"][:, :5] + 1000).all()
    mf = dev.match_filter(q, thr)
    assert isinstance(mf, DocFilter) and mf.per_query and mf.n_queries == B_MAX
    assert (_np(mf.words).view(np.uint32) == want["words"]).all()
    assert (ref.unpack_bits(_np(mf.words), 1000).sum(axis=1) == want["counts"]).all()                  # popcount == counts
    ids, _ = dev.search(q, 50, filter=mf)                           # a search under the match filter returns only matching rows
    m = ref.matches(S, thr)
    assert all(m[b, _np(ids)[b]].all() for b in range(B_MAX)) and (_np(ids) >= 0).all()
    lo = _mid_thresholds(S, B_MAX, 400)                             # a band: at least lo, below thr
    band = dev.match_filter(q, lo) & ~mf
    wb = ref.matches(S, lo) & ~m
    assert wb.any() and (_np(band.words).view(np.uint32) == ref.pack_bits(wb)).all()
    res = dev.search_range(q, -np.inf, max_hits=2048, filter=band)  # ... and a range search under it lists exactly the band
    assert (_np(res.counts) == wb.sum(axis=1)).all()
    ref.assert_equal_bits(dict(ids=_np(res.ids), scores=_np(res.scores), counts=_np(res.counts)), ref.search(S, -np.inf, 2048, wb), "band",
                          ("ids", "scores", "counts"))
    # the scores are explain's, bit for bit
    res = dev.search_range(q, thr, max_hits=40)
    ex = dev.explain(q, _np(res.ids), topn=0)
    assert (_np(ex.scores).view(np.uint32) == _np(res.scores).view(np.uint32)).all()


@pytest.mark.parametrize("store", ["fp32", "bin"])
def test_row_shards_equal_the_unsharded_index(store):
    whole, q, S = _case(1000, store)
    n = 1000
    ndev = torch.cuda.device_count()
    bounds = [0, 437, n]                                            # (437: a shard whose bits do not start on a word)
    shards = [whole.slice_rows(bounds[i], bounds[i + 1] - bounds[i], device=i if ndev >= 2 else 0) for i in range(2)]
    group = ShardGroup(shards)
    allowed = np.random.default_rng(2).random((B_MAX, n)) < 0.7
    flt = DocFilter.from_mask(torch.from_numpy(allowed))
    thr = _mid_thresholds(S, B_MAX, 120)
    for a, f in ((None, None), (allowed, flt)):
        for max_hits in (0, 30, 600):
            want = ref.search(S, thr, max_hits, a)
            for qq in (q, torch.from_numpy(q).cuda()):
                res = group.search_range(qq, thr, max_hits=max_hits, filter=f)
                ref.assert_equal_bits(dict(ids=_np(res.ids), scores=_np(res.scores), counts=_np(res.counts)), want, ("group", max_hits),
                                      ("ids", "scores", "counts"))
            one = whole.search_range(q, thr, max_hits=max_hits, filter=f)
            assert (_np(one.ids) == want["ids"]).all()
        assert (_np(group.count_matches(q, thr, filter=f)) == want["counts"]).all()
        mf = group.match_filter(q, thr, filter=f)
        assert mf.n_rows == n and (_np(mf.words).view(np.uint32) == want["words"]).all()
    group.delete_rows(np.array([5, 500, 999]))
    live = np.ones(n, dtype=bool)
    live[[5, 500, 999]] = False
    try:
        res = group.search_range(q, -np.inf, max_hits=4)
        assert (_np(res.counts) == n - 3).all()
        ref.assert_equal_bits(dict(ids=_np(res.ids), scores=_np(res.scores), counts=_np(res.counts)), ref.search(S, -np.inf, 4, live), "group, deleted",
                              ("ids", "scores", "counts"))
    finally:
        group.restore_rows()
        whole.restore_rows()
    group.close()


# ---- the facade ----------------------------------------------------------------------------------------------------------------------------------
def test_retriever_and_index_facade(tiny_retriever):
    from vsearch_amd.ir import BoTIndex, SparseIndex
    from vsearch_amd.ir.retriever.index import IndexType
    r = tiny_retriever
    n = 80
    r.build_index(make_texts(n, 5), index_type=IndexType.SPARSE)
    idx = r.index
    queries = make_texts(4, 9)
    q_emb = r.process_query(queries, 0, r.encoder_q.config.topk)
    every = torch.arange(n).repeat(4, 1)
    sc = _np(idx.explain(q_emb, every, topn=0).scores).astype(F32)  # [4, n]: the exact score of every pair
    # short random texts: many documents share no term with a query and score 0, so the threshold of a query is the middle one of its
    # DISTINCT scores -- some documents match, some do not
    distinct = [np.unique(sc[b]) for b in range(4)]
    assert all(d.size >= 3 for d in distinct)
    thr = np.array([d[d.size // 2] for d in distinct], dtype=F32)
    want = ref.search(sc, thr, 20)
    cnt = want["counts"]
    assert (cnt >= 1).all() and (cnt < n).all()
    got = r.retrieve_range(queries, thr, max_hits=20)
    assert isinstance(got, RangeResults)
    ref.assert_equal_bits(dict(ids=_np(got.ids), scores=_np(got.scores), counts=_np(got.counts)), want, "retrieve_range", ("ids", "scores", "counts"))
    same = idx.search_range(q_emb, thr, max_hits=20)
    assert (_np(same.ids) == _np(got.ids)).all() and (_np(idx.count_matches(q_emb, thr)) == cnt).all()
    mf = idx.match_filter(q_emb, thr)
    assert (ref.unpack_bits(_np(mf.words), n).sum(axis=1) == cnt).all()
    hits = r.retrieve(queries, k=5, filter=mf)
    m = ref.matches(sc, thr)
    assert all(m[b, _np(hits.ids)[b][_np(hits.ids)[b] >= 0]].all() for b in range(4)) and (_np(hits.ids)[:, 0] >= 0).all()
    cols = _np(idx.get_vectors(torch.tensor([3])).col_indices())   # must=: only the documents with that term are counted
    col = int(cols[_np(idx.doc_freq(cols)).argmin()])
    narrowed = r.retrieve_range(queries, -np.inf, max_hits=n, must=[col])
    df = int(_np(idx.doc_freq(np.array([col])))[0])
    assert 0 < df < n and (_np(narrowed.counts) == df).all()
    with pytest.raises(ValueError, match="2048"):
        r.retrieve_range(queries, 0.5, max_hits=4096)
    # a row-sharded SparseIndex and a BoTIndex
    ip, ix, va = ref.csr_case(1000, VR, seed=1040)
    _, q, S = _case(1000)
    tq = torch.from_numpy(q)
    thr = _mid_thresholds(S, B_MAX, 90)
    want = ref.search(S, thr, 150)
    sp = SparseIndex(device="cuda:0", fp16=False)
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(va), size=(1000, VR))
    sp.move_to_device("cuda:0")
    for sharded in (False, True):
        if sharded:
            sp.shard_rows([0, 0, 0])
            assert sp.shards is not None and len(sp.shards) == 3
        res = sp.search_range(tq, thr, max_hits=150)
        ref.assert_equal_bits(dict(ids=_np(res.ids), scores=_np(res.scores), counts=_np(res.counts)), want, ("SparseIndex", sharded), ("ids", "scores", "counts"))
        assert (_np(sp.count_matches(tq, thr)) == want["counts"]).all()
        assert (_np(sp.match_filter(tq, thr).words).view(np.uint32) == want["words"]).all()
    bot = BoTIndex(device="cuda:0", fp16=False)
    bot.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.ones(va.shape[0]), size=(1000, VR))
    bot.move_to_device("cuda:0")
    assert bot._device_index().info().store_dtype == nat.VS_NONE
    Sb = ref.scores(q, ip, ix, va, "bin")
    thr = _mid_thresholds(Sb, B_MAX, 90)
    res = bot.search_range(tq, thr, max_hits=150)
    ref.assert_equal_bits(dict(ids=_np(res.ids), scores=_np(res.scores), counts=_np(res.counts)), ref.search(Sb, thr, 150), "BoTIndex", ("ids", "scores", "counts"))
