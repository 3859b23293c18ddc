"""GPU tests of the filtered search (vs_index_search_filtered, vs_shard_group_search_filtered, vs_filter_pack; vsearch_amd.doc_filter) --
run on MI355X.

The contract: a filtered search returns, bit for bit, what an unfiltered search returns over the index that holds only the allowed
rows, with ids mapped back to the full index; positions beyond the allowed rows hold id -1, score -inf.  Every search path gates
candidate admission inside its kernels, so each path is forced here (the options the other GPU tests use) and checked against the
sub-index, the CPU oracle, or both."""
import types

import numpy as np
import pytest
import torch

import oracle
from oracle import compare
from conftest import V
from vsearch_amd import synth
from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, ShardGroup
from vsearch_amd.doc_filter import DocFilter

pytestmark = pytest.mark.gpu
RTOL = 1e-4

# (options, expected last_path, expected postings_walk or None); a fresh index per path: option changes rebuild the postings copy
VALUED_PATHS = {
    "quad": (dict(blocked_postings=1, postings_walk=4), 3, 4),
    "list-walk": (dict(blocked_postings=1, postings_walk=0), 3, 0),
    "fp64-walk": (dict(blocked_postings=1, postings_filter=0, postings_walk=-1), 2, None),
    "mq-scan": (dict(blocked_postings=0), 1, None),
    "one-query-scan": (dict(queries_per_pass=1), 0, None),
}
BINARY_PATHS = {
    "bq-packed": (dict(blocked_postings=1, postings_walk=6, postings_packed=1), 3, 6),
    "bq-int32": (dict(blocked_postings=1, postings_walk=6, postings_packed=0), 3, 6),
    "bin-records": (dict(blocked_postings=1, postings_walk=5), 3, 5),
    "mq-scan": (dict(blocked_postings=0), 1, None),
    "one-query-scan": (dict(queries_per_pass=1), 0, None),
}


def _opts(idx, opts):
    for name, value in opts.items():
        if name == "queries_per_pass":
            idx.set_queries_per_pass(value)
        else:
            idx.set_option(name, value)
    return idx


def _sub_csr(ip, ix, d, rows):
    """CSR of the given rows, in order"""
    rows = np.asarray(rows, dtype=np.int64)
    lens = ip[rows + 1] - ip[rows]
    sip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    take = np.concatenate([np.arange(ip[r], ip[r + 1]) for r in rows]) if rows.size else np.zeros(0, np.int64)
    return sip, ix[take], (None if d is None else d[take])


def _expect_sub(ip, ix, d, q, k, allowed, opts, store=None):
    """(ids, scores) of the unfiltered search of the allowed rows' sub-index (searched with the same options), ids mapped back and
    padded to k with -1 / -inf.  `allowed`: one bool mask [N] for the batch or [B, N]."""
    B = q.shape[0]
    ids = np.full((B, k), -1, np.int64)
    sc = np.full((B, k), -np.inf, np.float32)
    masks = [allowed] * B if allowed.ndim == 1 else list(allowed)
    cache = {}
    for b in range(B):
        rows = np.nonzero(masks[b])[0]
        m = min(k, rows.size)
        if m == 0:
            continue
        key = rows.tobytes()
        if key not in cache:
            sip, six, sd = _sub_csr(ip, ix, d, rows)
            sub = _opts(DeviceIndex.from_csr(sip, six, sd, V, store_dtype=store), opts)
            cache[key] = (sub, rows)
        sub, rows = cache[key]
        si, ss = sub.search(q[b:b + 1] if allowed.ndim == 2 else q, m)
        si, ss = np.asarray(si), np.asarray(ss)
        r = 0 if allowed.ndim == 2 else b
        ids[b, :m] = rows[si[r]]
        sc[b, :m] = ss[r]
    return ids, sc


def _check_oracle(ip, ix, d, q, k, allowed, ids, sc):
    """the result is a valid top-k of the oracle's scores with the disallowed rows at -inf, then the padding"""
    _, _, allsc = oracle.csr_search(ip, ix, d, V, q, 1, acc64=True, return_all=True)
    masks = np.broadcast_to(allowed, allsc.shape)
    allsc = np.where(masks, allsc, -np.inf)
    for b in range(q.shape[0]):
        m = min(k, int(masks[b].sum()))
        if m:
            compare.check_topk_valid(allsc[b:b + 1], ids[b:b + 1, :m], sc[b:b + 1, :m], rtol=RTOL)
        assert (ids[b, m:] == -1).all() and np.isneginf(sc[b, m:]).all(), f"query {b}: padding"


def _filters(n, k, rng):
    """the shared filters of the contract: all rows, 50 %, 1 %, only rows in the last partial block, fewer than k, empty"""
    last = np.zeros(n, bool)
    last[n - (n % 2048 or 2048) + 3::5] = True
    few = np.zeros(n, bool)
    few[rng.choice(n, k // 3, replace=False)] = True
    return {"all": np.ones(n, bool), "half": rng.random(n) < 0.5, "one-pct": rng.random(n) < 0.01, "last-block": last,
            "fewer-than-k": few, "empty": np.zeros(n, bool)}


def _assert_path(info, path, walk, name):
    assert info.last_path == path, (name, info.last_path)
    if walk is not None:
        assert info.postings_walk == walk, (name, info.postings_walk)


@pytest.mark.parametrize("store,kind", [(nat.VS_F32, synth.KIND_VDR), (nat.VS_F16, synth.KIND_VDR), (nat.VS_F32, synth.KIND_SKEW)])
def test_valued_paths_equal_the_sub_index(store, kind):
    n, B, k = 20000, 6, 100
    rng = np.random.default_rng(1)
    ip, ix, d = oracle.synth_csr(3, 0, n, V, 768, kind)
    d = d.astype(np.float16) if store == nat.VS_F16 else d
    q = oracle.synth_queries(2, B, kind=kind)
    filters = _filters(n, k, rng)
    for path, (opts, want_path, want_walk) in VALUED_PATHS.items():
        if kind == synth.KIND_SKEW and path == "quad":
            opts = dict(opts, postings_head=0)        # (head columns -- the Zipf corpus has them -- take the list walk; the quad walk runs without)
        idx = _opts(DeviceIndex.from_csr(ip, ix, d, V), opts)
        u_ids, u_sc = map(np.asarray, idx.search(q, k))
        if kind == synth.KIND_SKEW and path == "list-walk":
            assert idx.info().head_columns > 0                                # (the head pre-pass's sums go through the same gate)
        for fname, mask in filters.items():
            ids, sc = map(np.asarray, idx.search(q, k, filter=DocFilter.from_mask(mask)))
            _assert_path(idx.info(), want_path, want_walk, (path, fname))
            e_ids, e_sc = _expect_sub(ip, ix, d, q, k, mask, opts if path == "one-query-scan" else dict(blocked_postings=0))
            assert (ids == e_ids).all() and (sc == e_sc).all(), (path, fname)
            if fname == "all":
                assert (ids == u_ids).all() and (sc == u_sc).all(), (path, "all-ones filter != unfiltered")
            if path == "quad" and store == nat.VS_F32:
                _check_oracle(ip, ix, d.astype(np.float32), q, k, mask, ids, sc)


@pytest.mark.parametrize("n", [2000, 30000])
def test_binary_paths_equal_the_sub_index(n):
    B, k = 9, 50
    rng = np.random.default_rng(n)
    ip, ix, _ = oracle.synth_csr(5, 0, n, V, 86, synth.KIND_BOT)
    q = oracle.synth_queries(6, B, V, 776, synth.VAL_DYADIC)
    filters = _filters(n, k, rng)
    for path, (opts, want_path, want_walk) in BINARY_PATHS.items():
        idx = _opts(DeviceIndex.from_csr(ip, ix, None, V), opts)
        u_ids, u_sc = map(np.asarray, idx.search(q, k))
        for fname, mask in filters.items():
            ids, sc = map(np.asarray, idx.search(q, k, filter=mask))                 # (a bool mask: packed by the search)
            _assert_path(idx.info(), want_path, want_walk, (path, fname))
            e_ids, e_sc = _expect_sub(ip, ix, None, q, k, mask, dict(blocked_postings=0))
            assert (ids == e_ids).all() and (sc == e_sc).all(), (path, fname)
            if fname == "all":
                assert (ids == u_ids).all() and (sc == u_sc).all(), (path, "all-ones filter != unfiltered")
        if path == "bq-packed":
            _check_oracle(ip, ix, None, q, k, filters["half"], *map(np.asarray, idx.search(q, k, filter=filters["half"])))


def test_dense_index():
    n, C, B, k = 3000, 512, 5, 40
    rng = np.random.default_rng(7)
    mat = rng.standard_normal((n, C)).astype(np.float32)
    q = rng.standard_normal((B, C)).astype(np.float32)
    idx = DeviceIndex.from_dense(mat)
    u_ids, u_sc = map(np.asarray, idx.search(q, k))
    for fname, mask in _filters(n, k, rng).items():
        ids, sc = map(np.asarray, idx.search(q, k, filter=mask))
        rows = np.nonzero(mask)[0]
        m = min(k, rows.size)
        if m:
            s_ids, s_sc = map(np.asarray, DeviceIndex.from_dense(np.ascontiguousarray(mat[rows])).search(q, m))
            assert (ids[:, :m] == rows[s_ids]).all() and (sc[:, :m] == s_sc).all(), fname
        assert (ids[:, m:] == -1).all() and np.isneginf(sc[:, m:]).all(), fname
        if fname == "all":
            assert (ids == u_ids).all() and (sc == u_sc).all()


def test_per_query_filters_and_doc_to_doc():
    """one bitmap per query (filter_ld > 0): random halves, and doc-to-doc search that must not return the query's own row"""
    n, B, k = 20000, 8, 64
    rng = np.random.default_rng(11)
    ip, ix, d = oracle.synth_csr(9, 0, n, V, 768)
    own = rng.choice(n, B, replace=False)
    q = np.zeros((B, V), np.float32)
    for b, r in enumerate(own):
        q[b, ix[ip[r]:ip[r + 1]]] = d[ip[r]:ip[r + 1]]
    per = rng.random((B, n)) < 0.5
    excl = np.ones((B, n), bool)
    excl[np.arange(B), own] = False
    for path in ("quad", "list-walk", "mq-scan", "one-query-scan"):
        opts, want_path, want_walk = VALUED_PATHS[path]
        idx = _opts(DeviceIndex.from_csr(ip, ix, d, V), opts)
        u_ids, _ = map(np.asarray, idx.search(q, k))
        assert (u_ids[:, 0] == own).all()                                     # (the query's own row is its best match)
        for fname, mask in (("half", per), ("exclude-own", excl)):
            f = DocFilter.from_mask(torch.from_numpy(mask))
            assert f.per_query and f.ld == (n + 31) // 32
            ids, sc = map(np.asarray, idx.search(q, k, filter=f))
            _assert_path(idx.info(), want_path, want_walk, (path, fname))
            e_ids, e_sc = _expect_sub(ip, ix, d, q, k, mask, opts if path == "one-query-scan" else dict(blocked_postings=0))
            assert (ids == e_ids).all() and (sc == e_sc).all(), (path, fname)
        ids2, _ = map(np.asarray, idx.search(q, k, filter=DocFilter.from_ids(torch.from_numpy(own[:, None]), n, allow=False)))
        assert not (ids2 == own[:, None]).any() and (ids2 == e_ids).all(), path


def test_from_ids_per_query_with_padding():
    """[B, m] id sets padded with -1: a pad sets nothing, also where the row holds a real id 0 (allow and exclude)"""
    n = 70
    ids = torch.tensor([[0, 5, -1], [-1, 0, 7], [3, -1, -1], [-1, -1, -1], [0, -1, 69]])
    want = np.zeros((ids.shape[0], n), bool)
    for b, row in enumerate(ids.tolist()):
        want[b, [i for i in row if i >= 0]] = True
    for allow in (True, False):
        f = DocFilter.from_ids(ids, n, allow=allow)
        bits = np.unpackbits(f.words.cpu().numpy().view(np.uint32).view(np.uint8), bitorder="little").reshape(ids.shape[0], -1)[:, :n]
        assert (bits.astype(bool) == (want if allow else ~want)).all(), allow
    # doc-to-doc: each query is an index row and excludes itself and a known positive, row 0 among them, the lists ragged
    ip, ix, d = oracle.synth_csr(14, 0, 3000, V, 768)
    own = np.array([0, 17, 250, 1999])
    q = np.zeros((len(own), V), np.float32)
    for b, r in enumerate(own):
        q[b, ix[ip[r]:ip[r + 1]]] = d[ip[r]:ip[r + 1]]
    excl = torch.tensor([[0, -1], [17, 0], [250, -1], [1999, 0]])
    idx = DeviceIndex.from_csr(ip, ix, d, V)
    ids2, _ = map(np.asarray, idx.search(q, 20, filter=DocFilter.from_ids(excl, 3000, allow=False)))
    for b, row in enumerate(excl.tolist()):
        assert not np.isin(ids2[b], [i for i in row if i >= 0]).any(), b


def test_per_query_filters_over_many_tiles():
    """per-query filters for 40 queries: tiles whose first query is not 0 ((q0 + q) * filter_ld) on the quad walk and the 8-query scan"""
    n, B, k = 20000, 40, 50
    rng = np.random.default_rng(23)
    ip, ix, d = oracle.synth_csr(15, 0, n, V, 768)
    q = oracle.synth_queries(16, B)
    per = rng.random((B, n)) < np.linspace(0.05, 0.9, B)[:, None]
    for path in ("quad", "mq-scan"):
        opts, want_path, want_walk = VALUED_PATHS[path]
        idx = _opts(DeviceIndex.from_csr(ip, ix, d, V), opts)
        ids, sc = map(np.asarray, idx.search(q, k, filter=DocFilter.from_mask(per)))
        _assert_path(idx.info(), want_path, want_walk, path)
        e_ids, e_sc = _expect_sub(ip, ix, d, q, k, per, dict(blocked_postings=0))
        assert (ids == e_ids).all() and (sc == e_sc).all(), path


def _grouped(B, n, groups, rows_of):
    """per-query masks that take `groups` distinct values, the group changing every 100 queries"""
    g = (np.arange(B) // 100) % groups
    masks = np.stack([rows_of(x) for x in range(groups)])
    return g, masks[g]


def test_per_query_filters_across_sub_batches():
    """a batch the search cuts into sub-batches (the one-query scan at k = 2048, the dense index at 150 000 rows): every sub-batch reads its
    own queries' bitmaps (filter offset by the sub-batch's first query)"""
    # one-query scan: 1000 queries x k = 2048 take two sub-batches of the candidate scratch
    n, B, k = 20000, 1000, 2048
    ip, ix, d = oracle.synth_csr(17, 0, n, V, 768)
    q = oracle.synth_queries(18, B)
    g, per = _grouped(B, n, 5, lambda x: (np.arange(n) % 5) == x)
    idx = _opts(DeviceIndex.from_csr(ip, ix, d, V), dict(queries_per_pass=1))
    ids, sc = map(np.asarray, idx.search(q, k, filter=per))
    assert idx.info().last_path == 0
    for x in range(5):
        rows = np.nonzero(per[np.argmax(g == x)])[0]
        sip, six, sd = _sub_csr(ip, ix, d, rows)
        sub = _opts(DeviceIndex.from_csr(sip, six, sd, V), dict(queries_per_pass=1))
        s_ids, s_sc = map(np.asarray, sub.search(q[g == x], k))
        assert (ids[g == x] == rows[s_ids]).all() and (sc[g == x] == s_sc).all(), x
    # dense index of 150 000 rows: 894 queries a sub-batch, the select of > 8192 keys (select_topk_kernel), a group with fewer than k rows
    n, C, B, k = 150_000, 64, 1000, 40
    rng = np.random.default_rng(19)
    mat = rng.standard_normal((n, C)).astype(np.float32)
    qd = rng.standard_normal((B, C)).astype(np.float32)
    g, per = _grouped(B, n, 5, lambda x: ((np.arange(n) % 5) == x) if x < 4 else np.isin(np.arange(n), [3, 70_000, 149_999]))
    idx = DeviceIndex.from_dense(mat)
    ids, sc = map(np.asarray, idx.search(qd, k, filter=per))
    for x in range(5):
        rows = np.nonzero(per[np.argmax(g == x)])[0]
        m = min(k, rows.size)
        s_ids, s_sc = map(np.asarray, DeviceIndex.from_dense(np.ascontiguousarray(mat[rows])).search(qd[g == x], m))
        assert (ids[g == x, :m] == rows[s_ids]).all() and (sc[g == x, :m] == s_sc).all(), x
        assert (ids[g == x, m:] == -1).all() and np.isneginf(sc[g == x, m:]).all(), x


def test_dense_index_select_with_padding():
    """more than 8192 rows: the dense index's select (select_topk_kernel) under shared filters, fewer than k allowed rows included"""
    n, C, B, k = 12000, 128, 6, 64
    rng = np.random.default_rng(29)
    mat = rng.standard_normal((n, C)).astype(np.float32)
    q = rng.standard_normal((B, C)).astype(np.float32)
    idx = DeviceIndex.from_dense(mat)
    u_ids, u_sc = map(np.asarray, idx.search(q, k))
    for fname, mask in _filters(n, k, rng).items():
        ids, sc = map(np.asarray, idx.search(q, k, filter=mask))
        rows = np.nonzero(mask)[0]
        m = min(k, rows.size)
        if m:
            s_ids, s_sc = map(np.asarray, DeviceIndex.from_dense(np.ascontiguousarray(mat[rows])).search(q, m))
            assert (ids[:, :m] == rows[s_ids]).all() and (sc[:, :m] == s_sc).all(), fname
        assert (ids[:, m:] == -1).all() and np.isneginf(sc[:, m:]).all(), fname
        if fname == "all":
            assert (ids == u_ids).all() and (sc == u_sc).all()


def test_deep_k_padding_and_sub_index():
    """k = 1500 (past the one-pass candidate buffers): 1000 allowed rows give 500 padding entries; a 30 % filter equals the sub-index"""
    n, B, k = 20000, 4, 1500
    rng = np.random.default_rng(13)
    ip, ix, d = oracle.synth_csr(4, 0, n, V, 768)
    q = oracle.synth_queries(8, B)
    idx = DeviceIndex.from_csr(ip, ix, d, V)
    few = np.zeros(n, bool)
    few[rng.choice(n, 1000, replace=False)] = True
    ids, sc = map(np.asarray, idx.search(q, k, filter=DocFilter.from_ids(np.nonzero(few)[0], n)))
    assert (ids[:, 1000:] == -1).all() and np.isneginf(sc[:, 1000:]).all()
    assert all(set(ids[b, :1000].tolist()) == set(np.nonzero(few)[0].tolist()) for b in range(B))
    _check_oracle(ip, ix, d, q, k, few, ids, sc)
    third = rng.random(n) < 0.3
    ids, sc = map(np.asarray, idx.search(q, k, filter=third))
    e_ids, e_sc = _expect_sub(ip, ix, d, q, k, third, dict(blocked_postings=0))
    assert (ids == e_ids).all() and (sc == e_sc).all()


def test_sharded_group_with_unaligned_boundaries():
    n, B, k = 20000, 6, 100
    rng = np.random.default_rng(17)
    ip, ix, d = oracle.synth_csr(12, 0, n, V, 768)
    q = oracle.synth_queries(3, B)
    full = DeviceIndex.from_csr(ip, ix, d, V)
    bounds = [0, 7001, 13333, n]                                             # (no boundary on a word of the bitmap)
    shards = []
    for r0, r1 in zip(bounds[:-1], bounds[1:]):
        sip, six, sd = _sub_csr(ip, ix, d, np.arange(r0, r1))
        shards.append(DeviceIndex.from_csr(sip, six, sd, V))
    group = ShardGroup(shards)
    shared = rng.random(n) < 0.4
    per = rng.random((B, n)) < 0.2
    few = np.zeros(n, bool)
    few[[5, 7000, 7001, 7002, 13332, 13333, 19999]] = True                 # fewer than k, on both sides of every boundary
    for mask in (shared, per, few):
        want = map(np.asarray, full.search(q, k, filter=mask))
        got = map(np.asarray, group.search(q, k, filter=DocFilter.from_mask(mask)))
        (w_ids, w_sc), (g_ids, g_sc) = want, got
        assert (g_ids == w_ids).all() and (g_sc == w_sc).all()
    # host queries and a device bitmap, through the facade's row sharding (equal ranges of 6667 rows)
    from vsearch_amd.ir import SparseIndex
    sp = SparseIndex(device="cuda:0")
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(d), size=(n, V))
    sp.move_to_device("cuda:0")
    sp.shard_rows([0, 0, 0])
    res = sp.search(torch.from_numpy(q), k, filter=torch.from_numpy(shared))
    w_ids, w_sc = map(np.asarray, full.search(q, k, filter=shared))
    assert (res.ids.cpu().numpy() == w_ids).all() and (res.scores.float().cpu().numpy() == w_sc).all()
    with pytest.raises(ValueError):
        sp.search(torch.from_numpy(q), k, filter=torch.ones(n - 1, dtype=torch.bool))


def test_async_device_filter_on_torch_stream():
    n, B, k = 20000, 16, 100
    ip, ix, d = oracle.synth_csr(21, 0, n, V, 768)
    q = oracle.synth_queries(4, B)
    idx = DeviceIndex.from_csr(ip, ix, d, V).prepare()
    mask = torch.rand(n, generator=torch.Generator().manual_seed(3)) < 0.5
    want = map(np.asarray, idx.search(q, k, filter=mask.numpy()))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        f = DocFilter.from_mask(mask.cuda())                                  # (packed on the stream the search runs on)
        qd = torch.from_numpy(q).cuda()
        ids, sc = idx.search(qd, k, filter=f)
    stream.synchronize()
    assert idx.info().last_path == 3
    w_ids, w_sc = want
    assert (ids.cpu().numpy() == w_ids).all() and (sc.cpu().numpy() == w_sc).all()


def test_filter_pack_and_arguments():
    rng = np.random.default_rng(5)
    for n in (1, 31, 32, 33, 1000, 4099):
        m = rng.random((3, n)) < 0.5
        f = DocFilter.from_mask(m)
        words = f.words.cpu().numpy().view(np.uint32)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little").reshape(3, -1)
        assert (bits[:, :n] == m).all() and not bits[:, n:].any()
    idx = DeviceIndex.from_csr(*oracle.synth_csr(1, 0, 500, V, 768), V)
    q = oracle.synth_queries(1, 2)
    with pytest.raises(ValueError):
        idx.search(q, 10, filter=np.ones(499, bool))                          # a mask of another length
    with pytest.raises(ValueError):
        idx.search(q, 10, filter=DocFilter.from_mask(np.ones((3, 500), bool)))  # per-query filter of another batch
    with pytest.raises(RuntimeError):
        idx.search(q, 501, filter=np.ones(500, bool))                         # k > n_rows: VS_ERANGE as before
    ids, sc = map(np.asarray, idx.search(q, 10, filter=torch.tensor([3, 17, 499])))     # integer ids to allow
    assert sorted(ids[0, :3].tolist()) == [3, 17, 499] and (ids[:, 3:] == -1).all() and np.isneginf(sc[:, 3:]).all()


def _oracle_pin_filtered(seed, n, q, ids, sc, k, allowed, windows=24, window_rows=8192):
    """_oracle_pin of tests/test_gpu_filter.py under a filter: returned rows are allowed and re-scored by the oracle; in sampled windows no
    allowed row beats a query's k-th returned score without being returned."""
    B = q.shape[0]
    allow = np.broadcast_to(allowed, (B, n))
    for b in range(B):
        rows = ids[b]
        assert (rows >= 0).all() and allow[b, rows].all(), f"query {b}: a disallowed row was returned"
        parts = [oracle.synth_csr(seed, int(r), 1, V, 768, 0, 0) for r in rows]
        ip = np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])]).astype(np.int64)
        _, _, allsc = oracle.csr_search(ip, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), V, q[b:b + 1], 1,
                                        acc64=True, return_all=True)
        assert np.allclose(allsc[0].astype(np.float32), sc[b], rtol=RTOL, atol=0), f"query {b}: returned scores differ from the oracle's"
    starts = np.unique(np.concatenate([np.linspace(0, n - window_rows, windows).astype(np.int64), [n - window_rows]]))
    for r0 in starts:
        ip, ix, d = oracle.synth_csr(seed, int(r0), window_rows, V, 768, 0, 0)
        _, _, allsc = oracle.csr_search(ip, ix, d, V, q, 1, acc64=True, return_all=True)
        for b in range(B):
            kth = sc[b, k - 1]
            better = np.nonzero((allsc[b] > kth * (1 + RTOL)) & allow[b, r0:r0 + window_rows])[0] + r0
            missing = np.setdiff1d(better, ids[b])
            assert missing.size == 0, f"query {b}: allowed rows {missing[:5]} beat the k-th score {kth} and were not returned"


def test_large_index_quad_walk_against_one_query_scan_and_oracle():
    """4 M documents: the quad walk (the default of a valued index) under a 10 % shared filter and per-query filters equals the same
    filtered search on the one-query scan, and is pinned to the CPU oracle"""
    n, B, k, seed = 4_000_000, 8, 100, 31
    idx = DeviceIndex.synthetic(seed, 0, n, V, 768, synth.KIND_VDR, 0, nat.VS_F32)
    q = oracle.synth_queries(9, B)
    g = torch.Generator(device="cuda").manual_seed(1)
    shared = torch.rand(n, device="cuda", generator=g) < 0.1
    per = torch.rand((B, n), device="cuda", generator=g) < 0.1
    scan = DeviceIndex.synthetic(seed, 0, n, V, 768, synth.KIND_VDR, 0, nat.VS_F32)
    scan.set_queries_per_pass(1)
    for mask in (shared, per):
        f = DocFilter.from_mask(mask)
        ids, sc = map(np.asarray, idx.search(q, k, filter=f))
        info = idx.info()
        assert info.last_path == 3 and info.postings_walk == 4
        s_ids, s_sc = map(np.asarray, scan.search(q, k, filter=f))
        assert scan.info().last_path == 0
        # (the one-query scan's scores are fp32 partial sums per lane, the refine step's fp64 sums: they agree to rounding -- unfiltered as
        #  filtered -- and documents whose scores are that close may trade places)
        compare.compare_topk(s_ids, s_sc, ids, sc, rtol=1e-5, tie_rtol=1e-5)
        _oracle_pin_filtered(seed, n, q, ids, sc, k, mask.cpu().numpy())


def test_retrieve_with_filter_and_rerank():
    """Retriever.retrieve(filter=...) on a bag-of-token index with rerank: hits are allowed rows; with fewer allowed rows than k the padding
    (id -1, -inf) stays last and is never looked up with get_sample"""
    from vsearch_amd.ir import BoTIndex, Retriever
    n, B, k = 3000, 4, 20
    ip, ix, d = oracle.synth_csr(2, 0, n, V, 86, synth.KIND_BOT)
    bot = BoTIndex()
    bot.data = [str(i) for i in range(n)]
    bot.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(d.astype(np.float32)), size=(n, V))
    bot.move_to_device("cuda")
    looked_up = []
    get = bot.get_sample
    bot.get_sample = lambda i: (looked_up.append(i), get(i))[1]
    ip2, ix2, d2 = oracle.synth_csr(8, 0, n)
    p_dense = torch.sparse_csr_tensor(torch.from_numpy(ip2), torch.from_numpy(ix2.astype(np.int64)), torch.from_numpy(d2), size=(n, V)).to_dense().cuda()
    fake = types.SimpleNamespace(index=bot, device="cuda", encoder_q=types.SimpleNamespace(config=types.SimpleNamespace(topk=768)),
                                 encoder_p=types.SimpleNamespace(embed=lambda texts, batch_size=32, require_grad=False, **kw: p_dense[[int(t) for t in texts]]))
    fake.process_query = types.MethodType(Retriever.process_query, fake)
    fake._rerank = types.MethodType(Retriever._rerank, fake)
    q = torch.from_numpy(oracle.synth_queries(7, B))
    allowed = np.arange(100, 3000, 7)
    res = Retriever.retrieve(fake, q, k=k, rerank=True, filter=torch.from_numpy(allowed))
    assert np.isin(res.ids.cpu().numpy(), allowed).all()
    few = np.array([11, 500, 2999])
    looked_up.clear()
    res = Retriever.retrieve(fake, q, k=k, rerank=True, filter=torch.from_numpy(few), batch_size=1)
    ids, sc = res.ids.cpu().numpy(), res.scores.float().cpu().numpy()
    assert -1 not in looked_up and sorted(set(looked_up)) == few.tolist()
    assert (np.sort(ids[:, :3], axis=1) == few).all() and (ids[:, 3:] == -1).all() and np.isneginf(sc[:, 3:]).all()
    assert np.isfinite(sc[:, :3]).all() and (np.diff(sc[:, :3], axis=1) <= 0).all()
    plain = Retriever.retrieve(fake, q, k=k, filter=torch.from_numpy(few))
    assert (plain.ids.cpu().numpy()[:, 3:] == -1).all()
