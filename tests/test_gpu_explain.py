"""GPU tests of explain (vs_index_explain, vs_shard_group_explain; DeviceIndex / ShardGroup / Index .explain, Index.disentangle,
Retriever.explain_results) -- run on MI355X.

The contract: for every (query, document id) pair the top `topn` columns by contribution fl32(q[c] * v) (contribution descending, then
column ascending), the number of matched terms (non-zero products) and the pair's score, which on a CSR-packet index is the library's
exact row sum -- the score the search paths return for the pair.  Checked against a numpy oracle built from export_csr()."""
import numpy as np
import pytest
import torch

import oracle
from conftest import V
from vsearch_amd import synth
from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, ShardGroup
from vsearch_amd.doc_filter import DocFilter
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

pytestmark = pytest.mark.gpu
RTOL = 1e-4

# (options, expected last_path); the forced paths of tests/test_gpu_doc_filter.py
VALUED_PATHS = {
    "quad": dict(blocked_postings=1, postings_walk=4),
    "list-walk": dict(blocked_postings=1, postings_walk=0),
    "fp64-walk": dict(blocked_postings=1, postings_filter=0, postings_walk=-1),
    "mq-scan": dict(blocked_postings=0),
    "one-query-scan": dict(queries_per_pass=1),
}
BINARY_PATHS = {
    "bq-packed": dict(blocked_postings=1, postings_walk=6, postings_packed=1),
    "bq-int32": dict(blocked_postings=1, postings_walk=6, postings_packed=0),
    "bin-records": dict(blocked_postings=1, postings_walk=5),
    "mq-scan": dict(blocked_postings=0),
    "one-query-scan": dict(queries_per_pass=1),
}
# the one-query scan sums a row in fp32 across its lane group (csr_scan.h: row_partial); every other path re-scores with the exact row sum
FP32_SUM_PATHS = {"one-query-scan"}


def _opts(idx, opts):
    for name, value in opts.items():
        if name == "queries_per_pass":
            idx.set_queries_per_pass(value)
        else:
            idx.set_option(name, value)
    return idx


def _row_terms(ip, ix, d, r):
    cols = ix[ip[r]:ip[r + 1]].astype(np.int64)
    vals = np.ones(cols.size, np.float32) if d is None else d[ip[r]:ip[r + 1]].astype(np.float32)
    return cols, vals


def _oracle(ip, ix, d, q, ids, topn):
    """(cols, contrib, n_matched, fp64 sums) of every pair; q: fp32 rows as the index reads them (None: disentangle)"""
    B, k = ids.shape
    cols = np.full((B, k, topn), -1, np.int32)
    contrib = np.zeros((B, k, topn), np.float32)
    nm = np.zeros((B, k), np.int32)
    sums = np.full((B, k), -np.inf)
    for b in range(B):
        for j in range(k):
            r = int(ids[b, j])
            if r < 0:
                continue
            c, v = _row_terms(ip, ix, d, r)
            prod = v if q is None else (q[b, c].astype(np.float32) * v).astype(np.float32)
            m = prod != 0
            c, prod = c[m], prod[m]
            order = np.lexsort((c, -prod.astype(np.float64)))
            c, prod = c[order], prod[order]
            nm[b, j] = c.size
            sums[b, j] = prod.astype(np.float64).sum()
            t = min(topn, c.size)
            cols[b, j, :t] = c[:t]
            contrib[b, j, :t] = prod[:t]
    return cols, contrib, nm, sums


def _check(ex, want, label):
    cols, contrib, nm, _ = want
    g_cols, g_contrib, g_sc, g_nm = map(np.asarray, (t.cpu() if isinstance(t, torch.Tensor) else t for t in ex))
    assert (g_nm == nm).all(), (label, "n_matched")
    assert (g_cols == cols).all(), (label, "cols")
    assert (g_contrib.view(np.uint32) == contrib.view(np.uint32)).all(), (label, "contrib")
    return g_sc


def _q_as_index(q, store):
    return q.astype(np.float16).astype(np.float32) if store == nat.VS_F16 else q.astype(np.float32)


@pytest.mark.parametrize("store", [nat.VS_F32, nat.VS_F16])
def test_valued_index_equals_oracle_and_search_scores(store):
    n, B, k = 20000, 37, 50
    ip, ix, d = oracle.synth_csr(3, 0, n, V, 768, synth.KIND_VDR)
    d = d.astype(np.float16) if store == nat.VS_F16 else d
    q = oracle.synth_queries(2, B, kind=synth.KIND_VDR)
    qi = _q_as_index(q, store)
    eip, eix, ed = DeviceIndex.from_csr(ip, ix, d, V).export_csr()
    for path, opts in VALUED_PATHS.items():
        idx = _opts(DeviceIndex.from_csr(ip, ix, d, V), opts)
        ids, sc = map(np.asarray, idx.search(q, k))
        for topn in (0, 1, 10, 1024):
            ex = idx.explain(q, ids, topn=topn)
            want = _oracle(eip, eix, ed, qi, ids, topn)
            g_sc = _check(ex, want, (path, topn))
            if path in FP32_SUM_PATHS:
                np.testing.assert_allclose(g_sc, sc, rtol=RTOL)
            else:
                assert (g_sc.view(np.uint32) == sc.view(np.uint32)).all(), (path, topn, "score != search score")
            if topn == 1024:
                assert (want[2] <= topn).all()
                assert (want[3].astype(np.float32) == g_sc).all(), (path, "fp64 sum of contrib != score")


def test_binary_index_equals_oracle_and_search_scores():
    n, B, k = 30000, 37, 50
    ip, ix, _ = oracle.synth_csr(5, 0, n, V, 86, synth.KIND_BOT)
    q = oracle.synth_queries(6, B, V, 776, synth.VAL_DYADIC)
    eip, eix, _ = DeviceIndex.from_csr(ip, ix, None, V).export_csr()
    for path, opts in BINARY_PATHS.items():
        idx = _opts(DeviceIndex.from_csr(ip, ix, None, V), opts)
        ids, sc = map(np.asarray, idx.search(q, k))
        for topn in (0, 1, 10, 1024):
            ex = idx.explain(q, ids, topn=topn)
            want = _oracle(eip, eix, None, q.astype(np.float32), ids, topn)
            g_sc = _check(ex, want, (path, topn))
            assert (g_sc.view(np.uint32) == sc.view(np.uint32)).all(), (path, topn, "score != search score")
            if topn == 1024:
                assert (want[3].astype(np.float32) == g_sc).all()


def test_padding_unmatched_duplicates_and_range():
    from vsearch_amd.ir import SparseIndex
    n, B, k = 3000, 4, 50
    ip, ix, d = oracle.synth_csr(14, 0, n, V, 768)
    q = oracle.synth_queries(15, B)
    idx = DeviceIndex.from_csr(ip, ix, d, V)
    eip, eix, ed = idx.export_csr()
    # a filtered search with fewer allowed rows than k: its padding explains as padding
    allowed = np.zeros(n, bool)
    allowed[[5, 77, 1999]] = True
    ids, sc = map(np.asarray, idx.search(q, k, filter=DocFilter.from_mask(allowed)))
    assert (ids[:, 3:] == -1).all()
    ex = idx.explain(q, ids, topn=10)
    assert (ex.cols[:, 3:] == -1).all() and (ex.contrib[:, 3:] == 0).all()
    assert np.isneginf(ex.scores[:, 3:]).all() and (ex.n_matched[:, 3:] == 0).all()
    assert (ex.scores[:, :3].view(np.uint32) == sc[:, :3].view(np.uint32)).all()
    # a query sharing no column with a row: 0 matched, score 0; duplicates: identical rows
    r = 123
    qz = q.copy()
    qz[0, ix[ip[r]:ip[r + 1]]] = 0.0
    dup = np.array([[r, r, 7, 7]] * B, np.int64)
    ex = idx.explain(qz, dup, topn=16)
    assert ex.n_matched[0, 0] == 0 and ex.scores[0, 0] == 0.0 and (ex.cols[0, 0] == -1).all()
    for a, b in ((0, 1), (2, 3)):
        for t in ex:
            assert (t[:, a] == t[:, b]).all()
    _check(ex, _oracle(eip, eix, ed, qz, dup, 16), "dup")
    # rows outside [-1, N): "not mine" at the C level, IndexError at the Index level
    ex = idx.explain(q[:1], np.array([[n, n + 5, 0]], np.int64), topn=4)
    assert (ex.n_matched[0, :2] == -1).all() and ex.n_matched[0, 2] > 0
    ex = idx.explain(q[:1], np.array([[2, 3]], np.int64), topn=4, id_offset=2)
    assert ex.n_matched[0, 0] > 0 and ex.n_matched[0, 1] > 0
    assert (ex.scores[0] == idx.explain(q[:1], np.array([[0, 1]], np.int64), topn=4).scores[0]).all()
    sp = SparseIndex(device="cuda:0")
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(d), size=(n, V))
    sp.move_to_device("cuda:0")
    for bad in ([[n]], [[-2]]):
        with pytest.raises(IndexError):
            sp.explain(torch.from_numpy(q[:1]), torch.tensor(bad))


def test_dense_mfma_and_logical_dense_index():
    rng = np.random.default_rng(31)
    n, B, k = 300, 6, 20
    mat = np.where(rng.random((n, V)) < 0.5, rng.random((n, V)), 0).astype(np.float32)
    mat[:40] = rng.random((40, V)).astype(np.float32) + 0.01                      # dense rows: > 1024 matched terms with dense queries
    q = rng.random((B, V)).astype(np.float32) + 0.01                              # dense queries
    q[B // 2:] *= rng.random((B - B // 2, V)) < 0.05                              # and sparser ones
    q = q.astype(np.float32)
    dense = DeviceIndex.from_dense(mat)
    assert dense.info().n_packets == 0
    logical = DeviceIndex.from_dense(mat, max_density=1.0)
    assert logical.info().n_packets > 0                                          # (a dense Index stored as CSR packets)
    ip = np.concatenate([[0], np.cumsum((mat != 0).sum(1))]).astype(np.int64)
    ix = np.nonzero(mat)[1].astype(np.int64)
    dv = mat[mat != 0].astype(np.float32)
    for name, idx in (("mfma", dense), ("logical-dense", logical)):
        ids, sc = map(np.asarray, idx.search(q, k))
        ids[:, -4:] = np.arange(4)[None, :]                                       # the dense rows, whatever the search returned
        for topn in (10, 1024):
            ex = idx.explain(q, ids, topn=topn)
            want = _oracle(ip, ix, dv, q, ids, topn)
            assert (want[2][:, -4:] > 1024).all()
            g_sc = _check(ex, want, (name, topn))
            if name == "mfma":
                np.testing.assert_allclose(g_sc[:, :-4], sc[:, :-4], rtol=RTOL)
                assert (g_sc == want[3].astype(np.float32)).all()                 # (fp64 sums of the same products)
            elif idx.info().last_path != 0:
                assert (g_sc[:, :-4].view(np.uint32) == sc[:, :-4].view(np.uint32)).all()
            else:                                                                 # (the one-query scan: fp32 row sums)
                np.testing.assert_allclose(g_sc[:, :-4], sc[:, :-4], rtol=RTOL)
        # disentangle: the rows' own values
        ex = idx.explain(None, ids, topn=100)
        _check(ex, _oracle(ip, ix, dv, None, ids, 100), (name, "disentangle"))


def test_shard_group_equals_unsharded():
    n, B, k = 25000, 11, 40
    ip, ix, d = oracle.synth_csr(12, 0, n, V, 768)
    q = oracle.synth_queries(3, B)
    whole = DeviceIndex.from_csr(ip, ix, d, V)
    ids, _ = map(np.asarray, whole.search(q, k))
    ids[:, -1] = -1
    ids[:, -2] = n - 1
    ids[:, -3] = 0
    ngpu = torch.cuda.device_count()
    bounds = [0, 6001, 13337, 13338, n]                                       # unaligned boundaries, a one-row shard
    layouts = [[0] * 4]
    if ngpu > 1:
        layouts.append([i % ngpu for i in range(4)])
    for devs in layouts:
        shards = [whole.slice_rows(bounds[i], bounds[i + 1] - bounds[i], device=devs[i]) for i in range(4)]
        group = ShardGroup(shards)
        for topn in (0, 10, 300):
            a, b = whole.explain(q, ids, topn=topn), group.explain(q, ids, topn=topn)
            for x, y in zip(a, b):
                assert x.shape == y.shape and (np.asarray(x).view(np.uint32) == np.asarray(y).view(np.uint32)).all(), (devs, topn)
        a, b = whole.explain(None, ids, topn=50), group.explain(None, ids, topn=50)
        for x, y in zip(a, b):
            assert (np.asarray(x).view(np.uint32) == np.asarray(y).view(np.uint32)).all(), (devs, "disentangle")
        # device tensors in and out (first shard's device)
        dq, di = torch.from_numpy(q).to(f"cuda:{devs[0]}"), torch.from_numpy(ids).to(f"cuda:{devs[0]}")
        c = group.explain(dq, di, topn=10)
        for x, y in zip(whole.explain(q, ids, topn=10), c):
            assert (np.asarray(x).view(np.uint32) == y.cpu().numpy().view(np.uint32)).all()
        group.close()


def test_device_tensors_on_a_side_stream():
    n, B, k = 20000, 64, 100
    ip, ix, d = oracle.synth_csr(21, 0, n, V, 768)
    q = oracle.synth_queries(4, B)
    idx = DeviceIndex.from_csr(ip, ix, d, V)
    ids, _ = map(np.asarray, idx.search(q, k))
    want = idx.explain(q, ids, topn=10)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dq = torch.from_numpy(q).cuda()
        di = torch.from_numpy(ids).cuda()
        ex = idx.explain(dq, di, topn=10)
        for t in ex:
            assert t.is_cuda
    s.synchronize()
    for x, y in zip(want, ex):
        assert (np.asarray(x).view(np.uint32) == y.cpu().numpy().view(np.uint32)).all()


def test_disentangle_matches_the_rows():
    from vsearch_amd.ir import BoTIndex, SparseIndex
    n = 4000
    ip, ix, d = oracle.synth_csr(8, 0, n, V, 768)
    rng = np.random.default_rng(3)
    ids = rng.integers(0, n, (5, 7)).astype(np.int64)
    idx = DeviceIndex.from_csr(ip, ix, d, V)
    eip, eix, ed = idx.export_csr()
    want = _oracle(eip, eix, ed, None, ids, 64)
    g_sc = _check(idx.explain(None, ids, topn=64), want, "valued")
    assert (g_sc == want[3].astype(np.float32)).all()
    # the facade: SparseIndex / BoTIndex.disentangle, columns + shift
    sp = SparseIndex(device="cuda:0", shift=7)
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(d), size=(n, V))
    sp.move_to_device("cuda:0")
    ex = sp.disentangle(torch.from_numpy(ids), topn=64)
    cols = ex.cols.cpu().numpy()
    assert (np.where(want[0] >= 0, want[0] + 7, -1) == cols).all()
    ipb, ixb, _ = oracle.synth_csr(5, 0, n, V, 86, synth.KIND_BOT)
    bot = BoTIndex(device="cuda:0")
    bot.vector = torch.sparse_csr_tensor(torch.from_numpy(ipb), torch.from_numpy(ixb.astype(np.int64)),
                                         torch.ones(ixb.size, dtype=torch.float32), size=(n, V))
    bot.move_to_device("cuda:0")
    ex = bot.disentangle(torch.from_numpy(ids), topn=200)
    wb = _oracle(ipb, ixb, None, None, ids, 200)
    assert (ex.cols.cpu().numpy() == wb[0]).all() and (ex.n_matched.cpu().numpy() == wb[2]).all()
    assert (ex.contrib.cpu().numpy()[wb[0] >= 0] == 1).all()


def test_retriever_explain_results(tiny_retriever):
    from vsearch_amd.ir.retriever.index import IndexType
    r = tiny_retriever
    texts = make_texts(60, 5)
    r.build_index(texts, index_type=IndexType.SPARSE)
    queries = make_texts(3, 9)
    res = r.retrieve(queries, k=5)
    out = r.explain_results(queries, res, topn=1024)
    q_emb = r.process_query(queries).float().cpu().numpy()
    ip, ix, d = r.index._device_index().export_csr()
    shift = r.encoder_p.config.shift_vocab_num
    ids = res.ids.cpu().numpy()
    sc = res.scores.cpu().numpy()
    assert len(out) == 3 and all(len(row) == 5 for row in out)
    for b in range(3):
        for j in range(5):
            c, v = _row_terms(ip, ix, d, int(ids[b, j]))
            prod = (q_emb[b, c] * v).astype(np.float32)
            m = prod != 0
            order = np.lexsort((c[m], -prod[m].astype(np.float64)))
            want = {f"tok{int(x) + shift}": float(y) for x, y in zip(c[m][order], prod[m][order])}
            assert list(out[b][j].items()) == list(want.items()), (b, j)
            assert np.float32(sum(np.float64(x) for x in out[b][j].values())) == sc[b, j]


def test_argument_errors():
    idx = DeviceIndex.from_csr(*oracle.synth_csr(1, 0, 500, V, 768), V)
    q = oracle.synth_queries(1, 2)
    ids = np.zeros((2, 3), np.int64)
    for topn in (-1, 1025):
        with pytest.raises(ValueError):
            idx.explain(q, ids, topn=topn)
    with pytest.raises(TypeError):
        idx.explain(q, ids, topn=2.5)
    with pytest.raises(ValueError):
        idx.explain(q, ids[0], topn=1)                                  # ids must be [B, k]
    with pytest.raises(ValueError):
        idx.explain(q, np.zeros((3, 3), np.int64), topn=1)               # B mismatch
    with pytest.raises(TypeError):
        idx.explain(q, ids.astype(np.int32), topn=1)
    with pytest.raises(ValueError):
        idx.explain(torch.from_numpy(q).cuda(), ids, topn=1)            # device queries, host ids
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            idx.explain(torch.from_numpy(q).to("cuda:1"), torch.from_numpy(ids).to("cuda:1"), topn=1)
    ex = idx.explain(q, np.zeros((2, 0), np.int64), topn=3)              # k = 0: empty results
    assert ex.scores.shape == (2, 0) and ex.cols.shape == (2, 0, 3)
