"""GPU tests of query by example (vs_index_get_rows, vs_index_queries_from_rows, vs_topk_exclude and the shard-group versions;
DeviceIndex / ShardGroup .get_rows / .queries_from_rows / .search_by_example, Index.get_vectors / .queries_from_rows /
.search_by_example, Retriever.more_like_this / .retrieve_with_feedback) -- run on MI355X.

The contract: get_rows returns the export_csr rows bit for bit; queries_from_rows equals a float32 numpy loop bit for bit
(acc = fl32(alpha * q), then acc[c] = fl32(acc[c] + fl32(w * v)) row after row); search_by_example(exclude=True) equals the exact search
under a per-query deny filter of the example ids."""
import numpy as np
import pytest
import torch

import oracle
from oracle.compare import compare_topk
from conftest import V
from vsearch_amd import synth
from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, ShardGroup
from vsearch_amd.doc_filter import DocFilter
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

pytestmark = pytest.mark.gpu

# the forced paths of tests/test_gpu_explain.py
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


def _opts(idx, opts):
    for name, value in opts.items():
        if name == "queries_per_pass":
            idx.set_queries_per_pass(value)
        else:
            idx.set_option(name, value)
    return idx


def _row(rows, r):
    ip, ix, d = rows
    c = ix[ip[r]:ip[r + 1]].astype(np.int64)
    v = np.ones(c.size, np.float32) if d is None else d[ip[r]:ip[r + 1]].astype(np.float32)
    return c, v


def _want_rows(rows, ids):
    ptr, cols, vals = [0], [], []
    for r in ids:
        c, v = _row(rows, int(r)) if r >= 0 else (np.zeros(0, np.int64), np.zeros(0, np.float32))
        cols.append(c)
        vals.append(v)
        ptr.append(ptr[-1] + c.size)
    return np.asarray(ptr, np.int64), np.concatenate(cols).astype(np.int32), np.concatenate(vals).astype(np.float32)


def _check_rows(got, want, label):
    g = [np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t) for t in got]
    assert (g[0] == want[0]).all(), (label, "indptr")
    assert g[1].dtype == np.int32 and (g[1] == want[1]).all(), (label, "indices")
    assert g[2].dtype == np.float32 and (g[2].view(np.uint32) == want[2].view(np.uint32)).all(), (label, "values")


def _oracle_q(rows, ids, w=None, q=None, alpha=1.0):
    """the numerics contract, in float32 numpy"""
    B, m = ids.shape
    out = np.zeros((B, V), np.float32) if q is None else (np.float32(alpha) * q.astype(np.float32)).astype(np.float32)
    for b in range(B):
        for j in range(m):
            r = int(ids[b, j])
            if r < 0:
                continue
            c, v = _row(rows, r)
            wj = np.float32(1.0) if w is None else np.float32(w[b, j])
            out[b, c] = (out[b, c] + (wj * v).astype(np.float32)).astype(np.float32)
    return out


def _bits_equal(a, b):
    a = np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a)
    b = np.asarray(b.cpu() if isinstance(b, torch.Tensor) else b)
    return a.shape == b.shape and (a.view(np.uint32 if a.dtype == np.float32 else a.dtype) == b.view(np.uint32 if b.dtype == np.float32 else b.dtype)).all()


def _example_ids(rng, n, B, m, pad=True):
    ids = rng.integers(0, n, (B, m)).astype(np.int64)
    if m > 1:
        ids[:, 1] = ids[:, 0]                                                   # duplicates
    if pad and m > 2:
        ids[::3, -1] = -1                                                       # padding
    return ids


# ---- rows ----------------------------------------------------------------------------------------------------------------------------
def test_get_rows_equals_export_csr_on_every_kind():
    rng = np.random.default_rng(1)
    n = 5000
    ip, ix, d = oracle.synth_csr(3, 0, n, V, 200, synth.KIND_VDR)
    ipb, ixb, _ = oracle.synth_csr(5, 0, n, V, 86, synth.KIND_BOT)
    ids = np.concatenate([rng.integers(0, n, 300), [-1, 0, n - 1, 7, 7, -1]]).astype(np.int64)
    cases = {
        "fp32": DeviceIndex.from_csr(ip, ix, d, V),
        "fp16": DeviceIndex.from_csr(ip, ix, d.astype(np.float16), V),
        "binary": DeviceIndex.from_csr(ipb, ixb, None, V),
        "synthetic": DeviceIndex.synthetic(7, 0, n, V, 300),
    }
    # reserved + appended in two blocks
    pk = int(((ip[1:] - ip[:-1] + 7) // 8).sum())
    res = DeviceIndex.reserved(n, pk + 16, V, nat.VS_F32)
    h = n // 2 + 3
    res.append_csr(ip[:h + 1], ix[:ip[h]], d[:ip[h]])
    res.append_csr(ip[h:] - ip[h], ix[ip[h]:], d[ip[h]:])
    cases["reserved+appended"] = res
    for name, idx in cases.items():
        rows = idx.export_csr()
        if name == "binary":
            rows = (rows[0], rows[1], None)
        _check_rows(idx.get_rows(ids), _want_rows(rows, ids), name)
        di = torch.from_numpy(ids).cuda()
        got = idx.get_rows(di)
        assert all(t.is_cuda for t in got)
        _check_rows(got, _want_rows(rows, ids), (name, "device"))
    # out of range: ValueError (VS_EINVAL), nothing else; empty id list
    for bad in ([n], [-2], [3, n + 10]):
        with pytest.raises(ValueError):
            cases["fp32"].get_rows(np.asarray(bad, np.int64))
    e = cases["fp32"].get_rows(np.zeros(0, np.int64))
    assert e[0].tolist() == [0] and e[1].size == 0


def test_get_rows_dense_mfma_and_logical_dense():
    rng = np.random.default_rng(2)
    n = 300
    mat = np.where(rng.random((n, V)) < 0.3, rng.random((n, V)), 0).astype(np.float32)
    mat[5] = 0.0                                                                # an empty row
    dense = DeviceIndex.from_dense(mat)
    assert dense.info().n_packets == 0
    logical = DeviceIndex.from_dense(mat, max_density=1.0)
    assert logical.info().n_packets > 0
    rows = (np.concatenate([[0], np.cumsum((mat != 0).sum(1))]).astype(np.int64), np.nonzero(mat)[1].astype(np.int64), mat[mat != 0])
    ids = np.asarray([0, 5, -1, 299, 17, 17, 100], np.int64)
    for name, idx in (("mfma", dense), ("logical-dense", logical)):
        _check_rows(idx.get_rows(ids), _want_rows(rows, ids), name)
        w = rng.random((3, 4)).astype(np.float32)
        qi = rng.integers(-1, n, (3, 4)).astype(np.int64)
        assert _bits_equal(idx.queries_from_rows(qi, weights=w), _oracle_q(rows, qi, w)), name


# ---- queries -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", [nat.VS_F32, nat.VS_F16, nat.VS_NONE])
def test_queries_from_rows_equal_the_numpy_oracle(store):
    rng = np.random.default_rng(4)
    n = 8000
    if store == nat.VS_NONE:
        ip, ix, _ = oracle.synth_csr(5, 0, n, V, 86, synth.KIND_BOT)
        idx = DeviceIndex.from_csr(ip, ix, None, V)
    else:
        ip, ix, d = oracle.synth_csr(6, 0, n, V, 768)
        idx = DeviceIndex.from_csr(ip, ix, d.astype(np.float16) if store == nat.VS_F16 else d, V)
    rows = idx.export_csr()
    if store == nat.VS_NONE:
        rows = (rows[0], rows[1], None)
    for B, m in ((5, 1), (9, 7), (4, 64), (1024, 2)):
        ids = _example_ids(rng, n, B, m)
        w = (rng.standard_normal((B, m)) * 0.3).astype(np.float32)
        q = oracle.synth_queries(B + m, B)
        assert _bits_equal(idx.queries_from_rows(ids), _oracle_q(rows, ids)), (B, m, "plain")
        assert _bits_equal(idx.queries_from_rows(ids, weights=w), _oracle_q(rows, ids, w)), (B, m, "weights")
        got = idx.queries_from_rows(ids, weights=w, q=q, alpha=0.37)
        assert _bits_equal(got, _oracle_q(rows, ids, w, q, 0.37)), (B, m, "alpha q fp32")
        q16 = q.astype(np.float16)
        got = idx.queries_from_rows(ids, weights=w, q=q16, alpha=-1.5)
        assert _bits_equal(got, _oracle_q(rows, ids, w, q16, -1.5)), (B, m, "alpha q fp16")
    # all padding: alpha * q only
    ids = np.full((3, 4), -1, np.int64)
    q = oracle.synth_queries(1, 3)
    assert _bits_equal(idx.queries_from_rows(ids, q=q, alpha=2.0), (np.float32(2.0) * q).astype(np.float32))


# ---- search and exclusion --------------------------------------------------------------------------------------------------------
def test_search_by_example_without_exclusion_is_the_plain_search():
    rng = np.random.default_rng(5)
    n, B, k = 20000, 16, 50
    ip, ix, d = oracle.synth_csr(9, 0, n, V, 768)
    idx = DeviceIndex.from_csr(ip, ix, d, V)
    ids = _example_ids(rng, n, B, 3)
    w = rng.random((B, 3)).astype(np.float32)
    got = idx.search_by_example(ids, k, weights=w, exclude=False)
    qq = idx.queries_from_rows(ids, weights=w)
    want = idx.search(qq, k)
    assert _bits_equal(got[0], want[0]) and _bits_equal(got[1], want[1])
    o_ids, o_sc = oracle.csr_search(ip, ix, d, V, qq, k, acc64=True)
    compare_topk(o_ids, o_sc, np.asarray(got[0]), np.asarray(got[1]), rtol=1e-4)
    # the query's own row is its best hit; with exclusion it is gone
    one = ids[:, :1]
    assert (np.asarray(idx.search_by_example(one, 5, exclude=False)[0])[:, 0] == one[:, 0]).all()
    assert not (np.asarray(idx.search_by_example(one, 5)[0]) == one).any()


def _deny(ids, n, allowed=None):
    mask = np.ones((ids.shape[0], n), bool) if allowed is None else np.repeat(allowed[None, :], ids.shape[0], 0)
    for b in range(ids.shape[0]):
        mask[b, ids[b][ids[b] >= 0]] = False
    return DocFilter.from_mask(torch.from_numpy(mask))


@pytest.mark.parametrize("kind", ["valued", "binary"])
def test_exclusion_equals_the_exact_deny_filter_on_every_path(kind):
    rng = np.random.default_rng(6)
    n, B, k = 20000, 12, 40
    if kind == "valued":
        ip, ix, d = oracle.synth_csr(12, 0, n, V, 768)
        paths = VALUED_PATHS
    else:
        ip, ix, _ = oracle.synth_csr(13, 0, n, V, 86, synth.KIND_BOT)
        d = None
        paths = BINARY_PATHS
    ids = _example_ids(rng, n, B, 5)
    for path, opts in paths.items():
        idx = _opts(DeviceIndex.from_csr(ip, ix, d, V), opts)
        qq = idx.queries_from_rows(ids)
        got = idx.search_by_example(ids, k)
        want = idx.search(qq, k, filter=DocFilter.from_ids(torch.from_numpy(ids), n, allow=False))
        assert _bits_equal(got[0], want[0]) and _bits_equal(got[1], want[1]), path
        # with a user filter on top
        allowed = rng.random(n) < 0.5
        got = idx.search_by_example(ids, k, filter=DocFilter.from_mask(torch.from_numpy(allowed)))
        want = idx.search(qq, k, filter=_deny(ids, n, allowed))
        assert _bits_equal(got[0], want[0]) and _bits_equal(got[1], want[1]), (path, "user filter")


def test_exclusion_dense_index_and_fewer_than_k_survivors():
    rng = np.random.default_rng(7)
    n, B, k = 400, 6, 30
    mat = np.where(rng.random((n, V)) < 0.2, rng.random((n, V)), 0).astype(np.float32)
    idx = DeviceIndex.from_dense(mat)
    ids = _example_ids(rng, n, B, 4)
    got = idx.search_by_example(ids, k)
    want = idx.search(idx.queries_from_rows(ids), k, filter=DocFilter.from_ids(torch.from_numpy(ids), n, allow=False))
    assert _bits_equal(got[0], want[0]) and _bits_equal(got[1], want[1])
    # a filter that leaves 5 rows, 2 of them examples: 3 survive, then padding
    ip, ix, d = oracle.synth_csr(14, 0, 3000, V, 768)
    sp = DeviceIndex.from_csr(ip, ix, d, V)
    allowed = np.zeros(3000, bool)
    allowed[[3, 9, 50, 51, 2999]] = True
    ex = np.array([[9, 50], [9, 50]], np.int64)
    g_ids, g_sc = map(np.asarray, sp.search_by_example(ex, 10, filter=DocFilter.from_mask(torch.from_numpy(allowed))))
    assert set(g_ids[0, :3].tolist()) == {3, 51, 2999} and (g_ids[:, 3:] == -1).all() and np.isneginf(g_sc[:, 3:]).all()
    # k + m beyond the index: everything but the examples, padded
    small = DeviceIndex.from_csr(ip[:9], ix[:ip[8]], d[:ip[8]], V)
    g_ids, _ = map(np.asarray, small.search_by_example(np.array([[0, 1]], np.int64), 8))
    assert sorted(g_ids[0, :6].tolist()) == list(range(2, 8)) and (g_ids[0, 6:] == -1).all()


def test_resparsify_equals_the_oracle_mask():
    rng = np.random.default_rng(8)
    n, B, k, a = 20000, 8, 50, 768
    ip, ix, d = oracle.synth_csr(15, 0, n, V, 768)
    idx = DeviceIndex.from_csr(ip, ix, d, V)
    rows = idx.export_csr()
    ids = _example_ids(rng, n, B, 10, pad=False)
    qo = _oracle_q(rows, ids)
    assert ((qo != 0).sum(1) > a).all()
    qm = np.where(oracle.topk_mask(qo, a), qo, np.float32(0))
    for exclude in (False, True):
        got = idx.search_by_example(ids, k, a=a, exclude=exclude)
        if exclude:
            want = idx.search(qm, k, filter=DocFilter.from_ids(torch.from_numpy(ids), n, allow=False))
        else:
            want = idx.search(qm, k)
        assert _bits_equal(got[0], want[0]) and _bits_equal(got[1], want[1]), exclude
    with pytest.raises(ValueError):
        idx.search_by_example(ids, k, a=V + 1)


# ---- shard groups and streams ----------------------------------------------------------------------------------------------------
def test_shard_groups_equal_unsharded():
    rng = np.random.default_rng(9)
    n, B, k = 20000, 10, 40
    ip, ix, d = oracle.synth_csr(16, 0, n, V, 768)
    whole = DeviceIndex.from_csr(ip, ix, d, V)
    ids = _example_ids(rng, n, B, 6)
    ids[0, 2], ids[1, 2], ids[2, 2] = 0, n - 1, 6001
    flat = ids.ravel()
    w = rng.random((B, 6)).astype(np.float32)
    q = oracle.synth_queries(3, B).astype(np.float16)
    want_rows = whole.get_rows(flat)
    want_q = whole.queries_from_rows(ids, weights=w, q=q, alpha=0.5)
    want_s = whole.search_by_example(ids, k, weights=w)
    ngpu = torch.cuda.device_count()
    layouts = [([0, 6001, n], [0, 0]), ([0, 6001, 13337, n], [0, 0, 0])]
    if ngpu > 1:
        layouts.append(([0, 6001, 13337, n], [i % ngpu for i in range(3)]))
    for bounds, devs in layouts:
        shards = [whole.slice_rows(bounds[i], bounds[i + 1] - bounds[i], device=devs[i]) for i in range(len(devs))]
        group = ShardGroup(shards)
        got = group.get_rows(flat)
        assert all(_bits_equal(x, y) for x, y in zip(got, want_rows)), devs
        assert _bits_equal(group.queries_from_rows(ids, weights=w, q=q, alpha=0.5), want_q), devs
        got = group.search_by_example(ids, k, weights=w)
        assert _bits_equal(got[0], want_s[0]) and _bits_equal(got[1], want_s[1]), devs
        # device tensors in and out
        dev = f"cuda:{devs[0]}"
        got = group.queries_from_rows(torch.from_numpy(ids).to(dev), weights=torch.from_numpy(w).to(dev), q=torch.from_numpy(q).to(dev), alpha=0.5)
        assert got.is_cuda and _bits_equal(got, want_q)
        got = group.get_rows(torch.from_numpy(flat).to(dev))
        assert all(_bits_equal(x, y) for x, y in zip(got, want_rows))
        with pytest.raises(ValueError):
            group.get_rows(np.array([n], np.int64))
        group.close()


def test_device_tensors_on_a_side_stream():
    rng = np.random.default_rng(10)
    n, B, k = 20000, 64, 100
    ip, ix, d = oracle.synth_csr(17, 0, n, V, 768)
    idx = DeviceIndex.from_csr(ip, ix, d, V)
    ids = _example_ids(rng, n, B, 4)
    w = rng.random((B, 4)).astype(np.float32)
    want_q = idx.queries_from_rows(ids, weights=w)
    want_s = idx.search_by_example(ids, k, weights=w, a=500)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        di, dw = torch.from_numpy(ids).cuda(), torch.from_numpy(w).cuda()
        got_q = idx.queries_from_rows(di, weights=dw)
        got_s = idx.search_by_example(di, k, weights=dw, a=500)
        assert got_q.is_cuda and got_s[0].is_cuda
    s.synchronize()
    assert _bits_equal(got_q, want_q)
    assert _bits_equal(got_s[0], want_s[0]) and _bits_equal(got_s[1], want_s[1])


# ---- facade -------------------------------------------------------------------------------------------------------------------------
def test_facade_get_vectors_and_search_by_example():
    from vsearch_amd.ir import BoTIndex, Index, SparseIndex
    rng = np.random.default_rng(11)
    n = 600
    ip, ix, d = oracle.synth_csr(18, 0, n, V, 300)
    ids = torch.tensor([3, 0, n - 1, 3, -1, 77])
    real = ids.clamp(min=0)
    for fp16 in (False, True):
        sp = SparseIndex(device="cuda:0")
        vals = torch.from_numpy(d).to(torch.float16 if fp16 else torch.float32)
        sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), vals, size=(n, V))
        sp.move_to_device("cuda:0")
        gv = sp.get_vectors(ids)
        assert gv.layout == torch.sparse_csr and gv.dtype == vals.dtype and tuple(gv.shape) == (6, V)
        want = sp.vector.to_dense()[real]
        want[4] = 0
        assert torch.equal(gv.to_dense(), want), fp16
        ex = torch.from_numpy(rng.integers(0, n, (5, 3)))
        r1 = sp.search_by_example(ex, 10, exclude=False)
        r2 = sp.search(sp.queries_from_rows(ex), 10)
        assert torch.equal(r1.ids, r2.ids) and torch.equal(r1.scores, r2.scores) and r1.scores.dtype == sp._dtype
        for bad in ([[n]], [[-2]]):
            with pytest.raises(IndexError):
                sp.search_by_example(torch.tensor(bad), 3)
        with pytest.raises(IndexError):
            sp.get_vectors(torch.tensor([n]))
        # devices=: the shard group path (two row shards on one GPU)
        want_s = sp.search_by_example(ex, 10)
        sp.shard_rows([0, 0])
        assert sp.shards is not None and len(sp.shards) == 2
        assert torch.equal(sp.get_vectors(ids).to_dense(), want)
        got_s = sp.search_by_example(ex, 10)
        assert torch.equal(got_s.ids, want_s.ids) and torch.equal(got_s.scores, want_s.scores)
    ipb, ixb, _ = oracle.synth_csr(19, 0, n, V, 86, synth.KIND_BOT)
    bot = BoTIndex(device="cuda:0")
    bot.vector = torch.sparse_csr_tensor(torch.from_numpy(ipb), torch.from_numpy(ixb.astype(np.int64)), torch.ones(ixb.size), size=(n, V))
    bot.move_to_device("cuda:0")
    want = bot.vector.to_dense()[real].float()
    want[4] = 0
    assert torch.equal(bot.get_vectors(ids).to_dense().float(), want)
    mat = torch.from_numpy(np.where(rng.random((n, V)) < 0.2, rng.random((n, V)), 0).astype(np.float32))
    dense = Index(device="cuda:0")
    dense.vector = mat
    dense.move_to_device("cuda:0")
    gv = dense.get_vectors(ids)
    want = mat[real].clone()
    want[4] = 0
    assert gv.layout == torch.strided and torch.equal(gv.cpu(), want)


def test_retriever_more_like_this_and_feedback(tiny_retriever):
    from vsearch_amd.ir.retriever.index import IndexType
    from vsearch_amd.ir.utils import sparse as sp
    r = tiny_retriever
    texts = make_texts(80, 5)
    r.build_index(texts, index_type=IndexType.SPARSE)
    idx = r.index
    ids = torch.tensor([0, 5, 17])
    got = r.more_like_this(ids, k=4)
    want = idx.search_by_example(ids.unsqueeze(1), 4)
    assert torch.equal(got.ids, want.ids) and torch.equal(got.scores, want.scores)
    assert not (got.ids.cpu() == ids.unsqueeze(1)).any()
    queries = make_texts(3, 9)
    a = r.encoder_q.config.topk
    q = r.process_query(queries)
    for fb_weight in (0.75, 0.0):
        got = r.retrieve_with_feedback(queries, k=5, fb_docs=4, fb_weight=fb_weight)
        first = idx.search(q, k=4)
        m_b = (first.ids >= 0).sum(1, keepdim=True).clamp(min=1).double()
        w = (fb_weight / m_b).float().expand(first.ids.shape).contiguous()
        q2 = idx.queries_from_rows(first.ids, weights=w, q=q)
        q2 = q2.masked_fill(~sp.build_topk_mask(q2, k=a), 0.0)
        want = idx.search(q2, k=5)
        assert torch.equal(got.ids, want.ids) and torch.equal(got.scores, want.scores), fb_weight
        if fb_weight == 0.0:
            plain = idx.search(q.float().masked_fill(~sp.build_topk_mask(q.float(), k=a), 0.0), k=5)
            assert torch.equal(got.ids, plain.ids) and torch.equal(got.scores, plain.scores)
