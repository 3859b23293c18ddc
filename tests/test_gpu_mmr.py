"""GPU tests of diversified search (vs_mmr_select_csr; DeviceIndex / ShardGroup .search_diverse / .diversify, Index.search_diverse /
.diversify, Retriever.retrieve_diverse) -- run on MI355X.

The contract is tests/_mmr_ref.py.  Everything compares BITS -- ids, pos, and view(uint32) of scores, mmr and pen -- which
the inputs entitle the tests to: rows of values m / 256 have exact fp64 sums in any order (tests/test_mmr_cpu.py proves it).  The one
exception is the generic-values test at the end, with its stated tolerance."""
import itertools

import numpy as np
import pytest
import torch

from conftest import V
from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, DiverseResults, ShardGroup, _search_diverse, mmr_select
from vsearch_amd.doc_filter import DocFilter
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

import _mmr_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
OUT_DTYPES = (np.int64, np.float32, np.int32, np.float32, np.float32)
JUNK = (77, 1.5, 9, -2.5, 3.25)


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _junk(B, k, on_dev):
    out = tuple(np.full((B, k), v, dtype=dt) for v, dt in zip(JUNK, OUT_DTYPES))
    return tuple(torch.from_numpy(o).cuda() for o in out) if on_dev else out


def _run(c, k, lam, mode, on_dev, n_cols=V):
    """vs_mmr_select_csr over a case, into output buffers filled with junk -> dict of numpy arrays"""
    args = [c[n] for n in ("indptr", "indices", "values", "ids", "scores")]
    if on_dev:
        args = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
    B = c["ids"].shape[0]
    out = mmr_select(*args, k, lam, mode, n_cols, 0, out=_junk(B, k, on_dev))
    return dict(zip(ref.NAMES, (_np(o) for o in out)))


def _want(c, k, lam, mode, n_cols=V):
    return ref.select(c["ids"], c["scores"], c["indptr"], c["indices"], c["values"], n_cols, lam, k, mode)


LAMS = (0.0, 0.3, 0.5, 1.0, "per-query")


# ---- the kernel alone -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kk", [1, 2, 15, 16, 17, 63, 64, 65, 300, 1024])
def test_kernel_equals_the_reference(kk):
    B = 2 if kk == 1024 else 3
    n_cols = 32768 if kk in (17, 65) else V
    c = ref.kernel_case(kk, n_cols, kk, B=B)
    assert {0, n_cols - 1} <= set(c["indices"].tolist()) or kk < 3
    ks = [k for k in (1, kk, kk + 3) if k <= 1024]
    per_query = np.linspace(0, 1, B).astype(F32)
    for i, (mode, lam) in enumerate(itertools.product(("cosine", "dot"), LAMS)):
        k = ks[i % len(ks)] if kk > 100 else None                               # (long lists: one k a combination keeps the numpy reference quick)
        lam = per_query if lam == "per-query" else lam
        for k in ([k] if k else ks):
            want = _want(c, k, lam, mode, n_cols)
            for on_dev in (False, True):
                ref.assert_equal_bits(_run(c, k, lam, mode, on_dev, n_cols), want, (kk, mode, lam, k, on_dev))
    if kk == 1024:
        assert 1024 in ks and (_want(c, 1024, 0.5, "cosine")["pos"] >= 0).all()    # k = kk = 1024: every candidate picked


def _rows_of(c):
    rp, ix, va = c["indptr"], c["indices"], c["values"]
    return [(ix[rp[r]:rp[r + 1]], va[rp[r]:rp[r + 1]]) for r in range(rp.shape[0] - 1)]


def _with_rows(c, rows):
    rp = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(x) for x, _ in rows], out=rp[1:])
    return dict(c, indptr=rp, indices=np.concatenate([x for x, _ in rows]).astype(np.int32), values=np.concatenate([v for _, v in rows]).astype(F32))


def test_kernel_on_padding_single_twins_and_repeated_ids():
    kk = 16
    c = ref.kernel_case(kk, V, 41, B=5)
    ids, rows = c["ids"].copy(), _rows_of(c)
    ids[0, :] = -1                                                              # an all-padding list
    ids[1, 1:] = -1                                                             # a single candidate
    ids[2, 8] = -1                                                              # padded from the middle: 9 .. 15 are ignored although they hold ids
    long_row = max(rows[3 * kk:4 * kk], key=lambda r: len(r[0]))
    for j in (2, 5, 9):                                                         # three identical rows
        rows[3 * kk + j] = long_row
    ids[4, 10] = ids[4, 3]                                                      # the same id twice (two candidates all the same)
    c = _with_rows(dict(c, ids=ids), rows)
    for mode, lam, k in (("cosine", 0.5, kk), ("dot", 0.3, kk + 3), ("cosine", 0.0, 4)):
        want = _want(c, k, lam, mode)
        assert (want["ids"][0] == -1).all() and (want["pos"][1, 1:] == -1).all() and (want["pos"][2] < 8).all()
        if mode == "cosine" and k >= kk:
            twins = np.isin(want["pos"][3], (2, 5, 9))
            assert twins.sum() == 3 and (want["pen"][3][twins] == 1).sum() == 2  # the second and third twin carry similarity exactly 1
            assert (want["ids"][4] == ids[4, 3]).sum() == 2
        for on_dev in (False, True):
            ref.assert_equal_bits(_run(c, k, lam, mode, on_dev), want, (mode, lam, k, on_dev))


def test_image_is_clean_between_steps_and_queries():
    c = ref.kernel_case(64, V, 7, B=3)
    dev = {n: torch.from_numpy(np.ascontiguousarray(c[n])).cuda() for n in ("indptr", "indices", "values", "ids", "scores")}
    call = lambda d, B: mmr_select(d["indptr"], d["indices"], d["values"], d["ids"], d["scores"], 40, 0.4, "cosine", V, 0, out=_junk(B, 40, True))
    first, second = call(dev, 3), call(dev, 3)                                  # twice on one stream
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    want = _want(c, 40, 0.4, "cosine")
    ref.assert_equal_bits(dict(zip(ref.NAMES, (_np(o) for o in first))), want, "batch")
    for b in range(3):                                                          # and query by query
        rp = dev["indptr"][b * 64:(b + 1) * 64 + 1]
        one = dict(indptr=rp, indices=dev["indices"], values=dev["values"], ids=dev["ids"][b:b + 1], scores=dev["scores"][b:b + 1])
        for a, w in zip(call(one, 1), first):
            assert torch.equal(a[0], w[b]), b


def test_kernel_rejects_what_it_cannot_take():
    c = ref.kernel_case(8, V, 3, B=2)
    lib = nat.lib()
    lam = np.full(2, 0.5, dtype=F32)
    out = _junk(2, 4, False)

    def call(n_cols=V, kk=8, k=4, indices=c["indices"], indptr=c["indptr"], lam=lam, mode=0):
        return lib.vs_mmr_select_csr(indptr.ctypes.data, indices.ctypes.data, c["values"].ctypes.data, c["ids"].ctypes.data, c["scores"].ctypes.data,
                                     2, kk, kk, n_cols, lam.ctypes.data, k, mode, *[o.ctypes.data for o in out], 0, None)
    bad_col, bad_rp = c["indices"].copy(), c["indptr"].copy()
    bad_col[-1] = V
    bad_rp[5] = bad_rp[4] - 1
    for kw, exc in ((dict(n_cols=32769), NotImplementedError), (dict(kk=1025), ValueError), (dict(k=0), ValueError), (dict(k=1025), ValueError),
                    (dict(indices=bad_col), ValueError), (dict(indptr=bad_rp), ValueError), (dict(lam=np.array([0.5, 1.5], dtype=F32)), ValueError),
                    (dict(mode=2), ValueError)):
        with pytest.raises(exc):
            nat.check(call(**kw))
        for o, v in zip(out, JUNK):                                             # nothing is written
            assert (o == v).all(), kw
    assert "32768" in _err(lambda: nat.check(call(n_cols=32769))) and "outside" in _err(lambda: nat.check(call(indices=bad_col)))
    assert call() == nat.VS_OK and not (out[2] == 9).any()
    with pytest.raises(ValueError, match="host or all"):                        # host lists, device rows
        mmr_select(torch.from_numpy(c["indptr"]).cuda(), torch.from_numpy(c["indices"]).cuda(), torch.from_numpy(c["values"]).cuda(),
                   torch.from_numpy(c["ids"]).cuda(), torch.from_numpy(c["scores"]).cuda(), 4, 0.5, "cosine", V, 0, out=out)


def _err(fn):
    try:
        fn()
    except Exception as e:
        return str(e)
    return ""


def test_device_columns_outside_the_vocabulary_are_skipped():
    c = ref.kernel_case(16, V, 12, B=2)
    ix = c["indices"].copy()
    rng = np.random.default_rng(0)
    hit = rng.permutation(ix.shape[0])[:40]
    ix[hit[:20]], ix[hit[20:30]], ix[hit[30:]] = V, -3, 2 ** 31 - 1
    bad = dict(c, indices=ix)
    rp, cols, vals = ref.drop_columns_outside(c["indptr"], ix, c["values"], V)
    assert rp[-1] == c["indptr"][-1] - 40
    for mode in ("cosine", "dot"):
        want = ref.select(c["ids"], c["scores"], rp, cols, vals, V, 0.5, 16, mode)
        ref.assert_equal_bits(_run(bad, 16, 0.5, mode, True), want, mode)


# ---- search_diverse, end to end -------------------------------------------------------------------------------------------------------------
_made = {}


def _index(kind):
    """-> (object with search / search_diverse, its DeviceIndex, n_cols); one per kind for the cases that do not change the index"""
    if kind not in _made:
        n_cols = ref.V_DENSE if kind == "dense" else V
        ip, ix, va = ref.e2e_rows(kind, n_cols)
        if kind in ("fp32", "fp16"):
            dev = DeviceIndex.from_csr(ip, ix, va, n_cols, store_dtype=nat.VS_F16 if kind == "fp16" else nat.VS_F32)
            _made[kind] = (dev, dev, n_cols)
        else:
            from vsearch_amd.ir import BoTIndex, Index
            if kind == "bot":
                idx = BoTIndex(device="cuda:0", fp16=False)
                idx.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(va), size=(ref.N_E2E, n_cols))
            else:
                mat = np.zeros((ref.N_E2E, n_cols), dtype=F32)
                mat[np.repeat(np.arange(ref.N_E2E), np.diff(ip)), ix] = va
                idx = Index(device="cuda:0")
                idx.vector = torch.from_numpy(mat)
            idx.move_to_device("cuda:0")
            info = idx._device_index().info()
            if kind == "bot":
                assert info.store_dtype == nat.VS_NONE
            else:
                assert info.kind == nat.VS_KIND_DENSE and info.n_packets == 0   # the dense index of the matrix cores, not dense-as-packets
            _made[kind] = (idx, idx._device_index(), n_cols)
    return _made[kind]


def _lists(obj, q, depth, flt=None):
    r = obj.search(q, depth, filter=flt) if flt is not None else obj.search(q, depth)
    return _np(r[0]), _np(r[1]).astype(F32)


def _expected(dev, ids, sc, n_cols, k, lam, mode):
    """the reference over a hit list and the rows the index exports for it"""
    rp, ix, va = dev.get_rows(np.ascontiguousarray(ids.reshape(-1)))
    return ref.select(ids, sc, rp, ix, va, n_cols, lam, k, mode)


def _res(r):
    return dict(ids=_np(r.ids), scores=_np(r.scores).astype(F32), pos=_np(r.pos), mmr=_np(r.mmr))


E2E_NAMES = ("ids", "scores", "pos", "mmr")


@pytest.mark.parametrize("kind", ["fp32", "fp16", "bot", "dense"])
def test_search_diverse_equals_the_reference(kind):
    obj, dev, n_cols = _index(kind)
    q = ref.e2e_queries(n_cols)
    k, depth = 10, 64
    ids, sc = _lists(obj, q, depth)
    assert (ids >= 0).all()
    lam_q = np.linspace(0.1, 0.9, ref.B_E2E).astype(F32)
    moved = 0
    for mode, lam in (("cosine", 0.5), ("dot", 0.7), ("cosine", lam_q)):
        want = _expected(dev, ids, sc, n_cols, k, lam, mode)
        got = obj.search_diverse(q, k, lam=lam, depth=depth, sim=mode)
        assert isinstance(got, DiverseResults)
        ref.assert_equal_bits(_res(got), want, (kind, mode), E2E_NAMES)
        moved += int((want["pos"] != np.arange(k)).sum())
    assert moved > 0                                                            # near-duplicates exist: MMR does reorder
    top_ids, top_sc = _lists(obj, q, k)                                         # lam = 1 is the plain search, bit for bit
    one = _res(obj.search_diverse(q, k, lam=1.0, depth=depth))
    assert (one["ids"] == top_ids).all() and (one["scores"].view(np.uint32) == top_sc.view(np.uint32)).all() and (one["pos"] == np.arange(k)).all()
    tq = torch.from_numpy(q).cuda()                                             # torch in -> torch out; the default depth max(4 k, k + 16) = 40
    got = obj.search_diverse(tq, k, lam=0.5)
    assert got.ids.is_cuda and got.ids.dtype == torch.int64 and got.pos.dtype == torch.int32
    i40, s40 = _lists(obj, q, 40)
    ref.assert_equal_bits(_res(got), _expected(dev, i40, s40, n_cols, k, 0.5, "cosine"), (kind, "default depth"), E2E_NAMES)


def test_search_diverse_under_a_filter_and_deletions():
    ip, ix, va = ref.e2e_rows("fp32", V)
    dev = DeviceIndex.from_csr(ip, ix, va, V)
    q = ref.e2e_queries(V)
    k, depth = 10, 48
    mask = np.random.default_rng(5).random(ref.N_E2E) < 0.5
    few = np.zeros(ref.N_E2E, dtype=bool)
    few[::97] = True                                                            # 21 rows allowed: the lists end in padding
    for allowed in (mask, few):
        flt = DocFilter.from_mask(torch.from_numpy(allowed))
        ids, sc = _lists(dev, q, depth, flt)
        assert allowed[ids[ids >= 0]].all() and ((ids == -1).any() or allowed is mask)
        got = _res(dev.search_diverse(q, k, lam=0.5, depth=depth, filter=flt))
        assert allowed[got["ids"][got["ids"] >= 0]].all()
        ref.assert_equal_bits(got, _expected(dev, ids, sc, V, k, 0.5, "cosine"), "filter", E2E_NAMES)
    dead = np.unique(_lists(dev, q, 5)[0])
    dev.delete_rows(dead)
    ids, sc = _lists(dev, q, depth)
    got = _res(dev.search_diverse(q, k, lam=0.5, depth=depth))
    assert not np.isin(got["ids"], dead).any() and not np.isin(ids, dead).any()
    ref.assert_equal_bits(got, _expected(dev, ids, sc, V, k, 0.5, "cosine"), "deleted", E2E_NAMES)
    dev.close()


def test_chunked_rows_equal_one_chunk():
    dev, _, _ = _index("fp32")
    q = ref.e2e_queries(V)
    k, depth = 12, 64
    whole, runs = [], []
    a = _search_diverse(dev, q, k, 0.5, depth, "cosine", None, None, whole)
    b = _search_diverse(dev, q, k, 0.5, depth, "cosine", None, 150_000, runs)                    # a query's 64 rows of 64 .. 200 non-zeros take 33 .. 102 KB: at most 4 a run
    c = _search_diverse(dev, q, k, 0.5, depth, "cosine", None, 1, runs)                       # never less than a query
    assert whole == [1] and 3 <= runs[0] <= ref.B_E2E and runs[1] == ref.B_E2E
    for x in (b, c):
        ref.assert_equal_bits(_res(x), _res(a), "chunks", E2E_NAMES)


def test_row_shards_equal_the_unsharded_index():
    whole, _, _ = _index("fp32")
    q = ref.e2e_queries(V)
    k, depth = 10, 64
    bounds = [0, 601, 1399, ref.N_E2E]
    shards = [whole.slice_rows(bounds[i], bounds[i + 1] - bounds[i], device=0) for i in range(3)]
    group = ShardGroup(shards)
    ids, _ = _lists(whole, q, depth)
    owners = np.searchsorted(bounds, ids, side="right")
    assert all(set(owners[b].tolist()) == {1, 2, 3} for b in range(ref.B_E2E))  # every list draws rows from all three shards
    for mode, lam in (("cosine", 0.5), ("dot", 0.3)):
        want = _res(whole.search_diverse(q, k, lam=lam, depth=depth, sim=mode))
        ref.assert_equal_bits(_res(group.search_diverse(q, k, lam=lam, depth=depth, sim=mode)), want, ("group", mode), E2E_NAMES)
        got = group.search_diverse(torch.from_numpy(q).cuda(), k, lam=lam, depth=depth, sim=mode, max_row_bytes=150_000)
        assert got.ids.is_cuda
        ref.assert_equal_bits(_res(got), want, ("group, torch, chunks", mode), E2E_NAMES)
    want = _res(whole.search_diverse(q, k, lam=0.5, depth=depth))
    group.close()
    from vsearch_amd.ir import SparseIndex
    ip, ix, va = ref.e2e_rows("fp32", V)
    sp = SparseIndex(device="cuda:0", fp16=False)
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(va), size=(ref.N_E2E, V))
    sp.move_to_device("cuda:0")
    tq = torch.from_numpy(q)
    ref.assert_equal_bits(_res(sp.search_diverse(tq, k, lam=0.5, depth=depth)), want, "facade", E2E_NAMES)
    sp.shard_rows([0, 0, 0])
    assert sp.shards is not None and len(sp.shards) == 3
    ref.assert_equal_bits(_res(sp.search_diverse(tq, k, lam=0.5, depth=depth)), want, "facade, row shards", E2E_NAMES)
    ref.assert_equal_bits(_res(sp.diversify(sp.search(tq, depth), k, lam=0.5)), want, "facade, diversify", E2E_NAMES)


def test_diversify_on_lists_the_caller_has():
    obj, dev, n_cols = _index("bot")
    q = ref.e2e_queries(n_cols)
    ids, sc = _lists(obj, q, 40)
    rng = np.random.default_rng(8)
    pad_ids, pad_sc = ids.copy(), sc.copy()                                     # trailing padding, of a different length a query
    for b in range(ref.B_E2E):
        pad_ids[b, 40 - 3 * b:], pad_sc[b, 40 - 3 * b:] = -1, -np.inf
    perm = rng.permutation(40)                                                  # a list in no canonical order (a reranker's)
    lists = {"padded": (pad_ids, pad_sc), "shuffled": (np.ascontiguousarray(ids[:, perm]), np.ascontiguousarray(sc[:, perm]))}
    for name, (i, s) in lists.items():
        for mode in ("cosine", "dot"):
            want = _expected(dev, i, s, n_cols, 20, 0.5, mode)
            ref.assert_equal_bits(_res(dev.diversify(i, s, 20, lam=0.5, sim=mode)), want, (name, mode, "numpy"), E2E_NAMES)
            got = obj.diversify((torch.from_numpy(i), torch.from_numpy(s)), 20, lam=0.5, sim=mode)
            ref.assert_equal_bits(_res(got), want, (name, mode, "facade"), E2E_NAMES)
    assert (_expected(dev, pad_ids, pad_sc, n_cols, 20, 0.5, "cosine")["ids"][7, 19:] == -1).all()     # 19 candidates, 20 asked for
    with pytest.raises(ValueError, match="1024"):
        dev.diversify(np.zeros((1, 1025), np.int64), np.zeros((1, 1025), F32), 5)
    with pytest.raises(ValueError, match="1024"):
        dev.search_diverse(q, 5, depth=1025)
    with pytest.raises(ValueError, match="smaller than k"):
        dev.search_diverse(q, 5, depth=4)
    with pytest.raises(IndexError):
        obj.diversify((np.full((1, 4), ref.N_E2E, np.int64), np.zeros((1, 4), F32)), 2)


def test_retriever_retrieve_diverse(tiny_retriever):
    from vsearch_amd.ir.retriever.index import IndexType
    r = tiny_retriever
    n = 80
    r.build_index(make_texts(n, 5), index_type=IndexType.SPARSE)
    idx = r.index
    queries = make_texts(4, 9)
    q_emb = r.process_query(queries, 0, r.encoder_q.config.topk)
    k = 6
    got = r.retrieve_diverse(queries, k=k, lam=0.4, depth=30)
    want = idx.search_diverse(q_emb, k, lam=0.4, depth=30)
    ref.assert_equal_bits(_res(got), _res(want), "retriever", E2E_NAMES)
    deep = r.retrieve(queries, k=30)
    dev = idx._device_index()
    exp = _expected(dev, _np(deep.ids), _np(deep.scores).astype(F32), int(dev.info().n_cols), k, 0.4, "cosine")
    ref.assert_equal_bits(_res(got), exp, "retriever, reference", E2E_NAMES)
    cols = _np(idx.get_vectors(torch.tensor([3])).col_indices())               # must=: the candidates are the documents with that term --
    df = _np(idx.doc_freq(cols))                                               # document 3's rarest term
    col = int(cols[df.argmin()])
    assert 0 < df.min() < n
    narrowed = r.retrieve_diverse(queries, k=k, lam=0.4, depth=30, must=[col])
    plain = _np(deep.ids)
    deep = r.retrieve(queries, k=30, must=[col])
    assert not np.array_equal(_np(deep.ids), plain)
    exp = _expected(dev, _np(deep.ids), _np(deep.scores).astype(F32), int(dev.info().n_cols), k, 0.4, "cosine")
    ref.assert_equal_bits(_res(narrowed), exp, "retriever, must", E2E_NAMES)
    hits = np.unique(_np(narrowed.ids)[_np(narrowed.ids) >= 0])
    rp, ix, _ = dev.get_rows(hits)
    assert hits.size and all(col in ix[rp[i]:rp[i + 1]] for i in range(hits.size))


# ---- generic values: the one test that is not bitwise -----------------------------------------------------------------------------------
def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=F32))).astype(np.float64)


def test_generic_values_within_the_rounding_of_the_formula():
    """Rows with the bench's value law: the kernel's fp64 sums run in another order than the reference's, so g may differ by 1 float32 ulp.
    Tolerances, one ulp per operation of the formula: pen = sim = fl32(g(p,j) / sqrt(g(p,p) g(j,j))) has three such sums and its own
    rounding: 4 ulp(pen); mmr = fl32(fl32(lam rel) - fl32(mu pen)) adds the rounding of mu * pen and of the subtraction: 4 ulp(pen) +
    ulp(mu pen) + ulp(mmr) (lam * rel has the same inputs on both sides).  Picks are compared where the reference's best two vals are more
    than 1e-5 apart."""
    c = ref.generic_case()
    k, lam = c["k"], c["lam"]
    traces = []
    want = ref.select(c["ids"], c["scores"], c["indptr"], c["indices"], c["values"], c["n_cols"], lam, k, traces=traces)
    clear = ref.generic_clear_steps(traces)
    got = _run(c, k, lam, "cosine", True, c["n_cols"])
    print("left out:", int((~clear).sum()), "of", clear.size)
    print("max |pen - ref| / ulp:", float((np.abs(got["pen"].astype(np.float64) - want["pen"]) / _ulp(want["pen"] + (want["pen"] == 0))).max()))
    print("max |mmr - ref| / ulp:", float((np.abs(got["mmr"].astype(np.float64) - want["mmr"]) / _ulp(want["mmr"])).max()))
    assert (~clear).mean() <= 0.10
    assert (got["pos"][clear] == want["pos"][clear]).all() and (got["ids"][clear] == want["ids"][clear]).all()
    same = clear & (got["pos"] == want["pos"])
    pen_tol = 4 * _ulp(want["pen"])
    mmr_tol = pen_tol + _ulp(F32(1 - lam) * want["pen"]) + _ulp(want["mmr"])
    assert (np.abs(got["pen"].astype(np.float64) - want["pen"])[same] <= pen_tol[same]).all()
    assert (np.abs(got["mmr"].astype(np.float64) - want["mmr"])[same] <= mmr_tol[same]).all()
    assert (want["pen"][:, 1] > 0).all()                                        # (the second pick does carry a similarity)
