"""GPU tests of facet counts (vs_facet_counts / vs_index_facet_counts / vs_facet_topn; DeviceIndex / ShardGroup .facet_counts / .top_facets,
Index.set_facet / .facets, Retriever.retrieve_facets) -- run on MI355X.

The contract is tests/_facet_ref.py.  Every value is an integer, so everything compares exactly.  The raw calls go into
junk-filled outputs whose count rows carry spare columns (ld_counts > n_labels) that must keep their junk, once on host buffers and once
on device buffers."""
import ctypes as C

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, FacetCounts, ShardGroup, TopFacets, facet_plan, facet_topn
from vsearch_amd.doc_filter import DocFilter
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

import _facet_ref as ref
import _range_ref as rref

pytestmark = pytest.mark.gpu

BINS = nat.FACET_LDS_BINS
JUNK = -0x5A5A5A5A5A5A5A5B
PAD = 3                       # spare columns of a count row
VR = 2000
N_IDX = 1000


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _raw(words, bit0, ld_words, and_words, B, labels, n_rows, L, rpc, on_dev, index=None):
    """vs_facet_counts (or vs_index_facet_counts on `index`) into junk-filled outputs, host or device buffers throughout -> (counts, total, other)"""
    outs = dict(counts=np.full((B, L + PAD), JUNK, np.int64), total=np.full(B, JUNK, np.int64), other=np.full(B, JUNK, np.int64))
    ins = dict(labels=np.ascontiguousarray(labels, dtype=np.int32))
    if words is not None:
        ins["words"] = np.ascontiguousarray(words).view(np.int32)
    if and_words is not None:
        ins["and"] = np.ascontiguousarray(and_words).view(np.int32)
    if on_dev:
        outs = {k: torch.from_numpy(v).cuda() for k, v in outs.items()}
        ins = {k: torch.from_numpy(v).cuda() for k, v in ins.items()}
        ptr = lambda t: C.c_void_p(t.data_ptr())
        torch.cuda.synchronize()
    else:
        ptr = lambda a: C.c_void_p(a.ctypes.data)
    pw = ptr(ins["words"]) if words is not None else None
    if index is None:
        rc = nat.lib().vs_facet_counts(pw, bit0, ld_words, ptr(ins["and"]) if and_words is not None else None, B, ptr(ins["labels"]), n_rows, L, rpc,
                                       ptr(outs["counts"]), L + PAD, ptr(outs["total"]), ptr(outs["other"]), 0, None)
    else:
        rc = nat.lib().vs_index_facet_counts(index._h, pw, bit0, ld_words, B, ptr(ins["labels"]), L, rpc, ptr(outs["counts"]), L + PAD,
                                             ptr(outs["total"]), ptr(outs["other"]), None)
    nat.check(rc)
    counts = _np(outs["counts"])
    assert (counts[:, L:] == JUNK).all(), "a count row's spare columns were written"
    return counts[:, :L], _np(outs["total"]), _np(outs["other"])


def _check(masks, bit0, labels, L, and_mask=None, rpc=0, shared=False, what=None, spare=1):
    """per-query sets `masks` [B, n] packed at bit0 with every spare bit set -> both buffer kinds against the reference"""
    B, n = masks.shape
    words = ref.pack(masks, bit0, spare=spare)
    aw = ref.pack(and_mask[None, :], bit0, spare=spare)[0] if and_mask is not None else None
    ld = 0 if shared else words.shape[1]
    want = ref.facet_counts(words, ld, bit0, n, labels, L, aw)
    assert (want[0].sum(axis=1) + want[2] == want[1]).all()
    for on_dev in (False, True):
        got = _raw(words, bit0, ld, aw, B, labels, n, L, rpc, on_dev)
        for g, w, name in zip(got, want, ("counts", "total", "other")):
            assert g.dtype == np.int64 and (g == w).all(), (what, name, on_dev, bit0, rpc)
    return want


# ---- bitmap edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049])
def test_bitmap_edges(n_rows):
    L, B = 5, 3
    labels = ref.labels_case(n_rows, L, seed=n_rows, frac_none=0.15, frac_big=0.1)
    masks = ref.masks_case(B, n_rows, seed=n_rows + 1, density=0.9)
    live = np.random.default_rng(n_rows).random(n_rows) < 0.8
    for bit0 in (0, 1, 31, 32, 33):
        _check(masks, bit0, labels, L, what="sets")                                    # the last word's spare bits are all set
        _check(masks, bit0, labels, L, and_mask=live, what="sets & and_words")
    empty, full = np.zeros((B, n_rows), bool), np.ones((B, n_rows), bool)
    assert (_check(empty, 1, labels, L, what="empty")[1] == 0).all()
    assert (_check(full, 33, labels, L, what="full")[1] == n_rows).all()
    want = ref.facet_counts(None, 0, 0, n_rows, labels, L)                             # words = NULL: every row set
    aw = ref.pack(live[None, :], 0, spare=1)[0]
    want_live = ref.facet_counts(None, 0, 0, n_rows, labels, L, aw)
    for on_dev in (False, True):
        for got, w in ((_raw(None, 0, 0, None, 1, labels, n_rows, L, 0, on_dev), want), (_raw(None, 0, 0, aw, 1, labels, n_rows, L, 0, on_dev), want_live)):
            assert all((g == x).all() for g, x in zip(got, w))


@pytest.mark.parametrize("n_rows,chunks", [(3 * 2048 + 1, 4), (4 * 2048, 4)])
def test_chunk_edges(n_rows, chunks):
    """rows_per_chunk = 2048: four chunks, the last of one row / a full one"""
    L, B = 37, 9
    assert facet_plan(n_rows, B, L, True, 2048)[2:] == (chunks, 2048)
    labels = ref.labels_case(n_rows, L, seed=n_rows, frac_none=0.05, frac_big=0.05)
    masks = ref.masks_case(B, n_rows, seed=5, density=0.7)
    masks[:, -1] = True                                                                # the one-row chunk holds a member
    for bit0 in (0, 33):
        _check(masks, bit0, labels, L, rpc=2048, what="chunks")


# ---- query tiles -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 7, 8, 9])
def test_query_tiles(B):
    n, L = 5000, 300
    labels = ref.labels_case(n, L, seed=B, frac_none=0.1, frac_big=0.05)
    masks = ref.masks_case(B, n, seed=B + 10, density=0.6)
    assert facet_plan(n, B, L, True)[1] == 8
    _check(masks, 0, labels, L, what="tiles")
    _check(masks, 31, labels, L, rpc=64, what="tiles, 64-row chunks")


def test_shared_bitmap():
    n, L = 5000, 300
    labels = ref.labels_case(n, L, seed=4, frac_none=0.1)
    masks = ref.masks_case(1, n, seed=14, density=0.5)
    for bit0 in (0, 33):
        _check(masks, bit0, labels, L, shared=True, what="shared")


# ---- label edges -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, BINS // 8, BINS // 8 + 1, BINS // 4, BINS // 4 + 1, BINS // 2, BINS // 2 + 1, BINS, BINS + 1])
def test_label_edges_at_the_plan_switch_points(L):
    n, B = 10_000, 9
    labels = ref.labels_case(n, L, seed=L, frac_none=0.05, frac_big=0.05)
    labels[:3] = (0, L - 1, L)                                                          # the first, the last label and the first one outside
    masks = ref.masks_case(B, n, seed=L + 1, density=0.8)
    masks[:, :3] = True
    regime, qt, _, _ = facet_plan(n, B, L, True)
    assert regime == (1 if L > BINS else 0) and (regime == 1 or qt * L <= BINS)
    want = _check(masks, 0, labels, L, what="switch points")
    assert (want[2] > 0).all() and (want[0][:, L - 1] > 0).all()


@pytest.mark.parametrize("L", [1, 64, BINS + 1])
def test_every_row_on_one_label(L):
    """the most contended case: the label's count equals the total"""
    n, B = 10_000, 9
    labels = np.full(n, L - 1, dtype=np.int32)
    masks = ref.masks_case(B, n, seed=L, density=0.9)
    masks[0] = True
    want = _check(masks, 1, labels, L, what="one label")
    assert (want[0][:, L - 1] == want[1]).all() and want[1][0] == n and (want[2] == 0).all()


@pytest.mark.parametrize("L", [50, BINS + 1])
def test_labels_outside_the_range_and_chunk_sizes(L):
    n, B = 10_000, 9
    labels = ref.labels_case(n, L, seed=9, frac_none=0.3, frac_big=0.3)
    labels[:4] = (-1, -(1 << 31), (1 << 31) - 1, L)
    masks = ref.masks_case(B, n, seed=19, density=0.9)
    masks[:, :4] = True
    res = [_check(masks, 33, labels, L, rpc=rpc, what="outside") for rpc in (64, 2048, 0)]
    assert (res[0][2] >= 4).all()
    for r in res[1:]:
        assert all((a == b).all() for a, b in zip(r, res[0]))


# ---- top-n -------------------------------------------------------------------------------------------------------------------------------------
def _topn_both(counts, n, min_count=1):
    want = ref.topn(counts, n, min_count)
    B, L = counts.shape
    for on_dev in (False, True):
        outs = dict(labels=np.full((B, n), 77, np.int32), counts=np.full((B, n), JUNK, np.int64))
        c = np.ascontiguousarray(counts, dtype=np.int64)
        if on_dev:
            outs = {k: torch.from_numpy(v).cuda() for k, v in outs.items()}
            c = torch.from_numpy(c).cuda()
            ptr = lambda t: C.c_void_p(t.data_ptr())
            torch.cuda.synchronize()
        else:
            ptr = lambda a: C.c_void_p(a.ctypes.data)
        nat.check(nat.lib().vs_facet_topn(ptr(c), L, B, L, n, min_count, ptr(outs["labels"]), ptr(outs["counts"]), 0, None))
        assert (_np(outs["labels"]) == want[0]).all() and (_np(outs["counts"]) == want[1]).all(), (n, min_count, on_dev)
    return want


@pytest.mark.parametrize("n", [1, 64, 65, 1024])
def test_topn_sizes(n):
    rng = np.random.default_rng(n)
    counts = rng.integers(0, 40, size=(3, 3000)).astype(np.int64)                      # many ties, some zeros
    counts[1] = 0
    counts[2, ::7] = rng.integers(1 << 20, 1 << 32, size=counts[2, ::7].size)
    want = _topn_both(counts, n)
    assert (want[0][1] == -1).all() and (want[1][1] == 0).all()
    got = facet_topn(torch.from_numpy(counts).cuda(), n, device=0)
    assert (_np(got[0]) == want[0]).all() and (_np(got[1]) == want[1]).all()


def test_topn_ties_floor_and_more_slots_than_labels():
    counts = np.full((2, 200), 6, dtype=np.int64)                                      # all counts equal: label ascending
    want = _topn_both(counts, 64)
    assert want[0][0].tolist() == list(range(64))
    want = _topn_both(counts[:, :9], 20)                                               # n > n_labels
    assert want[0][0].tolist() == list(range(9)) + [-1] * 11
    counts = np.array([[5, 3, 3, 3, 2, 2, 9, 0]], dtype=np.int64)
    assert _topn_both(counts, 8, min_count=3)[0][0].tolist() == [6, 0, 1, 2, 3, -1, -1, -1]     # the floor keeps the whole tie at 3 ...
    assert _topn_both(counts, 8, min_count=4)[0][0].tolist() == [6, 0, -1, -1, -1, -1, -1, -1]  # ... or none of it
    assert _topn_both(counts, 3, min_count=0)[0][0].tolist() == [6, 0, 1]                       # n cuts inside the tie: the smallest label
    assert _topn_both(counts, 8, min_count=-5)[1][0].tolist() == [9, 5, 3, 3, 3, 2, 2, 0]


def test_topn_of_100000_labels():
    rng = np.random.default_rng(11)
    counts = rng.integers(0, 5000, size=(2, 100_000)).astype(np.int64)
    counts[1] = np.arange(100_000)                                                     # ascending: every step admits new candidates
    _topn_both(counts, 1024)


# ---- index level -----------------------------------------------------------------------------------------------------------------------------
_idx = {}


def _index_case():
    """-> (DeviceIndex of N_IDX rows, queries, reference scores, csr parts); built once, left as it was by every test"""
    if not _idx:
        ip, ix, va = rref.csr_case(N_IDX, VR, seed=1040)
        q = rref.sparse_queries(9, VR, seed=N_IDX + 1)
        _idx["case"] = (DeviceIndex.from_csr(ip, ix, va, VR, store_dtype=nat.VS_F32), q, rref.scores(q, ip, ix, va, "fp32"), (ip, ix, va))
    return _idx["case"]


def _mid_thresholds(S, B, rank):
    return np.array([np.sort(S[b])[::-1][rank] for b in range(B)], dtype=np.float32)


def test_deleted_rows_never_count():
    dev, q, S, _ = _index_case()
    n, L, B = N_IDX, 12, 9
    labels = ref.labels_case(n, L, seed=21, frac_none=0.1, frac_big=0.05)
    masks = ref.masks_case(B, n, seed=22, density=0.9)
    words = ref.pack(masks, 0, spare=1)
    dead = np.array([0, 31, 32, 500, 998, 999])
    live = np.ones(n, bool)
    live[dead] = False
    full = ref.facet_counts(words, words.shape[1], 0, n, labels, L)
    dev.delete_rows(dead)
    try:
        want = ref.facet_counts(words, words.shape[1], 0, n, labels, L, ref.pack(live[None, :])[0])
        assert (want[1] < full[1]).any()
        for on_dev in (False, True):
            for rpc in (0, 64):
                got = _raw(words, 0, words.shape[1], None, B, labels, n, L, rpc, on_dev, index=dev)
                assert all((g == w).all() for g, w in zip(got, want))
        res = dev.facet_counts(labels, L)                                              # no filter: the label distribution of the live index
        assert isinstance(res, FacetCounts) and isinstance(res.counts, np.ndarray)
        want_all = ref.facet_counts(None, 0, 0, n, labels, L, ref.pack(live[None, :])[0])
        assert all((_np(g) == w).all() for g, w in zip(res, want_all)) and int(res.total[0]) == n - dead.size == dev.n_live
        res = dev.facet_counts(torch.from_numpy(labels).cuda(), L, filter=DocFilter.from_mask(torch.from_numpy(masks)))
        assert isinstance(res.counts, torch.Tensor) and res.counts.is_cuda
        assert all((_np(g) == w).all() for g, w in zip(res, want))
        top = dev.top_facets(labels, L, 5, filter=torch.from_numpy(masks[0]), min_count=2)     # a shared mask: B = 1
        assert isinstance(top, TopFacets) and top.labels.shape == (1, 5)
        wl, wc = ref.topn(want[0][:1], 5, 2)
        assert (top.labels == wl).all() and (top.counts == wc).all() and top.total[0] == want[1][0] and top.other[0] == want[2][0]
    finally:
        dev.restore_rows()
    for on_dev in (False, True):
        got = _raw(words, 0, words.shape[1], None, B, labels, n, L, 0, on_dev, index=dev)
        assert all((g == w).all() for g, w in zip(got, full))


def test_row_shards_equal_the_unsharded_index():
    whole, q, S, _ = _index_case()
    n, B = N_IDX, 9
    ndev = torch.cuda.device_count()
    bounds = [0, 437, 770, n]                                       # shard sizes 437, 333, 230: none a multiple of 32
    shards = [whole.slice_rows(bounds[i], bounds[i + 1] - bounds[i], device=i if ndev >= 3 else 0) for i in range(3)]
    group = ShardGroup(shards)
    masks = ref.masks_case(B, n, seed=31, density=0.9)
    flt = DocFilter.from_mask(torch.from_numpy(masks))
    words = ref.pack(masks)
    dead = np.array([3, 436, 437, 769, 770, 999])
    live = np.ones(n, bool)
    live[dead] = False
    try:
        for L in (7, BINS + 1):
            labels = ref.labels_case(n, L, seed=L, frac_none=0.1, frac_big=0.05)
            t_labels = torch.from_numpy(labels).cuda()
            for and_words in (None, ref.pack(live[None, :])[0]):
                if and_words is not None:
                    group.delete_rows(dead)
                    whole.delete_rows(dead)
                want = ref.facet_counts(words, words.shape[1], 0, n, labels, L, and_words)
                want_all = ref.facet_counts(None, 0, 0, n, labels, L, and_words)
                for lab in (labels, t_labels):
                    got = group.facet_counts(lab, L, filter=flt)
                    one = whole.facet_counts(lab, L, filter=flt)
                    assert all((_np(g) == w).all() and (_np(o) == w).all() for g, o, w in zip(got, one, want))
                    assert all((_np(g) == w).all() for g, w in zip(group.facet_counts(lab, L), want_all))
                top = group.top_facets(t_labels, L, 4, filter=flt)                 # taken after the sum, never per shard
                wl, wc = ref.topn(want[0], 4)
                assert (_np(top.labels) == wl).all() and (_np(top.counts) == wc).all() and (_np(top.total) == want[1]).all()
                assert (_np(whole.top_facets(t_labels, L, 4, filter=flt).labels) == wl).all()
            group.restore_rows()
            whole.restore_rows()
    finally:
        group.restore_rows()
        whole.restore_rows()
        group.close()


def _sparse_index(ip, ix, va, n):
    from vsearch_amd.ir import SparseIndex
    sp = SparseIndex(device="cuda:0", fp16=False)
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(va), size=(n, VR))
    sp.move_to_device("cuda:0")
    return sp


def test_index_facade_fields_follow_the_index():
    _, q, S, (ip, ix, va) = _index_case()
    n, B = N_IDX, 9
    tq = torch.from_numpy(q)
    sp = _sparse_index(ip, ix, va, n)
    L = 11
    labels = ref.labels_case(n, L, seed=41, frac_none=0.1).astype(np.int64)
    groups = (np.arange(n) // 7).astype(np.int64)
    sp.set_facet("topic", labels, names=[f"t{i}" for i in range(L)])
    sp.set_facet("year", labels % 3)
    sp.set_groups(groups)
    assert sp.facet_fields == ["topic", "year"] and sp.facet_names("topic")[2] == "t2" and sp.facet_names("year") is None
    with pytest.raises(ValueError, match="no name"):
        sp.set_facet("bad", np.full(n, L), names=["x"] * L)
    with pytest.raises(KeyError):
        sp.facets("nope")
    thr = _mid_thresholds(S, B, 150)
    # facets(q, min_score): the set is match_filter's; total == count_matches; dense counts == the reference on match_filter's words
    mf = sp.match_filter(tq, thr)
    w = _np(mf.words).view(np.uint32)
    want = ref.facet_counts(w, w.shape[1], 0, n, labels, L)
    dense = sp.facets("topic", tq, thr, topn=None)
    assert isinstance(dense, FacetCounts) and all((_np(g) == x).all() for g, x in zip(dense, want))
    assert (_np(dense.total) == _np(sp.count_matches(tq, thr))).all() and (want[1] > 100).all()
    top = sp.facets("topic", tq, thr, topn=4, min_count=2)
    wl, wc = ref.topn(want[0], 4, 2)
    assert isinstance(top, TopFacets) and (_np(top.labels) == wl).all() and (_np(top.counts) == wc).all() and (_np(top.other) == want[2]).all()
    # a term filter and a `visible` mask combine with the match set
    cols = _np(sp.get_vectors(torch.tensor([3])).col_indices())
    col = int(cols[_np(sp.doc_freq(cols)).argmax()])
    visible = np.random.default_rng(42).random(n) < 0.7
    has = np.zeros(n, bool)
    has[np.repeat(np.arange(n), np.diff(ip))[ix == col]] = True
    f = sp.term_filter(must=[col]) & DocFilter.from_mask(torch.from_numpy(visible))
    allowed = (has & visible)[None, :]
    want_f = ref.facet_counts(w & ref.pack(allowed)[0][None, :], w.shape[1], 0, n, labels, L)
    got = sp.facets("topic", tq, thr, filter=f, topn=None)
    assert all((_np(g) == x).all() for g, x in zip(got, want_f))
    want_only = ref.facet_counts(ref.pack(allowed), 0, 0, n, labels, L)               # without queries: the filter alone, B = 1
    got = sp.facets("topic", filter=f, topn=None)
    assert all((_np(g) == x).all() for g, x in zip(got, want_only)) and 0 < int(got.total[0]) < n
    # field = "groups"
    n_groups = int(groups.max()) + 1
    got = sp.facets("groups", tq, thr, topn=None)
    assert all((_np(g) == x).all() for g, x in zip(got, ref.facet_counts(w, w.shape[1], 0, n, groups, n_groups)))
    # delete -> restore -> delete -> compact: the fields stay aligned with the documents
    dead = np.array([0, 5, 64, 500, 999])
    live = np.ones(n, bool)
    live[dead] = False
    sp.delete(dead)
    want_live = ref.facet_counts(None, 0, 0, n, labels, L, ref.pack(live[None, :])[0])
    assert all((_np(g) == x).all() for g, x in zip(sp.facets("topic", topn=None), want_live))
    sp.restore()
    assert int(sp.facets("topic", topn=None).total[0]) == n
    sp.delete(dead)
    old = _np(sp.compact())
    assert (old == np.flatnonzero(live)).all()
    got = sp.facets("topic", topn=None)
    assert all((_np(g) == x).all() for g, x in zip(got, ref.facet_counts(None, 0, 0, n - dead.size, labels[live], L)))
    assert (_np(sp.facets("year", topn=None).counts) == ref.facet_counts(None, 0, 0, n - dead.size, labels[live] % 3, 3)[0]).all()
    # add(..., facets=): required, validated before anything changes, then appended
    new = torch.zeros(3, VR)
    new[:, 5] = 1.0
    with pytest.raises(ValueError, match="facet fields"):
        sp.add(new, groups=[1, 2, 3])
    assert sp._n_rows() == n - dead.size
    ids = sp.add(new, groups=[1, 2, 3], facets={"topic": [2, 2, -1], "year": [7, 0, 1]})
    assert _np(ids).tolist() == [n - 5, n - 4, n - 3]
    labels2 = np.concatenate([labels[live], [2, 2, -1]])
    got = sp.facets("topic", topn=None)
    assert all((_np(g) == x).all() for g, x in zip(got, ref.facet_counts(None, 0, 0, n - 2, labels2, L)))
    year = sp.facets("year", topn=None)                             # a field without names grows its n_labels with the new codes
    assert year.counts.shape == (1, 8) and int(year.counts[0, 7]) == 1
    sp.set_facet("year", None)
    assert sp.facet_fields == ["topic"]


def test_sharded_facade_equals_the_single_index():
    _, q, S, (ip, ix, va) = _index_case()
    n, B, L = N_IDX, 9, 11
    tq = torch.from_numpy(q)
    labels = ref.labels_case(n, L, seed=51, frac_none=0.1)
    thr = _mid_thresholds(S, B, 150)
    sp = _sparse_index(ip, ix, va, n)
    sp.set_facet("topic", labels)
    want = tuple(_np(t) for t in sp.facets("topic", tq, thr, topn=None))
    want_top = tuple(_np(t) for t in sp.facets("topic", tq, thr, topn=3))
    sp.shard_rows([0, 0, 0])
    assert sp.shards is not None and len(sp.shards) == 3
    assert all((_np(g) == w).all() for g, w in zip(sp.facets("topic", tq, thr, topn=None), want))
    assert all((_np(g) == w).all() for g, w in zip(sp.facets("topic", tq, thr, topn=3), want_top))


# ---- the retriever -----------------------------------------------------------------------------------------------------------------------------
def test_retrieve_facets(tiny_retriever):
    from vsearch_amd.ir.retriever.index import IndexType
    r = tiny_retriever
    n = 80
    texts = make_texts(n, 5)
    r.build_index(texts, index_type=IndexType.SPARSE)
    idx = r.index
    langs = ["en", "de", "fr", None]
    idx.data = [dict(text=t, **({"lang": langs[i % 4]} if langs[i % 4] else {})) for i, t in enumerate(texts)]
    names = idx.facet_from_samples("lang")
    assert names == ["de", "en", "fr"] and idx.facet_fields == ["lang"]
    codes = np.array([{"en": 1, "de": 0, "fr": 2, None: -1}[langs[i % 4]] for i in range(n)])
    queries = make_texts(4, 9)
    q_emb = r.process_query(queries, 0, r.encoder_q.config.topk)
    sc = _np(idx.explain(q_emb, torch.arange(n).repeat(4, 1), topn=0).scores).astype(np.float32)
    distinct = [np.unique(sc[b]) for b in range(4)]
    thr = np.array([d[d.size // 2] for d in distinct], dtype=np.float32)
    m = sc >= thr[:, None]
    want = ref.facet_counts(ref.pack(m), 3, 0, n, codes, 3)
    facets, totals = r.retrieve_facets(queries, "lang", thr, topn=5)
    assert totals == want[1].tolist() == _np(r.retrieve_range(queries, thr, max_hits=0).counts).tolist()
    for b in range(4):
        wl, wc = ref.topn(want[0][b:b + 1], 5)
        assert facets[b] == [(names[l], int(c)) for l, c in zip(wl[0], wc[0]) if l >= 0]
    # term constraints act through the match set, as in retrieve_range
    cols = _np(idx.get_vectors(torch.tensor([3])).col_indices())
    col = int(cols[_np(idx.doc_freq(cols)).argmin()])
    facets, totals = r.retrieve_facets(queries, "lang", -np.inf, must=[col])
    assert totals == _np(r.retrieve_range(queries, -np.inf, max_hits=0, must=[col]).counts).tolist() and 0 < totals[0] < n
    assert all(sum(c for _, c in f) <= t for f, t in zip(facets, totals))
