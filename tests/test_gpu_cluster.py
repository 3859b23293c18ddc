"""GPU checks of the clustering calls: vs_index_assign, vs_centroid_half_norms, vs_label_bitmaps and the k-means loop against
the numpy reference (tests/_cluster_ref.py) applied to what get_rows returns.  Everything compares with ==: labels as integers, values and
centroids by their bits.  Outputs are junk-filled with spare slots that must keep their junk; host and device buffers are both driven."""
import ctypes as C

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import Assignment, DeviceIndex, KMeansResult, ShardGroup, assign_plan, centroid_half_norms, label_bitmaps
from vsearch_amd.doc_filter import DocFilter
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

import _range_ref as rref
import _term_agg_ref as aref
import _term_sum_ref as tref
import _cluster_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
JUNK_L, JUNK_V, JUNK_W = -0x5A5A5A5B, F32(-7.25e33), 0xA5A5A5A5
PAD = 3                       # spare slots behind the outputs, spare columns of a centroid row
STORES = {"fp32": nat.VS_F32, "fp16": nat.VS_F16, "bin": nat.VS_NONE}
_INF = F32(np.inf)


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _bits(x):
    return np.ascontiguousarray(_np(x), dtype=F32).view(np.uint32)


def _build(ip, ix, va, V, store="fp32"):
    return DeviceIndex.from_csr(ip, ix, None if store == "bin" else va, V, store_dtype=STORES[store])


def _rows(dev, store="fp32"):
    """the reference's view of the index: the cells get_rows returns for every row (None values for a binary index)"""
    ip, ix, va = dev.get_rows(np.arange(dev.n_rows, dtype=np.int64))
    return ip, ix, (None if store == "bin" else va)


def _case(lens, V, seed, grid=False):
    rng = np.random.default_rng(seed)
    ip, ix, va = aref.csr_case(np.asarray(lens), V, seed=seed)
    va = ref.grid(rng, va.size) if grid else (va * (0.5 + rng.random(va.size)).astype(F32)).astype(F32)
    return ip, ix, va, rng


def _bufs(arrs, on_dev):
    if on_dev:
        arrs = {k: torch.from_numpy(v).cuda() for k, v in arrs.items()}
        torch.cuda.synchronize()
        return arrs, (lambda t: C.c_void_p(t.data_ptr()))
    return arrs, (lambda a: C.c_void_p(a.ctypes.data))


def _raw_assign(dev, cen, bias, words, bit0, rpc, on_dev, want_values=True):
    """vs_index_assign into junk-filled outputs, host or device buffers throughout; the centroid rows carry PAD spare columns of NaN -> (rc, labels,
    values | None)"""
    n, (K, V) = dev.n_rows, cen.shape
    wide = np.full((K, V + PAD), np.nan, F32)
    wide[:, :V] = cen
    arrs = dict(cen=wide, labels=np.full(n + PAD, JUNK_L, np.int32))
    if want_values:
        arrs["values"] = np.full(n + PAD, JUNK_V, F32)
    if bias is not None:
        arrs["bias"] = np.ascontiguousarray(bias, dtype=F32)
    if words is not None:
        arrs["words"] = np.ascontiguousarray(words).view(np.int32)
    arrs, ptr = _bufs(arrs, on_dev)
    get = lambda k: ptr(arrs[k]) if k in arrs else None
    rc = nat.lib().vs_index_assign(dev._h, get("cen"), V + PAD, K, get("bias"), get("words"), bit0, rpc, get("labels"), get("values"), None)
    labels = _np(arrs["labels"])
    assert (labels[n:] == JUNK_L).all(), "slots behind the last row were written"
    values = None
    if want_values:
        values = _np(arrs["values"])
        assert (values[n:].view(np.uint32) == np.full(PAD, JUNK_V, F32).view(np.uint32)).all(), "slots behind the last row were written"
        values = values[:n]
    return rc, labels[:n], values


def _check(dev, rows, V, cen, bias=None, mask=None, bit0=0, live=None, rpc=0, store="fp32", what=None):
    """both buffer kinds against the reference; mask: bool [n] packed at bit0 with every spare bit set -> the reference's (labels, values)"""
    n = dev.n_rows
    allowed = None
    if mask is not None or live is not None:
        allowed = (mask if mask is not None else np.ones(n, bool)) & (live if live is not None else np.ones(n, bool))
    words = ref.pack(mask[None, :], bit0, spare=1)[0] if mask is not None else None
    want = ref.assign(*rows, V, cen, bias, allowed, store)
    for on_dev in (False, True):
        rc, labels, values = _raw_assign(dev, cen, bias, words, bit0, rpc, on_dev)
        assert rc == nat.VS_OK, nat.last_error()
        assert labels.dtype == np.int32 and (labels == want[0]).all(), (what, on_dev, np.flatnonzero(labels != want[0])[:5])
        assert (values.view(np.uint32) == want[1].view(np.uint32)).all(), (what, on_dev, np.flatnonzero(values != want[1])[:5])
    return want


# ---- slices and padded slots ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 128, 129, 257])
def test_slice_and_padding_edges(K):
    n, V = 150, 100
    lens = np.random.default_rng(K).integers(0, 41, size=n)
    lens[:2] = (0, 1)
    ip, ix, va, rng = _case(lens, V, seed=100 + K)
    va = np.abs(va)                                                   # values > 0
    dev = _build(ip, ix, va, V)
    rows = _rows(dev)
    w, slices = assign_plan(n, K, V)[:2]
    assert slices * w >= K and (K <= 64) == (w == 64)
    # all-negative centroids: every value of a non-empty row is negative, a padded slot's 0 would win if it were not masked
    cen = -(0.1 + rng.random((K, V))).astype(F32)
    want = _check(dev, rows, V, cen, what="negative centroids")
    assert (want[1][lens > 0] < 0).all() and (want[0] >= 0).all() and (want[0] < K).all()
    # a strongly negative bias: the same for every row, the empty ones included
    cen = rng.standard_normal((K, V)).astype(F32)
    bias = (-1000.0 - rng.random(K) * 50).astype(F32)
    want = _check(dev, rows, V, cen, bias, what="negative bias")
    assert (want[1] < -900).all() and want[0][0] == int(np.argmax(bias))
    if K > 2:
        assert len(set(want[0].tolist())) > 2


# ---- row lengths -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 70, 257])
def test_row_lengths_packets_and_trips(K):
    V = 1100
    lens = [0, 1, 8, 9, 512, 513, 1030, 7, 0, 511, 1030, 64]          # one packet, two, exactly 64, a second trip; last packets partly padding
    ip, ix, va, rng = _case(lens, V, seed=7 + K)
    dev = _build(ip, ix, va, V)
    rows = _rows(dev)
    assert (np.diff(rows[0]) == lens).all()
    cen = rng.standard_normal((K, V)).astype(F32)
    want = _check(dev, rows, V, cen, what="generic")
    assert want[0][0] == 0 and want[1][0] == 0                        # an empty row without a bias: label 0, value +0.0
    bias = rng.standard_normal(K).astype(F32)
    want = _check(dev, rows, V, cen, bias, what="bias")
    assert want[0][0] == want[0][8] == int(np.argmax(bias)) and want[1][0] == bias.max()


# ---- row counts and chunks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 2049])
def test_row_counts_and_chunks(n_rows):
    V, K = 100, 5
    lens = np.random.default_rng(n_rows).integers(0, 20, size=n_rows)
    ip, ix, va, rng = _case(lens, V, seed=n_rows)
    dev = _build(ip, ix, va, V)
    rows = _rows(dev)
    cen = rng.standard_normal((K, V)).astype(F32)
    mask = rng.random(n_rows) < 0.8
    for rpc in (0, 64):
        _check(dev, rows, V, cen, what=("plain", rpc), rpc=rpc)
        _check(dev, rows, V, cen, mask=mask, bit0=5, what=("filtered", rpc), rpc=rpc)
    assert assign_plan(n_rows, K, V, 64)[2] == (n_rows + 63) // 64


# ---- numerics ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["fp32", "fp16", "bin"])
def test_stores(store):
    n, V, K = 300, 100, 66
    lens = np.random.default_rng(5).integers(0, 50, size=n)
    ip, ix, va, rng = _case(lens, V, seed=17)
    dev = _build(ip, ix, va, V, store)
    rows = _rows(dev, store)
    cen = rng.standard_normal((K, V)).astype(F32)                      # no fp16 values: an fp16 store rounds them
    bias = rng.standard_normal(K).astype(F32)
    want = _check(dev, rows, V, cen, bias, store=store, what=store)
    if store == "fp16":
        unrounded = ref.assign(*rows, V, cen, bias, None, "fp32")
        assert (unrounded[1].view(np.uint32) != want[1].view(np.uint32)).any()        # the rounding of the centroids is visible
    hn = ref.half_norms(cen, store)
    _check(dev, rows, V, cen, -hn, store=store, what=(store, "l2"))
    assert (_bits(dev.half_norms(cen)) == hn.view(np.uint32)).all()


def test_duplicate_centroids_and_no_values():
    n, V = 200, 100
    lens = np.random.default_rng(9).integers(1, 30, size=n)
    ip, ix, va, rng = _case(lens, V, seed=19)
    dev = _build(ip, ix, va, V)
    rows = _rows(dev)
    base = rng.standard_normal((40, V)).astype(F32)
    cen = np.concatenate([base, base, base[:5]])                       # K = 85: every centroid has a copy at a higher index, in another lane
    want = _check(dev, rows, V, cen, what="duplicates")
    assert (want[0] < 40).all()                                       # the lower index wins
    for on_dev in (False, True):
        rc, labels, values = _raw_assign(dev, cen, None, None, 0, 0, on_dev, want_values=False)
        assert rc == nat.VS_OK and values is None and (labels == want[0]).all()
    res = dev.assign(cen)
    assert isinstance(res, Assignment) and res.labels.dtype == torch.int32 and res.values.dtype == torch.float32
    assert (_np(res.labels) == want[0]).all() and (_bits(res.values) == want[1].view(np.uint32)).all()
    res = dev.assign(torch.from_numpy(cen).cuda(), bias=torch.zeros(85, device="cuda"))          # device tensors, a zero bias: the same answer
    assert (_np(res.labels) == want[0]).all() and (_bits(res.values) == want[1].view(np.uint32)).all()


@pytest.mark.parametrize("V", [29523, 65535])
def test_wide_vocabularies(V):
    n, K = 200, 65
    lens = np.random.default_rng(V).integers(0, 60, size=n)
    lens[1] = 5
    ip, ix, va, rng = _case(lens, V, seed=V)
    ix[ip[1]:ip[2]][-1] = V - 1                                       # the last column is stored
    dev = _build(ip, ix, va, V)
    rows = _rows(dev)
    cen = rng.standard_normal((K, V)).astype(F32)
    _check(dev, rows, V, cen, -ref.half_norms(cen), what=V)
    hn = ref.half_norms(cen)
    assert (_bits(dev.half_norms(cen)) == hn.view(np.uint32)).all()


# ---- filters and deletions ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit0", [0, 5, 37])
def test_filters_and_deletions(bit0):
    n, V, K = 333, 100, 9
    lens = np.random.default_rng(bit0).integers(0, 30, size=n)
    ip, ix, va, rng = _case(lens, V, seed=23 + bit0)
    dev = _build(ip, ix, va, V)
    rows = _rows(dev)
    cen, bias = rng.standard_normal((K, V)).astype(F32), rng.standard_normal(K).astype(F32)
    mask = rng.random(n) < 0.6
    mask[64:128] = False                                              # a whole step of the walk is skipped
    want = _check(dev, rows, V, cen, bias, mask=mask, bit0=bit0, what="filter")
    assert (want[0][~mask] == -1).all() and np.isneginf(want[1][~mask]).all() and (want[0][mask] >= 0).all()
    none = _check(dev, rows, V, cen, bias, mask=np.zeros(n, bool), bit0=bit0, what="empty filter")
    assert (none[0] == -1).all()
    every = _check(dev, rows, V, cen, bias, what="no filter")
    dead = np.array([0, 5, 31, 32, 63, 64, 200, n - 1])
    live = np.ones(n, bool)
    live[dead] = False
    dev.delete_rows(dead)
    try:
        gone = _check(dev, rows, V, cen, bias, live=live, what="deleted")
        assert (gone[0][dead] == -1).all() and np.isneginf(gone[1][dead]).all()
        _check(dev, rows, V, cen, bias, mask=mask, bit0=bit0, live=live, what="deleted and filtered")
        res = dev.assign(cen, bias=bias, filter=DocFilter.from_mask(torch.from_numpy(mask)))
        both = ref.assign(*rows, V, cen, bias, mask & live)
        assert (_np(res.labels) == both[0]).all() and (_bits(res.values) == both[1].view(np.uint32)).all()
    finally:
        dev.restore_rows()
    back = _check(dev, rows, V, cen, bias, what="restored")
    assert (back[0] == every[0]).all()


# ---- cross-checks ------------------------------------------------------------------------------------------------------------------------------------
def test_values_equal_explain_on_grid_inputs():
    n, V, K = 120, 100, 11
    lens = np.random.default_rng(3).integers(0, 60, size=n)
    ip, ix, va, rng = _case(lens, V, seed=29, grid=True)
    dev = _build(ip, ix, va, V)
    rows = _rows(dev)
    cen = ref.grid(rng, (K, V))
    want = _check(dev, rows, V, cen, what="grid")
    ex = dev.explain(cen, np.tile(np.arange(n, dtype=np.int64), (K, 1)), topn=1)
    scores = _np(ex.scores).astype(F32)                               # [K, n]: the score of (centroid j, row r)
    picked = scores[want[0], np.arange(n)]
    assert (picked.view(np.uint32) == want[1].view(np.uint32)).all()
    assert (want[1] == scores.max(axis=0)).all() and (want[0] == scores.argmax(axis=0)).all()


def test_three_uneven_shards_equal_the_unsharded_index():
    n, V, K = 1000, 100, 70
    lens = np.random.default_rng(31).integers(0, 40, size=n)
    ip, ix, va, rng = _case(lens, V, seed=31)
    whole = _build(ip, ix, va, V)
    rows = _rows(whole)
    bounds = [0, 33, 437, n]                                          # no multiple of 32 at the seams
    group = ShardGroup([whole.slice_rows(bounds[i], bounds[i + 1] - bounds[i], device=0) for i in range(3)])
    cen, bias = rng.standard_normal((K, V)).astype(F32), rng.standard_normal(K).astype(F32)
    mask = rng.random(n) < 0.7
    flt = DocFilter.from_mask(torch.from_numpy(mask))
    dead = np.array([3, 32, 33, 436, 437, n - 1])
    live = np.ones(n, bool)
    try:
        for deleted in (False, True):
            if deleted:
                live[dead] = False
                group.delete_rows(dead)
                whole.delete_rows(dead)
            for f, allowed in ((None, live), (flt, mask & live)):
                want = ref.assign(*rows, V, cen, bias, allowed)
                for obj in (group, whole):
                    got = obj.assign(cen, bias=bias, filter=f)
                    assert (_np(got.labels) == want[0]).all() and (_bits(got.values) == want[1].view(np.uint32)).all()
    finally:
        group.restore_rows()
        whole.restore_rows()
        group.close()


# ---- half norms and label bitmaps --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 255, 256, 257, 29523])
def test_half_norms(V):
    rng = np.random.default_rng(V)
    K = 5
    cen = (rng.standard_normal((K, V)) * 10.0 ** rng.integers(-3, 3, size=(K, V))).astype(F32)
    for store, flag in (("fp32", False), ("fp16", True)):
        want = ref.half_norms(cen, store)
        got = centroid_half_norms(cen, round_f16=flag)
        assert got.dtype == F32 and (got.view(np.uint32) == want.view(np.uint32)).all(), (V, store)
        got = centroid_half_norms(torch.from_numpy(cen).cuda(), round_f16=flag)
        assert (_bits(got) == want.view(np.uint32)).all(), (V, store, "device")
    wide = np.full((K, V + PAD), np.nan, F32)                           # a row stride: the spare columns are not read, slots behind K not written
    wide[:, :V] = cen
    out = np.full(K + PAD, JUNK_V, F32)
    assert nat.lib().vs_centroid_half_norms(C.c_void_p(wide.ctypes.data), V + PAD, K, V, 0, C.c_void_p(out.ctypes.data), 0, None) == nat.VS_OK
    assert (out[:K].view(np.uint32) == ref.half_norms(cen).view(np.uint32)).all() and (out[K:].view(np.uint32) == _bits(np.full(PAD, JUNK_V))).all()


@pytest.mark.parametrize("bit0", [0, 5, 37])
@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 2049])
def test_label_bitmaps(bit0, n_rows):
    rng = np.random.default_rng(bit0 * 10000 + n_rows)
    labels = rng.integers(-1, 70, size=n_rows).astype(np.int32)
    span = (bit0 + n_rows + 31) // 32
    for B in (1, 3, 64, 65):
        values = rng.permutation(np.arange(-1, 90))[:B].astype(np.int32)                # -1 and values that occur nowhere among them
        values[0] = -1
        want = ref.label_bitmaps(labels, values, bit0)
        assert want.shape == (B, span)
        for on_dev in (False, True):
            arrs = dict(labels=labels, values=values, out=np.full((B, span + PAD), JUNK_W, np.uint32).view(np.int32))
            arrs, ptr = _bufs(arrs, on_dev)
            rc = nat.lib().vs_label_bitmaps(ptr(arrs["labels"]), n_rows, ptr(arrs["values"]), B, bit0, ptr(arrs["out"]), span + PAD, 0, None)
            assert rc == nat.VS_OK, nat.last_error()
            out = _np(arrs["out"]).view(np.uint32)
            assert (out[:, :span] == want).all(), (B, on_dev)
            assert (out[:, span:] == JUNK_W).all(), "words behind a bitmap's span were written"
        got = label_bitmaps(torch.from_numpy(labels).cuda(), values, bit0=bit0)
        assert got.dtype == torch.int32 and (_np(got).view(np.uint32) == want).all()
        assert (label_bitmaps(labels, values, bit0=bit0).view(np.uint32) == want).all()


def test_from_labels_composes_and_feeds_term_sums():
    n, V = 700, 100
    ip, ix, va = rref.csr_case(n, V, seed=41)
    dev = _build(ip, ix, va, V)
    cells = tref.Cells(*_rows(dev), V)
    rng = np.random.default_rng(41)
    labels = rng.integers(-1, 6, size=n).astype(np.int32)
    vals = [4, 0, 9, -1]                                              # 9 occurs nowhere
    f = DocFilter.from_labels(labels, vals)
    assert f.per_query and f.n_queries == 4 and f.n_rows == n
    masks = labels[None, :] == np.array(vals)[:, None]
    assert (_np(f.words).view(np.uint32) == ref.pack(masks)).all()
    one = DocFilter.from_labels(torch.from_numpy(labels).cuda(), 4)
    assert not one.per_query and (_np(one.words).view(np.uint32) == ref.pack(masks[:1])[0]).all()
    i64 = DocFilter.from_labels(torch.from_numpy(labels.astype(np.int64)), np.array(vals))
    assert (_np(i64.words) == _np(f.words)).all()
    visible = rng.random(n) < 0.5
    both = f & DocFilter.from_mask(torch.from_numpy(visible))
    assert (_np(both.words).view(np.uint32) == ref.pack(masks & visible[None, :])).all()
    assert (_np((~one).words).view(np.uint32) == ref.pack(~masks[:1])[0]).all()
    words = ref.pack(masks & visible[None, :])
    want = tref.term_sums(words, words.shape[1], 0, cells)
    got = dev.term_sums(filter=both)
    assert (_np(got.sums) == want[0]).all() and (_np(got.total) == want[1]).all() and want[1][2] == 0 and want[1][0] > 0
    res = dev.search(rref.sparse_queries(2, V, seed=5), 4, filter=one)           # a drill-down: only documents of label 4
    ids = _np(res[0])
    assert (ids >= 0).all() and (labels[ids] == 4).all()


# ---- argument errors on a device -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    n, V = 70, 100
    ip, ix, va = rref.csr_case(n, V, seed=43)
    dev = _build(ip, ix, va, V)
    cen = np.ones((3, V), F32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    labels = np.zeros(n, np.int32)
    call = lambda c=cen, ldc=V, K=3, b=None, bit0=0, rpc=0: nat.lib().vs_index_assign(dev._h, p(c), ldc, K, p(b) if b is not None else None, None,
                                                                                     bit0, rpc, p(labels), None, None)
    assert call() == nat.VS_OK
    assert call(K=0) == nat.VS_EINVAL and call(K=4097) == nat.VS_EINVAL and "4096" in nat.last_error()
    assert call(ldc=V - 1) == nat.VS_EINVAL and "ldc" in nat.last_error()
    assert call(rpc=100) == nat.VS_EINVAL and call(bit0=-1) == nat.VS_EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        c = cen.copy()
        c[2, V - 1] = bad
        assert call(c=c) == nat.VS_EINVAL and "finite" in nat.last_error()
        assert call(b=np.array([0, bad, 0], F32)) == nat.VS_EINVAL and "bias" in nat.last_error()
    d_lab = torch.zeros(n, dtype=torch.int32, device="cuda")            # host centroids, a device output: a mix
    assert nat.lib().vs_index_assign(dev._h, p(cen), V, 3, None, None, 0, 0, C.c_void_p(d_lab.data_ptr()), None, None) == nat.VS_EINVAL
    assert "all be host or all be device" in nat.last_error()
    for bad in (dict(centroids=np.ones((3, V + 1), F32)), dict(centroids=np.full((3, V), np.nan, F32)), dict(bias=np.ones(2, F32)),
                dict(filter=DocFilter.from_mask(torch.ones((2, n), dtype=torch.bool)))):
        with pytest.raises(ValueError):
            dev.assign(**{"centroids": cen, **bad})
    dense = DeviceIndex.from_dense(np.random.default_rng(3).random((64, 96)).astype(F32))
    with pytest.raises(NotImplementedError):
        dense.assign(np.ones((2, 96), F32))


# ---- k-means ---------------------------------------------------------------------------------------------------------------------------------------------
def _sparse_index(ip, ix, va, n, V):
    from vsearch_amd.ir import SparseIndex
    sp = SparseIndex(device="cuda:0", fp16=False)
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(np.asarray(ip)), torch.from_numpy(np.asarray(ix).astype(np.int64)), torch.from_numpy(va),
                                        size=(n, V))
    sp.move_to_device("cuda:0")
    return sp


def _same(res, want):
    """a KMeansResult against the reference's tuple, bit for bit"""
    assert isinstance(res, KMeansResult)
    assert (_bits(res.centroids) == want[0].view(np.uint32)).all(), "centroids"
    assert (_np(res.labels) == want[1]).all() and (_bits(res.values) == want[2].view(np.uint32)).all(), "assignment"
    assert res.counts.dtype == torch.int64 and (_np(res.counts) == want[3]).all() and res.n_iter == want[4] and list(res.changed) == want[5]


def _blobs(n=600, V=96, seed=51):
    """three planted blobs on disjoint column supports, plus a little noise on any column"""
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, 3, size=n)
    dense = np.zeros((n, V), F32)
    for r in range(n):
        cols = 32 * truth[r] + rng.choice(32, size=10, replace=False)
        dense[r, cols] = 1.0 + rng.random(10)
        dense[r, rng.choice(V, size=3, replace=False)] += 0.05 * rng.random(3)
    ip = np.concatenate([[0], np.cumsum((dense != 0).sum(axis=1))]).astype(np.int64)
    ix = np.nonzero(dense)[1].astype(np.int32)
    return ip, ix, dense[dense != 0].astype(F32), truth


def test_kmeans_recovers_three_planted_blobs():
    n, V = 600, 96
    ip, ix, va, truth = _blobs(n, V)
    sp = _sparse_index(ip, ix, va, n, V)
    starts = np.array([int(np.flatnonzero(truth == j)[0]) for j in range(3)])
    res = sp.kmeans(3, iters=10, init=torch.from_numpy(starts))
    assert (_np(res.labels) == truth).all() and (_np(res.counts) == np.bincount(truth)).all()          # (cluster j grew from a row of blob j)
    assert res.changed[-1] == 0 and res.n_iter < 10                   # the loop stops at changed == 0 before iters
    again = sp.kmeans(3, iters=10, seed=2)                            # a random start (its rows lie in three blobs): up to a relabelling
    lab = _np(again.labels)
    pairs = {(int(a), int(b)) for a, b in zip(lab, truth)}
    assert len(pairs) == 3 and len({a for a, _ in pairs}) == 3
    hits = sp.search(again.centroids, 5)                              # the centroids are queries for search
    for j in range(3):
        assert (lab[_np(hits.ids)[j]] == j).all()


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_kmeans_is_the_reference_loop_bit_for_bit(metric):
    n, V, K = 1500, 200, 7
    ip, ix, va = rref.csr_case(n, V, seed=61)
    sp = _sparse_index(ip, ix, va, n, V)
    rows = _rows(sp._device_index())
    starts = np.random.default_rng(61).choice(np.flatnonzero(np.diff(rows[0]) > 0), size=K, replace=False)
    start = np.zeros((K, V), F32)
    for j, r in enumerate(starts):
        start[j, rows[1][rows[0][r]:rows[0][r + 1]]] = rows[2][rows[0][r]:rows[0][r + 1]]
    want = ref.kmeans(*rows, V, start, 6, metric)
    res = sp.kmeans(K, iters=6, metric=metric, init=torch.from_numpy(starts))
    _same(res, want)
    assert len(want[5]) >= 3 and want[5][0] == n and (want[3] > 0).sum() >= 2
    _same(sp.kmeans(K, iters=6, metric=metric, init=torch.from_numpy(start)), want)        # the same start given as centroids
    two = sp.kmeans(K, iters=6, metric=metric, init=torch.from_numpy(starts))              # two runs are identical
    assert all((_bits(a) == _bits(b)).all() for a, b in zip(res[:3], two[:3])) and list(two.changed) == list(res.changed)
    # iters = 0 returns the start and its assignment
    zero = sp.kmeans(K, iters=0, metric=metric, init=torch.from_numpy(starts))
    _same(zero, ref.kmeans(*rows, V, start, 0, metric))
    assert zero.n_iter == 0 and zero.changed == [] and (_bits(zero.centroids) == start.view(np.uint32)).all()
    # a filter and deletions: the rows outside keep -1 and move no centroid
    mask = np.random.default_rng(62).random(n) < 0.6
    mask[starts] = True
    dead = np.flatnonzero(~mask)[:10]
    sp.delete(dead)
    flt = DocFilter.from_mask(torch.from_numpy(mask))
    part = sp.kmeans(K, iters=3, metric=metric, init=torch.from_numpy(starts), filter=flt)
    sp.restore()
    _same(part, ref.kmeans(*rows, V, start, 3, metric, allowed=mask))
    assert (_np(part.labels)[~mask] == -1).all()


def test_kmeans_duplicate_start_random_start_and_objective():
    n, V, K = 600, 96, 4
    ip, ix, va, truth = _blobs(n, V, seed=71)
    sp = _sparse_index(ip, ix, va, n, V)
    rows = _rows(sp._device_index())
    # a duplicated start centroid leaves the higher index empty; it keeps its centroid
    starts = np.array([0, 0, 1, 2])
    zero = sp.kmeans(K, iters=0, init=starts)
    assert int(zero.counts[1]) == 0 and (_np(zero.labels) != 1).all() and int(zero.counts[0]) > 0     # a tie goes to the lower index
    one = sp.kmeans(K, iters=1, init=starts)                           # one update: cluster 0 moved, the empty cluster 1 did not
    first = np.zeros(V, F32)
    first[rows[1][rows[0][0]:rows[0][1]]] = rows[2][rows[0][0]:rows[0][1]]
    assert (_bits(one.centroids[1]) == first.view(np.uint32)).all() and not (_bits(one.centroids[0]) == first.view(np.uint32)).all()
    assert one.changed == [n] and one.n_iter == 1
    # init=None: K distinct live, allowed rows under the seed; the same seed gives the same run, n_clusters above the rows raises
    a, b, c = sp.kmeans(K, iters=3, seed=5), sp.kmeans(K, iters=3, seed=5), sp.kmeans(K, iters=3, seed=6)
    assert all((_bits(x) == _bits(y)).all() for x, y in zip(a[:3], b[:3])) and not (_bits(a.centroids) == _bits(c.centroids)).all()
    few = np.zeros(n, bool)
    few[[3, 9, 27]] = True
    with pytest.raises(ValueError, match="exceeds"):
        sp.kmeans(4, filter=few)
    tiny = sp.kmeans(3, iters=2, filter=few)
    assert sorted(_np(tiny.labels)[few].tolist()) == [0, 1, 2] and int(tiny.counts.sum()) == 3
    with pytest.raises(IndexError):
        sp.kmeans(2, init=np.array([0, n]))
    # the l2 objective, from the returned values alone, never increases from one iteration to the next
    X2 = np.zeros(n)
    np.add.at(X2, np.repeat(np.arange(n), np.diff(rows[0])), rows[2].astype(np.float64) ** 2)
    starts = np.array([5, 17, 100, 333])
    obj = []
    for it in range(6):
        r = sp.kmeans(K, iters=it, init=starts)
        obj.append(float((X2 - 2.0 * _np(r.values).astype(np.float64)).sum()))
    print("k-means objective per iteration:", obj)
    assert all(y <= x for x, y in zip(obj, obj[1:])) and obj[-1] < obj[0]


def test_cluster_sets_the_facet_field_and_the_groups():
    n, V, K = 600, 96, 3
    ip, ix, va, truth = _blobs(n, V, seed=81)
    sp = _sparse_index(ip, ix, va, n, V)
    sp.delete(np.array([7, 8]))
    starts = np.array([int(np.flatnonzero(truth == j)[-1]) for j in range(3)])
    res = sp.cluster(K, iters=5, init=starts, set_groups=True)
    assert "cluster" in sp.facet_fields and sp.facet_names("cluster") == ["0", "1", "2"]
    top = sp.facets("cluster", topn=None)
    assert (_np(top.counts)[0] == _np(res.counts)).all() and int(top.total[0]) == n - 2 and int(res.counts.sum()) == n - 2
    lab = _np(res.labels)
    assert lab[7] == lab[8] == -1 and (_np(sp.groups) == np.where(lab < 0, K, lab)).all()
    q = _np(res.centroids).sum(axis=0, keepdims=True)
    got = sp.search_grouped(torch.from_numpy(q), k=3)                  # one hit per cluster
    groups = _np(got.groups)[0]
    assert sorted(groups.tolist()) == [0, 1, 2] and (lab[_np(got.ids)[0, :, 0]] == groups).all()
    sel = sp.search(torch.from_numpy(q), 6, filter=DocFilter.from_labels(res.labels, 1))            # the labels drive a DocFilter
    assert (lab[_np(sel.ids)[0]] == 1).all()
    terms = sp.cluster_terms(res.labels, K, topn=4)
    assert tuple(terms.cols.shape) == (K, 4) and (_np(terms.total) == _np(res.counts)).all()
    from vsearch_amd.ir import Index
    with pytest.raises(NotImplementedError):
        dense = Index(device="cuda:0", fp16=False)
        dense.vector = torch.rand(32, 16)
        dense.kmeans(2)


def test_retriever_cluster_documents(tiny_retriever):
    from vsearch_amd.ir.retriever.index import IndexType
    r = tiny_retriever
    n = 80
    r.build_index(make_texts(n, 5), index_type=IndexType.SPARSE)
    out = r.cluster_documents(4, topn=5, iters=3, seed=2)
    assert len(out) == 4 and sum(size for size, _ in out) == n
    assert "cluster" in r.index.facet_fields
    for size, terms in out:
        assert (size > 0) == bool(terms) and len(terms) <= 5
        assert all(isinstance(t, str) and w > 0 for t, w in terms) and [w for _, w in terms] == sorted((w for _, w in terms), reverse=True)
    assert all(t == FakeTokenizer().convert_ids_to_tokens([int(t[3:])])[0] for _, terms in out for t, _ in terms)
