"""GPU tests of the term aggregations (vs_index_term_counts / vs_index_term_counts_ids / vs_term_topn; DeviceIndex / ShardGroup .term_counts /
.top_terms, Index.term_counts / .significant_terms, Retriever.significant_terms) -- run on MI355X.

The contract is tests/_term_agg_ref.py.  The counts are integers and the scores fp64 arithmetic rounded once to fp32, so
everything compares exactly.  Expected counts come from the reference applied to what get_rows returns for the same index, so they hold whatever
the builder does with explicit zeros.  The raw calls go into junk-filled outputs whose count rows carry spare columns (ld_counts = n_cols + 3)
that must keep their junk, once on host buffers and once on device buffers."""
import ctypes as C

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, ShardGroup, TermCounts, TopTerms, facet_topn, term_plan, term_topn
from vsearch_amd.doc_filter import DocFilter
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

import _range_ref as rref
from _facet_ref import masks_case
import _term_agg_ref as ref

pytestmark = pytest.mark.gpu

LDS_COLS = nat.TERM_LDS_COLS
JUNK = -0x5A5A5A5A5A5A5A5B
PAD = 3                       # spare columns of a count row
F32 = np.float32
STORES = {"fp32": nat.VS_F32, "fp16": nat.VS_F16, "bin": nat.VS_NONE}


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _masks(B, n_rows, seed, density=0.9):
    """per-query sets of different densities with all-zero stretches (whole 64-row steps and 2048-row spans are skipped)"""
    return masks_case(B, n_rows, seed=seed, density=density)


def _build(ip, ix, va, V, store="fp32"):
    return DeviceIndex.from_csr(ip, ix, None if store == "bin" else va, V, store_dtype=STORES[store])


def _has(dev, V):
    """the reference's view of the index: has[r, c] from what get_rows returns for every row"""
    ip, ix, va = dev.get_rows(np.arange(dev.n_rows, dtype=np.int64))
    return ref.has_matrix(ip, ix, va, V)


def _bufs(arrs, on_dev):
    if on_dev:
        arrs = {k: torch.from_numpy(v).cuda() for k, v in arrs.items()}
        torch.cuda.synchronize()
        return arrs, (lambda t: C.c_void_p(t.data_ptr()))
    return arrs, (lambda a: C.c_void_p(a.ctypes.data))


def _outs(B, V):
    return dict(counts=np.full((B, V + PAD), JUNK, np.int64), total=np.full(B, JUNK, np.int64))


def _taken(outs, V):
    counts = _np(outs["counts"])
    assert (counts[:, V:] == JUNK).all(), "a count row's spare columns were written"
    return counts[:, :V], _np(outs["total"])


def _raw_counts(dev, V, words, bit0, ld_words, B, rpc, on_dev):
    """vs_index_term_counts into junk-filled outputs, host or device buffers throughout -> (counts, total)"""
    arrs = _outs(B, V)
    if words is not None:
        arrs["words"] = np.ascontiguousarray(words).view(np.int32)
    arrs, ptr = _bufs(arrs, on_dev)
    nat.check(nat.lib().vs_index_term_counts(dev._h, ptr(arrs["words"]) if words is not None else None, bit0, ld_words, B, rpc, ptr(arrs["counts"]),
                                             V + PAD, ptr(arrs["total"]), None))
    return _taken(arrs, V)


def _raw_ids(dev, V, ids, id_offset, strict, on_dev, ld=None):
    """vs_index_term_counts_ids into junk-filled outputs -> (rc, counts, total); ld > m: the list rows carry spare entries"""
    B, m = ids.shape
    ld = ld or m
    lists = np.full((B, ld), 0x7777777777, np.int64)                 # (spare entries name no row: they must not be read)
    lists[:, :m] = ids
    arrs = _outs(B, V)
    arrs["ids"] = lists
    arrs, ptr = _bufs(arrs, on_dev)
    rc = nat.lib().vs_index_term_counts_ids(dev._h, ptr(arrs["ids"]), B, m, ld, id_offset, strict, ptr(arrs["counts"]), V + PAD, ptr(arrs["total"]), None)
    return (rc,) + _taken(arrs, V)


def _check(dev, has, masks, bit0, live=None, rpc=0, shared=False, what=None):
    """per-query sets `masks` [B, n] packed at bit0 with every spare bit set -> both buffer kinds against the reference"""
    B, n = masks.shape
    V = has.shape[1]
    words = ref.pack(masks, bit0, spare=1)
    ld = 0 if shared else words.shape[1]
    want = ref.term_counts(words, ld, bit0, has, ref.pack(live[None, :])[0] if live is not None else None)
    for on_dev in (False, True):
        got = _raw_counts(dev, V, words, bit0, ld, B, rpc, on_dev)
        for g, w, name in zip(got, want, ("counts", "total")):
            assert g.dtype == np.int64 and (g == w).all(), (what, name, on_dev, bit0, rpc)
    return want


def _check_null(dev, has, live=None):
    want = ref.term_counts(None, 0, 0, has, ref.pack(live[None, :])[0] if live is not None else None)
    for on_dev in (False, True):
        got = _raw_counts(dev, has.shape[1], None, 0, 0, 1, 0, on_dev)
        assert all((g == w).all() for g, w in zip(got, want)), ("NULL words", on_dev)
    return want


# ---- bitmap edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049])
def test_bitmap_edges(n_rows):
    V, B = 50, 3
    rng = np.random.default_rng(n_rows)
    ip, ix, va = ref.csr_case(rng.integers(0, 13, size=n_rows), V, seed=n_rows, zeros=0.1)
    dev = _build(ip, ix, va, V)
    has = _has(dev, V)
    masks = _masks(B, n_rows, n_rows + 1)
    masks[:, -1] = True                                                                # the last row is a member: the spare bits sit right behind it
    for bit0 in (0, 1, 31, 32, 33):
        _check(dev, has, masks, bit0, what="sets")                                     # the last word's spare bits are all set
    empty, full = np.zeros((B, n_rows), bool), np.ones((B, n_rows), bool)
    assert (_check(dev, has, empty, 1, what="empty")[0] == 0).all()
    want = _check(dev, has, full, 33, what="full")
    assert (want[1] == n_rows).all() and (want[0][0] == has.sum(axis=0)).all()
    assert (_check_null(dev, has)[1] == n_rows).all()                                  # words = NULL: every row set
    if n_rows >= 33:                                                                   # tombstones are read at bit 0 whatever bit0 is
        dead = np.unique(np.array([0, 31, 32, n_rows - 1]))
        live = np.ones(n_rows, bool)
        live[dead] = False
        dev.delete_rows(dead)
        for bit0 in (0, 31, 33):
            _check(dev, has, masks, bit0, live=live, what="sets & live")
        assert (_check_null(dev, has, live)[1] == n_rows - dead.size).all()


# ---- row shapes and stores -----------------------------------------------------------------------------------------------------------------------
SHAPE_LENS = [0, 1, 7, 8, 9, 511, 512, 513, 0, 0, 64, 65, 3, 520, 16, 1]


@pytest.mark.parametrize("store", ["fp32", "fp16", "bin"])
def test_row_shapes_and_stores(store):
    V = 700
    rng = np.random.default_rng(5)
    lens = np.concatenate([SHAPE_LENS, rng.integers(0, 30, size=184)])                  # 200 rows
    ip, ix, va = ref.csr_case(lens, V, seed=6, zeros=0.15)
    assert (va == 0).sum() > 50 and np.signbit(va[va == 0]).any() and not np.signbit(va[va == 0]).all()    # explicit +0.0 and -0.0 cells
    dev = _build(ip, ix, va, V, store)
    has = _has(dev, V)
    assert (has == ref.has_matrix(ip, ix, None if store == "bin" else va, V)).all()    # get_rows and the input agree on who has what
    if store != "bin":
        assert has.sum() < ix.size                                                     # the stored zeros are not terms
    n = lens.size
    masks = _masks(3, n, 7)
    masks[:, :len(SHAPE_LENS)] = True
    _check(dev, has, masks, 0, what=store)
    _check(dev, has, masks, 33, what=store)
    for r in range(len(SHAPE_LENS)):                                                   # every shape alone: its count row is the row itself
        one = np.zeros((1, n), bool)
        one[0, r] = True
        want = _check(dev, has, one, 1, shared=True, what=(store, "row", r))
        assert want[1][0] == 1 and (want[0][0] == has[r]).all()
    # a row holding every column of a small n_cols
    Vs = 24
    ip2, ix2, va2 = ref.csr_case([Vs, 0, Vs, 5, Vs], Vs, seed=8, zeros=0.2)
    small = _build(ip2, ix2, va2, Vs, store)
    has2 = _has(small, Vs)
    want = _check_null(small, has2)
    if store == "bin":
        assert want[0][0].min() == 3 and want[0][0].max() == 4
    ids = np.array([[0, 2, 4, 0, 3, 1]], dtype=np.int64)
    for on_dev in (False, True):
        rc, c, t = _raw_ids(small, Vs, ids, 0, 1, on_dev)
        w = ref.term_counts_ids(ids, 0, has2)
        assert rc == nat.VS_OK and (c == w[0]).all() and (t == w[1]).all() and t[0] == 6


# ---- column counts: both regimes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 7, 8, 29523, LDS_COLS, LDS_COLS + 1, 65535])
def test_column_counts_in_both_regimes(V):
    n, B = 300, 3
    rng = np.random.default_rng(V)
    lens = rng.integers(0, min(V, 40) + 1, size=n)
    lens[:2] = (min(V, 40), 0)
    ip, ix, va = ref.csr_case(lens, V, seed=V + 1, zeros=0.05, hot=V - 1)              # every non-empty row carries the last column
    ix[ip[0]] = 0                                                                      # ... and row 0 the first one
    dev = _build(ip, ix, va, V)
    has = _has(dev, V)
    assert term_plan(n, B, V, True)[0] == (1 if V > LDS_COLS else 0)
    masks = _masks(B, n, V + 2)
    masks[:, 0] = True
    want = _check(dev, has, masks, 31, what="columns")
    assert (want[0][:, 0] >= 1).all()
    # all waves on one bin: only the hot column's cells are non-zero in this index
    keep = (ix == V - 1)
    hot = _build(ip, ix, np.where(keep, va, 0).astype(F32) + np.where(keep & (va == 0), 1, 0).astype(F32), V)
    has_hot = _has(hot, V)
    assert (has_hot[:, :V - 1] == 0).all()
    full = np.ones((B, n), bool)
    want = _check(hot, has_hot, full, 0, what="one bin")
    assert (want[0][:, V - 1] == (lens > 0).sum()).all() and (want[0].sum(axis=1) == want[0][:, V - 1]).all()
    ids = np.tile(np.arange(n, dtype=np.int64), (2, 1))
    for on_dev in (False, True):
        rc, c, t = _raw_ids(dev, V, ids, 0, 1, on_dev)
        assert rc == nat.VS_OK and (c[0] == has.sum(axis=0)).all() and (c[1] == c[0]).all() and (t == n).all()


# ---- plan and batch ------------------------------------------------------------------------------------------------------------------------------
_big = {}


def _big_index():
    if not _big:
        V, n = 300, 4 * 2048
        rng = np.random.default_rng(77)
        ip, ix, va = ref.csr_case(rng.integers(0, 13, size=n), V, seed=78, zeros=0.05)
        _big["case"] = (ip, ix, va, V)
    return _big["case"]


@pytest.mark.parametrize("n_rows,chunks", [(3 * 2048 + 1, 4), (4 * 2048, 4)])
def test_the_result_never_depends_on_the_plan(n_rows, chunks):
    ip, ix, va, V = _big_index()
    dev = _build(ip[:n_rows + 1], ix[:ip[n_rows]], va[:ip[n_rows]], V)
    has = _has(dev, V)
    assert term_plan(n_rows, 9, V, True, 2048)[1:] == (chunks, 2048) and term_plan(n_rows, 9, V, True, 64)[1] == (n_rows + 63) // 64
    for B in (1, 2, 9):
        masks = _masks(B, n_rows, B + 20, density=0.7)
        masks[:, -1] = True                                                            # the one-row chunk holds a member
        res = [_check(dev, has, masks, 33 if B == 2 else 0, rpc=rpc, what=("plan", B)) for rpc in (64, 2048, 0)]
        for r in res[1:]:
            assert all((a == b).all() for a, b in zip(r, res[0]))
    shared = _masks(1, n_rows, 31, density=0.5)
    for bit0 in (0, 33):
        _check(dev, has, shared, bit0, shared=True, rpc=2048, what="shared")


# ---- against existing code, and under mutations ----------------------------------------------------------------------------------------------------
def test_no_filter_equals_doc_freq_over_all_columns():
    n, V = 1000, 5000
    ip, ix, va = rref.csr_case(n, V, seed=1041)
    dev = DeviceIndex.from_csr(ip, ix, va, V, store_dtype=nat.VS_F32)
    dev.delete_rows(np.array([0, 31, 32, 500, 998, 999]))
    res = dev.term_counts()
    assert isinstance(res, TermCounts) and res.counts.shape == (1, V) and res.counts.dtype == torch.int64 and int(res.total[0]) == n - 6 == dev.n_live
    df = torch.cat([dev.doc_freq(np.arange(c0, min(c0 + 4096, V)), live_only=True) for c0 in range(0, V, 4096)])
    assert (res.counts[0] == df).all() and int(df.sum()) > 0


def _sparse_index(ip, ix, va, n, V):
    from vsearch_amd.ir import SparseIndex
    sp = SparseIndex(device="cuda:0", fp16=False)
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(va), size=(n, V))
    sp.move_to_device("cuda:0")
    return sp


def test_deleted_rows_never_count_through_restore_compact_and_add():
    n, V = 600, 400
    ip, ix, va = rref.csr_case(n, V, seed=1042)
    has = ref.has_matrix(ip, ix, va, V)
    sp = _sparse_index(ip, ix, va, n, V)
    every = ref.term_counts(None, 0, 0, has)
    assert all((_np(g) == w).all() for g, w in zip(sp.term_counts(), every))
    dead = np.array([0, 5, 31, 32, 64, 500, 599])
    live = np.ones(n, bool)
    live[dead] = False
    sp.delete(dead)
    lw = ref.pack(live[None, :])[0]
    assert all((_np(g) == w).all() for g, w in zip(sp.term_counts(), ref.term_counts(None, 0, 0, has, lw)))
    masks = _masks(3, n, 9)
    masks[:, dead] = True                                                              # the set names the deleted rows: they still do not count
    want = ref.term_counts(ref.pack(masks), 1, 0, has, lw)
    got = sp.term_counts(filter=DocFilter.from_mask(torch.from_numpy(masks)))
    assert all((_np(g) == w).all() for g, w in zip(got, want)) and (want[1] < masks.sum(axis=1)).all()
    ids = np.array([[0, 1, 5, 1, -1, 599, 2]], dtype=np.int64)                          # deleted ids are skipped, 1 counts twice
    got = sp.term_counts(ids=ids)
    want = ref.term_counts_ids(ids, 0, has, live)
    assert all((_np(g) == w).all() for g, w in zip(got, want)) and int(got.total[0]) == 3
    sp.restore()
    assert all((_np(g) == w).all() for g, w in zip(sp.term_counts(), every))
    sp.delete(dead)
    old = _np(sp.compact())
    assert (old == np.flatnonzero(live)).all()
    after = ref.term_counts(None, 0, 0, has[live])
    assert all((_np(g) == w).all() for g, w in zip(sp.term_counts(), after))
    new = torch.zeros(3, V)
    new[:, 5] = 1.0
    new[1, 7] = 2.0
    sp.add(new)
    want = (after[0].copy(), after[1] + 3)
    want[0][0, 5] += 3
    want[0][0, 7] += 1
    assert all((_np(g) == w).all() for g, w in zip(sp.term_counts(), want))
    sp.delete(np.array([n - dead.size]))                                               # the first added row
    want[0][0, 5] -= 1
    assert (_np(sp.term_counts().counts) == want[0]).all()


# ---- id lists --------------------------------------------------------------------------------------------------------------------------------------
_ids_case = {}


def _ids_index():
    if not _ids_case:
        n, V = 1000, 2000
        ip, ix, va = rref.csr_case(n, V, seed=1043)
        dev = DeviceIndex.from_csr(ip, ix, va, V, store_dtype=nat.VS_F16)
        dead = np.array([3, 64, 999])
        dev.delete_rows(dead)
        live = np.ones(n, bool)
        live[dead] = False
        _ids_case["case"] = (dev, _has(dev, V), live, n, V)
    return _ids_case["case"]


@pytest.mark.parametrize("m", [1, 63, 64, 65, 1024])
def test_id_lists(m):
    dev, has, live, n, V = _ids_index()
    B = 3
    rng = np.random.default_rng(m)
    ids = rng.integers(0, n, size=(B, m)).astype(np.int64)
    ids[rng.random((B, m)) < 0.2] = -1                                                 # padding anywhere in the list
    ids[0, 0] = 3                                                                      # a deleted id
    ids[1, -1] = ids[1, 0] = 7                                                         # a repeated id counts twice (m = 1: once)
    ids[2, m // 2] = 999
    off = 100_000
    want = ref.term_counts_ids(ids, 0, has, live)
    assert want[1][1] >= min(m, 2) and want[1][0] < m
    for on_dev in (False, True):
        for o in (0, off):
            rc, c, t = _raw_ids(dev, V, ids + np.where(ids >= 0, o, 0), o, 1, on_dev, ld=m + 2)
            assert rc == nat.VS_OK and (c == want[0]).all() and (t == want[1]).all(), (m, on_dev, o)
    # ids outside the index
    out = ids.copy()
    out[1, 0] = n
    out[2, -1] = -2
    want_out = ref.term_counts_ids(out, 0, has, live)
    rc, c, t = _raw_ids(dev, V, out, 0, 1, False)
    assert rc == nat.VS_EINVAL and "outside" in nat.last_error()                       # strict, a host list
    for on_dev, strict in ((False, 0), (True, 0), (True, 1)):                          # skipped: not strict, or a device list
        rc, c, t = _raw_ids(dev, V, out, 0, strict, on_dev)
        assert rc == nat.VS_OK and (c == want_out[0]).all() and (t == want_out[1]).all(), (m, on_dev, strict)
    got = dev.term_counts(ids=ids)                                                     # the facade: host list in, tensors out
    assert all((_np(g) == w).all() for g, w in zip(got, want))
    got = dev.term_counts(ids=torch.from_numpy(ids).cuda())
    assert all((_np(g) == w).all() for g, w in zip(got, want))
    with pytest.raises(ValueError, match="outside"):
        dev.term_counts(ids=out)


# ---- top-n -----------------------------------------------------------------------------------------------------------------------------------------
def _topn_both(counts, total, bg, bg_total, n, method, min_count=1):
    want = ref.topn(counts, total, bg, bg_total, n, method, min_count)
    B, V = counts.shape
    for on_dev in (False, True):
        arrs = dict(counts=np.full((B, V + PAD), JUNK, np.int64), total=np.ascontiguousarray(total, dtype=np.int64), bg=np.ascontiguousarray(bg, dtype=np.int64),
                    cols=np.full((B, n), 77, np.int32), score=np.full((B, n), 7.0, F32), fg=np.full((B, n), JUNK, np.int64), bgo=np.full((B, n), JUNK, np.int64))
        arrs["counts"][:, :V] = counts
        arrs, ptr = _bufs(arrs, on_dev)
        nat.check(nat.lib().vs_term_topn(ptr(arrs["counts"]), V + PAD, ptr(arrs["total"]), B, V, ptr(arrs["bg"]), int(bg_total), method, n, min_count,
                                         ptr(arrs["cols"]), ptr(arrs["score"]), ptr(arrs["fg"]), ptr(arrs["bgo"]), 0, None))
        got = tuple(_np(arrs[k]) for k in ("cols", "score", "fg", "bgo"))
        assert (got[0] == want[0]).all(), (n, method, min_count, on_dev, np.argwhere(got[0] != want[0])[:5])
        assert (got[1].view(np.uint32) == want[1].view(np.uint32)).all(), (n, method, on_dev)
        assert (got[2] == want[2]).all() and (got[3] == want[3]).all(), (n, method, on_dev)
    return want


@pytest.mark.parametrize("method", [ref.LIFT, ref.JLH])
@pytest.mark.parametrize("n", [1, 64, 65, 1024])
def test_topn_sizes(n, method):
    rng = np.random.default_rng(n)
    V = 3000
    counts = rng.integers(0, 40, size=(4, V)).astype(np.int64)                         # few distinct ratios: many ties, some zeros
    bg = rng.integers(0, 60, size=V).astype(np.int64)                                  # zeros in the background
    total = np.array([1000, 37, 0, 1 << 40], dtype=np.int64)                           # query 2: total = 0 lists nothing
    counts[3] = rng.integers(0, 1 << 62, size=V)                                       # conversions that round: values above 2^53
    want = _topn_both(counts, total, bg, 5000, n, method)
    assert (want[0][2] == -1).all() and np.isneginf(want[1][2]).all() and (want[0][0] >= 0).all()
    assert (bg[want[0][0]] > 0).all()
    got = term_topn(torch.from_numpy(counts).cuda(), torch.from_numpy(total).cuda(), torch.from_numpy(bg).cuda(), 5000, n,
                    "jlh" if method == ref.JLH else "lift", device=0)
    assert (_np(got[0]) == want[0]).all() and (_np(got[1]).view(np.uint32) == want[1].view(np.uint32)).all()


def test_topn_ties_floors_and_more_slots_than_columns():
    V = 200
    counts = np.full((2, V), 6, dtype=np.int64)                                        # all scores equal: column ascending
    bg = np.full(V, 12, dtype=np.int64)
    want = _topn_both(counts, [60, 60], bg, 1200, 64, ref.LIFT)
    assert want[0][0].tolist() == list(range(64)) and (want[1] == 10.0).all()
    assert (_topn_both(counts, [60, 60], bg, 120, 64, ref.JLH)[0] == -1).all()          # fgp == bgp: nothing is over-represented
    want = _topn_both(counts[:, :9], [60, 60], bg[:9], 1200, 20, ref.JLH)               # n > n_cols
    assert want[0][0].tolist() == list(range(9)) + [-1] * 11
    # two fp64 scores that differ and round to the same fp32: the column decides
    fg2, bg2 = np.array([[3, 3, 3]]), np.array([1 << 40, (1 << 40) + 1, (1 << 40) + 2])
    assert _topn_both(fg2, [3], bg2, 1 << 41, 3, ref.LIFT)[0].tolist() == [[0, 1, 2]]
    assert _topn_both(fg2[:, ::-1], [3], bg2[::-1].copy(), 1 << 41, 3, ref.LIFT)[0].tolist() == [[0, 1, 2]]
    counts = np.array([[5, 3, 3, 3, 2, 2, 9, 0]], dtype=np.int64)
    bg = np.array([5, 3, 3, 0, 2, 2, 9, 4], dtype=np.int64)
    assert _topn_both(counts, [10], bg, 100, 8, ref.LIFT, min_count=3)[0][0].tolist() == [0, 1, 2, 6, -1, -1, -1, -1]      # bg = 0 skips column 3
    assert _topn_both(counts, [10], bg, 100, 8, ref.LIFT, min_count=4)[0][0].tolist() == [0, 6, -1, -1, -1, -1, -1, -1]
    assert _topn_both(counts, [10], bg, 100, 3, ref.LIFT, min_count=-5)[0][0].tolist() == [0, 1, 2]
    assert (_topn_both(counts, [10], bg, 0, 4, ref.LIFT)[0] == -1).all()               # bg_total = 0
    assert (_topn_both(counts, [0], bg, 100, 4, ref.JLH)[0] == -1).all()               # total = 0


def test_topn_of_the_widest_vocabulary():
    rng = np.random.default_rng(13)
    V = 65535
    counts = rng.integers(0, 5000, size=(2, V)).astype(np.int64)
    bg = rng.integers(1, 50_000, size=V).astype(np.int64)
    counts[1] = np.arange(V)                                                           # ascending scores: every step admits new candidates
    bg[:] = np.where(np.arange(V) % 2 == 0, bg, 7)
    for method in (ref.LIFT, ref.JLH):
        _topn_both(counts, [5000, V], bg, 100_000, 1024, method)


# ---- shards ------------------------------------------------------------------------------------------------------------------------------------------
def test_row_shards_equal_the_unsharded_index():
    n, V, B = 1000, 2000, 9
    ip, ix, va = rref.csr_case(n, V, seed=1044)
    whole = DeviceIndex.from_csr(ip, ix, va, V, store_dtype=nat.VS_F32)
    has = _has(whole, V)
    ndev = torch.cuda.device_count()
    bounds = [0, 437, 770, n]                                       # shard sizes 437, 333, 230: none a multiple of 32
    shards = [whole.slice_rows(bounds[i], bounds[i + 1] - bounds[i], device=i if ndev >= 3 else 0) for i in range(3)]
    group = ShardGroup(shards)
    masks = _masks(B, n, 31)
    flt = DocFilter.from_mask(torch.from_numpy(masks))
    words = ref.pack(masks)
    rng = np.random.default_rng(32)
    ids = rng.integers(-1, n, size=(B, 70)).astype(np.int64)
    ids[:, :6] = (436, 437, 769, 770, 999, 437)                      # the seams, one of them twice
    dead = np.array([3, 436, 437, 769, 770, 999])
    live = np.ones(n, bool)
    try:
        for deleted in (False, True):
            if deleted:
                live[dead] = False
                group.delete_rows(dead)
                whole.delete_rows(dead)
            lw = ref.pack(live[None, :])[0]
            want = ref.term_counts(words, words.shape[1], 0, has, lw)
            for obj in (group, whole):
                assert all((_np(g) == w).all() for g, w in zip(obj.term_counts(filter=flt), want))
                assert all((_np(g) == w).all() for g, w in zip(obj.term_counts(), ref.term_counts(None, 0, 0, has, lw)))
                for given in (ids, torch.from_numpy(ids).cuda()):
                    assert all((_np(g) == w).all() for g, w in zip(obj.term_counts(ids=given), ref.term_counts_ids(ids, 0, has, live)))
            bg = ref.term_counts(None, 0, 0, has, lw)
            for method, code in (("jlh", ref.JLH), ("lift", ref.LIFT)):        # the top-n is taken after the sum, never per shard
                wt = ref.topn(want[0], want[1], bg[0][0], int(bg[1][0]), 8, code, 2)
                for obj in (group, whole):
                    top = obj.top_terms(filter=flt, topn=8, method=method, min_count=2)
                    assert isinstance(top, TopTerms) and (_np(top.cols) == wt[0]).all() and (_np(top.df) == wt[2]).all() and (_np(top.bg) == wt[3]).all()
                    assert (_np(top.scores).view(np.uint32) == wt[1].view(np.uint32)).all() and (_np(top.total) == want[1]).all()
        with pytest.raises(ValueError, match="outside"):
            group.term_counts(ids=np.array([[0, n]], dtype=np.int64))
    finally:
        group.restore_rows()
        group.close()


# ---- the facade -----------------------------------------------------------------------------------------------------------------------------------
def test_index_facade():
    n, V, B = 1000, 2000, 9
    ip, ix, va = rref.csr_case(n, V, seed=1045)
    q = rref.sparse_queries(B, V, seed=n + 2)
    S = rref.scores(q, ip, ix, va, "fp32")
    tq = torch.from_numpy(q)
    sp = _sparse_index(ip, ix, va, n, V)
    has = ref.has_matrix(ip, ix, va, V)
    thr = np.array([np.sort(S[b])[::-1][150] for b in range(B)], dtype=F32)
    bg = ref.term_counts(None, 0, 0, has)
    # q_embs + min_score: the set is match_filter's
    mf = sp.match_filter(tq, thr)
    w = _np(mf.words).view(np.uint32)
    want = ref.term_counts(w, w.shape[1], 0, has)
    got = sp.term_counts(tq, thr)
    assert isinstance(got, TermCounts) and all((_np(g) == x).all() for g, x in zip(got, want))
    assert (_np(got.total) == _np(sp.count_matches(tq, thr))).all() and (want[1] > 100).all()
    for method, code in (("jlh", ref.JLH), ("lift", ref.LIFT)):
        top = sp.significant_terms(tq, thr, topn=12, method=method, min_count=2)
        wt = ref.topn(want[0], want[1], bg[0][0], n, 12, code, 2)
        assert isinstance(top, TopTerms) and (_np(top.cols) == wt[0]).all() and (_np(top.scores).view(np.uint32) == wt[1].view(np.uint32)).all()
        assert (_np(top.df) == wt[2]).all() and (_np(top.bg) == wt[3]).all() and (_np(top.total) == want[1]).all()
    # a caller's background: paid once, and it decides the scores
    kept = sp.term_counts()
    assert all((_np(g) == x).all() for g, x in zip(kept, bg))
    again = sp.significant_terms(tq, thr, topn=12, min_count=2, background=kept)
    assert all((_np(a) == _np(b)).all() for a, b in zip(again, sp.significant_terms(tq, thr, topn=12, min_count=2)))
    half = TermCounts(torch.from_numpy(ref.term_counts(None, 0, 0, has[:500])[0]), torch.tensor([500]))
    top = sp.significant_terms(tq, thr, topn=5, method="lift", background=half)
    wt = ref.topn(want[0], want[1], _np(half.counts)[0], 500, 5, ref.LIFT)
    assert (_np(top.cols) == wt[0]).all() and (_np(top.bg) == wt[3]).all()
    # filter alone: B = 1
    cols = _np(sp.get_vectors(torch.tensor([3])).col_indices())
    col = int(cols[_np(sp.doc_freq(cols)).argmax()])
    visible = np.random.default_rng(42).random(n) < 0.7
    f = sp.term_filter(must=[col]) & DocFilter.from_mask(torch.from_numpy(visible))
    allowed = (has[:, col] & visible)[None, :]
    want_f = ref.term_counts(ref.pack(allowed), 0, 0, has)
    got = sp.term_counts(filter=f)
    assert all((_np(g) == x).all() for g, x in zip(got, want_f)) and 0 < int(got.total[0]) < n and int(got.counts[0, col]) == int(got.total[0])
    top = sp.significant_terms(filter=f, topn=3, method="lift")
    assert (_np(top.cols) == ref.topn(want_f[0], want_f[1], bg[0][0], n, 3, ref.LIFT)[0]).all()
    # ids = res.ids: the terms of a hit list
    res = sp.search(tq, 50)
    want_i = ref.term_counts_ids(_np(res.ids), 0, has)
    got = sp.term_counts(ids=res.ids)
    assert all((_np(g) == x).all() for g, x in zip(got, want_i)) and (_np(got.total) == 50).all()
    top = sp.significant_terms(ids=res.ids, topn=10)
    wt = ref.topn(want_i[0], want_i[1], bg[0][0], n, 10, ref.JLH)
    assert (_np(top.cols) == wt[0]).all() and (_np(top.scores).view(np.uint32) == wt[1].view(np.uint32)).all()
    with pytest.raises(IndexError):
        sp.term_counts(ids=torch.tensor([[0, n]]))
    # method = "count": vs_facet_topn over the counts, the exact integers
    top = sp.significant_terms(tq, thr, topn=7, method="count", min_count=3)
    fl, fc = facet_topn(torch.from_numpy(want[0]).cuda(), 7, 3, device=0)
    assert (_np(top.cols) == _np(fl)).all() and (_np(top.df) == _np(fc)).all() and (_np(top.bg) == 0).all()
    assert (_np(top.scores)[_np(fl) >= 0] == _np(fc)[_np(fl) >= 0].astype(F32)).all()
    top = sp.significant_terms(tq, thr, topn=7, method="count", background=kept)
    assert (_np(top.bg) == bg[0][0][_np(top.cols)]).all()
    # a row-sharded index gives the same answers
    one = tuple(_np(t) for t in sp.significant_terms(tq, thr, topn=12, min_count=2))
    sp.shard_rows([0, 0, 0])
    assert sp.shards is not None and len(sp.shards) == 3
    assert all((_np(g) == x).all() for g, x in zip(sp.term_counts(tq, thr), want))
    assert all((_np(g) == x).all() for g, x in zip(sp.significant_terms(tq, thr, topn=12, min_count=2), one))
    assert all((_np(g) == x).all() for g, x in zip(sp.term_counts(ids=res.ids), want_i))


def test_a_dense_index_on_the_matrix_cores_is_not_supported():
    mat = np.random.default_rng(3).random((64, 96)).astype(F32)
    dev = DeviceIndex.from_dense(mat)
    with pytest.raises(NotImplementedError):
        dev.term_counts()
    with pytest.raises(NotImplementedError):
        dev.term_counts(ids=np.array([[0, 1]], dtype=np.int64))


# ---- the retriever -----------------------------------------------------------------------------------------------------------------------------
def test_retriever_significant_terms(tiny_retriever):
    from vsearch_amd.ir.retriever.index import IndexType
    r = tiny_retriever
    n = 80
    texts = make_texts(n, 5)
    r.build_index(texts, index_type=IndexType.SPARSE)
    idx = r.index
    queries = make_texts(4, 9)
    shift = int(r.encoder_p.config.shift_vocab_num)
    tokens = lambda cols: FakeTokenizer().convert_ids_to_tokens([int(c) + shift for c in cols])
    # k: the set is retrieve's hits
    hits = r.retrieve(queries, k=10)
    top = idx.significant_terms(ids=hits.ids, topn=6, min_count=2)
    got = r.significant_terms(queries, k=10, topn=6, min_count=2)
    assert len(got) == 4
    for b in range(4):
        cols = _np(top.cols)[b]
        keep = cols >= 0
        assert [t for t, _, _, _ in got[b]] == tokens(cols[keep])
        assert [(s, d, g) for _, s, d, g in got[b]] == list(zip(_np(top.scores)[b][keep].tolist(), _np(top.df)[b][keep].tolist(), _np(top.bg)[b][keep].tolist()))
        assert all(d >= 2 and g >= d for _, _, d, g in got[b])                         # the hits are documents of the background too
    assert any(got)
    # min_score: the match set, with a term constraint acting through it
    q_emb = r.process_query(queries, 0, r.encoder_q.config.topk)
    sc = _np(idx.explain(q_emb, torch.arange(n).repeat(4, 1), topn=0).scores).astype(F32)
    thr = np.array([np.unique(sc[b])[np.unique(sc[b]).size // 2] for b in range(4)], dtype=F32)
    got = r.significant_terms(queries, min_score=thr, topn=5, method="lift")
    top = idx.significant_terms(q_emb, thr, topn=5, method="lift")
    assert (_np(top.total) == _np(r.retrieve_range(queries, thr, max_hits=0).counts)).all()
    for b in range(4):
        assert [t for t, _, _, _ in got[b]] == tokens(_np(top.cols)[b][_np(top.cols)[b] >= 0])
    cols = _np(idx.get_vectors(torch.tensor([3])).col_indices())
    col = int(cols[_np(idx.doc_freq(cols)).argmin()])
    got = r.significant_terms(queries, min_score=-np.inf, topn=400, method="count", must=[col])
    n_must = int(_np(idx.doc_freq([col]))[0])
    assert all(dict((t, d) for t, _, d, _ in g)[tokens([col])[0]] == n_must for g in got)      # every document of the set has the must term
