"""GPU tests of the per-label term aggregations (vs_label_order / vs_index_label_term_sums / vs_index_label_term_counts; DeviceIndex / ShardGroup
.label_term_sums / .label_term_counts / .label_order, Index.term_sums_by_facet / .centroids_by_facet / .centroid_terms_by_facet /
.significant_terms_by_facet, Retriever.facet_terms, and the k-means update that goes through them) -- run on MI355X.

The contract is tests/_label_term_ref.py.  Every output is an integer, so everything compares with ==.  Expected values come
from the reference applied to what get_rows returns for the same index.  The raw calls go into junk-filled outputs whose matrix rows carry spare
columns (ld = n_cols + 3) that must keep their junk, once on host buffers and once on device buffers.  The label order's segments are compared
sorted: the order inside a label is unspecified."""
import ctypes as C

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, LabelOrder, LabelTermCounts, LabelTermSums, ShardGroup, TopTerms, TopWeights, label_term_plan
from vsearch_amd.doc_filter import DocFilter
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

import _cluster_ref as cref
import _label_term_ref as ref
import _range_ref as rref
import _term_agg_ref as aref
import _term_sum_ref as tref
from _facet_ref import masks_case

pytestmark = pytest.mark.gpu

TILE = nat.TERM_SUM_TILE_COLS
JUNK = -0x5A5A5A5A5A5A5A5B
PAD = 3                       # spare columns of a matrix row
F32 = np.float32
STORES = {"fp32": nat.VS_F32, "fp16": nat.VS_F16, "bin": nat.VS_NONE}
ONE = ref.ONE
FN = {"sums": "vs_index_label_term_sums", "counts": "vs_index_label_term_counts"}


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _build(ip, ix, va, V, store="fp32"):
    return DeviceIndex.from_csr(ip, ix, None if store == "bin" else va, V, store_dtype=STORES[store])


def _rows(dev):
    return dev.get_rows(np.arange(dev.n_rows, dtype=np.int64))


def _view(dev, V):
    """the reference's view of the index: (Cells, has matrix) of the cells get_rows returns for every row"""
    rows = _rows(dev)
    return tref.Cells(*rows, V), aref.has_matrix(*rows, V)


def _generic(va, seed):
    """fp32 values fx has to round: the case generators' sixteenths times a random factor"""
    rng = np.random.default_rng(seed)
    return (va * (0.5 + rng.random(va.size)).astype(F32)).astype(F32)


def _bufs(arrs, on_dev):
    if on_dev:
        arrs = {k: torch.from_numpy(v).cuda() for k, v in arrs.items()}
        torch.cuda.synchronize()
        return arrs, (lambda t: C.c_void_p(t.data_ptr()))
    return arrs, (lambda a: C.c_void_p(a.ctypes.data))


def _raw(dev, what, V, words, bit0, labels, L, rpi, tc, on_dev):
    """vs_index_label_term_sums / _counts into junk-filled outputs, host or device buffers throughout -> (matrix, total, other)"""
    arrs = dict(out=np.full((L, V + PAD), JUNK, np.int64), total=np.full(L, JUNK, np.int64), other=np.full(1, JUNK, np.int64),
                labels=np.ascontiguousarray(labels, dtype=np.int32))
    if words is not None:
        arrs["words"] = np.ascontiguousarray(words).view(np.int32)
    arrs, ptr = _bufs(arrs, on_dev)
    nat.check(getattr(nat.lib(), FN[what])(dev._h, ptr(arrs["words"]) if words is not None else None, bit0, ptr(arrs["labels"]), L, rpi, tc,
                                           ptr(arrs["out"]), V + PAD, ptr(arrs["total"]), ptr(arrs["other"]), None))
    out = _np(arrs["out"])
    assert (out[:, V:] == JUNK).all(), "a matrix row's spare columns were written"
    return out[:, :V], _np(arrs["total"]), int(_np(arrs["other"])[0])


def _raw_order(dev, words, bit0, labels, L, on_dev):
    """vs_label_order into junk-filled outputs -> (ptr, the listed rows, other)"""
    n = dev.n_rows
    arrs = dict(ptr=np.full(L + 1, JUNK, np.int64), rows=np.full(n, 0x7FFFFFF0, np.int32), other=np.full(1, JUNK, np.int64),
                labels=np.ascontiguousarray(labels, dtype=np.int32))
    if words is not None:
        arrs["words"] = np.ascontiguousarray(words).view(np.int32)
    arrs, ptr = _bufs(arrs, on_dev)
    nat.check(nat.lib().vs_label_order(dev._h, ptr(arrs["words"]) if words is not None else None, bit0, ptr(arrs["labels"]), L, ptr(arrs["ptr"]),
                                       ptr(arrs["rows"]), ptr(arrs["other"]), None))
    p = _np(arrs["ptr"])
    return p, _np(arrs["rows"]).view(np.uint32).astype(np.int64)[:int(p[-1])], int(_np(arrs["other"])[0])


def _check(dev, view, mask, bit0, labels, L, live=None, rpi=0, tc=0, what=None, kinds=(False, True), order=True):
    """one set `mask` [n] (None: words = NULL) packed at bit0 with every spare bit set -> sums, counts and the order, both buffer kinds,
    against the reference -> (sums, counts, total, other)"""
    cells, has = view
    V, n = cells.n_cols, cells.n_rows
    words = None if mask is None else ref.pack(mask[None, :], bit0, spare=1)[0]
    lw = ref.pack(live[None, :])[0] if live is not None else None
    want_s = ref.label_term_sums(words, bit0, labels, L, cells, lw)
    want_c = ref.label_term_counts(words, bit0, labels, L, has, lw)
    want_o = ref.label_order(words, bit0, labels, L, lw)
    size = int((np.ones(n, bool) if mask is None else mask)[np.ones(n, bool) if live is None else live].sum())
    assert int(want_s[1].sum()) + want_s[2] == size and (want_s[1] == want_c[1]).all()
    for on_dev in kinds:
        for name, want in (("sums", want_s), ("counts", want_c)):
            got = _raw(dev, name, V, words, bit0, labels, L, rpi, tc, on_dev)
            assert got[0].dtype == np.int64 and (got[0] == want[0]).all(), (what, name, on_dev, bit0, rpi, tc, np.argwhere(got[0] != want[0])[:5])
            assert (got[1] == want[1]).all() and got[2] == want[2], (what, name, "total / other", on_dev, bit0, got[1:], want[1:])
        if order:
            p, r, o = _raw_order(dev, words, bit0, labels, L, on_dev)
            assert (p == want_o[0]).all() and o == want_o[2] and (ref.sorted_segments(p, r) == want_o[1]).all(), (what, "order", on_dev, bit0)
    return want_s[0], want_c[0], want_s[1], want_s[2]


def _labels(n, L, seed, outside=0.15):
    """random labels in [0, L) with a share outside: -1 ("no label") and values >= L"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, L, size=n).astype(np.int32)
    out = rng.random(n) < outside
    lab[out] = np.where(rng.random(int(out.sum())) < 0.5, -1, L + rng.integers(0, 5, size=int(out.sum())))
    return lab


# ---- shapes and labels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 7])
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 2047, 2048, 2049])
def test_rows_and_labels_at_the_step_and_span_edges(n_rows, L):
    V = 50
    rng = np.random.default_rng(n_rows + L)
    ip, ix, va = aref.csr_case(rng.integers(0, 13, size=n_rows), V, seed=n_rows, zeros=0.1)
    dev = _build(ip, ix, _generic(va, n_rows), V)
    view = _view(dev, V)
    labels = _labels(n_rows, L, n_rows + 3 * L)
    mask = masks_case(1, n_rows, seed=n_rows + 1, density=0.9)[0]
    mask[-1] = True                                                                    # the last row is a member: the spare bits sit right behind it
    for bit0 in (0, 5, 37):
        _check(dev, view, mask, bit0, labels, L, what="set")                           # every bit outside the rows is set
    got = _check(dev, view, None, 0, labels, L, what="NULL words")
    assert int(got[2].sum()) + got[3] == n_rows
    _check(dev, view, np.zeros(n_rows, bool), 5, labels, L, what="empty")


def test_outside_labels_an_empty_label_one_label_for_all_and_a_label_a_row():
    V, n = 40, 300
    rng = np.random.default_rng(5)
    ip, ix, va = aref.csr_case(rng.integers(0, 20, size=n), V, seed=6, zeros=0.1)
    dev = _build(ip, ix, _generic(va, 7), V)
    view = _view(dev, V)
    mask = masks_case(1, n, seed=8, density=0.8)[0]
    lab = _labels(n, 6, 9, outside=0.3)
    lab[lab == 4] = 2                                                                  # label 4 has no row: an all-zero row, total 0
    s, c, t, o = _check(dev, view, mask, 5, lab, 6, what="outside + empty")
    assert o == int((mask & ((lab < 0) | (lab >= 6))).sum()) > 0 and t[4] == 0 and (s[4] == 0).all() and (c[4] == 0).all()
    one = np.full(n, 3, np.int32)                                                      # one label holds every row
    s, c, t, o = _check(dev, view, mask, 37, one, 5, what="one label")
    assert t.tolist() == [0, 0, 0, int(mask.sum()), 0] and o == 0
    assert (s[3] == tref.term_sums(ref.pack(mask[None, :]), 0, 0, view[0])[0][0]).all()
    own = np.arange(n, dtype=np.int32)                                                 # every row its own label: n_labels == n_rows
    s, c, t, o = _check(dev, view, None, 0, own, n, what="a label a row")
    assert (t == 1).all() and o == 0 and (s[17] == view[0].slice(17, 18).rows_sum([1])).all()
    _check(dev, view, mask, 5, own[::-1].copy(), n, rpi=64, tc=7, what="a label a row, reversed")
    everything_outside = np.full(n, -1, np.int32)
    s, c, t, o = _check(dev, view, mask, 0, everything_outside, 3, what="no label at all")
    assert o == int(mask.sum()) and (s == 0).all() and (t == 0).all()


@pytest.mark.parametrize("L", [ref.LDS_BINS, ref.LDS_BINS + 1])
def test_label_order_on_both_sides_of_the_histogram_boundary(L):
    """16 384 labels are counted and ranked in LDS, 16 385 with global atomics; 8 columns keep n_labels x n_cols inside 2^27"""
    V, n = 8, 3 * 2048 + 77
    assert L * V <= ref.MAX_CELLS
    rng = np.random.default_rng(L)
    ip, ix, va = aref.csr_case(rng.integers(0, 9, size=n), V, seed=L + 1)
    dev = _build(ip, ix, _generic(va, L + 2), V)
    view = _view(dev, V)
    lab = rng.integers(0, L, size=n).astype(np.int32)
    lab[:3] = (0, L - 1, L)                                                            # the first label, the last, the first outside
    lab[100:400] = L - 1                                                               # a run on one label: 64 equal labels a step
    lab[rng.random(n) < 0.05] = -1
    mask = masks_case(1, n, seed=L + 3, density=0.9)[0]
    mask[:3] = True
    s, c, t, o = _check(dev, view, mask, 37, lab, L, what="boundary", kinds=(True,))
    assert t[L - 1] >= 200 and o >= 1 and t[0] >= 1
    _check(dev, view, None, 0, lab, L, what="boundary, NULL", kinds=(True,))


def test_an_all_zero_span_followed_by_a_set_row():
    V, n, L = 50, 2 * 2048 + 70, 4
    rng = np.random.default_rng(11)
    ip, ix, va = aref.csr_case(rng.integers(1, 9, size=n), V, seed=12)
    dev = _build(ip, ix, _generic(va, 13), V)
    view = _view(dev, V)
    lab = _labels(n, L, 14, outside=0.0)
    for rows in ([2048], [4096], [2047, 4096 + 69], [n - 1]):
        m = np.zeros(n, bool)
        m[rows] = True
        for bit0 in (0, 37):
            s, c, t, o = _check(dev, view, m, bit0, lab, L, what=("span", rows))
            assert int(t.sum()) == len(rows) and (s[lab[rows[-1]]] != 0).any()


# ---- the live bitmap ---------------------------------------------------------------------------------------------------------------------------------
def _sparse_index(ip, ix, va, n, V):
    from vsearch_amd.ir import SparseIndex
    sp = SparseIndex(device="cuda:0", fp16=False)
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(np.asarray(ip)), torch.from_numpy(np.asarray(ix).astype(np.int64)), torch.from_numpy(va),
                                        size=(n, V))
    sp.move_to_device("cuda:0")
    return sp


def _eq(got, want):
    return all((_np(g).reshape(-1) == np.asarray(w).reshape(-1)).all() for g, w in zip(got, want))


def test_tombstones_are_read_at_bit_0_whatever_bit0_is():
    V, n, L = 50, 2049, 5
    rng = np.random.default_rng(21)
    ip, ix, va = aref.csr_case(rng.integers(0, 13, size=n), V, seed=22, zeros=0.1)
    dev = _build(ip, ix, _generic(va, 23), V)
    view = _view(dev, V)
    lab = _labels(n, L, 24)
    mask = masks_case(1, n, seed=25, density=0.9)[0]
    dead = np.array([0, 31, 32, 63, 64, 2047, 2048])
    mask[dead] = True                                                                  # the set names the deleted rows: they add nothing
    live = np.ones(n, bool)
    live[dead] = False
    dev.delete_rows(dead)
    for bit0 in (0, 5, 37):
        _check(dev, view, mask, bit0, lab, L, live=live, what="set & live")
    got = _check(dev, view, None, 0, lab, L, live=live, what="NULL & live")
    assert int(got[2].sum()) + got[3] == n - dead.size


def test_deleted_rows_never_contribute_through_restore_compact_and_add():
    n, V, L = 600, 400, 6
    ip, ix, va = rref.csr_case(n, V, seed=1042)
    cells = tref.Cells(ip, ix, va, V)
    sp = _sparse_index(ip, ix, va, n, V)
    lab = _labels(n, L, 31)
    sp.set_facet("kind", lab.clip(-1, L - 1), names=[str(i) for i in range(L)])         # (set_facet takes codes in [-1, L))
    lab = lab.clip(-1, L - 1)
    every = ref.label_term_sums(None, 0, lab, L, cells)
    assert _eq(sp.term_sums_by_facet("kind"), every)
    dead = np.array([0, 5, 31, 32, 64, 500, 599])
    live = np.ones(n, bool)
    live[dead] = False
    sp.delete(dead)
    lw = ref.pack(live[None, :])[0]
    assert _eq(sp.term_sums_by_facet("kind"), ref.label_term_sums(None, 0, lab, L, cells, lw))
    mask = masks_case(1, n, seed=9, density=0.8)[0]
    mask[dead] = True
    want = ref.label_term_sums(ref.pack(mask[None, :])[0], 0, lab, L, cells, lw)
    got = sp.term_sums_by_facet("kind", filter=DocFilter.from_mask(torch.from_numpy(mask)))
    assert _eq(got, want) and int(want[1].sum()) + want[2] == int((mask & live).sum())
    sp.restore()
    assert _eq(sp.term_sums_by_facet("kind"), every)
    sp.delete(dead)
    sp.compact()
    keep = np.flatnonzero(live)
    kept = tref.Cells(*_rows(sp._device_index()), V)
    after = ref.label_term_sums(None, 0, lab[keep], L, kept)
    assert _eq(sp.term_sums_by_facet("kind"), after)
    new = torch.zeros(3, V)
    new[:, 5] = 1.0
    new[1, 7] = -2.5
    sp.add(new, facets={"kind": np.array([2, 2, -1], dtype=np.int32)})
    want = (after[0].copy(), after[1].copy(), after[2] + 1)
    want[0][2, 5] += 2 * ONE
    want[0][2, 7] -= 5 * ONE // 2
    want[1][2] += 2
    assert _eq(sp.term_sums_by_facet("kind"), want)


# ---- the plan and the tiles ----------------------------------------------------------------------------------------------------------------------
def test_segments_around_the_item_size():
    """rows_per_item = 64: segments of R - 1, R, R + 1 and 2 R + 1 rows are one, one, two and three items"""
    V, R = 60, 64
    sizes = [R - 1, R, R + 1, 2 * R + 1, 0, 1]
    lab = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    rng = np.random.default_rng(41)
    lab = lab[rng.permutation(lab.size)]
    n, L = lab.size, len(sizes)
    ip, ix, va = aref.csr_case(rng.integers(0, 20, size=n), V, seed=42, zeros=0.1)
    dev = _build(ip, ix, _generic(va, 43), V)
    view = _view(dev, V)
    tiles, tc, rpi, max_items = label_term_plan(n, L, V, R, 0)
    assert (tiles, tc, rpi, max_items) == ref.plan(n, L, V, R, 0) and ref.n_items(sizes, R) == 1 + 1 + 2 + 3 + 0 + 1 <= max_items
    s, c, t, o = _check(dev, view, None, 0, lab, L, rpi=R, what="segments")
    assert t.tolist() == sizes and o == 0
    for rpi in (128, 0):
        again = _check(dev, view, None, 0, lab, L, rpi=rpi, what="segments", kinds=(True,), order=False)
        assert all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(again, (s, c, t, o)))


_big = {}


def _big_index():
    if not _big:
        V, n = 9000, 3 * 2048 + 1
        rng = np.random.default_rng(77)
        ip, ix, va = aref.csr_case(rng.integers(0, 13, size=n), V, seed=78, zeros=0.05)
        dev = _build(ip, ix, _generic(va, 79), V)
        _big["case"] = (dev, _view(dev, V), n, V)
    return _big["case"]


@pytest.mark.parametrize("L", [3, 70])
def test_no_output_depends_on_the_plan(L):
    dev, view, n, V = _big_index()
    assert label_term_plan(n, L, V, 2048, 4096) == (3, 4096, 2048, 4 + L) and label_term_plan(n, L, V, 64, 0)[:3] == (1, V, 64)
    lab = _labels(n, L, L + 1)
    mask = masks_case(1, n, seed=L + 2, density=0.7)[0]
    mask[-1] = True
    res = [_check(dev, view, mask, 37, lab, L, rpi=rpi, tc=tc, what=("plan", rpi, tc), kinds=(True,), order=False)
           for rpi in (64, 2048, 0) for tc in (0, 4096)]
    for r in res[1:]:
        assert all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(r, res[0]))
    _check(dev, view, mask, 5, lab, L, rpi=2048, tc=4096, what="plan, host buffers", kinds=(False,))


@pytest.mark.parametrize("tc", [1, 7, 8, 40])
def test_explicit_tiles_cut_through_packets(tc):
    """V = 40: a row of 40 cells is 5 packets of 8 ascending ids; tiles of 7 cut inside packets, tiles of 1 leave most lanes with no id inside"""
    V, n, L = 40, 200, 3
    rng = np.random.default_rng(tc)
    lens = rng.integers(0, V + 1, size=n)
    lens[:4] = (40, 39, 8, 0)
    ip, ix, va = aref.csr_case(lens, V, seed=50 + tc, zeros=0.05)
    dev = _build(ip, ix, _generic(va, 51), V)
    view = _view(dev, V)
    assert label_term_plan(n, L, V, 0, tc)[:2] == (-(-V // tc), tc)
    lab = _labels(n, L, 52)
    lab[:4] = (0, 1, 2, 0)
    mask = masks_case(1, n, seed=53, density=0.9)[0]
    mask[:4] = True
    for bit0 in (0, 37):
        _check(dev, view, mask, bit0, lab, L, tc=tc, what="tiles", order=False)


@pytest.mark.parametrize("V", [8, 18432, 18433])
def test_automatic_tiles(V):
    n, L = 40, 3
    rng = np.random.default_rng(V)
    lens = rng.integers(0, min(V, 40) + 1, size=n)
    lens[:2] = (min(V, 40), 0)
    ip, ix, va = aref.csr_case(lens, V, seed=V + 1, zeros=0.05, hot=V - 1)              # every non-empty row carries the last column
    ix[ip[0]] = 0                                                                      # ... and row 0 the first one
    dev = _build(ip, ix, _generic(va, V + 2), V)
    view = _view(dev, V)
    tiles, tile_cols = label_term_plan(n, L, V)[:2]
    assert tiles == -(-V // TILE) and tiles * tile_cols >= V > (tiles - 1) * tile_cols
    lab = _labels(n, L, V + 3, outside=0.1)
    lab[0] = 1
    s, c, t, o = _check(dev, view, None, 0, lab, L, what="columns", kinds=(True,), order=False)
    assert (s[:, V - 1] != 0).any() and s[1, 0] != 0


# ---- stores and values ---------------------------------------------------------------------------------------------------------------------------
EDGE = [2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), 2.0 ** -24, 0.0, -0.0, np.nan, 2.0 ** 20, -(2.0 ** 20), 2.0 ** 21, -(2.0 ** 21), np.inf, -np.inf]
EDGE_FX = [0, 2, 0, 1, 0, 0, 0, 1 << 44, -(1 << 44), 1 << 44, -(1 << 44), 1 << 44, -(1 << 44)]
RAGGED = [0, 1, 7, 8, 9, 768]


def test_fp32_store_with_every_fx_edge_value():
    V, L = 1000, 4
    lens = np.array(RAGGED + [len(EDGE)] + [5] * 40)
    ip, ix, va = aref.csr_case(lens, V, seed=21)
    va = _generic(va, 22)
    r = len(RAGGED)
    ix[ip[r]:ip[r + 1]] = 3 * np.arange(len(EDGE))                                      # row 6: edge value j in column 3 j
    va[ip[r]:ip[r + 1]] = np.array(EDGE, dtype=F32)
    dev = _build(ip, ix, va, V)
    view = _view(dev, V)
    assert (tref.fx(np.array(EDGE, dtype=F32)) == EDGE_FX).all()
    lab = _labels(lens.size, L, 23, outside=0.1)
    lab[:r + 1] = [0, 1, 2, 3, 0, 1, 2]                                                # the edge row alone carries label 2 among the ragged rows
    lab[r + 1:][lab[r + 1:] == 2] = 3
    s, c, t, o = _check(dev, view, None, 0, lab, L, what="fp32")
    assert t[2] == 2 and [int(s[2, 3 * j]) - int(view[0].slice(2, 3).rows_sum([1])[3 * j]) for j in range(len(EDGE))] == EDGE_FX
    nan_col, zero_col = 3 * 6, 3 * 4
    assert c[2, nan_col] >= 1 and s[2, nan_col] == view[0].slice(2, 3).rows_sum([1])[nan_col]      # a NaN is had, and adds nothing
    assert c[2, zero_col] == view[1][2, zero_col]                                                  # a stored +0.0 is not had
    _check(dev, view, masks_case(1, lens.size, seed=24, density=0.9)[0], 37, lab, L, tc=7, what="fp32, 143 tiles", order=False)


@pytest.mark.parametrize("store", ["fp16", "bin"])
def test_fp16_and_binary_stores(store):
    V, L = 1000, 3
    lens = np.array(RAGGED + [4] + [6] * 40)
    ip, ix, va = aref.csr_case(lens, V, seed=31, zeros=0.1)                             # sixteenths: fp16-exact, with stored +0.0 and -0.0
    r = len(RAGGED)
    va[ip[r]:ip[r + 1]] = np.array([2.0 ** -24, -(2.0 ** -24), 65504.0, 2.0 ** -14], dtype=F32)    # fp16's smallest subnormal, largest, smallest normal
    dev = _build(ip, ix, va, V, store)
    view = _view(dev, V)
    lab = _labels(lens.size, L, 32, outside=0.1)
    lab[:r + 1] = 1
    s, c, t, o = _check(dev, view, None, 0, lab, L, what=store)
    if store == "bin":
        assert (s == c * ONE).all() and s.any()                                        # a binary index's sums are its counts x 2^24
    else:
        cols = ix[ip[r]:ip[r + 1]]
        assert view[0].slice(r, r + 1).rows_sum([1])[cols].tolist() == [1, -1, 65504 << 24, 1 << 10]
    mask = masks_case(1, lens.size, seed=33, density=0.9)[0]
    mask[:r + 1] = True
    s, c, t, o = _check(dev, view, mask, 37, lab, L, tc=8, what=store, order=False)
    if store == "bin":
        assert (s == c * ONE).all()


def test_signed_data_whose_column_sum_cancels_to_zero():
    V, n = 40, 130
    rng = np.random.default_rng(41)
    x = _generic(np.ones(n // 2, F32), 42) * 1000
    ip = np.arange(0, 2 * n + 1, 2, dtype=np.int64)
    ix = np.tile(np.array([7, 39], dtype=np.int32), n)
    va = np.empty(2 * n, F32)
    perm = rng.permutation(n)
    va[0::2] = np.concatenate([x, -x])[perm]                                            # column 7: every value and its negative
    va[1::2] = 1.0
    lab = np.empty(n, np.int32)
    lab[np.argsort(perm)] = np.concatenate([np.arange(n // 2) % 2, np.arange(n // 2) % 2])   # a value and its negative share a label
    dev = _build(ip, ix, va, V)
    view = _view(dev, V)
    for tc in (0, 8):
        s, c, t, o = _check(dev, view, None, 0, lab, 2, tc=tc, what="cancel", order=False)
        assert (s[:, 7] == 0).all() and (c[:, 7] == t).all() and (s[:, 39] == t * ONE).all() and np.abs(view[0].fx).max() > ONE


# ---- cross-checks against the calls the composition went through ---------------------------------------------------------------------------------------
def test_each_row_equals_term_sums_and_term_counts_over_from_labels_and_the_set():
    n, V, L = 1000, 2000, 9
    ip, ix, va = rref.csr_case(n, V, seed=1046)
    dev = DeviceIndex.from_csr(ip, ix, va, V, store_dtype=nat.VS_F32)
    lab = torch.from_numpy(_labels(n, L, 61)).cuda()
    mask = masks_case(1, n, seed=62, density=0.8)[0]
    flt = DocFilter.from_mask(torch.from_numpy(mask))
    dev.delete_rows(np.array([3, 64, 999]))
    live = np.ones(n, bool)
    live[[3, 64, 999]] = False
    for f in (None, flt):
        sets = DocFilter.from_labels(lab, np.arange(L, dtype=np.int32))
        sets = sets & f if f is not None else sets
        ts, tc = dev.term_sums(filter=sets), dev.term_counts(filter=sets)
        ls, lc = dev.label_term_sums(lab, L, filter=f), dev.label_term_counts(lab, L, filter=f)
        assert isinstance(ls, LabelTermSums) and isinstance(lc, LabelTermCounts)
        assert torch.equal(ls.sums, ts.sums) and torch.equal(ls.total, ts.total) and torch.equal(lc.counts, tc.counts) and torch.equal(lc.total, tc.total)
        size = int(dev.set_count(filter=f).reshape(-1)[0])
        assert int(ls.total.sum()) + int(ls.other[0]) == size == int(lc.total.sum()) + int(lc.other[0])     # what vs_set_count says of the set
        assert torch.equal(ls.mean().view(torch.int32), ts.mean().view(torch.int32)) and torch.equal(ls.values(), ts.values())
        order = dev.label_order(lab, L, filter=f)
        assert isinstance(order, LabelOrder) and torch.equal(order.ptr[1:] - order.ptr[:-1], ls.total) and torch.equal(order.other, ls.other)
        members = live & (_np(lab) == 3) & (mask if f is not None else True)
        seg = order.rows[int(order.ptr[3]):int(order.ptr[4])]
        assert (np.sort(_np(seg)) == np.flatnonzero(members)).all() and members.any()
    got = dev.label_term_sums(_np(lab), L, filter=mask)                                # numpy labels in -> numpy out
    assert isinstance(got.sums, np.ndarray) and (got.sums == _np(ls.sums)).all() and (got.total == _np(ls.total)).all()


@pytest.mark.parametrize("n_shards", [2, 3, 8])
def test_row_shards_equal_the_unsharded_index(n_shards):
    n, V, L = 1000, 2000, 11
    ip, ix, va = rref.csr_case(n, V, seed=1044)
    whole = DeviceIndex.from_csr(ip, ix, va, V, store_dtype=nat.VS_F32)
    view = _view(whole, V)
    rng = np.random.default_rng(n_shards)
    cuts = np.sort(rng.choice(np.arange(1, n), size=n_shards - 1, replace=False))
    cuts[0] = {2: 437, 3: 33, 8: 31}[n_shards]                       # no multiple of 32 at the first seam
    bounds = [0] + sorted(set(cuts.tolist())) + [n]
    shards = [whole.slice_rows(bounds[i], bounds[i + 1] - bounds[i], device=0) for i in range(len(bounds) - 1)]
    group = ShardGroup(shards)
    labels = _labels(n, L, 71)
    lab = torch.from_numpy(labels).cuda()
    mask = masks_case(1, n, seed=31, density=0.8)[0]
    flt = DocFilter.from_mask(torch.from_numpy(mask))
    words = ref.pack(mask[None, :])[0]
    dead = np.array([3, bounds[1] - 1, bounds[1], n - 1])
    live = np.ones(n, bool)
    try:
        for deleted in (False, True):
            if deleted:
                live[dead] = False
                group.delete_rows(dead)
                whole.delete_rows(dead)
            lw = ref.pack(live[None, :])[0]
            want_s = ref.label_term_sums(words, 0, labels, L, view[0], lw)
            want_c = ref.label_term_counts(words, 0, labels, L, view[1], lw)
            want_o = ref.label_order(words, 0, labels, L, lw)
            for obj in (group, whole):
                assert _eq(obj.label_term_sums(lab, L, filter=flt), want_s) and _eq(obj.label_term_counts(lab, L, filter=flt), want_c)
                assert _eq(obj.label_term_sums(lab, L), ref.label_term_sums(None, 0, labels, L, view[0], lw))
                o = obj.label_order(lab, L, filter=flt)
                assert (_np(o.ptr) == want_o[0]).all() and int(o.other[0]) == want_o[2]
                assert (ref.sorted_segments(_np(o.ptr), _np(o.rows)) == want_o[1]).all()
    finally:
        group.restore_rows()
        group.close()


def test_a_dense_index_on_the_matrix_cores_is_not_supported():
    mat = np.random.default_rng(3).random((64, 96)).astype(F32)
    dev = DeviceIndex.from_dense(mat)
    lab = np.zeros(64, np.int32)
    with pytest.raises(NotImplementedError):
        dev.label_term_sums(lab, 2)
    with pytest.raises(NotImplementedError):
        dev.label_term_counts(lab, 2)
    o = dev.label_order(np.arange(64, dtype=np.int32) % 3, 2)                          # the order needs no packets
    assert _np(o.ptr).tolist() == [0, 22, 43] and int(o.other[0]) == 21


# ---- the facades ------------------------------------------------------------------------------------------------------------------------------------
def test_index_facade():
    n, V, L = 1000, 2000, 6
    ip, ix, va = rref.csr_case(n, V, seed=1045)
    sp = _sparse_index(ip, ix, va, n, V)
    cells, has = tref.Cells(ip, ix, va, V), aref.has_matrix(ip, ix, va, V)
    labels = _labels(n, L, 81).clip(-1, L - 1)
    sp.set_facet("topic", labels, names=[f"t{i}" for i in range(L)])
    every = ref.label_term_sums(None, 0, labels, L, cells)
    got = sp.term_sums_by_facet("topic")
    assert isinstance(got, LabelTermSums) and _eq(got, every)
    assert _eq(sp.term_counts_by_facet("topic"), ref.label_term_counts(None, 0, labels, L, has))
    cen = sp.centroids_by_facet("topic")
    assert cen.dtype == torch.float32 and tuple(cen.shape) == (L, V) and (_np(cen).view(np.uint32) == tref.mean(every[0], every[1]).view(np.uint32)).all()
    res = sp.search(cen, 5)                                                            # the centroids are queries like any other
    assert tuple(res.ids.shape) == (L, 5) and (_np(res.ids) >= 0).all()
    # one query + min_score: the set is match_filter's
    q = rref.sparse_queries(1, V, seed=n + 2)
    S = rref.scores(q, ip, ix, va, "fp32")
    thr = np.array([np.sort(S[0])[::-1][300]], dtype=F32)
    tq = torch.from_numpy(q)
    w = _np(sp.match_filter(tq, thr).words).view(np.uint32)[0]
    want = ref.label_term_sums(w, 0, labels, L, cells)
    got = sp.term_sums_by_facet("topic", tq, thr)
    assert _eq(got, want) and int(got.total.sum()) + int(got.other[0]) == int(_np(sp.count_matches(tq, thr))[0])
    want_c = ref.label_term_counts(w, 0, labels, L, has)
    for min_count, cnt in ((0, None), (3, want_c[0])):
        top = sp.centroid_terms_by_facet("topic", topn=12, min_count=min_count, q_embs=tq, min_score=thr)
        wt = tref.topn(want[0], want[1], 12, cnt, min_count)
        assert isinstance(top, TopWeights) and (_np(top.cols) == wt[0]).all() and (_np(top.scores).view(np.uint32) == wt[1].view(np.uint32)).all()
        assert (_np(top.sums) == wt[2]).all() and (_np(top.total) == want[1]).all()
    bg = aref.term_counts(None, 0, 0, has)
    for method in ("jlh", "lift"):
        top = sp.significant_terms_by_facet("topic", topn=9, method=method, min_count=2, q_embs=tq, min_score=thr)
        wt = aref.topn(want_c[0], want_c[1], bg[0][0], int(bg[1][0]), 9, aref.JLH if method == "jlh" else aref.LIFT, 2)
        assert isinstance(top, TopTerms) and (_np(top.cols) == wt[0]).all() and (_np(top.scores).view(np.uint32) == wt[1].view(np.uint32)).all()
        assert (_np(top.df) == wt[2]).all() and (_np(top.bg) == wt[3]).all()
    top = sp.significant_terms_by_facet("topic", topn=4, method="count", filter=torch.from_numpy(labels >= 0))
    assert tuple(top.cols.shape) == (L, 4) and (_np(top.df)[:, 0] == ref.label_term_counts(None, 0, labels, L, has)[0].max(axis=1)).all()
    # host-side errors: a batch of queries, a per-query filter, an unknown field
    with pytest.raises(ValueError, match="ONE document set"):
        sp.term_sums_by_facet("topic", torch.zeros(2, V), np.zeros(2, F32))
    with pytest.raises(ValueError, match="ONE document set"):
        sp.term_sums_by_facet("topic", filter=DocFilter.from_mask(torch.ones(2, n, dtype=torch.bool)))
    with pytest.raises(KeyError):
        sp.term_sums_by_facet("nope")
    # "groups" serves as a field; a row-sharded index gives the same answers
    sp.set_groups(torch.from_numpy(np.where(labels < 0, L, labels)))
    g = sp.term_sums_by_facet("groups")
    assert tuple(g.sums.shape) == (L + 1, V) and (_np(g.sums)[:L] == every[0]).all() and int(g.other[0]) == 0
    one = tuple(_np(t) for t in sp.centroid_terms_by_facet("topic", topn=12, min_count=3, q_embs=tq, min_score=thr))
    cl = tuple(_np(t) for t in sp.cluster_terms(torch.from_numpy(labels), L, topn=7))
    wt = tref.topn(every[0], every[1], 7)
    assert (cl[0] == wt[0]).all() and (cl[1].view(np.uint32) == wt[1].view(np.uint32)).all() and (cl[3] == every[1]).all()
    sp.shard_rows([0, 0, 0])
    assert sp.shards is not None and len(sp.shards) == 3
    assert _eq(sp.term_sums_by_facet("topic", tq, thr), want)
    assert _eq(sp.centroid_terms_by_facet("topic", topn=12, min_count=3, q_embs=tq, min_score=thr), one)
    assert _eq(sp.cluster_terms(torch.from_numpy(labels), L, topn=7), cl)


def test_retriever_facet_terms(tiny_retriever):
    from vsearch_amd.ir.retriever.index import IndexType
    r = tiny_retriever
    n = 80
    r.build_index(make_texts(n, 5), index_type=IndexType.SPARSE)
    idx = r.index
    codes = (np.arange(n) % 4).astype(np.int32)
    codes[::7] = -1
    idx.set_facet("section", codes, names=["a", "b", "c", "d"])
    shift = int(r.encoder_p.config.shift_vocab_num)
    tokens = lambda cols: FakeTokenizer().convert_ids_to_tokens([int(c) + shift for c in cols])
    got = r.facet_terms("section", topn=5)
    top = idx.centroid_terms_by_facet("section", topn=5)
    assert list(got) == ["a", "b", "c", "d"]
    for l, name in enumerate(got):
        cols = _np(top.cols)[l]
        docs, terms = got[name]
        assert docs == int((codes == l).sum()) == int(top.total[l])
        assert [t for t, _ in terms] == tokens(cols[cols >= 0]) and [s for _, s in terms] == _np(top.scores)[l][cols >= 0].tolist()
    query = make_texts(1, 9)
    q_emb = r.process_query(query, 0, r.encoder_q.config.topk)
    sc = _np(idx.explain(q_emb, torch.arange(n).repeat(1, 1), topn=0).scores).astype(F32)
    thr = np.array([np.unique(sc[0])[np.unique(sc[0]).size // 2]], dtype=F32)
    for method in ("jlh", "count"):
        got = r.facet_terms("section", query, thr, topn=4, method=method)
        top = idx.significant_terms_by_facet("section", topn=4, method=method, q_embs=q_emb, min_score=thr)
        assert sum(d for d, _ in got.values()) + int((codes[sc[0] >= thr[0]] < 0).sum()) == int((sc[0] >= thr[0]).sum())
        for l, name in enumerate(got):
            cols = _np(top.cols)[l]
            assert [t for t, _ in got[name][1]] == tokens(cols[cols >= 0])
    with pytest.raises(ValueError, match="ONE document set"):
        r.facet_terms("section", make_texts(2, 9), np.zeros(2, F32))
    with pytest.raises(ValueError, match="method"):
        r.facet_terms("section", method="tfidf")


# ---- k-means goes through the per-label sums: nothing changed -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_kmeans_with_more_clusters_than_one_old_batch_is_the_reference_loop_bit_for_bit(metric):
    """K = 70 > 64: the update that took two from_labels + term_sums batches is one label_term_sums call (passes before and after the rerouting)"""
    n, V, K = 1500, 200, 70
    ip, ix, va = rref.csr_case(n, V, seed=61)
    sp = _sparse_index(ip, ix, va, n, V)
    rows = _rows(sp._device_index())
    starts = np.random.default_rng(63).choice(np.flatnonzero(np.diff(rows[0]) > 0), size=K, replace=False)
    start = np.zeros((K, V), F32)
    for j, r in enumerate(starts):
        start[j, rows[1][rows[0][r]:rows[0][r + 1]]] = rows[2][rows[0][r]:rows[0][r + 1]]
    want = cref.kmeans(*rows, V, start, 4, metric)
    res = sp.kmeans(K, iters=4, metric=metric, init=torch.from_numpy(starts))
    assert (_np(res.centroids).view(np.uint32) == want[0].view(np.uint32)).all(), "centroids"
    assert (_np(res.labels) == want[1]).all() and (_np(res.values).view(np.uint32) == want[2].view(np.uint32)).all(), "assignment"
    assert (_np(res.counts) == want[3]).all() and res.n_iter == want[4] and list(res.changed) == want[5] and len(want[5]) >= 2
    mask = np.random.default_rng(64).random(n) < 0.6
    mask[starts] = True
    part = sp.kmeans(K, iters=2, metric=metric, init=torch.from_numpy(starts), filter=DocFilter.from_mask(torch.from_numpy(mask)))
    wp = cref.kmeans(*rows, V, start, 2, metric, allowed=mask)
    assert (_np(part.centroids).view(np.uint32) == wp[0].view(np.uint32)).all() and (_np(part.labels) == wp[1]).all()


def test_kmeans_and_cluster_terms_slice_the_labels_beyond_one_calls_cells(monkeypatch):
    """K x V beyond the cells of one call (2^27; lowered here to 16 x V so that K = 70 takes five slices): the update and cluster_terms take a
    slice of the clusters a call and give the integers of one call -- bit for bit the reference loop, and the unsliced answer"""
    from vsearch_amd import device_index as di
    n, V, K = 1500, 200, 70
    ip, ix, va = rref.csr_case(n, V, seed=61)
    sp = _sparse_index(ip, ix, va, n, V)
    rows = _rows(sp._device_index())
    starts = np.random.default_rng(63).choice(np.flatnonzero(np.diff(rows[0]) > 0), size=K, replace=False)
    start = np.zeros((K, V), F32)
    for j, r in enumerate(starts):
        start[j, rows[1][rows[0][r]:rows[0][r + 1]]] = rows[2][rows[0][r]:rows[0][r + 1]]
    whole = sp.kmeans(K, iters=3, init=torch.from_numpy(starts))
    terms = tuple(_np(t) for t in sp.cluster_terms(whole.labels, K, topn=6))
    monkeypatch.setattr(di, "MAX_LABEL_TERM_CELLS", 16 * V)
    assert di.label_term_slices(K, V) == [(0, 16), (16, 16), (32, 16), (48, 16), (64, 6)]
    with pytest.raises(ValueError, match="cells"):                                     # one call for all 70 would be refused: the callers slice
        sp._device_index().label_term_sums(whole.labels, K)
    want = cref.kmeans(*rows, V, start, 3, "l2")
    mask = np.random.default_rng(64).random(n) < 0.6
    mask[starts] = True
    for obj_name in ("index", "sharded"):
        res = sp.kmeans(K, iters=3, init=torch.from_numpy(starts))
        assert (_np(res.centroids).view(np.uint32) == want[0].view(np.uint32)).all() and (_np(res.labels) == want[1]).all(), obj_name
        assert (_np(res.centroids).view(np.uint32) == _np(whole.centroids).view(np.uint32)).all() and list(res.changed) == want[5]
        part = sp.kmeans(K, iters=2, init=torch.from_numpy(starts), filter=DocFilter.from_mask(torch.from_numpy(mask)))
        wp = cref.kmeans(*rows, V, start, 2, "l2", allowed=mask)
        assert (_np(part.centroids).view(np.uint32) == wp[0].view(np.uint32)).all() and (_np(part.labels) == wp[1]).all(), obj_name
        assert _eq(sp.cluster_terms(whole.labels, K, topn=6), terms), obj_name
        if obj_name == "index":
            sp.shard_rows([0, 0, 0])
