"""GPU tests of the aggregations' shared Python path (vsearch_amd/device_index.py: _shard_parts and the combiners) -- run on
MI355X.

Every aggregation is written once over the parts of its object: a DeviceIndex is one part at row 0, a ShardGroup one part a shard.  The
same small index therefore answers three times -- as itself, as a group of that one index, and as a group of row shards cut at 0 | 5 | 101 |
300 (a shard shorter than a 32-bit word, a cut inside a word, a 64-row step crossed) -- and the three answers are equal field by field, bit
pattern by bit pattern; one of them is held against the numpy references, so that the equality is not between three wrong answers.  All
shards sit on device 0.  Everything is an integer or a 32-bit pattern: every comparison is exact."""
import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, ShardGroup
from vsearch_amd.doc_filter import DocFilter

import _cluster_ref as cref
import _facet_ref as fref
import _facet_value_ref as fvref
import _quantile_ref as qref
import _term_agg_ref as taref
import _term_sum_ref as tsref
import _value_ref as vref

pytestmark = pytest.mark.gpu

F32, I32 = np.float32, np.int32
N, V, L, K = 300, 40, 6, 5
CUTS = (0, 5, 101, N)
DEAD = np.array([2, 100, 101, 299])                    # one in the short shard, one on either side of a cut, the last row
FILTERS = ("none", "shared", "per_query")
NAMES = ("whole", "one", "cut")

_case = {}


def _targets():
    """-> (the DeviceIndex, a group of that one index, a group of its row shards), the csr, the live rows; built once, never changed"""
    if not _case:
        lens = np.random.default_rng(7).integers(0, 12, size=N)
        ip, ix, va = taref.csr_case(lens, V, seed=71, zeros=0.05)
        whole = DeviceIndex.from_csr(ip, ix, va, V, store_dtype=nat.VS_F32)
        cut = ShardGroup([whole.slice_rows(CUTS[i], CUTS[i + 1] - CUTS[i], device=0) for i in range(3)])
        one = ShardGroup([whole])
        whole.delete_rows(DEAD)
        cut.delete_rows(DEAD)
        live = np.ones(N, bool)
        live[DEAD] = False
        _case["v"] = ((whole, one, cut), (ip, ix, va), live)
    return _case["v"]


def _sets(kind):
    """-> (filter= as the calls take it, the reference's words, ld): per query 1 has no row in the middle shard, query 2 none in the first"""
    if kind == "none":
        return None, None, 0
    masks = fref.masks_case(3, N, seed=11, density=0.8)
    masks[0, :CUTS[1]] = True
    masks[1, CUTS[1]:CUTS[2]] = False
    masks[2, :CUTS[1]] = False
    if kind == "shared":
        return torch.from_numpy(masks[0]), fref.pack(masks[:1]), 0
    words = fref.pack(masks)
    return DocFilter.from_mask(torch.from_numpy(masks)), words, words.shape[1]


def _values(dtype, seed=3):
    v = vref.values_case(N, dtype, seed=seed, frac_missing=0.15, frac_special=0.1, spread=30)
    v[4] = vref.sentinel(dtype)                         # a missing value in the short shard
    v[[7, 150]] = ((1 << 24) + 1, -(1 << 24) - 1) if dtype == I32 else (np.float32(-0.0), np.float32("inf"))
    return v


def _labels(seed=5):
    lab = fref.labels_case(N, L, seed=seed, frac_none=0.1, frac_big=0.05)
    lab[[0, 6, 200]] = -1
    return lab


def _bits(x):
    """a field as what is compared: its 32-bit patterns where it is float32 (the missing sentinel is a NaN), itself otherwise"""
    if isinstance(x, torch.Tensor):
        return x.view(torch.int32) if x.dtype == torch.float32 else x
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _all_equal(results, what):
    """the three targets' results, field by field -> the first of them"""
    first = results[0]
    for name, res in zip(NAMES[1:], results[1:]):
        assert type(res) is type(first) and len(res) == len(first), (what, name)
        for i, (a, b) in enumerate(zip(first, res)):
            assert type(a) is type(b), (what, name, i)
            if isinstance(a, torch.Tensor):
                assert a.device == b.device and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b)), (what, name, i)
            else:
                assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), (what, name, i)
    return first


def _is(got, want, what):
    """one target's result against the numpy reference: dtype, shape and bit patterns"""
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = _np(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), (what, i)


def _each(call, want, what):
    targets, _, _ = _targets()
    _is(_all_equal([call(t) for t in targets], what), want, what)


@pytest.mark.parametrize("kind", FILTERS)
def test_facets(kind):
    _, _, live = _targets()
    flt, words, ld = _sets(kind)
    lw = fref.pack(live[None, :])[0]
    labels = _labels()
    tl = torch.from_numpy(labels).cuda()
    want = fref.facet_counts(words, ld, 0, N, labels, L, lw)
    assert want[2].min() > 0, "no label of -1 in a set"
    _each(lambda t: t.facet_counts(tl, L, filter=flt), want, ("facet_counts", kind))
    _each(lambda t: t.facet_counts(tl, L, filter=flt, rows_per_chunk=64), want, ("facet_counts, 64 rows a chunk", kind))
    _each(lambda t: t.top_facets(tl, L, 4, filter=flt, min_count=2), fref.topn(want[0], 4, 2) + want[1:], ("top_facets", kind))


@pytest.mark.parametrize("dtype", [F32, I32])
@pytest.mark.parametrize("kind", FILTERS)
def test_values(kind, dtype):
    _, _, live = _targets()
    flt, words, ld = _sets(kind)
    lw = fref.pack(live[None, :])[0]
    v = _values(dtype)
    tv = torch.from_numpy(v).cuda()
    e = vref.edges_case(5, dtype, spread=30)
    want = vref.stats(words, ld, 0, N, v, lw)
    assert want[1].min() > 0, "no missing value in a set"
    _each(lambda t: t.value_stats(tv, filter=flt), want, ("value_stats", kind))
    c, below, above, missing = vref.histogram(words, ld, 0, N, v, e, lw)
    _each(lambda t: t.value_histogram(tv, e, filter=flt), (c, below, above, missing, c.sum(1) + below + above + missing), ("value_histogram", kind))
    for k, descending in ((7, True), (300, False)):                                       # (300: the lists end in id -1 / the missing sentinel)
        _each(lambda t: t.value_topk(tv, k, descending=descending, filter=flt), vref.topk(words, ld, 0, N, v, k, descending, 0, lw),
              ("value_topk", kind, k))
    q = np.array([0.0, 0.3, 0.5, 1.0])
    for method in ("lower", "nearest"):
        _each(lambda t: t.value_quantiles(tv, q=q, method=method, filter=flt), qref.order_statistics(words, ld, 0, N, v, q, method, None, lw),
              ("value_quantiles", kind, method))
    if kind == "per_query":                                                               # the merge skipped the shards in which a set is empty
        sets = vref.inset(words, ld, 0, N, lw)
        assert not sets[1, CUTS[1]:CUTS[2]].any() and not sets[2, :CUTS[1]].any() and (want[0] > 0).all()


@pytest.mark.parametrize("dtype", [F32, I32])
def test_value_range_filter(dtype):
    targets, _, _ = _targets()
    v = _values(dtype)
    tv = torch.from_numpy(v).cuda()
    for lo, hi in ((-2, 3), (None, 0), ([-3, None, 1], [3, 2, None])):
        got = [t.value_range_filter(tv, lo, hi) for t in targets]
        assert all(isinstance(g, DocFilter) and g.n_rows == N and g.per_query == isinstance(lo, list) for g in got)
        words = _all_equal([(g.words,) for g in got], ("value_range_filter", lo, hi))[0]
        open_lo, open_hi = (-np.inf, np.inf) if dtype == F32 else (vref.INT32_MIN + 1, (1 << 31) - 1)
        los = [open_lo if x is None else x for x in (lo if isinstance(lo, list) else [lo])]
        his = [open_hi if x is None else x for x in (hi if isinstance(hi, list) else [hi])]
        want = vref.range_bitmaps(v, los, his)
        assert np.array_equal(_np(words).view(np.uint32).reshape(want.shape), want), (lo, hi)


@pytest.mark.parametrize("dtype", [F32, I32])
@pytest.mark.parametrize("kind", FILTERS)
def test_breakdowns(kind, dtype):
    _, _, live = _targets()
    flt, words, ld = _sets(kind)
    lw = fref.pack(live[None, :])[0]
    labels, v = _labels(), _values(dtype)
    tl, tv = torch.from_numpy(labels).cuda(), torch.from_numpy(v).cuda()
    e = vref.edges_case(5, dtype, spread=30)
    want = fvref.stats(words, ld, 0, N, labels, L, v, lw)
    assert want[1].max() > 0, "no missing value"         # (five rows, six labels: the first shard always has a label without a value)
    _each(lambda t: t.facet_value_stats(tl, L, tv, filter=flt), want, ("facet_value_stats", kind))
    _each(lambda t: t.facet_value_histogram(tl, L, tv, e, filter=flt), fvref.histogram(words, ld, 0, N, labels, L, v, e, lw),
          ("facet_value_histogram", kind))


@pytest.mark.parametrize("kind", FILTERS)
def test_term_aggregations_by_filter(kind):
    _, (ip, ix, va), live = _targets()
    flt, words, ld = _sets(kind)
    lw = fref.pack(live[None, :])[0]
    _each(lambda t: t.term_counts(filter=flt), taref.term_counts(words, ld, 0, taref.has_matrix(ip, ix, va, V), lw), ("term_counts", kind))
    _each(lambda t: t.term_sums(filter=flt), tsref.term_sums(words, ld, 0, tsref.Cells(ip, ix, va, V), lw), ("term_sums", kind))
    _each(lambda t: t.term_sums(filter=flt, rows_per_chunk=64, tile_cols=16), tsref.term_sums(words, ld, 0, tsref.Cells(ip, ix, va, V), lw),
          ("term_sums, 64 rows a chunk", kind))


def test_term_aggregations_by_ids():
    targets, (ip, ix, va), live = _targets()
    ids = np.random.default_rng(13).integers(-1, N, size=(3, 40)).astype(np.int64)
    ids[:, :8] = (4, 5, 100, 101, 299, 5, -1, 2)                                           # the seams, one id twice, a deleted row
    ids[1, 8:] = np.random.default_rng(14).integers(101, N, size=32)                       # a query with nothing in the middle shard
    wide = torch.from_numpy(np.concatenate([ids, np.full((3, 3), -1, np.int64)], axis=1)).cuda()
    for given in (ids, torch.from_numpy(ids), torch.from_numpy(ids).cuda(), wide[:, :40]):    # (the last: a column slice of a wider hit list)
        _each(lambda t: t.term_counts(ids=given), taref.term_counts_ids(ids, 0, taref.has_matrix(ip, ix, va, V), live), "term_counts by ids")
        _each(lambda t: t.term_sums(ids=given), tsref.term_sums_ids(ids, 0, tsref.Cells(ip, ix, va, V), live), "term_sums by ids")
    outside = np.array([[0, N]], dtype=np.int64)
    for t, message in zip(targets, ("outside", r"an id lies outside \[-1, 300\)", r"an id lies outside \[-1, 300\)")):
        with pytest.raises(ValueError, match=message):                                     # the library's message, the groups' own
            t.term_counts(ids=outside)
        with pytest.raises(ValueError, match="not both"):
            t.term_sums(filter=torch.ones(N, dtype=torch.bool), ids=ids)


@pytest.mark.parametrize("kind", ["none", "shared"])
def test_assign(kind):
    targets, (ip, ix, va), live = _targets()
    flt, words, ld = _sets(kind)
    allowed = live & (vref.inset(words, ld, 0, N)[0] if words is not None else True)
    rng = np.random.default_rng(17)
    cen, bias = cref.grid(rng, (K, V)), cref.grid(rng, K)              # (with the cells' multiples of 1 / 16: exact sums in any order)
    for b in (None, bias):
        _each(lambda t: t.assign(cen, bias=b, filter=flt), cref.assign(ip, ix, va, V, cen, b, allowed), ("assign", kind, b is not None))
    for t in targets:
        with pytest.raises(ValueError, match="ONE document set"):
            t.assign(cen, filter=_sets("per_query")[0])


def test_a_column_edited_in_place_changes_the_answer():
    """a group keeps every shard's slice of a label / value tensor until the tensor's version moves; a numpy array is never kept"""
    targets, _, live = _targets()
    lw = fref.pack(live[None, :])[0]
    labels, v = _labels(seed=21), _values(I32, seed=22)
    for t in targets:
        tl, tv = torch.from_numpy(labels.copy()).cuda(), torch.from_numpy(v.copy()).cuda()
        nl, nv = labels.copy(), v.copy()
        _is(t.facet_counts(tl, L), fref.facet_counts(None, 0, 0, N, labels, L, lw), "labels, first")
        _is(t.facet_value_stats(tl, L, tv), fvref.stats(None, 0, 0, N, labels, L, v, lw), "labels and values, first")
        _is(t.value_stats(tv), vref.stats(None, 0, 0, N, v, lw), "values, first")
        first = t.facet_counts(nl, L)
        assert isinstance(first.counts, np.ndarray)                                        # numpy in, numpy out
        _all_equal([first, t.facet_counts(nl, L)], "the same numpy labels twice")
        _is(first, fref.facet_counts(None, 0, 0, N, labels, L, lw), "numpy labels")
        _all_equal([t.value_stats(nv), t.value_stats(nv)], "the same numpy values twice")
        tl[:150] = 1
        tv[3:200] += 5
        nl[:150] = 1
        nv[3:200] += 5
        labels2, v2 = _np(tl), _np(tv)
        want = fref.facet_counts(None, 0, 0, N, labels2, L, lw)
        assert not np.array_equal(want[0], _np(first.counts))
        _is(t.facet_counts(tl, L), want, "labels, edited")
        _is(t.facet_counts(nl, L), want, "numpy labels, edited")
        _is(t.value_stats(tv), vref.stats(None, 0, 0, N, v2, lw), "values, edited")
        _is(t.value_stats(nv), vref.stats(None, 0, 0, N, v2, lw), "numpy values, edited")
        _is(t.facet_value_stats(tl, L, tv), fvref.stats(None, 0, 0, N, labels2, L, v2, lw), "labels and values, edited")
