"""GPU tests of the per-label percentiles (vs_facet_value_quantiles / vs_facet_value_radix_counts and their vs_index_* variants; DeviceIndex /
ShardGroup .facet_value_quantiles, Index.percentiles_by_facet / .median_by_facet, Retriever.retrieve_percentiles_by_facet) -- run on MI355X.

The contract is tests/_facet_quantile_ref.py.  Every result is an integer or a 32-bit pattern, so everything compares exactly:
values as raw 32-bit patterns, everything else as integers.  The raw calls go into junk-filled outputs, on host and on device buffers.  Every
case is a few thousand rows at most; the label counts at which the kernel changes its path are read from vs_facet_value_quantile_plan."""
import ctypes as C

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import (DeviceIndex, FacetValuePercentiles, FacetValueQuantiles, ShardGroup, facet_value_quantile_plan,
                                      value_radix_step)
from vsearch_amd.doc_filter import DocFilter
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

import _facet_quantile_ref as fq
import _facet_ref as fcref
import _facet_value_ref as fref
import _quantile_ref as qref
import _range_ref as rref
import _value_ref as ref

pytestmark = pytest.mark.gpu

F32, I32 = np.float32, np.int32
DTYPES = [F32, I32]
JUNK = -0x5A5A5A5A5A5A5A5B
JUNK32 = 0x5A5A5A5A
Q3 = [0.0, 0.5, 1.0]
T = nat.FACET_QUANTILE_MAX_LABEL_TILES
OUTS = ("vals", "rk", "count", "missing", "total", "other")


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _dt(v):
    return nat.VAL_F32 if v.dtype == F32 else nat.VAL_I32


def _same(got, want, what=None):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert ref.same(_np(g), w), (what, i, _np(g), w)


def _junk(shape, dtype):
    if np.dtype(dtype) == np.int64:
        return np.full(shape, JUNK, np.int64)
    return np.full(shape, JUNK32, np.uint32).view(dtype).reshape(shape)


class _Bufs:
    """inputs and junk-filled outputs of a raw call, host or device buffers throughout"""

    def __init__(self, on_dev, ins, outs):
        self.on_dev = on_dev
        ins = {k: np.ascontiguousarray(v) for k, v in ins.items() if v is not None}
        ins = {k: (v.view(np.int32) if v.dtype == np.uint32 else v) for k, v in ins.items()}
        if on_dev:
            self.ins = {k: torch.from_numpy(v).cuda() for k, v in ins.items()}
            self.outs = {k: torch.from_numpy(v).cuda() for k, v in outs.items()}
            torch.cuda.synchronize()
        else:
            self.ins, self.outs = ins, outs

    def p(self, name):
        t = self.ins.get(name, self.outs.get(name))
        if t is None:
            return None
        return C.c_void_p(t.data_ptr() if self.on_dev else t.ctypes.data)

    def out(self, name):
        return _np(self.outs[name])


def _raw(words, bit0, ld, aw, B, labels, L, v, n, on_dev, q=None, method="lower", ranks=None, rpc=0, index=None):
    """one vs_facet_value_quantiles / vs_index_facet_value_quantiles call -> the six outputs"""
    R = len(q) if q is not None else np.asarray(ranks).shape[2]
    b = _Bufs(on_dev, dict(words=words, aw=aw, labels=np.asarray(labels, I32), v=v, q=None if q is None else np.asarray(q, np.float64),
                           ranks=None if ranks is None else np.asarray(ranks, np.int64)),
              dict(vals=_junk((B, L, R), v.dtype), rk=_junk((B, L, R), np.int64), count=_junk((B, L), np.int64), missing=_junk((B, L), np.int64),
                   total=_junk(B, np.int64), other=_junk(B, np.int64)))
    outs = [b.p(k) for k in OUTS]
    m = qref.METHODS[method]
    if index is None:
        rc = nat.lib().vs_facet_value_quantiles(b.p("words"), bit0, ld, b.p("aw"), B, b.p("labels"), L, b.p("v"), _dt(v), n, b.p("q"), m, b.p("ranks"),
                                                R, rpc, *outs, 0, None)
    else:
        rc = nat.lib().vs_index_facet_value_quantiles(index._h, b.p("words"), bit0, ld, B, b.p("labels"), L, b.p("v"), _dt(v), b.p("q"), m,
                                                      b.p("ranks"), R, rpc, *outs, None)
    nat.check(rc)
    return tuple(b.out(k) for k in OUTS)


def _check(masks, bit0, labels, L, v, q=None, method="lower", ranks=None, and_mask=None, rpc=0, shared=False, what=None, kinds=(False, True)):
    """per-query sets `masks` [B, n] packed at bit0 with every spare bit set -> the call, both buffer kinds, against the sort per label"""
    B, n = masks.shape
    words = ref.pack(masks, bit0, spare=1)
    aw = ref.pack(and_mask[None, :], bit0, spare=1)[0] if and_mask is not None else None
    ld = 0 if shared else words.shape[1]
    want = fq.order_statistics(words, ld, bit0, n, v, labels, L, q=q, method=method, ranks=ranks, and_words=aw)
    assert (want[2].sum(1) + want[3].sum(1) + want[5] == want[4]).all()
    for on_dev in kinds:
        _same(_raw(words, bit0, ld, aw, B, labels, L, v, n, on_dev, q=q, method=method, ranks=ranks, rpc=rpc), want, (what, on_dev, bit0, rpc, method))
    return want


def _plan(n, B, L, R, per_query=True, rpc=0):
    """the plans of the three levels"""
    return [facet_value_quantile_plan(n, B, L, R, level, per_query, rpc) for level in range(3)]


# ---- row and bit edges, bitmap layouts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 2047, 2048, 2049])
def test_row_and_bit_edges(n_rows, dtype):
    B, L = 3, 5
    v = ref.values_case(n_rows, dtype, seed=n_rows, frac_missing=0.15, frac_special=0.1, spread=30)
    labels = fref.labels_shape("mixed", n_rows, L, n_rows)
    masks = ref.masks_case(B, n_rows, seed=n_rows + 1, density=0.9)
    live = np.random.default_rng(n_rows).random(n_rows) < 0.8
    for bit0 in (0, 5, 37):
        _check(masks, bit0, labels, L, v, q=Q3, method=("lower", "higher", "nearest")[bit0 % 3], and_mask=live, what="edges")
        _check(masks[:1], bit0, labels, L, v, q=Q3, method="nearest", shared=True, what="shared", kinds=(True,))
    aw = ref.pack(live[None, :], 0, spare=1)[0]
    for a in (None, aw):                                                              # words = NULL: every row set
        _same(_raw(None, 0, 0, a, 1, labels, L, v, n_rows, a is None, q=Q3, method="higher"),
              fq.order_statistics(None, 0, 0, n_rows, v, labels, L, q=Q3, method="higher", and_words=a))


@pytest.mark.parametrize("B", [1, 8, 9])
def test_query_tiles_and_ranks(B):
    n = 3000
    for R in (1, 2, 16):
        L = 3 if R == 16 else 4
        dtype = DTYPES[(B + R) & 1]
        v = ref.values_case(n, dtype, seed=B + R)
        labels = fref.labels_shape("random", n, L, B)
        masks = ref.masks_case(B, n, seed=B + 10, density=0.6)
        q = np.linspace(0.0, 1.0, R) if R > 1 else np.array([0.5])
        _check(masks, 31, labels, L, v, q=q, method="nearest", what=("tiles", R), kinds=(True,))
        _check(masks, 0, labels, L, v, q=q, rpc=64, what=("tiles, 64-row chunks", R), kinds=(False,))


# ---- label edges: the plan's tiles and regimes -------------------------------------------------------------------------------------------------------
def _label_edge_counts():
    """-> (tile, n_labels at which the kernel changes its path at level 0 with a shared bitmap and R = 1): 1, 2, one tile less one label /
    exactly / plus one (two tiles, the second holding one label), the last of the LDS regime and the smallest of the global regime -- read from
    vs_facet_value_quantile_plan"""
    plan = lambda L: facet_value_quantile_plan(1000, 1, L, 1, 0, False, 0)
    tile = next(L for L in range(1, 1 << 12) if plan(L + 1)[3] == 2)                   # the most labels of one tile
    first_global = next(L for L in range(tile, 1 << 20, tile) if plan(L + 1)[0] == 1) + 1
    assert plan(first_global - 1)[0] == 0 and plan(first_global - 1)[3] == T and plan(tile + 1)[2:4] == (tile, 2)
    return tile, [1, 2, tile - 1, tile, tile + 1, first_global - 1, first_global]


@pytest.mark.parametrize("kind", ["random", "mixed", "one", "runs64", "runs64_off1"])
def test_label_edges(kind):
    n = 2500
    tile, counts = _label_edge_counts()
    assert facet_value_quantile_plan(n, 1, tile + 1, 1, 0, False)[2:4] == (tile, 2)    # two tiles, the second holding one label
    for i, L in enumerate(counts):
        dtype = DTYPES[i & 1]
        v = ref.values_case(n, dtype, seed=L, frac_missing=0.1, spread=200)
        labels = fref.labels_shape(kind, n, L, seed=L)
        if kind == "mixed":
            labels[:4] = (-1, L, -1, L)                                                # -1 and n_labels, with and without a value
            v[:2] = ref.sentinel(dtype)
        masks = ref.masks_case(2, n, seed=L + 1, density=0.8)
        plans = _plan(n, 2, L, 2)
        assert plans[0][0] == (1 if L == counts[-1] else 0)
        _check(masks, 5, labels, L, v, q=[0.25, 1.0], method="higher", what=(kind, L, plans), kinds=(i % 2 == 0,))
        _check(masks[:1], 0, labels, L, v, q=[0.5], shared=True, what=(kind, L, "shared"), kinds=(True,))


def test_no_label_at_all_and_empty_cells():
    n, L = 1500, 6
    for dtype in DTYPES:
        v = ref.values_case(n, dtype, seed=3)
        masks = ref.masks_case(3, n, seed=4, density=0.7)
        masks[0] = False                                                               # query 0: the empty set
        want = _check(masks, 5, fref.labels_shape("none", n, L), L, v, q=Q3, what="none")
        assert (want[2] == 0).all() and (want[5] == want[4]).all() and ref.is_missing(want[0]).all() and (want[1] == -1).all()
        labels = fref.labels_shape("random", n, L, 5)
        labels[labels == 1] = 0                                                        # label 1: no rows
        v[labels == 2] = ref.sentinel(dtype)                                           # label 2: rows, none with a value
        want = _check(masks, 37, labels, L, v, q=Q3, method="nearest", what="empty cells")
        assert (want[2][:, 1:3] == 0).all() and (want[3][:, 1] == 0).all() and (want[3][1:, 2] > 0).all()
        assert ref.is_missing(want[0][:, 1:3]).all() and (want[1][:, 1:3] == -1).all() and (want[4][0] == 0)


# ---- ranks --------------------------------------------------------------------------------------------------------------------------------------
def test_explicit_ranks_equal_ranks_and_one_bin():
    n, B, L = 2000, 2, 3
    v = ref.values_case(n, I32, seed=8, spread=5, frac_special=0.0)                    # a coarse grid: many ranks fall into one bin
    labels = fref.labels_shape("random", n, L, 9)
    masks = ref.masks_case(B, n, seed=10, density=0.9)
    count = fq.order_statistics(ref.pack(masks), (n + 31) // 32, 0, n, v, labels, L, q=[0.5])[2]
    ranks = np.zeros((B, L, 5), np.int64)
    ranks[:, :, 1] = 1                                                                # two ranks in one bin
    ranks[:, :, 2] = count // 2
    ranks[:, :, 3] = count // 2                                                       # equal ranks
    ranks[:, :, 4] = count                                                            # at the count: no answer
    want = _check(masks, 5, labels, L, v, ranks=ranks, what="ranks")
    assert (want[1][:, :, 4] == -1).all() and (want[1][:, :, :4] == ranks[:, :, :4]).all() and ref.is_missing(want[0][:, :, 4]).all()
    _check(masks, 0, labels, L, v, q=[0.5, 0.5, 0.5000001, 1.0], what="equal quantiles")


# ---- digit edges ----------------------------------------------------------------------------------------------------------------------------------
def _digit_keys(level, dtype):
    """36 keys in three groups of 12; inside a group only the level's digit differs: the lowest and highest bins, their neighbours, the middle"""
    lo, hi = (0, 2047) if dtype == I32 else (4, 2043)
    dlo, dhi = (lo, hi) if level == 0 else (0, 2047 if level == 1 else 1023)
    mid = (dlo + dhi) // 2
    digs = [dlo, dlo + 1, dlo + 2, dlo + 3, mid - 1, mid, mid + 1, mid + 2, dhi - 3, dhi - 2, dhi - 1, dhi]
    keys = []
    for a, c in [(lo, 1), (hi, 1023), (1024, 512)]:
        for d in digs:
            keys.append((d << 21) | (a << 10) | c if level == 0 else (a << 21) | (d << 10) | c if level == 1 else (a << 21) | (c << 10) | d)
    return np.array(keys, np.uint64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("level", [0, 1, 2])
def test_digit_edges(level, dtype):
    keys = _digit_keys(level, dtype)
    v = np.tile(qref.unkey(keys, dtype), 2)                                            # every key under label 0 and label 1
    n, L = v.shape[0], 2
    labels = np.repeat(np.array([0, 1], I32), keys.size)
    perm = np.random.default_rng(level).permutation(n)
    v, labels = v[perm], labels[perm]
    masks = np.ones((2, n), bool)
    masks[1, ::3] = False
    for j0 in (0, 12, 24):
        ranks = np.tile(np.arange(j0, j0 + 12, dtype=np.int64), (2, L, 1))
        want = _check(masks, 5, labels, L, v, ranks=ranks, what=("digits", level, j0), kinds=(j0 != 12,))
        assert (ref.key(want[0][0, 0]) == np.sort(keys)[j0:j0 + 12]).all() and (ref.key(want[0][0, 1]) == np.sort(keys)[j0:j0 + 12]).all()


def test_extremes():
    vi = np.array([ref.INT32_MIN + 1, (1 << 31) - 1, (1 << 24) + 1, ref.INT32_MIN, 0, -1] * 2, I32)
    labels = np.repeat(np.array([1, 0], I32), 6)
    ranks = np.tile(np.arange(6, dtype=np.int64), (1, 2, 1))
    want = _check(np.ones((1, 12), bool), 0, labels, 2, vi, ranks=ranks, what="int extremes")
    assert want[0][0, 0].tolist() == [ref.INT32_MIN + 1, -1, 0, (1 << 24) + 1, (1 << 31) - 1, ref.INT32_MIN] and want[3][0].tolist() == [1, 1]
    den = np.nextafter(F32(0), F32(1))
    vf = np.array([np.inf, -np.inf, -0.0, 0.0, -den, np.nan, 1.1754942e-38, -3.4028235e38] * 2, F32)
    labels = np.repeat(np.array([0, 1], I32), 8)
    ranks = np.tile(np.arange(8, dtype=np.int64), (1, 2, 1))
    want = _check(np.ones((1, 16), bool), 33, labels, 2, vf, ranks=ranks, what="float extremes")
    assert ref.bits(want[0][0, 1, 3:5]).tolist() == [0, 0] and want[0][0, 0, 0] == -np.inf and want[0][0, 0, 6] == np.inf     # of -0.0 / +0.0: +0.0
    assert ref.bits(want[0][0, 0, 7:])[0] == ref.NAN_BITS


# ---- a field of years: every row in one bin at levels 0 and 1 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "runs64"])
def test_years_in_both_regimes(kind):
    n = 6000
    rng = np.random.default_rng(11)
    v = rng.integers(1900, 2030, size=n).astype(I32)
    v[rng.random(n) < 0.05] = ref.INT32_MIN
    k = ref.key(v[v != ref.INT32_MIN])
    assert np.unique(k >> 21).size == 1 and np.unique(k >> 10).size == 1
    masks = ref.masks_case(2, n, seed=12, density=0.5)
    masks[0] = True
    _, counts = _label_edge_counts()
    for L in (12, counts[-1]):                                                         # the LDS regime and the global one
        assert facet_value_quantile_plan(n, 2, L, 3, 0, True)[0] == (0 if L == 12 else 1)
        labels = fref.labels_shape(kind, n, L, 13)
        want = _check(masks, 33, labels, L, v, q=[0.0, 0.5, 1.0], method="nearest", what=("years", kind, L), kinds=(True,))
        if L == 12 and kind == "random":
            assert (want[0][0, :, 0] <= 1902).all() and (want[0][0, :, 2] >= 2027).all()


# ---- chunks and label tiles at once -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_several_chunks_and_label_tiles(dtype):
    n, B = 3 * 2048 + 1, 3
    tile, _ = _label_edge_counts()
    L = 2 * tile + 3
    for R, q in ((1, [0.5]), (3, Q3)):
        plans = _plan(n, B, L, R, True, 2048)
        assert all(p[0] == 0 and p[3] > 1 and p[4:] == (4, 2048) for p in plans), plans
    v = ref.values_case(n, dtype, seed=21, spread=100, frac_special=0.0)
    v[-1] = 5000
    labels = fref.labels_shape("random", n, L, 22)
    labels[-1] = L - 1                                                                # the one-row chunk holds the last tile's largest value
    masks = ref.masks_case(B, n, seed=23, density=0.7)
    masks[:, -1] = True
    for bit0 in (0, 37):
        want = _check(masks, bit0, labels, L, v, q=Q3, rpc=2048, what="chunks x tiles", kinds=(bit0 == 0,))
        assert (want[0][:, L - 1, 2] == v[-1]).all()
    _check(masks, 5, labels, L, v, q=[0.5], rpc=2048, what="chunks x tiles, R = 1", kinds=(True,))


# ---- the level ABI ------------------------------------------------------------------------------------------------------------------------------------
def _level_call(words, bit0, ld, aw, B, labels, L, v, n, level, R, sp, ns, on_dev, rpc=0):
    """one vs_facet_value_radix_counts call into junk -> (counts, missing, total, other)"""
    S, bins = (1 if level == 0 else R), qref.LEVEL_BINS[level]
    b = _Bufs(on_dev, dict(words=words, aw=aw, labels=np.asarray(labels, I32), v=v, sp=sp, ns=ns),
              dict(counts=_junk((B, L, S, bins), np.int64), missing=_junk((B, L), np.int64), total=_junk(B, np.int64), other=_junk(B, np.int64)))
    top = level == 0
    nat.check(nat.lib().vs_facet_value_radix_counts(b.p("words"), bit0, ld, b.p("aw"), B, b.p("labels"), L, b.p("v"), _dt(v), n, level, R,
                                                    None if top else b.p("sp"), None if top else b.p("ns"), rpc, b.p("counts"),
                                                    b.p("missing") if top else None, b.p("total") if top else None, b.p("other") if top else None,
                                                    0, None))
    return b.out("counts"), b.out("missing"), b.out("total"), b.out("other")


@pytest.mark.parametrize("dtype", DTYPES)
def test_levels_compose_to_the_call(dtype):
    n, B, R = 2500, 2, 5
    tile, counts = _label_edge_counts()
    dev = torch.device("cuda", 0)
    q = np.array([0.0, 0.1, 0.5, 0.5, 1.0])
    mid = next(L for L in range(tile, counts[-1]) if facet_value_quantile_plan(n, B, L, R, 1, True)[0] == 1)
    assert [p[0] for p in _plan(n, B, mid, R)][:2] == [0, 1]                            # level 0 in LDS tiles, level 1 with global atomics
    for L in (4, tile + 1, mid):                                                      # one tile, two tiles, a level in the global regime
        v = ref.values_case(n, dtype, seed=L, spread=400, frac_special=0.1)
        labels = fref.labels_shape("mixed", n, L, L + 1)
        masks = ref.masks_case(B, n, seed=4, density=0.7)
        live = np.random.default_rng(5).random(n) < 0.9
        bit0 = 37
        words = ref.pack(masks, bit0, spare=1)
        aw = ref.pack(live[None, :], bit0, spare=1)[0]
        ld = words.shape[1]
        trace = []
        want = fq.radix_select(words, ld, bit0, n, v, labels, L, q=q, method="nearest", and_words=aw, trace=trace)
        _same(want, fq.order_statistics(words, ld, bit0, n, v, labels, L, q=q, method="nearest", and_words=aw))
        d_q = torch.from_numpy(q).to(dev)
        state = None
        for level in range(3):
            sp = _np(state["slot_prefix"]) if level else None
            ns = _np(state["n_slots"]) if level else None
            for on_dev in (True, False):
                c, mis, tot, oth = _level_call(words, bit0, ld, aw, B, labels, L, v, n, level, R, sp, ns, on_dev)
                assert (c == trace[level][0]).all(), ("counts", L, level, on_dev)     # slots at or past n_slots stay 0: written whole
                if level == 0:
                    assert (mis == want[3]).all() and (tot == want[4]).all() and (oth == want[5]).all()
                else:
                    assert (mis == JUNK).all() and (tot == JUNK).all() and (oth == JUNK).all()
            state = value_radix_step(level, torch.from_numpy(c.reshape(B * L, c.shape[2], c.shape[3])).to(dev), R, state, d_q, qref.NEAREST, None,
                                     torch.float32 if dtype == F32 else torch.int32, 0)
            for name, w in trace[level][1].items():
                if name not in ("count", "ranks", "values"):
                    assert (_np(state[name]).view(w.dtype) == w).all(), (name, L, level)
        got = (_np(state["values"]).reshape(B, L, R), _np(state["ranks"]).reshape(B, L, R), _np(state["count"]).reshape(B, L)) + want[3:]
        _same(got, want, "composed")
        _same(_raw(words, bit0, ld, aw, B, labels, L, v, n, True, q=q, method="nearest"), want, "all in one")
    L = counts[-1]                                                                    # level 0 in the global regime: its counts by name
    labels = fref.labels_shape("mixed", n, L, 3)
    assert facet_value_quantile_plan(n, B, L, 1, 0, True)[0] == 1
    got = _level_call(words, bit0, ld, aw, B, labels, L, v, n, 0, 1, None, None, True)
    assert all((g == w).all() for g, w in zip(got, fq.level_counts(words, ld, bit0, n, v, labels, L, 0, 1, and_words=aw)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_label_equals_the_percentiles_counts(dtype):
    n, B, R = 3000, 3, 4
    v = ref.values_case(n, dtype, seed=31, spread=300)
    labels = np.zeros(n, I32)
    masks = ref.masks_case(B, n, seed=32, density=0.8)
    words = ref.pack(masks, 5, spare=1)
    ld = words.shape[1]
    trace = []
    qref.radix_select(words, ld, 5, n, v, q=[0.0, 0.3, 0.6, 1.0], trace=trace)
    state = None
    for level in range(3):
        sp, ns = (state["slot_prefix"], state["n_slots"]) if level else (None, None)
        S, bins = (1 if level == 0 else R), qref.LEVEL_BINS[level]
        b = _Bufs(True, dict(words=words, v=v, sp=sp, ns=ns), dict(counts=_junk((B, S, bins), np.int64), missing=_junk(B, np.int64)))
        nat.check(nat.lib().vs_value_radix_counts(b.p("words"), 5, ld, None, B, b.p("v"), _dt(v), n, level, R, b.p("sp") if level else None,
                                                  b.p("ns") if level else None, 0, b.p("counts"), b.p("missing") if level == 0 else None, 0, None))
        c, mis, tot, oth = _level_call(words, 5, ld, None, B, labels, 1, v, n, level, R, sp, ns, True)
        assert (c.reshape(B, S, bins) == b.out("counts")).all() and (c.reshape(B, S, bins) == trace[level][0]).all()
        if level == 0:
            assert (mis[:, 0] == b.out("missing")).all() and (oth == 0).all() and (tot == masks.sum(1)).all()
        state = trace[level][1]


# ---- identities ---------------------------------------------------------------------------------------------------------------------------------------
_idx = {}
N_IDX, VR = 1000, 2000


def _index_case():
    if not _idx:
        ip, ix, va = rref.csr_case(N_IDX, VR, seed=1040)
        q = rref.sparse_queries(9, VR, seed=N_IDX + 1)
        _idx["case"] = (DeviceIndex.from_csr(ip, ix, va, VR, store_dtype=nat.VS_F32), q, rref.scores(q, ip, ix, va, "fp32"), (ip, ix, va))
    return _idx["case"]


def _years(n, seed=0):
    v = ref.values_case(n, I32, seed=seed, spread=60, frac_special=0.0) + 1950
    v[ref.values_case(n, I32, seed=seed, spread=60, frac_special=0.0) == ref.INT32_MIN] = ref.INT32_MIN
    v[[1, n // 2, n - 2]] = ((1 << 24) + 1, (1 << 30) + 3, -(1 << 24) - 1)             # values fp32 cannot hold
    return v.astype(I32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_identities_with_facets_and_value_quantiles(dtype):
    dev = _index_case()[0]
    n, B, L = N_IDX, 4, 5
    v = _years(n, 3) if dtype == I32 else ref.values_case(n, F32, seed=3)
    labels = fref.labels_shape("mixed", n, L, 7)
    masks = ref.masks_case(B, n, seed=8, density=0.8)
    flt = DocFilter.from_mask(torch.from_numpy(masks))
    qs = [0.0, 0.25, 0.5, 1.0]
    res = dev.facet_value_quantiles(labels, L, v, q=qs, method="nearest", filter=flt)
    assert isinstance(res, FacetValueQuantiles) and isinstance(res.values, np.ndarray)
    fc = dev.facet_counts(labels, L, filter=flt)
    assert (res.count + res.missing == fc.counts).all() and (res.total == fc.total).all() and (res.other == fc.other).all()
    assert (res.count.sum(1) + res.missing.sum(1) + res.other == res.total).all()
    tl = torch.from_numpy(labels).cuda()
    for l in range(L):                                                                 # cell (b, l) = value_quantiles under filter & from_labels(l)
        one = dev.value_quantiles(v, q=qs, method="nearest", filter=flt & DocFilter.from_labels(tl, l))
        _same((res.values[:, l], res.ranks[:, l], res.count[:, l], res.missing[:, l]), tuple(_np(t) for t in one), ("cell", l))
    # tensors in, tensors out; ranks [R] and [B, L, R]
    r1 = dev.facet_value_quantiles(tl, L, torch.from_numpy(v).cuda(), ranks=[0, 3, 10 ** 7], filter=flt)
    assert r1.values.is_cuda
    words = ref.pack(masks)
    _same(r1, fq.order_statistics(words, words.shape[1], 0, n, v, labels, L, ranks=np.tile(np.array([0, 3, 10 ** 7], np.int64), (B, L, 1))))
    q20 = np.linspace(0, 1, 20)                                                        # more than 16: two batches
    _same(dev.facet_value_quantiles(labels, L, v, q=q20, filter=flt), fq.order_statistics(words, words.shape[1], 0, n, v, labels, L, q=q20))
    c0 = dev.facet_value_radix_counts(labels, L, v, 0, 2, filter=flt)
    w0 = fq.level_counts(words, words.shape[1], 0, n, v, labels, L, 0, 2)
    assert all((g == w).all() for g, w in zip(c0, w0))


@pytest.mark.parametrize("dtype", DTYPES)
def test_deleted_rows_never_count(dtype):
    dev = _index_case()[0]
    n, B, L = N_IDX, 9, 4
    v = _years(n, 21) if dtype == I32 else ref.values_case(n, F32, seed=21)
    labels = fref.labels_shape("mixed", n, L, 22)
    masks = ref.masks_case(B, n, seed=22, density=0.9)
    words = ref.pack(masks, 0, spare=1)
    ld = words.shape[1]
    dead = np.array([0, 1, 31, 32, 500, 998, 999])
    live = np.ones(n, bool)
    live[dead] = False
    lw = ref.pack(live[None, :])[0]
    full = fq.order_statistics(words, ld, 0, n, v, labels, L, q=Q3, method="higher")
    dev.delete_rows(dead)
    try:
        want = fq.order_statistics(words, ld, 0, n, v, labels, L, q=Q3, method="higher", and_words=lw)
        assert (want[4] < full[4]).any()
        for on_dev, rpc in ((False, 0), (True, 64)):
            _same(_raw(words, 0, ld, None, B, labels, L, v, n, on_dev, q=Q3, method="higher", rpc=rpc, index=dev), want)
        _same(dev.facet_value_quantiles(labels, L, v, q=Q3, method="higher"),
              fq.order_statistics(None, 0, 0, n, v, labels, L, q=Q3, method="higher", and_words=lw))
    finally:
        dev.restore_rows()
    _same(_raw(words, 0, ld, None, B, labels, L, v, n, True, q=Q3, method="higher", index=dev), full)


@pytest.mark.parametrize("ways", [2, 3])
def test_row_shards_equal_the_unsharded_index(ways):
    whole = _index_case()[0]
    n, B = N_IDX, 5
    _, counts = _label_edge_counts()
    ndev = torch.cuda.device_count()
    bounds = [0, 437, n] if ways == 2 else [0, 437, 770, n]                            # no shard size a multiple of 32
    shards = [whole.slice_rows(bounds[i], bounds[i + 1] - bounds[i], device=i if ndev >= ways else 0) for i in range(ways)]
    group = ShardGroup(shards)
    masks = ref.masks_case(B, n, seed=31, density=0.9)
    flt = DocFilter.from_mask(torch.from_numpy(masks))
    words = ref.pack(masks)
    ld = words.shape[1]
    dead = np.array([3, 436, 437, 769, 770, 999])
    live = np.ones(n, bool)
    live[dead] = False
    q20 = np.linspace(0.0, 1.0, 20)                                                    # more than 16: two batches
    try:
        for v, L in ((_years(n, 5), 6), (ref.values_case(n, F32, seed=6), counts[-1] if ways == 2 else 6)):
            labels = fref.labels_shape("mixed", n, L, 9)
            tv, tl = torch.from_numpy(v).cuda(), torch.from_numpy(labels).cuda()
            for lw in (None, ref.pack(live[None, :])[0]):
                if lw is not None:
                    group.delete_rows(dead)
                    whole.delete_rows(dead)
                want = fq.order_statistics(words, ld, 0, n, v, labels, L, q=q20, method="nearest", and_words=lw)
                _same(group.facet_value_quantiles(tl, L, tv, q=q20, method="nearest", filter=flt), want, "group")
                _same(whole.facet_value_quantiles(labels, L, v, q=q20, method="nearest", filter=flt), want, "whole")
                _same(group.facet_value_quantiles(tl, L, tv, q=[0.5]), fq.order_statistics(None, 0, 0, n, v, labels, L, q=[0.5], and_words=lw))
                rk = np.array([0, 5, 436], np.int64)
                _same(group.facet_value_quantiles(labels, L, v, ranks=rk, filter=flt),
                      fq.order_statistics(words, ld, 0, n, v, labels, L, ranks=np.tile(rk, (B, L, 1)), and_words=lw))
            group.restore_rows()
            whole.restore_rows()
    finally:
        group.restore_rows()
        whole.restore_rows()
        group.close()


# ---- the facade ---------------------------------------------------------------------------------------------------------------------------------------
def _sparse_index(ip, ix, va, n):
    from vsearch_amd.ir import SparseIndex
    sp = SparseIndex(device="cuda:0", fp16=False)
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(va), size=(n, VR))
    sp.move_to_device("cuda:0")
    return sp


def _linear(words, ld, n, v, labels, L, pcts):
    """percentiles_by_facet(method="linear") by the definition: floor and ceil selected by the sort, the project's formula in fp64"""
    q = np.asarray(pcts, np.float64) / 100.0
    lo = fq.order_statistics(words, ld, 0, n, v, labels, L, q=q, method="lower")
    hi = fq.order_statistics(words, ld, 0, n, v, labels, L, q=q, method="higher")
    pos = q[None, None, :] * (lo[2].astype(np.float64) - 1.0)[:, :, None]
    out = qref.lerp(lo[0], hi[0], pos - np.floor(pos))
    return (np.where(lo[1] < 0, np.nan, out),) + lo[2:]


def _same64(got, want):
    g, w = _np(got), np.asarray(want)
    assert g.dtype == np.float64 and g.shape == w.shape and (g.view(np.uint64)[~np.isnan(w)] == w.view(np.uint64)[~np.isnan(w)]).all()
    assert (np.isnan(g) == np.isnan(w)).all()


def test_index_facade_follows_the_index(monkeypatch):
    from vsearch_amd.ir.retriever.index import SCORE, Index
    _, q, S, (ip, ix, va) = _index_case()
    n, B, L = N_IDX, 9, 7
    tq = torch.from_numpy(q)
    sp = _sparse_index(ip, ix, va, n)
    years = _years(n, 41)
    topic = fref.labels_shape("mixed", n, L, 43)
    topic[topic >= L] = -1
    groups = (np.arange(n) // 90).astype(np.int64)
    sp.set_values("year", years.astype(np.int64), missing=years == ref.INT32_MIN)
    sp.set_facet("topic", topic, names=[f"t{i}" for i in range(L)])
    sp.set_groups(groups)
    thr = np.array([np.sort(S[b])[::-1][150] for b in range(B)], dtype=np.float32)
    mf = sp.match_filter(tq, thr)
    w = _np(mf.words).view(np.uint32)
    ld = w.shape[1]
    pcts = [0, 5, 25, 50, 75, 95, 100]
    for method in ("lower", "higher", "nearest"):
        res = sp.percentiles_by_facet("year", "topic", pcts, tq, thr, method=method)
        assert isinstance(res, FacetValuePercentiles)
        want = fq.order_statistics(w, ld, 0, n, years, topic, L, q=np.array(pcts) / 100.0, method=method)
        _same(res, (want[0],) + want[2:], method)
    res = sp.percentiles_by_facet("year", "topic", pcts, tq, thr)                      # linear
    wl = _linear(w, ld, n, years, topic, L, pcts)
    _same64(res.values, wl[0])
    _same(res[1:], wl[1:])
    inset = ref.unpack(w, 0, n)
    for b in range(0, B, 4):                                                           # numpy per label, on int data
        for l in range(L):
            x = years[inset[b] & (topic == l) & (years != ref.INT32_MIN)].astype(np.float64)
            if x.size:
                want = np.percentile(x, pcts, method="linear")
                lo = np.percentile(x, pcts, method="lower")
                hi = np.percentile(x, pcts, method="higher")
                assert (np.abs(_np(res.values)[b, l] - want) <= 4 * 2.0 ** -52 * np.maximum(np.abs(lo), np.abs(hi))).all()
    _same64(sp.median_by_facet("year", "topic", tq, thr).values, wl[0][:, :, 3:4])
    n_groups = int(groups.max()) + 1
    _same(sp.percentiles_by_facet("year", "groups", [50], method="higher"),
          (lambda o: (o[0],) + o[2:])(fq.order_statistics(None, 0, 0, n, years, groups, n_groups, q=[0.5], method="higher")))
    # the split: first over the queries, then over the percentiles -- a small budget forces both, and more than 16 percentiles a second pass
    many = np.linspace(0, 100, 40)
    want = fq.order_statistics(w, ld, 0, n, years, topic, L, q=many / 100.0, method="nearest")
    _same(sp.percentiles_by_facet("year", "topic", many, tq, thr, method="nearest"), (want[0],) + want[2:], "batches")
    calls = []
    target = sp._explain_target()[0]
    real = type(target).facet_value_quantiles
    monkeypatch.setattr(type(target), "facet_value_quantiles", lambda self, *a, **k: (calls.append((k["filter"].n_queries, len(k["q"]))), real(self, *a, **k))[1])
    monkeypatch.setattr(Index, "FACET_QUANTILE_CELLS", 4 * L * 8)                      # 4 queries a pass, all 8 ranks
    _same(sp.percentiles_by_facet("year", "topic", many[:8], tq, thr, method="nearest"), (want[0][:, :, :8],) + want[2:], "split over queries")
    assert calls == [(4, 8), (4, 8), (1, 8)]
    del calls[:]
    monkeypatch.setattr(Index, "FACET_QUANTILE_CELLS", 3 * L)                          # one query and 3 ranks a pass
    _same(sp.percentiles_by_facet("year", "topic", many[:8], tq, thr, method="nearest"), (want[0][:, :, :8],) + want[2:], "split over both")
    assert calls == [(1, 3), (1, 3), (1, 2)] * B
    _same64(sp.percentiles_by_facet("year", "topic", pcts, tq, thr).values, wl[0])
    monkeypatch.undo()
    # SCORE: the percentiles of each query's scores per label = percentiles(SCORE, filter & from_labels(l))
    res = sp.percentiles_by_facet(SCORE, "topic", [10, 50, 90], tq, thr, method="lower")
    tt = torch.from_numpy(topic).cuda()
    for l in (0, L - 1):
        one = sp.percentiles(SCORE, [10, 50, 90], tq, min_score=None, filter=mf & DocFilter.from_labels(tt, l), method="lower")
        assert ref.same(_np(res.values)[:, l], _np(one.values)) and (_np(res.count)[:, l] == _np(one.count)).all()
    # more labels than a pass can take: not covered, and said so
    sp.set_facet("wide", np.arange(n, dtype=np.int64) % 7, names=None)
    store = sp._facet_store()
    store["wide"] = (store["wide"][0], 65537, None)
    with pytest.raises(ValueError, match="not covered"):
        sp.percentiles_by_facet("year", "wide", [50])
    with pytest.raises(KeyError):
        sp.percentiles_by_facet("year", "nope", [50])
    with pytest.raises(ValueError, match="0..100"):
        sp.percentiles_by_facet("year", "topic", [101])


def test_sharded_facade_equals_the_single_index():
    _, q, S, (ip, ix, va) = _index_case()
    n, B, L = N_IDX, 9, 5
    tq = torch.from_numpy(q)
    years = _years(n, 51)
    topic = fref.labels_shape("random", n, L, 52)
    thr = np.array([np.sort(S[b])[::-1][150] for b in range(B)], dtype=np.float32)
    sp = _sparse_index(ip, ix, va, n)
    sp.set_values("year", years, missing=years == ref.INT32_MIN)
    sp.set_facet("topic", topic)
    pcts = np.linspace(0, 100, 21)
    want = [tuple(_np(t) for t in sp.percentiles_by_facet("year", "topic", pcts, tq, thr, method=m)) for m in ("linear", "nearest")]
    sp.shard_rows([0, 0, 0])
    assert sp.shards is not None and len(sp.shards) == 3
    for m, w in zip(("linear", "nearest"), want):
        got = tuple(_np(t) for t in sp.percentiles_by_facet("year", "topic", pcts, tq, thr, method=m))
        assert all(g.dtype == x.dtype and g.tobytes() == x.tobytes() for g, x in zip(got, w)), m
    assert int(_np(sp.percentiles_by_facet("year", "topic", [100], method="lower").values).max()) == (1 << 30) + 3


def test_retrieve_percentiles_by_facet(tiny_retriever):
    from vsearch_amd.ir.retriever.index import IndexType
    r = tiny_retriever
    n = 80
    texts = make_texts(n, 5)
    r.build_index(texts, index_type=IndexType.SPARSE)
    idx = r.index
    langs = ["en", "de", "fr", None]
    year = [1950 + (i * 7) % 60 if i % 9 else None for i in range(n)]
    idx.data = [dict(text=t, **({"lang": langs[i % 4]} if langs[i % 4] else {}), **({"year": y} if y is not None else {}))
                for i, (t, y) in enumerate(zip(texts, year))]
    names = idx.facet_from_samples("lang")
    idx.values_from_samples("year")
    assert names == ["de", "en", "fr"]
    codes = np.array([{"en": 1, "de": 0, "fr": 2, None: -1}[langs[i % 4]] for i in range(n)], I32)
    years = np.array([ref.INT32_MIN if y is None else y for y in year], I32)
    queries = make_texts(4, 9)
    q_emb = r.process_query(queries, 0, r.encoder_q.config.topk)
    sc = _np(idx.explain(q_emb, torch.arange(n).repeat(4, 1), topn=0).scores).astype(np.float32)
    thr = np.array([np.unique(sc[b])[np.unique(sc[b]).size // 2] for b in range(4)], dtype=np.float32)
    words = _np(idx.match_filter(q_emb, thr).words).view(np.uint32)
    pcts = [0, 50, 100]
    rows, totals = r.retrieve_percentiles_by_facet(queries, "year", "lang", pcts, thr, topn=2, method="nearest")
    want = fq.order_statistics(words, words.shape[1], 0, n, years, codes, 3, q=np.array(pcts) / 100.0, method="nearest")
    wl, wc = fcref.topn(want[2] + want[3], 2, 1)
    assert totals == want[4].tolist() == _np(r.retrieve_range(queries, thr, max_hits=0).counts).tolist()
    assert rows == [[(names[l], int(d), int(want[2][b, l]), want[0][b, l].tolist()) for l, d in zip(wl[b], wc[b]) if l >= 0] for b in range(4)]
    rows, _ = r.retrieve_percentiles_by_facet(queries, "year", "lang", [50], thr)      # linear: float64, numpy's per label
    inset = ref.unpack(words, 0, n)
    for b in range(4):
        for name, docs, count, vals in rows[b]:
            x = years[inset[b] & (codes == names.index(name)) & (years != ref.INT32_MIN)]
            assert count == x.size and docs == (inset[b] & (codes == names.index(name))).sum()
            assert vals == [np.percentile(x.astype(np.float64), 50)] if x.size else np.isnan(vals[0])
