"""GPU tests of the numeric fields (vs_value_range_bitmaps / vs_value_stats / vs_value_histogram / vs_value_topk and their vs_index_* variants;
DeviceIndex / ShardGroup .value_range_filter / .value_stats / .value_histogram / .value_topk, Index.set_values / .value_filter / .value_stats /
.histogram / .top_by_value, Retriever.retrieve_sorted / .retrieve_histogram) -- run on MI355X.

The contract is tests/_value_ref.py.  Every result is an integer or a 32-bit pattern, so everything compares exactly.  The raw
calls go into junk-filled outputs, once on host buffers and once on device buffers; the count rows of a histogram carry spare columns
(ld_counts > n_edges - 1) that must keep their junk."""
import ctypes as C

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, ShardGroup, SortedResults, ValueHistogram, ValueStats, value_plan, value_range_bitmaps
from vsearch_amd.doc_filter import DocFilter
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

import _range_ref as rref
import _value_ref as ref

pytestmark = pytest.mark.gpu

F32, I32 = np.float32, np.int32
DTYPES = [F32, I32]
JUNK = -0x5A5A5A5A5A5A5A5B
JUNK32 = 0x5A5A5A5A
PAD = 3                       # spare columns of a count row
VR = 2000
N_IDX = 1000


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _dt(v):
    return nat.VAL_F32 if v.dtype == F32 else nat.VAL_I32


def _same(got, want, what=None):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert ref.same(_np(g), w), (what, i)


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


def _junk(shape, dtype):
    if np.dtype(dtype) == np.int64:
        return np.full(shape, JUNK, np.int64)
    return np.full(shape, JUNK32, np.uint32).view(dtype).reshape(shape)


def _raw_stats(words, bit0, ld, aw, B, v, n, rpc, on_dev, index=None):
    b = _Bufs(on_dev, dict(words=words, aw=aw, v=v), dict(count=_junk(B, np.int64), missing=_junk(B, np.int64), lo=_junk(B, v.dtype),
                                                          hi=_junk(B, v.dtype), sum=_junk(B, np.int64)))
    outs = [b.p(k) for k in ("count", "missing", "lo", "hi", "sum")]
    if index is None:
        rc = nat.lib().vs_value_stats(b.p("words"), bit0, ld, b.p("aw"), B, b.p("v"), _dt(v), n, rpc, *outs, 0, None)
    else:
        rc = nat.lib().vs_index_value_stats(index._h, b.p("words"), bit0, ld, B, b.p("v"), _dt(v), rpc, *outs, None)
    nat.check(rc)
    return tuple(b.out(k) for k in ("count", "missing", "lo", "hi", "sum"))


def _raw_hist(words, bit0, ld, aw, B, v, n, edges, rpc, on_dev, index=None):
    E = len(edges)
    b = _Bufs(on_dev, dict(words=words, aw=aw, v=v, e=np.asarray(edges, v.dtype)),
              dict(counts=_junk((B, E - 1 + PAD), np.int64), below=_junk(B, np.int64), above=_junk(B, np.int64), missing=_junk(B, np.int64)))
    outs = [b.p("counts"), E - 1 + PAD, b.p("below"), b.p("above"), b.p("missing")]
    if index is None:
        rc = nat.lib().vs_value_histogram(b.p("words"), bit0, ld, b.p("aw"), B, b.p("v"), _dt(v), n, b.p("e"), E, rpc, *outs, 0, None)
    else:
        rc = nat.lib().vs_index_value_histogram(index._h, b.p("words"), bit0, ld, B, b.p("v"), _dt(v), b.p("e"), E, rpc, *outs, None)
    nat.check(rc)
    counts = b.out("counts")
    assert (counts[:, E - 1:] == JUNK).all(), "a count row's spare columns were written"
    return counts[:, :E - 1], b.out("below"), b.out("above"), b.out("missing")


def _raw_topk(words, bit0, ld, aw, B, v, n, k, desc, id_offset, rpc, on_dev, index=None):
    b = _Bufs(on_dev, dict(words=words, aw=aw, v=v), dict(ids=_junk((B, k), np.int64), vals=_junk((B, k), v.dtype)))
    if index is None:
        rc = nat.lib().vs_value_topk(b.p("words"), bit0, ld, b.p("aw"), B, b.p("v"), _dt(v), n, k, int(desc), id_offset, rpc, b.p("ids"), b.p("vals"),
                                     0, None)
    else:
        rc = nat.lib().vs_index_value_topk(index._h, b.p("words"), bit0, ld, B, b.p("v"), _dt(v), k, int(desc), id_offset, rpc, b.p("ids"),
                                           b.p("vals"), None)
    nat.check(rc)
    return b.out("ids"), b.out("vals")


def _check(masks, bit0, v, edges=None, k=5, and_mask=None, rpc=0, shared=False, what=None, desc=(True, False), id_offset=0):
    """per-query sets `masks` [B, n] packed at bit0 with every spare bit set -> stats, histogram and top-k, both buffer kinds, against the reference"""
    B, n = masks.shape
    words = ref.pack(masks, bit0, spare=1)
    aw = ref.pack(and_mask[None, :], bit0, spare=1)[0] if and_mask is not None else None
    ld = 0 if shared else words.shape[1]
    edges = ref.edges_case(9, v.dtype) if edges is None else edges
    size = (masks & and_mask[None, :] if and_mask is not None else masks).sum(axis=1)
    want_s = ref.stats(words, ld, bit0, n, v, aw)
    want_h = ref.histogram(words, ld, bit0, n, v, edges, aw)
    assert (want_s[0] + want_s[1] == size).all() and (want_h[0].sum(axis=1) + want_h[1] + want_h[2] + want_h[3] == size).all()
    for on_dev in (False, True):
        _same(_raw_stats(words, bit0, ld, aw, B, v, n, rpc, on_dev), want_s, (what, "stats", on_dev, bit0, rpc))
        _same(_raw_hist(words, bit0, ld, aw, B, v, n, edges, rpc, on_dev), want_h, (what, "histogram", on_dev, bit0, rpc))
        for d in desc:
            _same(_raw_topk(words, bit0, ld, aw, B, v, n, k, d, id_offset, rpc, on_dev), ref.topk(words, ld, bit0, n, v, k, d, id_offset, aw),
                  (what, "topk", d, on_dev, bit0, rpc))
    return want_s, want_h


# ---- row and bit edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049])
def test_row_and_bit_edges(n_rows, dtype):
    B = 3
    v = ref.values_case(n_rows, dtype, seed=n_rows, frac_missing=0.15, frac_special=0.1, spread=30)
    masks = ref.masks_case(B, n_rows, seed=n_rows + 1, density=0.9)
    live = np.random.default_rng(n_rows).random(n_rows) < 0.8
    for bit0, on_dev in [(b, d) for b in (0, 1, 31, 32, 33) for d in (False, True)]:
        words = ref.pack(masks, bit0, spare=1)                                        # the spare bits of the first and last word are all set
        for aw in (None, ref.pack(live[None, :], bit0, spare=1)[0]):
            ld = words.shape[1]
            _same(_raw_stats(words, bit0, ld, aw, B, v, n_rows, 0, on_dev), ref.stats(words, ld, bit0, n_rows, v, aw), ("stats", bit0))
            e = ref.edges_case(5, dtype, spread=30)
            _same(_raw_hist(words, bit0, ld, aw, B, v, n_rows, e, 0, on_dev), ref.histogram(words, ld, bit0, n_rows, v, e, aw), ("hist", bit0))
            _same(_raw_topk(words, bit0, ld, aw, B, v, n_rows, 4, bit0 & 1, 0, 0, on_dev), ref.topk(words, ld, bit0, n_rows, v, 4, bit0 & 1, 0, aw),
                  ("topk", bit0))
    empty, full = np.zeros((B, n_rows), bool), np.ones((B, n_rows), bool)
    assert (_check(empty, 1, v, what="empty")[0][0] == 0).all()
    st = _check(full, 33, v, what="full")[0]
    assert (st[0] + st[1] == n_rows).all()
    aw = ref.pack(live[None, :], 0, spare=1)[0]
    for on_dev in (False, True):                                                      # words = NULL: every row set
        for a in (None, aw):
            _same(_raw_stats(None, 0, 0, a, 1, v, n_rows, 0, on_dev), ref.stats(None, 0, 0, n_rows, v, a))
            _same(_raw_topk(None, 0, 0, a, 1, v, n_rows, 3, True, 5, 0, on_dev), ref.topk(None, 0, 0, n_rows, v, 3, True, 5, a))
            e = ref.edges_case(3, dtype, spread=30)
            _same(_raw_hist(None, 0, 0, a, 1, v, n_rows, e, 0, on_dev), ref.histogram(None, 0, 0, n_rows, v, e, a))


# ---- chunk edges -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_rows,chunks", [(3 * 2048 + 1, 4), (4 * 2048, 4)])
def test_chunk_edges(n_rows, chunks, dtype):
    """rows_per_chunk = 2048: four chunks, the last of one row / a full one; the last row carries the min or the max and the top hit"""
    B = 9
    assert value_plan(n_rows, B, 11, True, 2048) == (8, chunks, 2048)
    for top in (True, False):
        v = ref.values_case(n_rows, dtype, seed=n_rows, spread=100, frac_special=0.0)
        v[-1] = 5000 if top else -5000
        masks = ref.masks_case(B, n_rows, seed=5, density=0.7)
        masks[:, -1] = True                                                           # the one-row chunk holds a member
        for bit0 in (0, 33):
            st, _ = _check(masks, bit0, v, rpc=2048, what="chunks", desc=(top,))
            assert (st[3 if top else 2] == v[-1]).all()


# ---- query tiles and bitmaps -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 7, 8, 9, 17])
def test_query_tiles(B):
    n = 5000
    for dtype in DTYPES:
        v = ref.values_case(n, dtype, seed=B)
        masks = ref.masks_case(B, n, seed=B + 10, density=0.6)
        assert value_plan(n, B, 11, True)[0] == 8
        _check(masks, 0, v, what="tiles")
        _check(masks, 31, v, rpc=64, what="tiles, 64-row chunks", desc=(True,))


@pytest.mark.parametrize("dtype", DTYPES)
def test_shared_bitmap(dtype):
    n = 5000
    v = ref.values_case(n, dtype, seed=4)
    masks = ref.masks_case(1, n, seed=14, density=0.5)
    assert value_plan(n, 1, 11, False)[0] == 1
    for bit0 in (0, 33):
        _check(masks, bit0, v, shared=True, what="shared")


# ---- edges -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_edges", [2, 3, 1024, 1025])
def test_values_on_and_next_to_every_edge(n_edges):
    """every edge, and one ulp on either side of it, is a value; -0.0 against an edge at +0.0; +-inf"""
    e = np.unique(np.concatenate([np.linspace(-50, 50, n_edges - 1).astype(F32), np.array([0.0], F32)]))[:n_edges]
    if e.shape[0] < n_edges:
        e = np.concatenate([e, np.array([60.0 + i for i in range(n_edges - e.shape[0])], F32)])
    assert e.shape[0] == n_edges and (np.diff(e) > 0).all() and 0.0 in e
    v = np.concatenate([e, np.nextafter(e, F32(np.inf)), np.nextafter(e, F32(-np.inf)), np.array([-0.0, 0.0, np.inf, -np.inf, np.nan], F32)]).astype(F32)
    v = np.tile(v, 2)
    B = 9
    masks = ref.masks_case(B, v.shape[0], seed=n_edges, density=1.5)
    masks[0] = True
    _, h = _check(masks, 1, v, edges=e, what="on the edges")
    assert h[1][0] > 0 and h[2][0] > 0 and h[3][0] == 2
    # -0.0 falls where +0.0 falls: at or above the edge at +0.0
    i0 = int(np.flatnonzero(e == 0.0)[0])
    z = np.array([-0.0] * 3 + [0.0] * 2, F32)
    c, below, above, _ = _raw_hist(None, 0, 0, None, 1, z, 5, e, 0, True)
    assert (c[0, i0] if i0 < n_edges - 1 else above[0]) == 5
    # int32 at the ends of its range
    ei = (np.arange(n_edges, dtype=np.int64) * ((1 << 32) // (n_edges + 1)) + ref.INT32_MIN + 1).astype(I32)
    vi = np.concatenate([ei, ei[1:] - 1, ei[:-1] + 1, np.array([ref.INT32_MIN + 1, (1 << 31) - 1, ref.INT32_MIN], I32)]).astype(I32)
    mi = ref.masks_case(B, vi.shape[0], seed=n_edges + 1, density=1.5)
    mi[0] = True
    _, h = _check(mi, 33, vi, edges=ei, what="int edges")
    assert h[2][0] > 0 and h[3][0] == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_missing_and_one_distinct_value(dtype):
    n, B = 5000, 9
    masks = ref.masks_case(B, n, seed=3, density=0.9)
    masks[0] = True
    gone = np.full(n, ref.sentinel(dtype), dtype)
    st, h = _check(masks, 1, gone, what="all missing")
    assert (st[0] == 0).all() and st[1][0] == n and ref.is_missing(st[2]).all() and ref.is_missing(st[3]).all() and (st[4] == 0).all()
    assert (h[3] == st[1]).all() and (h[0] == 0).all()
    one = np.full(n, 7, dtype)                                                        # the most contended bin; ties everywhere: id order
    st, h = _check(masks, 1, one, k=64, what="one value")
    assert (st[2] == 7).all() and (st[3] == 7).all() and st[4][0] == n * (7 if dtype == I32 else 7 << 24)
    ids, _ = _raw_topk(None, 0, 0, None, 1, one, n, 64, True, 0, 0, True)
    assert ids[0].tolist() == list(range(64))


def test_int32_sums_and_extremes_are_exact():
    n = 4096
    v = np.full(n, (1 << 31) - 1, I32)
    v[::2] = ref.INT32_MIN + 1
    v[5] = (1 << 24) + 1
    st = _raw_stats(None, 0, 0, None, 1, v, n, 0, True)
    _same(st, ref.stats(None, 0, 0, n, v))
    assert st[2][0] == ref.INT32_MIN + 1 and st[3][0] == (1 << 31) - 1
    big = np.full(n, (1 << 31) - 1, I32)                                              # the sum leaves 32 bits far behind
    assert _raw_stats(None, 0, 0, None, 1, big, n, 64, False)[4][0] == n * ((1 << 31) - 1)


# ---- top-k ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 63, 64, 65, 255, 256, 257, 1023, 1024])
def test_topk_sizes(k):
    """n = 12 000 rows in chunks of 6 144: more than 4096 set rows a chunk (the buffer is cut), two chunks (the lists are merged)"""
    n, B = 12_000, 3
    for dtype, desc in ((F32, True), (I32, False)):
        v = ref.values_case(n, dtype, seed=k, spread=400)                             # 800 / 6400 distinct values: ties at every cut
        masks = np.ones((B, n), bool)
        masks[1] = ref.masks_case(1, n, seed=k, density=0.9)[0]
        masks[2, 100:] = False                                                        # fewer than k for the larger k: padding
        words = ref.pack(masks, 33, spare=1)
        assert (masks[0, :6144] & ~ref.is_missing(v[:6144])).sum() > 4096
        for on_dev in (False, True):
            got = _raw_topk(words, 33, words.shape[1], None, B, v, n, k, desc, 1 << 40, 6144, on_dev)
            _same(got, ref.topk(words, words.shape[1], 33, n, v, k, desc, 1 << 40), ("topk", k, on_dev))
    if k >= 255:
        assert (got[0][2, 100:] == -1).all() and ref.is_missing(got[1][2, 100:]).all()


@pytest.mark.parametrize("desc", [True, False])
def test_topk_ascending_input_admits_at_every_step_and_ties_give_id_order(desc):
    n = 20_000
    v = np.arange(n, dtype=I32) if desc else -np.arange(n, dtype=I32)                 # every span beats the threshold of the last cut
    for rpc in (0, 2048):
        _same(_raw_topk(None, 0, 0, None, 1, v, n, 100, desc, 0, rpc, True), ref.topk(None, 0, 0, n, v, 100, desc))
    flat = np.zeros(n, F32)
    flat[::3] = -0.0                                                                  # -0.0 and +0.0 tie: id order, the stored zero comes back
    ids, vals = _raw_topk(None, 0, 0, None, 1, flat, n, 1024, desc, 0, 2048, True)
    assert ids[0].tolist() == list(range(1024)) and ref.same(vals[0], flat[:1024])
    _same(_raw_topk(None, 0, 0, None, 1, flat, 10, 1024, desc, 7, 0, False), ref.topk(None, 0, 0, 10, flat[:10], 1024, desc, 7))     # k > n_rows


# ---- range bitmaps -------------------------------------------------------------------------------------------------------------------------------------
def _raw_ranges(v, lo, hi, bit0, on_dev, pad=2):
    n, B = v.shape[0], len(lo)
    span = (bit0 + n + 31) // 32
    b = _Bufs(on_dev, dict(v=v, lo=np.asarray(lo, v.dtype), hi=np.asarray(hi, v.dtype)), dict(out=_junk((B, span + pad), np.int32)))
    nat.check(nat.lib().vs_value_range_bitmaps(b.p("v"), _dt(v), n, b.p("lo"), b.p("hi"), B, bit0, b.p("out"), span + pad, 0, None))
    out = b.out("out").view(np.uint32)
    assert (out[:, span:] == JUNK32).all(), "words behind the span were written"
    return out[:, :span]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_rows", [1, 33, 64, 2049])
def test_range_bitmaps(n_rows, dtype):
    v = ref.values_case(n_rows, dtype, seed=n_rows, frac_special=0.1, spread=10)
    has = v[~ref.is_missing(v)]
    x = has[0] if has.size else dtype(1)
    open_lo, open_hi = (-np.inf, np.inf) if dtype == F32 else (ref.INT32_MIN + 1, (1 << 31) - 1)
    lo = np.array([-3, x, 5, open_lo, 2, open_lo, 0], dtype)                           # a range, lo == hi, lo > hi, open ends, +-0
    hi = np.array([4, x, 1, open_hi, open_hi, -2, 0], dtype)
    if dtype == F32:
        lo[6] = -0.0
    for bit0 in (0, 1, 33):
        want = ref.range_bitmaps(v, lo, hi, bit0)
        assert not ref.unpack(want, bit0, n_rows)[2].any()
        for on_dev in (False, True):
            got = _raw_ranges(v, lo, hi, bit0, on_dev)
            assert (got == want).all(), (bit0, on_dev)                                # whole words: 0 below bit0 and past the rows
        got = value_range_bitmaps(torch.from_numpy(v).cuda(), list(lo), list(hi), bit0=bit0)
        assert (_np(got).view(np.uint32) == want).all()
        assert (value_range_bitmaps(v, lo, hi, bit0=bit0).view(np.uint32) == want).all()


def test_4096_ranges_and_missing_bounds_on_the_device():
    n, B = 3000, 4096
    v = ref.values_case(n, I32, seed=1, spread=3000)
    rng = np.random.default_rng(2)
    lo = rng.integers(-3000, 3000, size=B).astype(I32)
    hi = (lo + rng.integers(-5, 200, size=B)).astype(I32)
    want = ref.range_bitmaps(v, lo, hi, 7)
    for on_dev in (False, True):
        assert (_raw_ranges(v, lo, hi, 7, on_dev) == want).all()
    f = ref.values_case(n, F32, seed=3)
    lo, hi = np.array([np.nan, -1.0, -np.inf], F32), np.array([1.0, np.nan, np.inf], F32)     # device bounds are not read on the host
    got = _raw_ranges(f, lo, hi, 0, True)
    assert not got[:2].any() and (ref.unpack(got, 0, n)[2] == ~np.isnan(f)).all()
    with pytest.raises(ValueError, match="missing bound"):
        _raw_ranges(f, lo, hi, 0, False)


# ---- index level -----------------------------------------------------------------------------------------------------------------------------------------
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


def _years(n, seed=0):
    v = ref.values_case(n, I32, seed=seed, spread=60, frac_special=0.0) + 1950
    v[ref.values_case(n, I32, seed=seed, spread=60, frac_special=0.0) == ref.INT32_MIN] = ref.INT32_MIN
    v[[1, n // 2, n - 2]] = ((1 << 24) + 1, (1 << 30) + 3, -(1 << 24) - 1)             # values fp32 cannot hold
    return v.astype(I32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_deleted_rows_never_count(dtype):
    dev, q, S, _ = _index_case()
    n, B = N_IDX, 9
    v = _years(n, 21) if dtype == I32 else ref.values_case(n, F32, seed=21)
    e = ref.edges_case(9, dtype) if dtype == F32 else np.arange(1940, 2020, 10).astype(I32)
    masks = ref.masks_case(B, n, seed=22, density=0.9)
    words = ref.pack(masks, 0, spare=1)
    ld = words.shape[1]
    dead = np.array([0, 1, 31, 32, 500, 998, 999])
    live = np.ones(n, bool)
    live[dead] = False
    lw = ref.pack(live[None, :])[0]
    full = ref.stats(words, ld, 0, n, v)
    dev.delete_rows(dead)
    try:
        want = ref.stats(words, ld, 0, n, v, lw)
        assert (want[0] + want[1] < full[0] + full[1]).any()
        for on_dev in (False, True):
            for rpc in (0, 64):
                _same(_raw_stats(words, 0, ld, None, B, v, n, rpc, on_dev, index=dev), want)
                _same(_raw_hist(words, 0, ld, None, B, v, n, e, rpc, on_dev, index=dev), ref.histogram(words, ld, 0, n, v, e, lw))
                _same(_raw_topk(words, 0, ld, None, B, v, n, 20, True, 3, rpc, on_dev, index=dev), ref.topk(words, ld, 0, n, v, 20, True, 3, lw))
        res = dev.value_stats(v)                                                      # no filter: every live document
        assert isinstance(res, ValueStats) and isinstance(res.count, np.ndarray)
        _same(res, ref.stats(None, 0, 0, n, v, lw))
        assert int(res.count[0] + res.missing[0]) == n - dead.size == dev.n_live
        flt = DocFilter.from_mask(torch.from_numpy(masks))
        res = dev.value_histogram(torch.from_numpy(v).cuda(), e, filter=flt)
        assert isinstance(res, ValueHistogram) and res.counts.is_cuda
        wh = ref.histogram(words, ld, 0, n, v, e, lw)
        _same(res[:4], wh)
        assert (_np(res.total) == want[0] + want[1]).all()
        top = dev.value_topk(v, 10, descending=False, filter=torch.from_numpy(masks[0]))          # a shared mask: B = 1
        assert isinstance(top, SortedResults) and top.ids.shape == (1, 10)
        _same(top, ref.topk(words[:1], 0, 0, n, v, 10, False, 0, lw))
    finally:
        dev.restore_rows()
    for on_dev in (False, True):
        _same(_raw_stats(words, 0, ld, None, B, v, n, 0, on_dev, index=dev), full)


@pytest.mark.parametrize("ways", [2, 3])
def test_row_shards_equal_the_unsharded_index(ways):
    whole, q, S, _ = _index_case()
    n, B = N_IDX, 9
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
    try:
        for v, e in ((_years(n, 5), np.arange(1940, 2020, 10).astype(I32)), (ref.values_case(n, F32, seed=6), ref.edges_case(9, F32))):
            tv = torch.from_numpy(v).cuda()
            for lw in (None, ref.pack(live[None, :])[0]):
                if lw is not None:
                    group.delete_rows(dead)
                    whole.delete_rows(dead)
                want_s, want_h = ref.stats(words, ld, 0, n, v, lw), ref.histogram(words, ld, 0, n, v, e, lw)
                for vals in (v, tv):
                    got, one = group.value_stats(vals, filter=flt), whole.value_stats(vals, filter=flt)
                    _same(got, want_s, "group stats")
                    _same(one, want_s, "whole stats")
                    _same(group.value_stats(vals), ref.stats(None, 0, 0, n, v, lw))
                    _same(group.value_histogram(vals, e, filter=flt)[:4], want_h, "group histogram")
                    for desc in (True, False):
                        want_t = ref.topk(words, ld, 0, n, v, 50, desc, 0, lw)
                        _same(group.value_topk(vals, 50, descending=desc, filter=flt), want_t, "group topk")
                        _same(whole.value_topk(vals, 50, descending=desc, filter=flt), want_t, "whole topk")
                _same(group.value_topk(tv, 1024), ref.topk(None, 0, 0, n, v, 1024, True, 0, lw))          # k above a shard's rows: padding merges
                lo, hi = ([1960, None, 2000], [1990, 1970, 1999]) if v.dtype == I32 else ([-10.0, None, 3.0], [10.0, 0.0, 2.0])
                gf, wf = group.value_range_filter(tv, lo, hi), whole.value_range_filter(v, lo, hi)
                open_lo = ref.INT32_MIN + 1 if v.dtype == I32 else -np.inf
                want_w = ref.range_bitmaps(v, [open_lo if x is None else x for x in lo], hi)
                assert (_np(gf.words).view(np.uint32) == want_w).all() and (_np(wf.words).view(np.uint32) == want_w).all()
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
    years = _years(n, 41)
    price = ref.values_case(n, F32, seed=42)
    sp.set_values("year", years.astype(np.int64), missing=years == ref.INT32_MIN)
    sp.set_values("price", price.astype(np.float64))
    assert sp.value_fields == ["year", "price"] and ref.same(_np(sp.get_values("year")), years) and ref.same(_np(sp.get_values("price")), price)
    sp.set_facet("topic", np.arange(n) % 5)
    with pytest.raises(ValueError, match="facet field"):
        sp.set_values("topic", years)
    thr = _mid_thresholds(S, B, 150)
    mf = sp.match_filter(tq, thr)
    w = _np(mf.words).view(np.uint32)
    ld = w.shape[1]
    # stats / histogram / top-k over the match set
    st = sp.value_stats("year", tq, thr)
    want = ref.stats(w, ld, 0, n, years)
    _same(st, want)
    assert (_np(st.count) + _np(st.missing) == _np(sp.count_matches(tq, thr))).all() and (want[0] > 100).all()
    assert np.allclose(_np(st.mean()), want[4] / want[0], rtol=0, atol=0)
    e = [1940, 1960, 1980, 2000, 2020]
    h = sp.histogram("year", e, tq, thr)
    _same(h[:4], ref.histogram(w, ld, 0, n, years, e))
    assert (_np(h.total) == want[0] + want[1]).all()
    for desc in (True, False):
        _same(sp.top_by_value("year", 10, desc, tq, thr), ref.topk(w, ld, 0, n, years, 10, desc))
        _same(sp.top_by_value("price", 10, desc, tq, thr), ref.topk(w, ld, 0, n, price, 10, desc))
    _same(sp.value_stats("price"), ref.stats(None, 0, 0, n, price))                   # no set: every document
    # value_filter & match_filter inside search: the top-k of the allowed rows
    vf = sp.value_filter("year", 1960, 1999)
    in_range = ref.range_masks(years, [1960], [1999])[0]
    assert (ref.unpack(_np(vf.words).view(np.uint32), 0, n) == in_range).all() and 0 < in_range.sum() < n
    res = sp.search(tq, 10, filter=vf & mf)
    allowed = in_range[None, :] & ref.unpack(w, 0, n)
    ids = _np(res.ids)
    assert all(allowed[b, ids[b][ids[b] >= 0]].all() for b in range(B))
    for b in range(B):
        best = np.lexsort((np.arange(n), -np.where(allowed[b], S[b], -np.inf)))[:min(10, int(allowed[b].sum()))]
        assert ids[b][:best.size].tolist() == best.tolist()
    pq = sp.value_filter("price", [-5.0, None], [5.0, 0.0])                           # per-query bounds, an open end
    assert pq.per_query and (ref.unpack(_np(pq.words).view(np.uint32), 0, n) == ref.range_masks(price, [-5.0, -np.inf], [5.0, 0.0])).all()
    # delete -> compact -> add(values=): the fields stay aligned with the documents
    dead = np.array([0, 5, 64, 500, 999])
    live = np.ones(n, bool)
    live[dead] = False
    sp.delete(dead)
    _same(sp.value_stats("year"), ref.stats(None, 0, 0, n, years, ref.pack(live[None, :])[0]))
    old = _np(sp.compact())
    assert (old == np.flatnonzero(live)).all()
    _same(sp.value_stats("year"), ref.stats(None, 0, 0, n - dead.size, years[live]))
    _same(sp.top_by_value("price", 7), ref.topk(None, 0, 0, n - dead.size, price[live], 7))
    new = torch.zeros(3, VR)
    new[:, 5] = 1.0
    with pytest.raises(ValueError, match="value fields"):
        sp.add(new, facets={"topic": [0, 1, 2]})
    with pytest.raises(ValueError, match="unknown"):
        sp.add(new, facets={"topic": [0, 1, 2]}, values={"year": [1, 2, 3], "price": [1.0, 2.0, 3.0], "nope": [1, 2, 3]})
    assert sp._n_rows() == n - dead.size
    ids = sp.add(new, facets={"topic": [0, 1, 2]}, values={"year": [2024, 1900, 2024], "price": [1.5, float("nan"), -2.5]})
    assert _np(ids).tolist() == [n - 5, n - 4, n - 3]
    years2 = np.concatenate([years[live], np.array([2024, 1900, 2024], I32)])
    price2 = np.concatenate([price[live], np.array([1.5, np.nan, -2.5], F32)])
    _same(sp.value_stats("year"), ref.stats(None, 0, 0, n - 2, years2))
    _same(sp.value_stats("price"), ref.stats(None, 0, 0, n - 2, price2))
    top = sp.top_by_value("year", 3, filter=sp.value_filter("year", None, 3000))
    assert _np(top.ids)[0].tolist() == [n - 5, n - 3] + [int(np.flatnonzero(years2 == np.sort(years2[years2 <= 3000])[-3])[0])]
    sp.set_values("price", None)
    assert sp.value_fields == ["year"]


def test_sharded_facade_equals_the_single_index():
    _, q, S, (ip, ix, va) = _index_case()
    n, B = N_IDX, 9
    tq = torch.from_numpy(q)
    years = _years(n, 51)
    thr = _mid_thresholds(S, B, 150)
    sp = _sparse_index(ip, ix, va, n)
    sp.set_values("year", years, missing=years == ref.INT32_MIN)
    e = [1940, 1960, 1980, 2000, 2020]
    want = [tuple(_np(t) for t in r) for r in (sp.value_stats("year", tq, thr), sp.histogram("year", e, tq, thr), sp.top_by_value("year", 20, True, tq, thr),
                                               sp.top_by_value("year", 20, False, tq, thr))]
    want_f = _np(sp.value_filter("year", 1960, 1999).words)
    sp.shard_rows([0, 0, 0])
    assert sp.shards is not None and len(sp.shards) == 3
    got = (sp.value_stats("year", tq, thr), sp.histogram("year", e, tq, thr), sp.top_by_value("year", 20, True, tq, thr),
           sp.top_by_value("year", 20, False, tq, thr))
    for g, w in zip(got, want):
        _same(g, w)
    assert (_np(sp.value_filter("year", 1960, 1999).words) == want_f).all()
    assert int(_np(sp.value_stats("year").max)[0]) == (1 << 30) + 3                                     # an int32 beyond 2^24 came through the merge unrounded


# ---- the retriever -----------------------------------------------------------------------------------------------------------------------------------
def test_retrieve_sorted_and_histogram(tiny_retriever):
    from vsearch_amd.ir.retriever.index import IndexType
    r = tiny_retriever
    n = 80
    texts = make_texts(n, 5)
    r.build_index(texts, index_type=IndexType.SPARSE)
    idx = r.index
    year = [1950 + (i * 7) % 60 if i % 9 else None for i in range(n)]
    idx.data = [dict(text=t, **({"year": y} if y is not None else {})) for t, y in zip(texts, year)]
    idx.values_from_samples("year")
    years = np.array([ref.INT32_MIN if y is None else y for y in year], I32)
    assert idx.value_fields == ["year"] and ref.same(_np(idx.get_values("year")), years)
    queries = make_texts(4, 9)
    q_emb = r.process_query(queries, 0, r.encoder_q.config.topk)
    sc = _np(idx.explain(q_emb, torch.arange(n).repeat(4, 1), topn=0).scores).astype(np.float32)
    thr = np.array([np.unique(sc[b])[np.unique(sc[b]).size // 2] for b in range(4)], dtype=np.float32)
    words = ref.pack(sc >= thr[:, None])
    res = r.retrieve_sorted(queries, "year", 6, thr)
    assert isinstance(res, SortedResults)
    _same(res, ref.topk(words, words.shape[1], 0, n, years, 6, True))
    _same(r.retrieve_sorted(queries, "year", 6, thr, descending=False), ref.topk(words, words.shape[1], 0, n, years, 6, False))
    e = [1950, 1970, 1990, 2010]
    h = r.retrieve_histogram(queries, "year", e, thr)
    _same(h[:4], ref.histogram(words, words.shape[1], 0, n, years, e))
    assert _np(h.total).tolist() == _np(r.retrieve_range(queries, thr, max_hits=0).counts).tolist()
    # value_filter is passed as filter= and composes with the term constraints
    cols = _np(idx.get_vectors(torch.tensor([3])).col_indices())
    col = int(cols[_np(idx.doc_freq(cols)).argmin()])
    vf = r.value_filter("year", 1970, None)
    both = r.retrieve_sorted(queries, "year", n, -np.inf, filter=vf, must=[col])
    ids = _np(both.ids)[0]
    ids = ids[ids >= 0]
    has = _np((r.term_filter(must=[col]) & vf).words).view(np.uint32)
    assert ids.size > 0 and sorted(ids.tolist()) == np.flatnonzero(ref.unpack(has, 0, n)).tolist() and (years[ids] >= 1970).all()
