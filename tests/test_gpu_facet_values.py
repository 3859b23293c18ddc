"""GPU tests of the breakdowns (vs_facet_value_stats / vs_facet_value_histogram and their vs_index_* variants; DeviceIndex / ShardGroup
.facet_value_stats / .facet_value_histogram, Index.stats_by_facet / .histogram_by_facet, Retriever.retrieve_stats_by_facet /
.retrieve_histogram_by_facet) -- run on MI355X.

The contract is tests/_facet_value_ref.py.  Every result is an integer or a 32-bit pattern, so everything compares exactly.
The raw calls go into junk-filled outputs, once on host buffers and once on device buffers; every matrix carries spare columns (ld_out >
n_labels, ld_counts > n_edges - 1) that must keep their junk.  The shapes are the smallest at which the kernels can go wrong: a few thousand
rows, except where a sum has to pass 2^64 (2^20 rows at the clamp of the fixed point; an int32 sum cannot wrap below 2^32 rows, so the int32
cases check sums far beyond 32 bits instead)."""
import ctypes as C

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, FacetValueHistogram, FacetValueStats, ShardGroup, facet_value_plan
from vsearch_amd.doc_filter import DocFilter
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

import _facet_ref as fref
import _facet_value_ref as ref
import _range_ref as rref
import _value_ref as vref

pytestmark = pytest.mark.gpu

F32, I32 = np.float32, np.int32
DTYPES = [F32, I32]
JUNK = -0x5A5A5A5A5A5A5A5B
JUNK32 = 0x5A5A5A5A
PAD = 3                       # spare columns of every matrix
VR = 2000
N_IDX = 1000
N = 4500                      # three spans: two full ones and 404 rows


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


def _raw_stats(words, bit0, ld, aw, B, labels, L, v, n, rpc, on_dev, index=None):
    ldo = L + PAD
    mats = ("count", "missing", "lo", "hi", "sum")
    b = _Bufs(on_dev, dict(words=words, aw=aw, labels=labels, v=v),
              dict(count=_junk((B, ldo), np.int64), missing=_junk((B, ldo), np.int64), lo=_junk((B, ldo), v.dtype), hi=_junk((B, ldo), v.dtype),
                   sum=_junk((B, ldo), np.int64), total=_junk(B, np.int64), other=_junk(B, np.int64)))
    outs = [b.p(k) for k in mats] + [ldo, b.p("total"), b.p("other")]
    if index is None:
        rc = nat.lib().vs_facet_value_stats(b.p("words"), bit0, ld, b.p("aw"), B, b.p("labels"), L, b.p("v"), _dt(v), n, rpc, *outs, 0, None)
    else:
        rc = nat.lib().vs_index_facet_value_stats(index._h, b.p("words"), bit0, ld, B, b.p("labels"), L, b.p("v"), _dt(v), rpc, *outs, None)
    nat.check(rc)
    for k in mats:
        spare = b.out(k)[:, L:]
        assert (spare == JUNK).all() if spare.dtype == np.int64 else (spare.view(np.uint32) == JUNK32).all(), f"{k}: spare columns were written"
    return tuple(np.ascontiguousarray(b.out(k)[:, :L]) for k in mats) + (b.out("total"), b.out("other"))


def _raw_hist(words, bit0, ld, aw, B, labels, L, v, n, edges, rpc, on_dev, index=None):
    E = len(edges)
    ldc = E - 1 + PAD
    b = _Bufs(on_dev, dict(words=words, aw=aw, labels=labels, v=v, e=np.asarray(edges, v.dtype)),
              dict(counts=_junk((B, L, ldc), np.int64), below=_junk((B, L), np.int64), above=_junk((B, L), np.int64), missing=_junk((B, L), np.int64),
                   total=_junk(B, np.int64), other=_junk(B, np.int64)))
    outs = [b.p("counts"), ldc] + [b.p(k) for k in ("below", "above", "missing", "total", "other")]
    if index is None:
        rc = nat.lib().vs_facet_value_histogram(b.p("words"), bit0, ld, b.p("aw"), B, b.p("labels"), L, b.p("v"), _dt(v), n, b.p("e"), E, rpc, *outs, 0,
                                                None)
    else:
        rc = nat.lib().vs_index_facet_value_histogram(index._h, b.p("words"), bit0, ld, B, b.p("labels"), L, b.p("v"), _dt(v), b.p("e"), E, rpc, *outs,
                                                      None)
    nat.check(rc)
    counts = b.out("counts")
    assert (counts[:, :, E - 1:] == JUNK).all(), "a count row's spare columns were written"
    return (np.ascontiguousarray(counts[:, :, :E - 1]),) + tuple(b.out(k) for k in ("below", "above", "missing", "total", "other"))


def _check(masks, bit0, labels, L, v, edges=None, and_mask=None, rpc=0, shared=False, what=None, words_null=False, kinds=(False, True), hist=True):
    """per-query sets `masks` [B, n] packed at bit0 with every spare bit set -> both calls, both buffer kinds, against the reference"""
    B, n = masks.shape
    words = None if words_null else ref.pack(masks, bit0, spare=1)
    aw = ref.pack(and_mask[None, :], bit0, spare=1)[0] if and_mask is not None else None
    ld = 0 if (shared or words_null) else words.shape[1]
    edges = ref.edges_case(5, v.dtype, spread=30) if edges is None else edges
    want_s = ref.stats(words, ld, bit0, n, labels, L, v, aw)
    assert (want_s[0].sum(axis=1) + want_s[1].sum(axis=1) + want_s[6] == want_s[5]).all()
    want_h = ref.histogram(words, ld, bit0, n, labels, L, v, edges, aw) if hist else None
    for on_dev in kinds:
        _same(_raw_stats(words, bit0, ld, aw, B, labels, L, v, n, rpc, on_dev), want_s, (what, "stats", on_dev, bit0, rpc))
        if hist:
            _same(_raw_hist(words, bit0, ld, aw, B, labels, L, v, n, edges, rpc, on_dev), want_h, (what, "histogram", on_dev, bit0, rpc))
    return want_s, want_h


def _values(n, dtype, seed):
    return ref.values_case(n, dtype, seed=seed, frac_missing=0.15, frac_special=0.1, spread=30)


# ---- row and bit edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 2047, 2048, 2049, 4500])
def test_row_and_bit_edges(n_rows, dtype):
    B, L = 3, 5
    v = _values(n_rows, dtype, n_rows)
    labels = ref.labels_shape("mixed", n_rows, L, n_rows + 2)
    masks = ref.masks_case(B, n_rows, seed=n_rows + 1, density=0.9)
    live = np.random.default_rng(n_rows).random(n_rows) < 0.8
    for bit0 in (0, 5, 31, 37):
        for am in (None, live):
            _check(masks, bit0, labels, L, v, and_mask=am, what="edges")
    st, _ = _check(np.zeros((B, n_rows), bool), 5, labels, L, v, what="empty", kinds=(True,))
    assert not st[0].any() and not st[5].any() and vref.is_missing(st[2]).all()
    st, _ = _check(np.ones((B, n_rows), bool), 37, labels, L, v, what="full", kinds=(True,))
    assert (st[5] == n_rows).all()


# ---- chunk edges -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_chunk_edges_never_change_the_result(dtype):
    B, L = 9, 7
    v = _values(N, dtype, 3)
    v[-1] = 5000                                                                     # the last chunk's last row carries a maximum
    labels = ref.labels_shape("mixed", N, L, 4)
    labels[-1] = 2
    masks = ref.masks_case(B, N, seed=5, density=0.7)
    masks[:, -1] = True
    first = None
    for rpc in (0, 64, 2048, 4096):
        assert facet_value_plan(N, B, L, 0, True, rpc)[2] == {0: 1, 64: 71, 2048: 3, 4096: 2}[rpc]
        for bit0 in (0, 37):
            st, h = _check(masks, bit0, labels, L, v, rpc=rpc, what="chunks")
            assert (st[3][:, 2] >= 5000).all()
            first = first or (st, h)
            _same(st, first[0])
            _same(h, first[1])


# ---- query tiles and bitmaps -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 8, 9])
def test_query_tiles(B):
    L = 6
    for dtype in DTYPES:
        v = _values(N, dtype, B)
        labels = ref.labels_shape("mixed", N, L, B + 1)
        masks = ref.masks_case(B, N, seed=B + 10, density=0.6)
        assert facet_value_plan(N, B, L, 0, True)[:2] == (0, 8)
        _check(masks, 0, labels, L, v, what="tiles")
        _check(masks, 31, labels, L, v, rpc=64, what="tiles, 64-row chunks")


@pytest.mark.parametrize("dtype", DTYPES)
def test_shared_bitmap_and_no_bitmap(dtype):
    L = 6
    v = _values(N, dtype, 4)
    labels = ref.labels_shape("mixed", N, L, 5)
    masks = ref.masks_case(1, N, seed=14, density=0.5)
    live = np.random.default_rng(6).random(N) < 0.8
    assert facet_value_plan(N, 1, L, 0, False)[:2] == (0, 1)
    for bit0 in (0, 37):
        _check(masks, bit0, labels, L, v, shared=True, what="shared")
    for am in (None, live):                                                          # words = NULL: every row set
        st, _ = _check(np.ones((1, N), bool), 0, labels, L, v, and_mask=am, words_null=True, what="words = NULL")
        assert st[5][0] == (N if am is None else live.sum())


# ---- label regimes -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,plan", [(1, (0, 8)), (2, (0, 8)), (7, (0, 8)), (256, (0, 8)), (257, (0, 4)), (2048, (0, 1)), (2049, (1, 8))])
def test_stats_label_regimes(L, plan):
    B = 9
    assert facet_value_plan(N, B, L, 0, True)[:2] == plan
    for dtype in DTYPES:
        v = _values(N, dtype, L)
        labels = ref.labels_shape("mixed", N, L, L + 1)
        labels[[0, 64, N - 1]] = (0, L - 1, L - 1)                                    # the first and the last record are used
        masks = ref.masks_case(B, N, seed=L + 2, density=0.8)
        masks[:, [0, 64, N - 1]] = True
        st, _ = _check(masks, 5, labels, L, v, what="regimes", hist=False)
        assert (st[0][:, L - 1] + st[1][:, L - 1] >= 2).all()


@pytest.mark.parametrize("L,E,plan", [(2, 2, (0, 8)), (512, 2, (0, 8)), (513, 2, (0, 4)), (2, 1022, (0, 8)), (2, 1025, (0, 4)), (4096, 2, (0, 1)),
                                      (4097, 2, (1, 8)), (16, 1022, (0, 1)), (16, 1023, (1, 8))])
def test_histogram_label_regimes(L, E, plan):
    """both sides of qt x n_labels x (n_edges + 2) = 16384 at qt = 8 and at qt = 1, through few labels and through few edges"""
    B = 9
    assert facet_value_plan(N, B, L, E + 2, True)[:2] == plan
    assert (8 * L * (E + 2) <= 16384) == (plan == (0, 8)) and (L * (E + 2) > 16384) == (plan[0] == 1)
    for dtype in DTYPES:
        v = ref.values_case(N, dtype, seed=L + E, frac_missing=0.1, frac_special=0.05, spread=600)
        e = ref.edges_case(E, dtype, spread=600) if E > 3 else (np.array([-40, 25][:E], dtype))
        labels = ref.labels_shape("mixed", N, L, L + 1)
        labels[[0, N - 1]] = L - 1
        masks = ref.masks_case(B, N, seed=E + 2, density=0.8)
        masks[:, [0, N - 1]] = True
        _, h = _check(masks, 37, labels, L, v, edges=e, what="hist regimes")
        assert h[0].sum() > 0 and h[1].sum() > 0 and h[2].sum() > 0 and h[3].sum() > 0


def test_global_regime_with_70000_labels():
    L, B = 70_000, 2
    assert facet_value_plan(N, B, L, 0, True)[:2] == (1, 8) and facet_value_plan(N, B, L, 4, True)[:2] == (1, 8)
    for dtype in DTYPES:
        v = _values(N, dtype, 70)
        labels = ref.labels_shape("mixed", N, L, 71)
        labels[:200] = L - 1                                                          # a run: the one-label path of the global regime
        labels[300:400] = 0
        masks = ref.masks_case(B, N, seed=72, density=0.9)
        masks[:, :500] = True
        st, h = _check(masks, 5, labels, L, v, edges=np.array([-1, 2], dtype), what="global")
        assert (st[0][:, L - 1] + st[1][:, L - 1] >= 200).all() and (st[0] + st[1] > 0).sum() > 2000


# ---- label shapes ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.LABEL_SHAPES)
@pytest.mark.parametrize("L", [7, 300])
def test_label_shapes(kind, L):
    """every step on one label, runs of 64 on and off the steps, random labels, labels outside the range, no label at all -- over a full
    set (the one-label path on every step) and over ragged ones"""
    B = 3
    for dtype in DTYPES:
        v = _values(N, dtype, L)
        labels = ref.labels_shape(kind, N, L, L + 3)
        masks = ref.masks_case(B, N, seed=L, density=0.9)
        masks[0] = True
        st, h = _check(masks, 5, labels, L, v, what=kind)
        if kind == "one":
            assert (st[0][:, :L - 1] == 0).all() and (st[0][0, L - 1] + st[1][0, L - 1] == N) and (st[6] == 0).all()
        if kind == "none":
            assert (st[6] == st[5]).all() and not st[0].any() and not st[1].any() and not h[0].any() and vref.is_missing(st[2]).all()
        if kind == "mixed":
            assert (st[6] > 0).all()


# ---- values ---------------------------------------------------------------------------------------------------------------------------------------------
def test_float_specials_and_the_clamp():
    L, B = 4, 3
    sp = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, 2.0 ** 20, 2.0 ** 21, -3e38, 3.4028235e38, 1e-45, -1e-45, 1.1754942e-38, 0.5], F32)
    v = np.tile(sp, N // sp.size + 1)[:N]
    labels = (np.arange(N) // sp.size % L).astype(I32)                                 # every label sees every special value
    masks = ref.masks_case(B, N, seed=1, density=0.9)
    masks[0] = True
    e = np.array([-np.inf, -1e-45, 0.0, 1e-45, 2.0 ** 20, np.inf], F32)
    st, h = _check(masks, 5, labels, L, v, edges=e, what="specials")
    assert (vref.bits(st[2][0]) == vref.bits(np.array([-np.inf], F32))[0]).all() and (st[3][0] == np.inf).all() and (st[1][0] > 0).all()
    zeros = np.where(np.arange(N) % 2 == 0, F32(-0.0), F32(0.0)).astype(F32)           # of -0.0 and +0.0 the answer is +0.0
    st, _ = _check(masks, 0, labels, L, zeros, what="zeros")
    assert (vref.bits(st[2]) == 0).all() and (vref.bits(st[3]) == 0).all() and (st[4] == 0).all()


def test_int_specials_and_sums_beyond_32_bits():
    L, B = 4, 3
    sp = np.array([ref.INT32_MIN, ref.INT32_MIN + 1, (1 << 31) - 1, (1 << 24) + 1, -(1 << 24) - 1, (1 << 30) + 3, -1, 0, 7], I32)
    v = np.tile(sp, N // sp.size + 1)[:N]
    labels = (np.arange(N) // sp.size % L).astype(I32)
    masks = ref.masks_case(B, N, seed=2, density=0.9)
    masks[0] = True
    e = np.array([ref.INT32_MIN + 1, -1, 0, (1 << 24) + 1, (1 << 31) - 1], I32)
    st, _ = _check(masks, 37, labels, L, v, edges=e, what="int specials")
    assert (st[2][0] == ref.INT32_MIN + 1).all() and (st[3][0] == (1 << 31) - 1).all() and (st[1][0] > 0).all()
    big = np.full(N, (1 << 31) - 1, I32)
    st, _ = _check(masks, 0, labels, L, big, what="big", hist=False)
    assert st[4][0].sum() == N * ((1 << 31) - 1) and (st[4][0] > 1 << 40).all()


def test_a_sum_that_wraps_2_to_the_64():
    """2^20 + 64 rows of 2^20 (fx = 2^44 each) on one label: the int64 sum passes 2^64 and holds the remainder"""
    n = (1 << 20) + 64
    v = np.full(n, 2.0 ** 20, F32)
    labels = np.zeros(n, I32)
    want = ref.stats(None, 0, 0, n, labels, 2, v)
    assert want[4][0, 0] == 64 << 44 and want[0][0, 0] == n
    _same(_raw_stats(None, 0, 0, None, 1, labels, 2, v, n, 0, True), want)
    v[::2] = -(2.0 ** 20)                                                             # and the two signs cancel exactly
    _same(_raw_stats(None, 0, 0, None, 1, labels, 2, v, n, 0, True), ref.stats(None, 0, 0, n, labels, 2, v))


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_missing_in_one_label_and_one_distinct_value(dtype):
    L, B = 5, 9
    labels = ref.labels_shape("random", N, L, 8)
    masks = ref.masks_case(B, N, seed=3, density=0.9)
    masks[0] = True
    v = _values(N, dtype, 9)
    v[labels == 2] = ref.sentinel(dtype)
    st, h = _check(masks, 5, labels, L, v, what="label 2 has no values")
    assert (st[0][:, 2] == 0).all() and (st[1][:, 2] > 0).all() and vref.is_missing(st[2][:, 2]).all() and vref.is_missing(st[3][:, 2]).all()
    assert (h[3][:, 2] == st[1][:, 2]).all() and not h[0][:, 2].any() and (st[0][:, [0, 1, 3, 4]] > 0).all()
    one = np.full(N, 7, dtype)                                                        # the most contended records and bins
    st, h = _check(masks, 5, labels, L, one, what="one value")
    assert (st[2] == 7).all() and (st[3] == 7).all() and (st[4][0] == st[0][0] * (7 if dtype == I32 else 7 << 24)).all()


# ---- agreement with the existing calls on the GPU ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_agrees_with_facet_counts_and_value_calls_on_the_gpu(dtype):
    from test_gpu_values import _raw_hist as value_hist, _raw_stats as value_stats
    B, L = 9, 11
    v = _values(N, dtype, 21)
    labels = ref.labels_shape("mixed", N, L, 22)
    e = ref.edges_case(9, dtype, spread=30)
    masks = ref.masks_case(B, N, seed=23, density=0.8)
    words = ref.pack(masks, 5, spare=1)
    ld = words.shape[1]
    count, missing, lo, hi, sm, total, other = _raw_stats(words, 5, ld, None, B, labels, L, v, N, 0, True)
    counts, below, above, hmiss, htotal, hother = _raw_hist(words, 5, ld, None, B, labels, L, v, N, e, 0, True)
    fb = _Bufs(True, dict(words=words, labels=labels), dict(counts=_junk((B, L), np.int64), total=_junk(B, np.int64), other=_junk(B, np.int64)))
    nat.check(nat.lib().vs_facet_counts(fb.p("words"), 5, ld, None, B, fb.p("labels"), N, L, 0, fb.p("counts"), L, fb.p("total"), fb.p("other"), 0, None))
    assert (count + missing == fb.out("counts")).all() and (total == fb.out("total")).all() and (other == fb.out("other")).all()
    assert (counts.sum(axis=2) + below + above + hmiss == fb.out("counts")).all() and (htotal == total).all() and (hother == other).all()
    has_label = ref.pack(((labels >= 0) & (labels < L))[None, :], 5, spare=1)[0]      # the column sums: the set ANDed with "has a label"
    vc, vm, vlo, vhi, vs = value_stats(words, 5, ld, has_label, B, v, N, 0, True)
    assert (count.sum(axis=1) == vc).all() and (missing.sum(axis=1) == vm).all() and (sm.sum(axis=1, dtype=np.int64) == vs).all()
    k = lambda a: vref.key(a.reshape(-1)).reshape(a.shape).astype(np.int64)
    assert (np.where(count > 0, k(lo), 1 << 32).min(axis=1) == np.where(vc > 0, k(vlo), 1 << 32)).all()
    assert (np.where(count > 0, k(hi), 0).max(axis=1) == np.where(vc > 0, k(vhi), 0)).all()
    hc, hb, ha, hm = value_hist(words, 5, ld, has_label, B, v, N, e, 0, True)
    assert (counts.sum(axis=1) == hc).all() and (below.sum(axis=1) == hb).all() and (above.sum(axis=1) == ha).all() and (hmiss.sum(axis=1) == hm).all()


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
    v = ref.values_case(n, I32, seed=seed, spread=60, frac_special=0.0)
    gone = v == ref.INT32_MIN
    v = v + 1950
    v[gone] = ref.INT32_MIN
    v[[1, n // 2, n - 2]] = ((1 << 24) + 1, (1 << 30) + 3, -(1 << 24) - 1)             # values fp32 cannot hold
    return v.astype(I32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_deleted_rows_never_count(dtype):
    dev, _, _, _ = _index_case()
    n, B, L = N_IDX, 9, 6
    v = _years(n, 21) if dtype == I32 else ref.values_case(n, F32, seed=21)
    e = ref.edges_case(9, dtype) if dtype == F32 else np.arange(1940, 2020, 10).astype(I32)
    labels = ref.labels_shape("mixed", n, L, 23)
    masks = ref.masks_case(B, n, seed=22, density=0.9)
    words = ref.pack(masks, 0, spare=1)
    ld = words.shape[1]
    dead = np.array([0, 1, 31, 32, 500, 998, 999])
    live = np.ones(n, bool)
    live[dead] = False
    lw = ref.pack(live[None, :])[0]
    full = ref.stats(words, ld, 0, n, labels, L, v)
    dev.delete_rows(dead)
    try:
        want = ref.stats(words, ld, 0, n, labels, L, v, lw)
        assert (want[5] < full[5]).any()
        for on_dev in (False, True):
            for rpc in (0, 64):
                _same(_raw_stats(words, 0, ld, None, B, labels, L, v, n, rpc, on_dev, index=dev), want)
                _same(_raw_hist(words, 0, ld, None, B, labels, L, v, n, e, rpc, on_dev, index=dev), ref.histogram(words, ld, 0, n, labels, L, v, e, lw))
        res = dev.facet_value_stats(labels, L, v)                                     # no filter: every live document
        assert isinstance(res, FacetValueStats) and isinstance(res.count, np.ndarray)
        _same(res, ref.stats(None, 0, 0, n, labels, L, v, lw))
        assert int(res.total[0]) == n - dead.size == dev.n_live
        flt = DocFilter.from_mask(torch.from_numpy(masks))
        res = dev.facet_value_histogram(torch.from_numpy(labels).cuda(), L, torch.from_numpy(v).cuda(), e, filter=flt)
        assert isinstance(res, FacetValueHistogram) and res.counts.is_cuda and res.counts.shape == (B, L, len(e) - 1)
        _same(res, ref.histogram(words, ld, 0, n, labels, L, v, e, lw))
        one = dev.facet_value_stats(labels.astype(np.int64), L, v, filter=torch.from_numpy(masks[0]))          # a shared mask: B = 1
        _same(one, ref.stats(words[:1], 0, 0, n, labels, L, v, lw))
    finally:
        dev.restore_rows()
    for on_dev in (False, True):
        _same(_raw_stats(words, 0, ld, None, B, labels, L, v, n, 0, on_dev, index=dev), full)


@pytest.mark.parametrize("ways", [2, 3])
def test_row_shards_equal_the_unsharded_index(ways):
    whole, _, _, _ = _index_case()
    n, B, L = N_IDX, 9, 6
    ndev = torch.cuda.device_count()
    bounds = [0, 437, n] if ways == 2 else [0, 437, 770, n]                            # no shard size a multiple of 32
    shards = [whole.slice_rows(bounds[i], bounds[i + 1] - bounds[i], device=i if ndev >= ways else 0) for i in range(ways)]
    group = ShardGroup(shards)
    masks = ref.masks_case(B, n, seed=31, density=0.9)
    flt = DocFilter.from_mask(torch.from_numpy(masks))
    words = ref.pack(masks)
    ld = words.shape[1]
    labels = ref.labels_shape("mixed", n, L, 32)
    labels[[1, n // 2, n - 2]] = 0                                                    # the rows of _years' large values carry a label
    tl = torch.from_numpy(labels).cuda()
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
                want_s, want_h = ref.stats(words, ld, 0, n, labels, L, v, lw), ref.histogram(words, ld, 0, n, labels, L, v, e, lw)
                for labs, vals in ((labels, v), (tl, tv)):
                    got = group.facet_value_stats(labs, L, vals, filter=flt)
                    assert isinstance(got.count, torch.Tensor) == isinstance(labs, torch.Tensor)
                    _same(got, want_s, "group stats")
                    _same(whole.facet_value_stats(labs, L, vals, filter=flt), want_s, "whole stats")
                    _same(group.facet_value_stats(labs, L, vals), ref.stats(None, 0, 0, n, labels, L, v, lw))
                    _same(group.facet_value_histogram(labs, L, vals, e, filter=flt), want_h, "group histogram")
                    _same(whole.facet_value_histogram(labs, L, vals, e, filter=flt), want_h, "whole histogram")
            group.restore_rows()
            whole.restore_rows()
        assert int(_np(group.facet_value_stats(tl, L, torch.from_numpy(_years(n, 5)).cuda()).max).max()) == (1 << 30) + 3      # unrounded through the merge
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
    n, B, L = N_IDX, 9, 5
    tq = torch.from_numpy(q)
    sp = _sparse_index(ip, ix, va, n)
    years = _years(n, 41)
    price = ref.values_case(n, F32, seed=42)
    topic = ref.labels_case(n, L, seed=43, frac_none=0.1)
    groups = (np.arange(n) // 7).astype(np.int64)
    n_groups = int(groups.max()) + 1
    sp.set_values("year", years.astype(np.int64), missing=years == ref.INT32_MIN)
    sp.set_values("price", price.astype(np.float64))
    sp.set_facet("topic", topic, names=[f"t{i}" for i in range(L)])
    sp.set_groups(groups)
    with pytest.raises(KeyError):
        sp.stats_by_facet("nope", "topic")
    with pytest.raises(KeyError):
        sp.stats_by_facet("year", "nope")
    thr = _mid_thresholds(S, B, 150)
    w = _np(sp.match_filter(tq, thr).words).view(np.uint32)
    ld = w.shape[1]
    st = sp.stats_by_facet("year", "topic", tq, thr)
    want = ref.stats(w, ld, 0, n, topic, L, years)
    assert isinstance(st, FacetValueStats)
    _same(st, want)
    assert (_np(st.total) == _np(sp.count_matches(tq, thr))).all() and (want[0] > 5).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(_np(st.mean()), np.where(want[0] > 0, want[4] / want[0], np.nan), equal_nan=True)
    e = [1940, 1960, 1980, 2000, 2020]
    h = sp.histogram_by_facet("year", "topic", e, tq, thr)
    assert isinstance(h, FacetValueHistogram)
    _same(h, ref.histogram(w, ld, 0, n, topic, L, years, e))
    # "groups" as the facet field; a float field; no queries: the filter alone, B = 1
    _same(sp.stats_by_facet("price", "groups", tq, thr), ref.stats(w, ld, 0, n, groups, n_groups, price))
    _same(sp.histogram_by_facet("price", "groups", [-50.0, 0.0, 50.0], tq, thr), ref.histogram(w, ld, 0, n, groups, n_groups, price, [-50.0, 0.0, 50.0]))
    _same(sp.stats_by_facet("price", "topic"), ref.stats(None, 0, 0, n, topic, L, price))
    vf = sp.value_filter("year", 1960, 1999)
    in_range = vref.range_masks(years, [1960], [1999])
    _same(sp.stats_by_facet("price", "groups", filter=vf), ref.stats(ref.pack(in_range), 0, 0, n, groups, n_groups, price))
    # delete -> compact -> add(..., facets=, values=): the fields stay aligned with the documents
    dead = np.array([0, 5, 64, 500, 999])
    live = np.ones(n, bool)
    live[dead] = False
    sp.delete(dead)
    _same(sp.stats_by_facet("year", "groups"), ref.stats(None, 0, 0, n, groups, n_groups, years, ref.pack(live[None, :])[0]))
    sp.compact()
    _same(sp.stats_by_facet("year", "groups"), ref.stats(None, 0, 0, n - dead.size, groups[live], n_groups, years[live]))
    _same(sp.histogram_by_facet("year", "topic", e), ref.histogram(None, 0, 0, n - dead.size, topic[live], L, years[live], e))
    new = torch.zeros(3, VR)
    new[:, 5] = 1.0
    sp.add(new, groups=[1, 2, n_groups], facets={"topic": [2, 2, -1]}, values={"year": [2024, 1900, 2024], "price": [1.5, float("nan"), -2.5]})
    years2 = np.concatenate([years[live], np.array([2024, 1900, 2024], I32)])
    price2 = np.concatenate([price[live], np.array([1.5, np.nan, -2.5], F32)])
    topic2 = np.concatenate([topic[live], np.array([2, 2, -1], I32)])
    groups2 = np.concatenate([groups[live], [1, 2, n_groups]])
    st = sp.stats_by_facet("year", "groups")
    _same(st, ref.stats(None, 0, 0, n - 2, groups2, n_groups + 1, years2))
    assert int(_np(st.max)[0, 1]) == 2024 and int(_np(st.count)[0, n_groups]) == 1
    _same(sp.stats_by_facet("price", "topic"), ref.stats(None, 0, 0, n - 2, topic2, L, price2))
    _same(sp.histogram_by_facet("price", "topic", [-2.5, 1.5]), ref.histogram(None, 0, 0, n - 2, topic2, L, price2, [-2.5, 1.5]))


def test_sharded_facade_equals_the_single_index():
    _, q, S, (ip, ix, va) = _index_case()
    n, B, L = N_IDX, 9, 5
    tq = torch.from_numpy(q)
    years = _years(n, 51)
    thr = _mid_thresholds(S, B, 150)
    sp = _sparse_index(ip, ix, va, n)
    sp.set_values("year", years, missing=years == ref.INT32_MIN)
    topic = ref.labels_case(n, L, seed=52, frac_none=0.1)
    topic[[1, n // 2, n - 2]] = 0                                                     # the rows of _years' large values carry a label
    sp.set_facet("topic", topic)
    sp.set_groups((np.arange(n) // 7).astype(np.int64))
    e = [1940, 1960, 1980, 2000, 2020]
    calls = (lambda: sp.stats_by_facet("year", "topic", tq, thr), lambda: sp.histogram_by_facet("year", "topic", e, tq, thr),
             lambda: sp.stats_by_facet("year", "groups", tq, thr), lambda: sp.stats_by_facet("year", "topic"))
    want = [tuple(_np(t) for t in c()) for c in calls]
    sp.shard_rows([0, 0, 0])
    assert sp.shards is not None and len(sp.shards) == 3
    for c, w in zip(calls, want):
        _same(c(), w)
    assert int(_np(sp.stats_by_facet("year", "topic").max).max()) == (1 << 30) + 3    # an int32 beyond 2^24 came through the merge unrounded


# ---- the retriever -----------------------------------------------------------------------------------------------------------------------------------
def test_retrieve_stats_and_histogram_by_facet(tiny_retriever):
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
    assert (ref.unpack(words, 0, n) == (sc >= thr[:, None])).all()

    def want_rows(w, topn, min_count=1):
        count, missing, lo, hi, sm, total, _ = ref.stats(w, w.shape[1], 0, n, codes, 3, years)
        wl, wc = fref.topn(count + missing, topn, min_count)                           # documents descending, label ascending
        rows = [[(names[l], int(d), int(count[b, l]), int(lo[b, l]) if count[b, l] else None, int(hi[b, l]) if count[b, l] else None,
                  float(sm[b, l] / count[b, l]) if count[b, l] else float("nan")) for l, d in zip(wl[b], wc[b]) if l >= 0] for b in range(w.shape[0])]
        return rows, total.tolist()

    def same_rows(got, want):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert [x[:5] for x in g] == [x[:5] for x in w]
            assert all((a[5] == b[5]) or (a[5] != a[5] and b[5] != b[5]) for a, b in zip(g, w))

    rows, totals = r.retrieve_stats_by_facet(queries, "year", "lang", thr, topn=5)
    want, want_totals = want_rows(words, 5)
    same_rows(rows, want)
    assert totals == want_totals == _np(r.retrieve_range(queries, thr, max_hits=0).counts).tolist()
    rows, _ = r.retrieve_stats_by_facet(queries, "year", "lang", thr, topn=2, min_count=3)
    same_rows(rows, want_rows(words, 2, 3)[0])
    e = [1950, 1970, 1990, 2010]
    h = r.retrieve_histogram_by_facet(queries, "year", "lang", e, thr)
    assert isinstance(h, FacetValueHistogram)
    _same(h, ref.histogram(words, words.shape[1], 0, n, codes, 3, years, e))
    # term constraints act through the match set
    cols = _np(idx.get_vectors(torch.tensor([3])).col_indices())
    col = int(cols[_np(idx.doc_freq(cols)).argmax()])
    wm = _np(idx.match_filter(q_emb, thr, filter=r.term_filter(must=[col])).words).view(np.uint32)
    rows, totals = r.retrieve_stats_by_facet(queries, "year", "lang", thr, must=[col])
    want, want_totals = want_rows(wm, 10)
    same_rows(rows, want)
    assert totals == want_totals and 0 < sum(totals)
    _same(r.retrieve_histogram_by_facet(queries, "year", "lang", e, thr, must=[col]), ref.histogram(wm, wm.shape[1], 0, n, codes, 3, years, e))
