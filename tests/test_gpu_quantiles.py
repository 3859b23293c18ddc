"""GPU tests of the percentiles (vs_value_quantiles / vs_value_radix_counts / vs_value_radix_step and their vs_index_* variants; DeviceIndex /
ShardGroup .value_quantiles, Index.percentiles / .median, Retriever.retrieve_percentiles) -- run on MI355X.

The contract is tests/_quantile_ref.py.  Every result is an integer or a 32-bit pattern, so everything compares exactly.  The
raw calls go into junk-filled outputs, once on host buffers and once on device buffers."""
import ctypes as C

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, ShardGroup, ValuePercentiles, ValueQuantiles, quantile_lerp, value_quantile_plan, value_radix_step
from vsearch_amd.doc_filter import DocFilter
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

import _quantile_ref as qref
import _range_ref as rref
import _value_ref as ref

pytestmark = pytest.mark.gpu

F32, I32 = np.float32, np.int32
DTYPES = [F32, I32]
JUNK = -0x5A5A5A5A5A5A5A5B
JUNK32 = 0x5A5A5A5A
VR = 2000
N_IDX = 1000
Q3 = [0.0, 0.5, 1.0]
METHODS = ["lower", "higher", "nearest"]


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


def _raw(words, bit0, ld, aw, B, v, n, on_dev, q=None, method="lower", ranks=None, rpc=0, index=None):
    """one vs_value_quantiles / vs_index_value_quantiles call -> (values [B, R], ranks [B, R], count, missing)"""
    R = len(q) if q is not None else np.asarray(ranks).shape[1]
    b = _Bufs(on_dev, dict(words=words, aw=aw, v=v, q=None if q is None else np.asarray(q, np.float64),
                           ranks=None if ranks is None else np.asarray(ranks, np.int64)),
              dict(vals=_junk((B, R), v.dtype), rk=_junk((B, R), np.int64), count=_junk(B, np.int64), missing=_junk(B, np.int64)))
    outs = [b.p(k) for k in ("vals", "rk", "count", "missing")]
    m = qref.METHODS[method]
    if index is None:
        rc = nat.lib().vs_value_quantiles(b.p("words"), bit0, ld, b.p("aw"), B, b.p("v"), _dt(v), n, b.p("q"), m, b.p("ranks"), R, rpc, *outs, 0, None)
    else:
        rc = nat.lib().vs_index_value_quantiles(index._h, b.p("words"), bit0, ld, B, b.p("v"), _dt(v), b.p("q"), m, b.p("ranks"), R, rpc, *outs, None)
    nat.check(rc)
    return tuple(b.out(k) for k in ("vals", "rk", "count", "missing"))


def _check(masks, bit0, v, q=None, method="lower", ranks=None, and_mask=None, rpc=0, shared=False, what=None):
    """per-query sets `masks` [B, n] packed at bit0 with every spare bit set -> the call, both buffer kinds, against the sort"""
    B, n = masks.shape
    words = ref.pack(masks, bit0, spare=1)
    aw = ref.pack(and_mask[None, :], bit0, spare=1)[0] if and_mask is not None else None
    ld = 0 if shared else words.shape[1]
    want = qref.order_statistics(words, ld, bit0, n, v, q=q, method=method, ranks=ranks, and_words=aw)
    for on_dev in (False, True):
        _same(_raw(words, bit0, ld, aw, B, v, n, on_dev, q=q, method=method, ranks=ranks, rpc=rpc), want, (what, on_dev, bit0, rpc, method))
    return want


# ---- row and bit edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049])
def test_row_and_bit_edges(n_rows, dtype):
    B = 3
    v = ref.values_case(n_rows, dtype, seed=n_rows, frac_missing=0.15, frac_special=0.1, spread=30)
    masks = ref.masks_case(B, n_rows, seed=n_rows + 1, density=0.9)
    live = np.random.default_rng(n_rows).random(n_rows) < 0.8
    for bit0 in (0, 5, 37):
        for method in METHODS:
            want = _check(masks, bit0, v, q=Q3, method=method, and_mask=live, what="edges")
            size = (masks & live[None, :]).sum(axis=1)
            assert (want[2] + want[3] == size).all()
        _check(masks[:1], bit0, v, q=Q3, method="nearest", shared=True, what="shared")
    aw = ref.pack(live[None, :], 0, spare=1)[0]
    for on_dev in (False, True):                                                      # words = NULL: every row set
        for a in (None, aw):
            _same(_raw(None, 0, 0, a, 1, v, n_rows, on_dev, q=Q3, method="higher"), qref.order_statistics(None, 0, 0, n_rows, v, q=Q3, method="higher", and_words=a))


# ---- chunk edges -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_rows,chunks", [(3 * 2048 + 1, 4), (4 * 2048, 4)])
def test_chunk_edges(n_rows, chunks, dtype):
    """rows_per_chunk = 2048: four chunks, the last of one row / a full one; the last row carries the largest or the smallest value"""
    B = 9
    assert value_quantile_plan(n_rows, B, 3, True, 2048) == (4, chunks, 2048)
    for top in (True, False):
        v = ref.values_case(n_rows, dtype, seed=n_rows, spread=100, frac_special=0.0)
        v[-1] = 5000 if top else -5000
        masks = ref.masks_case(B, n_rows, seed=5, density=0.7)
        masks[:, -1] = True                                                           # the one-row chunk holds a member
        for bit0 in (0, 37):
            want = _check(masks, bit0, v, q=Q3, rpc=2048, what="chunks")
            assert (want[0][:, 2 if top else 0] == v[-1]).all()
            _check(masks, bit0, v, q=Q3, rpc=0, what="automatic chunks")            # equal to rows_per_chunk = 0


# ---- query tiles -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 8, 9, 16])
def test_query_tiles(R):
    n = 5000
    qt = 8 if R <= 2 else 4 if R <= 4 else 2 if R <= 8 else 1
    q = np.linspace(0.0, 1.0, R) if R > 1 else np.array([0.5])
    for B in (1, 7, 8, 9, 17):
        got = value_quantile_plan(n, B, R, True)
        assert got[0] == qt and got == (qt, 1, 8192)
        o32, o64a, o64b = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        nat.check(nat.lib().vs_value_quantile_plan(n, B, R, 1, 0, C.byref(o32), C.byref(o64a), C.byref(o64b)))
        assert (o32.value, o64a.value, o64b.value) == got
        dtype = DTYPES[(B + R) & 1]
        v = ref.values_case(n, dtype, seed=B + R)
        masks = ref.masks_case(B, n, seed=B + 10, density=0.6)
        _check(masks, 31, v, q=q, method=METHODS[B % 3], what="tiles")
        _check(masks, 0, v, q=q, method="nearest", rpc=64, what="tiles, 64-row chunks")
    assert value_quantile_plan(n, 1, R, False)[0] == 1


# ---- digit edges -------------------------------------------------------------------------------------------------------------------------------------
def _digit_keys(level, dtype):
    """48 keys of values in four groups of 12; inside a group only the level's digit differs: the two smallest and two largest digits, the
    ones next to them and four in the middle.  The top digit of a float32 value lies in 4..2043 (below and above are the NaN patterns)."""
    lo, hi = (0, 2047) if dtype == I32 else (4, 2043)
    dlo, dhi = (lo, hi) if level == 0 else (0, 2047 if level == 1 else 1023)
    mid = (dlo + dhi) // 2
    digs = [dlo, dlo + 1, dlo + 2, dlo + 3, mid - 1, mid, mid + 1, mid + 2, dhi - 3, dhi - 2, dhi - 1, dhi]
    keys = []
    for a, c in [(lo, 1), (hi, 1023), (1024, 512), (lo + 1, 2)]:                        # the other two digits of a group
        for d in digs:
            keys.append((d << 21) | (a << 10) | c if level == 0 else (a << 21) | (d << 10) | c if level == 1 else (a << 21) | (c << 10) | d)
    return np.array(keys, np.uint64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("level", [0, 1, 2])
def test_digit_edges(level, dtype):
    keys = _digit_keys(level, dtype)
    v = qref.unkey(keys, dtype)
    n = v.shape[0]
    assert n == 48 and np.unique(keys).size == 48 and (ref.key(v) == keys).all() and not ref.is_missing(v).any()
    if dtype == I32:
        d = (keys >> qref.LEVEL_SHIFT[level]) & (qref.LEVEL_BINS[level] - 1)
        assert {0, 1, qref.LEVEL_BINS[level] - 2, qref.LEVEL_BINS[level] - 1} <= set(d.tolist())
    v = v[np.random.default_rng(level).permutation(n)]
    masks = np.ones((2, n), bool)
    masks[1, ::3] = False
    all_ranks = np.arange(48, dtype=np.int64)
    for j0 in (0, 16, 32):                                                            # all 48 ranks in three calls of 16
        ranks = np.tile(all_ranks[j0:j0 + 16], (2, 1))
        want = _check(masks, 5, v, ranks=ranks, what=("digits", level, j0))
        assert (ref.key(want[0][0]) == np.sort(keys)[j0:j0 + 16]).all() and (want[1][1, -1] == -1) == (j0 == 32)


# ---- slots ---------------------------------------------------------------------------------------------------------------------------------------------
def test_slots():
    k = lambda a, b, c: (a << 21) | (b << 10) | c
    keys = np.array([k(5, 3, 1), k(5, 3, 2), k(5, 9, 0), k(700, 0, 4), k(700, 0, 4)] + [k(100 + 60 * i, i, i) for i in range(16)], np.uint64)
    v = qref.unkey(keys, I32)
    order = np.argsort(keys, kind="stable")
    n = v.shape[0]
    full = np.ones((1, n), bool)
    pos = {int(i): int(r) for r, i in enumerate(order)}
    cases = {
        "part at the middle digit": [pos[0], pos[2]],
        "part at the last digit": [pos[0], pos[1]],
        "the same rank twice": [pos[2], pos[2], pos[3], pos[4]],
        "16 top bins": [pos[5 + i] for i in range(16)],
        "unsorted ranks": [pos[20], pos[0], pos[4], pos[1], pos[12]],
    }
    for what, ranks in cases.items():
        want = _check(full, 0, v, ranks=np.array([ranks], np.int64), what=what)
        assert ref.key(want[0][0]).tolist() == [int(np.sort(keys)[r]) for r in ranks]
    for dtype in DTYPES:                                                              # 16 ranks on an all-equal field: one slot, the add-once path
        same = np.full(5000, 7, dtype)
        masks = ref.masks_case(3, 5000, seed=1, density=0.8)
        want = _check(masks, 37, same, q=np.linspace(0, 1, 16), method="nearest", what="all equal")
        assert (want[0] == 7).all()


# ---- extremes ----------------------------------------------------------------------------------------------------------------------------------------
def test_extremes():
    vi = np.array([ref.INT32_MIN + 1, (1 << 31) - 1, (1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 3, ref.INT32_MIN, 0, -1], I32)
    ranks = np.arange(8, dtype=np.int64)[None, :]
    want = _check(np.ones((1, 8), bool), 0, vi, ranks=ranks, what="int extremes")
    assert want[0][0].tolist() == [ref.INT32_MIN + 1, -1, 0, (1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 3, (1 << 31) - 1, ref.INT32_MIN]
    assert want[1][0].tolist() == [0, 1, 2, 3, 4, 5, 6, -1] and want[2][0] == 7 and want[3][0] == 1
    den = np.nextafter(F32(0), F32(1))
    vf = np.array([np.inf, -np.inf, -0.0, 0.0, -0.0, den, -den, np.nan, 1.1754942e-38, -3.4028235e38], F32)
    ranks = np.arange(10, dtype=np.int64)[None, :]
    want = _check(np.ones((1, 10), bool), 33, vf, ranks=ranks, what="float extremes")
    assert ref.bits(want[0][0, 2:6]).tolist() == [ref.bits(np.array([-den], F32))[0], 0, 0, 0]       # of -0.0 / +0.0 the answer is +0.0
    assert want[0][0, 0] == -np.inf and want[0][0, 8] == np.inf and ref.bits(want[0][0, 9:])[0] == ref.NAN_BITS
    _check(np.ones((1, 10), bool), 0, vf, q=Q3, what="float extremes, quantiles")


# ---- empty answers -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_answers(dtype):
    n = 300
    v = ref.values_case(n, dtype, seed=9, frac_missing=0.2)
    masks = np.zeros((4, n), bool)                                                     # query 0: the empty set
    masks[1, np.flatnonzero(ref.is_missing(v))] = True                                 # missing rows only
    masks[2, np.flatnonzero(~ref.is_missing(v))[7]] = True                             # one value
    masks[3] = True
    for method in METHODS:
        want = _check(masks, 5, v, q=Q3, method=method, what="empty")
        assert want[2].tolist()[:3] == [0, 0, 1] and want[3][0] == 0 and want[3][1] == masks[1].sum() and want[3][2] == 0
        assert ref.is_missing(want[0][:2]).all() and (want[1][:2] == -1).all() and (want[1][2] == 0).all()
        assert (want[0][2] == v[masks[2]][0] + v.dtype.type(0)).all()
    count = int((~ref.is_missing(v)).sum())
    ranks = np.array([[0, 1], [0, 5], [0, 1], [count - 1, count]], np.int64)           # a rank at the count
    want = _check(masks, 5, v, ranks=ranks, what="rank past the count")
    assert want[1].tolist() == [[-1, -1], [-1, -1], [0, -1], [count - 1, -1]]
    # a NaN / out-of-range q on the device is not read on the host: the missing result, count and missing still right
    words = ref.pack(masks, 5, spare=1)
    got = _raw(words, 5, words.shape[1], None, 4, v, n, True, q=[np.nan, 0.5, 1.5, -0.5], method="lower")
    good = qref.order_statistics(words, words.shape[1], 5, n, v, q=[0.5], method="lower")
    assert ref.is_missing(got[0][:, [0, 2, 3]]).all() and (got[1][:, [0, 2, 3]] == -1).all()
    assert ref.same(got[0][:, 1:2], good[0]) and (got[1][:, 1:2] == good[1]).all() and (got[2] == good[2]).all() and (got[3] == good[3]).all()
    with pytest.raises(ValueError, match="outside"):
        _raw(words, 5, words.shape[1], None, 4, v, n, False, q=[np.nan, 0.5], method="lower")


# ---- skew ------------------------------------------------------------------------------------------------------------------------------------------------
def test_years_every_row_in_one_bin():
    n, B = 20_000, 9
    rng = np.random.default_rng(11)
    v = rng.integers(1900, 2030, size=n).astype(I32)
    v[rng.random(n) < 0.05] = ref.INT32_MIN
    k = ref.key(v[v != ref.INT32_MIN])
    assert np.unique(k >> 21).size == 1 and np.unique(k >> 10).size == 1                # one bin at levels 0 and 1
    masks = ref.masks_case(B, n, seed=12, density=0.5)
    masks[0] = True
    q = [0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0]
    want = _check(masks, 0, v, q=q, method="nearest", what="years")
    assert want[0][0, 0] == 1900 and want[0][0, -1] == 2029
    _check(masks, 33, v, q=[0.5], method="lower", what="years, median")


# ---- the level ABI -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_levels_compose_to_the_call(dtype):
    n, B, R = 5000, 5, 7
    v = ref.values_case(n, dtype, seed=3, spread=400, frac_special=0.1)
    masks = ref.masks_case(B, n, seed=4, density=0.7)
    live = np.random.default_rng(5).random(n) < 0.9
    bit0 = 37
    words = ref.pack(masks, bit0, spare=1)
    aw = ref.pack(live[None, :], bit0, spare=1)[0]
    ld = words.shape[1]
    q = np.array([0.0, 0.1, 0.5, 0.5, 0.9, 0.999, 1.0])
    trace = []
    want = qref.radix_select(words, ld, bit0, n, v, q=q, method="nearest", and_words=aw, trace=trace)
    _same(want, qref.order_statistics(words, ld, bit0, n, v, q=q, method="nearest", and_words=aw))
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a)).to(dev)
    d_w, d_a, d_v, d_q = t(words), t(aw), t(v), t(q)
    state, missing = None, None
    for level in range(3):
        S, bins = (1 if level == 0 else R), qref.LEVEL_BINS[level]
        for on_dev in (True, False):
            counts = torch.full((B, S, bins), JUNK, dtype=torch.int64, device=dev) if on_dev else np.full((B, S, bins), JUNK, np.int64)
            mis = torch.full((B,), JUNK, dtype=torch.int64, device=dev) if on_dev else np.full(B, JUNK, np.int64)
            if on_dev:
                args = [d_w, d_a, d_v, state["slot_prefix"] if level else None, state["n_slots"] if level else None]
                ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
            else:
                args = [words, aw, v, _np(state["slot_prefix"]) if level else None, _np(state["n_slots"]) if level else None]
                ptr = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
            nat.check(nat.lib().vs_value_radix_counts(ptr(args[0]), bit0, ld, ptr(args[1]), B, ptr(args[2]), _dt(v), n, level, R, ptr(args[3]), ptr(args[4]),
                                                      0, ptr(counts), ptr(mis) if level == 0 else None, 0, None))
            assert (_np(counts) == trace[level][0]).all(), ("counts", level, on_dev)   # each level's counts are the reference's digit histograms
            if level == 0:
                assert (_np(mis) == want[3]).all()
            else:
                assert (_np(mis) == JUNK).all()
            if on_dev:
                dev_counts = counts
        state = value_radix_step(level, dev_counts, R, state, d_q, qref.NEAREST, None, d_v.dtype, 0)
        for name, w in trace[level][1].items():
            if name in ("count", "ranks", "values"):
                continue
            assert (_np(state[name]).view(w.dtype) == w).all(), (name, level)
    got = (_np(state["values"]), _np(state["ranks"]), _np(state["count"]), want[3])
    _same(got, want, "composed")
    _same(_raw(words, bit0, ld, aw, B, v, n, True, q=q, method="nearest"), want, "all in one")


# ---- index level -------------------------------------------------------------------------------------------------------------------------------------------
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


QS = [0.0, 0.01, 0.25, 0.5, 0.75, 0.99, 1.0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_deleted_rows_never_count(dtype):
    dev, _, _, _ = _index_case()
    n, B = N_IDX, 9
    v = _years(n, 21) if dtype == I32 else ref.values_case(n, F32, seed=21)
    masks = ref.masks_case(B, n, seed=22, density=0.9)
    words = ref.pack(masks, 0, spare=1)
    ld = words.shape[1]
    dead = np.array([0, 1, 31, 32, 500, 998, 999])
    live = np.ones(n, bool)
    live[dead] = False
    lw = ref.pack(live[None, :])[0]
    full = qref.order_statistics(words, ld, 0, n, v, q=QS, method="higher")
    dev.delete_rows(dead)
    try:
        want = qref.order_statistics(words, ld, 0, n, v, q=QS, method="higher", and_words=lw)
        assert (want[2] + want[3] < full[2] + full[3]).any()
        for on_dev in (False, True):
            for rpc in (0, 64):
                _same(_raw(words, 0, ld, None, B, v, n, on_dev, q=QS, method="higher", rpc=rpc, index=dev), want)
        res = dev.value_quantiles(v, q=QS, method="higher")                            # no filter: every live document; numpy in, numpy out
        assert isinstance(res, ValueQuantiles) and isinstance(res.values, np.ndarray)
        _same(res, qref.order_statistics(None, 0, 0, n, v, q=QS, method="higher", and_words=lw))
        res = dev.value_quantiles(torch.from_numpy(v).cuda(), ranks=[0, 3, 10 ** 7], filter=DocFilter.from_mask(torch.from_numpy(masks)))
        assert res.values.is_cuda
        _same(res, qref.order_statistics(words, ld, 0, n, v, ranks=np.tile(np.array([0, 3, 10 ** 7], np.int64), (B, 1)), and_words=lw))
    finally:
        dev.restore_rows()
    for on_dev in (False, True):
        _same(_raw(words, 0, ld, None, B, v, n, on_dev, q=QS, method="higher", index=dev), full)


@pytest.mark.parametrize("ways", [2, 3])
def test_row_shards_equal_the_unsharded_index(ways):
    whole, _, _, _ = _index_case()
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
    q20 = np.linspace(0.0, 1.0, 20)                                                    # more than 16: two batches
    try:
        for v in (_years(n, 5), ref.values_case(n, F32, seed=6)):
            tv = torch.from_numpy(v).cuda()
            for lw in (None, ref.pack(live[None, :])[0]):
                if lw is not None:
                    group.delete_rows(dead)
                    whole.delete_rows(dead)
                for method in ("lower", "nearest"):
                    want = qref.order_statistics(words, ld, 0, n, v, q=q20, method=method, and_words=lw)
                    _same(qref.radix_select(words, ld, 0, n, v, q=q20[:16], method=method, and_words=lw, cuts=bounds),
                          tuple(w[:, :16] if w.ndim == 2 else w for w in want))
                    for vals in (v, tv):
                        _same(group.value_quantiles(vals, q=q20, method=method, filter=flt), want, "group")
                        _same(whole.value_quantiles(vals, q=q20, method=method, filter=flt), want, "whole")
                _same(group.value_quantiles(tv, q=[0.5]), qref.order_statistics(None, 0, 0, n, v, q=[0.5], and_words=lw))
                rk = np.array([0, 5, 436, 437, 999], np.int64)
                _same(group.value_quantiles(tv, ranks=rk, filter=flt), qref.order_statistics(words, ld, 0, n, v, ranks=np.tile(rk, (B, 1)), and_words=lw))
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


def _linear(words, ld, n, v, pcts):
    """percentiles(method="linear") by the definition: floor and ceil selected by the sort, the project's formula in fp64"""
    q = np.asarray(pcts, np.float64) / 100.0
    lo = qref.order_statistics(words, ld, 0, n, v, q=q, method="lower")
    hi = qref.order_statistics(words, ld, 0, n, v, q=q, method="higher")
    pos = q[None, :] * (lo[2].astype(np.float64) - 1.0)[:, None]
    out = qref.lerp(lo[0], hi[0], pos - np.floor(pos))
    return np.where(lo[1] < 0, np.nan, out), lo[2], lo[3]


def _close_to_numpy(got, x, pcts):
    """got [P] against np.quantile(method="linear") over the values x, within 4 * 2^-52 * max(|lo|, |hi|): a handful of fp64 roundings of two
    differently arranged lerps between the same two order statistics.  Where lo == hi the answer is exactly lo (numpy gives NaN between two
    equal infinities); between an infinity and anything else both sides give the same infinity or NaN."""
    x = np.sort(x.astype(np.float64))
    q = np.asarray(pcts, np.float64) / 100.0
    pos = q * float(x.size - 1)
    lo, hi = x[np.floor(pos).astype(int)], x[np.ceil(pos).astype(int)]
    with np.errstate(invalid="ignore"):
        want = np.quantile(x, q, method="linear")
    same, fin = lo == hi, np.isfinite(lo) & np.isfinite(hi)
    assert (got[same] == lo[same]).all()
    assert (np.abs(got - want)[fin] <= (4 * 2.0 ** -52 * np.maximum(np.abs(lo), np.abs(hi)))[fin]).all()
    rest = ~same & ~fin
    assert ((got[rest] == want[rest]) | (np.isnan(got[rest]) & np.isnan(want[rest]))).all()


def _same64(got, want):
    g, w = _np(got), np.asarray(want)
    assert g.dtype == np.float64 and g.shape == w.shape and (g.view(np.uint64)[~np.isnan(w)] == w.view(np.uint64)[~np.isnan(w)]).all()
    assert (np.isnan(g) == np.isnan(w)).all()


def test_index_facade_follows_the_index():
    _, q, S, (ip, ix, va) = _index_case()
    n, B = N_IDX, 9
    tq = torch.from_numpy(q)
    sp = _sparse_index(ip, ix, va, n)
    years = _years(n, 41)
    price = ref.values_case(n, F32, seed=42)
    sp.set_values("year", years.astype(np.int64), missing=years == ref.INT32_MIN)
    sp.set_values("price", price.astype(np.float64))
    thr = _mid_thresholds(S, B, 150)
    w = _np(sp.match_filter(tq, thr).words).view(np.uint32)
    ld = w.shape[1]
    pcts = [0, 5, 25, 50, 75, 95, 100]
    for field, v in (("year", years), ("price", price)):
        for method in METHODS:
            res = sp.percentiles(field, pcts, tq, thr, method=method)
            assert isinstance(res, ValuePercentiles)
            want = qref.order_statistics(w, ld, 0, n, v, q=np.array(pcts) / 100.0, method=method)
            _same((res.values, res.count, res.missing), (want[0], want[2], want[3]), (field, method))
        res = sp.percentiles(field, pcts, tq, thr)                                    # linear
        wl = _linear(w, ld, n, v, pcts)
        _same64(res.values, wl[0])
        assert (_np(res.count) == wl[1]).all() and (_np(res.missing) == wl[2]).all()
        med = sp.median(field, tq, thr)
        _same64(med.values, wl[0][:, 3:4])
        # numpy over the match set, within the bound of the linear formula
        for b in range(B):                                                            # numpy over the match set
            _close_to_numpy(_np(res.values)[b], v[ref.unpack(w, 0, n)[b] & ~ref.is_missing(v)], pcts)
    many = np.linspace(0, 100, 40)                                                     # more than 16 percentiles: batches
    want = qref.order_statistics(None, 0, 0, n, years, q=many / 100.0, method="nearest")
    res = sp.percentiles("year", many, method="nearest")
    _same((res.values, res.count, res.missing), (want[0], want[2], want[3]), "batches")
    _same64(sp.percentiles("price", many).values, _linear(None, 0, n, price, many)[0])
    # delete -> compact -> add(values=): the fields stay aligned with the documents
    dead = np.array([0, 5, 64, 500, 999])
    live = np.ones(n, bool)
    live[dead] = False
    sp.delete(dead)
    want = qref.order_statistics(None, 0, 0, n, years, q=[0.5], method="lower", and_words=ref.pack(live[None, :])[0])
    assert ref.same(_np(sp.median("year", method="lower").values), want[0])
    sp.compact()
    want = qref.order_statistics(None, 0, 0, n - dead.size, years[live], q=[0.5], method="lower")
    assert ref.same(_np(sp.median("year", method="lower").values), want[0])
    new = torch.zeros(3, VR)
    new[:, 5] = 1.0
    sp.add(new, values={"year": [2024, 1900, 2024], "price": [1.5, float("nan"), -2.5]})
    years2 = np.concatenate([years[live], np.array([2024, 1900, 2024], I32)])
    price2 = np.concatenate([price[live], np.array([1.5, np.nan, -2.5], F32)])
    res = sp.percentiles("year", [0, 50, 100], method="higher")
    want = qref.order_statistics(None, 0, 0, n - 2, years2, q=[0, 0.5, 1], method="higher")
    _same((res.values, res.count, res.missing), (want[0], want[2], want[3]))
    _same64(sp.percentiles("price", [10, 50, 90]).values, _linear(None, 0, n - 2, price2, [10, 50, 90])[0])
    none = sp.percentiles("year", [50], filter=sp.value_filter("year", (1 << 31) - 1, None))   # a set without values: NaN, not the int sentinel
    assert np.isnan(_np(none.values)).all() and int(_np(none.count)[0]) == 0


def test_sharded_facade_equals_the_single_index():
    _, q, S, (ip, ix, va) = _index_case()
    n, B = N_IDX, 9
    tq = torch.from_numpy(q)
    years = _years(n, 51)
    thr = _mid_thresholds(S, B, 150)
    sp = _sparse_index(ip, ix, va, n)
    sp.set_values("year", years, missing=years == ref.INT32_MIN)
    pcts = np.linspace(0, 100, 21)
    want = [tuple(_np(t) for t in sp.percentiles("year", pcts, tq, thr, method=m)) for m in ("linear", "nearest")]
    want_all = tuple(_np(t) for t in sp.median("year", method="higher"))
    sp.shard_rows([0, 0, 0])
    assert sp.shards is not None and len(sp.shards) == 3
    for m, w in zip(("linear", "nearest"), want):
        got = tuple(_np(t) for t in sp.percentiles("year", pcts, tq, thr, method=m))
        assert all(g.dtype == x.dtype and g.tobytes() == x.tobytes() for g, x in zip(got, w)), m
    got = tuple(_np(t) for t in sp.median("year", method="higher"))
    assert all(g.tobytes() == x.tobytes() for g, x in zip(got, want_all))
    assert int(_np(sp.percentiles("year", [100], method="lower").values)[0, 0]) == (1 << 30) + 3     # an int32 beyond 2^24 came through unrounded


# ---- the retriever -----------------------------------------------------------------------------------------------------------------------------------
def test_retrieve_percentiles(tiny_retriever):
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
    queries = make_texts(4, 9)
    q_emb = r.process_query(queries, 0, r.encoder_q.config.topk)
    sc = _np(idx.explain(q_emb, torch.arange(n).repeat(4, 1), topn=0).scores).astype(np.float32)
    thr = np.array([np.unique(sc[b])[np.unique(sc[b]).size // 2] for b in range(4)], dtype=np.float32)
    match = sc >= thr[:, None]                                                         # the reference's match set
    pcts = [0, 10, 50, 90, 100]
    res = r.retrieve_percentiles(queries, "year", pcts, thr)
    assert isinstance(res, ValuePercentiles) and _np(res.values).dtype == np.float64
    for b in range(4):
        x = years[match[b] & (years != ref.INT32_MIN)].astype(np.float64)
        assert int(_np(res.count)[b]) == x.size and int(_np(res.missing)[b]) == int((match[b] & (years == ref.INT32_MIN)).sum())
        _close_to_numpy(_np(res.values)[b], x, pcts)
        for method in METHODS:
            got = r.retrieve_percentiles(queries, "year", pcts, thr, method=method)
            assert _np(got.values).dtype == I32
            assert (_np(got.values)[b] == np.quantile(x, np.array(pcts) / 100.0, method=method).astype(I32)).all()
    assert _np(res.count).tolist() == [int(c - m) for c, m in zip(_np(r.retrieve_range(queries, thr, max_hits=0).counts).tolist(), _np(res.missing).tolist())]
