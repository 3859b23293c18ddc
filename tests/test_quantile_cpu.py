"""CPU checks of the percentiles: the radix composition of tests/_quantile_ref.py against the sort, the rank rule against
numpy, the facade's linear formula, the shard rule (summed level counts), the plan rule (vs_value_quantile_plan is pure host arithmetic), the
argument errors of the C ABI without a GPU, the facade's host logic, and the host-only code (vsearch_amd/csrc/quantile_check.h) run in a
stand-alone program under the host sanitizers.  No device is needed; nothing is loaded into Python under a sanitizer."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd import device_index as di

import _quantile_ref as qref
import _value_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, I32 = np.float32, np.int32
DTYPES = [F32, I32]
QS = [0.0, 0.1, 0.25, 0.5, 0.75, 0.99, 1.0]


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert ref.same(np.asarray(g), np.asarray(w)), i


# ---- the radix composition equals the sort ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bit0", [0, 5, 37])
def test_radix_select_equals_the_sort(dtype, bit0):
    n, B = 400, 3
    v = ref.values_case(n, dtype, seed=bit0 + 1, frac_missing=0.15, frac_special=0.2, spread=40)
    masks = ref.masks_case(B, n, seed=bit0 + 2, density=0.9)
    words = ref.pack(masks, bit0, spare=1)
    aw = ref.pack((np.random.default_rng(3).random(n) < 0.8)[None, :], bit0, spare=1)[0]
    ld = words.shape[1]
    for a in (None, aw):
        for method in ("lower", "higher", "nearest"):
            want = qref.order_statistics(words, ld, bit0, n, v, q=QS, method=method, and_words=a)
            _same(qref.radix_select(words, ld, bit0, n, v, q=QS, method=method, and_words=a), want)
            assert (want[2] + want[3] == (masks & (ref.unpack(a[None, :], bit0, n) if a is not None else True)).sum(axis=1)).all()
        ranks = np.array([[0, 1, 5, 10 ** 6], [3, 3, 2, 0], [0, 0, 0, 0]], np.int64)
        want = qref.order_statistics(words, ld, bit0, n, v, ranks=ranks, and_words=a)
        _same(qref.radix_select(words, ld, bit0, n, v, ranks=ranks, and_words=a), want)
        assert want[1][0, 3] == -1 and ref.is_missing(want[0][0, 3:4])[0]                           # a rank at or past the count
    # the plain-loop counts give the same composition
    _same(qref.radix_select(words, ld, bit0, 150, v[:150], q=QS, counts_fn=qref.level_counts_loops),
          qref.order_statistics(words, ld, bit0, 150, v[:150], q=QS))
    _same(qref.radix_select(None, 0, 0, n, v, q=QS), qref.order_statistics(None, 0, 0, n, v, q=QS))  # words = NULL: every row


def test_special_values():
    inf = np.inf
    den = np.nextafter(F32(0), F32(1))
    v = np.array([0.0, -0.0, inf, -inf, den, -den, 1.0, np.nan, -np.nan, 3.4028235e38], F32)
    nan_pats = np.array([0x7F800001, 0x7FFFFFFF, 0xFF800001, 0xFFFFFFFF, 0x7FC00000], np.uint32).view(F32)      # every kind of NaN: missing
    v = np.concatenate([v, nan_pats])
    n = v.shape[0]
    ranks = np.arange(n, dtype=np.int64)[None, :][:, :16]
    want = qref.order_statistics(None, 0, 0, n, v, ranks=ranks)
    _same(qref.radix_select(None, 0, 0, n, v, ranks=ranks), want)
    assert want[2][0] == 8 and want[3][0] == 7
    got = want[0][0, :8]
    assert got.tolist() == [-inf, -1.0 * 0 - float(den), 0.0, 0.0, float(den), 1.0, float(F32(3.4028235e38)), inf]
    assert ref.bits(got[2:4]).tolist() == [0, 0]                                                    # of -0.0 / +0.0 the answer is +0.0
    assert (ref.bits(want[0][0, 8:]) == ref.NAN_BITS).all() and (want[1][0, 8:] == -1).all()
    # keys 1 and 0xFFFFFFFF, and an all-equal field
    w = np.array([ref.INT32_MIN + 1, (1 << 31) - 1, ref.INT32_MIN, 0, (1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 3], I32)
    assert ref.key(w)[:2].tolist() == [1, 0xFFFFFFFF]
    ranks = np.arange(7, dtype=np.int64)[None, :]
    want = qref.order_statistics(None, 0, 0, 7, w, ranks=ranks)
    _same(qref.radix_select(None, 0, 0, 7, w, ranks=ranks), want)
    assert want[0][0].tolist() == [ref.INT32_MIN + 1, 0, (1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 3, (1 << 31) - 1, ref.INT32_MIN]
    for dtype in DTYPES:
        same = np.full(300, 7, dtype)
        trace = []
        got = qref.radix_select(None, 0, 0, 300, same, q=QS, trace=trace)
        _same(got, qref.order_statistics(None, 0, 0, 300, same, q=QS))
        assert (got[0] == 7).all() and all(int(st["n_slots"][0]) == 1 for _, st in trace)           # seven ranks, one slot at every level
        gone = np.full(50, ref.sentinel(dtype), dtype)
        got = qref.radix_select(None, 0, 0, 50, gone, q=QS)
        assert got[2][0] == 0 and got[3][0] == 50 and ref.is_missing(got[0]).all() and (got[1] == -1).all()


def test_slots_are_deduplicated_and_sorted():
    keys = np.array([(5 << 21) | (3 << 10) | 1, (5 << 21) | (3 << 10) | 2, (5 << 21) | (9 << 10), (700 << 21) | 4, (700 << 21) | 4], np.uint32)
    v = qref.unkey(keys, I32)
    trace = []
    ranks = np.array([[4, 0, 1, 2, 3, 1]], np.int64)
    got = qref.radix_select(None, 0, 0, 5, v, ranks=ranks, trace=trace)
    assert ref.key(got[0][0]).tolist() == [int(keys[i]) for i in (4, 0, 1, 2, 3, 1)]
    (c0, s0), (c1, s1), (c2, s2) = trace
    assert c0.shape == (1, 1, 2048) and c1.shape == (1, 6, 2048) and c2.shape == (1, 6, 1024)
    assert int(s0["n_slots"][0]) == 2 and s0["slot_prefix"][0, :2].tolist() == [5, 700] and (s0["slot_prefix"][0, 2:] == qref.NO_SLOT).all()
    assert s0["rank_slot"][0].tolist() == [1, 0, 0, 0, 1, 0] and s0["rank_res"][0].tolist() == [1, 0, 1, 2, 0, 1]
    assert int(s1["n_slots"][0]) == 3 and s1["slot_prefix"][0, :3].tolist() == [(5 << 11) | 3, (5 << 11) | 9, 700 << 11]
    assert int(s2["n_slots"][0]) == 4 and s2["rank_res"][0].tolist() == [1, 0, 0, 0, 0, 0]           # the second of two equal keys
    assert c1[0, 0].sum() == 3 and c1[0, 1].sum() == 2 and (c1[0, 2:] == 0).all()


# ---- the rank rule against numpy ---------------------------------------------------------------------------------------------------------------
def test_rank_rule_against_numpy():
    rng = np.random.default_rng(5)
    for case in range(4000):
        count = int(rng.integers(1, 400)) if case % 4 else int(rng.integers(1, 6))
        q = float(rng.random()) if case % 5 else float(rng.integers(0, 21)) / 20.0
        x = np.arange(count, dtype=np.float64)                                                       # sorted: the value IS the rank
        for method in ("lower", "higher", "nearest"):
            assert qref.rank_rule(q, count, method) == int(np.quantile(x, q, method=method)), (q, count, method)
    for m in ("lower", "higher", "nearest"):
        assert qref.rank_rule(0.5, 0, m) == -1 and qref.rank_rule(np.nan, 5, m) == -1 and qref.rank_rule(1.5, 5, m) == -1
        assert qref.rank_rule(0.0, (1 << 32) - 1, m) == 0 and qref.rank_rule(1.0, (1 << 32) - 1, m) == (1 << 32) - 2


def test_linear_formula_against_numpy():
    rng = np.random.default_rng(6)
    for case in range(300):
        n = int(rng.integers(1, 200))
        x = np.sort((rng.normal(size=n) * 10.0 ** rng.integers(-3, 6)).astype(F32)) if case % 2 else np.sort(rng.integers(-10 ** 6, 10 ** 6, size=n).astype(I32))
        q = np.concatenate([rng.random(5), [0.0, 0.5, 1.0]])
        pos = q * float(n - 1)
        lo, hi = x[np.floor(pos).astype(int)].astype(np.float64), x[np.ceil(pos).astype(int)].astype(np.float64)
        got = di.quantile_lerp(lo, hi, pos - np.floor(pos))
        assert got.dtype == np.float64 and (got.view(np.uint64) == qref.lerp(lo, hi, pos - np.floor(pos)).view(np.uint64)).all()      # pinned to the formula
        want = np.quantile(x.astype(np.float64), q, method="linear")
        bound = 4 * 2.0 ** -52 * np.maximum(np.abs(lo), np.abs(hi))
        assert (np.abs(got - want) <= bound).all(), (case, got, want)
    inf = np.array([np.inf, -np.inf, 1.0])
    assert di.quantile_lerp(inf, inf, np.array([0.5, 0.0, 0.3])).tolist() == [np.inf, -np.inf, 1.0]  # lo == hi: exactly lo, no NaN
    assert np.isnan(di.quantile_lerp(np.array([np.nan]), np.array([np.nan]), np.array([0.0])))[0]


# ---- the shard rule ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cuts", [[0, 437, 1000], [0, 437, 770, 1000], [0, 1, 1000], [0, 31, 64, 1000]])
def test_summed_level_counts_give_the_unsharded_answer(dtype, cuts):
    n, B = 1000, 4
    v = ref.values_case(n, dtype, seed=len(cuts), frac_special=0.1, spread=25)
    if dtype == I32:
        v[[0, n - 1]] = ((1 << 24) + 1, (1 << 30) + 3)
    masks = ref.masks_case(B, n, seed=7, density=0.9)
    words = ref.pack(masks)
    ld = words.shape[1]
    live = ref.pack((np.random.default_rng(8).random(n) < 0.9)[None, :])[0]
    for aw in (None, live):
        whole, parts = [], []
        want = qref.order_statistics(words, ld, 0, n, v, q=QS, method="nearest", and_words=aw)
        _same(qref.radix_select(words, ld, 0, n, v, q=QS, method="nearest", and_words=aw, trace=whole), want)
        _same(qref.radix_select(words, ld, 0, n, v, q=QS, method="nearest", and_words=aw, cuts=cuts, trace=parts), want)
        for (c0, s0), (c1, s1) in zip(whole, parts):
            assert (c0 == c1).all() and all((s0[k] == s1[k]).all() for k in s0)


# ---- the plan rule -------------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_constants():
    text = open(os.path.join(REPO, "include", "vsearch_hip.h")).read()
    get = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert get("VS_VALUE_RADIX_BINS") == nat.VALUE_RADIX_BINS == qref.BINS == 2048
    assert get("VS_VALUE_RADIX_LEVELS") == nat.VALUE_RADIX_LEVELS == qref.LEVELS == 3
    assert get("VS_VALUE_MAX_RANKS") == nat.VALUE_MAX_RANKS == qref.MAX_RANKS == di.MAX_VALUE_RANKS == 16
    assert get("VS_QUANTILE_LOWER") == nat.QUANTILE_LOWER == qref.LOWER == 0 and get("VS_QUANTILE_HIGHER") == nat.QUANTILE_HIGHER == qref.HIGHER == 1
    assert get("VS_QUANTILE_NEAREST") == nat.QUANTILE_NEAREST == qref.NEAREST == 2
    assert di.QUANTILE_METHODS == qref.METHODS and sum(b.bit_length() - 1 for b in qref.LEVEL_BINS) == 32
    for name in ("vs_value_quantile_plan", "vs_value_quantiles", "vs_index_value_quantiles", "vs_value_radix_counts", "vs_index_value_radix_counts",
                 "vs_value_radix_step"):
        assert name in nat.EXPORTED_SYMBOLS and ("VS_API int %s(" % name) in text
    assert "percentiles" not in text[text.index("Not covered: no index file stores values"):][:400]


def _plan_rule(n_rows, B, R, per_query, rpc):
    qt = 1 if not per_query else 8 if R <= 2 else 4 if R <= 4 else 2 if R <= 8 else 1
    tiles = -(-B // qt)
    if rpc == 0:
        rpc = max(-(-n_rows // max(1, 1024 // tiles)), 8192)
        rpc = -(-rpc // 2048) * 2048
    return qt, -(-n_rows // rpc), rpc


@pytest.mark.parametrize("n_rows", [1, 64, 2049, 1_000_000, 21_015_324, (1 << 32) - 1])
@pytest.mark.parametrize("B,per_query", [(1, False), (1, True), (8, True), (9, True), (17, True)])
def test_plan_against_its_rule(n_rows, B, per_query):
    for R in range(1, 17):
        for rpc_in in (0, 64, 2048):
            got = di.value_quantile_plan(n_rows, B, R, per_query, rpc_in)
            assert got == _plan_rule(n_rows, B, R, per_query, rpc_in)
            qt, chunks, rpc = got
            assert qt * R * 2048 * 4 <= 128 * 1024 and chunks * rpc >= n_rows > (chunks - 1) * rpc
            assert got[1:] == di.value_plan(n_rows, B, 0, per_query, rpc_in)[1:] or qt != 8           # the chunk rule is value_plan's


def test_plan_argument_errors():
    for args in [(0, 1, 1, True, 0), (100, 0, 1, True, 0), (100, 1, 0, True, 0), (100, 1, 17, True, 0), (100, 1, 1, True, 100), (100, 2, 1, False, 0)]:
        with pytest.raises(ValueError):
            di.value_quantile_plan(*args)
    o32, o64 = C.c_int32(0), C.c_int64(0)
    assert nat.lib().vs_value_quantile_plan(100, 1, 4, 1, 0, None, C.byref(o64), C.byref(o64)) == nat.VS_EINVAL


# ---- argument errors of the C ABI, checked before the device is touched ----------------------------------------------------------------------
def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def test_argument_errors_without_a_device(have_gpu):
    good = nat.VS_OK if have_gpu else nat.VS_ENODEVICE
    n, L = 100, nat.lib()
    vals = {0: ref.values_case(n, F32, 1), 1: ref.values_case(n, I32, 1)}
    words = np.full((3, 5), -1, np.int32)

    def quant(dt=0, B=3, R=3, bit0=0, ld=5, rpc=0, w=words, n_rows=n, q=(0.0, 0.5, 1.0), method=0, ranks=None, null=()):
        o = dict(vals=np.zeros((max(B, 1), 16), F32), ranks=np.zeros((max(B, 1), 16), np.int64), count=np.zeros(max(B, 1), np.int64),
                 missing=np.zeros(max(B, 1), np.int64))
        o = {k: (None if k in null else a) for k, a in o.items()}
        qa = None if q is None else np.asarray(q, np.float64)
        ra = None if ranks is None else np.asarray(ranks, np.int64)
        return L.vs_value_quantiles(_p(w), bit0, ld, None, B, None if "values" in null else _p(vals[dt & 1]), dt, n_rows, _p(qa), method, _p(ra), R, rpc,
                                    _p(o["vals"]), _p(o["ranks"]), _p(o["count"]), _p(o["missing"]), 0, None)
    assert quant() == good and quant(dt=1, method=2) == good and quant(bit0=33) == good and quant(w=None, B=1, ld=0) == good
    assert quant(q=None, ranks=np.zeros((3, 3))) == good and quant(R=16, q=np.linspace(0, 1, 16)) == good and quant(q=(-0.0, 1.0), R=2) == good
    assert quant(R=0) == nat.VS_EINVAL and "R must" in nat.last_error()
    assert quant(R=17) == nat.VS_EINVAL and "R must" in nat.last_error()
    assert quant(q=(0.0, 0.5, 1.5)) == nat.VS_EINVAL and "q[2]" in nat.last_error()
    assert quant(q=(0.0, np.nan, 1.0)) == nat.VS_EINVAL and "q[1]" in nat.last_error()
    assert quant(q=(-1e-9, 0.5, 1.0)) == nat.VS_EINVAL
    assert quant(method=3) == nat.VS_EINVAL and "method" in nat.last_error()
    assert quant(q=None, ranks=[[0, 1, 2], [0, -1, 2], [0, 1, 2]]) == nat.VS_EINVAL and "negative" in nat.last_error()
    assert quant(q=None) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert quant(dt=2) == nat.VS_EINVAL and "dtype" in nat.last_error()
    assert quant(B=0) == nat.VS_EINVAL and quant(bit0=-1) == nat.VS_EINVAL and quant(bit0=64) == nat.VS_EINVAL and "ld_words" in nat.last_error()
    assert quant(ld=0) == nat.VS_EINVAL and quant(rpc=100) == nat.VS_EINVAL and "multiple of 64" in nat.last_error()
    assert quant(n_rows=0) == nat.VS_EINVAL and quant(n_rows=1 << 32) == nat.VS_EINVAL
    for k in ("values", "vals", "ranks", "count", "missing"):
        assert quant(null=(k,)) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert L.vs_index_value_quantiles(None, None, 0, 0, 1, _p(vals[0]), 0, _p(np.zeros(1)), 0, None, 1, 0, _p(np.zeros(1, F32)), _p(np.zeros(1, np.int64)),
                                      _p(np.zeros(1, np.int64)), _p(np.zeros(1, np.int64)), None) == nat.VS_EINVAL and "NULL" in nat.last_error()

    def counts(level=0, R=3, B=3, dt=0, sp=True, ns=True, mis=True, cnt=True):
        c = np.zeros((B, R, 2048), np.int64)
        s, m, k = np.zeros((B, R), np.int32), np.zeros(B, np.int32), np.zeros(B, np.int64)
        return L.vs_value_radix_counts(_p(words), 0, 5, None, B, _p(vals[dt & 1]), dt, n, level, R, _p(s) if sp else None, _p(m) if ns else None, 0,
                                       _p(c) if cnt else None, _p(k) if mis else None, 0, None)
    assert counts() == good and counts(level=1, mis=False) == good and counts(level=2, dt=1) == good and counts(sp=False, ns=False) == good
    assert counts(level=3) == nat.VS_EINVAL and "level" in nat.last_error()
    assert counts(level=-1) == nat.VS_EINVAL
    assert counts(mis=False) == nat.VS_EINVAL and "missing" in nat.last_error()
    assert counts(level=1, sp=False) == nat.VS_EINVAL and counts(level=2, ns=False) == nat.VS_EINVAL and "slot_prefix" in nat.last_error()
    assert counts(cnt=False) == nat.VS_EINVAL and counts(R=17) == nat.VS_EINVAL and counts(dt=7) == nat.VS_EINVAL
    assert L.vs_index_value_radix_counts(None, None, 0, 0, 1, _p(vals[0]), 0, 0, 1, None, None, 0, _p(np.zeros(2048, np.int64)), _p(np.zeros(1, np.int64)),
                                         None) == nat.VS_EINVAL

    def step(level=0, R=3, B=2, method=0, dt=0, q=True, null=()):
        a = dict(counts=np.zeros((B, R, 2048), np.int64), q=np.zeros(R), res=np.zeros((B, R), np.int64), slot=np.zeros((B, R), np.int32),
                 pre=np.zeros((B, R), np.int32), sp=np.zeros((B, R), np.int32), ns=np.zeros(B, np.int32), count=np.zeros(B, np.int64),
                 ranks=np.zeros((B, R), np.int64), vals=np.zeros((B, R), F32))
        a = {k: (None if k in null else x) for k, x in a.items()}
        return L.vs_value_radix_step(level, _p(a["counts"]), B, R, _p(a["q"]) if q else None, method, None, _p(a["res"]), _p(a["slot"]), _p(a["pre"]),
                                     _p(a["sp"]), _p(a["ns"]), _p(a["count"]), _p(a["ranks"]), _p(a["vals"]), dt, 0, None)
    assert step(level=5) == nat.VS_EINVAL and step(R=0) == nat.VS_EINVAL and step(B=0) == nat.VS_EINVAL and step(dt=3) == nat.VS_EINVAL
    assert step(method=9) == nat.VS_EINVAL and "method" in nat.last_error()
    assert step(q=False) == nat.VS_EINVAL and step(null=("count",)) == nat.VS_EINVAL and step(level=2, null=("vals",)) == nat.VS_EINVAL
    for k in ("counts", "res", "slot", "pre", "sp", "ns"):
        assert step(null=(k,)) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert step() == (nat.VS_EINVAL if have_gpu else nat.VS_ENODEVICE)                               # host buffers: the step works on the device
    if have_gpu:
        assert "device buffers" in nat.last_error()


# ---- the facade's host logic -------------------------------------------------------------------------------------------------------------------
def test_quantile_and_percentile_args():
    q, m, r = di._quantile_args([0.0, 0.5], "nearest", None)
    assert q.dtype == np.float64 and q.tolist() == [0.0, 0.5] and m == nat.QUANTILE_NEAREST and r is None
    q, m, r = di._quantile_args(None, "lower", torch.tensor([[1, 2], [3, 4]]))
    assert q is None and r.dtype == np.int64 and r.shape == (2, 2)
    assert di._quantile_args(0.5, "higher", None)[0].tolist() == [0.5]
    assert di._quantile_ranks_for(np.array([1, 2], np.int64), 3).tolist() == [[1, 2]] * 3
    for bad in ((None, "lower", None), ([0.5], "lower", [1]), ([1.5], "lower", None), ([np.nan], "lower", None), ([0.5], "linear", None),
                (None, "lower", [-1]), ([], "lower", None)):
        with pytest.raises(ValueError):
            di._quantile_args(*bad)
    with pytest.raises(TypeError):
        di._quantile_args(None, "lower", [0.5])
    with pytest.raises(ValueError, match="3 queries"):
        di._quantile_ranks_for(np.zeros((2, 2), np.int64), 3)
    assert di._percentile_args([0, 50, 100], "linear").tolist() == [0.0, 0.5, 1.0] and di._percentile_args(25, "lower").tolist() == [0.25]
    for bad in ([101], [-1], [np.nan], []):
        with pytest.raises(ValueError):
            di._percentile_args(bad, "linear")
    with pytest.raises(ValueError, match="method"):
        di._percentile_args([50], "midpoint")
    with pytest.raises(TypeError):
        di._percentile_args(["a"], "linear")


def test_index_facade_host_checks():
    from vsearch_amd.ir import SparseIndex
    idx = SparseIndex()
    idx._n_rows = lambda: 4
    with pytest.raises(KeyError, match="no value field"):
        idx.percentiles("year", [50])
    idx._values = {"year": torch.tensor([1990, 2000, 2010, ref.INT32_MIN], dtype=torch.int32)}
    with pytest.raises(ValueError, match="go together"):
        idx.median("year", q_embs=torch.zeros(1, 6))
    with pytest.raises(ValueError, match="0..100"):
        idx.percentiles("year", [150])
    with pytest.raises(ValueError, match="method"):
        idx.percentiles("year", [50], method="midpoint")


# ---- the host-only code under the host sanitizers ------------------------------------------------------------------------------------------------
def test_host_checks_under_a_host_sanitizer(tmp_path):
    """quantile_check.h (the rank function at count = 0, 1, 2, 2^32 - 1 and q = 0, 1, the step's bin search against a linear scan on exact-size
    heap arrays, the slot search, the plan rule, every check, and a whole select against a sort) in a stand-alone program built with the host
    compiler under AddressSanitizer and UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "quantile_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "quantile_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "quantile_check: ok" in run.stdout, run.stdout + run.stderr
