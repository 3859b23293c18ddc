"""CPU checks of the numeric fields: the numpy reference against plain loops, the order-key rule (+-0, +-inf, denormals, every
NaN pattern), the invariants, the shard rule, the plan rule (vs_value_plan is pure host arithmetic), the argument errors of the C ABI without a
GPU, the facade's host logic, and the host-side code (vsearch_amd/csrc/value_check.h: keys, bin search, plan, checks) run in a stand-alone
program under the host sanitizers.  No device is needed."""
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

import _value_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, I32 = np.float32, np.int32
DTYPES = [F32, I32]


def _all_same(got, want):
    return len(got) == len(want) and all(ref.same(g, w) for g, w in zip(got, want))


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bit0", [0, 5, 37])
@pytest.mark.parametrize("with_live", [False, True])
def test_reference_equals_the_loops(dtype, bit0, with_live):
    n, B = 150, 3
    v = ref.values_case(n, dtype, seed=bit0 + 1, frac_missing=0.15, frac_special=0.2, spread=20)
    masks = ref.masks_case(B, n, seed=bit0 + 2, density=0.9)
    words = ref.pack(masks, bit0, spare=1)
    aw = ref.pack((np.random.default_rng(3).random(n) < 0.8)[None, :], bit0, spare=1)[0] if with_live else None
    edges = ref.edges_case(3, dtype) if dtype == F32 else np.array([-5, 0, 3, 17], I32)
    for desc in (True, False):
        lp = ref.loops(words, bit0, n, v, edges=list(edges), k=40, descending=desc, id_offset=1000, and_words=aw)
        assert _all_same(ref.stats(words, words.shape[1], bit0, n, v, aw), lp["stats"])
        assert _all_same(ref.histogram(words, words.shape[1], bit0, n, v, edges, aw), lp["histogram"])
        assert _all_same(ref.topk(words, words.shape[1], bit0, n, v, 40, desc, 1000, aw), lp["topk"])
    lp = ref.loops(None, 0, n, v, edges=list(edges), k=n + 5)                                      # words = NULL: every row, padding behind the last
    assert _all_same(ref.stats(None, 0, 0, n, v), lp["stats"]) and _all_same(ref.topk(None, 0, 0, n, v, n + 5), lp["topk"])
    assert (lp["topk"][0][0, -5:] == -1).all() and ref.is_missing(lp["topk"][1][0, -5:]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_range_bitmaps_reference(dtype):
    n = 100
    v = ref.values_case(n, dtype, seed=7, frac_missing=0.2, frac_special=0.2, spread=10)
    t = v.dtype.type
    lo = np.array([-3, 2, 5, v[~ref.is_missing(v)][0]], dtype)
    hi = np.array([4, 2, 1, v[~ref.is_missing(v)][0]], dtype)
    m = ref.range_masks(v, lo, hi)
    for b in range(4):
        for r in range(n):
            has = not ref.is_missing(v[r:r + 1])[0]
            assert m[b, r] == (has and float(lo[b]) <= float(v[r]) <= float(hi[b]))
    assert not m[2].any() and m[3].any()                                                           # lo > hi: empty; lo == hi: the rows that hold it
    w = ref.range_bitmaps(v, lo, hi, bit0=37)
    assert w.shape == (4, (37 + n + 31) // 32) and (ref.unpack(w, 37, n) == m).all()
    assert (w[:, 0] == 0).all() and (ref.unpack(w, 0, 37) == 0).all()                               # bits below bit0 are 0
    assert not ref.range_masks(v, np.array([ref.sentinel(dtype)]), np.array([t(5)])).any()          # a missing bound matches nothing


# ---- the order keys ------------------------------------------------------------------------------------------------------------------------
def test_fp32_keys_order_as_the_floats_do():
    rng = np.random.default_rng(0)
    pats = rng.integers(0, 1 << 32, size=200_000, dtype=np.uint64).astype(np.uint32)
    v = np.concatenate([pats.view(F32), ref.F32_SPECIALS, np.array([np.nextafter(F32(0), F32(1)), -np.nextafter(F32(0), F32(1))], F32)])
    k = ref.key(v)
    nan = np.isnan(v)
    assert (k[nan] == 0).all() and (k[~nan] >= 0x007FFFFF).all()                                    # missing: key 0; no value has it
    assert ref.key(np.array([-np.inf], F32))[0] == 0x007FFFFF and ref.key(np.array([np.inf], F32))[0] == 0xFF800000
    assert ref.key(np.array([0.0], F32))[0] == ref.key(np.array([-0.0], F32))[0] == 0x80000000
    x, kx = v[~nan], k[~nan]
    order = np.argsort(kx, kind="stable")
    assert (np.diff(x[order].astype(np.float64)) >= 0).all()                                        # ascending keys = ascending floats
    a, b = x[:-1], x[1:]
    assert ((a < b) == (kx[:-1] < kx[1:])).all() and ((a == b) == (kx[:-1] == kx[1:])).all()
    # searchsorted(side="right") gives the same slot on keys as on values
    edges = np.unique(np.concatenate([rng.normal(size=50).astype(F32), np.array([-np.inf, 0.0, np.inf, 1e-45, -1e-45], F32)]))
    assert (np.searchsorted(ref.key(edges), kx, side="right") == np.searchsorted(edges, x, side="right")).all()


def test_every_nan_pattern_is_missing():
    payload = np.arange(1, 1 << 23, 997, dtype=np.uint32)
    for sign in (0, 0x80000000):
        pats = (np.uint32(0x7F800000 | sign) | payload).astype(np.uint32)
        assert np.isnan(pats.view(F32)).all() and (ref.key(pats.view(F32)) == 0).all()
    ends = np.array([0x7F800001, 0x7FFFFFFF, 0xFF800001, 0xFFFFFFFF], np.uint32)
    assert (ref.key(ends.view(F32)) == 0).all()


def test_int32_keys():
    v = np.concatenate([ref.I32_SPECIALS, np.random.default_rng(1).integers(-(1 << 31), 1 << 31, size=100_000).astype(I32)])
    k = ref.key(v)
    assert ((k == 0) == (v == ref.INT32_MIN)).all()
    assert ref.key(np.array([ref.INT32_MIN + 1], I32))[0] == 1 and ref.key(np.array([(1 << 31) - 1], I32))[0] == 0xFFFFFFFF
    assert ((v[:-1] < v[1:]) == (k[:-1] < k[1:])).all()
    edges = np.unique(v[:500][v[:500] != ref.INT32_MIN])
    assert (np.searchsorted(ref.key(edges), k, side="right") == np.searchsorted(edges, v, side="right"))[v != ref.INT32_MIN].all()


def test_shard_merge_keys_are_the_reference_keys():
    v = np.concatenate([ref.F32_SPECIALS, np.array([np.nan, -np.nan], F32), ref.values_case(500, F32, seed=3)])
    assert (di._value_keys(torch.from_numpy(v)).numpy() == ref.key(v).astype(np.int64)).all()
    w = np.concatenate([ref.I32_SPECIALS, np.array([ref.INT32_MIN], I32), ref.values_case(500, I32, seed=3)])
    assert (di._value_keys(torch.from_numpy(w)).numpy() == ref.key(w).astype(np.int64)).all()


# ---- invariants ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_invariants(dtype):
    n, B = 3000, 5
    v = ref.values_case(n, dtype, seed=11)
    masks = ref.masks_case(B, n, seed=12, density=0.8)
    words = ref.pack(masks, 33, spare=1)
    size = masks.sum(axis=1)
    count, missing, lo, hi, total = ref.stats(words, words.shape[1], 33, n, v)
    assert (count + missing == size).all() and (missing > 0).all()
    for E in (2, 3, 64, 1025):
        c, below, above, miss = ref.histogram(words, words.shape[1], 33, n, v, ref.edges_case(E, dtype))
        assert c.shape == (B, E - 1) and (c.sum(axis=1) + below + above + miss == size).all() and (miss == missing).all()
    ids, vals = ref.topk(words, words.shape[1], 33, n, v, 7)
    assert ref.same(vals[:, 0], hi) or (vals[:, 0] == hi).all()                                     # (+0.0 against a stored -0.0)
    ids, vals = ref.topk(words, words.shape[1], 33, n, v, 7, descending=False)
    assert (vals[:, 0] == lo).all()
    empty = ref.stats(ref.pack(np.zeros((1, n), bool)), 0, 0, n, v)
    assert empty[0][0] == 0 and ref.is_missing(empty[2])[0] and ref.is_missing(empty[3])[0] and empty[4][0] == 0
    if dtype == F32:
        assert ref.bits(empty[2])[0] == ref.NAN_BITS


def test_sums_are_exact_and_wrap():
    big = np.full(3, (1 << 31) - 1, I32)
    assert ref.stats(None, 0, 0, 3, big)[4][0] == 3 * ((1 << 31) - 1)                               # beyond 32 bits, beyond fp32's 24
    v = np.array([2.0 ** 20] * 3 + [3e38, np.inf], F32)                                             # clamped to 2^20: 2^44 each
    assert ref.stats(None, 0, 0, 5, v)[4][0] == 5 << 44
    assert ref.fx(np.array([0.5, -0.25, 2.0 ** -25, 3 * 2.0 ** -25, np.nan], F32)).tolist() == [1 << 23, -(1 << 22), 0, 2, 0]
    st = di.ValueStats(np.array([2, 0]), np.array([0, 1]), np.array([1.0, np.nan], F32), np.array([2.0, np.nan], F32), np.array([3 << 24, 0]))
    m = st.mean()
    assert m.dtype == np.float64 and m[0] == 1.5 and np.isnan(m[1])
    st = di.ValueStats(torch.tensor([4]), torch.tensor([0]), torch.tensor([1], dtype=torch.int32), torch.tensor([9], dtype=torch.int32), torch.tensor([18]))
    assert st.mean().dtype == torch.float64 and float(st.mean()[0]) == 4.5


# ---- the shard rule ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cut", [1, 31, 32, 33])
def test_shard_rule(dtype, cut):
    """every shard works on its slice of the values and its bit range [cut, n) of the bitmap; merged = the whole"""
    n, B, k = 300, 4, 50
    v = ref.values_case(n, dtype, seed=cut, frac_special=0.2, spread=15)
    if dtype == I32:
        v[[0, n - 1]] = ((1 << 24) + 1, (1 << 30) + 3)                                              # values fp32 cannot hold
    masks = ref.masks_case(B, n, seed=cut + 1, density=0.9)
    words = ref.pack(masks)
    ld = words.shape[1]
    parts = [(0, cut), (cut, n)]
    whole = ref.stats(words, ld, 0, n, v)
    assert _all_same(ref.merge_stats([ref.stats(words, ld, r0, r1 - r0, v[r0:r1]) for r0, r1 in parts]), whole)
    edges = ref.edges_case(9, dtype, spread=15)
    whole = ref.histogram(words, ld, 0, n, v, edges)
    assert _all_same(ref.merge_histogram([ref.histogram(words, ld, r0, r1 - r0, v[r0:r1], edges) for r0, r1 in parts]), whole)
    for desc in (True, False):
        whole = ref.topk(words, ld, 0, n, v, k, desc)
        got = ref.merge_topk([ref.topk(words, ld, r0, r1 - r0, v[r0:r1], k, desc, id_offset=r0) for r0, r1 in parts], k, desc)
        assert _all_same(got, whole)
    lo, hi = np.array([-2, 0], dtype), np.array([3, 0], dtype)
    whole = ref.range_bitmaps(v, lo, hi)
    got = np.zeros_like(whole)
    for r0, r1 in parts:
        part = ref.range_bitmaps(v[r0:r1], lo, hi, bit0=r0 & 31)                                   # lands at its bit offset
        got[:, r0 >> 5:(r0 >> 5) + part.shape[1]] |= part
    assert (got == whole).all()


# ---- the plan rule ---------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_constants():
    text = open(os.path.join(REPO, "include", "vsearch_hip.h")).read()
    get = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert get("VS_VAL_F32") == nat.VAL_F32 == 0 and get("VS_VAL_I32") == nat.VAL_I32 == 1
    assert get("VS_VALUE_MAX_RANGES") == nat.VALUE_MAX_RANGES == ref.MAX_RANGES == di.MAX_VALUE_RANGES == 4096
    assert get("VS_VALUE_MAX_EDGES") == nat.VALUE_MAX_EDGES == ref.MAX_EDGES == di.MAX_VALUE_EDGES == 1025
    assert get("VS_VALUE_MAX_TOPK") == nat.VALUE_MAX_TOPK == ref.MAX_TOPK == di.MAX_VALUE_TOPK == 1024
    assert (8 * (1025 + 2) + 1025) * 4 <= 64 * 1024                                                # 8 histograms and the edges fit 64 KiB of LDS
    for name in ("vs_value_range_bitmaps", "vs_value_plan", "vs_value_stats", "vs_index_value_stats", "vs_value_histogram",
                 "vs_index_value_histogram", "vs_value_topk", "vs_index_value_topk"):
        assert name in nat.EXPORTED_SYMBOLS and ("VS_API int %s(" % name) in text


def _plan_rule(n_rows, B, n_bins, per_query, rpc):
    qt = 8 if per_query else 1
    tiles = -(-B // qt)
    if rpc == 0:
        want = max(1, 1024 // tiles)
        rpc = max(-(-n_rows // want), 8192, 16 * n_bins)
        rpc = -(-rpc // 2048) * 2048
    return qt, -(-n_rows // rpc), rpc


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 2049, 10_000, 1_000_000, 21_015_324, (1 << 32) - 1])
@pytest.mark.parametrize("B,per_query", [(1, False), (1, True), (8, True), (9, True), (17, True), (4096, True)])
def test_plan_against_its_rule(n_rows, B, per_query):
    for n_bins in (0, 4, 1027):
        for rpc_in in (0, 64, 2048, 1 << 20):
            got = di.value_plan(n_rows, B, n_bins, per_query, rpc_in)
            assert got == _plan_rule(n_rows, B, n_bins, per_query, rpc_in)
            qt, chunks, rpc = got
            assert rpc % 64 == 0 and chunks * rpc >= n_rows > (chunks - 1) * rpc
            if rpc_in:
                assert rpc == rpc_in                                                               # an explicit value is taken as given


def test_plan_argument_errors():
    for args in [(0, 1, 0, True, 0), (1 << 32, 1, 0, True, 0), (100, 0, 0, True, 0), (100, 1, -1, True, 0), (100, 1, 1028, True, 0),
                 (100, 1, 0, True, 100), (100, 1, 0, True, -64), (100, 2, 0, False, 0), (100, 8 * 65536, 0, True, 0)]:
        with pytest.raises(ValueError):
            di.value_plan(*args)
    with pytest.raises(ValueError, match="multiple of 64"):
        di.value_plan(100, 1, 0, True, 100)
    o32, o64 = C.c_int32(0), C.c_int64(0)
    assert nat.lib().vs_value_plan(100, 1, 4, 1, 0, None, C.byref(o64), C.byref(o64)) == nat.VS_EINVAL
    assert nat.lib().vs_value_plan(100, 1, 4, 1, 0, C.byref(o32), C.byref(o64), C.byref(o64)) == nat.VS_OK


# ---- argument errors of the C ABI, checked before the device is touched ----------------------------------------------------------------------
def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def test_index_calls_refuse_a_null_handle_without_a_device():
    v, o64, o32, ids = np.zeros(64, F32), np.zeros(4, np.int64), np.zeros(4, F32), np.zeros((1, 4), np.int64)
    e = np.array([0, 1], F32)
    L = nat.lib()
    assert L.vs_index_value_stats(None, None, 0, 0, 1, _p(v), 0, 0, _p(o64), _p(o64), _p(o32), _p(o32), _p(o64), None) == nat.VS_EINVAL
    assert "NULL" in nat.last_error()
    assert L.vs_index_value_histogram(None, None, 0, 0, 1, _p(v), 0, _p(e), 2, 0, _p(o64), 1, _p(o64), _p(o64), _p(o64), None) == nat.VS_EINVAL
    assert "NULL" in nat.last_error()
    assert L.vs_index_value_topk(None, None, 0, 0, 1, _p(v), 0, 4, 1, 0, 0, _p(ids), _p(o32), None) == nat.VS_EINVAL and "NULL" in nat.last_error()


def test_argument_errors_without_a_device(have_gpu):
    good = nat.VS_OK if have_gpu else nat.VS_ENODEVICE
    n = 100
    L = nat.lib()
    vals = {0: ref.values_case(n, F32, 1), 1: ref.values_case(n, I32, 1)}
    words = np.full((3, 5), -1, np.int32)
    out = lambda B=3, w=4: dict(count=np.zeros(B, np.int64), missing=np.zeros(B, np.int64), lo=np.zeros(B, F32), hi=np.zeros(B, F32),
                                sum=np.zeros(B, np.int64), counts=np.zeros((B, w), np.int64), ids=np.zeros((B, 1024), np.int64),
                                vals=np.zeros((B, 1024), F32))

    def stats(dt=0, B=3, bit0=0, ld=5, rpc=0, w=words, n_rows=n, null=()):
        o = {k: (None if k in null else a) for k, a in out(max(B, 1)).items()}
        return L.vs_value_stats(_p(w), bit0, ld, None, B, None if "values" in null else _p(vals[dt & 1]), dt, n_rows, rpc, _p(o["count"]),
                                _p(o["missing"]), _p(o["lo"]), _p(o["hi"]), _p(o["sum"]), 0, None)
    assert stats() == good and stats(dt=1) == good and stats(bit0=33) == good and stats(w=None, B=1, ld=0) == good and stats(rpc=64) == good
    assert stats(dt=2) == nat.VS_EINVAL and "dtype" in nat.last_error()
    assert stats(B=0) == nat.VS_EINVAL
    assert stats(bit0=-1) == nat.VS_EINVAL and "bit0" in nat.last_error()
    assert stats(bit0=64) == nat.VS_EINVAL and "ld_words" in nat.last_error()                       # 164 bits: 6 words
    assert stats(ld=0) == nat.VS_EINVAL and "B = 1" in nat.last_error()                             # a shared bitmap takes B = 1
    assert stats(w=None, ld=0) == nat.VS_EINVAL
    assert stats(rpc=100) == nat.VS_EINVAL and "multiple of 64" in nat.last_error()
    assert stats(n_rows=0) == nat.VS_EINVAL and stats(n_rows=1 << 32) == nat.VS_EINVAL
    for k in ("values", "count", "missing", "lo", "hi", "sum"):
        assert stats(null=(k,)) == nat.VS_EINVAL and "NULL" in nat.last_error()

    def hist(dt=0, edges=(0.0, 1.0, 2.0), ldc=4, B=3, ld=5, null=(), n_edges=None):
        o = {k: (None if k in null else a) for k, a in out(B).items()}
        e = np.asarray(edges, dtype=F32 if dt == 0 else I32)
        return L.vs_value_histogram(_p(words), 0, ld, None, B, _p(vals[dt]), dt, n, None if "edges" in null else _p(e),
                                    len(e) if n_edges is None else n_edges, 0, _p(o["counts"]), ldc, _p(o["count"]), _p(o["missing"]), _p(o["sum"]), 0, None)
    assert hist() == good and hist(dt=1, edges=(-5, 0, 7)) == good and hist(edges=(-np.inf, np.inf)) == good
    assert hist(edges=(0.0,)) == nat.VS_EINVAL and "n_edges" in nat.last_error()
    assert hist(edges=np.arange(1026)) == nat.VS_EINVAL and "n_edges" in nat.last_error()
    assert hist(ldc=1) == nat.VS_EINVAL and "ld_counts" in nat.last_error()
    assert hist(edges=(0.0, 0.0, 1.0)) == nat.VS_EINVAL and "ascending" in nat.last_error()
    assert hist(edges=(-0.0, 0.0)) == nat.VS_EINVAL and "ascending" in nat.last_error()             # one key
    assert hist(edges=(1.0, 0.5)) == nat.VS_EINVAL
    assert hist(edges=(0.0, np.nan)) == nat.VS_EINVAL and "missing" in nat.last_error()
    assert hist(dt=1, edges=(ref.INT32_MIN, 0)) == nat.VS_EINVAL and "missing" in nat.last_error()
    assert hist(dt=1, edges=(3, 3)) == nat.VS_EINVAL
    for k in ("edges", "counts", "count", "missing", "sum"):
        assert hist(null=(k,)) == nat.VS_EINVAL and "NULL" in nat.last_error()

    def topk(k=10, dt=0, B=3, rpc=0, null=(), n_rows=n):
        o = {kk: (None if kk in null else a) for kk, a in out(B).items()}
        return L.vs_value_topk(_p(words), 0, 5, None, B, _p(vals[dt]), dt, n_rows, k, 1, 7, rpc, _p(o["ids"]), _p(o["vals"]), 0, None)
    assert topk() == good and topk(k=1024) == good and topk(k=1, dt=1) == good
    assert topk(k=0) == nat.VS_EINVAL and topk(k=1025) == nat.VS_EINVAL and "1024" in nat.last_error()
    assert topk(rpc=32) == nat.VS_EINVAL
    for k in ("ids", "vals"):
        assert topk(null=(k,)) == nat.VS_EINVAL and "NULL" in nat.last_error()

    def ranges(lo=(0.0, 1.0), hi=(1.0, 0.0), dt=0, bit0=0, ld=4, B=None, null=(), n_rows=n):
        t = F32 if dt == 0 else I32
        l, h = np.asarray(lo, t), np.asarray(hi, t)
        B = len(l) if B is None else B
        w = np.zeros((max(B, 1), max(ld, 1)), np.int32)
        return L.vs_value_range_bitmaps(None if "values" in null else _p(vals[dt & 1]), dt, n_rows, None if "lo" in null else _p(l),
                                        None if "hi" in null else _p(h), B, bit0, None if "out" in null else _p(w), ld, 0, None)
    assert ranges() == good and ranges(lo=(-np.inf,), hi=(np.inf,)) == good and ranges(dt=1, lo=(ref.INT32_MIN + 1,), hi=((1 << 31) - 1,)) == good
    assert ranges(bit0=33, ld=5) == good
    assert ranges(lo=(np.nan,), hi=(1.0,)) == nat.VS_EINVAL and "missing bound" in nat.last_error()
    assert ranges(dt=1, lo=(0,), hi=(ref.INT32_MIN,)) == nat.VS_EINVAL and "missing bound" in nat.last_error()
    assert ranges(B=0) == nat.VS_EINVAL and ranges(lo=np.zeros(4097), hi=np.zeros(4097)) == nat.VS_EINVAL and "4096" in nat.last_error()
    assert ranges(ld=3) == nat.VS_EINVAL and "ld_words" in nat.last_error()
    assert ranges(bit0=-1) == nat.VS_EINVAL and ranges(dt=5) == nat.VS_EINVAL and ranges(n_rows=0) == nat.VS_EINVAL
    for k in ("values", "lo", "hi", "out"):
        assert ranges(null=(k,)) == nat.VS_EINVAL and "NULL" in nat.last_error()


# ---- the facade's host logic -----------------------------------------------------------------------------------------------------------------
def test_value_column():
    c = di.value_column([1990, 2000, -5])
    assert c.dtype == I32 and c.tolist() == [1990, 2000, -5]
    assert di.value_column(np.array([1, 2], np.uint8)).dtype == I32 and di.value_column(torch.tensor([1.5, float("nan")])).dtype == F32
    c = di.value_column(np.array([1.5, 2.5, 3.5]), missing=np.array([False, True, False]))
    assert c.dtype == F32 and np.isnan(c[1]) and c[0] == 1.5
    c = di.value_column(np.array([7, 8], np.int64), missing=[True, False])
    assert c.tolist() == [ref.INT32_MIN, 8]
    assert di.value_column([(1 << 31) - 1, ref.INT32_MIN + 1]).tolist() == [(1 << 31) - 1, ref.INT32_MIN + 1]
    for bad in ([1 << 31], [ref.INT32_MIN], [-(1 << 40)]):
        with pytest.raises(ValueError, match="integer field"):
            di.value_column(bad)
    for bad in (["a"], [True, False], np.zeros((2, 2))):
        with pytest.raises((TypeError, ValueError)):
            di.value_column(bad)
    with pytest.raises(ValueError, match="missing"):
        di.value_column([1, 2], missing=[True])
    with pytest.raises(ValueError, match="missing"):
        di.value_column([1, 2], missing=[1, 0])


def test_bounds_edges_and_k():
    l, h, scalar = di._value_bounds(None, None, nat.VAL_F32)
    assert scalar and l.dtype == F32 and l[0] == -np.inf and h[0] == np.inf
    l, h, scalar = di._value_bounds(1990, None, nat.VAL_I32)
    assert scalar and l.dtype == I32 and l.tolist() == [1990] and h.tolist() == [(1 << 31) - 1]
    l, h, scalar = di._value_bounds([1, None, 3], 5, nat.VAL_I32)
    assert not scalar and l.tolist() == [1, ref.INT32_MIN + 1, 3] and h.tolist() == [5, 5, 5]
    l, h, _ = di._value_bounds(1.5, 2.5, nat.VAL_I32)                                               # over integers: rounded inwards
    assert (l[0], h[0]) == (2, 2)
    l, h, _ = di._value_bounds(-np.inf, np.inf, nat.VAL_I32)
    assert (l[0], h[0]) == (ref.INT32_MIN + 1, (1 << 31) - 1)
    for bad in ((np.nan, 1.0, nat.VAL_F32), (1 << 31, None, nat.VAL_I32), (None, ref.INT32_MIN, nat.VAL_I32), ([1, 2], [1, 2, 3], nat.VAL_I32),
                (np.zeros(4097), None, nat.VAL_F32)):
        with pytest.raises(ValueError):
            di._value_bounds(*bad)
    with pytest.raises(TypeError):
        di._value_bounds("a", None, nat.VAL_F32)
    assert di._value_edges([1990, 2000, 2010], nat.VAL_I32).dtype == I32 and di._value_edges([0, 0.5], nat.VAL_F32).dtype == F32
    for bad in ([1], list(range(1026)), [0, 0], [1, 0], [0.0, -0.0], [0, np.nan]):
        with pytest.raises(ValueError):
            di._value_edges(bad, nat.VAL_F32)
    for bad in ([0.5, 1], [ref.INT32_MIN, 0], [0, 1 << 31]):
        with pytest.raises(ValueError):
            di._value_edges(bad, nat.VAL_I32)
    with pytest.raises(ValueError, match="ascending"):
        di._value_edges([1.0, 1.0 + 1e-9], nat.VAL_F32)                                            # one float32
    assert di._value_topk_args(np.int64(5), False) == (5, 0) and di._value_topk_args(1024) == (1024, 1)
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            di._value_topk_args(bad)
    for bad in (2.0, True, "3"):
        with pytest.raises(TypeError):
            di._value_topk_args(bad)
    v = np.zeros(10, F32)
    assert di._value_args(v, 10, 128) == (nat.VAL_F32, 128) and di._value_args(torch.zeros(10, dtype=torch.int32), 10) == (nat.VAL_I32, 0)
    with pytest.raises(ValueError, match="one entry per row"):
        di._value_args(v, 11)
    with pytest.raises(ValueError, match="multiple of 64"):
        di._value_args(v, 10, 100)
    with pytest.raises(TypeError, match="float32 or int32"):
        di._value_args(np.zeros(10, np.float64), 10)


class _HostIndex:
    """the host side of an Index with 4 documents: what set_values / add(values=) check before any device work"""

    def __new__(cls):
        from vsearch_amd.ir import SparseIndex
        idx = SparseIndex()
        idx._n_rows = lambda: 4
        return idx


def test_index_facade_host_checks():
    idx = _HostIndex()
    idx._facets = {"topic": (torch.zeros(4, dtype=torch.int32), 1, None)}
    with pytest.raises(ValueError, match="groups"):
        idx.set_values("groups", [1, 2, 3, 4])
    with pytest.raises(ValueError, match="facet field"):
        idx.set_values("topic", [1, 2, 3, 4])
    with pytest.raises(TypeError):
        idx.set_values("", [1, 2, 3, 4])
    with pytest.raises(ValueError, match="integer field"):
        idx.set_values("year", [1, 2, 3, 1 << 31])
    with pytest.raises(ValueError, match="4 documents"):
        idx.set_values("year", [1, 2, 3])
    idx._facets = {}
    assert idx.value_fields == []
    idx.set_values("year", None)                                                                    # removing a field that is not there
    with pytest.raises(KeyError, match="no value field"):
        idx.value_filter("year", 1990, 2000)
    with pytest.raises(KeyError):
        idx.top_by_value("year", 3)
    # add(values=) fails before anything changes
    with pytest.raises(ValueError, match="no value fields"):
        idx._added_values({"year": [1]}, 1)
    assert idx._added_values(None, 1) is None
    idx._values = {"year": torch.tensor([1990, 2000, 2010, ref.INT32_MIN], dtype=torch.int32), "price": torch.zeros(4)}
    assert idx.value_fields == ["year", "price"]
    for bad in (None, {"year": [1]}, {"year": [1], "price": [1.0], "extra": [2]}):
        with pytest.raises(ValueError, match="exactly these"):
            idx._added_values(bad, 1)
    with pytest.raises(ValueError, match="2 added"):
        idx._added_values({"year": [1], "price": [1.0]}, 2)
    with pytest.raises(TypeError, match="integers"):
        idx._added_values({"year": [1.5], "price": [1.0]}, 1)
    with pytest.raises(ValueError, match="integer field"):
        idx._added_values({"year": [1 << 31], "price": [1.0]}, 1)
    got = idx._added_values({"year": [2020], "price": [3]}, 1)                                      # an int into a float field converts
    assert got["year"].dtype == I32 and got["price"].dtype == F32 and got["price"][0] == 3.0
    with pytest.raises(ValueError, match="value fields"):                                           # update() checks before it deletes
        idx.update([0], torch.zeros(1, 4))
    with pytest.raises(ValueError, match="go together"):
        idx.value_stats("year", q_embs=torch.zeros(1, 6))
    with pytest.raises(ValueError, match="go together"):
        idx.histogram("year", [0, 1], min_score=0.5)
    with pytest.raises(ValueError):
        idx.histogram("year", [1, 0])
    with pytest.raises(ValueError):
        idx.top_by_value("year", 0)


# ---- the host-side code under the host sanitizers --------------------------------------------------------------------------------------------
def test_host_checks_under_a_host_sanitizer(tmp_path):
    """value_check.h (the order keys over two million bit patterns, the bin search against a linear scan on exact-size heap arrays, the plan rule
    and every limit of the calls) in a stand-alone program built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "value_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "value_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "value_check: ok" in run.stdout, run.stdout + run.stderr
