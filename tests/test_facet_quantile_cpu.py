"""CPU checks of the per-label percentiles: the reference of tests/_facet_quantile_ref.py against numpy's sort and percentile
per label, the shard rule (summed level counts), the plan rule (vs_facet_value_quantile_plan is pure host arithmetic), the header's constants
against the bindings, the argument errors of the C ABI without a GPU, and the host-only code (vsearch_amd/csrc/facet_quantile_check.h) run in
a stand-alone program under the host sanitizers.  No device is needed; nothing is loaded into Python under a sanitizer."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from vsearch_amd import _native as nat
from vsearch_amd import device_index as di

import _facet_quantile_ref as fq
import _facet_value_ref as fref
import _value_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, I32 = np.float32, np.int32
QS = [0.0, 0.1, 0.5, 0.9, 1.0]


def _same(got, want, what=None):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert ref.same(np.asarray(g), np.asarray(w)), (what, i)


def _case(n, B, L, dtype, seed, kind="mixed"):
    v = ref.values_case(n, dtype, seed=seed, frac_missing=0.15, frac_special=0.1, spread=40)
    labels = fref.labels_shape(kind, n, L, seed + 1)
    masks = ref.masks_case(B, n, seed=seed + 2, density=0.85)
    return v, labels, masks


# ---- the reference against numpy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit0", [0, 5, 37])
def test_reference_against_numpy_per_label(bit0):
    n, B, L = 600, 3, 4
    v, labels, masks = _case(n, B, L, I32, seed=bit0)
    words = ref.pack(masks, bit0, spare=1)
    ld = words.shape[1]
    for method in ("lower", "higher", "nearest"):
        vals, rk, count, missing, total, other = fq.order_statistics(words, ld, bit0, n, v, labels, L, q=QS, method=method)
        for b in range(B):
            for l in range(L):
                rows = masks[b] & (labels == l)
                x = np.sort(v[rows & (v != ref.INT32_MIN)])
                assert count[b, l] == x.size and missing[b, l] == (rows & (v == ref.INT32_MIN)).sum()
                assert x.size > 0
                assert (vals[b, l] == np.percentile(x, np.array(QS) * 100, method=method).astype(I32)).all()
                assert (x[rk[b, l]] == vals[b, l]).all()
            assert total[b] == masks[b].sum() and other[b] == (masks[b] & ((labels < 0) | (labels >= L))).sum()
            assert count[b].sum() + missing[b].sum() + other[b] == total[b]
    assert (labels < 0).any() and (labels >= L).any()
    # explicit ranks, one at the count
    ranks = np.zeros((B, L, 2), np.int64)
    ranks[:, :, 1] = count
    vals, rk, *_ = fq.order_statistics(words, ld, bit0, n, v, labels, L, ranks=ranks)
    assert (rk[:, :, 0] == 0).all() and (rk[:, :, 1] == -1).all() and ref.is_missing(vals[:, :, 1]).all()


@pytest.mark.parametrize("dtype", [F32, I32])
def test_radix_composition_equals_the_sort(dtype):
    n, B, L = 300, 2, 3
    v, labels, masks = _case(n, B, L, dtype, seed=7)
    labels[labels == 1] = 0                                                            # label 1 has no rows
    v[labels == 2] = ref.sentinel(dtype)                                               # label 2 has no values
    words = ref.pack(masks, 5, spare=1)
    want = fq.order_statistics(words, words.shape[1], 5, n, v, labels, L, q=QS, method="nearest")
    _same(fq.radix_select(words, words.shape[1], 5, n, v, labels, L, q=QS, method="nearest"), want)
    assert want[2][:, 1].tolist() == [0, 0] and want[3][:, 1].tolist() == [0, 0] and (want[2][:, 2] == 0).all() and (want[3][:, 2] > 0).all()
    assert ref.is_missing(want[0][:, 1:]).all() and (want[1][:, 1:] == -1).all()


@pytest.mark.parametrize("cuts", [[0, 437, 1000], [0, 31, 64, 1000]])
def test_summed_level_counts_of_row_cuts_give_the_unsharded_answer(cuts):
    n, B, L = 1000, 2, 3
    for dtype in (F32, I32):
        v, labels, masks = _case(n, B, L, dtype, seed=cuts[1])
        words = ref.pack(masks)
        ld = words.shape[1]
        whole, parts = [], []
        want = fq.radix_select(words, ld, 0, n, v, labels, L, q=[0.0, 0.5, 1.0], trace=whole)
        _same(fq.radix_select(words, ld, 0, n, v, labels, L, q=[0.0, 0.5, 1.0], cuts=cuts, trace=parts), want, cuts)
        for (c0, _), (c1, _) in zip(whole, parts):
            assert (c0 == c1).all()
        _same(want, fq.order_statistics(words, ld, 0, n, v, labels, L, q=[0.0, 0.5, 1.0]))


# ---- the plan rule -------------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_constants():
    text = open(os.path.join(REPO, "include", "vsearch_hip.h")).read()
    get = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert get("VS_FACET_QUANTILE_MAX_LABEL_TILES") == nat.FACET_QUANTILE_MAX_LABEL_TILES
    assert get("VS_VALUE_MAX_RANKS") == nat.VALUE_MAX_RANKS == di.MAX_VALUE_RANKS and get("VS_VALUE_RADIX_BINS") == nat.VALUE_RADIX_BINS
    for name in ("vs_facet_value_quantile_plan", "vs_facet_value_quantiles", "vs_index_facet_value_quantiles", "vs_facet_value_radix_counts",
                 "vs_index_facet_value_radix_counts"):
        assert name in nat.EXPORTED_SYMBOLS and ("VS_API int %s(" % name) in text
    assert "facet_quantiles.hip" in open(os.path.join(REPO, "vsearch_amd", "csrc", "Makefile")).read()


def _cells(R, level):
    return 128 * 1024 // ((1 if level == 0 else R) * (1024 if level == 2 else 2048) * 4)


def _plan_rule(n_rows, B, L, R, level, per_query, rpc):
    """the rule as the header states it"""
    cap, best = _cells(R, level), None
    qt = 1
    while qt <= (8 if per_query else 1) and qt <= cap:
        tl = min(L, cap // qt)
        lt = -(-L // tl)
        passes = -(-B // qt) * lt
        if lt <= nat.FACET_QUANTILE_MAX_LABEL_TILES and (best is None or passes < best[0]):
            best = (passes, qt, tl, lt)
        qt *= 2
    regime, qt, tl, lt = (0,) + best[1:] if best else (1, 8 if per_query else 1, L, 1)
    if rpc == 0:
        want = max(1, 1024 // (-(-B // qt) * lt))
        rpc = -(-max(-(-n_rows // want), 8192) // 2048) * 2048
    return regime, qt, tl, lt, -(-n_rows // rpc), rpc


@pytest.mark.parametrize("n_rows", [1, 64, 2049, 1_000_000, 21_015_324, (1 << 32) - 1])
@pytest.mark.parametrize("B,per_query", [(1, False), (1, True), (8, True), (9, True)])
def test_plan_against_its_rule(n_rows, B, per_query):
    T = nat.FACET_QUANTILE_MAX_LABEL_TILES
    for level in range(3):
        for R in (1, 2, 3, 7, 8, 16):
            cap = _cells(R, level)
            Ls = {1, 2, cap, cap + 1, 2 * cap, 2 * cap + 1}
            for qt in (1, 2, 4, 8):                                                    # both sides of every tile and regime boundary
                tl = max(1, cap // qt)
                Ls |= {tl - 1, tl, tl + 1, tl * T - 1, tl * T, tl * T + 1}
            for L in sorted(x for x in Ls if x >= 1):
                for rpc_in in (0, 2048):
                    got = di.facet_value_quantile_plan(n_rows, B, L, R, level, per_query, rpc_in)
                    assert got == _plan_rule(n_rows, B, L, R, level, per_query, rpc_in), (L, R, level, rpc_in)
                    regime, qt, tl, lt, chunks, rpc = got
                    assert chunks * rpc >= n_rows > (chunks - 1) * rpc
                    if regime == 0:
                        assert qt * tl <= cap and tl * lt >= L > tl * (lt - 1) and lt <= T
                    else:
                        assert (qt, tl, lt) == (8 if per_query else 1, L, 1)
    # the regimes' boundary by name: a shared bitmap at level 0 holds 16 labels a tile
    assert di.facet_value_quantile_plan(1000, 1, 16 * T, 1, 0, False)[:4] == (0, 1, 16, T)
    assert di.facet_value_quantile_plan(1000, 1, 16 * T + 1, 1, 0, False)[:4] == (1, 1, 16 * T + 1, 1)


def test_plan_argument_errors():
    for args in [(0, 1, 4, 1, 0, True, 0), (1 << 32, 1, 4, 1, 0, True, 0), (100, 0, 4, 1, 0, True, 0), (100, 1, 0, 1, 0, True, 0),
                 (100, 1, 4, 0, 0, True, 0), (100, 1, 4, 17, 0, True, 0), (100, 1, 4, 1, 3, True, 0), (100, 1, 4, 1, -1, True, 0),
                 (100, 1, 4, 1, 0, True, 100), (100, 2, 4, 1, 0, False, 0), (100, 1 << 16, 1 << 15, 1, 0, True, 0)]:
        with pytest.raises(ValueError):
            di.facet_value_quantile_plan(*args)
    o32, o64 = C.c_int32(0), C.c_int64(0)
    p32, p64 = C.byref(o32), C.byref(o64)
    assert nat.lib().vs_facet_value_quantile_plan(100, 1, 4, 1, 0, 1, 0, None, p32, p32, p32, p64, p64) == nat.VS_EINVAL
    assert nat.lib().vs_facet_value_quantile_plan(100, 1, 4, 1, 0, 1, 0, p32, p32, p32, p32, p64, p64) == nat.VS_OK


# ---- argument errors of the C ABI, checked before the device is touched ----------------------------------------------------------------------
def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def test_index_calls_refuse_a_null_handle_without_a_device():
    v, lab, o64, o32, q = np.zeros(64, F32), np.zeros(64, I32), np.zeros(8, np.int64), np.zeros(8, F32), np.array([0.5])
    L = nat.lib()
    assert L.vs_index_facet_value_quantiles(None, None, 0, 0, 1, _p(lab), 2, _p(v), 0, _p(q), 0, None, 1, 0, _p(o32), _p(o64), _p(o64), _p(o64),
                                            _p(o64), _p(o64), None) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert L.vs_index_facet_value_radix_counts(None, None, 0, 0, 1, _p(lab), 2, _p(v), 0, 0, 1, None, None, 0, _p(np.zeros(4096, np.int64)), _p(o64),
                                               _p(o64), _p(o64), None) == nat.VS_EINVAL and "NULL" in nat.last_error()


def test_argument_errors_without_a_device(have_gpu):
    good = nat.VS_OK if have_gpu else nat.VS_ENODEVICE
    n, nl, R = 100, 3, 2
    L = nat.lib()
    vals = {0: ref.values_case(n, F32, 1), 1: ref.values_case(n, I32, 1)}
    labels = fref.labels_shape("mixed", n, nl, 2)
    words = np.full((3, 5), -1, np.int32)
    outs = ("vals", "rk", "count", "missing", "total", "other")

    def quant(dt=0, B=3, bit0=0, ld=5, rpc=0, w=words, n_rows=n, n_labels=nl, q=(0.25, 0.5), method=0, ranks=None, R=R, null=()):
        cells = 3 * max(n_labels, 1) if n_labels < 1000 else 3
        o = dict(vals=np.zeros((cells, 16), F32), rk=np.zeros((cells, 16), np.int64), count=np.zeros(cells, np.int64),
                 missing=np.zeros(cells, np.int64), total=np.zeros(3, np.int64), other=np.zeros(3, np.int64))
        o = {k: (None if k in null else a) for k, a in o.items()}
        qa = None if q is None else np.asarray(q, np.float64)
        ra = None if ranks is None else np.asarray(ranks, np.int64)
        return L.vs_facet_value_quantiles(_p(w), bit0, ld, None, B, None if "labels" in null else _p(labels), n_labels,
                                          None if "values" in null else _p(vals[dt & 1]), dt, n_rows, _p(qa), method, _p(ra), R, rpc,
                                          *[_p(o[k]) for k in outs], 0, None)
    assert quant() == good and quant(dt=1) == good and quant(bit0=33) == good and quant(w=None, B=1, ld=0) == good and quant(rpc=64) == good
    assert quant(q=None, ranks=np.zeros((3, nl, R))) == good and quant(method=2) == good
    assert quant(dt=2) == nat.VS_EINVAL and "dtype" in nat.last_error()
    assert quant(B=0) == nat.VS_EINVAL
    assert quant(bit0=-1) == nat.VS_EINVAL and "bit0" in nat.last_error()
    assert quant(bit0=64) == nat.VS_EINVAL and "ld_words" in nat.last_error()
    assert quant(ld=0) == nat.VS_EINVAL and "B = 1" in nat.last_error()
    assert quant(rpc=100) == nat.VS_EINVAL and "multiple of 64" in nat.last_error()
    assert quant(n_rows=0) == nat.VS_EINVAL and quant(n_labels=0) == nat.VS_EINVAL and "n_labels" in nat.last_error()
    assert quant(R=0) == nat.VS_EINVAL and "R must" in nat.last_error() and quant(R=17) == nat.VS_EINVAL and "R must" in nat.last_error()
    assert quant(n_labels=65536 // 3 // 16 + 1, R=16, null=outs) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert quant(n_labels=65536 // 3 // R + 1) == nat.VS_EINVAL and "2^27" in nat.last_error()      # B x L x R x 2048 > 2^27, seen before any array is
    assert quant(method=3) == nat.VS_EINVAL and "method" in nat.last_error()
    assert quant(q=(0.5, 1.5)) == nat.VS_EINVAL and "outside" in nat.last_error()
    assert quant(q=(np.nan, 0.5)) == nat.VS_EINVAL and "outside" in nat.last_error()
    assert quant(q=None) == nat.VS_EINVAL and "NULL" in nat.last_error()
    bad = np.zeros((3, nl, R), np.int64)
    bad[2, 1, 1] = -1
    assert quant(q=None, ranks=bad) == nat.VS_EINVAL and "negative" in nat.last_error()
    for k in ("labels", "values") + outs:
        assert quant(null=(k,)) == nat.VS_EINVAL and "NULL" in nat.last_error()

    def level(lv=0, dt=0, B=3, ld=5, n_labels=nl, R=R, null=(), rpc=0):
        bins = 1024 if lv == 2 else 2048
        o = dict(counts=np.zeros((3, nl, R, bins), np.int64), missing=np.zeros((3, nl), np.int64), total=np.zeros(3, np.int64),
                 other=np.zeros(3, np.int64), sp=np.full((3 * nl, R), -1, np.int32), ns=np.zeros(3 * nl, np.int32))
        o = {k: (None if k in null else a) for k, a in o.items()}
        return L.vs_facet_value_radix_counts(_p(words), 0, ld, None, B, _p(labels), n_labels, _p(vals[dt]), dt, n, lv, R, _p(o["sp"]), _p(o["ns"]), rpc,
                                             _p(o["counts"]), _p(o["missing"]), _p(o["total"]), _p(o["other"]), 0, None)
    assert level() == good and level(1) == good and level(2, dt=1) == good
    assert level(0, null=("sp", "ns")) == good and level(1, null=("missing", "total", "other")) == good
    assert level(3) == nat.VS_EINVAL and "level" in nat.last_error() and level(-1) == nat.VS_EINVAL
    assert level(null=("counts",)) == nat.VS_EINVAL and "NULL" in nat.last_error()
    for k in ("missing", "total", "other"):
        assert level(0, null=(k,)) == nat.VS_EINVAL and "level 0 needs" in nat.last_error()
    for k in ("sp", "ns"):
        assert level(2, null=(k,)) == nat.VS_EINVAL and "slot_prefix" in nat.last_error()
    assert level(R=17) == nat.VS_EINVAL and level(n_labels=0) == nat.VS_EINVAL and level(rpc=100) == nat.VS_EINVAL


# ---- the facade's host logic -----------------------------------------------------------------------------------------------------------------
def test_python_argument_checks():
    q, m, r = di._facet_quantile_args([0.5], "nearest", None, 4)
    assert q.tolist() == [0.5] and m == nat.QUANTILE_NEAREST and r is None
    _, _, r = di._facet_quantile_args(None, "lower", np.zeros((2, 4, 3), np.int32), 4)
    assert r.shape == (2, 4, 3) and r.dtype == np.int64
    assert di._facet_quantile_args(None, "lower", [0, 5], 4)[2].tolist() == [0, 5]
    with pytest.raises(ValueError, match="labels"):
        di._facet_quantile_args(None, "lower", np.zeros((2, 5, 3), np.int64), 4)
    with pytest.raises(ValueError):
        di._facet_quantile_args(None, "lower", np.zeros((2, 4), np.int64), 4)
    with pytest.raises(ValueError, match=">= 0"):
        di._facet_quantile_args(None, "lower", -np.ones((2, 4, 1), np.int64), 4)
    with pytest.raises(ValueError, match="exactly one"):
        di._facet_quantile_args([0.5], "lower", [1], 4)
    with pytest.raises(ValueError, match="method"):
        di._facet_quantile_args([0.5], "linear", None, 4)
    assert di.FacetValueQuantiles._fields == ("values", "ranks", "count", "missing", "total", "other")
    assert di.FacetValuePercentiles._fields == ("values", "count", "missing", "total", "other")


# ---- the host-only code under the host sanitizers --------------------------------------------------------------------------------------------
def test_host_checks_under_a_host_sanitizer(tmp_path):
    """facet_quantile_check.h (the plan against its rule at every level, the limits, every check in the order it is reported, and a per-label
    select against a sort per label) in a stand-alone program built with the host compiler under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "facet_quantile_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "facet_quantile_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "facet_quantile_check: ok" in run.stdout, run.stdout + run.stderr
