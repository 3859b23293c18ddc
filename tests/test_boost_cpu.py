"""CPU checks of boosted search: the numpy reference against its plain-loop twin, the consequences of the contract (weight 0 is
range search, a missing value is neutral, the NaN rule, the pinned field order), the properties of the test inputs that make the GPU tests mean
something, the shard rule on the reference, the argument errors of the Python layers without a device, and boost_check.h (the very
boost_apply the kernels run, and the host-side argument checks) in a stand-alone program under the host sanitizers.  No device is needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd import device_index as di

import _boost_ref as ref
import _range_ref as rr

F32, F64 = np.float32, np.float64
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VR = 2000


def _case(n, B=9):
    ip, ix, va = rr.csr_case(n, VR, seed=n + 40)
    q = rr.sparse_queries(B, VR, seed=n + 1)
    return ip, ix, va, q


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- the reference against its loop twin ---------------------------------------------------------------------------------------------------
def test_sums_are_range_search_before_the_cast():
    ip, ix, va, q = _case(300)
    for store in ("fp32", "fp16", "bin"):
        S = ref.sums(q, ip, ix, va, store)
        assert S.dtype == F64 and (_bits(S.astype(F32)) == _bits(rr.scores(q, ip, ix, va, store))).all()
        assert (S[:, 8::9] == 0).all() and not np.signbit(S[:, 8::9]).any()        # rows with no packets: +0.0


@pytest.mark.parametrize("mode", [ref.ADD, ref.MUL])
def test_numpy_reference_equals_the_loop_reference(mode):
    n, B = 160, 3
    ip, ix, va, q = _case(n, B)
    S = ref.sums(q, ip, ix, va)
    f0, f1, f2, f3 = ref.field_f32(n, 1), ref.field_i32(n, 2), ref.field_f32(n, 3, missing_every=5), ref.field_i32(n, 4, lo=-2 ** 31 + 1, hi=2 ** 31 - 1)
    f0[[3, 4, 17]] = [np.inf, -np.inf, -0.0]
    f2[[8, 9]] = [np.inf, 1e-45]                                     # (row 8 has no packets: S = 0 meets an infinity under "mul")
    for fields, w in (([f0], [0.25]), ([f1, f0], [[0.0, 1.0], [-0.5, 0.05], [1e-3, 0.0]]), ([f0, f1, f2, f3], [0.05, -1e-3, 0.25, 1e-9]),
                      ([f2, f0], [[1.0, -1.0], [np.inf, 1.0], [np.nan, 1.0]])):
        X, valid = ref.boosted(S, fields, w, mode)
        Xl, validl = ref.boosted_loop(S, fields, w, mode)
        assert (valid == validl).all() and (_bits(X)[valid] == _bits(Xl)[valid]).all()
        assert not np.isnan(X[valid]).any() and not (np.signbit(X[valid]) & (X[valid] == 0)).any()
    assert not valid[2].any() and valid[0].any()                     # a NaN weight: its query matches nothing, the others are served
    want = ref.search(S, [f0, f1], [0.05, 0.01], mode, None, 7)
    loop = rr.search_loop(np.where(*ref.boosted(S, [f0, f1], [0.05, 0.01], mode)[::-1], F32(-np.inf)), -np.inf, 7,
                          ref.boosted(S, [f0, f1], [0.05, 0.01], mode)[1])
    rr.assert_equal_bits(loop, want, "search over the boosted matrix")


# ---- the consequences of the contract --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [ref.ADD, ref.MUL])
def test_weight_zero_is_range_search_and_missing_is_neutral(mode):
    n = 500
    ip, ix, va, q = _case(n)
    S = ref.sums(q, ip, ix, va)
    plain = rr.scores(q, ip, ix, va)
    f = ref.field_f32(n, 5)
    f[[0, 1, 2, 8]] = [np.inf, -np.inf, np.inf, -np.inf]             # (row 8 has no packets)
    g = ref.field_i32(n, 6)
    thr = np.sort(plain, axis=1)[:, -120].astype(F32)
    for max_hits in (0, 16, 600):
        want = rr.search(plain, thr, max_hits)
        rr.assert_equal_bits(ref.search(S, [f, g], [0.0, -0.0], mode, thr, max_hits), want, "weight 0")
        gone = [np.full(n, np.nan, F32), np.full(n, ref.INT32_MISSING, np.int32)]
        rr.assert_equal_bits(ref.search(S, gone, [3.0, -2.0], mode, thr, max_hits), want, "all missing")
    # a missing value is neutral row by row
    X, valid = ref.boosted(S, [f], [0.5], mode)
    miss = np.isnan(f)
    assert miss.sum() > 30 and valid[:, miss].all() and (_bits(X[:, miss]) == _bits(plain[:, miss])).all()


def test_nan_rule_and_rows_without_packets():
    n = 200
    ip, ix, va, q = _case(n, 2)
    S = ref.sums(q, ip, ix, va)
    f = ref.field_f32(n, 7, missing_every=0)
    g = f.copy()
    p = int(np.flatnonzero((S > 0).all(axis=0))[0])                  # a row both queries score above 0; row 8 has no packets: S = +0.0
    f[[p, 8]] = np.inf
    g[[p, 8]] = -np.inf
    X, valid = ref.boosted(S, [f, g], [1.0, 1.0], ref.ADD)           # inf + -inf
    assert not valid[:, [p, 8]].any() and valid.sum() == 2 * (n - 2)
    res = ref.search(S, [f, g], [1.0, 1.0], ref.ADD, None, n)
    assert (res["counts"] == n - 2).all() and not np.isin([p, 8], res["ids"]).any()
    assert not (rr.unpack_bits(res["words"], n)[:, [p, 8]]).any()
    X, valid = ref.boosted(S, [f], [1.0], ref.MUL)                   # S = 0 times 1 + inf
    assert not valid[:, 8].any() and valid[:, p].all() and np.isposinf(X[:, p]).all()
    # a row with no packets is ranked by its boost alone
    h = ref.field_f32(n, 8, missing_every=0)
    X, valid = ref.boosted(S, [h], [0.5], ref.ADD)
    empty = np.arange(8, n, 9)
    assert (_bits(X[:, empty]) == _bits(F32(0.5) * h[empty].astype(F64))[None, :]).all()
    X, _ = ref.boosted(S, [h], [0.5], ref.MUL)
    assert (_bits(X[:, empty]) == 0).all()


def test_field_order_is_pinned():
    """S one fp64 ulp above an fp32 tie, a half-ulp and a minus-one-ulp term: the two orders differ in the last bit of the fp32 result"""
    S = np.array([[1.0 + 2.0 ** -24 + 2.0 ** -52]], dtype=F64)
    h, u = np.array([2.0 ** -53], F32), np.array([-2.0 ** -52], F32)
    a, _ = ref.boosted(S, [h, u], [1.0, 1.0], ref.ADD)
    b, _ = ref.boosted(S, [u, h], [1.0, 1.0], ref.ADD)
    assert a[0, 0] == F32(1.0) + F32(2.0 ** -23) and b[0, 0] == F32(1.0) and _bits(a)[0, 0] == _bits(b)[0, 0] + 1
    al, _ = ref.boosted_loop(S, [h, u], [1.0, 1.0], ref.ADD)
    assert _bits(al)[0, 0] == _bits(a)[0, 0]


# ---- the inputs of the GPU tests: a boost that changes nothing, or a case without ties, proves nothing ---------------------------------------------
def test_the_test_inputs_have_the_properties_the_gpu_tests_rely_on():
    n = 1000
    ip, ix, va, q = _case(n)
    S = ref.sums(q, ip, ix, va)
    rows = np.random.default_rng(0).choice(n, size=60, replace=False)
    for store in ("fp32", "fp16"):
        assert ref.exact_sums(q, ip, ix, va, store, rows, b=3)
    f = ref.field_f32(n, n + 7)
    for w in (0.05, 0.25):
        for mode in (ref.ADD, ref.MUL):
            X, valid = ref.boosted(S, [f], [w], mode)
            assert valid.all() and ref.tops_differ(S, X).all()
            assert all(ref.has_ties(X, valid, b) for b in range(9))
    src = ref.twin_sources(n)
    assert len(src) > 100 and all((S[:, r] == S[:, s]).all() for r, s in src.items())
    same = [r for r, s in src.items() if f[r] == f[s]]
    other = [r for r, s in src.items() if f[r] > f[s]]                 # the later row has the larger value: the boost puts it first
    assert len(same) > 20 and len(other) > 10


# ---- the shard rule ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [ref.ADD, ref.MUL])
def test_shard_rule_on_the_reference(mode):
    n = 1000
    ip, ix, va, q = _case(n)
    S = ref.sums(q, ip, ix, va)
    fields, w = [ref.field_f32(n, 11), ref.field_i32(n, 12)], np.random.default_rng(1).normal(size=(9, 2)).astype(F32) * F32(0.01)
    allowed = np.random.default_rng(2).random((9, n)) < 0.7
    X, _ = ref.boosted(S, fields, w, mode)
    thr = np.sort(X, axis=1)[:, -150]
    for a in (None, allowed):
        for max_hits in (0, 30, 600):
            want = ref.search(S, fields, w, mode, thr, max_hits, a)
            rr.assert_equal_bits(ref.shard_search(S, fields, w, mode, thr, max_hits, [0, 437, 438, n], a), want, ("shards", max_hits))


# ---- argument errors without a device -------------------------------------------------------------------------------------------------------------
def test_boost_args():
    q = np.zeros((3, 8), F32)
    f, g = np.zeros(10, F32), np.zeros(10, np.int32)
    B, thr, K, (fields, dtypes, w, mode) = di._boost_args(q, [f, g], [0.5, -1], "mul", None, 7, 10)
    assert B == 3 and K == 7 and np.isneginf(thr).all() and thr.dtype == F32 and dtypes == [nat.VAL_F32, nat.VAL_I32] and mode == nat.BOOST_MUL
    assert w.dtype == F32 and w.shape == (3, 2) and w.flags.c_contiguous and (w == [[0.5, -1]] * 3).all()
    _, thr, _, (_, _, w, mode) = di._boost_args(torch.zeros(3, 8), [torch.zeros(10)], np.ones((3, 1)), "add", [0.0, 1.0, 2.0], 0)
    assert (thr == [0, 1, 2]).all() and mode == nat.BOOST_ADD and w.shape == (3, 1)
    bad = [
        (ValueError, "mode", dict(mode="max")),
        (TypeError, "list", dict(boosts=f)),
        (TypeError, "list", dict(boosts={"a": f})),
        (ValueError, "1..4", dict(boosts=[])),
        (ValueError, "1..4", dict(boosts=[f] * 5, weights=[1] * 5)),
        (TypeError, "float32 or int32", dict(boosts=[f.astype(np.float64)])),
        (TypeError, "not an array", dict(boosts=[None])),
        (ValueError, "one entry per row", dict(boosts=[np.zeros(9, F32)])),
        (ValueError, "one entry per row", dict(boosts=[np.zeros((10, 1), F32)])),
        (ValueError, "weights", dict(weights=[1.0, 2.0])),
        (ValueError, "weights", dict(weights=np.ones((2, 1)))),
        (ValueError, "weights", dict(weights=1.0)),
        (ValueError, "finite", dict(weights=[np.nan])),
        (ValueError, "finite", dict(weights=[[1.0], [np.inf], [0.0]])),
        (ValueError, "NaN", dict(min_score=np.nan)),
        (ValueError, "min_score", dict(min_score=[0.0, 1.0])),
        (ValueError, "max_hits", dict(max_hits=2049)),
        (TypeError, "max_hits", dict(max_hits=1.5)),
        (ValueError, "queries", dict(q=np.zeros(8, F32))),
    ]
    for exc, match, kw in bad:
        args = dict(q=q, boosts=[f], weights=[1.0], mode="add", min_score=None, max_hits=5, n_rows=10)
        args.update(kw)
        with pytest.raises(exc, match=match):
            di._boost_args(**args)


def test_index_facade_errors_before_any_device_work():
    from vsearch_amd.ir import SparseIndex
    idx = SparseIndex(device="cpu")
    idx._values = {name: torch.zeros(4) for name in "abcde"}
    q = torch.zeros(2, 6)
    names, w = idx._boost_fields({"b": 0.5, "a": [1.0, -1.0]}, 2)
    assert names == ["b", "a"] and w.dtype == F32 and (w == [[0.5, 1.0], [0.5, -1.0]]).all()
    with pytest.raises(KeyError, match="no value field 'year'"):
        idx.search_boosted(q, 5, boosts={"a": 1.0, "year": 0.5})
    with pytest.raises(ValueError, match="at most 4"):
        idx.search_boosted(q, 5, boosts=dict.fromkeys("abcde", 1.0))
    with pytest.raises(TypeError, match="dict"):
        idx.search_boosted(q, 5, boosts=None)
    with pytest.raises(TypeError, match="dict"):
        idx.search_boosted(q, 5, boosts={})
    with pytest.raises(ValueError, match="one per query"):
        idx.search_boosted(q, 5, boosts={"a": [1.0, 2.0, 3.0]})
    with pytest.raises(ValueError, match="finite"):
        idx.search_boosted(q, 5, boosts={"a": float("nan")})
    with pytest.raises(ValueError, match="mode"):
        idx.search_boosted(q, 5, boosts={"a": 1.0}, mode="max")


def test_the_prototype_matches_the_header():
    hdr = open(os.path.join(REPO, "include", "vsearch_hip.h")).read()
    decl = hdr[hdr.index("VS_API int vs_index_search_boosted("):]
    decl = decl[:decl.index(";")]
    assert decl.count(",") + 1 == len(nat._SIGNATURES["vs_index_search_boosted"][0]) == 22
    for name, val in (("VS_BOOST_ADD", nat.BOOST_ADD), ("VS_BOOST_MUL", nat.BOOST_MUL), ("VS_BOOST_MAX_FIELDS", nat.BOOST_MAX_FIELDS)):
        assert f"#define {name} {val}\n" in hdr


# ---- boost_check.h under the host sanitizers -----------------------------------------------------------------------------------------------------
RECORD = np.dtype([("S", "<f8"), ("w", "<f4", 4), ("raw", "<u4", 4), ("dtype", "<i4", 4), ("F", "<i4"), ("mode", "<i4")])


def _tuples():
    """(records, expected ok, expected bits): groups of rows under one weight vector each, so that the numpy reference serves a group a call"""
    rng = np.random.default_rng(123)
    s_special = np.array([0.0, -0.0, np.inf, -np.inf, 1.0 + 2.0 ** -24 + 2.0 ** -52, 5e-324, -2.0 ** -1074, 3.0e38, 3.5e38, -3.5e38, 2.0 ** -149, 2.0 ** -150,
                          1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 - 2.0 ** -53], F64)
    f_special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3.4e38, -3.4e38, 2.0 ** -53, -2.0 ** -52, 1.0], F32)
    i_special = np.array([-2 ** 31, -2 ** 31 + 1, 2 ** 31 - 1, 0, -1, 1, 2 ** 24 + 1], np.int32)
    w_special = [0.0, -0.0, 1.0, -1.0, 0.05, 0.25, 1e-45, 3.4e38, -3.4e38, np.inf, -np.inf, np.nan, 2.0 ** -24]
    recs, oks, bits = [], [], []
    m = 150
    for mode in (ref.ADD, ref.MUL):
        for F in (1, 2, 3, 4):
            for g in range(8):
                w = np.array([w_special[(g * 3 + 5 * j + F) % len(w_special)] if (g + j) % 3 else rng.normal() for j in range(F)], F32)
                S = np.where(rng.random(m) < 0.3, rng.choice(s_special, m), rng.normal(size=m) * 10.0 ** rng.integers(-3, 4, m)).astype(F64)
                fields, dts = [], []
                for j in range(F):
                    if (g + j + F) % 2:
                        col = np.where(rng.random(m) < 0.4, rng.choice(f_special, m), (rng.random(m) * 10).astype(F32)).astype(F32)
                        dts.append(nat.VAL_F32)
                    else:
                        col = np.where(rng.random(m) < 0.4, rng.choice(i_special, m), rng.integers(-2000, 2000, m)).astype(np.int32)
                        dts.append(nat.VAL_I32)
                    fields.append(col)
                X, valid = ref.boosted(S[None, :], fields, w, mode)
                r = np.zeros(m, RECORD)
                r["S"], r["F"], r["mode"] = S, F, nat.BOOST_ADD if mode == ref.ADD else nat.BOOST_MUL
                for j in range(F):
                    r["w"][:, j], r["raw"][:, j], r["dtype"][:, j] = w[j], fields[j].view(np.uint32), dts[j]
                recs.append(r)
                oks.append(valid[0])
                bits.append(_bits(X)[0])
    return np.concatenate(recs), np.concatenate(oks), np.concatenate(bits)


def test_boost_apply_and_the_host_checks_under_a_host_sanitizer(tmp_path):
    """boost_check.h in a stand-alone program built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer: its own checks
    (argument errors, hand-made tuples), then boost_apply over thousands of (S, w, v) tuples against the bits numpy computes"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "boost_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "boost_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "boost_check: ok" in run.stdout, run.stdout + run.stderr
    recs, ok, bits = _tuples()
    n = recs.shape[0]
    assert n >= 4000 and RECORD.itemsize == 64 and 0.02 < 1 - ok.mean() < 0.5        # thousands of tuples, some of which match nothing
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(np.int32(n).tobytes())
        fh.write(recs.tobytes())
    run = subprocess.run([prog, fin, fout], capture_output=True, text=True)
    assert run.returncode == 0 and f"{n} records" in run.stdout, run.stdout + run.stderr
    got = np.fromfile(fout, dtype=np.uint32).reshape(n, 2)
    bad = np.flatnonzero((got[:, 0] != ok) | ((got[:, 1] != bits) & ok))
    assert bad.size == 0, (bad[:5], recs[bad[:5]], got[bad[:5]], ok[bad[:5]], bits[bad[:5]])
