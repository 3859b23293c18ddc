"""CPU checks of the clustering calls: the numpy reference against a plain triple loop, ties, zeros and NaN, empty rows, the
Euclidean bias against a brute-force argmin, the half norms' fixed order, the shard rule, the plan rule (vs_assign_plan is pure host arithmetic),
the argument errors of the C ABI without a GPU, the facade's host logic, and the host-side checks (vsearch_amd/csrc/assign_check.h) run in a
stand-alone program under the host sanitizers.  No device is needed."""
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

import _term_agg_ref as aref
import _cluster_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _case(n, V, seed, grid=False, max_len=None):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, (max_len or V) + 1, size=n)
    lens[:3] = (0, 1, min(V, max_len or V))                               # an empty row, one cell, the longest
    ip, ix, va = aref.csr_case(lens, V, seed=seed)
    va = ref.grid(rng, va.size) if grid else (va * (0.5 + rng.random(va.size)).astype(F32)).astype(F32)
    return ip, ix, va, rng


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["fp32", "fp16", "bin"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_reference_equals_the_triple_loop(store, with_bias):
    n, V, K = 23, 11, 5
    ip, ix, va, rng = _case(n, V, seed=3 + with_bias)
    if store == "fp16":
        va = va.astype(np.float16).astype(F32)
    vals = None if store == "bin" else va
    cen = rng.standard_normal((K, V)).astype(F32)
    bias = rng.standard_normal(K).astype(F32) if with_bias else None
    allowed = rng.random(n) < 0.8
    got = ref.assign(ip, ix, vals, V, cen, bias, allowed, store)
    want = ref.assign_loop(ip, ix, vals, V, cen, bias, allowed, store)
    assert got[0].dtype == np.int32 and got[1].dtype == F32
    assert (got[0] == want[0]).all() and (got[1].view(np.uint32) == want[1].view(np.uint32)).all()
    assert (got[0][~allowed] == -1).all() and np.isneginf(got[1][~allowed]).all() and (got[0][allowed] >= 0).all()
    assert len(set(got[0][allowed].tolist())) > 1


def test_ties_go_to_the_lowest_centroid():
    ip, ix, va = np.array([0, 2, 4]), np.array([0, 1, 1, 2]), np.array([1, 2, 3, 4], F32)
    cen = np.array([[0, 0, 0], [1, 1, 1], [1, 1, 1], [5, 0, 0], [5, 0, 0]], F32)
    labels, values = ref.assign(ip, ix, va, 3, cen)
    assert labels.tolist() == [3, 1] and values.tolist() == [5.0, 7.0]
    labels, _ = ref.assign(ip, ix, va, 3, cen[::-1].copy())                # the same centroids in reverse: still the lower index
    assert labels.tolist() == [0, 2]


def test_zeros_compare_equal_and_nan_counts_as_minus_inf():
    ip, ix, va = np.array([0, 1]), np.array([0]), np.array([1e-30], F32)
    cen = np.array([[-1e-30], [0.0], [1e-30]], F32)                       # the products underflow in fp32: -0.0, +0.0, +0.0
    labels, values = ref.assign(ip, ix, va, 1, cen)
    assert labels.tolist() == [0] and values.view(np.uint32).tolist() == [0]        # -0.0 == +0.0: the lowest j, reported as +0.0
    cen = np.array([[np.inf], [1.0], [-np.inf]], F32)
    va0 = np.array([0.0], F32)                                             # inf * 0 = NaN: as -inf, so centroid 1 (value 0) wins
    labels, values = ref.assign(ip, ix, va0, 1, cen)
    assert labels.tolist() == [1] and values.tolist() == [0.0]
    labels, values = ref.assign(ip, ix, va0, 1, cen[[0, 2]])               # all NaN: label 0, value -inf
    assert labels.tolist() == [0] and np.isneginf(values).all()
    assert ref.assign_loop(ip, ix, va0, 1, cen[[0, 2]])[0].tolist() == [0]


def test_an_empty_row_with_and_without_bias():
    ip, ix, va = np.array([0, 0, 1]), np.array([2]), np.array([1.0], F32)
    cen = np.array([[1, 1, -3], [2, 2, -2], [3, 3, -1]], F32)
    labels, values = ref.assign(ip, ix, va, 3, cen)
    assert labels.tolist() == [0, 2] and values.tolist() == [0.0, -1.0]    # S = +0.0 for every centroid: label 0
    bias = np.array([-5, -1, -9], F32)
    labels, values = ref.assign(ip, ix, va, 3, cen, bias)
    assert labels.tolist() == [1, 1] and values.tolist() == [-1.0, -3.0]   # the argmax of the bias
    pad = ref.assign(np.array([0, 2, 3]), np.array([3, 3, 2]), np.array([7.0, 7.0, 1.0], F32), 3, cen, bias)      # cells with the padding id are skipped
    assert pad[0].tolist() == [1, 1] and pad[1].tolist() == [-1.0, -3.0]


def test_l2_labels_equal_a_brute_force_argmin_on_grid_inputs():
    n, V, K = 60, 17, 9
    ip, ix, va, rng = _case(n, V, seed=11, grid=True)
    cen = ref.grid(rng, (K, V), denom=16)                                  # sixteenths: the half norms and the values are exact in fp32 as well
    hn = ref.half_norms(cen)
    assert (hn.astype(np.float64) == 0.5 * (cen.astype(np.float64) ** 2).sum(axis=1)).all()       # exact on grid inputs
    labels, values = ref.assign(ip, ix, va, V, cen, -hn)
    X = np.zeros((n, V))
    X[np.repeat(np.arange(n), np.diff(ip)), ix] = va
    d2 = ((X[:, None, :] - cen[None, :, :].astype(np.float64)) ** 2).sum(axis=2)                   # exact in fp64
    assert (labels == d2.argmin(axis=1)).all()
    assert ((X ** 2).sum(axis=1) - 2 * values.astype(np.float64) == d2.min(axis=1)).all()


@pytest.mark.parametrize("V", [1, 255, 256, 257, 1000])
def test_half_norm_order_equals_the_explicit_tree(V):
    rng = np.random.default_rng(V)
    cen = (rng.standard_normal((3, V)) * 10.0 ** rng.integers(-3, 4, size=(3, V))).astype(F32)
    for store in ("fp32", "fp16"):
        got = ref.half_norms(cen, store)
        want = np.array([ref.half_norms_tree(cen[j], store) for j in range(3)], F32)
        assert got.dtype == F32 and (got.view(np.uint32) == want.view(np.uint32)).all()
    assert (ref.half_norms(np.zeros((2, V), F32)) == 0).all()


def test_row_shards_concatenate_to_the_whole():
    n, V, K = 70, 13, 6
    ip, ix, va, rng = _case(n, V, seed=5)
    cen, bias = rng.standard_normal((K, V)).astype(F32), rng.standard_normal(K).astype(F32)
    allowed = rng.random(n) < 0.7
    whole = ref.assign(ip, ix, va, V, cen, bias, allowed)
    parts = []
    for r0, r1 in ((0, 33), (33, 34), (34, n)):
        sub = ip[r0:r1 + 1] - ip[r0]
        parts.append(ref.assign(sub, ix[ip[r0]:ip[r1]], va[ip[r0]:ip[r1]], V, cen, bias, allowed[r0:r1]))
    assert (np.concatenate([p[0] for p in parts]) == whole[0]).all()
    assert (np.concatenate([p[1] for p in parts]).view(np.uint32) == whole[1].view(np.uint32)).all()


def test_label_bitmaps_reference():
    labels = np.array([0, 2, -1, 2, 5, 0], np.int32)
    w = ref.label_bitmaps(labels, [0, 2, 7, -1], bit0=0)
    assert w.dtype == np.uint32 and w[:, 0].tolist() == [0b100001, 0b001010, 0, 0b000100]
    w = ref.label_bitmaps(labels, [2], bit0=30)
    assert w.shape == (1, 2) and w[0].tolist() == [1 << 31, 0b10]
    m = ref.unpack(ref.label_bitmaps(labels, np.arange(6), bit0=37), 37, 6)
    assert (m == (labels[None, :] == np.arange(6)[:, None])).all()


def test_kmeans_reference_on_two_obvious_blobs():
    ip = np.arange(0, 13, 2)
    ix = np.array([0, 1] * 3 + [2, 3] * 3)
    va = np.array([1, 1, 1.5, 1, 1, 1.25, 2, 2, 2.5, 2, 2, 2.25], F32)
    for metric in ("l2", "dot"):
        C, labels, values, counts, n_iter, changed = ref.kmeans(ip, ix, va, 4, np.eye(4, dtype=F32)[[0, 2]], 5, metric)
        assert labels.tolist() == [0, 0, 0, 1, 1, 1] and counts.tolist() == [3, 3] and changed == [6, 0] and n_iter == 2
        assert C[0].tolist() == [F32(3.5 / 3), F32(3.25 / 3), 0, 0]
    dup = ref.kmeans(ip, ix, va, 4, np.eye(4, dtype=F32)[[0, 0, 2]], 5)     # a duplicated start: the higher index stays empty and is kept
    assert dup[3].tolist() == [3, 0, 3] and dup[0][1].tolist() == [1, 0, 0, 0]
    none = ref.kmeans(ip, ix, va, 4, np.eye(4, dtype=F32)[[0, 2]], 0)
    assert none[4] == 0 and none[5] == [] and (none[0] == np.eye(4, dtype=F32)[[0, 2]]).all() and none[1].tolist() == [0, 0, 0, 1, 1, 1]


# ---- the plan rule (pure host arithmetic: no device) ------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_constants():
    text = open(os.path.join(REPO, "include", "vsearch_hip.h")).read()
    get = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert get("VS_ASSIGN_MAX_K") == nat.ASSIGN_MAX_K == ref.MAX_K == di.MAX_ASSIGN_K == 4096
    assert get("VS_LABEL_MAX_VALUES") == nat.LABEL_MAX_VALUES == ref.MAX_VALUES == di.MAX_LABEL_VALUES
    assert di.KMEANS_UPDATE_BATCH == ref.UPDATE_BATCH == 64
    for name in ("vs_assign_plan", "vs_index_assign", "vs_centroid_half_norms", "vs_label_bitmaps"):
        assert name in nat.EXPORTED_SYMBOLS and re.search(r"VS_API int %s\(" % name, text)


@pytest.mark.parametrize("K", [1, 64, 65, 128, 129, 257, 4096])
def test_plan_rule(K):
    for n_rows in (1, 63, 64, 65, 2049, 1_000_000, 21_000_000, (1 << 32) - 1):
        for rpc_in in (0, 64, 2048, 1 << 20):
            got = di.assign_plan(n_rows, K, 29523, rpc_in)
            assert got == ref.plan(n_rows, K, 29523, rpc_in)
            w, slices, chunks, rpc, slab = got
            assert w in (64, 128, 256) and slices * w >= K > (slices - 1) * w                # the slices cover the centroids, none is empty
            assert rpc > 0 and rpc % 64 == 0 and chunks * rpc >= n_rows > (chunks - 1) * rpc  # the chunks cover the rows
            assert slab == 29524 * slices * w * 4
            if rpc_in:
                assert rpc == rpc_in                                                         # an explicit value is taken as given
            else:
                assert chunks <= 4096
    assert di.assign_plan(100, K, 29523)[0] == (64 if K <= 64 else 128 if K <= 128 else 256)


def test_plan_argument_errors():
    for args in [(0, 1, 4, 0), (1 << 32, 1, 4, 0), (100, 0, 4, 0), (100, 4097, 4, 0), (100, 1, 0, 0), (100, 1, 65536, 0), (100, 1, 4, 100),
                 (100, 1, 4, -64)]:
        with pytest.raises(ValueError):
            di.assign_plan(*args)
    with pytest.raises(ValueError, match="multiple of 64"):
        di.assign_plan(100, 1, 4, 100)
    with pytest.raises(ValueError, match="4096"):
        di.assign_plan(100, 4097, 4)
    o32, o64 = C.c_int32(0), C.c_int64(0)
    assert nat.lib().vs_assign_plan(100, 1, 4, 0, None, C.byref(o32), C.byref(o64), C.byref(o64), C.byref(o64)) == nat.VS_EINVAL
    assert nat.lib().vs_assign_plan(100, 1, 4, 0, C.byref(o32), C.byref(o32), C.byref(o64), C.byref(o64), C.byref(o64)) == nat.VS_OK


# ---- argument errors of the C ABI, checked before the device is touched ----------------------------------------------------------------------
def test_assign_refuses_a_null_handle_without_a_device():
    cen, labels = np.zeros((2, 4), F32), np.zeros(8, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert nat.lib().vs_index_assign(None, p(cen), 4, 2, None, None, 0, 0, p(labels), None, None) == nat.VS_EINVAL and "NULL" in nat.last_error()


def test_norm_and_bitmap_argument_errors_without_a_device(have_gpu):
    good = nat.VS_OK if have_gpu else nat.VS_ENODEVICE
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    cen, out = np.ones((2, 6), F32), np.zeros(2, F32)
    norms = lambda c=cen, ldc=6, K=2, V=6, o=out: nat.lib().vs_centroid_half_norms(p(c), ldc, K, V, 0, p(o), 0, None)
    assert norms() == good
    assert norms(K=0) == nat.VS_EINVAL and norms(K=4097) == nat.VS_EINVAL and "4096" in nat.last_error()
    assert norms(V=0) == nat.VS_EINVAL and norms(ldc=5) == nat.VS_EINVAL and "ldc" in nat.last_error()
    assert norms(c=None) == nat.VS_EINVAL and norms(o=None) == nat.VS_EINVAL and "NULL" in nat.last_error()
    labels, values, words = np.zeros(100, np.int32), np.zeros(3, np.int32), np.zeros((3, 5), np.uint32)
    maps = lambda l=labels, n=100, v=values, B=3, bit0=0, w=words, ld=5: nat.lib().vs_label_bitmaps(p(l), n, p(v), B, bit0, p(w), ld, 0, None)
    assert maps() == good and maps(bit0=31) == good                                  # 131 bits span 5 words
    assert maps(bit0=61) == nat.VS_EINVAL and "ld_words" in nat.last_error()
    assert maps(n=0) == nat.VS_EINVAL and maps(B=0) == nat.VS_EINVAL and maps(B=4097) == nat.VS_EINVAL and maps(bit0=-1) == nat.VS_EINVAL
    for null in (dict(l=None), dict(v=None), dict(w=None)):
        assert maps(**null) == nat.VS_EINVAL and "NULL" in nat.last_error()


# ---- the facade's host logic -----------------------------------------------------------------------------------------------------------------
def test_facade_validation_needs_no_device():
    from vsearch_amd.doc_filter import DocFilter
    from vsearch_amd.ir import SparseIndex
    from vsearch_amd.ir.retriever.retriever import Retriever
    c, b, rpc = di._assign_args(np.ones((3, 5)), [0.5, 1, 2], 5, 128)
    assert c.dtype == torch.float32 and tuple(c.shape) == (3, 5) and b.dtype == torch.float32 and rpc == 128
    for bad in (dict(centroids=np.ones((0, 5), F32)), dict(centroids=np.ones((4097, 5), F32)), dict(centroids=np.ones((3, 4), F32)),
                dict(centroids=np.ones(5, F32)), dict(centroids=np.full((3, 5), np.nan, F32)), dict(centroids=np.full((3, 5), np.inf, F32)),
                dict(bias=np.ones(2, F32)), dict(bias=np.array([0, np.inf, 0], F32)), dict(bias=np.array([0, np.nan, 0], F32)),
                dict(rows_per_chunk=100), dict(rows_per_chunk=-64), dict(rows_per_chunk=True)):
        with pytest.raises(ValueError):
            di._assign_args(**{"centroids": np.ones((3, 5), F32), "bias": None, "n_cols": 5, **bad})
    for bad in (dict(centroids=np.ones((3, 5), np.int64)), dict(bias=np.ones(3, np.int32))):
        with pytest.raises(TypeError):
            di._assign_args(**{"centroids": np.ones((3, 5), F32), "bias": None, "n_cols": 5, **bad})
    assert di._kmeans_args(7, 0, "dot") == (7, 0) and di._kmeans_args(np.int64(4096), np.int32(3), "l2") == (4096, 3)
    for bad in ((0, 1, "l2"), (4097, 1, "l2"), (3, -1, "l2"), (3, 1, "cosine"), (3, 1, None)):
        with pytest.raises(ValueError):
            di._kmeans_args(*bad)
    for bad in ((2.0, 1, "l2"), (True, 1, "l2"), (3, "1", "l2")):
        with pytest.raises(TypeError):
            di._kmeans_args(*bad)
    with pytest.raises(ValueError, match="init"):
        di._kmeans_args(3, 1, "l2", np.arange(4), 5)
    with pytest.raises(ValueError, match="columns"):
        di._kmeans_args(3, 1, "l2", np.ones((3, 4), F32), 5)
    with pytest.raises(ValueError, match="finite"):
        di._kmeans_args(3, 1, "l2", np.full((3, 5), np.nan, F32), 5)
    with pytest.raises(TypeError):
        di._kmeans_args(3, 1, "l2", np.ones(3, F32), 5)
    with pytest.raises(TypeError):
        di._kmeans_args(3, 1, "l2", np.ones((3, 5), np.int64), 5)
    assert di._kmeans_args(3, 1, "l2", torch.arange(3), 5) == (3, 1) and di._kmeans_args(3, 1, "l2", np.ones((3, 5), F32), 5) == (3, 1)
    vals, scalar = di._label_values(3)
    assert vals.dtype == np.int32 and vals.tolist() == [3] and scalar
    assert di._label_values([1, -1, 7])[0].tolist() == [1, -1, 7] and not di._label_values(np.arange(4096))[1]
    for bad in ([], np.arange(4097), [1 << 31]):
        with pytest.raises(ValueError):
            di._label_values(bad)
    for bad in ([0.5], [[1, 2]], [True]):
        with pytest.raises(TypeError):
            di._label_values(bad)
    with pytest.raises(TypeError):
        DocFilter.from_labels(np.ones(5, F32), 1)
    with pytest.raises(TypeError):
        DocFilter.from_labels(np.ones((2, 5), np.int32), 1)
    with pytest.raises(ValueError):
        DocFilter.from_labels(np.ones(5, np.int32), [])
    with pytest.raises(ValueError, match="ld_words"):
        di.label_bitmaps(np.zeros(100, np.int32), [1], bit0=31, ld_words=4)
    idx = SparseIndex()
    with pytest.raises(ValueError, match="metric"):
        idx.assign(np.ones((2, 5), F32), metric="cosine")
    with pytest.raises(ValueError, match="n_clusters"):
        idx.kmeans(0)
    with pytest.raises(ValueError, match="n_clusters"):
        idx.cluster(4097)
    with pytest.raises(ValueError, match="metric"):
        idx.kmeans(3, metric="cosine")
    with pytest.raises(ValueError, match="iters"):
        idx.kmeans(3, iters=-1)
    with pytest.raises(RuntimeError, match="no index"):
        Retriever.cluster_documents(type("R", (), {"index": None})(), 3)


# ---- the host-side checks under the host sanitizers ------------------------------------------------------------------------------------------
def test_host_checks_under_a_host_sanitizer(tmp_path):
    """assign_check.h (the plan rule with its slices and its slab, every limit of the calls, and what vs_index_assign checks in host centroids and
    a host bias before it stages them) in a stand-alone program built with the host compiler under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "assign_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "assign_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "assign_check: ok" in run.stdout, run.stdout + run.stderr
