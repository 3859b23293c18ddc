"""Scores as a field without a GPU: the numpy reference against plain loops, the shard rule, vs_set_score_plan's arithmetic,
the argument errors of vs_index_set_scores that the host decides, and the facade's argument errors."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _score_field_ref as ref
from vsearch_amd import _native as nat
from vsearch_amd import device_index as di

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _p(a):
    return C.c_void_p(a.ctypes.data)


# ---- the reference -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["fp32", "fp16", "bin"])
@pytest.mark.parametrize("bit0,ld", [(0, 0), (5, 0), (37, 1), (0, None)])
def test_reference_equals_plain_loops(store, bit0, ld):
    n, V, B = 150, 97, 3
    indptr, indices, values = ref.csr_case(n, V, seed=3, max_nnz=12)
    q = ref.sparse_queries(B, V, seed=4, nnz=20)
    rng = np.random.default_rng(5)
    deleted = rng.random(n) < 0.1
    if ld is None:
        words, ldw = None, 0
    else:
        words = ref.pack_at(rng.random((B if ld else 1, n)) < 0.4, bit0)
        ldw = words.shape[1] if ld else 0
    S = ref.scores(q, indptr, indices, values, store)
    got = ref.set_scores(S, words, ldw, bit0, deleted)
    want = ref.set_scores_loop(q, indptr, indices, values, store, words, ldw, bit0, deleted)
    assert ref.same(got, want)
    outside = ~ref.in_set(words, ldw, bit0, n, B) | deleted[None, :]
    assert (ref.bits(got)[outside] == ref.NAN_BITS).all() and not np.isnan(got[~outside]).any()
    assert (ref.bits(got)[~outside] == ref.bits(S)[~outside]).all()


def test_empty_rows_score_plus_zero_and_the_sentinel_is_one_pattern():
    indptr, indices, values = ref.csr_case(40, 31, seed=1, max_nnz=5, empty_every=4)
    S = ref.scores(ref.sparse_queries(2, 31, seed=2, nnz=10), indptr, indices, values)
    out = ref.set_scores(S)
    empty = np.flatnonzero(np.diff(indptr) == 0)
    assert empty.size and (ref.bits(out)[:, empty] == 0).all()                          # +0.0, never -0.0, never missing
    assert (ref.bits(ref.set_scores(S, ref.pack_at(np.zeros((1, 40), bool), 0), 0, 0)) == 0x7FC00000).all()
    assert (ref.key(ref.set_scores(S, ref.pack_at(np.zeros((1, 40), bool), 0), 0, 0)) == 0).all()   # the sentinel's order key: missing


@pytest.mark.parametrize("cuts", [(0, 5, 101, 150), (0, 33, 64, 150), (0, 1, 149, 150)])
@pytest.mark.parametrize("per_query", [False, True])
def test_shard_rule_slices_side_by_side_equal_the_whole(cuts, per_query):
    n, V, B = 150, 97, 3
    indptr, indices, values = ref.csr_case(n, V, seed=7, max_nnz=12)
    S = ref.scores(ref.sparse_queries(B, V, seed=8, nnz=20), indptr, indices, values)
    rng = np.random.default_rng(9)
    deleted = rng.random(n) < 0.1
    for bit0 in (0, 5):
        words = ref.pack_at(rng.random((B if per_query else 1, n)) < 0.5, bit0)
        ld = words.shape[1] if per_query else 0
        assert ref.same(ref.shard_slices(S, cuts, words, ld, bit0, deleted), ref.set_scores(S, words, ld, bit0, deleted))
    assert ref.same(ref.shard_slices(S, cuts, None, 0, 0, deleted), ref.set_scores(S, None, 0, 0, deleted))


def test_the_set_shapes_of_the_gpu_tests_are_what_they_say():
    n, B = ref.N_ROWS, 3
    sets = ref.set_shapes(n, B)
    assert n == 2 * 2048 + 77 and n % 32 != 0
    assert sets["every"].all() and not sets["none"].any()
    assert sets["first"].sum() == 1 and sets["first"][0, 0] and sets["last"].sum() == 1 and sets["last"][0, n - 1]
    assert sets["gap"][0, :2048].any() and not sets["gap"][0, 2048:4096].any() and sets["gap"][0, 4096:].all()
    assert 0.003 < sets["p1"].mean() < 0.03 and 0.45 < sets["p50"].mean() < 0.55
    assert (sets["run"].sum(axis=1) == 300).all() and sets["run"][0, 2047] and sets["run"][0, 2048]
    ip, ix, v = ref.long_rows_case(n, 1000, seed=11)
    lens = np.diff(ip)
    assert (lens >= 520).sum() >= 4 and lens.max() <= 1000 and (lens == 0).sum() > n // 10       # > 64 packets a row; empty rows


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    text = open(os.path.join(REPO, "include", "vsearch_hip.h")).read()
    for name in ("vs_set_score_plan", "vs_index_set_scores"):
        assert name in nat.EXPORTED_SYMBOLS and ("VS_API int %s(" % name) in text
    assert re.search(r"NaN 0x7FC00000", text) and ref.NAN_BITS == 0x7FC00000


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 2049, ref.N_ROWS, 10_000, 1_000_000, 21_000_000, (1 << 32) - 1])
@pytest.mark.parametrize("B,V", [(1, 1), (3, 1000), (8, 29523), (64, 32763)])
def test_plan_chunks_cover_the_rows(n_rows, B, V):
    for rpc_in in (0, 64, 2048, 4096, 1 << 20):
        if rpc_in and -(-n_rows // rpc_in) * B > 0x7FFFFFFF:
            with pytest.raises(ValueError, match="too many"):
                di.set_score_plan(n_rows, B, V, True, rpc_in)
            continue
        for per_query in (True, False):                                                # a shared bitmap serves any B: the rule is the same
            chunks, rpc = di.set_score_plan(n_rows, B, V, per_query, rpc_in)
            assert rpc > 0 and rpc % 64 == 0
            assert chunks * rpc >= n_rows > (chunks - 1) * rpc
            if rpc_in:
                assert rpc == rpc_in                                                   # an explicit value is taken as given
            else:
                assert B * chunks <= max(1024, B)                                      # about 1024 work items over the batch
                want = max(1, 1024 // B)
                assert rpc == max(2048, -(-(-(-n_rows // want)) // 64) * 64)           # n_rows / want rounded up to 64 rows, one span at least
                if n_rows >= 2048 * want:
                    assert B * chunks > (want - 64) * B                                # ... so the rounds of workgroups are full but for the last few


def test_plan_argument_errors():
    for args in [(0, 1, 4, True, 0), (1 << 32, 1, 4, True, 0), (100, 0, 4, True, 0), (100, 1, 0, True, 0), (100, 1, 65536, True, 0),
                 (100, 1, 4, True, 100), (100, 1, 4, True, -64)]:
        with pytest.raises(ValueError):
            di.set_score_plan(*args)
    out = C.c_int64(0)
    assert nat.lib().vs_set_score_plan(100, 1, 4, 1, 0, None, C.byref(out)) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert nat.lib().vs_set_score_plan(100, 1, 4, 1, 0, C.byref(out), None) == nat.VS_EINVAL
    assert nat.lib().vs_set_score_plan(100, 2, 4, 0, 0, C.byref(out), C.byref(out)) == nat.VS_OK


# ---- vs_index_set_scores: what the host refuses before it looks at the index or the device -------------------------------------------------
def test_call_errors_without_a_device():
    """The checks that need no index come first, so they are reachable without a GPU: a handle cannot exist there.  The checks against an
    index's shape (ldq, ld_words too short, ld_scores, the unsupported kinds) are test_gpu_score_field's."""
    q, out, words = np.zeros((2, 8), F32), np.zeros((2, 64), F32), np.full((2, 4), -1, np.int32)
    L = nat.lib()

    def call(idx=None, q=q, q_dtype=nat.VS_F32, ldq=8, B=2, words=words, bit0=0, ld_words=4, rpc=0, out=out, ld_scores=64):
        return L.vs_index_set_scores(idx, _p(q) if q is not None else None, q_dtype, ldq, B, _p(words) if words is not None else None, bit0,
                                     ld_words, rpc, _p(out) if out is not None else None, ld_scores, None)
    assert call(q=None) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert call(out=None) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert call(q_dtype=nat.VS_I32) == nat.VS_EINVAL and "q_dtype" in nat.last_error()
    assert call(B=0) == nat.VS_EINVAL and "B must be positive" in nat.last_error()
    assert call(bit0=-1) == nat.VS_EINVAL and "bit0" in nat.last_error()
    assert call(ld_words=-1) == nat.VS_EINVAL and "ld_words" in nat.last_error()
    for rpc in (100, -64, 1 << 33):
        assert call(rpc=rpc) == nat.VS_EINVAL and "rows_per_chunk" in nat.last_error()
    assert call() == nat.VS_EINVAL and "NULL" in nat.last_error()                      # everything right but the handle
    assert call(words=None, ld_words=0) == nat.VS_EINVAL and "NULL" in nat.last_error()


def test_a_good_call_without_a_device_is_enodevice(have_gpu):
    """a good call needs an index, and making one is where a machine without a GPU says VS_ENODEVICE; with one, host buffers work"""
    n, V = 10, 8
    ip, ix, v = ref.csr_case(n, V, seed=0, max_nnz=3)
    h = C.c_void_p()
    rc = nat.lib().vs_index_create_csr(_p(ip), nat.VS_I64, _p(ix), nat.VS_I32, _p(v), nat.VS_F32, nat.VS_F32, n, V, 0, C.byref(h))
    if not have_gpu:
        assert rc == nat.VS_ENODEVICE and not h.value
        return
    assert rc == nat.VS_OK
    try:
        q = ref.sparse_queries(2, V, seed=1, nnz=4)
        out = np.full((2, n + 3), 7.0, F32)
        assert nat.lib().vs_index_set_scores(h, _p(q), nat.VS_F32, V, 2, None, 0, 0, 0, _p(out), n + 3, None) == nat.VS_OK, nat.last_error()
        assert ref.same(out[:, :n], ref.set_scores(ref.scores(q, ip, ix, v))) and (out[:, n:] == 7.0).all()
    finally:
        nat.lib().vs_index_destroy(h)


def test_host_checks_under_a_host_sanitizer(tmp_path):
    """set_score_check.h (the plan rule, and every argument check of vs_index_set_scores -- those against an index's shape included, which no
    handle-less machine reaches through the C ABI) in a stand-alone program built with the host compiler under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "set_score_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "set_score_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "set_score_check: ok" in run.stdout, run.stdout + run.stderr


# ---- the facade's argument errors, before any device work -------------------------------------------------------------------------------------
def test_facade_argument_errors_need_no_device():
    from vsearch_amd.ir import SCORE, SparseIndex
    from vsearch_amd.ir.retriever import index as index_mod
    assert repr(SCORE) == "SCORE" and SCORE is index_mod.SCORE and not isinstance(SCORE, str)
    idx = SparseIndex()
    edges = [0.0, 1.0]
    calls = [lambda **k: idx.value_stats(SCORE, **k), lambda **k: idx.histogram(SCORE, edges, **k), lambda **k: idx.percentiles(SCORE, [50], **k),
             lambda **k: idx.median(SCORE, **k), lambda **k: idx.top_by_value(SCORE, 3, **k), lambda **k: idx.stats_by_facet(SCORE, "cat", **k),
             lambda **k: idx.histogram_by_facet(SCORE, "cat", edges, **k), lambda **k: idx.set_scores(None, **k)]
    for call in calls:
        with pytest.raises(ValueError, match="q_embs"):
            call()
        with pytest.raises(ValueError, match="q_embs"):
            call(min_score=0.5)
    q = torch.zeros(1, 6)
    with pytest.raises(ValueError, match="score_scratch"):
        idx.value_stats(SCORE, q_embs=q, score_scratch=0)
    with pytest.raises(ValueError, match="ascending"):
        idx.histogram(SCORE, [1.0, 1.0], q_embs=q)
    with pytest.raises(ValueError):
        idx.top_by_value(SCORE, 0, q_embs=q)
    with pytest.raises(ValueError):
        idx.percentiles(SCORE, [101], q_embs=q)
    # SCORE is no reserved name: a stored field may be called "_score" or "SCORE", and a missing one is still a KeyError
    for name in ("_score", "SCORE"):
        with pytest.raises(KeyError, match="no value field"):
            idx.value_stats(name)
    # the chunk knob
    for bad in (100, -64, 1.5, True):
        with pytest.raises(ValueError, match="rows_per_chunk"):
            di._set_scores(None, np.zeros((1, 4), F32), None, bad)
    with pytest.raises(ValueError, match=r"\[B, V\]"):
        di._set_scores(None, np.zeros(4, F32), None, 0)
