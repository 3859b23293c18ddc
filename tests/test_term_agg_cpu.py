"""CPU checks of the term aggregations: the numpy reference against a plain double loop, the contract's corner cases, the
shard rule, the top-n reference on cases small enough to work out by hand, the plan rule (vs_term_plan is pure host arithmetic), the argument
errors of the C ABI without a GPU, the facade's host logic, and the host-side checks (vsearch_amd/csrc/term_agg_check.h) run in a stand-alone
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

import _term_agg_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_COLS = nat.TERM_LDS_COLS
F32 = np.float32


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit0", [0, 1, 31, 32, 33])
@pytest.mark.parametrize("with_live", [False, True])
def test_reference_equals_the_double_loop(bit0, with_live):
    n, V, B = 45, 13, 3
    rng = np.random.default_rng(bit0 + 7 * with_live)
    lens = rng.integers(0, V + 1, size=n)
    lens[:3] = (0, 1, V)                                                  # an empty row, one cell, every column
    ip, ix, va = ref.csr_case(lens, V, seed=bit0, zeros=0.2)
    masks = rng.random((B, n)) < 0.6
    words = ref.pack(masks, bit0, spare=1)                                # (every bit outside the rows set: it must not count)
    live = ref.pack(rng.random((1, n)) < 0.7, 0, spare=1)[0] if with_live else None
    has = ref.has_matrix(ip, ix, va, V)
    got = ref.term_counts(words, words.shape[1], bit0, has, live)
    want = ref.term_counts_loop(words, words.shape[1], bit0, ip, ix, va, V, live)
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and (g == w).all()
    assert (got[0] <= got[1][:, None]).all() and (got[0] > 0).any()
    if not with_live:
        assert (got[1] == masks.sum(axis=1)).all()


def test_stored_zeros_and_the_padding_column_do_not_count():
    V = 6
    ip = np.array([0, 4, 6, 6], dtype=np.int64)
    ix = np.array([0, 2, 3, V, 2, 5], dtype=np.int32)                     # row 0 carries the padding id V
    va = np.array([1.0, 0.0, -0.0, 9.0, 0.5, np.nan], dtype=F32)          # +0.0 and -0.0 are zero; NaN is not
    has = ref.has_matrix(ip, ix, va, V)
    assert has.astype(int).tolist() == [[1, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 1], [0] * 6]
    counts, total = ref.term_counts(None, 0, 0, has)
    assert counts.tolist() == [[1, 0, 1, 0, 0, 1]] and total.tolist() == [3]
    binary = ref.has_matrix(ip, ix, None, V)                              # a binary index: every stored cell counts, the padding still does not
    assert binary.sum() == 5 and binary[0].astype(int).tolist() == [1, 0, 1, 1, 0, 0]
    half = ref.has_matrix(ip, ix, va.astype(np.float16), V)               # an fp16 store widens exactly
    assert (half == has).all()
    loop = ref.term_counts_loop(ref.pack(np.ones((1, 3), bool)), 1, 0, ip, ix, va, V)
    assert loop[0].tolist() == counts.tolist()


@pytest.mark.parametrize("cut", [1, 31, 32, 33])
def test_shard_rule_counts_over_row_ranges_sum_to_the_whole(cut):
    """every shard counts its own rows, reading them from bit `row0` of the global bitmap, and its own live bitmap from bit 0"""
    n, V, B = 150, 17, 4
    rng = np.random.default_rng(cut)
    ip, ix, va = ref.csr_case(rng.integers(0, 9, size=n), V, seed=cut, zeros=0.1)
    has = ref.has_matrix(ip, ix, va, V)
    masks = rng.random((B, n)) < 0.7
    alive = rng.random(n) < 0.8
    words = ref.pack(masks)
    whole = ref.term_counts(words, words.shape[1], 0, has, ref.pack(alive[None, :])[0])
    bounds = [0, cut, cut + 64 + cut, n]
    parts = [ref.term_counts(words, words.shape[1], r0, has[r0:r1], ref.pack(alive[None, r0:r1])[0]) for r0, r1 in zip(bounds[:-1], bounds[1:])]
    for i in range(2):
        assert (sum(p[i] for p in parts) == whole[i]).all()
    ids = np.stack([rng.integers(-1, n, size=20) for _ in range(B)]).astype(np.int64)
    whole_ids = ref.term_counts_ids(ids, 0, has, alive)
    parts = [ref.term_counts_ids(ids, r0, has[r0:r1], alive[r0:r1]) for r0, r1 in zip(bounds[:-1], bounds[1:])]
    for i in range(2):
        assert (sum(p[i] for p in parts) == whole_ids[i]).all()


def test_reference_id_lists():
    has = np.eye(4, dtype=bool)
    has[3, 0] = True
    live = np.array([True, True, False, True])
    counts, total = ref.term_counts_ids(np.array([[0, 0, -1, 3, 2, 9, -7]]), 0, has, live)
    assert total.tolist() == [3] and counts.tolist() == [[3, 0, 0, 1]]           # 0 twice, 3 once; -1, the deleted 2 and the outsiders skipped
    counts, total = ref.term_counts_ids(np.array([[10, 13, 9]]), 10, has)
    assert total.tolist() == [2] and counts.tolist() == [[2, 0, 0, 1]]


# ---- the top-n of the reference ------------------------------------------------------------------------------------------------------------
def test_topn_order_and_ties_are_decided_by_the_column():
    #          col:  0   1   2   3   4   5
    fg = np.array([[4, 2, 4, 1, 0, 2]])
    bg = np.array([8, 4, 8, 1, 5, 4])
    cols, sc, f, g = ref.topn(fg, [4], bg, 16, 6, ref.LIFT)
    # lift = (fg / 4) / (bg / 16): 2, 2, 2, 4, -, 2  ->  3 first, then the four-way tie by column
    assert cols.tolist() == [[3, 0, 1, 2, 5, -1]] and sc[0, :5].tolist() == [4.0, 2.0, 2.0, 2.0, 2.0] and np.isneginf(sc[0, 5])
    assert f.tolist() == [[1, 4, 2, 4, 2, 0]] and g.tolist() == [[1, 8, 4, 8, 4, 0]]
    assert cols.dtype == np.int32 and sc.dtype == F32 and f.dtype == np.int64 and g.dtype == np.int64
    assert ref.topn(fg, [4], bg, 16, 2, ref.LIFT)[0].tolist() == [[3, 0]]        # n cuts inside the tie: the smallest column
    # two fp64 scores that differ but round to the same fp32: the column decides
    fg2, bg2 = np.array([[3, 3]]), np.array([(1 << 40) + 1, 1 << 40])
    cand, s = ref.scores(fg2[0], 3, bg2, 1 << 41, ref.LIFT)
    assert s[0] == s[1] and ((1 << 41) / ((1 << 40) + 1)) != 2.0
    assert ref.topn(fg2, [3], bg2, 1 << 41, 2, ref.LIFT)[0].tolist() == [[0, 1]]


def test_topn_jlh_excludes_what_is_not_over_represented():
    fg = np.array([[2, 1, 4, 3]])
    bg = np.array([8, 4, 4, 16])
    # total 4, bg_total 16: fgp = .5 .25 1 .75, bgp = .5 .25 .25 1: columns 0, 1 (fgp == bgp) and 3 (fgp < bgp) are no candidates
    cols, sc, _, _ = ref.topn(fg, [4], bg, 16, 4, ref.JLH)
    assert cols.tolist() == [[2, -1, -1, -1]] and sc[0, 0] == F32((1 - 0.25) * (1 / 0.25))
    assert ref.topn(fg, [4], bg, 16, 4, ref.LIFT)[0].tolist() == [[2, 0, 1, 3]]  # lift lists them: 4, 1, 1, 0.75


def test_topn_floors_and_empty_inputs():
    fg = np.array([[5, 1, 3, 0], [0, 0, 0, 0]])
    bg = np.array([5, 1, 0, 7])
    total = [5, 0]
    cols = ref.topn(fg, total, bg, 10, 3, ref.LIFT)[0]
    assert cols.tolist() == [[0, 1, -1], [-1, -1, -1]]                            # bg = 0 is skipped; total = 0 lists nothing
    assert ref.topn(fg, total, bg, 10, 3, ref.LIFT, min_count=2)[0].tolist() == [[0, -1, -1], [-1, -1, -1]]
    assert ref.topn(fg, total, bg, 10, 3, ref.LIFT, min_count=-4)[0].tolist() == cols.tolist()      # min_count below 1 is 1
    assert (ref.topn(fg, total, bg, 0, 3, ref.LIFT)[0] == -1).all()              # bg_total = 0 lists nothing
    out = ref.topn(fg[:1], total[:1], bg, 10, 9, ref.LIFT)                        # n > n_cols
    assert out[0].tolist() == [[0, 1] + [-1] * 7] and np.isneginf(out[1][0, 2:]).all() and (out[2][0, 2:] == 0).all() and (out[3][0, 2:] == 0).all()


# ---- the plan rule ---------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_constants():
    text = open(os.path.join(REPO, "include", "vsearch_hip.h")).read()
    get = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert get("VS_TERM_LDS_COLS") == nat.TERM_LDS_COLS >= 29523
    assert nat.TERM_LDS_COLS * 4 + 1024 <= 160 * 1024                             # the bins and the counters fit a CU's LDS
    assert get("VS_TERM_MAX_TOPN") == nat.TERM_MAX_TOPN == ref.MAX_TOPN == di.MAX_TERM_TOPN
    assert get("VS_TERM_LIFT") == nat.TERM_LIFT == ref.LIFT and get("VS_TERM_JLH") == nat.TERM_JLH == ref.JLH


def test_plan_regime_switches_behind_the_lds_columns():
    for V, regime in ((1, 0), (29523, 0), (LDS_COLS, 0), (LDS_COLS + 1, 1), (65535, 1)):
        assert di.term_plan(10_000, 9, V, True)[0] == regime, V
        assert di.term_plan(10_000, 1, V, False)[0] == regime, V


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 2049, 10_000, 1_000_000, 21_000_000, (1 << 32) - 1])
@pytest.mark.parametrize("B,V", [(1, 1), (9, 29523), (64, LDS_COLS), (64, 65535)])
def test_plan_chunks_cover_the_rows(n_rows, B, V):
    for rpc_in in (0, 64, 2048, 1 << 20):
        if rpc_in and -(-n_rows // rpc_in) * B > 0x7FFFFFFF:                        # more work items than one grid holds
            with pytest.raises(ValueError, match="too many"):
                di.term_plan(n_rows, B, V, True, rpc_in)
            continue
        regime, chunks, rpc = di.term_plan(n_rows, B, V, True, rpc_in)
        assert rpc > 0 and rpc % 64 == 0
        assert chunks * rpc >= n_rows > (chunks - 1) * rpc
        if rpc_in:
            assert rpc == rpc_in                                                   # an explicit value is taken as given
        else:
            assert rpc % 2048 == 0 and B * chunks <= max(1024, B)                  # a few workgroups per CU over the batch
        assert regime == (1 if V > LDS_COLS else 0)


def test_plan_argument_errors():
    for args in [(0, 1, 4, True, 0), (1 << 32, 1, 4, True, 0), (100, 0, 4, True, 0), (100, 1, 0, True, 0), (100, 1, 65536, True, 0),
                 (100, 1, 4, True, 100), (100, 1, 4, True, -64), (100, 2, 4, False, 0)]:
        with pytest.raises(ValueError):
            di.term_plan(*args)
    out32, out64 = C.c_int32(0), C.c_int64(0)
    assert nat.lib().vs_term_plan(100, 1, 4, 1, 0, None, C.byref(out64), C.byref(out64)) == nat.VS_EINVAL
    assert nat.lib().vs_term_plan(100, 1, 4, 1, 0, C.byref(out32), C.byref(out64), C.byref(out64)) == nat.VS_OK


# ---- argument errors of the C ABI, checked before the device is touched ----------------------------------------------------------------------
def test_index_calls_refuse_a_null_handle_without_a_device():
    counts, total, ids = np.zeros((1, 4), np.int64), np.zeros(1, np.int64), np.zeros((1, 3), np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert nat.lib().vs_index_term_counts(None, None, 0, 0, 1, 0, p(counts), 4, p(total), None) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert nat.lib().vs_index_term_counts_ids(None, p(ids), 1, 3, 3, 0, 1, p(counts), 4, p(total), None) == nat.VS_EINVAL
    assert "NULL" in nat.last_error()


def test_topn_argument_errors_without_a_device(have_gpu):
    good = nat.VS_OK if have_gpu else nat.VS_ENODEVICE
    counts, total, bg = np.ones((2, 6), np.int64), np.full(2, 3, np.int64), np.full(6, 2, np.int64)

    def call(n=3, V=6, ld=6, B=2, method=nat.TERM_JLH, null=()):
        outs = dict(cols=np.zeros((2, max(n, 1)), np.int32), score=np.zeros((2, max(n, 1)), F32), fg=np.zeros((2, max(n, 1)), np.int64),
                    bg_out=np.zeros((2, max(n, 1)), np.int64))
        p = {k: C.c_void_p(v.ctypes.data) for k, v in dict(counts=counts, total=total, bg=bg, **outs).items()}
        for k in null:
            p[k] = None
        return nat.lib().vs_term_topn(p["counts"], ld, p["total"], B, V, p["bg"], 12, method, n, 1, p["cols"], p["score"], p["fg"], p["bg_out"], 0, None)
    assert call() == good
    assert call(method=nat.TERM_LIFT) == good
    assert call(n=nat.TERM_MAX_TOPN + 1) == nat.VS_EINVAL and "1024" in nat.last_error()
    assert call(n=0) == nat.VS_EINVAL
    assert call(V=0) == nat.VS_EINVAL
    assert call(ld=5) == nat.VS_EINVAL and "ld_counts" in nat.last_error()
    assert call(B=0) == nat.VS_EINVAL
    assert call(method=2) == nat.VS_EINVAL and "method" in nat.last_error()
    for k in ("counts", "total", "bg", "cols", "score", "fg", "bg_out"):
        assert call(null=(k,)) == nat.VS_EINVAL and "NULL" in nat.last_error()


# ---- the facade's host logic -----------------------------------------------------------------------------------------------------------------
def test_facade_validation_needs_no_device():
    from vsearch_amd.ir import SparseIndex
    from vsearch_amd.ir.retriever.retriever import Retriever
    assert di._term_topn_args(20, "jlh", 1) == (20, "jlh", 1) and di._term_topn_args(np.int64(1), "count", 0)[1] == "count"
    for bad in (dict(topn=0), dict(topn=1025), dict(method="pmi"), dict(method=None)):
        with pytest.raises(ValueError):
            di._term_topn_args(**{"topn": 5, "method": "jlh", "min_count": 1, **bad})
    for bad in (dict(topn=2.0), dict(topn=True), dict(min_count="1")):
        with pytest.raises(TypeError):
            di._term_topn_args(**{"topn": 5, "method": "jlh", "min_count": 1, **bad})
    counts = np.ones((2, 6), np.int64)
    with pytest.raises(ValueError, match="count"):
        di.term_topn(counts, np.ones(2, np.int64), np.ones(6, np.int64), 4, 3, "count")
    with pytest.raises(ValueError, match="bg"):
        di.term_topn(counts, np.ones(2, np.int64), np.ones(5, np.int64), 4, 3, "lift")
    assert di._term_ids([1, 2, 3]).shape == (1, 3) and di._term_ids(torch.zeros(2, 4, dtype=torch.int64)).shape == (2, 4)
    with pytest.raises(TypeError, match="int64"):
        di._term_ids(np.zeros((2, 3), np.int32))
    with pytest.raises(ValueError):
        di._term_ids(np.zeros((2, 0), np.int64))
    idx = SparseIndex()
    with pytest.raises(ValueError, match="method"):
        idx.significant_terms(method="tfidf")
    with pytest.raises(ValueError, match="go together"):
        idx.term_counts(q_embs=torch.zeros(1, 6))
    with pytest.raises(ValueError, match="go together"):
        idx.significant_terms(min_score=0.5)
    with pytest.raises(ValueError, match="ids name the set"):
        idx.term_counts(filter=torch.ones(3, dtype=torch.bool), ids=torch.zeros(1, 2, dtype=torch.int64))
    # the retriever: exactly one of min_score and k, a known method -- checked before anything else is touched
    for kwargs in (dict(), dict(min_score=0.5, k=3)):
        with pytest.raises(ValueError, match="exactly one"):
            Retriever.significant_terms(None, ["q"], **kwargs)
    with pytest.raises(ValueError, match="method"):
        Retriever.significant_terms(None, ["q"], k=3, method="pmi")


# ---- the host-side checks under the host sanitizers ------------------------------------------------------------------------------------------
def test_host_checks_under_a_host_sanitizer(tmp_path):
    """term_agg_check.h (the plan rule, every limit of the three calls, and what vs_index_term_counts_ids checks in a host id list before it
    stages it) in a stand-alone program built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "term_agg_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "term_agg_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "term_agg_check: ok" in run.stdout, run.stdout + run.stderr
