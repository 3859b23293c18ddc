"""CPU tests of diversified search: the numpy contract (tests/_mmr_ref.py) on a worked example and on its stated properties, the proof that
the GPU tests' inputs have exact sums (so that bits may be compared whatever order the kernel sums in), the generic-values case's margin
cap, the argument checks that need no device, and the host-side checks of vs_mmr_select_csr under a host sanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, V

import _mmr_ref as ref

F32 = np.float32


def _csr(rows, n_cols=8):
    """[(cols, vals), ...] -> (indptr, indices, values)"""
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(c) for c, _ in rows], out=indptr[1:])
    cols = np.array([x for c, _ in rows for x in c], dtype=np.int32)
    vals = np.array([x for _, v in rows for x in v], dtype=F32)
    return indptr, cols, vals


def _one(rows, scores, lam, k, mode="cosine", ids=None, n_cols=8):
    ids = np.arange(len(rows), dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    out = ref.select_one(ids, np.asarray(scores, dtype=F32), *_csr(rows), n_cols, lam, k, mode)
    return dict(zip(ref.NAMES, out))


# Worked example.  Four candidates over 8 columns, scores 4, 3, 2, 1:
#   r0 = {0: 1, 1: 1}    r1 = r0 (an identical row)    r2 = {2: 2} (orthogonal to r0)    r3 = {0: 1, 2: 1}
#   g(0,0) = g(1,1) = 2, g(2,2) = 4, g(3,3) = 2;  g(0,1) = 2, g(0,2) = 0, g(0,3) = 1, g(2,1) = 0, g(2,3) = 2
# cosine, lam = mu = 0.5:  rel = 1, 0.75, 0.5, 0.25
#   step 0: val = 0.5 rel = 0.5, 0.375, 0.25, 0.125                           -> pick 0 (mmr 0.5, pen 0)
#           sim(0, .) = 2 / sqrt(2 * 2) = 1;  0;  1 / sqrt(2 * 2) = 0.5         pen = -, 1, 0, 0.5
#   step 1: val = 0.375 - 0.5 = -0.125;  0.25 - 0 = 0.25;  0.125 - 0.25 = -0.125    -> pick 2 (mmr 0.25, pen 0)
#           sim(2, 1) = 0;  sim(2, 3) = 2 / sqrt(4 * 2) = 0.70710678...           pen = -, 1, -, 0.70710678
#   step 2: val = -0.125;  0.125 - fl32(0.5 * 0.70710678) = -0.22855339        -> pick 1 (mmr -0.125, pen 1)
# lam = 1: val = rel - 0 * pen -> 0, 1, 2 (the prefix).
EXAMPLE = [((0, 1), (1, 1)), ((0, 1), (1, 1)), ((2,), (2,)), ((0, 2), (1, 1))]


def test_worked_example():
    got = _one(EXAMPLE, [4, 3, 2, 1], 0.5, 3)
    assert got["pos"].tolist() == [0, 2, 1] and got["ids"].tolist() == [0, 2, 1]
    assert got["scores"].tolist() == [4, 2, 3]
    assert got["mmr"].tolist() == [0.5, 0.25, -0.125] and got["pen"].tolist() == [0, 0, 1]
    four = _one(EXAMPLE, [4, 3, 2, 1], 0.5, 4)
    s23 = F32(np.float64(2) / np.sqrt(np.float64(8)))
    assert four["pos"].tolist() == [0, 2, 1, 3] and four["pen"][3] == s23 and four["mmr"][3] == F32(0.125) - F32(0.5) * s23
    assert _one(EXAMPLE, [4, 3, 2, 1], 1.0, 3)["pos"].tolist() == [0, 1, 2]
    dot = _one(EXAMPLE, [4, 3, 2, 1], 0.5, 3, "dot")                            # rel = s, sim = g: 2; 1.5 - 1 = 0.5, 1 - 0 = 1, 0.5 - 0.5 = 0
    assert dot["pos"].tolist() == [0, 2, 1] and dot["mmr"].tolist() == [2, 1, 0.5] and dot["pen"].tolist() == [0, 0, 2]


def test_lam_one_is_the_prefix_and_k_beyond_n_pads():
    c = ref.kernel_case(17, V, 3)
    for mode in ("cosine", "dot"):
        got = ref.select(c["ids"], c["scores"], c["indptr"], c["indices"], c["values"], V, 1.0, 20, mode)
        assert (got["ids"][:, :17] == c["ids"]).all() and (got["pos"][:, :17] == np.arange(17)).all()
        assert (got["scores"][:, :17].view(np.uint32) == c["scores"].view(np.uint32)).all()
        assert (got["ids"][:, 17:] == -1).all() and (got["pos"][:, 17:] == -1).all() and (got["pen"][:, 17:] == 0).all()
        assert np.isneginf(got["scores"][:, 17:]).all() and np.isneginf(got["mmr"][:, 17:]).all()


def test_padding_ends_a_list():
    none = _one(EXAMPLE, [4, 3, 2, 1], 0.5, 2, ids=[-1, -1, -1, -1])
    assert none["ids"].tolist() == [-1, -1] and none["pos"].tolist() == [-1, -1] and none["pen"].tolist() == [0, 0]
    assert np.isneginf(none["scores"]).all() and np.isneginf(none["mmr"]).all()
    mid = _one(EXAMPLE, [4, 3, 2, 1], 0.5, 4, ids=[9, 8, -1, 7])                # what follows the first -1 is ignored
    assert mid["ids"].tolist() == [9, 8, -1, -1] and mid["pos"].tolist() == [0, 1, -1, -1]


def test_empty_row_is_similar_to_nothing():
    rows = [((0, 1), (1, 1)), ((), ()), ((0, 1), (1, 1))]
    for mode in ("cosine", "dot"):
        got = _one(rows, [3, 2, 1], 0.5, 3, mode)
        assert got["pos"].tolist() == [0, 1, 2] and got["pen"].tolist()[:2] == [0, 0] and got["pen"][2] > 0
    first = _one([((), ()), ((0,), (1,)), ((0,), (1,))], [3, 2, 1], 0.25, 3)     # an empty first pick penalises nobody
    assert first["pos"].tolist() == [0, 1, 2] and first["pen"].tolist() == [0, 0, 1]


def test_ties_go_to_the_lower_position():
    rows = [((0,), (1,)), ((1,), (1,)), ((2,), (1,)), ((1,), (1,))]
    got = _one(rows, [2, 1, 1, 1], 0.5, 4)                                      # 1 and 2 tie at every step they are both in; 3 is 1's twin
    assert got["pos"].tolist() == [0, 1, 2, 3]
    got = _one(rows, [0, -0.0, 0, 0], 1.0, 4, "dot")                            # -0.0 equals 0.0
    assert got["pos"].tolist() == [0, 1, 2, 3]


def test_cosine_with_a_non_positive_best_score_uses_raw_scores():
    rows = EXAMPLE[:3]
    for s in ([0, -1, -2], [-1, -2, -4]):
        got = _one(rows, s, 0.5, 3)
        raw = _one(rows, s, 0.5, 3, "dot")
        assert got["mmr"][0] == F32(0.5) * F32(s[0]) == raw["mmr"][0]
        assert got["pen"].max() <= 1                                            # (the similarities are still cosines)


def test_lam_per_query():
    c = ref.kernel_case(16, V, 5)
    lam = np.array([0.0, 0.3, 1.0], dtype=F32)
    both = ref.select(c["ids"], c["scores"], c["indptr"], c["indices"], c["values"], V, lam, 16)
    for b in range(3):
        one = ref.select_one(c["ids"][b], c["scores"][b], c["indptr"][b * 16:(b + 1) * 16 + 1], c["indices"], c["values"], V, lam[b], 16)
        ref.assert_equal_bits({n: both[n][b] for n in ref.NAMES}, dict(zip(ref.NAMES, one)), b)
    assert (both["pos"][2] == np.arange(16)).all() and not (both["pos"][0] == np.arange(16)).all()


def test_identical_rows_have_cosine_one():
    c = ref.kernel_case(65, V, 9)
    rp, ix, va = c["indptr"][:66], c["indices"], c["values"]
    diag = ref.row_norms(rp, ix, va)
    for p in (0, 5, 64):
        g = ref.row_products(p, rp, ix, va, V)
        assert g[p] == diag[p]
        if diag[p] > 0:
            assert ref.similarity(g, diag[p], diag, "cosine")[p] == 1


def test_the_generator_is_exact():
    """every g of exact_rows equals integer arithmetic on the m's, rounded once -- in whatever order it is summed"""
    rng = np.random.default_rng(1)
    u = ref.universe(rng, V)
    lengths = list(ref.ROW_LENGTHS) * 3 + [2048, 2048, 768]
    for binary in (False, True):
        indptr, indices, values, m = ref.exact_rows(rng, lengths, u, binary)
        n = len(lengths)
        assert (np.diff(indptr) == lengths).all() and indices.min() >= 0 and indices.max() < V
        for r in range(n):
            assert (np.diff(indices[indptr[r]:indptr[r + 1]]) > 0).all()         # columns distinct, ascending
        assert m.min() >= 1 and m.max() <= 768 and (values == (m / 256).astype(F32)).all() and ((values * 256) == m).all()
        M = np.zeros((n, V), dtype=np.int64)
        M[np.repeat(np.arange(n), lengths), indices] = m
        G = M @ M.T                                                             # exact: entries below 2048 * 768^2 < 2^31
        assert int(G.max()) < 2 ** 31 and 768 * 768 < 2 ** 20
        want = np.array([[F32(int(G[i, j]) / 65536) for j in range(n)] for i in range(n)])
        for p in range(n):
            assert (ref.row_products(p, indptr, indices, values, V).view(np.uint32) == want[p].view(np.uint32)).all(), p
        assert (ref.row_norms(indptr, indices, values).view(np.uint32) == np.diag(want).copy().view(np.uint32)).all()
        order = rng.permutation(indptr[-1])                                     # the fp64 sum of the fp32 products, in another order
        p = n - 1
        img = np.zeros(V, dtype=F32)
        img[indices[indptr[p]:indptr[p + 1]]] = values[indptr[p]:indptr[p + 1]]
        prod = (img[indices] * values)[order]
        row_of = np.repeat(np.arange(n), lengths)[order]
        assert (np.bincount(row_of, weights=prod.astype(np.float64), minlength=n).astype(F32).view(np.uint32) == want[p].view(np.uint32)).all()


def test_kernel_cases_use_every_row_length():
    for kk in (15, 300, 1024):
        c = ref.kernel_case(kk, V, kk)
        assert set(np.diff(c["indptr"]).tolist()) == set(ref.ROW_LENGTHS)
        assert (np.diff(c["scores"], axis=1) <= 0).all() and {0, V - 1} <= set(c["indices"].tolist())


def test_generic_case_leaves_out_at_most_a_tenth_of_the_steps():
    c = ref.generic_case()
    traces = []
    ref.select(c["ids"], c["scores"], c["indptr"], c["indices"], c["values"], c["n_cols"], c["lam"], c["k"], traces=traces)
    clear = ref.generic_clear_steps(traces)
    assert clear.shape == (8, 2) and (~clear).mean() <= 0.10


def test_argument_checks_need_no_device():
    from vsearch_amd.device_index import MAX_MMR_DEPTH, _diverse_args, _lam_array
    assert MAX_MMR_DEPTH == 1024
    assert _diverse_args(10, None, "cosine") == (10, None, 0) and _diverse_args(np.int64(5), 1024, "dot") == (5, 1024, 1)
    with pytest.raises(ValueError, match="smaller than k"):
        _diverse_args(10, 9)
    with pytest.raises(ValueError, match="1024"):
        _diverse_args(10, 1025)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            _diverse_args(bad)
    with pytest.raises(TypeError):
        _diverse_args(2.5)
    with pytest.raises(ValueError, match="sim"):
        _diverse_args(3, None, "jaccard")
    assert _lam_array(0.5, 3).tolist() == [0.5] * 3 and _lam_array(1, 2).dtype == F32
    assert _lam_array([0, 0.25, 1], 3).tolist() == [0, 0.25, 1]
    for bad in (1.5, -0.1, float("nan"), [0.5, 2.0]):
        with pytest.raises(ValueError):
            _lam_array(bad, 2)
    with pytest.raises(ValueError):
        _lam_array([0.5, 0.5, 0.5], 2)
    with pytest.raises(TypeError):
        _lam_array("half", 2)


def test_host_checks_under_a_host_sanitizer(tmp_path):
    """mmr_check.h (sizes, rowptr, columns, lam: what vs_mmr_select_csr checks before it stages host arrays) in a stand-alone program
    built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "mmr_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "mmr_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "mmr_check: ok" in run.stdout, run.stdout + run.stderr
