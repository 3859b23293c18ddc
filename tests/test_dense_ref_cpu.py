"""The references of tests/_dense_ref.py pinned to brute force at tiny sizes, and the shape tables of tests/test_gpu_dense_edges.py
checked against the launch-plan mirror at 256 CUs (an MI355X): every listed shape reaches the branch it is listed for.  No GPU needed."""
import itertools

import numpy as np
import pytest
import torch

import _dense_ref as ref

CU = 256


# ---- helpers against brute force ---------------------------------------------------------------------------------------------------
def test_scores64_is_the_plain_sum_of_products():
    mat, q = ref.dyadic_np(1, 9, 3, 13)
    want = np.array([[sum(float(a) * float(b) for a, b in zip(qr, mr)) for mr in mat] for qr in q])
    assert (ref.scores64(q, mat) == want).all()
    t = ref.scores64(torch.from_numpy(q), torch.from_numpy(mat), block_bytes=8 * 13 * 2)          # two rows a block
    assert t.dtype == torch.float64 and (t.numpy() == want).all()
    assert (ref.exact32(q, mat) == want.astype(np.float32)).all()


def test_exact32_holds_no_negative_zero():
    q = np.array([[-1.0, -0.5]], dtype=np.float32)
    mat = np.zeros((2, 2), dtype=np.float32)                                      # every product is -0.0; a sum that starts at +0.0 is +0.0
    assert not np.signbit(ref.exact32(q, mat)).any()
    assert not np.signbit(ref.exact32(q[:, :1], mat[:, :1])).any()                # (one term: a matmul may return the bare product)
    assert not torch.signbit(ref.exact32(torch.from_numpy(q), torch.from_numpy(mat))).any()


@pytest.mark.parametrize("as_torch", [False, True])
def test_canonical_topk_against_a_python_sort(as_torch):
    rng = np.random.default_rng(2)
    s = rng.integers(-3, 4, size=(4, 37)).astype(np.float32) / 2                  # many ties, both signs
    s[0, 5], s[0, 9] = -0.0, 0.0
    allowed = rng.random((4, 37)) < 0.3
    allowed[3] = False
    for k, al in itertools.product((1, 7, 37), (None, allowed[1], allowed)):
        arg = (torch.from_numpy(s), k, None if al is None else torch.from_numpy(al)) if as_torch else (s, k, al)
        ids, sc = (np.asarray(x) for x in ref.canonical_topk(*arg))
        for b in range(4):
            ok = np.ones(37, bool) if al is None else (al if al.ndim == 1 else al[b])
            order = sorted((i for i in range(37) if ok[i]), key=lambda i: (-float(s[b, i]), i))[:k]
            want_ids = order + [-1] * (k - len(order))
            want_sc = [s[b, i] for i in order] + [-np.inf] * (k - len(order))
            assert ids[b].tolist() == want_ids
            assert (sc[b] == np.array(want_sc, dtype=np.float32)).all()


def test_round_f16_ties_and_subnormals():
    x = np.array([2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -26, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2049.0, -(2.0 ** -25)], dtype=np.float32)
    want = np.array([0.0, 2.0 ** -24, 0.0, 1.0, 1 + 2.0 ** -9, 2048.0, -0.0], dtype=np.float32)
    got = ref.round_f16(x)
    assert got.dtype == np.float32 and (got == want).all() and np.signbit(got[-1])


def test_nonzeros_csr_drops_negative_zero_and_keeps_nan():
    m = np.array([[0.0, -0.0, 2.0, np.nan], [0.0, 0.0, 0.0, -0.0], [-1.0, 0.0, 0.0, 3.0]], dtype=np.float32)
    ip, ix, d = ref.nonzeros_csr(m)
    assert ip.tolist() == [0, 2, 2, 4] and ix.tolist() == [2, 3, 0, 3]
    assert d[0] == 2 and np.isnan(d[1]) and d[2:].tolist() == [-1.0, 3.0]
    t = torch.from_numpy(np.nan_to_num(m, nan=5.0)).to_sparse_csr()
    assert t.crow_indices().tolist() == ip.tolist() and t.col_indices().tolist() == ix.tolist()


def test_err_bound_formula():
    q = np.array([[1.0, -2.0, 0.5]], dtype=np.float32)
    mat = np.array([[-1.0, 1.0, 4.0]], dtype=np.float32)
    assert ref.err_bound(q, mat, ldp=32)[0, 0] == (2 * 32 + 1 + 2) * 2.0 ** -24 * 5.0
    assert ref.err_bound(q, mat, ldp=1120)[0, 0] == (2 * 512 + 3 + 2) * 2.0 ** -24 * 5.0
    assert ref.err_bound(q, mat, nnz_row=3)[0, 0] == 8 * 2.0 ** -24 * 5.0


def test_dyadic_laws_sum_exactly():
    """the widest V any dyadic GPU case uses, in the worst order fp32 can meet: every partial sum is a multiple of 1/8 below 2^24 / 8"""
    widest = max([c[0] for c in ref.QUARTER_CASES + ref.main_quarter_cases(CU) + ref.split_cases(CU)] + [ref.fallback_cases(CU)[0], 65_536])
    assert ref.dyadic_ok(widest)
    mat, q = ref.dyadic_np(3, 4, 4, 2049)
    assert (np.abs(q) @ mat.T).max() * 8 < 2 ** 24
    assert (np.cumsum((q[:, None, :] * mat[None]).astype(np.float32), axis=2, dtype=np.float32)[..., -1] == ref.exact32(q, mat)).all()


def test_pool_ref_is_elu1p_of_the_max():
    rng = np.random.default_rng(4)
    h = rng.integers(-4, 4, size=(2, 5, 8)).astype(np.float32) / 2
    W = rng.integers(-8, 8, size=(3, 8)).astype(np.float32) / 4
    m, out = ref.pool_ref(h, W)
    want = torch.nn.functional.elu(torch.from_numpy(h).double() @ torch.from_numpy(W).double().t()).add(1).max(1)[0]
    assert np.allclose(out, want.numpy(), rtol=1e-15, atol=0)
    assert (m == (torch.from_numpy(h).double() @ torch.from_numpy(W).double().t()).max(1)[0].numpy()).all()


# ---- the plan mirror -----------------------------------------------------------------------------------------------------------------
def test_plan_of_the_shapes_the_suite_already_runs():
    """dense.hip's own comment (100 000 x 29 523, B = 256: 14 of 782 document tiles left after three rounds) and the two big shapes of
    tests/test_gpu_search.py"""
    p = ref.dense_plan(100_000, 256, 29_523, CU)
    assert (p.main_doc_tiles, ref.ceil_div(p.n_tail, 128), p.kind) == (768, 14, "split")
    p = ref.dense_plan(66_000, 130, 2048, CU)
    assert (p.main_doc_tiles, p.n_tail, p.kind, p.S, p.cps) == (512, 464, "split", 4, 16)
    p = ref.dense_plan(66_236, 256, 2048, CU)
    assert (p.main_doc_tiles, p.kind) == (512, "split")
    for N in (2000, 512, 9000):
        assert ref.dense_plan(N, 8, 96, CU).kind == "quarter" and ref.dense_plan(N, 8, 96, CU).main_doc_tiles == 0


def test_plan_invariants():
    rng = np.random.default_rng(6)
    shapes = [(int(rng.integers(1, 200_000)), int(rng.integers(1, 600)), int(rng.integers(1, 40_000)), int(rng.choice([8, 104, 256, 304])))
              for _ in range(3000)]
    shapes += [(N, B, V, CU) for N, B, V in itertools.product((1, 127, 128, 65_531, 65_536, 65_537, 131_072), (1, 128, 129), (1, 992, 993, 8200))]
    for N, B, V, cu in shapes:
        p = ref.dense_plan(N, B, V, cu)
        assert p.n_begin + p.n_tail == N and p.n_begin % 128 == 0 and p.n_begin == p.main_doc_tiles * 128
        assert (p.kind == "none") == (p.n_tail == 0)
        assert 1 <= p.bs_max <= B and p.bs_max * N * 8 <= max(ref.SLICE_BYTES, N * 8)
        if p.kind == "split":
            assert p.cps % 16 == 0 and p.S >= 2 and p.main_doc_tiles > 0 and p.ws_bytes <= ref.WS_LIMIT
            assert (p.S - 1) * p.cps < p.chunks <= p.S * p.cps                        # every slice has work, the slices cover K
            assert ref.ceil_div(p.n_tail, 128) * ref.ceil_div(B, 128) * p.S <= 2 * cu  # ... in the idle slots of one round
        else:
            assert p.S < 2 or p.main_doc_tiles == 0 or p.ws_bytes > ref.WS_LIMIT or p.kind == "none"


# ---- the shape tables of the GPU file, at 256 CUs -----------------------------------------------------------------------------------
def test_quarter_cases_cover_their_lists_and_stay_quarter():
    for axis, values in ((0, (1, 31, 32, 33, 511, 512, 513, 1055)), (1, (1, 127, 128, 129, 300)), (2, (1, 31, 32, 33, 129))):
        seen = [c[axis] for c in ref.QUARTER_CASES]
        assert set(seen) == set(values) and all(seen.count(v) >= 2 for v in values)
    for V, N, B in ref.QUARTER_CASES:
        p = ref.dense_plan(N, B, V, CU)
        assert (p.main_doc_tiles, p.kind, p.n_tail) == (0, "quarter", N)


def test_main_quarter_cases_reach_the_main_kernel_and_the_quarter_tail():
    cases = ref.main_quarter_cases(CU)
    assert {c[0] for c in cases} == {1, 33, 96, 513, 992} and {c[1] for c in cases} == {1, 127, 128, 129, 257}
    assert {c[4] for c in cases} == {0, 1, 127, 129} and {c[3] for c in cases} == {1, 2}
    for V, B, N, rounds, r in cases:
        p = ref.dense_plan(N, B, V, CU)
        q_tiles = ref.ceil_div(B, 128)
        assert p.main_doc_tiles == rounds * 2 * CU // q_tiles and N % 128 == r % 128, (V, B, N)
        assert p.kind == ("none" if p.n_tail == 0 else "quarter") and (p.n_tail == 0) == (r == 0 and (2 * CU) % q_tiles == 0), (V, B, N)
        assert p.n_tail in (r, 128), (V, B, N)
    assert ref.n_after_rounds(1, 128, CU, 1) == 65_537 and ref.n_after_rounds(2, 129, CU, 0) == 65_536


def test_clamp_cases_need_the_clamp():
    assert ref.clamp_cases(CU)[0] == (96, 128, 65_531)
    for (V, B, N), kind in zip(ref.clamp_cases(CU), ("quarter", "split")):
        doc_tiles, q_tiles = ref.ceil_div(N, 128), ref.ceil_div(B, 128)
        assert (doc_tiles * q_tiles) % (2 * CU) == 0 and N % 128 != 0             # the full rounds cover every tile, the last one partial
        p = ref.dense_plan(N, B, V, CU)
        assert (p.main_doc_tiles, p.n_tail, p.kind) == (N // 128, N % 128, kind)


def test_split_cases_split_with_the_listed_slices():
    cases = ref.split_cases(CU)
    assert {c[0] for c in cases} == {993, 1024, 1100, 2049} and {c[1] for c in cases} == {1, 130} and {c[3] for c in cases} == {1, 200}
    want = {993: (32, 2, 16, 2, 16), 1024: (32, 2, 16, 2, 16), 1100: (35, 2, 32, 3, 3), 2049: (65, 3, 32, 5, 1)}
    for V, B, N, r, host in cases:
        p = ref.dense_plan(N, B, V, CU)
        assert p.kind == "split" and p.n_tail == r and p.main_doc_tiles == 2 * CU // ref.ceil_div(B, 128), (V, B, N)
        last = p.chunks - (p.S - 1) * p.cps
        assert (p.chunks, p.S, p.cps, p.n_sum_blocks, last) == want[V], (V, B, N)
        if host:
            assert ((256 << 20) // (V * 4)) < N                                   # vs_index_create_dense uploads it in more than one chunk
    assert sum(c[4] for c in cases) == 1
    V, n_main, n_copy = ref.invariance_case(CU)
    for B in (128, 256):
        p = ref.dense_plan(n_main + n_copy, B, V, CU)
        assert (p.n_begin, p.n_tail, p.kind) == (n_main, n_copy, "split")


def test_fallback_cases_straddle_the_workspace_limit():
    V, B, n_over, n_under = ref.fallback_cases(CU)
    assert (V, B, n_over - 65_536) == (8200, 128, 30_848)
    over, under = ref.dense_plan(n_over, B, V, CU), ref.dense_plan(n_under, B, V, CU)
    assert over.kind == "quarter" and over.S >= 2 and over.main_doc_tiles > 0 and over.ws_bytes > ref.WS_LIMIT
    assert under.kind == "split" and under.ws_bytes <= ref.WS_LIMIT < under.ws_bytes + under.n_sum_blocks * B * 128 * 4
    assert n_over * ref.ldp_of(V) * 4 < 3.5e9                                     # matrix + index + an fp64 block stay under ~8 GB


def test_select_and_slice_cases():
    assert ref.SELECT_ABOVE in ref.SELECT_N and ref.SELECT_ABOVE + 1 in ref.SELECT_N
    N, B, V = ref.slice_case()
    p = ref.dense_plan(N, B, V, CU)
    assert B * N * 8 > ref.SLICE_BYTES and 1 < p.bs_max < B and B - p.bs_max < p.bs_max       # two slices, the second one short
    assert p.bs_max == 1917


def test_pool_cases_cover_their_lists():
    assert {c[0] for c in ref.POOL_CASES} == set(ref.POOL_L)
    for L in ref.POOL_L:
        mine = [c for c in ref.POOL_CASES if c[0] == L]
        assert {c[1] for c in mine} == {1, 3} and {c[2] for c in mine} == {32, 96}
    assert {c[3] for c in ref.POOL_CASES} == {1, 127, 129}


@pytest.mark.parametrize("n_cols", ref.AUTO_COLS + (65_536,))
def test_auto_matrix_has_the_rows_it_lists(n_cols):
    m = ref.auto_matrix(n_cols)
    nz = m != 0
    assert not nz[0].any() and not nz[-1].any() and not nz[7].any() and nz[1].all()
    assert np.flatnonzero(nz[2]).tolist() == [0] and np.flatnonzero(nz[3]).tolist() == [n_cols - 1]
    assert np.flatnonzero(nz[4]).tolist() == sorted({0, n_cols - 1})
    for edge in range(1024, n_cols + 1, 1024):
        assert nz[5, edge - 1] and (edge == n_cols or nz[5, edge])
    assert np.signbit(m[6][~nz[6]]).all() and nz[6].sum() == min(n_cols, 5) - 1
    mn = ref.auto_matrix(n_cols, nan=True)
    assert np.isnan(mn).sum() == 1 and (np.nan_to_num(mn, nan=0.0) == m).all()
    ip, ix, d = ref.nonzeros_csr(mn)
    assert ip[-1] == nz.sum() + 1 and np.isnan(d).sum() == 1
