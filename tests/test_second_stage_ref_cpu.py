"""The numpy references of tests/_second_stage_ref.py, pinned on the CPU: to the C oracle (merge), to torch's bmm + topk (rerank, the
reference's retriever.py:137-147 restated in oracle/torch_ref.py style), to torch.topk(...).values.mean(1) (mean pooling), and to
themselves where the GPU tests rely on exact sums.  No GPU needed."""
import numpy as np
import pytest
import torch

import oracle
from oracle import compare
import _second_stage_ref as ref


@pytest.mark.parametrize("law", ref.MERGE_LAWS)
@pytest.mark.parametrize("n_cand,k", [(100, 100), (101, 100), (4097, 128), (6145, 129), (8192, 2048), (16384, 1)])
def test_merge_ref_equals_the_c_oracle(law, n_cand, k):
    """(no dropped ids here: the oracle has no drop rule)"""
    rng = np.random.default_rng(n_cand * 31 + k)
    ids = ref.merge_ids(rng, 3, n_cand)
    sc = ref.merge_scores(rng, law, 3, n_cand, k)
    got = ref.merge_topk_ref(ids, sc, k)
    want = oracle.merge_topk(ids, sc, k)
    assert (got[0] == want[0]).all() and (ref.bits32(got[1]) == ref.bits32(want[1])).all()


def test_merge_laws_are_what_they_say():
    rng = np.random.default_rng(5)
    n, k = 6145, 129
    assert np.unique(ref.merge_scores(rng, "few", 2, n, k)).size <= 8
    tf = ref.merge_scores(rng, "tiefree", 2, n, k)
    assert all(np.unique(r).size == n for r in tf)
    for law, sl in (("winners_last", slice(n - k, n)), ("winners_first", slice(0, k))):
        sc = ref.merge_scores(rng, law, 2, n, k)
        for r in sc:
            assert set(np.argsort(-r, kind="stable")[:k]) <= set(range(n)[sl])
    sc = ref.merge_scores(rng, "winners_last", 2, n, 1)
    assert (np.argmax(sc, axis=1) >= n - 100).all()
    runs = ref.merge_scores(rng, "runs8", 2, n, k)
    for part in np.array_split(np.arange(n), 8):
        assert (np.diff(runs[:, part], axis=1) <= 0).all()
    ids = ref.merge_ids(rng, 2, n)
    assert all(np.unique(r).size == n and r.min() == 0 and r.max() == ref.ID_LIMIT - 1 for r in ids)


def test_merge_ref_drops_pads_and_ties_signed_zeros():
    ids = np.array([[5, -1, 2 ** 32 - 1, 2 ** 32, 2 ** 40, 2 ** 32 - 2, 3, 4]], dtype=np.int64)
    sc = np.array([[0.0, 9, 9, 9, 9, -0.0, -0.0, 1.0]], dtype=np.float32)
    got_ids, got_sc = ref.merge_topk_ref(ids, sc, 6)
    assert got_ids.tolist() == [[4, 3, 5, 2 ** 32 - 2, -1, -1]]
    assert ref.bits32(got_sc).tolist() == ref.bits32(np.array([[1.0, 0.0, 0.0, 0.0, -np.inf, -np.inf]], dtype=np.float32)).tolist()


def test_rerank_topk_ref_order_rules():
    sc = np.array([[-np.inf, 0.0, -0.0, 2.0, -np.inf, 2.0, np.inf]], dtype=np.float32)
    ids = np.array([[-1, 10, 11, 12, -1, 13, 14]], dtype=np.int64) + 0
    got_ids, got_sc = ref.rerank_topk_ref(sc, ids)
    assert got_ids.tolist() == [[14, 12, 13, 10, 11, -1, -1]]
    assert ref.bits32(got_sc).tolist() == ref.bits32(np.array([[np.inf, 2, 2, 0.0, 0.0, -np.inf, -np.inf]], dtype=np.float32)).tolist()


@pytest.mark.parametrize("V", [5, 773, 4099])
def test_rerank_refs_match_torch_bmm_topk(V):
    """retriever.py:137-147: p_emb.view(B, k, V) bmm q.unsqueeze(2), topk(k) -- tie-free inputs, the project's 1e-4 score parity"""
    rng = np.random.default_rng(V)
    B, k = 4, 16
    # non-negative like the encoder's elu1p activations: no cancellation, so a relative bound on the scores means something
    p = np.abs(ref.sparse_randn(rng, (B * k, V), 0.0 if V < 100 else 0.97))
    q = np.abs(rng.standard_normal((B, V))).astype(np.float32)
    ids = np.stack([rng.permutation(1000)[:k] for _ in range(B)]).astype(np.int64)
    sc = ref.rerank_scores_ref(p, q, k).exact32.reshape(B, k)
    assert all(np.unique(r).size == k for r in sc)
    got_ids, got_sc = ref.rerank_topk_ref(sc, ids)
    t_sc = torch.bmm(torch.from_numpy(p).view(B, k, V), torch.from_numpy(q).unsqueeze(2)).squeeze(2)
    top = t_sc.topk(k, dim=1)
    want_ids = torch.gather(torch.from_numpy(ids), 1, top.indices).numpy()
    compare.compare_topk(want_ids, top.values.numpy(), got_ids, got_sc, rtol=1e-4)


def test_rerank_scores_ref_streams_and_masks():
    rng = np.random.default_rng(2)
    B, k, V = 3, 5, 37
    p = ref.dyadic_signed(rng, (B * k, V))
    q = ref.dyadic_signed(rng, (B, V))
    full = ref.rerank_scores_ref(p, q, k)
    part = ref.rerank_scores_ref(p[7:12], q, k, row0=7)
    assert (ref.bits32(part.exact32) == ref.bits32(full.exact32[7:12])).all()
    p2, q2 = p.copy(), q.copy()
    p2[:, 3] = 0.0
    p2[:, 4] = -0.0
    q2[0, 3], q2[1, 3], q2[2, 4] = np.inf, np.nan, -np.inf
    q0 = q2.copy()
    q0[:, 3:5] = 0.0
    a, b = ref.rerank_scores_ref(p2, q2, k), ref.rerank_scores_ref(p2, q0, k)
    assert (ref.bits32(a.exact32) == ref.bits32(b.exact32)).all() and (a.hi == b.hi).all()


@pytest.mark.parametrize("p_dtype", [np.float32, np.float16])
@pytest.mark.parametrize("V", ref.RERANK_WIDTHS)
def test_dyadic_inputs_sum_exactly(V, p_dtype):
    """The bit-exact GPU assertions rest on this: on the dyadic grid float32 products are exact and so is their float64 sum.
    These are the very arrays test_rerank_scores_dyadic_every_width_and_stride scores (ref.rerank_dyadic_case).  The other dyadic
    GPU rerank cases (the 40 x 1000-row grid-stride case, the special values) draw other arrays from the same law; for them
    exactness follows from the law itself -- products that are multiples of 2^-12 below 16, far fewer than 2^36 terms -- not from
    a run of those arrays here."""
    p, q, k = ref.rerank_dyadic_case(V, p_dtype)
    rng = np.random.default_rng(V)
    r = ref.rerank_scores_ref(p, q, k)
    assert (ref.bits32(r.exact32) == ref.bits32(r.hi.astype(np.float32))).all()
    assert (np.abs(r.hi) * 4096 == np.round(np.abs(r.hi) * 4096)).all()          # a whole number of 2^-12 units
    # any other summation order gives the same float64 sum
    perm = rng.permutation(V)
    r2 = ref.rerank_scores_ref(p[:, perm], q[:, perm], k)
    assert (r2.hi == r.hi).all() and (r2.abs_sum == r.abs_sum).all()


@pytest.mark.parametrize("t", [1, 2, 31, 32])
def test_pool_refs_match_torch(t):
    rng = np.random.default_rng(t)
    for L in sorted({t, t + 1, 33}):
        x = (rng.standard_normal((2, L, 67)) * 2).astype(np.float32)
        x[rng.random(x.shape) < 0.1] = -np.inf
        tx = torch.from_numpy(x).double()
        act = torch.where(tx > 0, tx + 1, torch.exp(tx))                         # elu1p (sparse.py:6)
        want = act.topk(t, dim=1).values.mean(1).numpy()
        # float64 throughout: sums of t <= 32 terms in two orders (rtol), and exp(x) against expm1(x) + 1, each within 2^-53
        # absolute of the true value where x <= 0 (atol)
        np.testing.assert_allclose(ref.mean_topk_ref(x, t), want, rtol=64 * 2.0 ** -53, atol=2.0 ** -52)
        np.testing.assert_allclose(ref.head_pool_ref(x), act.max(dim=1).values.numpy(), rtol=4 * 2.0 ** -53, atol=2.0 ** -52)
        for pattern in ref.POOL_PATTERNS:
            xd = ref.pool_logits_dyadic(rng, pattern, 2, L, 67)
            td = torch.from_numpy(xd).double()
            actd = torch.where(td > 0, td + 1, torch.exp(td))
            assert (ref.mean_topk_ref(xd, t) == actd.topk(t, dim=1).values.mean(1).numpy()).all(), (pattern, L)
            assert (ref.head_pool_ref(xd) == actd.max(dim=1).values.numpy()).all(), (pattern, L)
            # and exact in float32: every partial sum is a multiple of 1/8 below 2^24 / 8
            top = -np.sort(-ref._elu1p64(xd), axis=1)[:, :t]
            assert (np.cumsum(top.astype(np.float32), axis=1, dtype=np.float32) == np.cumsum(top, axis=1)).all()


def test_ulp_helpers():
    a = np.array([1.0, -1.0, 0.0, 1e-45], dtype=np.float32)
    assert ref.ulp_distance32(a, a).tolist() == [0, 0, 0, 0]
    assert ref.ulp_distance32(a, np.nextafter(a, np.float32(np.inf))).tolist() == [1, 1, 1, 1]
    assert ref.ulp_distance32(np.float32([0.0]), np.float32([-0.0])).tolist() == [0]
    assert ref.ulp32(np.array([1.0, 3.0]))[0] == 2.0 ** -23 and ref.ulp32(np.array([1.0, 3.0]))[1] == 2.0 ** -22
