"""tests/_sparsify_ref.py -- the plain references the GPU tests of the encoder tail compare against -- pinned to independent sources on a
machine without a GPU: torch.topk (tie-free rows), Tensor.to_sparse_csr(), F.elu in float64, and the CPU oracle on inputs without
signed-zero ties or NaN (where the oracle's float comparison and the library's order keys agree).  Also: every seeded builder lands in
the kernel path it is there for, and the header states the contract the reference implements."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _sparsify_ref as ref
import oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_order_key_is_the_float_order_with_signed_zeros_and_nans_by_bit_pattern():
    vals = ref.from_bits([0xFFFFFFFF, 0xFFC00000, 0xFF800000, 0xC0000000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x3F800000,
                          0x7F800000, 0x7F800001, 0x7FFFFFFF])            # ascending in the selection order
    keys = ref.order_key(vals).astype(np.int64)
    assert (np.diff(keys) > 0).all()
    assert keys[0] == 0 and keys[-1] == 0xFFFFFFFF
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(4096) * 100).astype(np.float32)
    assert (np.argsort(ref.order_key(x), kind="stable") == np.argsort(x, kind="stable")).all()


@pytest.mark.parametrize("V,k", [(1, 1), (201, 7), (8193, 1), (8193, 4096), (8193, 8193), (32769, 768)])
def test_topk_mask_ref_against_torch_topk_on_tie_free_rows(V, k):
    rng = np.random.default_rng(V + k)
    x = np.stack([ref.distinct_values(rng, V), -np.abs(ref.distinct_values(rng, V, signed=False)), ref.distinct_values(rng, V)])
    want = torch.zeros(x.shape, dtype=torch.bool)
    want.scatter_(1, torch.topk(torch.from_numpy(x), k, dim=1).indices, True)
    assert (ref.topk_mask_ref(x, k) == want.numpy()).all()
    assert (ref.topk_mask_ref(x, k) == oracle.topk_mask(x, k)).all()


def test_topk_mask_ref_ties_go_to_the_lower_column_and_zeros_rank_by_sign():
    x = np.float32([[1, 2, 2, 2, 0], [5, 5, 5, 5, 5]])
    assert ref.topk_mask_ref(x, 2).tolist() == [[False, True, True, False, False], [True, True, False, False, False]]
    assert (ref.topk_mask_ref(x, 2) == oracle.topk_mask(x, 2)).all()
    # the contract's row: the order key ranks +0.0 above -0.0 (the float comparison of the oracle would take column 0)
    assert ref.topk_mask_ref(np.float32([[-0.0, 0.0, -1.0]]), 1).tolist() == [[False, True, False]]
    assert ref.topk_mask_ref(np.float32([[-0.0, 0.0, -0.0, 0.0, -1.0]]), 3).tolist() == [[True, True, False, True, False]]
    assert ref.topk_mask_ref(x, 0).sum() == 0


@pytest.mark.parametrize("shift", [0, 999])
@pytest.mark.parametrize("topk,lexical", [(1, True), (768, True), (768, False), (0, True), (-1, False), (3001, True)])
def test_embed_mask_ref_against_the_oracle(shift, topk, lexical):
    vocab = 3001 + shift
    rng = np.random.default_rng(topk + 7 * shift + 3)
    x = np.stack([ref.distinct_values(rng, 3001) for _ in range(5)])
    x[1] = np.abs(x[1])
    ids = ref.token_batch(x, vocab, shift, 40, seed=5)
    got = ref.embed_mask_ref(x, ids, vocab, shift, topk, lexical)
    want = oracle.embed_mask(x, ids, vocab, shift, None if topk < 0 else topk, lexical)
    assert (got == want.view(np.uint32)).all()
    if topk > 0 and not lexical:
        assert ((got & 0x7FFFFFFF) != 0).sum(axis=1).tolist() == [topk] * 5
    bow = ref.embed_mask_ref(x, ids, vocab, shift, topk, lexical, bow=True)
    assert (bow == oracle.embed_mask(x, ids, vocab, shift, topk, lexical, bow=True).view(np.uint32)).all()


@pytest.mark.parametrize("L", [1, 40, 1100])
@pytest.mark.parametrize("norm", [False, True])
def test_bow_mask_ref_against_the_oracle_and_torch(L, norm):
    vocab, shift = 5000, 999
    rng = np.random.default_rng(L)
    ids = rng.integers(0, vocab, size=(6, L))
    ids[0, :] = 5                                           # nothing at or above shift: an empty row (norm: 0 / 1e-12)
    ids[1, -1] = vocab - 1
    got = ref.bow_mask_ref(ids, vocab, shift, norm)
    np.testing.assert_allclose(got, oracle.bow_mask(ids, vocab, shift, norm), rtol=1e-6)
    t = torch.zeros(6, vocab, dtype=torch.float64).scatter_(1, torch.from_numpy(ids), 1.0)[:, shift:]
    if norm:
        t = F.normalize(t, dim=1)
    np.testing.assert_allclose(got, t.numpy(), rtol=1e-12)
    assert got[0].sum() == 0
    for bad in (-1, vocab):
        ids[3, L // 2] = bad
        with pytest.raises(ValueError):
            ref.bow_mask_ref(ids, vocab, shift, norm)


@pytest.mark.parametrize("B,V", [(3, 1), (3, 65), (1, 1025), (7, 300)])
def test_dense_to_csr_ref_against_to_sparse_csr(B, V):
    x = ref.dense_rows(B, V, seed=2)
    got = ref.dense_to_csr_ref(x)
    finite = np.where(np.isnan(x), np.float32(7), x)            # (to_sparse_csr keeps NaN too, but a NaN never equals itself below)
    t = torch.from_numpy(finite).to_sparse_csr()
    assert (got.rowptr == t.crow_indices().numpy()).all()
    assert (got.cols == t.col_indices().numpy()).all()
    assert (np.where(np.isnan(got.vals), np.float32(7), got.vals).view(np.uint32) == t.values().numpy().view(np.uint32)).all()
    assert B == 1 or got.rowptr[1] == 0                         # the row of signed zeros keeps nothing
    t_nan = torch.from_numpy(x).to_sparse_csr()                 # ... and with the NaNs in place the structure is the same
    assert (got.rowptr == t_nan.crow_indices().numpy()).all()
    kinds = got.vals.view(np.uint32)
    if B * V >= 2100:
        assert np.isnan(got.vals).any() and np.isinf(got.vals).any() and ((kinds & 0x7F800000) == 0).any(), "no NaN / inf / subnormal stored"


def test_masked_csr_ref_is_the_csr_of_the_masked_matrix_on_finite_input_and_drops_unselected_non_finite():
    rng = np.random.default_rng(3)
    x = np.stack([ref.distinct_values(rng, 500) for _ in range(4)])
    x[2, ::3] = 0.0
    x[3, ::2] = -0.0
    keep = ref.topk_mask_ref(x, 200)
    fused, two = ref.masked_csr_ref(x, keep), ref.two_call_csr_ref(x, keep)
    t = (torch.from_numpy(x) * torch.from_numpy(keep)).to_sparse_csr()
    for got in (fused, two):
        assert (got.rowptr == t.crow_indices().numpy()).all() and (got.cols == t.col_indices().numpy()).all()
        assert (got.vals.view(np.uint32) == t.values().numpy().view(np.uint32)).all()
    # the contract's row: an unselected inf / NaN -- the two-call path (and torch) store the NaN of x * 0, the fused call drops it
    y = np.float32([[3.0, -np.inf, 2.0, np.nan, 1.0, np.inf]])
    keep = ref.topk_mask_ref(y, 2)
    assert keep.tolist() == [[False, False, False, True, False, True]]             # +NaN's key is above +inf's
    keep = ref.topk_mask_ref(y, 1)
    assert keep.tolist() == [[False, False, False, True, False, False]]            # +NaN ranks first
    y = np.float32([[3.0, -np.inf, 2.0, 1.0, -np.inf]])
    keep = ref.topk_mask_ref(y, 2)
    fused, two = ref.masked_csr_ref(y, keep), ref.two_call_csr_ref(y, keep)
    assert fused.cols.tolist() == [0, 2] and fused.vals.tolist() == [3.0, 2.0]
    assert two.cols.tolist() == [0, 1, 2, 4] and np.isnan(two.vals[[1, 3]]).all()
    t = (torch.from_numpy(y) * torch.from_numpy(keep)).to_sparse_csr()
    assert two.cols.tolist() == t.col_indices().tolist()


def test_elu1p_and_head_pool_ref_against_torch_in_float64():
    x = ref.elu_input(5000, seed=4)
    want = (F.elu(torch.from_numpy(x).double()) + 1).numpy()
    got = ref.elu1p_ref(x)
    ok = (got == want) | (np.isnan(got) & np.isnan(want))
    assert ok.all() or np.allclose(got[~ok], want[~ok], rtol=1e-15, atol=0)
    e32, exact = ref.elu1p_exact(x)
    assert exact[:5].all() and e32[:4].tolist() == [1.0, 1.0, 0.0, np.inf] and np.isnan(e32[4])
    assert (e32[exact & ~np.isnan(x)].astype(np.float64) == want[exact & ~np.isnan(x)].astype(np.float32)).all()
    lg = ref.pool_logits(3, 4, 9, seed=1)
    m, p = ref.head_pool_ref(lg)
    t = (F.elu(torch.from_numpy(lg).double()) + 1).max(dim=1).values.numpy()
    np.testing.assert_allclose(p, t, rtol=1e-15)
    np.testing.assert_allclose(oracle.head_pool(lg), p, rtol=2e-7, atol=1.2e-7)
    assert (m[:, 0] == -np.inf).all() and (p[:, 0] == 0).all() and (p[:, 1] == 1).all() and (p[:, 3] == np.inf).all()
    lg1 = ref.pool_logits(2, 1, 5, seed=1)
    assert (ref.head_pool_ref(lg1)[0] == lg1[:, 0, :]).all()


# ---- the builders land in the paths they claim ---------------------------------------------------------------------------------------
def test_select_path_on_hand_made_rows():
    row = np.float32([4.0, 1.0, 1.0 + 2 ** -23, 1.0, -2.0, 8.0])
    assert ref.select_path(row, 6, 1) == (1, 1, 0xC100)          # 8.0 alone in its top half
    assert ref.select_path(row, 6, 3) == (3, 1, 0xBF80)          # the three keys of top half 0x3F80 | sign, one selected
    assert ref.select_path(row, 6, 5) == (3, 3, 0xBF80)
    assert ref.select_path(row, 4, 4) == (3, 3, 0xBF80)          # only the first V columns count
    assert ref.select_path(ref.from_bits([0x3F800000, 0xFFFFFFFF, 0xFFFF0001]), 3, 3) == (2, 2, 0)
    s = ref.select_paths(row[None], 4)
    assert (int(s.n_same[0]), int(s.r_same[0])) == (2, 1)        # 8, 4, 1 + ulp, then one of the two 1.0
    s = ref.select_paths(row[None], 5)
    assert (int(s.n_same[0]), int(s.r_same[0])) == (2, 2)
    assert ref.path_name(3, 3, 2, 2) == "take_all" and ref.path_name(129, 1, 1, 1) == "list_256" and ref.path_name(2049, 5, 9, 9) == "hist_all_eq"


def _cluster_paths(V, topk):
    x, names = ref.mask_rows(V, topk, seed=0)
    return x, names, dict(zip(names, ref.paths_of(x, topk))), ref.select_paths(x, topk)


def test_cluster_rows_reach_every_band_with_the_remaining_they_claim():
    V = 16385
    topk = V // 2
    x, names, paths, s = _cluster_paths(V, topk)
    row = {n: i for i, n in enumerate(names)}
    for m in ref.CLUSTER_M:
        band = "list_128" if m <= 128 else "list_256" if m <= 256 else "list_2048" if m <= 2048 else "hist_all_eq"      # (distinct values: one key equals the k-th)
        for rw in sorted({1, m - 1, m}):
            i = row[f"cluster_{m}_r{rw}"]
            assert (int(s.n_eq[i]), int(s.remaining[i]), int(s.P[i])) == (m, rw, 0xBF80), (m, rw)
            assert paths[names[i]][0] == ("take_all" if rw == m else band), (m, rw)
            assert ref.select_path(x[i], V, topk) == (m, rw, 0xBF80)
    for m in (2049, 5000):
        for n_lows in (2, 3):
            assert paths[f"cluster_{m}_lows{n_lows}_r1"][0] == "hist_bitmap"
            assert paths[f"cluster_{m}_lows{n_lows}_r{m - 1}"][0] == "hist_bitmap"
            assert paths[f"cluster_{m}_lows{n_lows}_rgroup"][0] == "hist_all_eq"
            i = row[f"cluster_{m}_lows{n_lows}_rgroup"]
            assert int(s.n_eq[i]) == m and 1 < int(s.n_same[i]) == int(s.r_same[i]) < m
    assert paths["one_value"][0] == "hist_bitmap" and int(s.n_eq[row["one_value"]]) == V
    assert paths["zeros_mixed"][0] in ("list_128", "take_all") and int(s.P[row["zeros_mixed"]]) in (0x8000, 0x7FFF)
    assert int(s.P[row["zeros_one_positive"]]) == 0x7FFF and int(s.remaining[row["zeros_one_positive"]]) == 2
    assert x.shape[0] % 4 == 0 and len(names) == x.shape[0]


@pytest.mark.parametrize("V", [8191, 32768, 32769])
def test_every_path_is_reached_at_a_width_over_its_topk_values(V):
    seen, p0 = set(), set()
    for topk in ref.mask_topks(V):
        x, names, paths, s = _cluster_paths(V, topk)
        seen |= {p for p, _ in paths.values()}
        p0 |= {(n, p) for n, (p, z) in paths.items() if z}
        zi = names.index("zeros_mixed")
        assert int(s.P[zi]) in (0x8000, 0x7FFF), "zeros do not form the threshold"
        if topk == V:
            assert paths["one_value"][0] == "take_all"
    assert seen == set(ref.PATHS)
    # P == 0: k-th key = a negative NaN of the highest payload bits -- alone (take_all) and ranked among three (the list)
    assert ("nan_lowest_one", "take_all") in p0 and ("nan_lowest_three", "list_128") in p0 and ("nan_lowest_three", "take_all") in p0
    assert ("nan_lowest_last_column", "list_128") in p0
    assert ("nan_lowest_many", "hist_all_eq") in p0 and ("nan_lowest_many", "take_all") in p0        # (topk = V / 2; topk = V: both)


def test_fused_topk_values_stay_inside_the_stage():
    for V in ref.MASK_WIDTHS[:-1]:
        for L in (0,) + ref.LEX_L:
            ks = ref.csr_topks(V, L)
            assert all(0 < k <= V and min(V, k + L) <= ref.MR_STAGE for k in ks), (V, L, ks)
            assert max(min(V, k + L) for k in ks) == min(V, ref.MR_STAGE)
        if V not in (8191, 8193, 16384, 30720, 32768):      # (the path coverage: one width per G and both sides of the stage; the GPU test
            continue                                        #  asserts it at every width it runs)
        seen = set()
        for topk in ref.csr_topks(V):
            x, _ = ref.mask_rows(V, topk, seed=0)
            seen |= set(ref.paths_of(x, topk))
        assert {p for p, _ in seen} == set(ref.PATHS), (V, seen)
        p0 = {p for p, zero in seen if zero}                    # P == 0 in the fused call: the histograms; the list and take_all too
        assert "hist_all_eq" in p0 and (V > ref.MR_STAGE or p0 >= {"take_all", "list_128"}), (V, p0)       # where topk reaches V


def test_geometry_mirrors():
    assert [ref.fast_g(V) for V in ref.MASK_WIDTHS[:-1]] == [4, 4, 8, 8, 8, 15, 15, 15, 16, 16, 16]
    assert ref.slow_max_v() == 36556 and ref.slow_lds_bytes(36556) == 160 * 1024
    src = open(os.path.join(REPO, "vsearch_amd", "csrc", "mask_rows_fast.h")).read()
    for line in ("constexpr int kMrCand = 2048;", "constexpr int kMrThreads = 512;", "constexpr int kMrCols = 32 * 1024;"):
        assert line in src, line
    assert ref.MR_STAGE == 2 * 256 * 32 // 2


def test_token_batch_holds_what_it_claims():
    shift, V = 999, 8193
    x, _ = ref.mask_rows(V, 2, seed=0)
    for L in ref.LEX_L:
        ids = ref.token_batch(x, V + shift, shift, L, seed=1)
        assert ids.shape == (x.shape[0], L) and ids.min() >= 0 and ids.max() == V + shift - 1
        lex = ref.lexical_mask_ref(ids, V + shift, shift)
        top = ref.topk_mask_ref(x, 1)
        assert (lex & top).any(), "no lexical column in the top-k"
        assert (lex & (x == 0)).any(), "no lexical column whose value is 0.0"
        assert (ids < shift).any(), "no token below shift"
        if L > 1:
            assert all(len(set(r)) < L for r in ids.tolist()), "no duplicate"
            assert (lex & top).any(axis=1).all()
        if L > 512:
            assert (lex & ~ref.topk_mask_ref(x, V - 1))[:, :].any(), "the token read in place adds nothing to the mask"


def test_the_header_states_the_contract_of_the_reference():
    text = " ".join(open(os.path.join(REPO, "include", "vsearch_hip.h")).read().split()).replace(" * ", " ")
    for phrase in ("+0.0 ranks above -0.0", "NaNs rank by bit pattern", "expects finite input",
                   "an unselected NaN or +-inf is dropped"):
        assert phrase in text, f"include/vsearch_hip.h no longer says: {phrase}"
    assert ref.topk_mask_ref(np.float32([[-0.0, 0.0, -1.0]]), 1).tolist() == [[False, True, False]]
