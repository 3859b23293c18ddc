"""CPU checks of facet counts: the numpy reference against a plain double loop, the invariants of the contract, the
shard rule, the plan rule (vs_facet_plan is pure host arithmetic), the argument errors of the C ABI without a GPU, and the facade's host
logic.  No device is needed."""
import ctypes as C

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd import device_index as di

import _facet_ref as ref

BINS = nat.FACET_LDS_BINS


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit0", [0, 1, 31, 32, 33])
@pytest.mark.parametrize("with_and", [False, True])
def test_reference_equals_the_double_loop(bit0, with_and):
    n, L, B = 45, 5, 3
    rng = np.random.default_rng(bit0 + 7 * with_and)
    labels = ref.labels_case(n, L, seed=bit0, frac_none=0.2, frac_big=0.1)
    masks = rng.random((B, n)) < 0.6
    words = ref.pack(masks, bit0, spare=1)                          # (every bit outside the rows set: it must not count)
    aw = ref.pack(rng.random((1, n)) < 0.7, bit0, spare=1)[0] if with_and else None
    got = ref.facet_counts(words, words.shape[1], bit0, n, labels, L, aw)
    want = ref.facet_counts_loop(words, words.shape[1], bit0, n, labels, L, aw)
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and (g == w).all()
    assert (ref.unpack(words, bit0, n) == masks).all()
    counts, total, other = got
    assert (counts.sum(axis=1) + other == total).all()
    assert (other > 0).any() and (counts > 0).any()


def test_reference_null_bitmap_and_invariant():
    n, L = 200, 7
    labels = ref.labels_case(n, L, seed=3, frac_none=0.1, frac_big=0.1)
    counts, total, other = ref.facet_counts(None, 0, 0, n, labels, L)
    assert total.tolist() == [n] and counts.sum() + other[0] == n
    assert other[0] == int(((labels < 0) | (labels >= L)).sum())
    live = ref.pack(np.arange(n)[None, :] % 3 != 0)[0]
    c2, t2, o2 = ref.facet_counts(None, 0, 0, n, labels, L, live)
    assert t2[0] == int((np.arange(n) % 3 != 0).sum()) and c2.sum() + o2[0] == t2[0]


def test_reference_topn_order_ties_and_floor():
    counts = np.array([[3, 5, 0, 5, 3, 1, 5], [0, 0, 0, 0, 0, 0, 0]])
    lab, cnt = ref.topn(counts, 4)
    assert lab[0].tolist() == [1, 3, 6, 0] and cnt[0].tolist() == [5, 5, 5, 3]          # ties: label ascending
    assert lab[1].tolist() == [-1] * 4 and cnt[1].tolist() == [0] * 4                    # a zero count is never listed
    lab, cnt = ref.topn(counts, 9)                                                       # n > n_labels
    assert lab[0].tolist() == [1, 3, 6, 0, 4, 5, -1, -1, -1] and cnt[0].tolist() == [5, 5, 5, 3, 3, 1, 0, 0, 0]
    lab, cnt = ref.topn(counts, 9, min_count=3)                                          # the floor keeps the whole tie at 3
    assert lab[0].tolist() == [1, 3, 6, 0, 4, -1, -1, -1, -1]
    lab, cnt = ref.topn(counts, 2, min_count=0)                                          # min_count below 1 is 1
    assert lab[1].tolist() == [-1, -1]
    assert lab.dtype == np.int32 and cnt.dtype == np.int64


@pytest.mark.parametrize("cut", [1, 31, 32, 33])
def test_shard_rule_counts_at_bit_offsets_sum_to_the_whole(cut):
    """every shard counts its rows with its slice of the labels, reading its rows from bit `row0` of the global bitmap"""
    n, L, B = 150, 6, 4
    labels = ref.labels_case(n, L, seed=cut, frac_none=0.1)
    masks = ref.masks_case(B, n, seed=cut + 1, density=0.8)
    words = ref.pack(masks)
    whole = ref.facet_counts(words, words.shape[1], 0, n, labels, L)
    bounds = [0, cut, cut + 64 + cut, n]
    parts = [ref.facet_counts(words, words.shape[1], r0, r1 - r0, labels[r0:r1], L) for r0, r1 in zip(bounds[:-1], bounds[1:])]
    for i in range(3):
        assert (sum(p[i] for p in parts) == whole[i]).all()
    assert (ref.topn(sum(p[0] for p in parts), 3)[0] == ref.topn(whole[0], 3)[0]).all()


# ---- the plan rule ---------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_constants():
    import os
    import re
    from conftest import REPO
    text = open(os.path.join(REPO, "include", "vsearch_hip.h")).read()
    assert int(re.search(r"#define\s+VS_FACET_LDS_BINS\s+(\d+)", text).group(1)) == nat.FACET_LDS_BINS
    assert int(re.search(r"#define\s+VS_FACET_MAX_TOPN\s+(\d+)", text).group(1)) == nat.FACET_MAX_TOPN == ref.MAX_TOPN == di.MAX_FACET_TOPN


def test_plan_qt_steps_and_regime():
    n, B = 10_000, 9
    want = [(1, 8), (BINS // 8, 8), (BINS // 8 + 1, 4), (BINS // 4, 4), (BINS // 4 + 1, 2), (BINS // 2, 2), (BINS // 2 + 1, 1), (BINS, 1)]
    for L, qt in want:
        regime, got, chunks, rpc = di.facet_plan(n, B, L, True)
        assert (regime, got) == (0, qt), L
        assert got * L <= BINS
    regime, qt, _, _ = di.facet_plan(n, B, BINS + 1, True)
    assert regime == 1 and qt >= 1
    assert di.facet_plan(n, 1, BINS + 1, False)[:2] == (1, 1)
    for L in (1, 100, BINS // 8, BINS):                             # a shared bitmap: one query a workgroup
        assert di.facet_plan(n, 1, L, False)[:2] == (0, 1)


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 2049, 10_000, 1_000_000, 21_000_000, (1 << 32) - 1])
@pytest.mark.parametrize("B,L", [(1, 1), (9, 256), (64, 16384), (64, 1_000_000)])
def test_plan_chunks_cover_the_rows(n_rows, B, L):
    for rpc_in in (0, 64, 2048, 1 << 20):
        regime, qt, chunks, rpc = di.facet_plan(n_rows, B, L, True, rpc_in)
        assert rpc > 0 and rpc % 64 == 0
        assert chunks * rpc >= n_rows > (chunks - 1) * rpc
        if rpc_in:
            assert rpc == rpc_in                                    # an explicit value is taken as given
        assert regime == (1 if L > BINS else 0)


def test_plan_argument_errors():
    for args in [(0, 1, 4, True, 0), (1 << 32, 1, 4, True, 0), (100, 0, 4, True, 0), (100, 1, 0, True, 0), (100, 1, 4, True, 100),
                 (100, 1, 4, True, -64), (100, 2, 4, False, 0)]:
        with pytest.raises(ValueError):
            di.facet_plan(*args)
    out32, out64 = C.c_int32(0), C.c_int64(0)
    assert nat.lib().vs_facet_plan(100, 1, 4, 1, 0, None, C.byref(out32), C.byref(out64), C.byref(out64)) == nat.VS_EINVAL


# ---- argument errors of the C ABI, checked before the device is touched ----------------------------------------------------------------------
def _counts_call(n=100, B=1, L=4, ld_words=None, bit0=0, rpc=0, ld_counts=None, null=(), words=True):
    W = (bit0 + n + 31) // 32
    bufs = dict(words=np.zeros((max(B, 1), max(W, 1)), np.uint32), labels=np.zeros(max(n, 1), np.int32), counts=np.zeros((max(B, 1), max(ld_counts or L, 1)), np.int64),
                total=np.zeros(max(B, 1), np.int64), other=np.zeros(max(B, 1), np.int64))
    p = {k: (None if k in null or (k == "words" and not words) else C.c_void_p(v.ctypes.data)) for k, v in bufs.items()}
    return nat.lib().vs_facet_counts(p["words"], bit0, W if ld_words is None else ld_words, None, B, p["labels"], n, L, rpc, p["counts"],
                                     L if ld_counts is None else ld_counts, p["total"], p["other"], 0, None)


def test_counts_argument_errors_without_a_device(have_gpu):
    good = nat.VS_OK if have_gpu else nat.VS_ENODEVICE
    assert _counts_call() == good
    assert _counts_call(B=1, ld_words=0) == good                    # one bitmap for all queries
    assert _counts_call(words=False) == good                        # NULL words: every row set
    for name in ("labels", "counts", "total", "other"):
        assert _counts_call(null=(name,)) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert _counts_call(L=0) == nat.VS_EINVAL
    assert _counts_call(L=-3) == nat.VS_EINVAL
    assert _counts_call(rpc=100) == nat.VS_EINVAL and "64" in nat.last_error()
    assert _counts_call(rpc=-64) == nat.VS_EINVAL
    assert _counts_call(B=2, ld_words=0) == nat.VS_EINVAL
    assert _counts_call(n=100, bit0=31, ld_words=4) == nat.VS_EINVAL and "ld_words" in nat.last_error()    # 131 bits span 5 words
    assert _counts_call(n=100, bit0=31, ld_words=5) == good
    assert _counts_call(bit0=-1) == nat.VS_EINVAL
    assert _counts_call(n=0) == nat.VS_EINVAL
    assert _counts_call(B=0) == nat.VS_EINVAL
    assert nat.lib().vs_index_facet_counts(None, None, 0, 0, 1, None, 4, 0, None, 4, None, None, None) == nat.VS_EINVAL


def test_topn_argument_errors_without_a_device(have_gpu):
    good = nat.VS_OK if have_gpu else nat.VS_ENODEVICE
    counts = np.zeros((2, 6), np.int64)
    def call(n=3, L=6, ld=6, B=2, null=()):
        labels, out = np.zeros((2, max(n, 1)), np.int32), np.zeros((2, max(n, 1)), np.int64)
        p = dict(counts=C.c_void_p(counts.ctypes.data), labels=C.c_void_p(labels.ctypes.data), out=C.c_void_p(out.ctypes.data))
        for k in null:
            p[k] = None
        return nat.lib().vs_facet_topn(p["counts"], ld, B, L, n, 1, p["labels"], p["out"], 0, None)
    assert call() == good
    assert call(n=nat.FACET_MAX_TOPN + 1) == nat.VS_EINVAL
    assert call(n=0) == nat.VS_EINVAL
    assert call(L=0) == nat.VS_EINVAL
    assert call(ld=5) == nat.VS_EINVAL
    assert call(B=0) == nat.VS_EINVAL
    for k in ("counts", "labels", "out"):
        assert call(null=(k,)) == nat.VS_EINVAL
    with pytest.raises(ValueError, match="1024"):
        di.facet_topn(counts, 1025)
    with pytest.raises(TypeError):
        di.facet_topn(counts, 2.0)
    with pytest.raises(ValueError, match="n_labels"):
        di._facet_args(np.zeros(5, np.int32), 0, 5)
    with pytest.raises(ValueError, match="one entry per row"):
        di._facet_args(np.zeros(4, np.int32), 3, 5)
    with pytest.raises(TypeError, match="integer"):
        di._facet_args(np.zeros(5, np.float32), 3, 5)
    with pytest.raises(ValueError, match="64"):
        di._facet_args(np.zeros(5, np.int32), 3, 5, rows_per_chunk=96)


# ---- the facade's host logic ---------------------------------------------------------------------------------------------------------------------
def test_set_facet_validation_and_add_without_facets():
    from vsearch_amd.ir import SparseIndex
    idx = SparseIndex()
    assert idx.facet_fields == []
    with pytest.raises(TypeError):
        idx.set_facet(3, [0, 1])
    with pytest.raises(ValueError, match="groups"):
        idx.set_facet("groups", [0, 1])
    idx.set_facet("lang", None)                                     # removing a field that is not there is a no-op
    codes = SparseIndex._facet_codes
    assert codes([0, 2, -1], 3).dtype == torch.int32
    with pytest.raises(ValueError, match="-1"):
        codes([0, -2, 1], 3)
    with pytest.raises(TypeError, match="integer"):
        codes(np.array([0.5, 1.0]), 2)
    with pytest.raises(ValueError, match="entries"):
        codes([0, 1], 3)
    with pytest.raises(ValueError, match="1-D"):
        codes(np.zeros((2, 2), np.int64), 4)
    with pytest.raises(ValueError, match="31 bits"):
        codes(np.array([1 << 31]), 1)
    # an index with facet fields: add() / update() must give exactly these fields, and raise before anything changes
    idx._facets = {"lang": (torch.tensor([0, 1, 1], dtype=torch.int32), 2, ["de", "en"]), "year": (torch.tensor([5, 5, 7], dtype=torch.int32), 8, None)}
    assert idx.facet_fields == ["lang", "year"]
    vec = torch.eye(2, 6)
    before = {k: v[0].clone() for k, v in idx._facets.items()}
    for bad in (None, {"lang": [0, 1]}, {"lang": [0, 1], "year": [1, 2], "size": [0, 0]}):
        with pytest.raises(ValueError, match="facet fields"):
            idx.add(vec, facets=bad)
        with pytest.raises(ValueError, match="facet fields"):
            idx.update([0], vec, facets=bad)
    with pytest.raises(ValueError, match="no name"):
        idx.add(vec, facets={"lang": [0, 2], "year": [1, 2]})
    with pytest.raises(ValueError, match="entries"):
        idx.add(vec, facets={"lang": [0], "year": [1, 2]})
    assert all((idx._facets[k][0] == before[k]).all() and idx._facets[k][0].shape[0] == 3 for k in before)
    plain = SparseIndex()
    with pytest.raises(ValueError, match="no facet fields"):
        plain._added_facets({"lang": [0]}, 1)
    assert plain._added_facets(None, 1) is None
    with pytest.raises(ValueError, match="go together"):
        idx.facets("lang", q_embs=torch.zeros(1, 6))
    with pytest.raises(ValueError, match="1024"):
        idx.facets("lang", topn=5000)
