"""CPU tests of range search: the numpy reference (tests/_range_ref.py) against a plain Python loop, the shard rule against the unsharded
reference, and the parts of the interface that need no device."""
import numpy as np
import pytest

import _range_ref as ref
from vsearch_amd import _native as nat

F32 = np.float32


def _small_case(seed, store):
    rng = np.random.default_rng(seed)
    n, V, B = int(rng.integers(1, 70)), 40, 3
    ip, ix, va = ref.csr_case(n, V, seed, max_nnz=6, empty_every=4)
    q = ref.sparse_queries(B, V, seed + 1, nnz=10)
    q[1] = -q[1]                                                         # a query of negative weights: negative scores, and -0.0 nowhere
    return n, B, q, ip, ix, va


@pytest.mark.parametrize("store", ["fp32", "fp16", "bin"])
def test_scores_equal_the_plain_loop(store):
    for seed in range(4):
        n, B, q, ip, ix, va = _small_case(seed, store)
        got, want = ref.scores(q, ip, ix, va, store), ref.scores_loop(q, ip, ix, va, store)
        assert (got.view(np.uint32) == want.view(np.uint32)).all()
        assert (got[:, np.diff(ip) == 0].view(np.uint32) == 0).all()    # an empty row scores +0.0


def test_reference_equals_the_plain_loop():
    for seed in range(12):
        n, B, q, ip, ix, va = _small_case(seed, "fp32")
        S = ref.scores(q, ip, ix, va)
        rng = np.random.default_rng(100 + seed)
        live = rng.random(n) < 0.8                                       # deleted rows
        per_q = rng.random((B, n)) < 0.7                                 # a per-query filter
        tie = S[0, rng.integers(n)]                                      # a threshold that is a row's score
        thrs = [-np.inf, np.inf, 0.0, -0.0, F32(tie), np.array([tie, 0.0, -np.inf], F32), np.array([np.nan, 0.5, -1.0], F32)]
        for thr in thrs:
            for allowed in (None, live, per_q & live):
                for max_hits in (0, 1, 5, n + 3):
                    got, want = ref.search(S, thr, max_hits, allowed), ref.search_loop(S, thr, max_hits, allowed)
                    ref.assert_equal_bits(got, want, (seed, thr, max_hits))
                    assert (got["counts"] == ref.unpack_bits(got["words"], n).sum(axis=1)).all()
                    if max_hits >= n:
                        assert ((got["ids"] >= 0).sum(axis=1) == got["counts"]).all()


def test_signed_zeros_and_infinities():
    S = np.array([[0.0, -0.0, 1.0, -1.0, 0.0]], dtype=F32)
    for thr in (0.0, -0.0):
        r = ref.search(S, thr, 5)
        assert r["counts"][0] == 4 and r["ids"][0].tolist() == [2, 0, 1, 4, -1]   # +0.0 and -0.0 tie: the id decides
    assert ref.search(S, -np.inf, 5)["counts"][0] == 5
    assert ref.search(S, np.inf, 5)["counts"][0] == 0 and (ref.search(S, np.inf, 5)["ids"] == -1).all()
    assert ref.search(S, np.nan, 5)["counts"][0] == 0
    assert ref.search(S, -np.inf, 5, allowed=np.array([1, 0, 1, 0, 1], bool))["counts"][0] == 3


def test_shard_rule_equals_the_unsharded_reference():
    for seed in range(6):
        rng = np.random.default_rng(seed)
        n, B = 150, 4
        ip, ix, va = ref.csr_case(n, 40, seed, max_nnz=6)
        S = ref.scores(ref.sparse_queries(B, 40, seed + 50, nnz=10), ip, ix, va)
        allowed = rng.random((B, n)) < 0.8
        bounds = [0, 33, 97, n]
        for thr in (-np.inf, 0.0, F32(np.median(S)), np.inf):
            for max_hits in (1, 7, 64, 200):
                whole = ref.search(S, thr, max_hits, allowed)
                parts = [ref.search(S[:, a:b], thr, max_hits, allowed[:, a:b], id_offset=a) for a, b in zip(bounds, bounds[1:])]
                got = ref.merge_shards(parts, max_hits)
                ref.assert_equal_bits(got, whole, (seed, thr, max_hits), ("ids", "scores", "counts"))
                words = np.concatenate([ref.unpack_bits(p["words"], b - a) for p, (a, b) in zip(parts, zip(bounds, bounds[1:]))], axis=1)
                assert (ref.pack_bits(words) == whole["words"]).all()


def test_symbol_and_methods_exist():
    assert "vs_index_search_range" in nat.EXPORTED_SYMBOLS and "vs_index_last_range_plan" in nat.EXPORTED_SYMBOLS
    assert nat.RANGE_MAX_HITS == ref.MAX_HITS == 2048
    from vsearch_amd.device_index import DeviceIndex, RangeResults, ShardGroup
    from vsearch_amd.ir.retriever.index import Index
    from vsearch_amd.ir.retriever.retriever import Retriever
    for cls in (DeviceIndex, ShardGroup, Index):
        for name in ("search_range", "count_matches", "match_filter"):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(Retriever.retrieve_range)
    assert RangeResults._fields == ("ids", "scores", "counts")


def test_argument_errors_come_before_any_device_call(monkeypatch):
    from vsearch_amd import device_index as di

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(nat, "lib", no_device)
    monkeypatch.setattr(nat, "require_device", no_device)
    q = np.zeros((3, 16), dtype=F32)
    dev = object.__new__(di.DeviceIndex)                                 # no handle: nothing below may reach it
    grp = object.__new__(di.ShardGroup)
    for obj in (dev, grp):
        with pytest.raises(ValueError, match="max_hits"):
            obj.search_range(q, 0.5, max_hits=-1)
        with pytest.raises(ValueError, match="2048"):
            obj.search_range(q, 0.5, max_hits=2049)
        with pytest.raises(ValueError, match="NaN"):
            obj.search_range(q, float("nan"))
        with pytest.raises(ValueError, match="NaN"):
            obj.count_matches(q, np.array([0.1, np.nan, 0.2], F32))
        with pytest.raises(ValueError, match="one per query"):
            obj.search_range(q, np.zeros(4, F32))
        with pytest.raises(ValueError, match="one per query"):
            obj.count_matches(q, [0.1, 0.2])
        with pytest.raises(ValueError, match="NaN"):
            obj.match_filter(q, float("nan"))
        with pytest.raises(TypeError, match="max_hits"):
            obj.search_range(q, 0.5, max_hits=2.5)
        with pytest.raises(ValueError, match=r"\[B, V\]"):
            obj.search_range(q[0], 0.5)
    B, thr, K = di._range_args(q, [0.1, -np.inf, np.inf], 2048)
    assert (B, K) == (3, 2048) and thr.dtype == F32 and thr.tolist() == [F32(0.1), -np.inf, np.inf]
