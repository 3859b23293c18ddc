"""Grouped search without a GPU: the numpy references agree with a plain Python loop, the round procedure of DESIGN.md 3.1f equals the
one-shot walk over the complete ranking (the exactness argument, executed), the end-to-end cases of tests/test_gpu_grouped.py have well
defined expected values, and the argument errors that need no device."""
import numpy as np
import pytest
import torch

import oracle
from conftest import V
from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, ShardGroup, _grouped_args, _search_grouped
from vsearch_amd.ir import Index, SparseIndex

import _grouped_ref as ref


def _python_walk(ids, scores, groups, k, m):
    """the contract as a dict-based loop over one ranked list"""
    opened, kept = [], {}
    for r, s in zip(ids, scores):
        if r < 0:
            break
        g = int(groups[r])
        if g in kept:
            if len(kept[g]) < m:
                kept[g].append((int(r), s))
        elif len(opened) < k:
            opened.append(g)
            kept[g] = [(int(r), s)]
    return opened, kept


def _same(a, b):
    return all((x == y).all() for x, y in ((a.group, b.group), (a.count, b.count), (a.ids, b.ids), (a.scores.view(np.uint32), b.scores.view(np.uint32))))


def test_symbols_and_signatures():
    for name in ("vs_topk_collapse", "vs_group_filter"):
        assert name in nat.EXPORTED_SYMBOLS
        assert hasattr(nat.lib(), name)
    for name in ("search_grouped",):
        assert hasattr(DeviceIndex, name) and hasattr(ShardGroup, name)
    for name in ("set_groups", "groups", "search_grouped", "groups_from_samples"):
        assert hasattr(Index, name)
    from vsearch_amd.ir import Retriever
    assert hasattr(Retriever, "retrieve_grouped")


def test_numpy_walk_equals_the_python_loop():
    rng = np.random.default_rng(0)
    for trial in range(60):
        n = int(rng.integers(5, 300))
        kk = int(rng.integers(1, n + 1))
        k, m = int(rng.integers(1, 12)), int(rng.integers(1, 5))
        groups = rng.integers(0, max(1, n // int(rng.integers(1, 9))), n).astype(np.int32)
        ids = rng.permutation(n)[:kk].astype(np.int64)
        sc = np.sort(rng.integers(0, 6, kk).astype(np.float32))[::-1].copy()      # ties in score
        if trial % 3 == 0 and kk > 2:
            cut = int(rng.integers(1, kk))
            ids[cut:] = -1
            sc[cut:] = -np.inf
        st = ref.State(1, k, m)
        left = ref.walk(st, ids[None], sc[None], groups)
        opened, kept = _python_walk(ids, sc, groups, k, m)
        assert st.group[0, :len(opened)].tolist() == opened and (st.group[0, len(opened):] == -1).all()
        for s, g in enumerate(opened):
            assert st.count[0, s] == len(kept[g])
            assert st.ids[0, s, :len(kept[g])].tolist() == [r for r, _ in kept[g]]
            assert st.scores[0, s, :len(kept[g])].tolist() == [x for _, x in kept[g]]
            assert (st.ids[0, s, len(kept[g]):] == -1).all() and np.isneginf(st.scores[0, s, len(kept[g]):]).all()
        complete = (ids < 0).any() or (len(opened) == k and all(len(kept[g]) == m for g in opened))
        assert left == (0 if complete else 1) and st.status[0] == int(complete)


@pytest.fixture(scope="module")
def scored():
    n, B = 1500, 6
    ip, ix, d = oracle.synth_csr(41, 0, n, V, 200)
    q = oracle.synth_queries(42, B)
    _, _, allsc = oracle.csr_search(ip, ix, d, V, q, 10, acc64=True, return_all=True)
    return np.asarray(allsc, dtype=np.float32)


@pytest.mark.parametrize("law", ["div8", "random", "giant", "singletons"])
@pytest.mark.parametrize("k,m", [(7, 1), (7, 3), (40, 2)])
def test_rounds_equal_the_one_shot_walk(scored, law, k, m):
    B, n = scored.shape
    rng = np.random.default_rng(k * 10 + m)
    groups = {"div8": np.arange(n) // 8, "random": rng.integers(0, 200, n), "singletons": np.arange(n),
              "giant": np.where(rng.random(n) < 0.6, 0, 1 + np.arange(n) // 5)}[law].astype(np.int32)
    for allowed in (None, rng.random(n) < 0.5, rng.random((B, n)) < 0.3):
        want = ref.one_shot(scored, groups, k, m, allowed)
        seen_rounds = []
        for depth in (k, 2 * k, n):
            got, t = ref.rounds(scored, groups, k, m, depth, allowed)
            assert _same(got, want), (law, depth)
            assert t <= int(np.ceil(np.log2(n / min(n, depth)))) + 1
            seen_rounds.append(t)
        assert seen_rounds[-1] == 1 and (m == 1 or seen_rounds[0] > 1)


def test_singleton_groups_give_the_plain_topk(scored):
    B, n = scored.shape
    k = 25
    st, t = ref.rounds(scored, np.arange(n, dtype=np.int32), k, 1, k)
    ids, sc = ref.topk_lists(scored, k)
    assert t == 1
    assert (st.ids[:, :, 0] == ids).all() and (st.scores[:, :, 0].view(np.uint32) == sc.view(np.uint32)).all() and (st.group == ids).all()


@pytest.mark.parametrize("name", ref.E2E_CASES)
def test_gpu_cases_complete_inside_k_deep(name):
    c = ref.e2e_case(name)
    ip, ix, d = c["rows"]
    _, _, allsc = oracle.csr_search(ip, ix, d, V, c["q"], 10, acc64=True, return_all=True)
    ids, sc = ref.topk_lists(np.asarray(allsc, dtype=np.float32), ref.K_DEEP, c["allowed"])
    st = ref.State(ref.B_E2E, c["k"], c["m"])
    assert ref.walk(st, ids, sc, c["groups"]) == 0, "the walk does not complete inside K_DEEP: the GPU test's expected value is undefined"
    # ... and not trivially: with the forced depth k no case is done after its first round unless it holds a single group
    st1 = ref.State(ref.B_E2E, c["k"], c["m"])
    left = ref.walk(st1, ids[:, :c["k"]], sc[:, :c["k"]], c["groups"])
    assert left > 0 or c["m"] == 1


def test_pack_bits_layout():
    mask = np.zeros(70, dtype=bool)
    mask[[0, 31, 32, 69]] = True
    assert ref.pack_bits(mask).tolist() == [0x80000001, 1, 1 << 5]


def test_argument_errors_need_no_device():
    for bad in (dict(k=0, per_group=1), dict(k=1025, per_group=1), dict(k=1, per_group=65), dict(k=1024, per_group=9), dict(k=3, per_group=1, depth=0)):
        with pytest.raises(ValueError):
            _grouped_args(**bad)
    for bad in (dict(k=1.5, per_group=1), dict(k=True, per_group=1), dict(k=2, per_group="1")):
        with pytest.raises(TypeError):
            _grouped_args(**bad)
    assert _grouped_args(1024, 8) == (1024, 8, None) and _grouped_args(np.int64(3), 2, 5) == (3, 2, 5)

    class Fake:
        n_rows, device = 10, 0
    with pytest.raises(ValueError):
        _search_grouped(Fake(), np.zeros((2, 4), np.float32), 3, 1, np.zeros(9, np.int32), None, None)      # length mismatch
    with pytest.raises(ValueError):
        _search_grouped(Fake(), np.zeros(4, np.float32), 3, 1, np.zeros(10, np.int32), None, None)          # queries not [B, V]
    lib = nat.lib()
    if nat.device_count() <= 0:
        assert lib.vs_topk_collapse(None, None, 1, 1, 1, None, None, 1, 1, 1, 1, None, None, None, None, None, None, 1, 0, 0, None) == nat.VS_ENODEVICE
        assert lib.vs_group_filter(None, 1, 1, None, 1, 1, 1, None, None, None, None, 0, None, 1, 0, None) == nat.VS_ENODEVICE


class _HostIndex(SparseIndex):
    """a facade index whose row count is known without a device"""
    def _n_rows(self):
        return 12

    def _explain_target(self):
        raise nat.VsearchNativeError("no device in this test")


def test_facade_argument_errors():
    idx = _HostIndex()
    with pytest.raises(ValueError, match="12 documents"):
        idx.set_groups(np.zeros(11, np.int32))                       # length mismatch
    with pytest.raises(ValueError, match=">= 0"):
        idx.set_groups(np.array([0] * 11 + [-1]))                    # negative group
    with pytest.raises(TypeError):
        idx.set_groups(np.zeros(12, np.float32))
    with pytest.raises(ValueError):
        idx.set_groups(np.zeros((3, 4), np.int64))
    assert idx.groups is None
    with pytest.raises(RuntimeError, match="no groups"):
        idx.search_grouped(np.zeros((1, 4), np.float32), 3)
    idx._groups = torch.zeros(12, dtype=torch.int32)                 # a grouped index (as set_groups leaves it, on the host here)
    with pytest.raises(ValueError, match="groups="):
        idx._added_groups(None, 2)                                   # add without groups
    with pytest.raises(ValueError, match="groups="):
        idx.update(torch.tensor([1]), torch.zeros((1, 4)))           # update without groups: raises before anything is deleted
    with pytest.raises(ValueError):
        idx._added_groups(np.array([1, 2, 3]), 2)
    with pytest.raises(ValueError):
        idx._added_groups(np.array([1, -2]), 2)
    assert idx._added_groups([4, 5], 2).tolist() == [4, 5]
    idx._groups = None
    with pytest.raises(ValueError, match="no groups"):
        idx._added_groups([1], 1)
