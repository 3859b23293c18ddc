"""GPU tests of grouped search (vs_topk_collapse, vs_group_filter; DeviceIndex / ShardGroup .search_grouped, Index.search_grouped,
Retriever.retrieve_grouped) -- run on MI355X.

The contract: the result is the serial walk of tests/_grouped_ref.py over the complete canonical ranking, whatever the
first depth; group ids, ids and score BITS are compared.  End to end the expected value is the numpy walk over a deep plain search of the
same handle (K_DEEP <= 800), which tests/test_grouped_cpu.py proves to complete for every case used here."""
import numpy as np
import pytest
import torch

from conftest import V
from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, GroupState, ShardGroup, _search_grouped, group_filter, topk_collapse
from vsearch_amd.doc_filter import DocFilter
from test_gpu_by_example import BINARY_PATHS, VALUED_PATHS, _opts
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

import _grouped_ref as ref

pytestmark = pytest.mark.gpu


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _gstate(st, on_dev):
    """a ref.State as the GroupState the bindings take (host arrays, or tensors on GPU 0)"""
    gs = GroupState(st.B, st.k, st.m, 0 if on_dev else None)
    for name in ("group", "count", "ids", "scores", "status"):
        src = getattr(st, name)
        if on_dev:
            getattr(gs, name).copy_(torch.from_numpy(src))
        else:
            setattr(gs, name, src.copy())
    return gs


def _assert_state(gs, st, label, status=True):
    for name in ("group", "count", "ids") + (("status",) if status else ()):
        assert (_np(getattr(gs, name)) == getattr(st, name)).all(), (label, name)
    assert (_np(gs.scores).view(np.uint32) == st.scores.view(np.uint32)).all(), (label, "scores")


def _dev(x, on_dev):
    if x is None or not on_dev:
        return x
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _lists(rng, Bp, kk, n_rows):
    """Bp ranked lists over rows of [0, n_rows): distinct ids, scores descending with ties"""
    ids = np.stack([rng.permutation(n_rows)[:kk] for _ in range(Bp)]).astype(np.int64)
    sc = -np.sort(-rng.integers(0, max(2, kk // 3), (Bp, kk)).astype(np.float32), axis=1) * np.float32(0.37)
    return ids, sc


LAWS = {
    "mod7": lambda n: (np.arange(n) % 7).astype(np.int32),          # every group repeats inside a 64-entry chunk and across chunks
    "one": lambda n: np.full(n, 3, dtype=np.int32),                 # every row one group
    "own": lambda n: np.arange(n, dtype=np.int32)[::-1].copy(),     # every row its own group
    "runs": lambda n: (np.arange(n) // 3 * 1000003 % 2147483647).astype(np.int32),
}
KM = [(1, 1), (1, 64), (5, 2), (40, 3), (128, 64), (1024, 1), (1024, 8)]


# ---- vs_topk_collapse alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kk", [1, 63, 64, 65, 128, 1000])
def test_collapse_equals_the_serial_walk(kk):
    rng = np.random.default_rng(kk)
    n_rows, Bp = 1500, 5
    for law, make in LAWS.items():
        groups = make(n_rows)
        ids, sc = _lists(rng, Bp, kk, n_rows)
        if kk > 2:                                                  # padding mid-list: list 1 ends early, list 2 inside its first chunk
            ids[1, kk // 2:], sc[1, kk // 2:] = -1, -np.inf
            ids[2, 1:], sc[2, 1:] = -1, -np.inf
        for k, m in KM:
            want = ref.State(Bp, k, m)
            left = ref.walk(want, ids, sc, groups)
            for on_dev in (False, True):
                gs = GroupState(Bp, k, m, 0 if on_dev else None)
                if not on_dev:                                      # init must clear whatever the buffers held
                    gs.group[:], gs.count[:], gs.ids[:], gs.scores[:], gs.status[:] = 5, 9, 77, 1.5, 1
                topk_collapse(gs, _dev(ids, on_dev), _dev(sc, on_dev), _dev(groups, on_dev), init=True)
                _assert_state(gs, want, (law, k, m, on_dev))
                assert int(_np(gs.incomplete)[0]) == left, (law, k, m, on_dev)


def test_collapse_fills_1024_groups_and_exhaustion_hint():
    rng = np.random.default_rng(5)
    n_rows, kk = 4000, 3000
    ids, sc = _lists(rng, 3, kk, n_rows)
    for groups, k, m in ((LAWS["own"](n_rows), 1024, 1), ((np.arange(n_rows) // 2).astype(np.int32), 1024, 2), (LAWS["mod7"](n_rows), 7, 64)):
        want = ref.State(3, k, m)
        left = ref.walk(want, ids, sc, groups)
        assert left == (3 if m == 2 else 0)                         # k groups open and full: complete without the end of the list
        assert ((want.group >= 0).sum(1) == k).all()
        gs = GroupState(3, k, m, 0)
        topk_collapse(gs, _dev(ids, True), _dev(sc, True), _dev(groups, True), init=True)
        _assert_state(gs, want, (k, m))
        assert int(gs.incomplete.item()) == left
    groups = LAWS["own"](n_rows)
    for hint in (False, True):                                      # 100 rows, 200 groups wanted: complete only when nothing ranks behind
        want = ref.State(3, 200, 1)
        left = ref.walk(want, ids[:, :100], sc[:, :100], groups, exhausted_hint=hint)
        assert left == (0 if hint else 3)
        gs = GroupState(3, 200, 1, None)
        topk_collapse(gs, ids[:, :100], sc[:, :100], groups, init=True, exhausted_hint=hint)
        _assert_state(gs, want, hint)
        assert int(gs.incomplete[0]) == left


@pytest.mark.parametrize("on_dev", [False, True])
def test_collapse_continues_a_round_through_a_qmap(on_dev):
    rng = np.random.default_rng(11)
    n_rows, B, k, m = 900, 6, 6, 3
    groups = (np.arange(n_rows) % 15).astype(np.int32)
    perm = np.stack([rng.permutation(n_rows) for _ in range(B)]).astype(np.int64)
    sc = -np.sort(-rng.random((B, n_rows)).astype(np.float32), axis=1)
    st = ref.State(B, k, m)
    assert ref.walk(st, perm[:, :20], sc[:, :20], groups) == B      # round 1: groups open, some full, some half full, none complete
    assert (st.count == m).any() and ((st.count > 0) & (st.count < m)).any()
    st.status[2] = 1                                                # a finished query that is listed all the same: left as it is
    qmap = np.array([4, 2, 0, 5], dtype=np.int32)
    ids2, sc2 = perm[qmap, 20:220], sc[qmap, 20:220]
    want = st.copy()
    left = ref.walk(want, ids2, sc2, groups, qmap=qmap)
    gs = _gstate(st, on_dev)
    topk_collapse(gs, _dev(ids2, on_dev), _dev(sc2, on_dev), _dev(groups, on_dev), qmap=_dev(qmap, on_dev))
    _assert_state(gs, want, on_dev)
    assert int(_np(gs.incomplete)[0]) == left
    assert (want.group[[1, 3]] == st.group[[1, 3]]).all()           # (the queries not listed keep their state)
    # the two rounds together are the walk over the joined list
    whole = ref.State(B, k, m)
    ref.walk(whole, perm[:, :220], sc[:, :220], groups)
    for b in (0, 4, 5):
        assert (whole.ids[b] == want.ids[b]).all() and (whole.group[b] == want.group[b]).all()


def test_collapse_rejects_what_it_cannot_take():
    n_rows = 100
    groups = np.zeros(n_rows, np.int32)
    ids, sc = np.arange(8, dtype=np.int64)[None], np.zeros((1, 8), np.float32)
    for k, m in ((0, 1), (1025, 1), (1, 0), (1, 65), (1024, 9), (129, 64)):
        with pytest.raises(ValueError):
            topk_collapse(_bad_state(k, m), ids, sc, groups, init=True)
    gs = GroupState(1, 4, 2, None)
    lib = nat.lib()
    call = lambda kk, ld, i=ids: lib.vs_topk_collapse(i.ctypes.data, sc.ctypes.data, 1, kk, ld, None, groups.ctypes.data, n_rows, 1, 4, 2, gs.group.ctypes.data,
                                                      gs.count.ctypes.data, gs.ids.ctypes.data, gs.scores.ctypes.data, gs.status.ctypes.data,
                                                      gs.incomplete.ctypes.data, 1, 0, 0, None)
    assert call(0, 8) == nat.VS_EINVAL and call(16385, 16385) == nat.VS_EINVAL and call(8, 7) == nat.VS_EINVAL
    for bad in (n_rows, -2):                                        # a host list is checked ...
        b = ids.copy()
        b[0, 3] = bad
        assert call(8, 8, b) == nat.VS_EINVAL and "outside" in nat.last_error()
        want = ref.State(1, 4, 2)                                   # ... a device list ends there
        ref.walk(want, b, sc, groups)
        gd = GroupState(1, 4, 2, 0)
        topk_collapse(gd, _dev(b, True), _dev(sc, True), _dev(groups, True), init=True)
        _assert_state(gd, want, bad)
        assert want.status[0] == 1 and want.count[0, 0] == 2
    with pytest.raises(ValueError, match="host or all"):            # host lists, device state
        topk_collapse(GroupState(1, 4, 2, 0), ids, sc, groups, init=True)
    with pytest.raises(ValueError):                                 # qmap outside the state
        topk_collapse(GroupState(1, 4, 2, None), ids, sc, groups, qmap=np.array([1], np.int32), init=True)
    assert call(8, 8) == nat.VS_OK


def _bad_state(k, m):
    gs = GroupState(1, 1, 1, None)
    gs.k, gs.m = k, m
    return gs


# ---- vs_group_filter alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [31, 32, 33, 1023, 1025, 6001])
def test_group_filter_equals_the_rule(n_rows):
    rng = np.random.default_rng(n_rows)
    B, k, m = 6, 5, 2
    groups = (rng.integers(0, 12, n_rows) * 1000).astype(np.int32)
    ids, sc = _lists(rng, B, 24, n_rows)
    ids[0, 3:], sc[0, 3:] = -1, -np.inf                             # query 0: fewer than k groups open
    ids[1, 6:], sc[1, 6:] = -1, -np.inf                             # query 1: a short list, groups half full
    st = ref.State(B, k, m)
    ref.walk(st, ids, sc, groups)
    n_open = (st.group >= 0).sum(1)
    assert n_open[0] < k and ((n_open == k) & (st.count == m).any(1)).any() and ((st.count > 0) & (st.count < m)).any()
    W = (n_rows + 31) // 32
    shared = rng.random(n_rows) < 0.6
    per_q = rng.random((B, n_rows)) < 0.6
    for qmap in (np.arange(B, dtype=np.int32), np.array([5, 0, 3], dtype=np.int32)):
        for label, allowed in (("none", None), ("shared", shared), ("per-query", per_q)):
            mask = ref.next_filter(st, groups, qmap, allowed)
            kept = st.ids[qmap].reshape(len(qmap), -1)
            for i in range(len(qmap)):                              # kept rows are cleared
                assert not mask[i, kept[i][kept[i] >= 0]].any()
            want = ref.pack_bits(mask)
            fw = None if allowed is None else ref.pack_bits(allowed)
            fld = 0 if allowed is None or allowed.ndim == 1 else W
            for on_dev in (False, True):
                gs = _gstate(st, on_dev)
                out = np.full((len(qmap), W), 0xFFFFFFFF, dtype=np.uint32)     # every word is written whole; bits past n_rows are 0
                out_d = torch.from_numpy(out.view(np.int32)).cuda() if on_dev else out
                got = group_filter(gs, _dev(groups, on_dev), _dev(qmap, on_dev), None if fw is None else _dev(fw.view(np.int32) if on_dev else fw, on_dev),
                                   fld, out=out_d)
                got = _np(got).view(np.uint32)
                assert (got == want).all(), (label, on_dev, len(qmap))
                if n_rows & 31:
                    assert (got[:, -1] >> (n_rows & 31) == 0).all()


def test_group_filter_with_1024_groups():
    rng = np.random.default_rng(3)
    n_rows, B, k, m = 6001, 3, 1024, 2
    groups = (rng.permutation(n_rows) // 3).astype(np.int32)
    ids, sc = _lists(rng, B, 2500, n_rows)
    st = ref.State(B, k, m)
    assert ref.walk(st, ids, sc, groups) == B and ((st.group >= 0).sum(1) == k).all()
    qmap = np.arange(B, dtype=np.int32)
    want = ref.pack_bits(ref.next_filter(st, groups, qmap))
    got = group_filter(_gstate(st, True), _dev(groups, True), _dev(qmap, True))
    assert (_np(got).view(np.uint32) == want).all()


# ---- search_grouped, end to end -------------------------------------------------------------------------------------------------------
_handles = {}


def _handle(kind):
    """one DeviceIndex per kind for the cases without tombstones or options"""
    if kind not in _handles:
        ip, ix, d = ref.e2e_rows(kind)
        _handles[kind] = DeviceIndex.from_csr(ip, ix, d, V)
    return _handles[kind]


def _expected(idx, c, flt):
    """the numpy walk over the deep plain search of the same handle; it must complete inside that list"""
    ids, sc = idx.search(c["q"], ref.K_DEEP, filter=flt)
    st = ref.State(ref.B_E2E, c["k"], c["m"])
    assert ref.walk(st, ids, sc, c["groups"]) == 0, "the walk did not complete inside K_DEEP"
    if c["allowed"] is not None:
        assert c["allowed"][ids[ids >= 0]].all()
    return st


def _check(res, st, label):
    assert (_np(res.groups) == st.group).all(), (label, "groups")
    assert (_np(res.ids) == st.ids).all(), (label, "ids")
    assert _np(res.scores).dtype == np.float32 and (_np(res.scores).view(np.uint32) == st.scores.view(np.uint32)).all(), (label, "scores")


def _filter_of(idx, c):
    flt = None
    if c["mask"] is not None:
        flt = DocFilter.from_mask(torch.from_numpy(c["mask"]))
    if c["terms"] is not None:
        t = DocFilter.from_terms(idx, **c["terms"])
        flt = t if flt is None else flt & t
    return flt


@pytest.mark.parametrize("name", ref.E2E_CASES)
def test_search_grouped_equals_the_walk_at_every_depth(name):
    c = ref.e2e_case(name)
    k, m, groups = c["k"], c["m"], c["groups"]
    if c["deleted"] is not None:
        ip, ix, d = c["rows"]
        idx = DeviceIndex.from_csr(ip, ix, d, V)
        idx.delete_rows(c["deleted"])
    else:
        idx = _handle(c["kind"])
    flt = _filter_of(idx, c)
    want = _expected(idx, c, flt)
    rounds = []
    for depth in (k, None, ref.K_DEEP):
        got = _search_grouped(idx, c["q"], k, m, groups, flt, depth, rounds_out=rounds)
        assert isinstance(got.ids, np.ndarray)                      # numpy in -> numpy out
        _check(got, want, (name, depth))
    assert rounds[2] == 1 and (rounds[0] > 1 or m == 1), rounds     # depth = k forces several rounds
    # torch in -> torch out, groups already on the device
    got = idx.search_grouped(torch.from_numpy(c["q"]).cuda(), k, torch.from_numpy(groups).cuda(), per_group=m, filter=flt, depth=k)
    assert got.ids.is_cuda and got.groups.dtype == torch.int32 and got.ids.dtype == torch.int64
    _check(got, want, (name, "torch"))
    if "onegroup" in name:                                          # fewer groups than k: padded
        assert (want.group[:, 0] == 7).all() and (want.group[:, 1:] == -1).all()
        assert (want.ids[:, 1:] == -1).all() and np.isneginf(want.scores[:, 1:]).all()


def test_singleton_groups_at_one_row_a_group_are_the_plain_search():
    c = ref.e2e_case("vdr-singletons-m1")
    idx = _handle("vdr")
    ids, sc = idx.search(c["q"], 50)
    got = idx.search_grouped(c["q"], 50, c["groups"])
    assert (got.ids[:, :, 0] == ids).all() and (got.groups == ids).all() and (got.scores[:, :, 0].view(np.uint32) == sc.view(np.uint32)).all()


@pytest.mark.parametrize("path", ["quad", "mq-scan", "one-query-scan", "bq-packed"])
def test_search_grouped_on_forced_paths(path):
    valued = path != "bq-packed"
    c = ref.e2e_case("vdr-div8-m3" if valued else "bot-div8-m3")
    ip, ix, d = c["rows"]
    idx = _opts(DeviceIndex.from_csr(ip, ix, d, V), (VALUED_PATHS if valued else BINARY_PATHS)[path])
    want = _expected(idx, c, None)
    for depth in (c["k"], None):
        _check(idx.search_grouped(c["q"], c["k"], c["groups"], per_group=c["m"], depth=depth), want, (path, depth))
    mask = ref.e2e_case("vdr-div8-m3-mask")["mask"]
    if valued:                                                      # and under a filter (its own expected value)
        cm = ref.e2e_case("vdr-div8-m3-mask")
        flt = DocFilter.from_mask(torch.from_numpy(mask))
        _check(idx.search_grouped(cm["q"], cm["k"], cm["groups"], per_group=cm["m"], filter=flt, depth=cm["k"]), _expected(idx, cm, flt), (path, "mask"))


def test_three_shards_equal_the_unsharded_index():
    for name in ("vdr-div8-m3", "vdr-div8-m3-mask", "vdr-giant-m1"):
        c = ref.e2e_case(name)
        whole = _handle("vdr")
        flt = _filter_of(whole, c)
        want = _expected(whole, c, flt)
        bounds = [0, 1999, 4001, ref.N_E2E]
        shards = [whole.slice_rows(bounds[i], bounds[i + 1] - bounds[i], device=0) for i in range(3)]
        group = ShardGroup(shards)
        for depth in (c["k"], None):
            _check(group.search_grouped(c["q"], c["k"], c["groups"], per_group=c["m"], filter=flt, depth=depth), want, (name, depth))
        got = group.search_grouped(torch.from_numpy(c["q"]).cuda(), c["k"], c["groups"], per_group=c["m"], filter=flt)
        assert got.ids.is_cuda
        _check(got, want, (name, "torch"))
        group.close()


# ---- facade ---------------------------------------------------------------------------------------------------------------------------
def _sparse_index(rows):
    from vsearch_amd.ir import SparseIndex
    ip, ix, d = rows
    sp = SparseIndex(device="cuda:0")
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(d), size=(ip.shape[0] - 1, V))
    sp.move_to_device("cuda:0")
    return sp


def test_facade_search_grouped_compact_and_add():
    c = ref.e2e_case("vdr-div8-m3")
    n, k, m = ref.N_E2E, c["k"], c["m"]
    sp = _sparse_index(c["rows"])
    with pytest.raises(RuntimeError, match="no groups"):
        sp.search_grouped(c["q"], k)
    with pytest.raises(ValueError):
        sp.set_groups(c["groups"][:-1])
    with pytest.raises(ValueError):
        sp.set_groups(-c["groups"] - 1)
    sp.set_groups(c["groups"])
    assert sp.groups.is_cuda and sp.groups.dtype == torch.int32 and (sp.groups.cpu().numpy() == c["groups"]).all()

    def expected(index, groups, q):
        r = index.search(q, ref.K_DEEP)
        st = ref.State(q.shape[0], k, m)
        assert ref.walk(st, _np(r.ids), _np(r.scores), groups) == 0
        return st
    q = torch.from_numpy(c["q"])
    got = sp.search_grouped(q, k, per_group=m, depth=k)
    assert got.ids.is_cuda and got.scores.dtype == sp._dtype
    _check(got, expected(sp, c["groups"], q), "facade")
    # deleted documents do not come back; compact() moves the groups with the rows
    dead = _np(got.ids[:, 0, 0])
    sp.delete(torch.from_numpy(dead))
    got = sp.search_grouped(q, k, per_group=m)
    assert not np.isin(_np(got.ids), dead).any()
    _check(got, expected(sp, c["groups"], q), "facade, deleted")
    old = sp.compact().numpy()
    assert old.shape[0] == n - np.unique(dead).size and (sp.groups.cpu().numpy() == c["groups"][old]).all()
    after = sp.search_grouped(q, k, per_group=m)
    assert (_np(after.groups) == _np(got.groups)).all() and (old[_np(after.ids)][_np(after.ids) >= 0] == _np(got.ids)[_np(got.ids) >= 0]).all()
    # add(groups=): the new documents join their groups; a grouped index refuses an add without them
    ip, ix, d = c["rows"]
    new = torch.sparse_csr_tensor(torch.from_numpy(ip[:4]), torch.from_numpy(ix[:ip[3]].astype(np.int64)), torch.from_numpy(d[:ip[3]]), size=(3, V))
    with pytest.raises(ValueError, match="groups="):
        sp.add(new)
    with pytest.raises(ValueError, match="groups="):
        sp.update(torch.tensor([0]), new)
    n0 = sp._n_rows()
    new_ids = sp.add(new, groups=[900000, 5, 900000])
    assert new_ids.tolist() == [n0, n0 + 1, n0 + 2] and sp.groups.shape[0] == n0 + 3 and sp.groups[-3:].tolist() == [900000, 5, 900000]
    g_now = sp.groups.cpu().numpy()
    _check(sp.search_grouped(q, k, per_group=m, depth=k), expected(sp, g_now, q), "facade, added")
    # row shards on one GPU: the same answer
    want = sp.search_grouped(q, k, per_group=m)
    sp.shard_rows([0, 0, 0])
    got = sp.search_grouped(q, k, per_group=m, depth=k)
    assert torch.equal(got.groups, want.groups) and torch.equal(got.ids, want.ids) and torch.equal(got.scores, want.scores)


def test_groups_from_samples_factorises_a_field():
    c = ref.e2e_case("vdr-div8-m1")
    ip, ix, d = c["rows"]
    sp = _sparse_index((ip[:41], ix[:ip[40]], d[:ip[40]]))
    titles = ["t%d" % (i % 7) for i in range(40)]
    sp.data = [{"title": t, "text": str(i)} for i, t in enumerate(titles)]
    names = sp.groups_from_samples("title")
    assert names == ["t%d" % i for i in range(7)] and sp.groups.tolist() == [i % 7 for i in range(40)]
    with pytest.raises(KeyError):
        sp.groups_from_samples("nope")


def test_retriever_retrieve_grouped(tiny_retriever):
    from vsearch_amd.ir.retriever.index import IndexType
    r = tiny_retriever
    n = 80
    r.build_index(make_texts(n, 5), index_type=IndexType.SPARSE)
    idx = r.index
    groups = (np.arange(n) % 16).astype(np.int32)
    idx.set_groups(groups)
    queries = make_texts(4, 9)
    k, m = 6, 2
    col = int(idx.get_vectors(torch.tensor([3])).col_indices()[0])
    for kw in ({}, dict(must_not=[col]), dict(filter=np.arange(n) % 3 != 0)):
        deep = r.retrieve(queries, k=n, **kw)
        st = ref.State(4, k, m)
        ref.walk(st, _np(deep.ids), _np(deep.scores), groups, exhausted_hint=True)
        got = r.retrieve_grouped(queries, k=k, per_group=m, depth=3, **kw)
        _check(got, st, kw)
    assert (st.group >= 0).all()
