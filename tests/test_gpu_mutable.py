"""GPU tests of the mutable index (vs_index_delete_rows / restore_rows / live_rows / live_bitmap / compact, vs_shard_group_delete_rows;
DeviceIndex / ShardGroup / Index .delete .restore .compact .add) -- run on MI355X.

The yardstick is always something that existed before this feature: the filtered search with an explicit deny DocFilter on an untouched
twin handle, an index built with from_csr from only the surviving rows, export_csr, and the CPU oracle.  Where both sides run this library
the comparison is bit for bit (ids and fp32 score bits)."""
import ctypes as C
import json
import types

import numpy as np
import pytest
import torch

import oracle
from oracle import compare
from conftest import V
from vsearch_amd import synth
from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, ShardGroup
from vsearch_amd.doc_filter import DocFilter

import _select_ref as select_ref

pytestmark = pytest.mark.gpu
RTOL = 1e-4

VALUED_PATHS = {
    "quad": (dict(blocked_postings=1, postings_walk=4), 3, 4),
    "list-walk": (dict(blocked_postings=1, postings_walk=0), 3, 0),
    "fp64-walk": (dict(blocked_postings=1, postings_filter=0, postings_walk=-1), 2, None),
    "mq-scan": (dict(blocked_postings=0), 1, None),
    "one-query-scan": (dict(queries_per_pass=1), 0, None),
}
BINARY_PATHS = {
    "bq-packed": (dict(blocked_postings=1, postings_walk=6, postings_packed=1), 3, 6),
    "bq-int32": (dict(blocked_postings=1, postings_walk=6, postings_packed=0), 3, 6),
    "bin-records": (dict(blocked_postings=1, postings_walk=5), 3, 5),
    "mq-scan": (dict(blocked_postings=0), 1, None),
    "one-query-scan": (dict(queries_per_pass=1), 0, None),
}


def _opts(idx, opts):
    for name, value in opts.items():
        if name == "queries_per_pass":
            idx.set_queries_per_pass(value)
        else:
            idx.set_option(name, value)
    return idx


def _sub_csr(ip, ix, d, rows):
    rows = np.asarray(rows, dtype=np.int64)
    lens = ip[rows + 1] - ip[rows]
    sip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    take = np.concatenate([np.arange(ip[r], ip[r + 1]) for r in rows]) if rows.size else np.zeros(0, np.int64)
    return sip, ix[take], (None if d is None else d[take])


def _same(a, b, what=""):
    (a_ids, a_sc), (b_ids, b_sc) = [tuple(np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x) for x in r) for r in (a, b)]
    assert (a_ids == b_ids).all(), (what, "ids")
    assert (a_sc.view(np.uint32) == b_sc.view(np.uint32)).all(), (what, "score bits")


def _deleted(n, rng, share=0.3):
    """ids to delete: a random share, a whole run, the first and the last row; with duplicates, unsorted"""
    D = np.unique(np.concatenate([np.nonzero(rng.random(n) < share)[0], np.arange(n // 2, n // 2 + 77), [0, n - 1]]))
    return rng.permutation(np.concatenate([D, D[:50]])).astype(np.int64), D


def _check_oracle(ip, ix, d, q, k, allowed, ids, sc):
    _, _, allsc = oracle.csr_search(ip, ix, d, V, q, 1, acc64=True, return_all=True)
    masks = np.broadcast_to(allowed, allsc.shape)
    allsc = np.where(masks, allsc, -np.inf)
    for b in range(q.shape[0]):
        m = min(k, int(masks[b].sum()))
        if m:
            compare.check_topk_valid(allsc[b:b + 1], ids[b:b + 1, :m], sc[b:b + 1, :m], rtol=RTOL)
        assert (ids[b, m:] == -1).all() and np.isneginf(sc[b, m:]).all(), f"query {b}: padding"


# ---- 1. delete = deny filter ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", [nat.VS_F32, nat.VS_F16])
def test_delete_equals_deny_filter_on_every_valued_path(store):
    n, B, k = 20000, 6, 100
    rng = np.random.default_rng(1)
    ip, ix, d = oracle.synth_csr(3, 0, n, V, 768)
    d = d.astype(np.float16) if store == nat.VS_F16 else d
    q = oracle.synth_queries(2, B)
    dup, D = _deleted(n, rng)
    for path, (opts, want_path, want_walk) in VALUED_PATHS.items():
        idx = _opts(DeviceIndex.from_csr(ip, ix, d, V), opts)
        twin = _opts(DeviceIndex.from_csr(ip, ix, d, V), opts)
        assert idx.n_live == n and idx.info().n_live == n
        idx.delete_rows(dup)
        assert idx.n_live == n - D.size and idx.info().n_live == n - D.size and idx.n_rows == n
        got = idx.search(q, k)
        info = idx.info()
        assert info.last_path == want_path and (want_walk is None or info.postings_walk == want_walk), path
        want = twin.search(q, k, filter=DocFilter.from_ids(D, n, allow=False))
        _same(got, want, path)
        assert not np.isin(np.asarray(got[0]), D).any()
        mask = np.ones(n, bool)
        mask[D] = False
        assert (idx.live_mask().cpu().numpy() == mask).all()
        if path == "quad" and store == nat.VS_F32:
            _check_oracle(ip, ix, d, q, k, mask, *map(np.asarray, got))


def test_delete_equals_deny_filter_on_every_binary_path():
    n, B, k = 30000, 9, 50
    rng = np.random.default_rng(5)
    ip, ix, _ = oracle.synth_csr(5, 0, n, V, 86, synth.KIND_BOT)
    q = oracle.synth_queries(6, B, V, 776, synth.VAL_DYADIC)
    dup, D = _deleted(n, rng)
    for path, (opts, want_path, want_walk) in BINARY_PATHS.items():
        idx = _opts(DeviceIndex.from_csr(ip, ix, None, V), opts)
        twin = _opts(DeviceIndex.from_csr(ip, ix, None, V), opts)
        idx.delete_rows(torch.from_numpy(dup))
        got = idx.search(q, k)
        info = idx.info()
        assert info.last_path == want_path and (want_walk is None or info.postings_walk == want_walk), path
        _same(got, twin.search(q, k, filter=DocFilter.from_ids(D, n, allow=False)), path)


def test_delete_on_the_dense_matrix_kind():
    n, Cc, B, k = 12000, 128, 6, 64
    rng = np.random.default_rng(7)
    mat = rng.standard_normal((n, Cc)).astype(np.float32)
    q = rng.standard_normal((B, Cc)).astype(np.float32)
    dup, D = _deleted(n, rng)
    idx, twin = DeviceIndex.from_dense(mat), DeviceIndex.from_dense(mat)
    assert idx.info().n_packets == 0                                   # the matrix-core kind
    idx.delete_rows(dup)
    assert idx.n_live == n - D.size
    _same(idx.search(q, k), twin.search(q, k, filter=DocFilter.from_ids(D, n, allow=False)))
    user = rng.random(n) < 0.5
    both = user.copy()
    both[D] = False
    _same(idx.search(q, k, filter=user), twin.search(q, k, filter=both))
    # compaction: a row gather of the matrix
    new, old = idx.compact()
    keep = np.setdiff1d(np.arange(n), D)
    assert (old == keep).all() and new.n_rows == keep.size and new.n_live == keep.size
    assert (new.export_dense() == mat[keep]).all()
    g_ids, g_sc = map(np.asarray, new.search(q, k))
    _same((old[g_ids], g_sc), idx.search(q, k))


# ---- 2. composition with a user's filter ---------------------------------------------------------------------------------------------
def test_composition_with_shared_and_per_query_filters():
    n, B, k = 20000, 12, 100
    rng = np.random.default_rng(11)
    ip, ix, d = oracle.synth_csr(9, 0, n, V, 768)
    q = oracle.synth_queries(4, B)
    dup, D = _deleted(n, rng)
    shared = rng.random(n) < 0.4
    per = rng.random((B, n)) < 0.3
    few = np.zeros(n, bool)
    few[[0, 5, n // 2 + 3, 9000, n - 1, n - 2]] = True                  # some of them deleted
    for path in ("quad", "mq-scan", "one-query-scan"):
        opts = VALUED_PATHS[path][0]
        idx = _opts(DeviceIndex.from_csr(ip, ix, d, V), opts)
        twin = _opts(DeviceIndex.from_csr(ip, ix, d, V), opts)
        idx.delete_rows(dup)
        for name, mask in (("shared", shared), ("per-query", per), ("few", few)):
            both = mask.copy()
            both[..., D] = False
            _same(idx.search(q, k, filter=DocFilter.from_mask(mask)), twin.search(q, k, filter=DocFilter.from_mask(both)), (path, name))
            _same(idx.search(q, k, filter=mask), twin.search(q, k, filter=both), (path, name, "host mask"))


def test_filter_bit0_through_the_c_entry_point():
    """a user bitmap that starts at an arbitrary bit (vs_index_search_filtered's filter_bit0): the AND kernel's funnel shift"""
    n, B, k = 5003, 5, 60
    rng = np.random.default_rng(13)
    ip, ix, d = oracle.synth_csr(10, 0, n, V, 768)
    q = torch.from_numpy(oracle.synth_queries(5, B)).cuda()
    idx, twin = DeviceIndex.from_csr(ip, ix, d, V), DeviceIndex.from_csr(ip, ix, d, V)
    dup, D = _deleted(n, rng)
    idx.delete_rows(dup)
    for bit0, per_query in ((0, False), (1, False), (31, True), (32, False), (77, True), (4099, False)):
        nb = B if per_query else 1
        big = rng.random((nb, bit0 + n)) < 0.5                         # the rows' bits start at bit0 of a longer bitmap
        f = DocFilter.from_mask(big)
        ld = f.ld if per_query else 0
        both = big[:, bit0:].copy()
        both[:, D] = False
        want = twin.search(q, k, filter=DocFilter.from_mask(both if per_query else both[0]))
        ids = torch.empty((B, k), dtype=torch.int64, device="cuda")
        sc = torch.empty((B, k), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        nat.check(nat.lib().vs_index_search_filtered(idx._h, C.c_void_p(q.data_ptr()), nat.VS_F32, V, B, k, C.c_void_p(f.words.data_ptr()), bit0, ld, 0,
                                                     C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()), None))
        _same((ids, sc), want, (bit0, per_query))


def test_shard_group_with_unaligned_boundaries():
    n, B, k = 20000, 6, 100
    rng = np.random.default_rng(17)
    ip, ix, d = oracle.synth_csr(12, 0, n, V, 768)
    q = oracle.synth_queries(3, B)
    twin = DeviceIndex.from_csr(ip, ix, d, V)
    bounds = [0, 7001, 13333, n]                                        # (no boundary on a word of the bitmap)
    shards = [DeviceIndex.from_csr(*_sub_csr(ip, ix, d, np.arange(r0, r1)), V) for r0, r1 in zip(bounds[:-1], bounds[1:])]
    group = ShardGroup(shards)
    dup, D = _deleted(n, rng)
    D = np.unique(np.concatenate([D, [7000, 7001, 13332, 13333]]))
    group.delete_rows(np.concatenate([dup, [7000, 7001, 13332, 13333, -1]]))
    assert group.n_live == n - D.size and [s.n_rows for s in shards] == [7001, 6332, 6667]
    deny = np.ones(n, bool)
    deny[D] = False
    _same(group.search(q, k), twin.search(q, k, filter=deny), "no user filter")
    shared = rng.random(n) < 0.4
    per = rng.random((B, n)) < 0.2
    for name, mask in (("shared", shared), ("per-query", per)):
        _same(group.search(q, k, filter=DocFilter.from_mask(mask)), twin.search(q, k, filter=mask & deny), name)
    with pytest.raises(ValueError):
        group.delete_rows([n])
    group.delete_rows(torch.tensor([n + 5, 3], device="cuda"))          # device ids: out of range skipped
    assert group.n_live == n - D.size - (0 if 3 in D else 1)
    # compaction of every shard, ids stitched
    group.restore_rows([3])
    new_group, old = group.compact()
    keep = np.nonzero(deny)[0]
    assert (old == keep).all() and new_group.n_rows == keep.size
    g_ids, g_sc = map(np.asarray, new_group.search(q, k))
    _same((old[g_ids], g_sc), group.search(q, k), "compacted group")
    group.restore_rows()
    assert group.n_live == n
    _same(group.search(q, k), twin.search(q, k), "restored group")


# ---- 3. padding ----------------------------------------------------------------------------------------------------------------------
def test_padding_when_fewer_than_k_rows_are_live():
    n, B, k = 3000, 4, 40
    rng = np.random.default_rng(19)
    ip, ix, d = oracle.synth_csr(14, 0, n, V, 768)
    q = oracle.synth_queries(7, B)
    idx, twin = DeviceIndex.from_csr(ip, ix, d, V), DeviceIndex.from_csr(ip, ix, d, V)
    keep = np.sort(rng.choice(n, k - 3, replace=False))
    D = np.setdiff1d(np.arange(n), keep)
    idx.delete_rows(D)
    ids, sc = map(np.asarray, idx.search(q, k))
    assert (ids[:, k - 3:] == -1).all() and np.isneginf(sc[:, k - 3:]).all() and (np.sort(ids[:, :k - 3], axis=1) == keep).all()
    _same((ids, sc), twin.search(q, k, filter=DocFilter.from_ids(keep, n)))
    idx.delete_rows(keep)
    assert idx.n_live == 0
    ids, sc = map(np.asarray, idx.search(q, k))
    assert (ids == -1).all() and np.isneginf(sc).all()
    with pytest.raises(RuntimeError):
        idx.search(q, n + 1)                                           # k > stored rows: VS_ERANGE as before
    new, old = idx.compact()
    assert new.n_rows == 0 and old.size == 0 and new.info().nnz == 0


# ---- 4. restore ----------------------------------------------------------------------------------------------------------------------
def test_restore_and_counting():
    n, B, k = 20000, 6, 100
    rng = np.random.default_rng(23)
    ip, ix, d = oracle.synth_csr(15, 0, n, V, 768)
    q = oracle.synth_queries(8, B)
    idx, twin = DeviceIndex.from_csr(ip, ix, d, V), DeviceIndex.from_csr(ip, ix, d, V)
    want = twin.search(q, k)
    dup, D = _deleted(n, rng)
    idx.delete_rows(dup)                                               # duplicates within one call
    assert idx.n_live == n - D.size
    idx.delete_rows(D[:100])                                           # and again in a second call
    idx.delete_rows(np.array([-1, -1], dtype=np.int64))
    assert idx.n_live == n - D.size
    idx.restore_rows(D[:10])
    idx.restore_rows(D[:10])
    assert idx.n_live == n - D.size + 10
    idx.restore_rows(D)
    assert idx.n_live == n and idx.live_mask().all()
    _same(idx.search(q, k), want, "restored one by one")
    idx.delete_rows(D)
    idx.restore_rows()
    assert idx.n_live == n
    _same(idx.search(q, k), want, "restore all")
    for bad in ([n], [-2], [0, n + 7]):
        with pytest.raises(ValueError):
            idx.delete_rows(bad)
        with pytest.raises(ValueError):
            idx.restore_rows(bad)
    assert idx.n_live == n
    idx.delete_rows(torch.tensor([n, n + 100, -5, 7, 7], device="cuda"))   # device ids: outside the index skipped, never dereferenced
    assert idx.n_live == n - 1


# ---- 5. compaction -------------------------------------------------------------------------------------------------------------------
def _ragged_csr(rng, n, lens_of_note):
    """rows of assorted lengths: empty rows, rows of exactly 8 / 9 non-zeros, long rows"""
    lens = rng.choice([0, 1, 7, 8, 9, 16, 17, 100, 768], n)
    for r, ln in lens_of_note.items():
        lens[r] = ln
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ix = np.concatenate([np.sort(rng.choice(V, ln, replace=False)) for ln in lens] + [np.zeros(0, np.int64)]).astype(np.int64)
    d = (rng.random(ip[-1]) + 0.25).astype(np.float32)
    return ip, ix, d


def _dyadic_queries(rng, B):
    q = np.zeros((B, V), np.float32)
    for b in range(B):
        q[b, rng.choice(V, 768, replace=False)] = rng.integers(1, 9, 768) / 8.0
    return q


@pytest.mark.parametrize("store", [nat.VS_F32, nat.VS_F16, nat.VS_NONE])
def test_compact_equals_the_index_of_the_surviving_rows(store):
    n, B, k = 5000, 5, 50
    rng = np.random.default_rng(29)
    # a deleted run [100, 200) with rows of exactly 8 / 9 non-zeros and an empty row on either side of it
    ip, ix, d = _ragged_csr(rng, n, {97: 8, 98: 9, 99: 0, 200: 0, 201: 8, 202: 9, 0: 9, n - 1: 8})
    if store == nat.VS_F16:
        d = d.astype(np.float16)
    if store == nat.VS_NONE:
        d = None
    D = np.unique(np.concatenate([np.arange(100, 200), [0, n - 1], np.nonzero(rng.random(n) < 0.2)[0]]))
    D = np.setdiff1d(D, [97, 98, 99, 200, 201, 202])
    keep = np.setdiff1d(np.arange(n), D)
    q = _dyadic_queries(rng, B)
    idx = DeviceIndex.from_csr(ip, ix, d, V)
    idx.delete_rows(D)
    new, old = idx.compact()
    assert old.dtype == np.int64 and (old == keep).all()
    ref = DeviceIndex.from_csr(*_sub_csr(ip, ix, d, keep), V)
    for a, b in zip(new.export_csr(), ref.export_csr()):
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all()
    ni, ri = new.info(), ref.info()
    assert (ni.n_rows, ni.nnz, ni.n_packets, ni.n_live, ni.store_dtype, ni.kind) == (keep.size, ri.nnz, ri.n_packets, keep.size, ri.store_dtype, ri.kind)
    assert ni.device == idx.device and idx.n_rows == n and idx.n_live == keep.size       # the source is untouched
    g_ids, g_sc = map(np.asarray, new.search(q, k))
    _same((np.where(g_ids >= 0, old[g_ids], -1), g_sc), idx.search(q, k), "compacted vs tombstoned")
    _same((g_ids, g_sc), ref.search(q, k), "compacted vs rebuilt")
    # a source without tombstones compacts to a copy
    copy, old2 = ref.compact()
    assert (old2 == np.arange(keep.size)).all()
    for a, b in zip(copy.export_csr(), ref.export_csr()):
        assert (a == b).all()


# The packets of a compaction move by the gather of the sub-index (select.hip): a wave takes a run of 64 new rows and rounds of four 64-packet
# steps, 256 packets a round.  (cells of the source rows, surviving rows) at the edges of a run and of a round; a deleted row of 3 cells stands
# before every survivor of the interleaved cases, so that no packet keeps its place.  Rows of 9 / 25 / 30 / 33 cells: 2 / 4 / 4 / 5 packets.
def _before_each(lens):
    src = np.full(2 * len(lens), 3, dtype=np.int64)
    src[1::2] = lens
    return src, np.arange(1, 2 * len(lens), 2)


GATHER_CASES = {
    "65 rows: a full run and a run of one row": _before_each([9] * 64 + [17]),
    "a run of 257 packets: lane 0 of a second round": _before_each([9] * 64 + [25] * 63 + [33]),
    "a run of exactly 256 packets: one round": _before_each([9] * 64 + [30] * 64),
    "a run of empty rows between two runs": _before_each([9] * 64 + [0] * 64 + [9] * 64),
    "the source's last row alone": (np.array([5, 9, 0, 17, 12]), np.array([4])),
    "every row survives": (np.array([0, 1, 8, 9, 40] * 26), np.arange(130)),
}


@pytest.mark.parametrize("case", list(GATHER_CASES))
@pytest.mark.parametrize("store", [nat.VS_F32, nat.VS_F16, nat.VS_NONE])
def test_compact_moves_packets_by_the_shared_gather(store, case):
    lens, keep = GATHER_CASES[case]
    rng = np.random.default_rng(41)
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ix = np.concatenate([np.sort(rng.permutation(V)[:ln]) for ln in lens]).astype(np.int64)
    d = rng.standard_normal(int(ip[-1])).astype(np.float32)
    idx = DeviceIndex.from_csr(ip, ix, None if store == nat.VS_NONE else d, V, store_dtype=store)
    src = idx.export_csr()                                             # the stored rows: fp16 values as stored
    dead = np.setdiff1d(np.arange(len(lens)), keep)
    if dead.size:
        idx.delete_rows(dead)
    new, old = idx.compact()
    assert (old == keep).all()
    want = select_ref.select_ref(*src, keep)                           # the host gather of the surviving rows
    got = new.export_csr()
    assert np.array_equal(got[0], want[0]), "row pointers"
    assert np.array_equal(got[1], want[1]), "columns"
    assert got[2].dtype == want[2].dtype == np.float32 and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), "value bits"
    info = new.info()
    assert (info.n_rows, info.nnz, info.n_packets) == (keep.size, int(lens[keep].sum()), int(((lens[keep] + 7) // 8).sum()))
    assert info.store_dtype == store and new.n_live == keep.size


@pytest.mark.parametrize("survivors", ["one row", "all but row 0"])
def test_compact_gathers_the_rows_of_a_matrix(survivors):
    n, Cc = 70, 96
    rng = np.random.default_rng(43)
    mat = rng.standard_normal((n, Cc)).astype(np.float32)
    keep = np.array([37]) if survivors == "one row" else np.arange(1, n)
    idx = DeviceIndex.from_dense(mat)
    assert idx.info().n_packets == 0                                   # the matrix-core kind
    idx.delete_rows(np.setdiff1d(np.arange(n), keep))
    new, old = idx.compact()
    assert (old == keep).all()
    # the matrix as a CSR of full rows, gathered on the host
    _, _, want = select_ref.select_ref(np.arange(n + 1) * Cc, np.tile(np.arange(Cc), n), mat.reshape(-1), keep)
    got = new.export_dense()
    assert got.shape == (keep.size, Cc) and np.array_equal(np.ascontiguousarray(got).view(np.uint32).reshape(-1), want.view(np.uint32))
    info = new.info()
    assert (info.n_rows, info.nnz, new.n_live) == (keep.size, keep.size * Cc, keep.size)


def test_compact_a_dense_index_stored_as_packets():
    n, Cc, B, k = 4000, 600, 4, 30
    rng = np.random.default_rng(31)
    mat = np.where(rng.random((n, Cc)) < 0.02, rng.standard_normal((n, Cc)), 0).astype(np.float32)
    q = rng.standard_normal((B, Cc)).astype(np.float32)
    idx = DeviceIndex.from_dense(mat, max_density=0.05)
    assert idx.info().kind == nat.VS_KIND_DENSE and idx.info().n_packets > 0
    D = np.unique(np.concatenate([[0, n - 1], np.nonzero(rng.random(n) < 0.3)[0]]))
    keep = np.setdiff1d(np.arange(n), D)
    idx.delete_rows(D)
    new, old = idx.compact()
    assert (old == keep).all() and new.info().kind == nat.VS_KIND_DENSE
    assert (new.export_dense() == mat[keep]).all()
    g_ids, g_sc = map(np.asarray, new.search(q, k))
    _same((old[g_ids], g_sc), idx.search(q, k))


def test_compact_onto_another_gpu():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    n = 5000
    rng = np.random.default_rng(37)
    ip, ix, d = _ragged_csr(rng, n, {})
    idx = DeviceIndex.from_csr(ip, ix, d, V)
    D = np.nonzero(rng.random(n) < 0.2)[0]
    idx.delete_rows(D)
    new, old = idx.compact(device=1)
    assert new.device == 1
    same, _ = idx.compact()
    for a, b in zip(new.export_csr(), same.export_csr()):
        assert (a == b).all()


def test_compact_at_a_million_rows():
    """1 M bag-of-token rows (many scan blocks, short rows of ~11 packets): the compacted index against the tombstoned one and export_csr"""
    n, B, k = 1_000_000, 8, 100
    idx = DeviceIndex.synthetic(41, 0, n, V, 86, synth.KIND_BOT, 0, nat.VS_NONE)
    twin = DeviceIndex.synthetic(41, 0, n, V, 86, synth.KIND_BOT, 0, nat.VS_NONE)
    q = oracle.synth_queries(6, B, V, 776, synth.VAL_DYADIC)
    g = torch.Generator(device="cuda").manual_seed(2)
    dead = torch.rand(n, device="cuda", generator=g) < 0.1
    dead[0] = dead[n - 1] = True
    D = torch.nonzero(dead).flatten()
    idx.delete_rows(D)                                                 # device ids: enqueued on torch's stream
    keep = torch.nonzero(~dead).flatten().cpu().numpy()
    assert idx.n_live == keep.size
    got = idx.search(q, k)
    _same(got, twin.search(q, k, filter=DocFilter.from_mask(~dead)), "1 M rows: delete = deny filter")
    new, old = idx.compact()
    assert (old == keep).all()
    g_ids, g_sc = map(np.asarray, new.search(q, k))
    _same((old[g_ids], g_sc), got, "1 M rows: compacted vs tombstoned")
    a_ip, a_ix, _ = new.export_csr()
    b_ip, b_ix, _ = idx.export_csr()
    lens = np.diff(b_ip)
    assert (np.diff(a_ip) == lens[keep]).all() and new.info().nnz == int(lens[keep].sum())
    sample = np.concatenate([np.arange(0, 2000), np.arange(keep.size - 2000, keep.size), np.random.default_rng(1).choice(keep.size, 5000)])
    for j in sample:
        r = keep[j]
        assert (a_ix[a_ip[j]:a_ip[j + 1]] == b_ix[b_ip[r]:b_ip[r + 1]]).all(), j


# ---- 6. grow -------------------------------------------------------------------------------------------------------------------------
def test_compact_with_spare_capacity_then_append():
    n, m, B, k = 3000, 500, 4, 50
    rng = np.random.default_rng(43)
    ip, ix, d = _ragged_csr(rng, n + m, {})
    q = _dyadic_queries(rng, B)
    a_ip, a_ix, a_d = _sub_csr(ip, ix, d, np.arange(n))
    b_ip, b_ix, b_d = _sub_csr(ip, ix, d, np.arange(n, n + m))
    full = DeviceIndex.from_csr(a_ip, a_ix, a_d, V)
    with pytest.raises(ValueError, match="reserved"):
        full.append_csr(b_ip, b_ix, b_d)                               # from_csr reserves exactly its own rows
    packets = int(((np.diff(b_ip) + 7) // 8).sum())
    grown, old = full.compact(rows_extra=m, packets_extra=packets)
    assert (old == np.arange(n)).all()
    grown.delete_rows([5, n - 1])
    grown.append_csr(b_ip, b_ix, b_d)
    assert grown.n_rows == n + m and grown.n_live == n + m - 2         # the appended rows are live
    assert grown.live_mask()[n:].all()
    grown.restore_rows()
    whole = DeviceIndex.from_csr(ip, ix, d, V)
    for a, b in zip(grown.export_csr(), whole.export_csr()):
        assert (a == b).all()
    _same(grown.search(q, k), whole.search(q, k))
    with pytest.raises(ValueError, match="reserved"):
        grown.append_csr(*_sub_csr(ip, ix, d, [3]))                    # one row too many


def _sparse_index(ip, ix, d, n, cls=None, data=None):
    from vsearch_amd.ir import SparseIndex
    sp = (cls or SparseIndex)(device="cuda:0")
    sp.data = data
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(d), size=(n, V))
    sp.move_to_device("cuda:0")
    return sp


def test_facade_add_grows_an_index_without_spare_capacity():
    n, m, B = 3000, 40, 4
    ip, ix, d = oracle.synth_csr(16, 0, n + m, V, 768)
    a = _sub_csr(ip, ix, d, np.arange(n))
    b = _sub_csr(ip, ix, d, np.arange(n, n + m))
    sp = _sparse_index(*a, n, data=[f"t{i}" for i in range(n)])
    new_rows = torch.sparse_csr_tensor(torch.from_numpy(b[0]), torch.from_numpy(b[1].astype(np.int64)), torch.from_numpy(b[2]), size=(m, V))
    ids = sp.add(new_rows, samples=[f"t{i}" for i in range(n, n + m)])
    assert ids.tolist() == list(range(n, n + m)) and len(sp) == n + m and sp.n_live == n + m
    q = new_rows.to_dense()[:B]                                        # the added rows as queries: each finds itself first
    res = sp.search(q, 5)
    assert res.ids[:, 0].cpu().tolist() == list(range(n, n + B)) and sp.get_sample(n + 1) == f"t{n + 1}"
    whole = DeviceIndex.from_csr(ip, ix, d, V)
    _same((res.ids, res.scores.float()), whole.search(q.numpy(), 5))
    c = _sub_csr(ip, ix, d, np.arange(n, n + 3))
    three = torch.sparse_csr_tensor(torch.from_numpy(c[0]), torch.from_numpy(c[1].astype(np.int64)), torch.from_numpy(c[2]), size=(3, V))
    one = torch.sparse_csr_tensor(torch.from_numpy(c[0][:2]), torch.from_numpy(c[1][:c[0][1]].astype(np.int64)), torch.from_numpy(c[2][:c[0][1]]), size=(1, V))
    ids2 = sp.add(three)                                               # spare capacity from the geometric growth: no second compaction
    assert ids2.tolist() == [n + m, n + m + 1, n + m + 2]
    sp.delete([1, 2])
    big = torch.sparse_csr_tensor(torch.from_numpy(a[0]), torch.from_numpy(a[1].astype(np.int64)), torch.from_numpy(a[2]), size=(n, V))
    with pytest.raises(RuntimeError, match="compact"):
        sp.add(big)                                                    # full, with deleted rows: growing would move ids
    new_ids = sp.update([7], one)
    assert new_ids.tolist() == [n + m + 3] and sp.n_live == n + m + 3 - 3 + 1


# ---- 7. persistence ------------------------------------------------------------------------------------------------------------------
def test_vsx_round_trip_keeps_tombstones(tmp_path):
    n, B, k = 5003, 5, 60
    rng = np.random.default_rng(47)
    ip, ix, d = oracle.synth_csr(18, 0, n, V, 768)
    q = oracle.synth_queries(9, B)
    idx = DeviceIndex.from_csr(ip, ix, d, V)
    idx.save_native(str(tmp_path / "before.vsx"))
    idx.save_npz(str(tmp_path / "before.npz"))
    dup, D = _deleted(n, rng)
    idx.delete_rows(dup)
    idx.save_native(str(tmp_path / "tomb.vsx"))
    with pytest.raises(ValueError, match="compact"):
        idx.save_npz(str(tmp_path / "tomb.npz"))
    back = DeviceIndex.load_native(str(tmp_path / "tomb.vsx"))
    assert back.n_live == n - D.size and back.n_rows == n
    assert (back.live_mask() == idx.live_mask()).all()
    _same(back.search(q, k), idx.search(q, k))
    back.restore_rows(D[:5])
    assert back.n_live == n - D.size + 5
    idx.restore_rows(D)                                                # restored id by id, then all at once: today's bytes either way
    idx.save_native(str(tmp_path / "after1.vsx"))
    idx.delete_rows(D)
    idx.restore_rows()
    idx.save_native(str(tmp_path / "after2.vsx"))
    idx.save_npz(str(tmp_path / "after.npz"))
    want = (tmp_path / "before.vsx").read_bytes()
    assert (tmp_path / "after1.vsx").read_bytes() == want and (tmp_path / "after2.vsx").read_bytes() == want
    assert (tmp_path / "after.npz").read_bytes() == (tmp_path / "before.npz").read_bytes()
    assert len((tmp_path / "tomb.vsx").read_bytes()) == len(want) + 4 * ((n + 31) // 32)
    # slice_rows carries the slice's bits
    idx.delete_rows(D)
    part = idx.slice_rows(1001, 3001)
    inside = D[(D >= 1001) & (D < 4002)] - 1001
    mask = np.ones(3001, bool)
    mask[inside] = False
    assert part.n_live == 3001 - inside.size and (part.live_mask().cpu().numpy() == mask).all()


# ---- 8. facade -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("low_memory", [False, True])
def test_facade_delete_and_compact_follow_the_text_store(tmp_path, low_memory):
    from vsearch_amd.ir import SparseIndex
    n, B, k = 3000, 4, 20
    ip, ix, d = oracle.synth_csr(20, 0, n, V, 768)
    p = tmp_path / "corpus.jsonl"
    p.write_text("".join(json.dumps(f"text {i}") + "\n" for i in range(n)))
    sp = SparseIndex(None, str(p), device="cuda:0", low_memory=low_memory)
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(d), size=(n, V))
    sp.move_to_device("cuda:0")
    q = torch.from_numpy(oracle.synth_queries(10, B))
    first = sp.search(q, k)
    D = np.unique(np.concatenate([first.ids.cpu().numpy()[:, :5].ravel(), [0, n - 1]]))
    sp.delete(torch.from_numpy(D))
    assert sp.n_live == n - D.size and len(sp) == n
    res = sp.search(q, k)
    assert not np.isin(res.ids.cpu().numpy(), D).any()
    ex = sp.explain(q[:1], torch.from_numpy(D[:1].reshape(1, 1)))
    assert int(ex.n_matched[0, 0]) >= 0 and np.isfinite(float(ex.scores[0, 0]))       # a deleted id still answers before compact()
    assert sp.get_vectors(torch.from_numpy(D[:2])).shape[0] == 2
    with pytest.raises(ValueError, match="compact"):
        sp.save(str(tmp_path / "x.npz"))
    sp.save(str(tmp_path / "x.vsx"))
    assert DeviceIndex.load_native(str(tmp_path / "x.vsx")).n_live == n - D.size
    old = sp.compact()
    keep = np.setdiff1d(np.arange(n), D)
    assert (old.numpy() == keep).all() and len(sp) == keep.size and sp.n_live == keep.size
    assert [sp.get_sample(j) for j in (0, 1, keep.size - 1)] == [f"text {keep[j]}" for j in (0, 1, keep.size - 1)]
    after = sp.search(q, k)
    _same((old.numpy()[after.ids.cpu().numpy()], after.scores.float()), (res.ids, res.scores.float()))
    sp.save(str(tmp_path / "y.npz"))
    sp.restore()
    assert sp.n_live == keep.size


def test_facade_sharded_delete_and_compact():
    n, B, k = 20000, 6, 50
    ip, ix, d = oracle.synth_csr(22, 0, n, V, 768)
    sp = _sparse_index(ip, ix, d, n, data=[str(i) for i in range(n)])
    sp.shard_rows([0, 0, 0])                                           # equal ranges of 6667 rows: boundaries off the bitmap's words
    twin = DeviceIndex.from_csr(ip, ix, d, V)
    q = torch.from_numpy(oracle.synth_queries(11, B))
    rng = np.random.default_rng(53)
    dup, D = _deleted(n, rng)
    sp.delete(dup)
    assert sp.n_live == n - D.size
    res = sp.search(q, k)
    _same((res.ids, res.scores.float()), twin.search(q.numpy(), k, filter=DocFilter.from_ids(D, n, allow=False)))
    old = sp.compact().numpy()
    assert (old == np.setdiff1d(np.arange(n), D)).all() and sp.get_sample(5) == str(old[5]) and len(sp.shards) == 3
    after = sp.search(q, k)
    _same((old[after.ids.cpu().numpy()], after.scores.float()), (res.ids, res.scores.float()))


def test_retriever_never_returns_a_deleted_document():
    from vsearch_amd.ir import BoTIndex, Retriever
    n, B, k = 3000, 4, 20
    ip, ix, d = oracle.synth_csr(2, 0, n, V, 86, synth.KIND_BOT)
    bot = _sparse_index(ip, ix, d.astype(np.float32), n, cls=BoTIndex, data=[str(i) for i in range(n)])
    ip2, ix2, d2 = oracle.synth_csr(8, 0, n)
    p_dense = torch.sparse_csr_tensor(torch.from_numpy(ip2), torch.from_numpy(ix2.astype(np.int64)), torch.from_numpy(d2), size=(n, V)).to_dense().cuda()
    fake = types.SimpleNamespace(index=bot, device="cuda", encoder_q=types.SimpleNamespace(config=types.SimpleNamespace(topk=768)),
                                 encoder_p=types.SimpleNamespace(embed=lambda texts, batch_size=32, require_grad=False, **kw: p_dense[[int(t) for t in texts]]))
    for name in ("process_query", "_rerank", "retrieve", "more_like_this", "retrieve_with_feedback", "delete_documents", "compact_index"):
        setattr(fake, name, types.MethodType(getattr(Retriever, name), fake))
    q = torch.from_numpy(oracle.synth_queries(7, B))
    seeds = torch.tensor([[10], [11], [12], [13]])
    before = [fake.retrieve(q, k=k, rerank=True), fake.more_like_this(seeds, k=k), fake.retrieve_with_feedback(q, k=k)]
    D = np.unique(np.concatenate([r.ids.cpu().numpy()[:, :6].ravel() for r in before]))
    D = D[D >= 0]
    fake.delete_documents(D)
    after = [fake.retrieve(q, k=k, rerank=True), fake.retrieve(q, k=k), fake.more_like_this(seeds, k=k), fake.retrieve_with_feedback(q, k=k)]
    for r in after:
        ids = r.ids.cpu().numpy()
        assert not np.isin(ids, D).any() and (ids >= 0).all()
    old = fake.compact_index()
    assert old.shape[0] == n - D.size and bot.get_sample(3) == str(int(old[3]))
    again = fake.retrieve(q, k=k)
    assert (old.numpy()[again.ids.cpu().numpy()] == after[1].ids.cpu().numpy()).all()


# ---- 9. streams ----------------------------------------------------------------------------------------------------------------------
def test_delete_search_restore_search_back_to_back_on_one_stream():
    n, B, k = 20000, 16, 100
    rng = np.random.default_rng(59)
    ip, ix, d = oracle.synth_csr(21, 0, n, V, 768)
    q = oracle.synth_queries(4, B)
    idx = DeviceIndex.from_csr(ip, ix, d, V).prepare()
    twin = DeviceIndex.from_csr(ip, ix, d, V).prepare()
    dup, D = _deleted(n, rng)
    want_del = twin.search(q, k, filter=DocFilter.from_ids(D, n, allow=False))
    want_all = twin.search(q, k)
    user = rng.random(n) < 0.5
    deny = np.ones(n, bool)
    deny[D] = False
    want_both = twin.search(q, k, filter=user & deny)
    idx.delete_rows([0])                                               # (the bitmap exists: from here on nothing allocates)
    idx.restore_rows([0])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        qd, ids_d = torch.from_numpy(q).cuda(), torch.from_numpy(dup).cuda()
        f = DocFilter.from_mask(torch.from_numpy(user).cuda())
        idx.delete_rows(ids_d)
        r1 = idx.search(qd, k)
        r2 = idx.search(qd, k, filter=f)
        idx.restore_rows(ids_d)
        r3 = idx.search(qd, k)
    s.synchronize()
    assert idx.info().last_path == 3 and idx.n_live == n
    _same(r1, want_del, "deleted")
    _same(r2, want_both, "deleted AND filter")
    _same(r3, want_all, "restored")
