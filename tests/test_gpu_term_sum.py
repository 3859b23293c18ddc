"""GPU tests of the term sums (vs_index_term_sums / vs_index_term_sums_ids / vs_term_sum_topn; DeviceIndex / ShardGroup .term_sums /
.top_weight_terms, Index.term_sums / .centroid / .centroid_terms, Retriever.centroid_terms) -- run on MI355X.

The contract is tests/_term_sum_ref.py.  The sums are fixed-point integers and the scores fp64 arithmetic rounded once to
fp32, so everything compares with ==.  Expected sums come from the reference applied to what get_rows returns for the same index, so they hold
whatever the builder does with explicit zeros.  The raw calls go into junk-filled outputs whose sum rows carry spare columns (ld_sums = n_cols
+ 3) that must keep their junk, once on host buffers and once on device buffers."""
import ctypes as C

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, ShardGroup, TermSums, TopWeights, term_sum_plan, term_sum_topn
from vsearch_amd.doc_filter import DocFilter
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

import _range_ref as rref
from _facet_ref import masks_case
import _term_agg_ref as aref
import _term_sum_ref as ref

pytestmark = pytest.mark.gpu

TILE = nat.TERM_SUM_TILE_COLS
JUNK = -0x5A5A5A5A5A5A5A5B
PAD = 3                       # spare columns of a sum row
F32 = np.float32
STORES = {"fp32": nat.VS_F32, "fp16": nat.VS_F16, "bin": nat.VS_NONE}
ONE = ref.ONE


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _masks(B, n_rows, seed, density=0.9):
    """per-query sets of different densities with all-zero stretches (whole 64-row steps and 2048-row spans are skipped)"""
    return masks_case(B, n_rows, seed=seed, density=density)


def _build(ip, ix, va, V, store="fp32"):
    return DeviceIndex.from_csr(ip, ix, None if store == "bin" else va, V, store_dtype=STORES[store])


def _rows(dev):
    return dev.get_rows(np.arange(dev.n_rows, dtype=np.int64))


def _cells(dev, V):
    """the reference's view of the index: the cells get_rows returns for every row"""
    return ref.Cells(*_rows(dev), V)


def _bufs(arrs, on_dev):
    if on_dev:
        arrs = {k: torch.from_numpy(v).cuda() for k, v in arrs.items()}
        torch.cuda.synchronize()
        return arrs, (lambda t: C.c_void_p(t.data_ptr()))
    return arrs, (lambda a: C.c_void_p(a.ctypes.data))


def _outs(B, V):
    return dict(sums=np.full((B, V + PAD), JUNK, np.int64), total=np.full(B, JUNK, np.int64))


def _taken(outs, V):
    sums = _np(outs["sums"])
    assert (sums[:, V:] == JUNK).all(), "a sum row's spare columns were written"
    return sums[:, :V], _np(outs["total"])


def _raw_sums(dev, V, words, bit0, ld_words, B, rpc, tc, on_dev):
    """vs_index_term_sums into junk-filled outputs, host or device buffers throughout -> (sums, total)"""
    arrs = _outs(B, V)
    if words is not None:
        arrs["words"] = np.ascontiguousarray(words).view(np.int32)
    arrs, ptr = _bufs(arrs, on_dev)
    nat.check(nat.lib().vs_index_term_sums(dev._h, ptr(arrs["words"]) if words is not None else None, bit0, ld_words, B, rpc, tc, ptr(arrs["sums"]),
                                           V + PAD, ptr(arrs["total"]), None))
    return _taken(arrs, V)


def _raw_ids(dev, V, ids, id_offset, strict, on_dev, ld=None, tc=0):
    """vs_index_term_sums_ids into junk-filled outputs -> (rc, sums, total); ld > m: the list rows carry spare entries"""
    B, m = ids.shape
    ld = ld or m
    lists = np.full((B, ld), 0x7777777777, np.int64)                 # (spare entries name no row: they must not be read)
    lists[:, :m] = ids
    arrs = _outs(B, V)
    arrs["ids"] = lists
    arrs, ptr = _bufs(arrs, on_dev)
    rc = nat.lib().vs_index_term_sums_ids(dev._h, ptr(arrs["ids"]), B, m, ld, id_offset, strict, tc, ptr(arrs["sums"]), V + PAD, ptr(arrs["total"]), None)
    return (rc,) + _taken(arrs, V)


def _check(dev, cells, masks, bit0, live=None, rpc=0, tc=0, shared=False, what=None, kinds=(False, True)):
    """per-query sets `masks` [B, n] packed at bit0 with every spare bit set -> both buffer kinds against the reference"""
    B, n = masks.shape
    V = cells.n_cols
    words = ref.pack(masks, bit0, spare=1)
    ld = 0 if shared else words.shape[1]
    want = ref.term_sums(words, ld, bit0, cells, ref.pack(live[None, :])[0] if live is not None else None)
    for on_dev in kinds:
        got = _raw_sums(dev, V, words, bit0, ld, B, rpc, tc, on_dev)
        for g, w, name in zip(got, want, ("sums", "total")):
            assert g.dtype == np.int64 and (g == w).all(), (what, name, on_dev, bit0, rpc, tc, np.argwhere(g != w)[:5])
    return want


def _check_null(dev, cells, live=None, tc=0):
    want = ref.term_sums(None, 0, 0, cells, ref.pack(live[None, :])[0] if live is not None else None)
    for on_dev in (False, True):
        got = _raw_sums(dev, cells.n_cols, None, 0, 0, 1, 0, tc, on_dev)
        assert all((g == w).all() for g, w in zip(got, want)), ("NULL words", on_dev, tc)
    return want


def _generic(va, seed):
    """fp32 values fx has to round: the case generators' sixteenths times a random factor"""
    rng = np.random.default_rng(seed)
    return (va * (0.5 + rng.random(va.size)).astype(F32)).astype(F32)


# ---- bitmap edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049])
def test_bitmap_edges(n_rows):
    V, B = 50, 3
    rng = np.random.default_rng(n_rows)
    ip, ix, va = aref.csr_case(rng.integers(0, 13, size=n_rows), V, seed=n_rows, zeros=0.1)
    dev = _build(ip, ix, _generic(va, n_rows), V)
    cells = _cells(dev, V)
    masks = _masks(B, n_rows, n_rows + 1)
    masks[:, -1] = True                                                                # the last row is a member: the spare bits sit right behind it
    for bit0 in (0, 5, 37):
        _check(dev, cells, masks, bit0, what="sets")                                   # the last word's spare bits are all set
        _check(dev, cells, masks[:1], bit0, shared=True, what="shared")
    empty, full = np.zeros((B, n_rows), bool), np.ones((B, n_rows), bool)
    want = _check(dev, cells, empty, 5, what="empty")
    assert (want[0] == 0).all() and (want[1] == 0).all()
    want = _check(dev, cells, full, 37, what="full")
    assert (want[1] == n_rows).all()
    assert (_check_null(dev, cells)[0] == want[0][:1]).all()                           # words = NULL: every row set
    if n_rows >= 33:                                                                   # tombstones are read at bit 0 whatever bit0 is
        dead = np.unique(np.array([0, 31, 32, n_rows - 1]))
        live = np.ones(n_rows, bool)
        live[dead] = False
        dev.delete_rows(dead)
        for bit0 in (0, 5, 37):
            _check(dev, cells, masks, bit0, live=live, what="sets & live")
        assert (_check_null(dev, cells, live)[1] == n_rows - dead.size).all()


def test_an_all_zero_span_followed_by_a_set_row():
    V, n = 50, 2 * 2048 + 70
    rng = np.random.default_rng(11)
    ip, ix, va = aref.csr_case(rng.integers(1, 9, size=n), V, seed=12)
    dev = _build(ip, ix, _generic(va, 13), V)
    cells = _cells(dev, V)
    for rows in ([2048], [4096], [2047, 4096 + 69], [n - 1]):
        m = np.zeros((2, n), bool)
        m[0, rows] = True
        m[1, rows[-1]] = True
        for bit0 in (0, 37):
            want = _check(dev, cells, m, bit0, rpc=0, what=("span", rows))
            assert want[1].tolist() == [len(rows), 1] and (want[0][1] == cells.slice(rows[-1], rows[-1] + 1).rows_sum([1])).all()


# ---- stores ----------------------------------------------------------------------------------------------------------------------------------------
EDGE = [2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), 2.0 ** -24, 0.0, -0.0, np.nan, 2.0 ** 20, -(2.0 ** 20), 2.0 ** 21, -(2.0 ** 21), np.inf, -np.inf]
EDGE_FX = [0, 2, 0, 1, 0, 0, 0, 1 << 44, -(1 << 44), 1 << 44, -(1 << 44), 1 << 44, -(1 << 44)]
RAGGED = [0, 1, 7, 8, 9, 768]


def test_fp32_store_with_every_fx_edge_value():
    V = 1000
    lens = np.array(RAGGED + [len(EDGE)] + [5] * 40)
    ip, ix, va = aref.csr_case(lens, V, seed=21)
    va = _generic(va, 22)
    r = len(RAGGED)
    ix[ip[r]:ip[r + 1]] = 3 * np.arange(len(EDGE))                                      # row 6: edge value j in column 3 j
    va[ip[r]:ip[r + 1]] = np.array(EDGE, dtype=F32)
    dev = _build(ip, ix, va, V)
    gi, gx, gv = _rows(dev)
    assert (ref.fx(np.array(EDGE, dtype=F32)) == EDGE_FX).all()
    stored = dict(zip(gx[gi[r]:gi[r + 1]].tolist(), gv[gi[r]:gi[r + 1]].view(np.uint32).tolist()))
    for j, v in enumerate(EDGE):                                                       # the builder keeps every non-zero edge value bit for bit
        if v != 0:
            assert stored[3 * j] == int(np.array(v, dtype=F32).view(np.uint32)) or np.isnan(v), j
    cells = ref.Cells(gi, gx, gv, V)
    _check_null(dev, cells)
    one = np.zeros((1, lens.size), bool)
    for row in range(len(RAGGED) + 1):                                                 # every ragged shape alone: its sums are the row itself
        one[:] = False
        one[0, row] = True
        w = _check(dev, cells, one, 5, shared=True, what=("row", row))
        assert w[1][0] == 1 and (w[0][0] == cells.slice(row, row + 1).rows_sum([1])).all()
        if row == r:                                                                   # the edge values alone: their sums by hand
            assert [int(w[0][0, 3 * j]) for j in range(len(EDGE))] == EDGE_FX and np.count_nonzero(w[0][0]) == sum(1 for x in EDGE_FX if x)
    _check(dev, cells, _masks(3, lens.size, 23), 37, what="fp32")
    _check(dev, cells, _masks(3, lens.size, 23), 0, tc=7, what="fp32, 143 tiles")
    # 2^19 saturated rows fill an int64 to the brim: the id list names the +inf row 2^19 - 1 times and the sum is still exact
    ids = np.full((1, (1 << 19) - 1), r, dtype=np.int64)
    rc, s, t = _raw_ids(dev, V, ids, 0, 1, True)
    col = 3 * EDGE.index(np.inf)
    assert rc == nat.VS_OK and int(s[0, col]) == (1 << 63) - (1 << 44) and int(t[0]) == (1 << 19) - 1
    assert int(s[0, 3 * EDGE.index(-np.inf)]) == -(1 << 63) + (1 << 44)


@pytest.mark.parametrize("store", ["fp16", "bin"])
def test_fp16_and_binary_stores(store):
    V = 1000
    lens = np.array(RAGGED + [4] + [6] * 40)
    ip, ix, va = aref.csr_case(lens, V, seed=31, zeros=0.1)                             # sixteenths: fp16-exact, with stored +0.0 and -0.0
    r = len(RAGGED)
    va[ip[r]:ip[r + 1]] = np.array([2.0 ** -24, -(2.0 ** -24), 65504.0, 2.0 ** -14], dtype=F32)    # fp16's smallest subnormal, largest, smallest normal
    dev = _build(ip, ix, va, V, store)
    gi, gx, gv = _rows(dev)
    cells = ref.Cells(gi, gx, gv, V)
    want = _check_null(dev, cells)
    if store == "fp16":
        cols = ix[ip[r]:ip[r + 1]]
        row = cells.slice(r, r + 1).rows_sum([1])
        assert row[cols].tolist() == [1, -1, 65504 << 24, 1 << 10]
        assert (want[0][0] == ref.Cells(ip, ix, va, V).rows_sum(np.ones(lens.size))).all()      # exact: the input's own fixed-point sums
    else:
        counts = dev.term_counts()
        assert (_np(counts.counts) * ONE == want[0]).all() and (_np(counts.total) == want[1]).all()
    masks = _masks(3, lens.size, 32)
    masks[:, :len(RAGGED) + 1] = True
    _check(dev, cells, masks, 5, what=store)
    _check(dev, cells, masks, 37, tc=8, what=store)


def test_signed_data_whose_column_sum_cancels_to_zero():
    V, n = 40, 130
    rng = np.random.default_rng(41)
    x = _generic(np.ones(n // 2, F32), 42) * 1000
    ip = np.arange(0, 2 * n + 1, 2, dtype=np.int64)
    ix = np.tile(np.array([7, 39], dtype=np.int32), n)
    va = np.empty(2 * n, F32)
    va[0::2] = np.concatenate([x, -x])[rng.permutation(n)]                              # column 7: every value and its negative
    va[1::2] = 1.0
    dev = _build(ip, ix, va, V)
    cells = _cells(dev, V)
    for tc in (0, 8):
        want = _check_null(dev, cells, tc=tc)
        assert int(want[0][0, 7]) == 0 and int(want[0][0, 39]) == n * ONE and np.abs(cells.fx).max() > ONE


# ---- tiles ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 7, 8, 18431, 18432, 18433, 29523, 65535])
def test_automatic_tiles(V):
    n, B = 300, 3
    rng = np.random.default_rng(V)
    lens = rng.integers(0, min(V, 40) + 1, size=n)
    lens[:2] = (min(V, 40), 0)
    ip, ix, va = aref.csr_case(lens, V, seed=V + 1, zeros=0.05, hot=V - 1)              # every non-empty row carries the last column
    ix[ip[0]] = 0                                                                      # ... and row 0 the first one
    dev = _build(ip, ix, _generic(va, V + 2), V)
    cells = _cells(dev, V)
    tiles, tile_cols = term_sum_plan(n, B, V, True)[:2]
    assert tiles == -(-V // TILE) and tiles * tile_cols >= V
    masks = _masks(B, n, V + 2)
    masks[:, 0] = True
    want = _check(dev, cells, masks, 37, what="columns")
    assert (want[0][:, V - 1] != 0).any()
    ids = np.tile(np.arange(n, dtype=np.int64), (2, 1))
    for on_dev in (False, True):
        rc, s, t = _raw_ids(dev, V, ids, 0, 1, on_dev)
        assert rc == nat.VS_OK and (s[0] == cells.rows_sum(np.ones(n))).all() and (s[1] == s[0]).all() and (t == n).all()
    # a hot column: every row stores the same single column -- inside a tile, and as the last column of the index
    for hot in sorted({V // 3, V - 1}):
        hip, hix, hva = np.arange(n + 1, dtype=np.int64), np.full(n, hot, np.int32), _generic(np.ones(n, F32), hot)
        hd = _build(hip, hix, hva, V)
        hc = _cells(hd, V)
        w = _check(hd, hc, np.ones((B, n), bool), 0, what=("hot", hot), kinds=(True,))
        assert (w[0][:, hot] == ref.fx(hva).sum()).all() and (w[0].sum(axis=1) == w[0][:, hot]).all()


@pytest.mark.parametrize("tc", [1, 7, 8, 40])
def test_explicit_tiles_cut_through_packets(tc):
    """V = 40: a row of 40 cells is 5 packets of 8 ascending ids; tiles of 7 cut inside packets, tiles of 1 leave most lanes with no id inside"""
    V, n, B = 40, 200, 3
    rng = np.random.default_rng(tc)
    lens = rng.integers(0, V + 1, size=n)
    lens[:4] = (40, 39, 8, 0)
    ip, ix, va = aref.csr_case(lens, V, seed=50 + tc, zeros=0.05)
    dev = _build(ip, ix, _generic(va, 51), V)
    cells = _cells(dev, V)
    assert term_sum_plan(n, B, V, True, 0, tc)[:2] == (-(-V // tc), tc)
    masks = _masks(B, n, 52)
    masks[:, :4] = True
    for bit0 in (0, 37):
        _check(dev, cells, masks, bit0, tc=tc, what="tiles")
    _check_null(dev, cells, tc=tc)
    ids = rng.integers(-1, n, size=(B, 70)).astype(np.int64)
    for on_dev in (False, True):
        rc, s, t = _raw_ids(dev, V, ids, 0, 1, on_dev, tc=tc)
        w = ref.term_sums_ids(ids, 0, cells)
        assert rc == nat.VS_OK and (s == w[0]).all() and (t == w[1]).all()


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------------
_big = {}


def _big_index():
    if not _big:
        V, n = 9000, 4 * 2048
        rng = np.random.default_rng(77)
        ip, ix, va = aref.csr_case(rng.integers(0, 13, size=n), V, seed=78, zeros=0.05)
        _big["case"] = (ip, ix, _generic(va, 79), V)
    return _big["case"]


@pytest.mark.parametrize("n_rows,chunks", [(3 * 2048 + 1, 4), (4 * 2048, 4)])
def test_the_result_never_depends_on_the_plan(n_rows, chunks):
    ip, ix, va, V = _big_index()
    dev = _build(ip[:n_rows + 1], ix[:ip[n_rows]], va[:ip[n_rows]], V)
    cells = _cells(dev, V)
    assert term_sum_plan(n_rows, 9, V, True, 2048, 4096) == (3, 4096, chunks, 2048) and term_sum_plan(n_rows, 9, V, True, 64)[:3] == (1, V, (n_rows + 63) // 64)
    for B in (1, 2, 9):
        masks = _masks(B, n_rows, B + 20, density=0.7)
        masks[:, -1] = True                                                            # the one-row chunk holds a member
        res = [_check(dev, cells, masks, 37 if B == 2 else 0, rpc=rpc, tc=tc, what=("plan", B), kinds=(False, True) if B == 2 else (True,))
               for rpc in (64, 2048, 0) for tc in (0, 4096)]
        for r in res[1:]:
            assert all((a == b).all() for a, b in zip(r, res[0]))
    shared = _masks(1, n_rows, 31, density=0.5)
    for bit0 in (0, 37):
        _check(dev, cells, shared, bit0, shared=True, rpc=2048, tc=4096, what="shared")


# ---- id lists --------------------------------------------------------------------------------------------------------------------------------------
_ids_case = {}


def _ids_index():
    if not _ids_case:
        n, V = 1000, 2000
        ip, ix, va = rref.csr_case(n, V, seed=1043)
        dev = DeviceIndex.from_csr(ip, ix, va, V, store_dtype=nat.VS_F32)
        dead = np.array([3, 64, 999])
        dev.delete_rows(dead)
        live = np.ones(n, bool)
        live[dead] = False
        _ids_case["case"] = (dev, _cells(dev, V), live, n, V)
    return _ids_case["case"]


@pytest.mark.parametrize("m", [1, 63, 64, 65, 1024])
def test_id_lists(m):
    dev, cells, live, n, V = _ids_index()
    B = 3
    rng = np.random.default_rng(m)
    ids = rng.integers(0, n, size=(B, m)).astype(np.int64)
    ids[rng.random((B, m)) < 0.2] = -1                                                 # padding anywhere in the list
    ids[0, 0] = 3                                                                      # a deleted id
    ids[1, -1] = ids[1, 0] = 7                                                         # a repeated id counts twice (m = 1: once)
    ids[2, m // 2] = 999
    off = 100_000
    want = ref.term_sums_ids(ids, 0, cells, live)
    assert want[1][1] >= min(m, 2) and want[1][0] < m
    for on_dev in (False, True):
        for o in (0, off):
            rc, s, t = _raw_ids(dev, V, ids + np.where(ids >= 0, o, 0), o, 1, on_dev, ld=m + 2, tc=0 if o else 512)
            assert rc == nat.VS_OK and (s == want[0]).all() and (t == want[1]).all(), (m, on_dev, o)
    # ids outside the index
    out = ids.copy()
    out[1, 0] = n
    out[2, -1] = -2
    want_out = ref.term_sums_ids(out, 0, cells, live)
    assert not ref.check_strict(out, 0, n)
    rc, s, t = _raw_ids(dev, V, out, 0, 1, False)
    assert rc == nat.VS_EINVAL and "outside" in nat.last_error()                       # strict, a host list
    for on_dev, strict in ((False, 0), (True, 0), (True, 1)):                          # skipped: not strict, or a device list
        rc, s, t = _raw_ids(dev, V, out, 0, strict, on_dev)
        assert rc == nat.VS_OK and (s == want_out[0]).all() and (t == want_out[1]).all(), (m, on_dev, strict)
    got = dev.term_sums(ids=ids)                                                       # the facade: host list in, tensors out
    assert isinstance(got, TermSums) and all((_np(g) == w).all() for g, w in zip(got, want))
    got = dev.term_sums(ids=torch.from_numpy(ids).cuda(), tile_cols=100)
    assert all((_np(g) == w).all() for g, w in zip(got, want))
    with pytest.raises(ValueError, match="outside"):
        dev.term_sums(ids=out)


# ---- mutations -----------------------------------------------------------------------------------------------------------------------------------
def _sparse_index(ip, ix, va, n, V):
    from vsearch_amd.ir import SparseIndex
    sp = SparseIndex(device="cuda:0", fp16=False)
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(va), size=(n, V))
    sp.move_to_device("cuda:0")
    return sp


def _eq(got, want):
    return all((_np(g) == w).all() for g, w in zip(got, want))


def test_deleted_rows_never_contribute_through_restore_compact_and_add():
    n, V = 600, 400
    ip, ix, va = rref.csr_case(n, V, seed=1042)
    cells = ref.Cells(ip, ix, va, V)
    sp = _sparse_index(ip, ix, va, n, V)
    every = ref.term_sums(None, 0, 0, cells)
    assert _eq(sp.term_sums(), every)
    dead = np.array([0, 5, 31, 32, 64, 500, 599])
    live = np.ones(n, bool)
    live[dead] = False
    sp.delete(dead)
    lw = ref.pack(live[None, :])[0]
    assert _eq(sp.term_sums(), ref.term_sums(None, 0, 0, cells, lw))
    masks = _masks(3, n, 9)
    masks[:, dead] = True                                                              # the set names the deleted rows: they still add nothing
    want = ref.term_sums(ref.pack(masks), 1, 0, cells, lw)
    got = sp.term_sums(filter=DocFilter.from_mask(torch.from_numpy(masks)))
    assert _eq(got, want) and (want[1] < masks.sum(axis=1)).all()
    ids = np.array([[0, 1, 5, 1, -1, 599, 2]], dtype=np.int64)                          # deleted ids are skipped, 1 counts twice
    got = sp.term_sums(ids=ids)
    assert _eq(got, ref.term_sums_ids(ids, 0, cells, live)) and int(got.total[0]) == 3
    sp.restore()
    assert _eq(sp.term_sums(), every)
    sp.delete(dead)
    old = _np(sp.compact())
    assert (old == np.flatnonzero(live)).all()
    after = ref.term_sums(None, 0, 0, cells, lw)
    after = (after[0], after[1])
    assert _eq(sp.term_sums(), after)
    new = torch.zeros(3, V)
    new[:, 5] = 1.0
    new[1, 7] = -2.5
    sp.add(new)
    want = (after[0].copy(), after[1] + 3)
    want[0][0, 5] += 3 * ONE
    want[0][0, 7] -= 5 * ONE // 2
    assert _eq(sp.term_sums(), want)
    sp.delete(np.array([n - dead.size]))                                               # the first added row
    want[0][0, 5] -= ONE
    assert (_np(sp.term_sums().sums) == want[0]).all()


# ---- top-n -----------------------------------------------------------------------------------------------------------------------------------------
def _topn_both(sums, total, n, counts=None, min_count=0):
    want = ref.topn(sums, total, n, counts, min_count)
    B, V = sums.shape
    for on_dev in (False, True):
        arrs = dict(sums=np.full((B, V + PAD), JUNK, np.int64), total=np.ascontiguousarray(total, dtype=np.int64),
                    cols=np.full((B, n), 77, np.int32), score=np.full((B, n), 7.0, F32), out=np.full((B, n), JUNK, np.int64))
        arrs["sums"][:, :V] = sums
        if counts is not None:
            arrs["counts"] = np.full((B, V + 1), JUNK, np.int64)
            arrs["counts"][:, :V] = counts
        arrs, ptr = _bufs(arrs, on_dev)
        nat.check(nat.lib().vs_term_sum_topn(ptr(arrs["sums"]), V + PAD, ptr(arrs["total"]), ptr(arrs["counts"]) if counts is not None else None, V + 1, B,
                                             V, n, min_count, ptr(arrs["cols"]), ptr(arrs["score"]), ptr(arrs["out"]), 0, None))
        got = tuple(_np(arrs[k]) for k in ("cols", "score", "out"))
        assert (got[0] == want[0]).all(), (n, min_count, on_dev, np.argwhere(got[0] != want[0])[:5])
        assert (got[1].view(np.uint32) == want[1].view(np.uint32)).all(), (n, on_dev)
        assert (got[2] == want[2]).all(), (n, on_dev)
    return want


@pytest.mark.parametrize("n", [1, 64, 65, 1024])
def test_topn_sizes(n):
    rng = np.random.default_rng(n)
    V = 3000
    sums = (rng.integers(-5, 40, size=(4, V)) * (ONE // 8)).astype(np.int64)           # few distinct means: many ties, zeros and negatives
    total = np.array([1000, 37, 0, 1 << 40], dtype=np.int64)                           # query 2: total = 0 lists nothing
    sums[3] = rng.integers(-(1 << 62), 1 << 62, size=V)                                # conversions that round: values above 2^53
    counts = rng.integers(0, 6, size=(4, V)).astype(np.int64)
    want = _topn_both(sums, total, n)
    assert (want[0][2] == -1).all() and np.isneginf(want[1][2]).all() and (want[0][0] >= 0).all() and (want[2][0] > 0).all()
    _topn_both(sums, total, n, counts, 3)
    got = term_sum_topn(torch.from_numpy(sums).cuda(), torch.from_numpy(total).cuda(), n, device=0)
    assert (_np(got[0]) == want[0]).all() and (_np(got[1]).view(np.uint32) == want[1].view(np.uint32)).all() and (_np(got[2]) == want[2]).all()


def test_topn_ties_floors_and_more_slots_than_columns():
    V = 200
    sums = np.full((2, V), 6 * ONE, dtype=np.int64)                                    # all scores equal: column ascending
    want = _topn_both(sums, [3, 3], 64)
    assert want[0][0].tolist() == list(range(64)) and (want[1] == 2.0).all()
    want = _topn_both(sums[:, :9], [3, 3], 20)                                         # n > n_cols
    assert want[0][0].tolist() == list(range(9)) + [-1] * 11
    # fp64 means that differ and round to the same fp32: the column decides, whatever the order of the sums
    s2 = np.array([[1 << 40, (1 << 40) + 1, (1 << 40) + 2]])
    assert _topn_both(s2, [1], 3)[0].tolist() == [[0, 1, 2]]
    assert _topn_both(s2[:, ::-1].copy(), [1], 3)[0].tolist() == [[0, 1, 2]]
    sums = np.array([[5 * ONE, 3 * ONE, 3 * ONE, -ONE, 0, 2 * ONE, 9 * ONE, 1]], dtype=np.int64)
    counts = np.array([[5, 3, 2, 9, 9, 0, 4, 1]], dtype=np.int64)
    assert _topn_both(sums, [10], 8)[0][0].tolist() == [6, 0, 1, 2, 5, 7, -1, -1]       # sum <= 0 is no candidate
    assert _topn_both(sums, [10], 8, None, 99)[0][0].tolist() == [6, 0, 1, 2, 5, 7, -1, -1]      # without counts min_count is not looked at
    assert _topn_both(sums, [10], 8, counts, 3)[0][0].tolist() == [6, 0, 1, -1, -1, -1, -1, -1]
    assert _topn_both(sums, [10], 8, counts, 0)[0][0].tolist() == [6, 0, 1, 2, 5, 7, -1, -1]
    assert _topn_both(sums, [10], 2, counts, 1)[0][0].tolist() == [6, 0]
    assert (_topn_both(sums, [0], 4)[0] == -1).all()                                   # total = 0


def test_topn_orders_sums_above_2_32():
    rng = np.random.default_rng(5)
    V = 65535
    sums = np.zeros((2, V), dtype=np.int64)
    big = rng.permutation(V)[:3000]
    sums[0, big] = (1 << 32) + rng.integers(0, 1 << 40, size=big.size)                 # a key saturating at 2^32 would tie all of them
    sums[0, big[:5]] = np.array([1 << 33, (1 << 33) + (1 << 12), 1 << 62, (1 << 62) + (1 << 40), (1 << 32) + 1])
    sums[1] = np.arange(V, dtype=np.int64) << 20                                       # ascending scores: every step admits new candidates
    want = _topn_both(sums, [7, 1 << 20], 1024)
    assert (want[2][0] > (1 << 32)).all() and (np.diff(want[1][0]) <= 0).all() and want[0][0, 0] == big[3] and want[0][0, 1] == big[2]
    assert want[0][1].tolist() == list(range(V - 1, V - 1025, -1))


# ---- shards ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_shards", [2, 3, 8])
def test_row_shards_equal_the_unsharded_index(n_shards):
    n, V, B = 1000, 2000, 5
    ip, ix, va = rref.csr_case(n, V, seed=1044)
    whole = DeviceIndex.from_csr(ip, ix, va, V, store_dtype=nat.VS_F32)
    cells = _cells(whole, V)
    rng = np.random.default_rng(n_shards)
    cuts = np.sort(rng.choice(np.arange(1, n), size=n_shards - 1, replace=False))
    cuts[0] = {2: 437, 3: 33, 8: 31}[n_shards]                       # no multiple of 32 at the first seam
    bounds = [0] + sorted(set(cuts.tolist())) + [n]
    shards = [whole.slice_rows(bounds[i], bounds[i + 1] - bounds[i], device=0) for i in range(len(bounds) - 1)]
    group = ShardGroup(shards)
    masks = _masks(B, n, 31)
    flt = DocFilter.from_mask(torch.from_numpy(masks))
    words = ref.pack(masks)
    ids = rng.integers(-1, n, size=(B, 70)).astype(np.int64)
    ids[:, :4] = (bounds[1] - 1, bounds[1], n - 1, bounds[1])          # the seam, one side of it twice
    dead = np.array([3, bounds[1] - 1, bounds[1], n - 1])
    live = np.ones(n, bool)
    try:
        for deleted in (False, True):
            if deleted:
                live[dead] = False
                group.delete_rows(dead)
                whole.delete_rows(dead)
            lw = ref.pack(live[None, :])[0]
            want = ref.term_sums(words, words.shape[1], 0, cells, lw)
            want_i = ref.term_sums_ids(ids, 0, cells, live)
            for obj in (group, whole):
                assert _eq(obj.term_sums(filter=flt), want)
                assert _eq(obj.term_sums(), ref.term_sums(None, 0, 0, cells, lw))
                for given in (ids, torch.from_numpy(ids).cuda()):
                    assert _eq(obj.term_sums(ids=given), want_i)
            counts = _np(whole.term_counts(filter=flt).counts)
            for min_count, cnt in ((0, None), (2, counts)):                            # the top-n is taken after the sum, never per shard
                wt = ref.topn(want[0], want[1], 8, cnt, min_count)
                for obj in (group, whole):
                    top = obj.top_weight_terms(filter=flt, topn=8, min_count=min_count)
                    assert isinstance(top, TopWeights) and (_np(top.cols) == wt[0]).all() and (_np(top.sums) == wt[2]).all()
                    assert (_np(top.scores).view(np.uint32) == wt[1].view(np.uint32)).all() and (_np(top.total) == want[1]).all()
        with pytest.raises(ValueError, match="outside"):
            group.term_sums(ids=np.array([[0, n]], dtype=np.int64))
    finally:
        group.restore_rows()
        group.close()


# ---- consistency with the term counts ----------------------------------------------------------------------------------------------------------------
def test_a_binary_index_sums_to_its_term_counts():
    n, V, B = 3000, 29523, 4
    rng = np.random.default_rng(61)
    ip, ix, _ = aref.csr_case(rng.integers(0, 60, size=n), V, seed=62, binary=True)
    dev = _build(ip, ix, None, V, "bin")
    masks = _masks(B, n, 63)
    flt = DocFilter.from_mask(torch.from_numpy(masks))
    for kw in (dict(filter=flt), dict(), dict(ids=torch.from_numpy(rng.integers(-1, n, size=(B, 200))).cuda())):
        s, c = dev.term_sums(**kw), dev.term_counts(**kw)
        assert (s.sums == c.counts * ONE).all() and (s.total == c.total).all() and int(s.total.sum()) > 0
    assert (_np(dev.term_sums(filter=flt).total) == masks.sum(axis=1)).all()


# ---- the facade -----------------------------------------------------------------------------------------------------------------------------------
def test_index_facade():
    n, V, B = 1000, 2000, 9
    ip, ix, va = rref.csr_case(n, V, seed=1045)
    q = rref.sparse_queries(B, V, seed=n + 2)
    S = rref.scores(q, ip, ix, va, "fp32")
    tq = torch.from_numpy(q)
    sp = _sparse_index(ip, ix, va, n, V)
    cells = ref.Cells(ip, ix, va, V)
    thr = np.array([np.sort(S[b])[::-1][150] for b in range(B)], dtype=F32)
    # q_embs + min_score: the set is match_filter's
    mf = sp.match_filter(tq, thr)
    w = _np(mf.words).view(np.uint32)
    want = ref.term_sums(w, w.shape[1], 0, cells)
    got = sp.term_sums(tq, thr)
    assert isinstance(got, TermSums) and _eq(got, want)
    assert (_np(got.total) == _np(sp.count_matches(tq, thr))).all() and (want[1] > 100).all()
    cen = sp.centroid(tq, thr)
    assert cen.dtype == torch.float32 and tuple(cen.shape) == (B, V)
    assert (_np(cen).view(np.uint32) == ref.mean(want[0], want[1]).view(np.uint32)).all()
    assert (_np(got.values()) == want[0].astype(np.float64) * 2.0 ** -24).all()
    res = sp.search(cen, 5)                                                            # a centroid is a query like any other
    assert tuple(res.ids.shape) == (B, 5) and (_np(res.ids) >= 0).all()
    counts = _np(sp.term_counts(tq, thr).counts)
    for min_count, cnt in ((0, None), (3, counts)):
        top = sp.centroid_terms(tq, thr, topn=12, min_count=min_count)
        wt = ref.topn(want[0], want[1], 12, cnt, min_count)
        assert isinstance(top, TopWeights) and (_np(top.cols) == wt[0]).all() and (_np(top.scores).view(np.uint32) == wt[1].view(np.uint32)).all()
        assert (_np(top.sums) == wt[2]).all() and (_np(top.total) == want[1]).all()
    # filter alone: B = 1
    cols = _np(sp.get_vectors(torch.tensor([3])).col_indices())
    col = int(cols[_np(sp.doc_freq(cols)).argmax()])
    visible = np.random.default_rng(42).random(n) < 0.7
    f = sp.term_filter(must=[col]) & DocFilter.from_mask(torch.from_numpy(visible))
    has = aref.has_matrix(ip, ix, va, V)
    allowed = (has[:, col] & visible)[None, :]
    want_f = ref.term_sums(ref.pack(allowed), 0, 0, cells)
    got = sp.term_sums(filter=f)
    assert _eq(got, want_f) and 0 < int(got.total[0]) < n
    assert (_np(sp.centroid(filter=f)).view(np.uint32) == ref.mean(want_f[0], want_f[1]).view(np.uint32)).all()
    assert (_np(sp.centroid_terms(filter=f, topn=3).cols) == ref.topn(want_f[0], want_f[1], 3)[0]).all()
    # ids = res.ids: the weight of a hit list
    res = sp.search(tq, 50)
    want_i = ref.term_sums_ids(_np(res.ids), 0, cells)
    got = sp.term_sums(ids=res.ids)
    assert _eq(got, want_i) and (_np(got.total) == 50).all()
    top = sp.centroid_terms(ids=res.ids, topn=10)
    wt = ref.topn(want_i[0], want_i[1], 10)
    assert (_np(top.cols) == wt[0]).all() and (_np(top.scores).view(np.uint32) == wt[1].view(np.uint32)).all()
    with pytest.raises(IndexError):
        sp.term_sums(ids=torch.tensor([[0, n]]))
    # nothing: every live document
    every = ref.term_sums(None, 0, 0, cells)
    assert _eq(sp.term_sums(), every) and int(sp.term_sums().total[0]) == n
    # an empty set: the centroid is the zero vector
    none = sp.centroid(filter=DocFilter.from_mask(torch.zeros(n, dtype=torch.bool)))
    assert tuple(none.shape) == (1, V) and (_np(none) == 0).all()
    # a row-sharded index gives the same answers
    one = tuple(_np(t) for t in sp.centroid_terms(tq, thr, topn=12, min_count=3))
    sp.shard_rows([0, 0, 0])
    assert sp.shards is not None and len(sp.shards) == 3
    assert _eq(sp.term_sums(tq, thr), want)
    assert _eq(sp.centroid_terms(tq, thr, topn=12, min_count=3), one)
    assert _eq(sp.term_sums(ids=res.ids), want_i)


def test_a_dense_index_on_the_matrix_cores_is_not_supported():
    mat = np.random.default_rng(3).random((64, 96)).astype(F32)
    dev = DeviceIndex.from_dense(mat)
    with pytest.raises(NotImplementedError):
        dev.term_sums()
    with pytest.raises(NotImplementedError):
        dev.term_sums(ids=np.array([[0, 1]], dtype=np.int64))
    with pytest.raises(NotImplementedError):
        dev.top_weight_terms(topn=3)


# ---- the retriever -----------------------------------------------------------------------------------------------------------------------------
def test_retriever_centroid_terms(tiny_retriever):
    from vsearch_amd.ir.retriever.index import IndexType
    r = tiny_retriever
    n = 80
    texts = make_texts(n, 5)
    r.build_index(texts, index_type=IndexType.SPARSE)
    idx = r.index
    queries = make_texts(4, 9)
    shift = int(r.encoder_p.config.shift_vocab_num)
    tokens = lambda cols: FakeTokenizer().convert_ids_to_tokens([int(c) + shift for c in cols])
    # k: the set is retrieve's hits
    hits = r.retrieve(queries, k=10)
    top = idx.centroid_terms(ids=hits.ids, topn=6, min_count=2)
    got = r.centroid_terms(queries, k=10, topn=6, min_count=2)
    assert len(got) == 4 and any(got)
    for b in range(4):
        cols = _np(top.cols)[b]
        keep = cols >= 0
        assert [t for t, _, _ in got[b]] == tokens(cols[keep])
        assert [(s, d) for _, s, d in got[b]] == list(zip(_np(top.scores)[b][keep].tolist(), _np(top.sums)[b][keep].tolist()))
        assert all(s > 0 and d > 0 for _, s, d in got[b]) and [s for _, s, _ in got[b]] == sorted((s for _, s, _ in got[b]), reverse=True)
    # min_score: the match set
    q_emb = r.process_query(queries, 0, r.encoder_q.config.topk)
    sc = _np(idx.explain(q_emb, torch.arange(n).repeat(4, 1), topn=0).scores).astype(F32)
    thr = np.array([np.unique(sc[b])[np.unique(sc[b]).size // 2] for b in range(4)], dtype=F32)
    got = r.centroid_terms(queries, min_score=thr, topn=5)
    top = idx.centroid_terms(q_emb, thr, topn=5)
    assert (_np(top.total) == _np(r.retrieve_range(queries, thr, max_hits=0).counts)).all()
    for b in range(4):
        assert [t for t, _, _ in got[b]] == tokens(_np(top.cols)[b][_np(top.cols)[b] >= 0])
    # the centroid of the hits, fed back into the search
    cen = idx.centroid(ids=hits.ids)
    again = idx.search(cen, k=3)
    assert tuple(again.ids.shape) == (4, 3)
