"""GPU tests of index pruning (vs_index_prune; DeviceIndex.prune, ShardGroup.prune, Index.pruned, Retriever.prune_index) -- run on MI355X.

Every case compares export_csr of the pruned index with the numpy reference (tests/_prune_ref.py) of export_csr of the source by array_equal on
row pointers, columns and value BITS; the kept counts, nnz and the packet count follow from the reference too, and the source's export is
bit-identical before and after.  Small indexes built from numpy CSR: V = 29 523, and V = 300 for the narrow cases."""
import types

import numpy as np
import pytest
import torch

import oracle
from conftest import V
from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, ShardGroup, prune_plan

import _prune_ref as ref

pytestmark = pytest.mark.gpu
VN = 300                                                 # the narrow vocabulary
REG = prune_plan(1, 1, V, nat.VS_F32)[0]                 # cells of the longest row selected from registers
STORES = {"fp32": nat.VS_F32, "fp16": nat.VS_F16}


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------------------
def make_csr(lengths, n_cols, rng, values=None):
    """rows of the given lengths: distinct sorted columns, values standard normal (or values(n) -> float32 [n])"""
    ip = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ix = np.concatenate([np.sort(rng.permutation(n_cols)[:n]) for n in lengths] + [np.zeros(0, np.int64)]).astype(np.int64)
    d = np.concatenate([(rng.standard_normal(n) if values is None else values(n)).astype(np.float32) for n in lengths] + [np.zeros(0, np.float32)])
    return ip, ix, d.astype(np.float32)


def build(csr, n_cols, store=nat.VS_F32):
    ip, ix, d = csr
    return DeviceIndex.from_csr(ip, ix, None if store == nat.VS_NONE else d, n_cols, store_dtype=store)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_csr(a, b, binary=False):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (binary or np.array_equal(bits(a[2]), bits(b[2])))


def col_mask(n_cols, keep_cols=None, drop_cols=None):
    if keep_cols is None and drop_cols is None:
        return None
    m = np.ones(n_cols, dtype=bool)
    if keep_cols is not None:
        if np.asarray(keep_cols).dtype == np.bool_:
            m = np.asarray(keep_cols).copy()
        else:
            m[:] = False
            m[np.asarray(keep_cols, dtype=np.int64)] = True
    if drop_cols is not None:
        m[np.asarray(drop_cols, dtype=np.int64)] = False
    return m


def check(src, protect=None, binary=False, topk=None, min_value=None, keep_cols=None, drop_cols=None, **extra):
    """prune `src` under the rules and compare with the reference -> (pruned DeviceIndex, the reference's CSR + kept)"""
    n_cols = int(src.info().n_cols)
    before = src.export_csr()
    out, kept = src.prune(topk=topk, min_value=min_value, keep_cols=keep_cols, drop_cols=drop_cols, protect=protect, **extra)
    assert same_csr(src.export_csr(), before), "the source changed"
    want = ref.prune_ref(before[0], before[1], None if binary else before[2], topk=topk, min_value=min_value,
                         col_keep=col_mask(n_cols, keep_cols, drop_cols), protect=None if protect is None else protect.export_csr()[:2])
    got = out.export_csr()
    assert np.array_equal(got[0], want[0]), "row pointers"
    assert np.array_equal(got[1], want[1]), "columns"
    if not binary:
        assert np.array_equal(bits(got[2]), bits(want[2])), "value bits"
    assert kept.dtype == np.int32 and np.array_equal(kept, want[3]), "kept counts"
    info = out.info()
    assert info.n_rows == src.info().n_rows and info.nnz == int(want[3].sum()) and info.n_packets == int(((want[3].astype(np.int64) + 7) // 8).sum())
    assert info.store_dtype == src.info().store_dtype and info.n_cols == n_cols
    return out, want


# ---- row lengths: the lane wrap, both paths and their boundary, one very long row ------------------------------------------------------------------
LENGTHS = [0, 1, 7, 8, 9, 511, 512, 513, REG - 1, REG, REG + 1, 2 * REG + 3, V, 0, 40]


@pytest.fixture(scope="module")
def long_rows():
    csr = make_csr(LENGTHS, V, np.random.default_rng(1))
    return {name: build(csr, V, store) for name, store in STORES.items()}


@pytest.mark.parametrize("store", list(STORES))
def test_row_lengths_and_m(long_rows, store):
    """m below, at and above the row lengths (n - 1, n, n + 1 of the 8-, 512- and reg_cells-cell rows), the widest m, and no cut"""
    assert REG >= 768
    for m in (1, 7, 8, 9, 511, 512, 513, REG - 1, REG, REG + 1, 2 * REG, 65535, 0, None):
        check(long_rows[store], topk=m)


@pytest.mark.parametrize("n_rows", [1, 4096, 4097, 8200])
def test_row_counts_cross_the_scan_block(n_rows):
    rng = np.random.default_rng(n_rows)
    src = build(make_csr(rng.integers(0, 21, size=n_rows), VN, rng), VN)
    out, want = check(src, topk=5)
    assert want[3].max() == 5 and (n_rows == 1 or want[3].min() == 0)
    # the scan from the kept counts to the row pointers at the packet edge: rows that keep 0, 8 and 9 cells (no packet, one, two), no cut
    lens = rng.choice([0, 8, 9], size=n_rows)
    lens[-1] = 9
    out, want = check(build(make_csr(lens, VN, rng), VN), topk=None)
    assert np.array_equal(want[3], lens) and np.array_equal(out.export_csr()[0], np.concatenate([[0], np.cumsum(lens)]))
    assert out.info().n_packets == int(((lens + 7) // 8).sum())


# ---- ties at the cut ---------------------------------------------------------------------------------------------------------------------------------
TIE_LENGTHS = [9, 100, 600, REG - 1, REG, REG + 1, 1500, 2 * REG + 3]


@pytest.mark.parametrize("store", list(STORES))
def test_ties_everywhere(store):
    """values from four levels: every cut falls inside a tie group -- across the packets of two lanes, across the 64-packet wrap, in rows of
    reg_cells and reg_cells + 1 cells (the register and the re-reading path); the earlier stored cell wins"""
    rng = np.random.default_rng(2)
    src = build(make_csr(TIE_LENGTHS, V, rng, values=lambda n: rng.integers(0, 4, size=n) - 1.0), V, STORES[store])
    for m in (1, 5, 8, 64, 300, 511, 512, 513, 1000, REG, 1400):
        check(src, topk=m)


def test_all_equal_rows_keep_the_first_m():
    rng = np.random.default_rng(3)
    src = build(make_csr(TIE_LENGTHS, V, rng, values=lambda n: np.full(n, 2.5)), V)
    for m in (1, 8, 9, 513, REG, REG + 1):
        out, want = check(src, topk=m)
        ip, ix, _ = src.export_csr()
        got = out.export_csr()
        for r, n in enumerate(TIE_LENGTHS):
            assert np.array_equal(got[1][got[0][r]:got[0][r + 1]], ix[ip[r]:ip[r] + min(m, n)])


def test_tie_group_at_chosen_places():
    """one tie group of the largest value at cells 5..20 (two lanes' packets), 505..530 (lane 63 to lane 0 of the next round) and 1015..1040 (a row
    of the re-reading path), cut inside"""
    rng = np.random.default_rng(4)
    rows = []
    for n, a, b in ((100, 5, 20), (REG, 505, 530), (REG + 300, 1015, 1040), (REG + 1, REG - 3, REG + 1)):
        v = (rng.random(n) * 0.5).astype(np.float32)
        v[a:b] = 7.0
        rows.append(v)
    it = iter(rows)
    src = build(make_csr([len(v) for v in rows], V, rng, values=lambda n: next(it)), V)
    for m in (1, 3, 4, 10, 12, 16, 25, 26, 40):
        check(src, topk=m)


def test_special_values():
    """+-0.0 tie, -inf < finite < +inf, a NaN ranks last and fails min_value, negative values, denormals"""
    rng = np.random.default_rng(5)
    pool = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, 2.5, 1e-40, -1e-40, 3.0, -3.0, 0.0, -0.0], dtype=np.float32)
    src = build(make_csr([14, 200, 700, REG + 50], V, rng, values=lambda n: pool[rng.integers(0, len(pool), size=n)] if n != 14 else pool), V)
    exported = src.export_csr()[2]
    assert np.isnan(exported).any() and np.isinf(exported).any() and (bits(exported) == 0x80000000).any()
    for m in (1, 2, 5, 9, 13, 100, 650):
        check(src, topk=m)
    for mv in (0.0, -0.0, -np.inf, np.inf, 1e-40, -2.0):
        check(src, min_value=mv)
        check(src, topk=7, min_value=mv)


def test_fp16_store_collapses_distinct_inputs():
    """fp32 inputs 1 + i * 1e-6 (half an fp16 ulp at 1 is 4.9e-4) are all 1.0 as halves: the fp16 store ranks by what it stores, so the first m
    cells stay"""
    rng = np.random.default_rng(6)
    it = iter([1.0 + np.arange(300) * 1e-6, 1.0 + np.arange(REG + 9)[::-1] * 1e-7])
    csr = make_csr([300, REG + 9], V, rng, values=lambda n: next(it))
    src = build(csr, V, nat.VS_F16)
    out, want = check(src, topk=10)
    got = out.export_csr()
    assert np.array_equal(got[1][:10], csr[1][:10]) and np.array_equal(got[1][10:], csr[1][300:310]) and (got[2] == 1.0).all()
    out32, _ = check(build(csr, V, nat.VS_F32), topk=10)                  # the fp32 store tells them apart
    assert np.array_equal(out32.export_csr()[1][:10], csr[1][290:300][np.argsort(csr[1][290:300])])


# ---- stores ------------------------------------------------------------------------------------------------------------------------------------------------
def test_binary_store_takes_col_keep_only():
    rng = np.random.default_rng(7)
    src = build(make_csr([0, 5, 86, 600, REG + 7, 3000], V, rng), V, nat.VS_NONE)
    assert src.info().store_dtype == nat.VS_NONE
    check(src, binary=True, keep_cols=np.arange(0, V, 3))
    check(src, binary=True, drop_cols=[0, 1, V - 1])
    check(src, binary=True)
    check(src, binary=True, keep_cols=[])
    for rules in (dict(topk=5), dict(min_value=0.5), dict(topk=5, keep_cols=[1, 2])):
        with pytest.raises(ValueError, match="binary"):
            src.prune(**rules)


def test_dense_indexes():
    """a dense index stored as packets is pruned like any CSR index and stays reported dense; the matrix-core kind is refused"""
    rng = np.random.default_rng(8)
    mat = (rng.standard_normal((70, 256)) * (rng.random((70, 256)) < 0.2)).astype(np.float32)
    as_csr = DeviceIndex.from_dense(mat, max_density=1.0)
    assert as_csr.info().kind == nat.VS_KIND_DENSE and as_csr.info().n_packets > 0
    out, _ = check(as_csr, topk=9)
    assert out.info().kind == nat.VS_KIND_DENSE
    with pytest.raises(NotImplementedError, match="dense"):
        DeviceIndex.from_dense(mat).prune(topk=9)


# ---- the rules -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow():
    """2100 rows over 300 columns; column 0 is in every non-empty row and is its largest value"""
    rng = np.random.default_rng(9)
    lengths = rng.integers(0, 120, size=2100)
    lengths[:4] = [0, 1, 8, 9]
    ip, ix, d = make_csr(lengths, VN, rng)
    for r in range(len(lengths)):
        if lengths[r]:
            ix[ip[r]:ip[r + 1]] = np.concatenate([[0], np.sort(1 + rng.permutation(VN - 1)[:lengths[r] - 1])])
            d[ip[r]] = 100.0
    return (ip, ix, d), build((ip, ix, d), VN), build((ip, ix, d), VN, nat.VS_F16)


def test_rules(narrow):
    csr, src, src16 = narrow
    for s in (src, src16):
        check(s, min_value=0.25)
        check(s, keep_cols=np.arange(0, VN, 2))
        out, want = check(s, topk=3, drop_cols=[0])                           # the dropped column is every row's largest
        assert not (want[1] == 0).any() and want[3].max() == 3
        keep = np.zeros(VN, dtype=bool)
        keep[::3] = True
        check(s, topk=4, min_value=-0.5, keep_cols=keep, drop_cols=[0, 3, 150])
        assert check(s, topk=1)[1][1].max() == 0                              # without the drop, the top 1 is column 0 everywhere


def test_rules_that_empty_every_row(narrow):
    csr, src, _ = narrow
    q = torch.from_numpy(oracle.synth_queries(1, 3, VN, 20)).to("cuda:0")
    for rules in (dict(min_value=1e9), dict(keep_cols=[]), dict(topk=5, drop_cols=np.arange(VN))):
        out, want = check(src, **rules)
        assert out.info().n_packets == 0 and out.info().nnz == 0 and want[3].sum() == 0
        ids, scores = out.search(q, 5)                                         # a query over empty rows returns without error
        assert ids.shape == (3, 5) and (scores.cpu().numpy() == 0).all()


# ---- protect -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_protect(narrow):
    csr, src, src16 = narrow
    ip, ix, d = csr
    rng = np.random.default_rng(10)
    n = len(ip) - 1
    # protect rows: a few of the row's own columns (inside and outside the top m), columns the row does not store, often longer than the row
    p_lengths = rng.integers(0, 200, size=n)
    pip, pix, pd = make_csr(p_lengths, VN, rng)
    binary = build((pip, pix, pd), VN, nat.VS_NONE)
    valued = build((pip, pix, np.zeros_like(pd)), VN)                          # any stored cell counts, whatever its value: here 0
    assert (np.diff(pip) > np.diff(ip)).any()
    for s in (src, src16):
        out, want = check(s, protect=binary, topk=5)
        assert (want[3] > 5).any() and (want[3] <= 5).any()
        check(s, protect=valued, topk=5)
        check(s, protect=binary, topk=2, drop_cols=[0, 7], min_value=-1.0)     # an ineligible protected cell is dropped
        check(s, protect=binary)                                               # no cut: protect adds nothing
    for bad in (build(make_csr(p_lengths[:-1], VN, rng), VN, nat.VS_NONE), build(make_csr(p_lengths, VN + 1, rng), VN + 1, nat.VS_NONE)):
        with pytest.raises(ValueError, match="protect"):
            src.prune(topk=5, protect=bad)
    with pytest.raises(TypeError, match="protect"):
        src.prune(topk=5, protect=(pip, pix))


def test_protect_long_rows():
    """protect on rows of both paths, protect rows of more than 64 packets"""
    rng = np.random.default_rng(11)
    lengths = [600, REG, REG + 1, 2 * REG + 3, 30, 0]
    src = build(make_csr(lengths, V, rng), V)
    prot = build(make_csr([700, 3, REG + 500, 40, 900, 10], V, rng), V, nat.VS_NONE)
    for m in (1, 29, 512, REG):
        check(src, protect=prot, topk=m)


# ---- tombstones, capacity, devices ----------------------------------------------------------------------------------------------------------------------------
def test_tombstones_are_carried(narrow):
    csr, _, _ = narrow
    src = build(csr, VN)
    n = src.n_rows
    dead = np.array([0, 5, 6, 7, 1000, n - 1], dtype=np.int64)
    src.delete_rows(dead)
    out, want = check(src, topk=6)                                             # deleted rows are pruned like the others
    assert out.n_live == n - len(dead) and torch.equal(out.live_mask(), src.live_mask())
    q = torch.from_numpy(oracle.synth_queries(2, 4, VN, 30)).to("cuda:0")
    ids, _ = out.search(q, 50)
    assert not np.isin(ids.cpu().numpy(), dead).any()
    out.restore_rows()                                                         # ... and come back pruned
    assert out.n_live == n and src.n_live == n - len(dead)
    twin = DeviceIndex.from_csr(want[0], want[1], want[2], VN)
    a, b = out.search(q, 50), twin.search(q, 50)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_spare_capacity_then_append(narrow):
    csr, src, _ = narrow
    out, want = check(src, topk=4, rows_extra=3, packets_extra=10)
    rng = np.random.default_rng(12)
    more = make_csr([5, 0, 70], VN, rng)
    out.append_csr(*more)
    got = out.export_csr()
    assert np.array_equal(got[0], np.concatenate([want[0], want[0][-1] + more[0][1:]]))
    assert np.array_equal(got[1], np.concatenate([want[1], more[1]])) and np.array_equal(bits(got[2]), bits(np.concatenate([want[2], more[2]])))
    q = torch.from_numpy(oracle.synth_queries(3, 4, VN, 30)).to("cuda:0")
    twin = DeviceIndex.from_csr(*got, VN)
    a, b = out.search(q, 20), twin.search(q, 20)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match="exceeds the reserved"):
        check(src, topk=4)[0].append_csr(*more)                               # without the spare capacity there is no room
    for bad in (dict(rows_extra=-1), dict(packets_extra=-1)):
        with pytest.raises(ValueError):
            src.prune(topk=4, **bad)


def test_onto_another_gpu(narrow):
    if nat.device_count() < 2:
        pytest.skip("one GPU")
    csr, _, _ = narrow
    src = build(csr, VN)
    src.delete_rows(np.array([3, 4], dtype=np.int64))
    out, _ = check(src, topk=4, device=1, rows_extra=2, packets_extra=2)
    assert out.device == 1 and out.n_live == src.n_rows - 2


# ---- search on the pruned index ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("postings", [1, 0])
def test_search_equals_the_index_built_from_the_reference(postings):
    """same cells, same order, same kernels: ids and scores equal with ==, on the postings copy and on the CSR scan"""
    n, B, k = 20000, 8, 100
    ip, ix, d = oracle.synth_csr(21, 0, n, V, 96)
    bp, bx, _ = oracle.synth_csr(22, 0, n, V, 40)
    q = torch.from_numpy(oracle.synth_queries(23, B)).to("cuda:0")
    for store, rules, with_protect in ((nat.VS_F32, dict(topk=32), False), (nat.VS_F16, dict(topk=24, min_value=0.0), True),
                                       (nat.VS_F32, dict(topk=50, drop_cols=np.arange(0, V, 7)), True)):
        src = DeviceIndex.from_csr(ip, ix, d, V, store_dtype=store)
        prot = DeviceIndex.from_csr(bp, bx, None, V) if with_protect else None
        out, want = check(src, protect=prot, **rules)
        twin = DeviceIndex.from_csr(want[0], want[1], want[2], V, store_dtype=store)
        for idx in (out, twin):
            idx.set_option("blocked_postings", postings)
        a, b = out.search(q, k), twin.search(q, k)
        assert out.info().last_path == twin.info().last_path and (out.info().last_path >= 2) == bool(postings)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- sharding -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_shard_group_of_uneven_shards(narrow):
    csr, src, _ = narrow
    rng = np.random.default_rng(13)
    n = src.n_rows
    prot = build(make_csr(rng.integers(0, 60, size=n), VN, rng), VN, nat.VS_NONE)
    cuts = [0, 700, 1500, n]
    group = ShardGroup([src.slice_rows(cuts[i], cuts[i + 1] - cuts[i], device=0) for i in range(3)])
    pgroup = ShardGroup([prot.slice_rows(cuts[i], cuts[i + 1] - cuts[i], device=0) for i in range(3)])
    whole, want = check(src, protect=prot, topk=5, drop_cols=[0])
    new, kept = group.prune(topk=5, drop_cols=[0], protect=pgroup)
    assert isinstance(new, ShardGroup) and new.n_rows == n and np.array_equal(kept, want[3])
    parts = [s.export_csr() for s in new._shards]
    assert [len(p[0]) - 1 for p in parts] == [700, 800, n - 1500]
    assert np.array_equal(np.concatenate([p[1] for p in parts]), want[1])
    assert np.array_equal(bits(np.concatenate([p[2] for p in parts])), bits(want[2]))
    assert np.array_equal(np.concatenate([np.diff(p[0]) for p in parts]), np.diff(want[0]))
    q = torch.from_numpy(oracle.synth_queries(4, 4, VN, 30)).to("cuda:0")
    a, b = new.search(q, 30), whole.search(q, 30)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match="protect"):
        group.prune(topk=5, protect=ShardGroup([prot.slice_rows(0, 800, device=0), prot.slice_rows(800, 700, device=0), prot.slice_rows(1500, n - 1500, device=0)]))
    with pytest.raises(TypeError, match="protect"):
        group.prune(topk=5, protect=prot)


# ---- the facade ------------------------------------------------------------------------------------------------------------------------------------------------------
def _eq(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor):
        return a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())
    return a == b


@pytest.fixture()
def sparse_index(narrow):
    from vsearch_amd.ir import SparseIndex
    ip, ix, d = narrow[0]
    n = len(ip) - 1
    sp = SparseIndex(device="cuda:0")
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix), torch.from_numpy(d), size=(n, VN))
    sp.move_to_device("cuda:0")
    sp.data = [{"text": f"doc {i}"} for i in range(n)]
    sp.set_groups(np.arange(n) // 3)
    sp.set_facet("lang", np.arange(n) % 5, names=["a", "b", "c", "d", "e"])
    sp.set_values("year", (1990 + np.arange(n) % 30).astype(np.float32))
    return sp


def test_facade_pruned_returns_a_new_index(sparse_index):
    from vsearch_amd.ir import SparseIndex
    sp = sparse_index
    n = len(sp)
    sp.delete([10, 11])
    before = sp._device_index().export_csr()
    new = sp.pruned(topk=4, drop_columns=[0])
    assert type(new) is SparseIndex and new is not sp and new._dev is not sp._dev and len(new) == n and new.n_live == n - 2
    assert same_csr(sp._device_index().export_csr(), before)                   # the source is left exactly as it was
    want = ref.prune_ref(*before, topk=4, col_keep=col_mask(VN, drop_cols=[0]))
    assert same_csr(new._device_index().export_csr(), want[:3])
    assert new.get_sample(7) == sp.get_sample(7) and torch.equal(new.groups, sp.groups)
    assert _eq(tuple(new.facets("lang")), tuple(sp.facets("lang")))
    assert _eq(tuple(new.value_stats("year")), tuple(sp.value_stats("year")))
    q = torch.from_numpy(oracle.synth_queries(5, 4, VN, 30)).to("cuda:0")
    twin = DeviceIndex.from_csr(*want[:3], VN)
    twin.delete_rows(np.array([10, 11], dtype=np.int64))
    res, (ids, scores) = new.search(q, 20), twin.search(q, 20)
    assert torch.equal(res.ids, ids) and torch.equal(res.scores, scores)
    new.set_facet("other", np.zeros(n, dtype=np.int64))                        # the registries are the new index's own
    assert "other" in new.facet_fields and "other" not in sp.facet_fields


def test_facade_max_df_and_protect(sparse_index):
    from vsearch_amd.ir import BoTIndex
    sp = sparse_index
    n = len(sp)
    counts = sp.term_counts().counts[0].cpu().numpy()
    assert counts[0] == (np.diff(sparse_index._device_index().export_csr()[0]) > 0).sum()
    limit = int(np.sort(counts)[-20])                                          # about twenty columns are more frequent
    for max_df, lim in ((limit, limit), (limit / n, limit / n * n)):
        new = sp.pruned(max_df=max_df)
        want = np.where(counts > lim, 0, counts)
        assert (want == 0).sum() > (counts == 0).sum() and np.array_equal(new.term_counts().counts[0].cpu().numpy(), want)
    rng = np.random.default_rng(14)
    pip, pix, _ = make_csr(rng.integers(0, 60, size=n), VN, rng)
    bot = BoTIndex(device="cuda:0")
    bot.vector = torch.sparse_csr_tensor(torch.from_numpy(pip), torch.from_numpy(pix), torch.ones(len(pix)), size=(n, VN))
    bot.move_to_device("cuda:0")
    new = sp.pruned(topk=3, protect=bot)
    before = sp._device_index().export_csr()
    assert same_csr(new._device_index().export_csr(), ref.prune_ref(*before, topk=3, protect=(pip, pix))[:3])
    with pytest.raises(TypeError, match="protect"):
        sp.pruned(topk=3, protect=(pip, pix))
    for bad in (1.5, 0.0, -1):
        with pytest.raises(ValueError, match="max_df"):
            sp.pruned(max_df=bad)


def test_facade_row_sharded(sparse_index):
    sp = sparse_index
    q = torch.from_numpy(oracle.synth_queries(6, 4, VN, 30)).to("cuda:0")
    want = sp.pruned(topk=4).search(q, 20)
    sp.shard_rows([0, 0, 0])
    new = sp.pruned(topk=4)
    assert new.shards is not None and len(new.shards) == 3 and new.shards[0] is not sp.shards[0] and torch.equal(new.groups, sp.groups)
    got = new.search(q, 20)
    assert torch.equal(got.ids, want.ids) and torch.equal(got.scores, want.scores)


def test_retriever_prune_index_resolves_tokens(sparse_index):
    from vsearch_amd.ir import Retriever
    shift = 999
    tok = types.SimpleNamespace(vocab={f"tok{i}": i for i in range(VN + shift)})

    class Fake:                                  # (methods as class attributes: no reference cycle through the instance)
        prune_index = Retriever.prune_index
    fake = Fake()
    fake.index, fake.device = sparse_index, "cuda"
    fake.encoder_p = types.SimpleNamespace(tokenizer=tok, config=types.SimpleNamespace(shift_vocab_num=shift))
    before = sparse_index._device_index().export_csr()
    new = fake.prune_index(topk=3, drop_tokens=[f"tok{shift}", 17], inplace=False)
    assert fake.index is sparse_index
    assert same_csr(new._device_index().export_csr(), ref.prune_ref(*before, topk=3, col_keep=col_mask(VN, drop_cols=[0, 17]))[:3])
    kept = fake.prune_index(keep_tokens=[f"tok{shift + 5}", f"tok{shift + 6}"])
    assert fake.index is kept and set(kept._device_index().export_csr()[1].tolist()) <= {5, 6}
    with pytest.raises(ValueError, match="tok5"):
        fake.prune_index(drop_tokens=["tok5"])


def test_facade_dense_matrix_index_is_refused():
    from vsearch_amd.ir import Index
    idx = Index(device="cuda:0")
    idx.vector = torch.randn(64, 128)
    idx.move_to_device("cuda:0")
    with pytest.raises(NotImplementedError, match="dense"):
        idx.pruned(topk=5)
