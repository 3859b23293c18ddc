"""GPU tests of the joined index (vs_index_concat; DeviceIndex.concat, ShardGroup.gathered, Index.concatenated / unsharded,
Retriever.merge_index) -- run on MI355X.

Every case compares export_csr of the new index with the numpy reference (tests/_concat_ref.py) of the sources' exports by array_equal on row
pointers, columns and value BITS (a NaN equal to any NaN); nnz and the packet count follow from the reference too, and every source's export is
bit-identical before and after.  Padding cells do not show in an export: they are compared through the .vsx file, which holds the packets as
they are.  Small indexes built from numpy CSR over a narrow vocabulary (V = 300), rows of 0 to 40 cells."""
import numpy as np
import pytest
import torch

import oracle
from conftest import V
from vsearch_amd import _native as nat
from vsearch_amd import device_index as di
from vsearch_amd.device_index import DeviceIndex, ShardGroup

import _concat_ref as ref

pytestmark = pytest.mark.gpu
VN = 300                                                 # the narrow vocabulary
STORES = {"fp32": nat.VS_F32, "fp16": nat.VS_F16, "binary": nat.VS_NONE}
NAMES = {v: k for k, v in STORES.items()}
LEGAL = [("fp32", "fp32"), ("fp32", "fp16"), ("fp16", "fp16"), ("fp16", "fp32"), ("binary", "binary"), ("binary", "fp32"), ("binary", "fp16")]


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------------------
def make_csr(lengths, n_cols, rng, values=None):
    """rows of the given lengths: distinct sorted columns, values standard normal (or values(n) -> float32 [n])"""
    ip = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ix = np.concatenate([np.sort(rng.permutation(n_cols)[:n]) for n in lengths] + [np.zeros(0, np.int64)]).astype(np.int64)
    d = np.concatenate([(rng.standard_normal(n) if values is None else values(n)).astype(np.float32) for n in lengths] + [np.zeros(0, np.float32)])
    return ip, ix, d.astype(np.float32)


def build(csr, n_cols=VN, store=nat.VS_F32):
    ip, ix, d = csr
    return DeviceIndex.from_csr(ip, ix, None if store == nat.VS_NONE else d, n_cols, store_dtype=store)


def lengths_of(rng, n_rows, first=None, last=None):
    l = rng.integers(0, 41, size=n_rows)
    if first is not None:
        l[0] = first
    if last is not None:
        l[-1] = last
    return l


def exported(src):
    """(indptr, indices, data | None) of a source as the reference takes it"""
    info = src.info()
    if info.n_rows == 0:
        return np.zeros(1, np.int64), np.zeros(0, np.int64), None if info.store_dtype == nat.VS_NONE else np.zeros(0, np.float32)
    ip, ix, d = src.export_csr()
    return ip, ix, None if info.store_dtype == nat.VS_NONE else d


def check(srcs, out=None, **extra):
    """join `srcs` and compare with the reference -> (the new DeviceIndex, the reference's CSR)"""
    before = [exported(s) for s in srcs]
    stores = [NAMES[int(s.info().store_dtype)] for s in srcs]
    new = srcs[0].concat(srcs[1:], dtype=out, **extra)
    for s, b in zip(srcs, before):
        assert ref.same_csr(exported(s), b), "a source changed"
    want = ref.concat_ref(before, out or ref.default_store(stores))
    got = new.export_csr()
    assert np.array_equal(got[0], want[0]), "row pointers"
    assert np.array_equal(got[1], want[1]), "columns"
    assert want[2] is None or ref.same_bits(got[2], want[2]), "value bits"
    info = new.info()
    lengths = np.diff(want[0])
    assert info.n_rows == len(lengths) and info.nnz == int(lengths.sum()) and info.n_packets == ref.packets_of(want[0])
    assert info.n_packets == sum(int(s.info().n_packets) for s in srcs) and info.nnz == sum(int(s.info().nnz) for s in srcs)
    assert info.store_dtype == STORES[out or ref.default_store(stores)] and info.n_cols == srcs[0].info().n_cols
    return new, want


def twin_of(want, store, n_cols=VN):
    return DeviceIndex.from_csr(want[0], want[1], want[2], n_cols, store_dtype=STORES[store])


def same_file(a, b, tmp_path):
    a.save_native(str(tmp_path / "a.vsx"))
    b.save_native(str(tmp_path / "b.vsx"))
    return (tmp_path / "a.vsx").read_bytes() == (tmp_path / "b.vsx").read_bytes()


def same_search(a, b, q, k):
    x, y = a.search(q, k), b.search(q, k)
    return torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])


def queries(seed, B=4):
    return torch.from_numpy(oracle.synth_queries(seed, B, VN, 30)).to("cuda:0")


# ---- source row counts: a live word and a ballot wave over one, two and three-plus sources ----------------------------------------------------------------
ROWS = [1, 31, 32, 33, 63, 64, 65, 129]


@pytest.fixture(scope="module")
def by_rows():
    """a source of every row count in every store; the first and the last row of each are empty in turn"""
    rng = np.random.default_rng(1)
    csrs = [make_csr(lengths_of(rng, n, first=0 if i % 2 else None, last=0 if i % 3 == 0 else None), VN, rng) for i, n in enumerate(ROWS)]
    return {name: [build(c, VN, store) for c in csrs] for name, store in STORES.items()}


@pytest.mark.parametrize("store,out", LEGAL)
def test_source_row_counts(by_rows, store, out):
    srcs = by_rows[store]
    check(srcs, out)                                                             # bases 1, 32, 64, 97, 160, 224, 289
    check(srcs[::-1], out)                                                       # 129, 194, 258, 321, 354, 386, 417
    rng = np.random.default_rng(2)
    for _ in range(3):
        check([srcs[i] for i in rng.permutation(len(srcs))], out)
    check([srcs[0]] * 5 + [srcs[1]], out)                                        # five one-row sources: a wave over many sources
    if out == store:
        check(srcs, None)                                                        # dtype=None keeps a common store


# ---- source packet totals: the four-step round and the uniform-step shortcut on either side of a boundary -----------------------------------------------
PACKETS = [1, 63, 64, 65, 255, 256, 257, 0]


def csr_of_packets(rng, total):
    """rows of 0 to 5 packets (the last cells of a row's last packet missing at random) with exactly `total` packets; 0: five empty rows"""
    if total == 0:
        return make_csr([0] * 5, VN, rng)
    lengths, left = [], total
    while left:
        p = int(min(left, rng.integers(0, 6)))
        lengths.append(0 if p == 0 else 8 * p - int(rng.integers(0, 8)))
        left -= p
    return make_csr(lengths, VN, rng)


@pytest.fixture(scope="module")
def by_packets():
    rng = np.random.default_rng(3)
    csrs = [csr_of_packets(rng, p) for p in PACKETS]
    out = {name: [build(c, VN, store) for c in csrs] for name, store in STORES.items()}
    for srcs in out.values():
        assert [int(s.info().n_packets) for s in srcs] == PACKETS
    return out


@pytest.mark.parametrize("store,out", LEGAL)
def test_source_packet_totals(by_packets, store, out):
    srcs = by_packets[store]
    check(srcs, out)                                                             # boundaries at 1, 64, 128, 193, 448, 704, 961
    check(srcs[::-1], out)                                                       # the source without packets first
    for i in range(len(srcs) - 1):                                               # every total as the first source of a pair, and alone
        check([srcs[i], srcs[(i + 3) % 7]], out)
        check([srcs[i]], out)
    check([srcs[5], srcs[5], srcs[7], srcs[5]], out)                             # boundaries on whole rounds: 256, 512


def test_empty_rows_first_and_last_in_a_source():
    rng = np.random.default_rng(4)
    a = build(make_csr([0, 5, 9, 0], VN, rng))
    b = build(make_csr([0, 0, 17, 0, 0], VN, rng), store=nat.VS_F16)
    c = build(make_csr([0], VN, rng), store=nat.VS_NONE)
    for srcs in ([a, b, c], [c, b, a], [c, c, a, c], [b, b]):
        check(srcs, "fp32")
        check(srcs, "fp16")
    new, _ = check([c, c], "binary")
    assert new.info().n_packets == 0 and new.n_rows == 2


def test_a_source_without_rows_in_every_place(by_rows):
    a, b = by_rows["fp32"][1], by_rows["fp16"][3]
    for store in STORES.values():
        e = DeviceIndex.reserved(4, 4, VN, store)                                # a reserved index nothing was appended to
        assert e.n_rows == 0
        for srcs in ([e, a, b], [a, e, b], [a, b, e], [e, e, a, e]):
            new, _ = check(srcs, "fp32")
            check(srcs, "fp16")
        assert new.n_rows == a.n_rows
    with pytest.raises(ValueError, match="empty join"):
        DeviceIndex.reserved(4, 4, VN, nat.VS_F32).concat([DeviceIndex.reserved(1, 1, VN, nat.VS_F16)])


def test_256_sources_one_and_the_same_three_times(by_rows):
    rng = np.random.default_rng(5)
    stores = [nat.VS_F32, nat.VS_F16, nat.VS_NONE]
    many = [build(make_csr(lengths_of(rng, int(rng.integers(1, 4))), VN, rng), store=stores[i % 3]) for i in range(256)]
    new, _ = check(many, "fp16")                                                 # a 256-packet round crosses dozens of sources
    assert 256 <= new.n_rows <= 768
    check(many, "fp32")
    check(many[0::3], "fp32")                                                    # 86 fp32 sources
    check(many[2::3], "binary")                                                  # 85 binary sources
    with pytest.raises(ValueError, match="at most 256"):
        many[0].concat(many)
    one = by_rows["fp16"][7]
    for out in ("fp16", "fp32"):
        new, _ = check([one], out)                                               # n_src = 1: a copy, or a conversion
    new, want = check([one, one, one], None)                                     # the same handle three times
    assert new.n_rows == 3 * one.n_rows and np.array_equal(want[1][:len(want[1]) // 3], want[1][len(want[1]) // 3:2 * len(want[1]) // 3])


# ---- mixed stores ----------------------------------------------------------------------------------------------------------------------------------------
def special_values(n):
    """fp32 values that are fp16 ties, subnormal in fp16, below its range, overflowing -- cycled to n"""
    u = 2.0 ** -11
    pool = np.array([1.0 + u, 1.0 + 3 * u, -(1.0 + u), 2049.0, 2051.0, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), 2.0 ** -14 - 2.0 ** -25,
                     1e-45, -1e-45, 65504.0, 65519.996, 65520.0, -65520.0, 1e30, np.inf, -np.inf, 0.0, -0.0, 0.333333], dtype=np.float32)
    return pool[np.arange(n) % len(pool)]


@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(6)
    a = build(make_csr(lengths_of(rng, 70), VN, rng, values=special_values), store=nat.VS_F32)
    b = build(make_csr(lengths_of(rng, 45), VN, rng), store=nat.VS_F16)
    c = build(make_csr(lengths_of(rng, 33, first=3), VN, rng), store=nat.VS_NONE)           # (rows of 3 cells: a packet that is mostly padding)
    return a, b, c


@pytest.mark.parametrize("out", ["fp32", "fp16"])
def test_mixed_stores(mixed, out, tmp_path):
    a, b, c = mixed
    for srcs in ([a, b, c], [c, a, b], [b, c, a, c]):
        new, want = check(srcs, out)
        # the file holds the packets as they are: a binary source's real cells are 1.0 and its padding cells (id n_cols, +0), as in an index built
        # from the joined CSR
        assert same_file(new, twin_of(want, out), tmp_path)
        assert same_search(new, twin_of(want, out), queries(1), 20)
    new, want = check([c, a], out)
    first = int(want[0][c.n_rows])
    assert np.array_equal(want[2][:first], np.ones(first, np.float32)) and np.array_equal(new.export_csr()[2][:first], np.ones(first, np.float32))
    assert check([a, b, c], None)[0].info().store_dtype == nat.VS_F32 and check([b, c], None)[0].info().store_dtype == nat.VS_F16


def test_nan_stays_nan(mixed):
    rng = np.random.default_rng(7)
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF], dtype=np.uint32).view(np.float32)
    a = build(make_csr(lengths_of(rng, 20, first=9), VN, rng, values=lambda n: np.where(np.arange(n) % 3 == 0, nans[np.arange(n) % 4], np.float32(1.5))))
    for out in ("fp16", "fp32"):
        new, want = check([mixed[1], a], out)
        assert np.isnan(want[2]).sum() > 20 and np.array_equal(np.isnan(new.export_csr()[2]), np.isnan(want[2]))


def test_all_binary_stays_binary_and_binarising_raises(mixed, by_rows, tmp_path):
    a, b, c = mixed
    new, want = check([c, by_rows["binary"][4], c], "binary")
    assert new.info().store_dtype == nat.VS_NONE
    assert same_file(new, DeviceIndex.from_csr(want[0], want[1], None, VN), tmp_path)
    assert check([c, c], None)[0].info().store_dtype == nat.VS_NONE
    for srcs in ([c, a], [b, c]):
        with pytest.raises(ValueError, match="binarising"):
            srcs[0].concat(srcs[1:], dtype="binary")
    arr = (di.C.c_void_p * 2)(c._h, a._h)                                        # ... and through the C ABI
    h = di.C.c_void_p()
    assert nat.lib().vs_index_concat(arr, 2, nat.VS_NONE, 0, 0, 0, di.C.byref(h)) == nat.VS_EINVAL and "binarising is not covered" in nat.last_error()
    assert not h.value


# ---- round trips ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow():
    """2100 rows over 300 columns, lengths 0..119"""
    rng = np.random.default_rng(9)
    lengths = rng.integers(0, 120, size=2100)
    lengths[:4] = [0, 1, 8, 9]
    csr = make_csr(lengths, VN, rng)
    return csr, build(csr, VN), build(csr, VN, nat.VS_F16)


@pytest.mark.parametrize("a", [1, 64, 700, 2099])
def test_two_slices_give_back_the_source(narrow, a, tmp_path):
    csr, src, src16 = narrow
    n = src.n_rows
    for s, store in ((src, "fp32"), (src16, "fp16")):
        new, want = check([s.slice_rows(0, a), s.slice_rows(a, n - a)])
        assert ref.same_csr(new.export_csr(), s.export_csr())
        assert (new.info().nnz, new.info().n_packets, new.info().lanes_per_row) == (s.info().nnz, s.info().n_packets, s.info().lanes_per_row)
        assert same_file(new, twin_of(want, store), tmp_path) and new.n_live == n      # no tombstones: the file of an index built from the joined CSR


def test_search_equals_the_source_on_the_scan():
    n, B, k = 3000, 5, 100
    ip, ix, d = oracle.synth_csr(21, 0, n, V, 96)
    q = torch.from_numpy(oracle.synth_queries(23, B)).to("cuda:0")
    for store in (nat.VS_F32, nat.VS_F16, nat.VS_NONE):
        src = DeviceIndex.from_csr(ip, ix, None if store == nat.VS_NONE else d, V, store_dtype=store)
        src.set_option("blocked_postings", 0)
        new = src.slice_rows(0, 1001).concat([src.slice_rows(1001, 64), src.slice_rows(1065, n - 1065)])
        new.set_option("blocked_postings", 0)
        new.prepare()
        assert same_search(new, src, q, k) and new.info().last_path < 2 and src.info().last_path < 2


def test_search_equals_the_source_on_the_postings_copy():
    """rows long enough, and enough of them, that prepare() builds the new index's postings copy by the automatic rule"""
    n, nnz, B, k = 20_000, 300, 8, 100
    src = DeviceIndex.synthetic(5, 0, n, V, nnz)
    new = src.slice_rows(0, 7777).concat(src.slice_rows(7777, n - 7777)).prepare()
    info = new.info()
    assert info.postings_state == 1 and info.aux_bytes > 0
    q = torch.from_numpy(oracle.synth_queries(9, B)).to("cuda:0")
    got = new.search(q, k)
    assert new.info().last_path >= 2
    want = src.prepare().search(q, k)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- tombstones --------------------------------------------------------------------------------------------------------------------------------------------------
def live_of(srcs):
    return ref.concat_live([s.live_mask().cpu().numpy() if s.n_rows else np.zeros(0, bool) for s in srcs])


@pytest.mark.parametrize("sizes", [(31, 33, 64), (64, 31, 33), (33, 64, 31, 1)])
def test_tombstones_travel_with_the_rows(sizes):
    """deletions at a source's first and last row: the edges of the live words lie inside, at and across the sources' boundaries"""
    rng = np.random.default_rng(sum(sizes))
    srcs = [build(make_csr(lengths_of(rng, n), VN, rng)) for n in sizes]
    mid = [srcs[0], build(make_csr(lengths_of(rng, 40), VN, rng), store=nat.VS_F16), srcs[2]]
    mid[1].delete_rows(np.array([0, 17, 39], dtype=np.int64))                  # deletions in the middle source only
    new, _ = check(mid, "fp32")
    assert np.array_equal(new.live_mask().cpu().numpy(), live_of(mid)) and new.n_live == new.n_rows - 3
    for s in srcs:
        s.delete_rows(np.unique(np.array([0, s.n_rows - 1, s.n_rows // 2], dtype=np.int64)))
    new, want = check(srcs)
    live = live_of(srcs)
    assert np.array_equal(new.live_mask().cpu().numpy(), live) and new.n_live == int(live.sum()) == sum(s.n_live for s in srcs)
    q = queries(2)
    got, _ = new.search(q, new.n_rows)
    got = got.cpu().numpy()
    assert live[got[got >= 0]].all() and (got >= 0).sum() == 4 * new.n_live
    twin = twin_of(want, "fp32")
    twin.delete_rows(np.nonzero(~live)[0].astype(np.int64))
    assert same_search(new, twin, q, new.n_rows)
    new.restore_rows()                                                          # ... and they come back
    assert new.n_live == new.n_rows and same_search(new, twin_of(want, "fp32"), q, new.n_rows)
    assert all(s.n_live == s.n_rows - len({0, s.n_rows - 1, s.n_rows // 2}) for s in srcs)       # the sources keep their deletions


def test_without_deletions_there_is_no_bitmap(narrow, tmp_path):
    _, src, _ = narrow
    a, b = src.slice_rows(0, 100), src.slice_rows(100, 50)
    a.delete_rows(np.array([5], dtype=np.int64))
    a.restore_rows()                                                             # a bitmap with every bit set: no joined row is deleted
    new, want = check([a, b])
    assert new.n_live == 150 and same_file(new, twin_of(want, "fp32"), tmp_path)
    new.delete_rows(np.array([149], dtype=np.int64))                           # ... and the result takes deletions like any other
    assert new.n_live == 149 and not bool(new.live_mask()[149])


def test_spare_capacity_then_append(narrow):
    _, src, _ = narrow
    a, b = src.slice_rows(0, 33), src.slice_rows(33, 31)
    b.delete_rows(np.array([0, 30], dtype=np.int64))
    new, want = check([a, b], rows_extra=40, packets_extra=100)
    more = make_csr([5, 0, 70], VN, np.random.default_rng(12))
    new.append_csr(*more)                                                        # the appended rows are live
    assert new.n_rows == 67 and new.n_live == 65
    mask = new.live_mask().cpu().numpy()
    assert mask[64:].all() and not mask[33] and not mask[63] and mask[:33].all()
    got = new.export_csr()
    assert np.array_equal(got[1], np.concatenate([want[1], more[1]])) and ref.same_bits(got[2], np.concatenate([want[2], more[2]]))
    with pytest.raises(ValueError, match="exceeds the reserved"):
        check([a, b])[0].append_csr(*more)                                       # without the spare capacity there is no room


# ---- errors --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_sources_searching(narrow):
    _, src, _ = narrow
    q = queries(3)
    before = src.search(q, 20)
    wide = build(make_csr([3, 4], VN + 1, np.random.default_rng(13)), n_cols=VN + 1)
    with pytest.raises(ValueError, match="source 1 has 301 columns"):
        src.concat(wide)
    dense = DeviceIndex.from_dense(np.random.default_rng(14).standard_normal((8, VN)).astype(np.float32))
    assert dense.info().kind == nat.VS_KIND_DENSE and dense.info().n_packets == 0
    for srcs in ([src, dense], [dense, src]):
        with pytest.raises(NotImplementedError, match="dense \\(matrix\\) index"):
            srcs[0].concat(srcs[1:])
    with pytest.raises(NotImplementedError, match="2\\^32"):                     # by the plan only: nothing of that size is built
        di.concat_plan([1 << 31, 1 << 31], [5, 5], VN, [nat.VS_F32] * 2, nat.VS_F32)
    with pytest.raises(NotImplementedError, match="2\\^32"):
        src.concat(src, rows_extra=1 << 32)
    for bad in (dict(rows_extra=-1), dict(packets_extra=-1)):
        with pytest.raises(ValueError):
            src.concat(src, **bad)
    with pytest.raises(TypeError):
        src.concat([3])
    p = src.concat_plan([src, src])
    assert p.rows == 3 * src.n_rows and p.packets == 3 * src.info().n_packets
    after = src.search(q, 20)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


def test_dense_stored_as_packets_joins_like_any_other():
    rng = np.random.default_rng(8)
    mats = [(rng.standard_normal((n, 256)) * (rng.random((n, 256)) < 0.2)).astype(np.float32) for n in (70, 33)]
    a, b = [DeviceIndex.from_dense(m, max_density=1.0) for m in mats]
    assert a.info().kind == nat.VS_KIND_DENSE and a.info().n_packets > 0
    new = a.concat(b)
    assert new.info().kind == nat.VS_KIND_DENSE and np.array_equal(new.export_dense(np.float32), np.concatenate(mats))
    ip, ix, d = a.export_csr()
    sparse = DeviceIndex.from_csr(ip, ix, d, 256)
    assert sparse.concat(b).info().kind == nat.VS_KIND_CSR                       # dense only when every source is


# ---- another GPU, and the shard group ------------------------------------------------------------------------------------------------------------------------------
def test_gathered_equals_the_unsharded_index(narrow, tmp_path):
    csr, src, _ = narrow
    n = src.n_rows
    cuts = [0, 700, 1500, n]
    group = ShardGroup([src.slice_rows(cuts[i], cuts[i + 1] - cuts[i], device=0) for i in range(3)])
    group.delete_rows(np.array([0, 699, 700, 2099], dtype=np.int64))
    whole = group.gathered()
    assert isinstance(whole, DeviceIndex) and ref.same_csr(whole.export_csr(), src.export_csr()) and whole.n_live == n - 4
    assert whole.live_mask().cpu().numpy().tolist() == [i not in (0, 699, 700, 2099) for i in range(n)]
    assert same_search(whole, group, queries(4), 30)
    half = group.gathered(dtype="fp16")
    assert half.info().store_dtype == nat.VS_F16 and ref.same_bits(half.export_csr()[2], ref.to_f16(csr[2]))
    assert group.n_rows == n and group.n_live == n - 4                           # the group is untouched


def test_onto_another_gpu(narrow):
    if nat.device_count() < 2:
        pytest.skip("one GPU")
    csr, src, _ = narrow
    a, b = src.slice_rows(0, 900), src.slice_rows(900, 1200)
    b.delete_rows(np.array([0, 1199], dtype=np.int64))
    new, _ = check([a, b], device=1, rows_extra=2, packets_extra=2)
    assert new.device == 1 and new.n_live == 2098 and not bool(new.live_mask()[900]) and not bool(new.live_mask()[2099])
    group = ShardGroup([src.slice_rows(0, 1000, device=0), src.slice_rows(1000, 1100, device=1)])
    for device in (0, 1):
        whole = group.gathered(device=device)
        assert whole.device == device and ref.same_csr(whole.export_csr(), src.export_csr())


# ---- the facade ------------------------------------------------------------------------------------------------------------------------------------------------------
def _eq(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor):
        return a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())
    return a == b


def make_index(csr, seed, cls=None, named=True, tag="doc"):
    from vsearch_amd.ir import BoTIndex, SparseIndex
    cls = cls or SparseIndex
    ip, ix, d = csr
    n = len(ip) - 1
    rng = np.random.default_rng(seed)
    sp = cls(device="cuda:0")
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix), torch.ones(len(d)) if cls is BoTIndex else torch.from_numpy(d), size=(n, VN))
    sp.move_to_device("cuda:0")
    sp.data = [{"text": f"{tag} {i}"} for i in range(n)]
    sp.set_groups(np.arange(n) // 3)
    sp.set_facet("lang", rng.integers(-1, 5, size=n), names=["a", "b", "c", "d", "e"] if named else None)
    year = (1990 + rng.integers(0, 30, size=n)).astype(np.float32)
    year[::17] = np.nan
    sp.set_values("year", year)
    sp.set_values("pos", np.arange(n, dtype=np.int32))
    return sp


def cut(csr, r0, r1):
    ip, ix, d = csr
    return ip[r0:r1 + 1] - ip[r0], ix[ip[r0]:ip[r1]], d[ip[r0]:ip[r1]]


def test_facade_concatenated_carries_everything(narrow):
    from vsearch_amd.ir import BoTIndex, SparseIndex
    csr = narrow[0]
    a, b, c = make_index(cut(csr, 0, 100), 1, tag="a"), make_index(cut(csr, 100, 133), 2, tag="b"), make_index(cut(csr, 133, 400), 3, tag="c")
    b.delete([0, 32])
    q = queries(5)
    before = [x.search(q, 10) for x in (a, b, c)]
    new = a.concatenated(b, c)
    assert type(new) is SparseIndex and new is not a and new.parts.tolist() == [0, 100, 133, 400] and a.parts is None
    assert len(new) == 400 and new.n_live == 398 and new.source_ids is None
    assert ref.same_csr(new._device_index().export_csr(), cut(csr, 0, 400))
    assert [new.get_sample(j)["text"] for j in (0, 99, 100, 132, 133, 399)] == ["a 0", "a 99", "b 0", "b 32", "c 0", "c 266"]
    assert torch.equal(new.groups, torch.cat([a.groups, b.groups, c.groups]))
    assert torch.equal(new._facet_field("lang")[0], torch.cat([x._facet_field("lang")[0] for x in (a, b, c)])) and new.facet_names("lang") == ["a", "b", "c", "d", "e"]
    for name in ("year", "pos"):
        assert _eq(new.get_values(name), torch.cat([x.get_values(name) for x in (a, b, c)]))
    counts = new.facets("lang", topn=None)
    parts = [x.facets("lang", topn=None) for x in (a, b, c)]
    assert torch.equal(counts.counts, sum(p.counts for p in parts))            # the deleted documents of b do not count
    whole = build(cut(csr, 0, 400))
    whole.delete_rows(np.array([100, 132], dtype=np.int64))
    got, want = new.search(q, 50), whole.search(q, 50)
    assert torch.equal(got.ids, want[0]) and torch.equal(got.scores, want[1])
    new.set_facet("other", np.zeros(400, dtype=np.int64))                      # the registries are the new index's own
    assert "other" in new.facet_fields and "other" not in a.facet_fields
    for x, r in zip((a, b, c), before):                                         # the sources answer exactly as before
        again = x.search(q, 10)
        assert torch.equal(again.ids, r.ids) and torch.equal(again.scores, r.scores)
    assert b.n_live == 31 and len(a) == 100
    # without names n_labels is the maximum; a BoTIndex joined with a valued index comes back a SparseIndex, all bag-of-token a BoTIndex
    u, v = make_index(cut(csr, 0, 40), 4, BoTIndex, named=False), make_index(cut(csr, 40, 90), 5, named=False)
    u._facets["lang"] = (u._facets["lang"][0], 7, None)
    both = u.concatenated(v)
    assert type(both) is SparseIndex and both._facet_field("lang")[1] == 7 and both._device_index().info().store_dtype != nat.VS_NONE
    assert np.array_equal(both._device_index().export_csr()[2][:int(cut(csr, 0, 40)[0][-1])], np.ones(int(cut(csr, 0, 40)[0][-1]), np.float32))
    bots = u.concatenated(u)
    assert type(bots) is BoTIndex and bots._device_index().info().store_dtype == nat.VS_NONE and len(bots) == 80
    v.data = None                                                                # one source without texts in memory: no text store
    assert u.concatenated(v).data is None and len(u.concatenated(v)) == 0
    v.set_values("year", None)
    with pytest.raises(ValueError, match="value field 'year' is missing in source 1"):
        u.concatenated(v)


def test_facade_subsets_of_disjoint_filters_joined(narrow):
    sp = make_index(narrow[0], 6)
    sp.delete([7, 1500])
    years = sp.value_filter("year", 1995, 2004)
    lo, hi = sp.value_filter("pos", None, 999) & years, sp.value_filter("pos", 1000, None) & years
    joined = sp.subset(filter=lo).concatenated(sp.subset(filter=hi))
    want = sp.subset(filter=years)                                              # the ids ascend: the union in one piece
    assert len(joined) == len(want) and joined.parts.tolist() == [0, len(sp.subset(filter=lo)), len(want)]
    assert ref.same_csr(joined._device_index().export_csr(), want._device_index().export_csr())
    assert _eq(joined.get_values("pos"), want.source_ids.to(torch.int32)) and torch.equal(joined.groups, want.groups)
    q = queries(6)
    a, b = joined.search(q, 30), want.search(q, 30)
    assert torch.equal(a.ids, b.ids) and torch.equal(a.scores, b.scores)
    assert [joined.get_sample(j) for j in (0, len(want) - 1)] == [want.get_sample(j) for j in (0, len(want) - 1)]


def test_facade_unsharded_then_sorted_by(narrow):
    never, sp = make_index(narrow[0], 7), make_index(narrow[0], 7)
    dead = [0, 5, 77, 2099]
    never.delete(dead)
    sp.shard_rows([0, 0, 0])
    sp.delete(dead)
    with pytest.raises(NotImplementedError, match="shard"):
        sp.sorted_by("lang")
    with pytest.raises(NotImplementedError, match=r"unsharded\(\)"):
        never.concatenated(sp)
    one = sp.unsharded()
    assert one.shards is None and sp.shards is not None and len(sp.shards) == 3 and one.n_live == never.n_live == 2096
    assert ref.same_csr(one._device_index().export_csr(), never._device_index().export_csr())
    q = queries(7)
    a, b, c = one.search(q, 30), never.search(q, 30), sp.search(q, 30)
    assert torch.equal(a.ids, b.ids) and torch.equal(a.scores, b.scores) and torch.equal(a.ids, c.ids) and torch.equal(a.scores, c.scores)
    for field, desc in (("lang", False), ("year", True)):
        got, want = one.sorted_by(field, descending=desc), never.sorted_by(field, descending=desc)
        assert torch.equal(got.source_ids, want.source_ids)
        assert ref.same_csr(got._device_index().export_csr(), want._device_index().export_csr())
        assert _eq(got.get_values("year"), want.get_values("year")) and got.get_sample(3) == want.get_sample(3)
    with pytest.raises(ValueError, match="not row-sharded"):
        never.unsharded()


def test_retriever_merge_index(narrow):
    from vsearch_amd.ir import Retriever

    class Fake:                                  # (methods as class attributes: no reference cycle through the instance)
        merge_index = Retriever.merge_index
    csr = narrow[0]
    main, delta, more = make_index(cut(csr, 0, 500), 8), make_index(cut(csr, 500, 533), 9), make_index(cut(csr, 533, 540), 10)
    fake = Fake()
    fake.index, fake.device = main, "cuda"
    new = fake.merge_index(delta, inplace=False)
    assert fake.index is main and len(new) == 533 and new.parts.tolist() == [0, 500, 533]
    merged = fake.merge_index([delta, more])
    assert fake.index is merged and merged is not main and len(merged) == 540 and len(main) == 500
    assert ref.same_csr(merged._device_index().export_csr(), cut(csr, 0, 540))
