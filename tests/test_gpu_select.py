"""GPU tests of the sub-index (vs_index_select_rows; DeviceIndex.select_rows, ShardGroup.select_rows, Index.subset / sorted_by,
Retriever.subset_index / sort_index_by) -- run on MI355X.

Every case compares export_csr of the new index with the numpy reference (tests/_select_ref.py) of export_csr of the source by array_equal on
row pointers, columns and value BITS; nnz and the packet count follow from the reference too, and the source's export is bit-identical before
and after.  Small indexes built from numpy CSR: V = 29 523, and V = 300 for the narrow cases."""
import numpy as np
import pytest
import torch

import oracle
from conftest import V
from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, ShardGroup
from vsearch_amd.doc_filter import DocFilter

import _select_ref as ref

pytestmark = pytest.mark.gpu
VN = 300                                                 # the narrow vocabulary
STORES = {"fp32": nat.VS_F32, "fp16": nat.VS_F16, "binary": nat.VS_NONE}
SCAN = 4096                                              # ids of a scan block (block_scan.h: kScanRows)


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


def check(src, ids, **extra):
    """select `ids` of `src` and compare with the reference -> (the new DeviceIndex, the reference's CSR)"""
    before = src.export_csr()
    out = src.select_rows(ids, **extra)
    assert same_csr(src.export_csr(), before), "the source changed"
    host = ids.cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
    want = ref.select_ref(*before, host)
    got = out.export_csr()
    assert np.array_equal(got[0], want[0]), "row pointers"
    assert np.array_equal(got[1], want[1]), "columns"
    assert np.array_equal(bits(got[2]), bits(want[2])), "value bits"
    info, sinfo = out.info(), src.info()
    lengths = np.diff(want[0])
    assert info.n_rows == len(host) and info.nnz == int(lengths.sum()) and info.n_packets == int(((lengths + 7) // 8).sum())
    assert info.store_dtype == sinfo.store_dtype and info.n_cols == sinfo.n_cols and info.kind == sinfo.kind
    return out, want


def mapped(new_ids, ids):
    """the ids a search of the new index returns, as ids of the source (the padding -1 stays)"""
    ids = torch.as_tensor(ids, device=new_ids.device)
    return torch.where(new_ids >= 0, ids[new_ids.clamp(min=0)], new_ids)


# ---- stores and row lengths ------------------------------------------------------------------------------------------------------------------------
# 0, 1, the packet edge 7 / 8 / 9, exactly 64 packets, a row longer than one 64-packet gather step, the flagship row, more than one load group
LENGTHS = [0, 1, 7, 8, 9, 64 * 8, 65 * 8 + 1, 768, 0, 4 * 64 * 8 + 3, 40, 0]
NARROW_LENGTHS = [0, 1, 7, 8, 9, 64, 255, VN, 0, 33, 40, 0]


@pytest.fixture(scope="module")
def long_rows():
    csr = make_csr(LENGTHS, V, np.random.default_rng(1))
    return {name: build(csr, V, store) for name, store in STORES.items()}


@pytest.fixture(scope="module")
def short_rows():
    csr = make_csr(NARROW_LENGTHS, VN, np.random.default_rng(2))
    return {name: build(csr, VN, store) for name, store in STORES.items()}


@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("wide", [True, False])
def test_stores_and_row_lengths(long_rows, short_rows, store, wide):
    src = (long_rows if wide else short_rows)[store]
    n = src.n_rows
    rng = np.random.default_rng(3)
    check(src, np.arange(n))
    check(src, np.arange(n)[::-1].copy())
    check(src, rng.permutation(n))
    check(src, rng.integers(0, n, size=200))                                   # repeats, more than one 64-row run
    check(src, torch.from_numpy(rng.integers(0, n, size=70)).to("cuda:0"))     # ids on the device
    check(src, [6, 6, 6])                                                      # a list
    check(src, np.array([7, 0, 7], dtype=np.int32))                            # any integer width


# ---- the gather's edges ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 128])
def test_run_counts(long_rows, n):
    src = long_rows["fp32"]
    rng = np.random.default_rng(n)
    check(src, rng.integers(0, src.n_rows, size=n))
    check(src, np.full(n, 6))                                                  # the 521-cell row n times: every run crosses the step
    check(src, np.full(n, 0))                                                  # nothing but empty rows: an index without packets
    assert src.select_rows(np.full(n, 0)).info().n_packets == 0


def test_empty_rows_at_every_place_of_a_run(long_rows):
    src = long_rows["fp16"]
    e, rows = 0, [1, 4, 6, 7, 10, 3]
    ids = [e, e, e] + rows + [e] * 5 + rows                                    # at the start and in the middle of the first run
    ids += [e] * (64 - len(ids))                                               # ... and at its end
    ids += [e] * 64                                                            # the whole of the second run
    ids += rows + [e]                                                          # the last run ends on one
    assert len(ids) == 64 + 64 + 7
    check(src, np.array(ids))
    check(src, np.array([e] * 64 + [5]))                                       # an empty run first


def test_runs_whose_packets_are_a_multiple_of_64(long_rows, short_rows):
    one_packet = [1, 2, 3]                                                     # rows of 1, 7 and 8 cells of the wide source: one packet each
    out, _ = check(long_rows["fp32"], np.array([one_packet[i % 3] for i in range(64)] + [4, 6, 1]))
    assert out.info().n_packets == 64 + 2 + 66 + 1
    out, _ = check(long_rows["fp32"], np.array([5] + [0] * 63 + [7]))          # one row of exactly 64 packets fills the run
    assert out.info().n_packets == 64 + 96
    out, _ = check(long_rows["binary"], np.array([5, 5, 5, 5] + [0] * 60 + [5] * 8))      # 256 packets: exactly the loads of one group; then 512
    assert out.info().n_packets == 256 + 512
    check(short_rows["fp32"], np.array([5] * 8 + [0] * 56 + [1]))              # 8 rows of 8 packets


# ---- the scan's edges ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow():
    """2100 rows over 300 columns, lengths 0..119"""
    rng = np.random.default_rng(9)
    lengths = rng.integers(0, 120, size=2100)
    lengths[:4] = [0, 1, 8, 9]
    csr = make_csr(lengths, VN, rng)
    return csr, build(csr, VN), build(csr, VN, nat.VS_F16)


@pytest.mark.parametrize("n", [SCAN - 1, SCAN, SCAN + 1])
def test_id_counts_cross_the_scan_block(narrow, n):
    _, src, _ = narrow
    check(src, np.random.default_rng(n).integers(0, src.n_rows, size=n))


def test_more_than_1024_scan_blocks():
    """1024 x 4096 + 1 ids: the scan of the block sums takes a second round of 1024.  A 64-row binary source of one-packet rows: 4.2 M packets of
    16 bytes; the counts and the first and last 100 rows are checked"""
    rng = np.random.default_rng(10)
    lengths = rng.integers(1, 9, size=64)
    csr = make_csr(lengths, VN, rng)
    src = build(csr, VN, nat.VS_NONE)
    n = 1024 * SCAN + 1
    ids = torch.randint(0, 64, (n,), dtype=torch.int64, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(1))
    out = src.select_rows(ids)
    host = ids.cpu().numpy()
    info = out.info()
    assert info.n_rows == n and info.n_packets == n and info.nnz == int(lengths[host].sum())
    before = src.export_csr()
    for r0 in (0, n - 100):
        assert same_csr(out.slice_rows(r0, 100).export_csr(), ref.select_ref(*before, host[r0:r0 + 100]))


# ---- order ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_permutation_and_its_inverse_give_back_the_source(narrow):
    csr, src, src16 = narrow
    for s in (src, src16):
        perm = np.random.default_rng(11).permutation(s.n_rows)
        once, _ = check(s, perm)
        back, _ = check(once, np.argsort(perm))
        assert same_csr(back.export_csr(), s.export_csr())
        assert back.info().nnz == s.info().nnz and back.info().n_packets == s.info().n_packets


def test_repeats_are_kept(narrow):
    _, src, _ = narrow
    out, want = check(src, np.array([3, 3, 2, 3, 2, 1, 1]))                     # rows of 9, 8 and 1 cells
    ip = want[0]
    assert np.array_equal(want[1][ip[0]:ip[1]], want[1][ip[3]:ip[4]]) and ip[1] - ip[0] == ip[4] - ip[3] > 0
    q = torch.from_numpy(oracle.synth_queries(1, 3, VN, 30)).to("cuda:0")
    ids, sc = out.search(q, 7)
    by_row = torch.empty_like(sc).scatter_(1, ids, sc)
    assert torch.equal(by_row[:, 0], by_row[:, 1]) and torch.equal(by_row[:, 0], by_row[:, 3]) and torch.equal(by_row[:, 2], by_row[:, 4])


def test_a_range_equals_slice_rows(narrow):
    _, src, _ = narrow
    for r0, m in ((0, 1), (3, 64), (700, 1300), (0, src.n_rows)):
        out, _ = check(src, np.arange(r0, r0 + m))
        assert same_csr(out.export_csr(), src.slice_rows(r0, m).export_csr())


def test_the_old_ids_of_compact_give_compacts_index(narrow, tmp_path):
    csr, _, _ = narrow
    src = build(csr, VN)
    src.delete_rows(np.array([0, 5, 6, 7, 1000, src.n_rows - 1], dtype=np.int64))
    packed, old = src.compact()
    out = src.select_rows(old)
    assert same_csr(out.export_csr(), packed.export_csr())
    a, b = out.info(), packed.info()
    assert (a.n_rows, a.nnz, a.n_packets) == (b.n_rows, b.nnz, b.n_packets) and out.n_live == out.n_rows
    out.save_native(str(tmp_path / "a.vsx"))                                    # no selected row is deleted: the file of a handle without tombstones
    packed.save_native(str(tmp_path / "b.vsx"))
    assert (tmp_path / "a.vsx").read_bytes() == (tmp_path / "b.vsx").read_bytes()
    out.delete_rows(np.array([1], dtype=np.int64))                             # ... which takes deletions like any other
    assert out.n_live == out.n_rows - 1 and not bool(out.live_mask()[1]) and bool(out.live_mask()[0])


# ---- search ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_search_equals_the_filtered_search_of_the_source_on_the_scan():
    """ascending distinct ids: the new index's hits, mapped through ids, are the source's hits under the filter of those ids, ids and scores bit
    for bit; k is larger than the selection, so the source pads exactly where the new index ends"""
    n, B, m, k = 3000, 5, 500, 600
    ip, ix, d = oracle.synth_csr(21, 0, n, V, 96)
    q = torch.from_numpy(oracle.synth_queries(23, B)).to("cuda:0")
    ids = np.sort(np.random.default_rng(12).permutation(n)[:m])
    for store in (nat.VS_F32, nat.VS_F16, nat.VS_NONE):
        src = DeviceIndex.from_csr(ip, ix, None if store == nat.VS_NONE else d, V, store_dtype=store)
        src.set_option("blocked_postings", 0)
        new = src.select_rows(ids)
        new.set_option("blocked_postings", 0)
        got_ids, got_sc = new.search(q, m)
        want_ids, want_sc = src.search(q, k, filter=DocFilter.from_ids(ids, n))
        assert new.info().last_path < 2 and src.info().last_path < 2
        assert torch.equal(mapped(got_ids, ids), want_ids[:, :m]) and torch.equal(got_sc, want_sc[:, :m])
        assert bool((want_ids[:, m:] == -1).all()) and bool(torch.isinf(want_sc[:, m:]).all())


def test_search_equals_the_filtered_search_of_the_source_on_the_postings_copy():
    """rows long enough, and enough of them, that prepare() builds the new index's postings copy by the automatic rule"""
    n, nnz, B, k = 20_000, 300, 8, 100
    src = DeviceIndex.synthetic(5, 0, n, V, nnz)
    ids = np.nonzero(np.arange(n) % 6 != 0)[0]                                 # 16 667 rows
    assert len(ids) >= 16384
    new = src.select_rows(ids).prepare()
    info = new.info()
    assert info.postings_state == 1 and info.aux_bytes > 0
    q = torch.from_numpy(oracle.synth_queries(9, B)).to("cuda:0")
    got_ids, got_sc = new.search(q, k)
    assert new.info().last_path >= 2
    want_ids, want_sc = src.prepare().search(q, k, filter=DocFilter.from_ids(ids, n))
    assert torch.equal(mapped(got_ids, ids), want_ids) and torch.equal(got_sc, want_sc)


# ---- tombstones --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 65, 95])
def test_tombstones_travel_with_the_rows(narrow, n):
    """n % 32 in {0, 1, 31}; the list holds deleted rows, some of them twice"""
    csr, _, _ = narrow
    src = build(csr, VN)
    dead = np.array([5, 6, 7, 1000, 2099], dtype=np.int64)
    src.delete_rows(dead)
    rng = np.random.default_rng(n)
    ids = rng.integers(0, src.n_rows, size=n)
    ids[[0, 31, 32, 40, n - 1]] = [5, 1000, 5, 2099, 1000]                     # the first bit, both sides of a word edge, the last bit
    out, want = check(src, ids)
    live = src.live_mask().cpu().numpy()
    assert np.array_equal(out.live_mask().cpu().numpy(), live[ids])
    assert out.n_live == int(live[ids].sum()) == n - int(np.isin(ids, dead).sum()) and src.n_live == src.n_rows - len(dead)
    q = torch.from_numpy(oracle.synth_queries(2, 4, VN, 30)).to("cuda:0")
    got, _ = out.search(q, n)
    got = got.cpu().numpy()
    assert not np.isin(ids[got[got >= 0]], dead).any() and (got >= 0).sum() == 4 * out.n_live
    out.restore_rows()                                                         # ... and they come back
    assert out.n_live == n
    twin = DeviceIndex.from_csr(*want, VN)
    a, b = out.search(q, n), twin.search(q, n)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_tombstones_with_spare_capacity_then_append(narrow):
    csr, _, _ = narrow
    src = build(csr, VN)
    src.delete_rows(np.array([3], dtype=np.int64))
    out, want = check(src, np.array([3, 9, 3, 10]), rows_extra=40, packets_extra=100)
    more = make_csr([5, 0, 70], VN, np.random.default_rng(12))
    out.append_csr(*more)                                                      # the appended rows are live
    assert out.n_rows == 7 and out.n_live == 5
    assert out.live_mask().cpu().numpy().tolist() == [False, True, False, True, True, True, True]
    got = out.export_csr()
    assert np.array_equal(got[1], np.concatenate([want[1], more[1]])) and np.array_equal(bits(got[2]), bits(np.concatenate([want[2], more[2]])))
    with pytest.raises(ValueError, match="exceeds the reserved"):
        check(src, np.array([3, 9]))[0].append_csr(*more)                      # without the spare capacity there is no room


def test_without_deletions_the_file_is_that_of_the_same_csr(narrow, tmp_path):
    _, src, _ = narrow
    out, want = check(src, np.random.default_rng(13).integers(0, src.n_rows, size=777))
    twin = DeviceIndex.from_csr(*want, VN)
    out.save_native(str(tmp_path / "a.vsx"))
    twin.save_native(str(tmp_path / "b.vsx"))
    assert (tmp_path / "a.vsx").read_bytes() == (tmp_path / "b.vsx").read_bytes()
    assert out.n_live == 777


# ---- errors --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_ids_outside_the_index_raise_and_leave_the_source_searching(narrow):
    _, src, _ = narrow
    n = src.n_rows
    q = torch.from_numpy(oracle.synth_queries(3, 4, VN, 30)).to("cuda:0")
    before = src.search(q, 20)
    for bad in (n, -1):
        for pos in (0, 4999):                                                  # in the first and in the second scan block
            ids = np.random.default_rng(14).integers(0, n, size=5000)
            ids[pos] = bad
            with pytest.raises(ValueError, match="outside"):
                src.select_rows(torch.from_numpy(ids).to("cuda:0"))            # device ids: the first kernel's flag
            with pytest.raises(ValueError, match="outside"):
                src.select_rows(ids)                                           # host ids: the host's check
    with pytest.raises(ValueError, match="empty selection"):
        src.select_rows(np.zeros(0, dtype=np.int64))
    with pytest.raises(ValueError, match="empty selection"):
        src.select_rows(torch.zeros(0, dtype=torch.int64, device="cuda:0"))
    for bad in (dict(rows_extra=-1), dict(packets_extra=-1)):
        with pytest.raises(ValueError):
            src.select_rows(np.array([1]), **bad)
    after = src.search(q, 20)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


# ---- the dense kinds ---------------------------------------------------------------------------------------------------------------------------------------------
def test_dense_indexes():
    """a dense index stored as packets is selected from like any CSR index and stays reported dense; the matrix kind is a row gather"""
    rng = np.random.default_rng(8)
    mat = (rng.standard_normal((70, 256)) * (rng.random((70, 256)) < 0.2)).astype(np.float32)
    as_csr = DeviceIndex.from_dense(mat, max_density=1.0)
    assert as_csr.info().kind == nat.VS_KIND_DENSE and as_csr.info().n_packets > 0
    out, _ = check(as_csr, rng.integers(0, 70, size=100))
    assert out.info().kind == nat.VS_KIND_DENSE

    full = rng.standard_normal((70, 256)).astype(np.float32)
    for store in (np.float32, np.float16):
        dense = DeviceIndex.from_dense(full.astype(store))
        assert dense.info().kind == nat.VS_KIND_DENSE and dense.info().n_packets == 0
        ids = np.array([69, 0, 0, 33, 69, 1])
        got = dense.select_rows(ids)
        assert got.info().kind == nat.VS_KIND_DENSE and got.n_rows == 6
        assert np.array_equal(got.export_dense(np.float32), dense.export_dense(np.float32)[ids])
        ids = np.sort(rng.permutation(70)[:40])                                # ascending: the search maps to the filtered search
        new = dense.select_rows(torch.from_numpy(ids).to("cuda:0"))
        q = torch.from_numpy(rng.standard_normal((3, 256)).astype(np.float32)).to("cuda:0")
        got_ids, got_sc = new.search(q, 40)
        want_ids, want_sc = dense.search(q, 50, filter=DocFilter.from_ids(ids, 70))
        assert torch.equal(mapped(got_ids, ids), want_ids[:, :40]) and torch.equal(got_sc, want_sc[:, :40]) and bool((want_ids[:, 40:] == -1).all())
        for bad in (dict(rows_extra=1), dict(packets_extra=1)):
            with pytest.raises(ValueError, match="no append"):
                dense.select_rows(ids, **bad)
        dense.delete_rows(np.array([0, 33], dtype=np.int64))                   # tombstones travel on the matrix kind too
        carried = dense.select_rows(np.array([69, 0, 0, 33, 69, 1]))
        assert carried.n_live == 3 and carried.live_mask().cpu().numpy().tolist() == [True, False, False, False, True, True]


def test_onto_another_gpu(narrow):
    if nat.device_count() < 2:
        pytest.skip("one GPU")
    csr, _, _ = narrow
    src = build(csr, VN)
    src.delete_rows(np.array([3, 4], dtype=np.int64))
    ids = np.array([4, 10, 3, 3, 2000])
    out, _ = check(src, ids, device=1, rows_extra=2, packets_extra=2)
    assert out.device == 1 and out.n_live == 2 and out.live_mask().cpu().numpy().tolist() == [False, True, False, False, True]


# ---- sharding ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_shard_group(narrow):
    csr, src, _ = narrow
    n = src.n_rows
    cuts = [0, 700, 1500, n]
    group = ShardGroup([src.slice_rows(cuts[i], cuts[i + 1] - cuts[i], device=0) for i in range(3)])
    f = DocFilter.from_ids(np.random.default_rng(15).permutation(n)[:900], n)
    ids = f.ids().ids[0]                                                       # a filter's set: ascending, on the GPU
    whole, want = check(src, ids)
    new = group.select_rows(ids)
    assert isinstance(new, ShardGroup) and new.n_rows == 900 and len(new._shards) == 3
    parts = [s.export_csr() for s in new._shards]
    host = ids.cpu().numpy()
    assert [len(p[0]) - 1 for p in parts] == [int(((host >= cuts[i]) & (host < cuts[i + 1])).sum()) for i in range(3)]
    assert np.array_equal(np.concatenate([np.diff(p[0]) for p in parts]), np.diff(want[0]))
    assert np.array_equal(np.concatenate([p[1] for p in parts]), want[1]) and np.array_equal(bits(np.concatenate([p[2] for p in parts])), bits(want[2]))
    q = torch.from_numpy(oracle.synth_queries(4, 4, VN, 30)).to("cuda:0")
    a, b = new.search(q, 30), whole.search(q, 30)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    inside = np.array([699, 0, 699, 1499, 700, 2099])                          # any order inside a shard, host ids
    got = group.select_rows(inside)
    joined = [s.export_csr() for s in got._shards]
    want2 = ref.select_ref(*src.export_csr(), inside)
    assert np.array_equal(np.concatenate([np.diff(p[0]) for p in joined]), np.diff(want2[0])) and np.array_equal(np.concatenate([p[1] for p in joined]), want2[1])
    for back in (np.array([3, 800, 9]), torch.tensor([2000, 1499], device="cuda:0")):      # back to an earlier shard
        with pytest.raises(ValueError, match="earlier shard"):
            group.select_rows(back)
    two = group.select_rows(np.array([5, 6, 1600]))                            # the middle shard gets no id and disappears
    assert len(two._shards) == 2 and two.n_rows == 3 and [s.n_rows for s in two._shards] == [2, 1]
    assert same_csr(two._shards[1].export_csr(), ref.select_ref(*src.export_csr(), [1600]))


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
    rng = np.random.default_rng(16)
    sp = SparseIndex(device="cuda:0")
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix), torch.from_numpy(d), size=(n, VN))
    sp.move_to_device("cuda:0")
    sp.data = [{"text": f"doc {i}"} for i in range(n)]
    sp.set_groups(np.arange(n) // 3)
    sp.set_facet("lang", rng.integers(-1, 5, size=n), names=["a", "b", "c", "d", "e"])
    year = (1990 + rng.integers(0, 30, size=n)).astype(np.float32)
    year[::17] = np.nan
    year[5], year[6] = 0.0, -0.0
    sp.set_values("year", year)
    sp.set_values("pages", rng.integers(1, 50, size=n).astype(np.int32))
    return sp


def _snapshot(sp, q):
    res = sp.search(q, 20)
    return (sp._explain_target()[0].export_csr() if sp.shards is None else None, res.ids.clone(), res.scores.clone(), tuple(sp.facets("lang")),
            tuple(sp.value_stats("year")), sp.n_live, len(sp), sp.groups.clone(), sp.get_sample(7))


def _same_snapshot(a, b):
    return (a[0] is None or same_csr(a[0], b[0])) and _eq(tuple(a[1:]), tuple(b[1:]))


def test_facade_subset_of_a_filter(sparse_index):
    from vsearch_amd.ir import SparseIndex
    sp = sparse_index
    q = torch.from_numpy(oracle.synth_queries(5, 4, VN, 30)).to("cuda:0")
    snap = _snapshot(sp, q)
    f = sp.value_filter("year", 1995, 2004) & sp.value_filter("pages", 10, None)
    sub = sp.subset(filter=f)
    src = f.ids().ids[0]
    assert type(sub) is SparseIndex and sub is not sp and sub._dev is not sp._dev and 0 < len(sub) == int(src.shape[0]) < len(sp)
    assert torch.equal(sub.source_ids, src) and sp.source_ids is None
    host = src.cpu().numpy()
    assert same_csr(sub._device_index().export_csr(), ref.select_ref(*snap[0], host))
    assert all(sub.get_sample(j) == sp.get_sample(int(i)) for j, i in enumerate(host))
    assert torch.equal(sub.groups, sp.groups[src])
    assert torch.equal(sub._facet_field("lang")[0], sp._facet_field("lang")[0][src]) and sub.facet_names("lang") == ["a", "b", "c", "d", "e"]
    assert sub._facet_field("lang")[1] == 5
    for name in ("year", "pages"):
        assert _eq(sub.get_values(name), sp.get_values(name)[src])
    assert _eq(tuple(sub.facets("lang")), tuple(sp.facets("lang", filter=f)))
    assert _eq(tuple(sub.value_stats("pages")), tuple(sp.value_stats("pages", filter=f)))
    got, want = sub.search(q, 20), sp.search(q, 20, filter=f)
    assert torch.equal(mapped(got.ids, src), want.ids) and torch.equal(got.scores, want.scores)
    sub.set_facet("other", np.zeros(len(sub), dtype=np.int64))                 # the registries are the new index's own
    assert "other" in sub.facet_fields and "other" not in sp.facet_fields
    assert _same_snapshot(snap, _snapshot(sp, q))                              # the source answers every call exactly as before


def test_facade_subset_of_a_match_set_and_of_ids(sparse_index):
    sp = sparse_index
    q = torch.from_numpy(oracle.synth_queries(6, 2, VN, 30)).to("cuda:0")
    snap = _snapshot(sp, q)
    thr = float(sp.search(q[:1], 50).scores[0, -1])
    sub = sp.subset(q[:1], min_score=thr)                                      # the match set of ONE query
    assert torch.equal(sub.source_ids, sp.list_ids(q[:1], min_score=thr).ids[0]) and len(sub) >= 50
    with pytest.raises(ValueError, match="ONE"):
        sp.subset(q, min_score=thr)
    sp.delete([10, 11])
    picked = np.array([12, 10, 12, 2099, 0, 10])                               # ids=: order and repeats kept, a deleted id carried as deleted
    sub = sp.subset(ids=picked)
    assert sub.source_ids.tolist() == picked.tolist() and len(sub) == 6 and sub.n_live == 4
    assert same_csr(sub._device_index().export_csr(), ref.select_ref(*snap[0], picked))
    assert [sub.get_sample(j)["text"] for j in range(6)] == [f"doc {i}" for i in picked]
    mini = sp.subset(ids=sp.sample_ids(100, seed=0).ids[0])                    # a uniform miniature (never a deleted document)
    assert len(mini) == 100 and mini.n_live == 100 and not np.isin(mini.source_ids.cpu().numpy(), [10, 11]).any()
    everything = sp.subset()                                                   # no set: every live document
    assert len(everything) == sp.n_live == 2098 and not np.isin(everything.source_ids.cpu().numpy(), [10, 11]).any()
    for bad in (np.array([-1]), np.array([2100]), np.zeros(0, np.int64)):
        with pytest.raises(ValueError):
            sp.subset(ids=bad)
    with pytest.raises(ValueError, match="ids="):
        sp.subset(ids=picked, filter=sp.value_filter("year", 1995, None))
    with pytest.raises(ValueError, match="empty selection"):
        sp.subset(filter=sp.value_filter("year", 3000, None))


def test_facade_sorted_by(sparse_index):
    from vsearch_amd.ir import SCORE
    sp = sparse_index
    n = len(sp)
    dead = np.array([0, 5, 77, 2099])
    sp.delete(dead)
    q = torch.from_numpy(oracle.synth_queries(7, 4, VN, 30)).to("cuda:0")
    snap = _snapshot(sp, q)
    live = sp._device_index().live_mask().cpu().numpy()
    srt = sp.sorted_by("lang")
    src = srt.source_ids.cpu().numpy()
    assert len(srt) == srt.n_live == sp.n_live == n - 4 and not np.isin(src, dead).any() and len(np.unique(src)) == len(src)
    lab = srt._facet_field("lang")[0].cpu().numpy()
    assert np.array_equal(lab, sp._facet_field("lang")[0].cpu().numpy()[src])
    rank = np.where(lab < 0, 1 << 20, lab)
    assert (np.diff(rank) >= 0).all() and (lab[-1] == -1) and (np.diff(src)[np.diff(rank) == 0] > 0).all()
    assert np.array_equal(src, ref.sort_order(ref.order_key(sp._facet_field("lang")[0].cpu().numpy(), labels=True), live))
    assert same_csr(srt._device_index().export_csr(), ref.select_ref(*snap[0], src))
    assert _eq(tuple(srt.facets("lang")), tuple(sp.facets("lang")))            # the same documents: the same counts
    for field, desc in (("year", True), ("year", False), ("pages", True), ("groups", False)):
        got = sp.sorted_by(field, descending=desc)
        if field == "groups":
            keys = ref.order_key(sp.groups.cpu().numpy(), labels=True)
        else:
            keys = ref.order_key(sp.get_values(field).cpu().numpy())
        assert np.array_equal(got.source_ids.cpu().numpy(), ref.sort_order(keys, live, descending=desc)), (field, desc)
        assert _eq(got.get_values("year"), sp.get_values("year")[got.source_ids])
    year = sp.sorted_by("year", descending=True).get_values("year").cpu().numpy()
    assert np.isnan(year[-1]) and not np.isnan(year[0]) and year[0] == np.nanmax(year)
    with pytest.raises(ValueError, match="SCORE"):
        sp.sorted_by(SCORE)
    with pytest.raises(KeyError):
        sp.sorted_by("nothing")
    assert _same_snapshot(snap, _snapshot(sp, q))


def test_facade_row_sharded(sparse_index):
    sp = sparse_index
    q = torch.from_numpy(oracle.synth_queries(8, 4, VN, 30)).to("cuda:0")
    f = sp.value_filter("year", 1995, 2004)
    want = sp.subset(filter=f)
    want_res = want.search(q, 20)
    sp.shard_rows([0, 0, 0])
    snap = _snapshot(sp, q)
    sub = sp.subset(filter=f)
    assert sub.shards is not None and len(sub.shards) == 3 and sub.shards[0] is not sp.shards[0]
    assert torch.equal(sub.source_ids, want.source_ids) and torch.equal(sub.groups, want.groups) and len(sub) == len(want)
    got = sub.search(q, 20)
    assert torch.equal(got.ids, want_res.ids) and torch.equal(got.scores, want_res.scores)
    assert _eq(tuple(sub.facets("lang")), tuple(want.facets("lang")))
    few = sp.subset(ids=[3, 1, 2000])                                          # the middle shard is left out
    assert len(few.shards) == 2 and len(few) == 3
    with pytest.raises(ValueError, match="earlier shard"):
        sp.subset(ids=[2000, 3])
    with pytest.raises(NotImplementedError, match="shard"):
        sp.sorted_by("lang")
    assert _same_snapshot(snap, _snapshot(sp, q))


def test_facade_dense_matrix_index():
    from vsearch_amd.ir import Index
    idx = Index(device="cuda:0")
    mat = torch.randn(64, 128, generator=torch.Generator().manual_seed(3))
    idx.vector = mat
    idx.move_to_device("cuda:0")
    idx.set_values("len", np.arange(64, dtype=np.float32) % 7)
    srt = idx.sorted_by("len")
    src = srt.source_ids.cpu()
    assert type(srt) is Index and np.array_equal(src.numpy(), ref.sort_order(ref.order_key(np.arange(64, dtype=np.float32) % 7), np.ones(64, bool)))
    assert torch.equal(srt.vector.cpu(), mat[src])


def test_retriever_subset_index_and_sort_index_by(sparse_index):
    from vsearch_amd.ir import Retriever

    class Fake:                                  # (methods as class attributes: no reference cycle through the instance)
        subset_index = Retriever.subset_index
        sort_index_by = Retriever.sort_index_by
    fake = Fake()
    fake.index, fake.device = sparse_index, "cuda"
    f = sparse_index.value_filter("pages", 40, None)
    new = fake.subset_index(filter=f, inplace=False)
    assert fake.index is sparse_index and torch.equal(new.source_ids, f.ids().ids[0])
    srt = fake.sort_index_by("lang")
    assert fake.index is srt and srt is not sparse_index and len(srt) == len(sparse_index)
    lab = srt._facet_field("lang")[0].cpu().numpy()
    assert (np.diff(np.where(lab < 0, 1 << 20, lab)) >= 0).all()
    again = fake.subset_index(ids=[4, 4, 1])                                   # of the sorted index now, in place
    assert fake.index is again and torch.equal(again.source_ids, torch.tensor([4, 4, 1], device=again.source_ids.device))
