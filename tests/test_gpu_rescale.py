"""GPU tests of the reweighted index (vs_index_row_stats, vs_index_rescale; DeviceIndex / ShardGroup row_stats and rescale, Index.row_stats,
row_norms, rescaled, normalized, astype, idf_weights, Retriever.normalize_index / reweight_index) -- run on MI355X.

Every rescale case compares export_csr of the result with the numpy reference (tests/_rescale_ref.py) of export_csr of the source: row pointers
and columns by array_equal, values by their BITS (where the reference holds a NaN, any NaN); the statistics compare the float64 sums by their
bits.  The source's export is bit-identical before and after.  Small indexes built from numpy CSR: V = 29 523, and V = 300 for the narrow cases."""
import types

import numpy as np
import pytest
import torch

import oracle
from conftest import V
from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, ShardGroup, rescale_plan

import _rescale_ref as ref

pytestmark = pytest.mark.gpu
VN = 300                                                 # the narrow vocabulary
STORES = {"fp32": nat.VS_F32, "fp16": nat.VS_F16, "binary": nat.VS_NONE}
OUTS = {"fp32": nat.VS_F32, "fp16": nat.VS_F16}
LENGTHS = [0, 1, 7, 8, 9, 504, 511, 512, 513, 520, V, 0]      # 504 .. 520 cells: 63 / 64 / 65 packets, the lane wrap


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


def same_csr(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and ref.same_values(a[2], b[2])


def scales(rng, n_rows, n_cols):
    return (rng.standard_normal(n_rows) * 3).astype(np.float32), np.exp(rng.standard_normal(n_cols) * 2).astype(np.float32)


def check(src, row_scale=None, col_scale=None, out=None, **extra):
    """rescale `src` and compare with the reference -> (the new DeviceIndex, the reference's values)"""
    info = src.info()
    binary = info.store_dtype == nat.VS_NONE
    before = src.export_csr()
    new = src.rescale(row_scale, col_scale, out, **extra)
    assert same_csr(src.export_csr(), before), "the source changed"
    out_dtype = info.store_dtype if out is None else OUTS[out]
    want = ref.rescale_ref(before[0], before[1], None if binary else before[2], row_scale, col_scale, "fp16" if out_dtype == nat.VS_F16 else "fp32")
    got = new.export_csr()
    assert np.array_equal(got[0], before[0]), "row pointers"
    assert np.array_equal(got[1], before[1]), "columns"
    assert ref.same_values(got[2], want), "value bits"
    ni = new.info()
    assert (ni.n_rows, ni.n_packets, ni.nnz, ni.n_cols, ni.store_dtype) == (info.n_rows, info.n_packets, info.nnz, info.n_cols, out_dtype)
    return new, want


def check_stats(src):
    info = src.info()
    csr = src.export_csr()
    want = ref.row_stats_ref(csr[0], None if info.store_dtype == nat.VS_NONE else csr[2])
    got = src.row_stats()
    assert [t.dtype for t in got] == [torch.int32, torch.int32, torch.float64, torch.float64, torch.float32]
    assert all(t.is_cuda and t.shape == (info.n_rows,) for t in got)
    got = [t.cpu().numpy() for t in got]
    assert np.array_equal(got[0], want[0]), "cells"
    assert np.array_equal(got[1], want[1]), "nonzero"
    assert ref.same_f64(got[2], want[2]), "l1 bits"
    assert ref.same_f64(got[3], want[3]), "sumsq bits"
    assert np.array_equal(bits(got[4]), bits(want[4])), "max bits"
    return got


# ---- row lengths, every store, every out dtype, every combination of scales ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_rows():
    csr = make_csr(LENGTHS, V, np.random.default_rng(1))
    return {name: build(csr, V, store) for name, store in STORES.items()}


@pytest.mark.parametrize("out", list(OUTS))
@pytest.mark.parametrize("store", list(STORES))
def test_row_lengths_stores_and_scale_combinations(long_rows, store, out):
    src = long_rows[store]
    rs, cs = scales(np.random.default_rng(2), len(LENGTHS), V)
    assert src.rescale_plan(None, cs, out)[2] == "lds"
    for r, c in ((None, None), (rs, None), (None, cs), (rs, cs)):
        check(src, r, c, out)


@pytest.mark.parametrize("store", list(STORES))
def test_stats_row_lengths(long_rows, store):
    got = check_stats(long_rows[store])
    assert got[0].tolist() == LENGTHS


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 4096, 4097])
def test_row_counts(n_rows):
    """rows of 0 to 20 cells; the first and the last row of the first 64-row run are empty"""
    rng = np.random.default_rng(n_rows)
    lengths = rng.integers(0, 21, size=n_rows)
    if n_rows >= 64:
        lengths[0] = lengths[63] = 0
    rs, cs = scales(rng, n_rows, VN)
    for store in STORES.values():
        src = build(make_csr(lengths, VN, rng), VN, store)
        check(src, rs, cs, "fp32")
        check(src, rs, None, "fp16")
        check_stats(src)


def test_an_index_without_a_packet():
    rng = np.random.default_rng(3)
    src, _ = build(make_csr([3] * 70, VN, rng), VN).prune(keep_cols=[])       # every cell dropped: 70 rows, no packet
    assert src.info().n_packets == 0 and src.n_rows == 70
    rs, cs = scales(rng, 70, VN)
    new, _ = check(src, rs, cs, "fp16")
    got = check_stats(new)
    assert not got[0].any() and not got[2].any() and np.isnan(got[4]).all()


def test_widths_and_the_route_of_the_column_scales():
    """n_cols = 300 and V hold the column scales as an LDS image; one width past the image limit reads them from memory: the route is asked of
    the plan, the limit found by bisection on it"""
    lo, hi = V, 65535
    assert rescale_plan(1, 1, lo, nat.VS_F32, nat.VS_F32, False, True)[2] == "lds" and rescale_plan(1, 1, hi, nat.VS_F32, nat.VS_F32, False, True)[2] == "memory"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if rescale_plan(1, 1, mid, nat.VS_F32, nat.VS_F32, False, True)[2] == "lds" else (lo, mid)
    for n_cols, route in ((VN, "lds"), (V, "lds"), (lo, "lds"), (hi, "memory"), (65535, "memory")):
        rng = np.random.default_rng(n_cols)
        lengths = [5, 0, min(600, n_cols), 9, 64, 1]
        csr = make_csr(lengths, n_cols, rng)
        csr[1][-1] = n_cols - 1                                                # the last column is stored (row 5's only cell)
        rs, cs = scales(rng, len(lengths), n_cols)
        for store in STORES.values():
            src = build(csr, n_cols, store)
            assert src.rescale_plan(None, cs, "fp32")[2] == route
            assert src.rescale_plan(rs, None, "fp32")[2] == "none"
            check(src, rs, cs, "fp32")
            check(src, None, cs, "fp16")


# ---- special values ------------------------------------------------------------------------------------------------------------------------------------
SPECIAL = [  # (stored value, column scale)
    (0.0, 5.0), (-0.0, 5.0), (-0.0, -1.0), (1e-40, 1.0), (1e-40, 0.5), (1e-20, 1e-20), (-1e-20, 1e-20),        # +-0, subnormal fp32 inputs and results
    (1.0, 2.0 ** -24), (1.0, 2.0 ** -25), (-1.0, 2.0 ** -26), (1.5, 2.0 ** -24), (3.0, 2.0 ** -15),                  # fp16 results: subnormal, underflow to +-0
    (1 + 2.0 ** -11, 1.0), (1 + 3 * 2.0 ** -11, 1.0), (65519.0, 1.0), (65520.0, 1.0), (-65520.0, 1.0),            # ties to even, the overflow
    (3.0, 0.0), (3.0, -1.0), (3.0, np.inf), (-3.0, np.inf), (3.0, np.nan), (0.0, np.inf), (np.inf, 0.0),             # scales of 0, -1, +inf, NaN; inf * 0
    (np.nan, 1.0), (np.inf, -2.0), (3e38, 2.0), (1e-45, 0.5), (1e-45, 0.75),
    (1 + 2.0 ** -12, 1 + 2.0 ** -12),         # 1 + 2^-11 + 2^-24: float32 takes it to the fp16 tie, which goes to 1; ONE rounding would give 1 + 2^-10
]


@pytest.mark.parametrize("out", list(OUTS))
def test_special_values(out):
    n = len(SPECIAL)
    ip = np.array([0, n, n + 3], dtype=np.int64)
    ix = np.concatenate([np.arange(n), [0, 5, 17]]).astype(np.int64)
    d = np.array([w for w, _ in SPECIAL] + [1.0, -2.0, 0.5], dtype=np.float32)
    cs = np.ones(VN, np.float32)
    cs[:n] = [s for _, s in SPECIAL]
    src = build((ip, ix, d), VN)
    assert np.array_equal(bits(src.export_csr()[2]), bits(d))                  # subnormals, NaN and -0.0 are stored as given
    _, want = check(src, None, cs, out)
    assert np.isnan(want[[21, 22, 23, 24]]).all() and want[17] == 0 and np.isinf(want[19])
    if out == "fp16":
        assert want[7] == 2.0 ** -24 and bits(want[8:10]).tolist() == [0, 0x80000000] and want[12] == 1.0 and want[13] == 1 + 2.0 ** -9
        assert want[14] == 65504.0 and want[15] == np.inf and want[16] == -np.inf
        assert want[29] == 1.0
    else:
        assert want[4] == np.float32(1e-40) * np.float32(0.5) and 0 < want[5] < 1.2e-38 and want[26] == np.inf
    for rs in ([0.0, 1.0], [-1.0, np.inf], [np.nan, -0.0], [np.inf, 2.0 ** -140]):
        check(src, np.array(rs, np.float32), None, out)
        check(src, np.array(rs, np.float32), cs, out)
    check(build((ip, ix, d), VN, nat.VS_F16), np.array([2.0 ** -10, 3.0], np.float32), cs, out)


def test_padding_stays_zero_under_an_infinite_scale():
    """a 9-cell row of positive values with row_scale = +inf: its seven padding cells stay +0, so under a positive query the row scores +inf,
    not NaN (inf * 0), and its neighbours' scores do not move"""
    rng = np.random.default_rng(4)
    csr = make_csr([5, 9, 12, 3], VN, rng, values=lambda n: rng.random(n) + 0.5)
    q = torch.from_numpy(rng.random((1, VN)).astype(np.float32) + 0.1).to("cuda:0")
    rs = np.array([1.0, np.inf, 1.0, 1.0], np.float32)
    for store in (nat.VS_F32, nat.VS_F16, nat.VS_NONE):
        src = build(csr, VN, store)
        before = src.set_scores(q).cpu().numpy()[0]
        for out in OUTS:
            same = store == OUTS[out]
            new, want = check(src, rs, None, out)
            got = new.set_scores(q).cpu().numpy()[0]
            assert got[1] == np.inf and np.isinf(want[5:14]).all()
            if same:
                assert np.array_equal(bits(got[[0, 2, 3]]), bits(before[[0, 2, 3]]))
            inf_cols, _ = check(src, None, np.full(VN, np.inf, np.float32), out)
            assert (inf_cols.set_scores(q).cpu().numpy()[0] == np.inf).all()


def test_padding_bits_equal_the_index_built_from_the_result(tmp_path):
    """the .vsx bytes of a rescaled index -- padding ids and padding values included -- are those of the index built from the reference's CSR"""
    rng = np.random.default_rng(5)
    csr = make_csr([5, 9, 0, 12, 3, 64, 65], VN, rng, values=lambda n: rng.random(n) + 0.5)
    rs, cs = np.array([1.0, np.inf, 2.0, 1.0, -1.0, 0.5, 3.0], np.float32), np.exp(rng.standard_normal(VN)).astype(np.float32)
    for store in (nat.VS_F32, nat.VS_NONE):
        src = build(csr, VN, store)
        for out in OUTS:
            new, want = check(src, rs, cs, out)
            twin = DeviceIndex.from_csr(csr[0], csr[1], want, VN, store_dtype=OUTS[out])
            new.save_native(str(tmp_path / "a.vsx"))
            twin.save_native(str(tmp_path / "b.vsx"))
            assert (tmp_path / "a.vsx").read_bytes() == (tmp_path / "b.vsx").read_bytes()


# ---- no scale: copies and conversions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["fp32", "fp16"])
def test_no_scale_same_dtype_is_a_copy(long_rows, store, tmp_path):
    src = long_rows[store]
    before = src.export_csr()
    new = src.rescale()
    got = new.export_csr()
    assert np.array_equal(got[0], before[0]) and np.array_equal(got[1], before[1]) and np.array_equal(bits(got[2]), bits(before[2]))
    new.save_native(str(tmp_path / "a.vsx"))
    src.select_rows(np.arange(src.n_rows)).save_native(str(tmp_path / "b.vsx"))
    assert (tmp_path / "a.vsx").read_bytes() == (tmp_path / "b.vsx").read_bytes()
    with pytest.raises(ValueError, match="binary index has no value dtype"):
        long_rows["binary"].rescale()


def test_to_fp16_equals_the_index_built_as_fp16():
    rng = np.random.default_rng(6)
    csr = make_csr([0, 3, 40, 513, 8], VN * 3, rng, values=lambda n: rng.standard_normal(n).astype(np.float16))     # values representable in fp16
    src = build(csr, VN * 3)
    new, _ = check(src, out="fp16")
    twin = build(csr, VN * 3, nat.VS_F16)
    a, b = new.export_csr(), twin.export_csr()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))
    back, _ = check(new, out="fp32")
    assert np.array_equal(bits(back.export_csr()[2]), bits(csr[2]))


# ---- tombstones, capacity, devices, arguments ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow():
    rng = np.random.default_rng(9)
    lengths = rng.integers(0, 120, size=2100)
    lengths[:4] = [0, 1, 8, 9]
    csr = make_csr(lengths, VN, rng)
    return csr, build(csr, VN), build(csr, VN, nat.VS_F16)


def test_tombstones_are_carried(narrow):
    csr, _, _ = narrow
    src = build(csr, VN)
    n = src.n_rows
    rs, cs = scales(np.random.default_rng(10), n, VN)
    dead = np.array([0, 5, 6, 7, 1000, n - 1], dtype=np.int64)
    src.delete_rows(dead)
    check_stats(src)                                                           # deleted rows are stored rows
    new, want = check(src, rs, cs)
    assert new.n_live == n - len(dead) and torch.equal(new.live_mask(), src.live_mask())
    q = torch.from_numpy(oracle.synth_queries(2, 4, VN, 30)).to("cuda:0")
    ids, _ = new.search(q, 50)
    assert not np.isin(ids.cpu().numpy(), dead).any()
    new.restore_rows()                                                         # ... and come back rescaled
    assert new.n_live == n and src.n_live == n - len(dead)
    twin = DeviceIndex.from_csr(csr[0], csr[1], want, VN)
    a, b = new.search(q, 50), twin.search(q, 50)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_spare_capacity_then_append(narrow):
    csr, src, _ = narrow
    rng = np.random.default_rng(12)
    rs, cs = scales(rng, src.n_rows, VN)
    new, want = check(src, rs, cs, rows_extra=3, packets_extra=10)
    more = make_csr([5, 0, 70], VN, rng)
    new.append_csr(*more)
    got = new.export_csr()
    assert np.array_equal(got[0], np.concatenate([csr[0], csr[0][-1] + more[0][1:]]))
    assert np.array_equal(got[1], np.concatenate([csr[1], more[1]])) and ref.same_values(got[2], np.concatenate([want, more[2]]))
    with pytest.raises(ValueError, match="exceeds the reserved"):
        check(src, rs, cs)[0].append_csr(*more)                                # without the spare capacity there is no room
    for bad in (dict(rows_extra=-1), dict(packets_extra=-1)):
        with pytest.raises(ValueError):
            src.rescale(rs, **bad)


def test_arguments(narrow):
    csr, src, _ = narrow
    n = src.n_rows
    with pytest.raises(ValueError, match="row_scale must have shape"):
        src.rescale(np.ones(n + 1, np.float32))
    with pytest.raises(ValueError, match="col_scale must have shape"):
        src.rescale(None, np.ones(VN - 1, np.float32))
    with pytest.raises(ValueError, match="dtype must be"):
        src.rescale(dtype="binary")
    for bad in (torch.ones(n, dtype=torch.bool, device="cuda:0"), np.ones(n, dtype=bool)):
        with pytest.raises(TypeError, match="numbers"):
            src.rescale(bad)
    import ctypes as C
    h = C.c_void_p()
    assert nat.lib().vs_index_rescale(src._h, None, None, nat.VS_NONE, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and not h.value
    assert nat.lib().vs_index_rescale(src._h, None, None, nat.VS_F32, 0, 0, 99, C.byref(h)) == nat.VS_EINVAL and "device" in nat.last_error()
    # scales as torch tensors on the GPU, float64 and integer scales (cast to float32), a host row scale beside a device column scale
    rs, cs = scales(np.random.default_rng(13), n, VN)
    a = src.rescale(torch.from_numpy(rs).to("cuda:0"), torch.from_numpy(cs).to("cuda:0")).export_csr()
    b = src.rescale(rs.astype(np.float64), torch.from_numpy(cs).to("cuda:0")).export_csr()
    c, _ = check(src, rs, cs)
    assert same_csr(a, c.export_csr()) and same_csr(b, c.export_csr())
    check(src, np.full(n, 2, dtype=np.int64).astype(np.float32), None)


def test_onto_another_gpu(narrow):
    if nat.device_count() < 2:
        pytest.skip("one GPU")
    csr, _, _ = narrow
    src = build(csr, VN)
    src.delete_rows(np.array([3, 4], dtype=np.int64))
    rs, cs = scales(np.random.default_rng(14), src.n_rows, VN)
    new, _ = check(src, rs, cs, "fp16", device=1, rows_extra=2, packets_extra=2)
    assert new.device == 1 and new.n_live == src.n_rows - 2


def test_dense_indexes():
    """a dense index stored as packets is a CSR index here and stays reported dense; the matrix-core kind is refused"""
    rng = np.random.default_rng(8)
    mat = (rng.standard_normal((70, 256)) * (rng.random((70, 256)) < 0.2)).astype(np.float32)
    as_csr = DeviceIndex.from_dense(mat, max_density=1.0)
    assert as_csr.info().kind == nat.VS_KIND_DENSE and as_csr.info().n_packets > 0
    rs, cs = scales(rng, 70, 256)
    new, _ = check(as_csr, rs, cs)
    assert new.info().kind == nat.VS_KIND_DENSE
    check_stats(as_csr)
    with pytest.raises(NotImplementedError, match="dense"):
        DeviceIndex.from_dense(mat).rescale(rs)
    with pytest.raises(NotImplementedError, match="dense"):
        DeviceIndex.from_dense(mat).row_stats()


# ---- the statistics ------------------------------------------------------------------------------------------------------------------------------------------
def test_stats_magnitudes_from_2_to_the_minus_60_to_2_to_the_60():
    """inside one row: float32 squares lose the small cells, and a sum in another order differs in the last bits"""
    rng = np.random.default_rng(15)
    lengths = [700, 520, 65 * 8, 9, 1100]
    csr = make_csr(lengths, V, rng, values=lambda n: rng.standard_normal(n) * 2.0 ** rng.integers(-60, 61, size=n))
    got = check_stats(build(csr, V))
    x = csr[2].astype(np.float64)
    plain = np.add.reduceat(x * x, csr[0][:-1])
    assert np.isfinite(got[3]).all() and np.allclose(got[3], plain, rtol=1e-12)
    with np.errstate(all="ignore"):                                            # float32 squares summed in float32 are off in the 7th digit
        single = np.add.reduceat(csr[2] * csr[2], csr[0][:-1]).astype(np.float64)
    assert (np.abs(single - got[3]) > 1e-9 * got[3]).any()
    d = np.zeros(65 * 8, np.float32)                                           # the case of tests/test_rescale_cpu.py where the order decides
    d[0] = 2.0 ** 27
    d[8:64:8] = 1.0
    ip, ix = np.array([0, d.size], dtype=np.int64), np.arange(d.size, dtype=np.int64)
    assert check_stats(build((ip, ix, d), V))[3][0] == 2.0 ** 54 + 4.0


def test_stats_nan_cells_empty_rows_and_zero_signs():
    nan = np.nan
    rows = [[], [-0.0, 0.0], [nan, nan], [-0.0], [nan, -3.0, -7.0], [2.0, nan, 5.0, -1.0], [0.0, -2.0], []]
    ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ix = np.concatenate([np.arange(len(r)) for r in rows]).astype(np.int64)
    d = np.array([v for r in rows for v in r], np.float32)
    for store in (nat.VS_F32, nat.VS_F16):
        got = check_stats(build((ip, ix, d), VN, store))
        assert bits(got[4]).tolist() == [0x7FC00000, 0, 0x7FC00000, 0, bits(np.float32(-3))[0], bits(np.float32(5))[0], 0, 0x7FC00000]
        assert got[1].tolist() == [0, 0, 2, 0, 3, 4, 1, 0] and np.isnan(got[2][[2, 4, 5]]).all() and got[2][0] == 0 and got[3][7] == 0


def test_stats_null_host_and_device_outputs(narrow):
    import ctypes as C
    csr, src, _ = narrow
    n = src.n_rows
    want = ref.row_stats_ref(csr[0], csr[2])
    host = [np.full(n, 7, np.int32), np.full(n, 7, np.int32), np.full(n, 7.0), np.full(n, 7.0), np.full(n, 7, np.float32)]
    ptr = [C.c_void_p(a.ctypes.data) for a in host]
    L = nat.lib()
    nat.check(L.vs_index_row_stats(src._h, *ptr))                              # all on the host
    assert np.array_equal(host[0], want[0]) and np.array_equal(host[1], want[1]) and ref.same_f64(host[2], want[2]) and ref.same_f64(host[3], want[3])
    assert np.array_equal(bits(host[4]), bits(want[4]))
    for keep in ([3], [0, 4], [1, 2]):                                         # any output may be NULL
        host2 = [np.full(n, 7, a.dtype) for a in host]
        nat.check(L.vs_index_row_stats(src._h, *[C.c_void_p(a.ctypes.data) if i in keep else None for i, a in enumerate(host2)]))
        for i in range(5):
            assert np.array_equal(host2[i].view(np.uint8), (host[i] if i in keep else np.full(n, 7, host[i].dtype)).view(np.uint8))
    nat.check(L.vs_index_row_stats(src._h, None, None, None, None, None))
    dev = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    nat.check(L.vs_index_row_stats(src._h, None, None, None, C.c_void_p(dev.data_ptr()), None))       # one device output
    assert ref.same_f64(dev.cpu().numpy(), want[3])
    assert L.vs_index_row_stats(src._h, ptr[0], None, None, C.c_void_p(dev.data_ptr()), None) == nat.VS_EINVAL and "mix host and device" in nat.last_error()


# ---- sharding -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_shard_group_of_uneven_shards(narrow):
    csr, src, _ = narrow
    n = src.n_rows
    rs, cs = scales(np.random.default_rng(16), n, VN)
    cuts = [0, 700, 1500, n]
    group = ShardGroup([src.slice_rows(cuts[i], cuts[i + 1] - cuts[i], device=0) for i in range(3)])
    whole, want = check(src, rs, cs, "fp16")
    new = group.rescale(rs, torch.from_numpy(cs), "fp16")
    assert isinstance(new, ShardGroup) and new.n_rows == n
    parts = [s.export_csr() for s in new._shards]
    assert [len(p[0]) - 1 for p in parts] == [700, 800, n - 1500]
    assert np.array_equal(np.concatenate([p[1] for p in parts]), csr[1]) and ref.same_values(np.concatenate([p[2] for p in parts]), want)
    q = torch.from_numpy(oracle.synth_queries(4, 4, VN, 30)).to("cuda:0")
    a, b = new.search(q, 30), whole.search(q, 30)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    one, many = src.row_stats(), group.row_stats()
    for x, y in zip(one, many):
        assert x.dtype == y.dtype and np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    assert [p[2] for p in group.rescale_plan(rs, cs)] == ["lds"] * 3
    with pytest.raises(ValueError, match="row_scale must have shape"):
        group.rescale(rs[:-1])
    with pytest.raises(ValueError, match="row_scale must have shape"):
        group.rescale(torch.ones(n - 1, device="cuda:0"))                     # a tensor on the GPU is refused the same way


# ---- the facade ------------------------------------------------------------------------------------------------------------------------------------------------------
def _eq(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor):
        return a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())
    return a == b


def _ulps(a, b):
    """distance in float32 units in the last place (same-sign finite values)"""
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


COS_N, COS_SEED = 3000, 20


def cosine_csr():
    """rows of very different lengths and magnitudes: the dot product and the cosine rank them differently"""
    rng = np.random.default_rng(COS_SEED)
    lengths = rng.integers(1, 120, size=COS_N)
    ip, ix, d = make_csr(lengths, VN, rng, values=lambda n: (rng.random(n) + 0.1) * rng.choice([0.5, 1.0, 4.0]))
    return ip, ix, d


@pytest.fixture()
def sparse_index():
    from vsearch_amd.ir import SparseIndex
    ip, ix, d = cosine_csr()
    n = len(ip) - 1
    sp = SparseIndex(device="cuda:0", fp16=False)
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix), torch.from_numpy(d), size=(n, VN))
    sp.move_to_device("cuda:0")
    sp.data = [{"text": f"doc {i}"} for i in range(n)]
    sp.set_groups(np.arange(n) // 3)
    sp.set_facet("lang", np.arange(n) % 5, names=["a", "b", "c", "d", "e"])
    sp.set_values("year", (1990 + np.arange(n) % 30).astype(np.float32))
    return sp


def test_facade_normalized_searches_by_cosine(sparse_index):
    from vsearch_amd.ir import SparseIndex
    sp = sparse_index
    ip, ix, d = cosine_csr()
    n, k = len(ip) - 1, 10
    rng = np.random.default_rng(21)
    q = (rng.random((4, VN)) * (rng.random((4, VN)) < 0.2)).astype(np.float32)
    dense = np.zeros((n, VN))
    dense[np.repeat(np.arange(n), np.diff(ip)), ix] = d
    cos = (dense @ q.T.astype(np.float64)).T / np.sqrt((dense * dense).sum(1))[None, :]
    order = np.argsort(-cos, axis=1, kind="stable")[:, :k + 1]
    top = np.take_along_axis(cos, order, 1)
    assert (top[:, :-1] - top[:, 1:] > 1e-5 * top[:, :1]).all()               # no near-ties among the first k + 1: float32 scores cannot swap them
    dots = np.argsort(-(dense @ q.T.astype(np.float64)).T, axis=1, kind="stable")[:, :k]
    assert not np.array_equal(dots, order[:, :k])                              # ... and the raw dot product ranks differently
    new = sp.normalized()
    assert type(new) is SparseIndex and new is not sp and len(new) == n
    res = new.search(torch.from_numpy(q).to("cuda:0"), k)
    assert np.array_equal(res.ids.cpu().numpy(), order[:, :k])
    norms = new.row_norms(2).cpu().numpy()
    assert norms.dtype == np.float32 and (np.abs(norms.astype(np.float64) - 1.0) <= 2.0 ** -22).all()
    l1 = sp.normalized(p=1).row_norms(1).cpu().numpy()
    assert (np.abs(l1.astype(np.float64) - 1.0) <= 2.0 ** -22).all()
    # the scale is float32(1 / norm_fp64): the result is the reference applied with that scale
    st = sp.row_stats()
    scale = (1.0 / np.sqrt(st.sumsq.cpu().numpy())).astype(np.float32)
    assert ref.same_values(new._device_index().export_csr()[2], ref.rescale_ref(ip, ix, d, row_scale=scale))
    for bad in (0, 3, "2", True):
        with pytest.raises(ValueError, match="p must be"):
            sp.normalized(p=bad)


def test_facade_normalized_keeps_rows_without_a_norm():
    from vsearch_amd.ir import SparseIndex
    ip = np.array([0, 0, 2, 4], dtype=np.int64)
    ix = np.array([0, 1, 0, 1], dtype=np.int64)
    d = np.array([0.0, -0.0, 3.0, 4.0], np.float32)                            # an empty row, a zero row, a 3-4-5 row
    sp = SparseIndex(device="cuda:0", fp16=False)
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix), torch.from_numpy(d), size=(3, VN))
    sp.move_to_device("cuda:0")
    got = sp.normalized()._device_index().export_csr()[2]
    assert np.array_equal(bits(got), bits(np.array([0.0, -0.0, np.float32(3.0) * np.float32(0.2), np.float32(4.0) * np.float32(0.2)], np.float32)))
    assert sp.row_norms(2).cpu().numpy().tolist() == [0.0, 0.0, 5.0] and sp.row_norms(1).cpu().numpy().tolist() == [0.0, 0.0, 7.0]


def test_facade_row_stats_and_norms(sparse_index):
    sp = sparse_index
    ip, ix, d = cosine_csr()
    want = ref.row_stats_ref(ip, d)
    st = sp.row_stats()
    assert np.array_equal(st.cells.cpu().numpy(), want[0]) and ref.same_f64(st.sumsq.cpu().numpy(), want[3]) and ref.same_f64(st.l1.cpu().numpy(), want[2])
    # the device root errs by at most 1 float64 ulp before the cast: at most 1 float32 ulp from the correctly rounded root
    assert _ulps(sp.row_norms(2).cpu().numpy(), np.float32(np.sqrt(want[3]))).max() <= 1
    assert np.array_equal(bits(sp.row_norms(1).cpu().numpy()), bits(want[2].astype(np.float32)))
    sp.set_values("length", st.cells.cpu().numpy())                            # document length as a field
    assert int(sp.value_stats("length").max[0]) == want[0].max()
    with pytest.raises(ValueError, match="p must be"):
        sp.row_norms(3)


def test_facade_idf_weighted_bot_index():
    from vsearch_amd.ir import BoTIndex, SparseIndex
    rng = np.random.default_rng(22)
    n = 1500
    ip, ix, _ = make_csr(rng.integers(0, 60, size=n), VN, rng)
    bot = BoTIndex(device="cuda:0", fp16=False)
    bot.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix), torch.ones(len(ix)), size=(n, VN))
    bot.move_to_device("cuda:0")
    bot.data = [{"text": f"doc {i}"} for i in range(n)]
    bot.delete([3, 4])
    live = np.ones(n, bool)
    live[[3, 4]] = False
    df = np.bincount(ix[np.repeat(live, np.diff(ip))], minlength=VN).astype(np.float64)
    for k in (0.5, 1.0):
        want = np.where(df > 0, np.log(1 + (live.sum() - df + k) / (df + k)), 0.0).astype(np.float32)
        w = bot.idf_weights(k)
        assert w.dtype == torch.float32 and w.shape == (VN,)
        w = w.cpu().numpy()
        assert np.array_equal(w == 0, want == 0) and _ulps(w[want != 0], want[want != 0]).max() <= 1
    w = bot.idf_weights().cpu().numpy()
    new = bot.rescaled(col_scale=w)
    assert type(new) is SparseIndex and len(new) == n and new.n_live == n - 2 and new.get_sample(9) == bot.get_sample(9)
    got = new._device_index().export_csr()
    assert np.array_equal(got[0], ip) and np.array_equal(got[1], ix) and np.array_equal(bits(got[2]), bits(ref.rescale_ref(ip, ix, None, col_scale=w)))
    assert new._device_index().info().store_dtype == nat.VS_F32 and bot._device_index().info().store_dtype == nat.VS_NONE
    sums = new.term_sums()                                                     # a valued index now: the valued aggregations take it
    assert int(sums.total[0]) == n - 2 and int(sums.sums[0].sum()) > 0
    assert bot.rescaled(col_scale=w, dtype="fp16")._device_index().info().store_dtype == nat.VS_F16


def test_facade_astype_round_trip_and_carry(sparse_index):
    from vsearch_amd.ir import SparseIndex
    sp = sparse_index
    n = len(sp)
    sp.delete([10, 11])
    before = sp._device_index().export_csr()
    half = sp.astype("fp16")
    assert type(half) is SparseIndex and half._device_index().info().store_dtype == nat.VS_F16 and half.n_live == n - 2
    assert same_csr(sp._device_index().export_csr(), before)                   # the source is left exactly as it was
    h = half._device_index().export_csr()
    assert np.array_equal(bits(h[2]), bits(before[2].astype(np.float16).astype(np.float32)))
    back = half.astype("fp32").astype("fp16")                                  # fp16 -> fp32 -> fp16 is the identity on bits
    assert np.array_equal(bits(back._device_index().export_csr()[2]), bits(h[2])) and back._device_index().info().store_dtype == nat.VS_F16
    for new in (half, sp.rescaled(col_scale=np.full(VN, 2.0)), sp.normalized()):
        assert new.get_sample(7) == sp.get_sample(7) and torch.equal(new.groups, sp.groups) and new.n_live == n - 2
        assert _eq(tuple(new.facets("lang")), tuple(sp.facets("lang")))
        assert _eq(tuple(new.value_stats("year")), tuple(sp.value_stats("year")))
    new.set_facet("other", np.zeros(n, dtype=np.int64))                        # the registries are the new index's own
    assert "other" in new.facet_fields and "other" not in sp.facet_fields
    with pytest.raises(ValueError, match="dtype must be"):
        sp.astype("int8")


def test_facade_row_sharded(sparse_index):
    sp = sparse_index
    q = torch.from_numpy(oracle.synth_queries(6, 4, VN, 30)).to("cuda:0")
    want = sp.normalized().search(q, 20)
    norms = sp.row_norms(2)
    sp.shard_rows([0, 0, 0])
    new = sp.normalized()
    assert new.shards is not None and len(new.shards) == 3 and new.shards[0] is not sp.shards[0] and torch.equal(new.groups, sp.groups)
    got = new.search(q, 20)
    assert torch.equal(got.ids, want.ids) and torch.equal(got.scores, want.scores) and torch.equal(sp.row_norms(2), norms)


def test_retriever_calls_resolve_tokens(sparse_index):
    from vsearch_amd.ir import Retriever
    shift = 999
    tok = types.SimpleNamespace(vocab={f"tok{i}": i for i in range(VN + shift)})

    class Fake:                                  # (methods as class attributes: no reference cycle through the instance)
        normalize_index = Retriever.normalize_index
        reweight_index = Retriever.reweight_index
    fake = Fake()
    fake.index, fake.device = sparse_index, "cuda"
    fake.encoder_p = types.SimpleNamespace(tokenizer=tok, config=types.SimpleNamespace(shift_vocab_num=shift))
    before = sparse_index._device_index().export_csr()
    new = fake.reweight_index(token_weights={f"tok{shift}": 2.5, 17: 0.0})
    assert fake.index is sparse_index                                          # inplace defaults to False
    cs = np.ones(VN, np.float32)
    cs[0], cs[17] = 2.5, 0.0
    assert ref.same_values(new._device_index().export_csr()[2], ref.rescale_ref(*before, col_scale=cs))
    idf = sparse_index.idf_weights().cpu().numpy()
    both = fake.reweight_index(token_weights={"tok1000": 3.0}, idf=True)
    cs = idf.copy()
    cs[1] = np.float32(cs[1]) * np.float32(3.0)
    assert ref.same_values(both._device_index().export_csr()[2], ref.rescale_ref(*before, col_scale=cs))
    with pytest.raises(ValueError, match="tok5"):
        fake.reweight_index(token_weights={"tok5": 1.0})
    with pytest.raises(ValueError, match="not a column"):
        fake.reweight_index(token_weights={VN: 1.0})
    unit = fake.normalize_index(inplace=True)
    assert fake.index is unit and unit is not sparse_index


def test_facade_dense_matrix_index_is_refused():
    from vsearch_amd.ir import Index
    idx = Index(device="cuda:0")
    idx.vector = torch.randn(64, 128)
    idx.move_to_device("cuda:0")
    for call in (idx.row_stats, idx.normalized, lambda: idx.rescaled(row_scale=np.ones(64)), lambda: idx.astype("fp16"), lambda: idx.row_norms(2)):
        with pytest.raises(NotImplementedError, match="dense"):
            call()
