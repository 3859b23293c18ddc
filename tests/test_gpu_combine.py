"""GPU tests of the combined index (vs_index_combine; DeviceIndex / ShardGroup combine, Index.combined, Retriever.combine_index) -- run on MI355X.

Every case compares export_csr of the result with the numpy reference (tests/_combine_ref.py) of export_csr of the two sources: row pointers
and columns by array_equal, values by their BITS (where the reference holds a NaN, any NaN).  Both sources' exports are bit-identical before
and after.  Small indexes built from numpy CSR: V = 29 523, V = 300 for the narrow cases, 65 535 for the widest."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import V
from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, ShardGroup, combine_plan

import _combine_ref as ref

pytestmark = pytest.mark.gpu
VN = 300                                                 # the narrow vocabulary
VW = 65535                                               # the widest
STORES = {"fp32": nat.VS_F32, "fp16": nat.VS_F16, "binary": nat.VS_NONE}
OUTS = {"fp32": nat.VS_F32, "fp16": nat.VS_F16}


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------------------
def from_rows(rows, rng, values=None):
    """rows: a list of column lists in the order they are to be stored -> CSR with standard normal values (or values(n) -> float32 [n])"""
    ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ix = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows] + [np.zeros(0, np.int64)])
    d = (rng.standard_normal(len(ix)) if values is None else values(len(ix))).astype(np.float32)
    return ip, ix, d


def random_rows(lengths, n_cols, rng, order="shuffled"):
    rows = []
    for n in lengths:
        c = rng.permutation(n_cols)[:n]
        rows.append(c if order == "shuffled" else (np.sort(c)[::-1] if order == "descending" else np.sort(c)))
    return rows


def build(csr, n_cols, store=nat.VS_F32):
    ip, ix, d = csr
    return DeviceIndex.from_csr(ip, ix, None if store == nat.VS_NONE else d, n_cols, store_dtype=store)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def exported(idx):
    ip, ix, d = idx.export_csr()
    return ip, ix, (None if idx.info().store_dtype == nat.VS_NONE else d)


def same_export(x, y):
    return np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and (x[2] is None or np.array_equal(bits(x[2]), bits(y[2])))


def check(a, b, wa=1.0, wb=1.0, out=None, **extra):
    """combine a and b and compare with the reference -> (the new DeviceIndex, the reference's CSR)"""
    ea, eb = exported(a), exported(b)
    new = a.combine(b, wa, wb, out, **extra)
    assert same_export(exported(a), ea) and same_export(exported(b), eb), "a source changed"
    both_half = a.info().store_dtype == nat.VS_F16 and b.info().store_dtype == nat.VS_F16
    out_dtype = OUTS[out] if out is not None else (nat.VS_F16 if both_half else nat.VS_F32)
    want = ref.combine_ref(ea, eb, wa, wb, "fp16" if out_dtype == nat.VS_F16 else "fp32")
    got = new.export_csr()
    assert np.array_equal(got[0], want[0]), "row pointers"
    assert np.array_equal(got[1], want[1]), "columns"
    assert ref.same_values(got[2], want[2]), "value bits"
    ni = new.info()
    assert (ni.n_rows, ni.nnz, ni.n_cols, ni.store_dtype) == (a.n_rows, len(want[1]), a.info().n_cols, out_dtype)
    assert ni.n_packets == int(((np.diff(want[0]) + 7) // 8).sum())
    return new, want


# ---- row shapes, every pair of stores, both out dtypes ------------------------------------------------------------------------------------------------
def shape_rows(n_cols, rng):
    """-> (rows of a, rows of b): 0 / 1 / 7 / 8 / 9 cells a side in every pairing and shuffled order; disjoint, identical and partly overlapping
    columns; unions of exactly 8 and 9 cells; the bitmap's word edges; descending order"""
    ra, rb = [], []
    for na in (0, 1, 7, 8, 9):
        for nb in (0, 1, 7, 8, 9):
            ra.append(rng.permutation(40)[:na])                 # of 40 columns: partly overlapping
            rb.append(rng.permutation(40)[:nb])
    ra += [np.arange(0, 40, 2), rng.permutation(np.arange(0, 18, 2))]                      # disjoint: even | odd
    rb += [np.arange(1, 40, 2)[::-1], rng.permutation(np.arange(1, 18, 2))]
    same = rng.permutation(n_cols)[:21]
    ra += [same, same[:8]]                                                                # identical columns, another order
    rb += [rng.permutation(same), same[:8][::-1]]
    ra += [[4, 0, 3, 1, 2], [4, 0, 3, 1, 2]]                                              # unions of exactly 8 and 9
    rb += [[7, 3, 5, 4, 6], [8, 7, 3, 5, 4, 6]]
    edges = [0, 31, 32, 63, 64, n_cols - 1]
    ra += [edges, edges[::-1], [31, 64], [n_cols - 1]]                                    # the bitmap's word edges
    rb += [[63, 0, n_cols - 1, 32], edges, [32, 63, 0], [n_cols - 1]]
    big = rng.permutation(n_cols)[:200]
    ra += [np.sort(big[:150])[::-1], []]                                                  # descending, 100 shared columns; an empty last row
    rb += [np.sort(big[50:])[::-1], []]
    return ra, rb


@pytest.fixture(scope="module")
def shapes():
    rng = np.random.default_rng(1)
    ra, rb = shape_rows(VN, rng)
    ca, cb = from_rows(ra, rng), from_rows(rb, rng)
    return {name: (build(ca, VN, store), build(cb, VN, store)) for name, store in STORES.items()}


@pytest.mark.parametrize("out", list(OUTS))
@pytest.mark.parametrize("sb", list(STORES))
@pytest.mark.parametrize("sa", list(STORES))
def test_row_shapes_and_store_pairs(shapes, sa, sb, out):
    a, b = shapes[sa][0], shapes[sb][1]
    _, want = check(a, b, 0.75, -1.25, out)
    sizes = np.diff(want[0])
    assert sizes[0] == 0 and sizes[-1] == 0 and {8, 9} <= set(sizes.tolist())
    if sa != "fp16" or sb != "fp16":
        check(a, b)                                                                       # dtype None: fp32, unless both sources are fp16
    else:
        assert a.combine(b).info().store_dtype == nat.VS_F16


@pytest.mark.parametrize("n_cols", [VN, V, VW])
def test_widths(n_cols):
    rng = np.random.default_rng(n_cols)
    ra, rb = shape_rows(n_cols, rng)
    ra.insert(3, rng.permutation(n_cols)[:700])                                            # 88 packets: two rounds of a wave
    rb.insert(3, rng.permutation(n_cols)[:90])
    a, b = build(from_rows(ra, rng), n_cols), build(from_rows(rb, rng), n_cols, nat.VS_NONE)
    plan = a.combine_plan(b)
    assert plan == combine_plan(len(ra), a.info().n_packets, b.info().n_packets, n_cols, nat.VS_F32, nat.VS_NONE, nat.VS_F32)
    check(a, b, 1.0, 0.3)
    check(b, a, 2.0, -1.0, "fp16")


# ---- the edges of the two routes, read from the plan -------------------------------------------------------------------------------------------------
def test_route_edges_at_the_wave_limit():
    """cells_a + cells_b at the wave route's limit - 1 / at it / + 1, between short rows; a row of V cells on both sides"""
    rng = np.random.default_rng(2)
    limit = combine_plan(1, 1, 1, V, nat.VS_F32, nat.VS_F32, nat.VS_F32).wave_cells
    assert limit % 2 == 0
    h = limit // 2
    la = [5, h, 0, h, h, 3, V, 9, h + 76, h + 1, 7]                                          # (the last three: the wave route on rows too long to be
    lb = [9, h - 1, 2, h, h + 1, 0, V, 5, 9, h - 1, h + 1]                                   #  held in registers -- more than 128 packets a side)
    a, b = build(from_rows(random_rows(la, V, rng), rng), V), build(from_rows(random_rows(lb, V, rng, "descending"), rng), V, nat.VS_F16)
    _, want = check(a, b, 1.0, -0.5)
    assert np.diff(want[0])[6] == V
    check(b, a, 0.3, 1.0, "fp16")
    # a long row whose union is small: 1100 + 1100 cells on the same columns, and nothing but long rows
    cols = rng.permutation(V)[:1100]
    a2, b2 = build(from_rows([cols, rng.permutation(cols)], rng), V), build(from_rows([rng.permutation(cols), cols[::-1]], rng), V)
    _, want = check(a2, b2, 1.0, 1.0)
    assert np.diff(want[0]).tolist() == [1100, 1100]


def test_route_edges_at_the_workgroup_limit():
    """65 535 columns: a union of exactly group_cells cells is staged; one past it is refused by the count step, naming the row"""
    rng = np.random.default_rng(3)
    cap = combine_plan(1, 1, 1, VW, nat.VS_F32, nat.VS_F32, nat.VS_F32).group_cells
    assert cap < VW
    cols = rng.permutation(VW)
    na = 20000
    fit_a, fit_b = cols[:na], cols[na - 700:cap]                                             # 700 shared columns, a union of cap
    a = build(from_rows([[3, 1], fit_a, [5]], rng), VW)
    b = build(from_rows([[1, 2], fit_b, []], rng), VW, nat.VS_F16)
    _, want = check(a, b, 1.0, 0.5)
    assert np.diff(want[0]).tolist() == [3, cap, 1]
    b_over = build(from_rows([[1, 2], cols[na - 700:cap + 1], []], rng), VW, nat.VS_F16)    # one more column
    with pytest.raises(NotImplementedError, match=f"row 1 has a union of more than {cap} cells"):
        a.combine(b_over)
    h = C.c_void_p()
    rc = nat.lib().vs_index_combine(a._h, b_over._h, C.c_float(1.0), C.c_float(1.0), nat.VS_F32, 0, 0, 0, C.byref(h))
    assert rc == nat.VS_EUNSUPPORTED and not h.value                                         # no handle is made
    check(a, b, -1.0, 1.0, "fp16")                                                           # ... and the next call is served


# ---- row counts ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 4097])
def test_row_counts(n_rows):
    """rows of 0 to 20 cells a side; the first and the last row are empty on both sides"""
    rng = np.random.default_rng(n_rows)
    la, lb = rng.integers(0, 21, size=n_rows), rng.integers(0, 21, size=n_rows)
    la[0] = lb[0] = la[-1] = lb[-1] = 0
    base = np.argsort(rng.random((n_rows, 60)), axis=1)                                      # a shuffled row of 60 columns each
    ca = from_rows([base[r, :la[r]] for r in range(n_rows)], rng)
    cb = from_rows([base[r, 10:10 + lb[r]] for r in range(n_rows)], rng)
    check(build(ca, VN), build(cb, VN, nat.VS_F16), 1.0, 0.3)
    if n_rows in (1, 4097):
        check(build(cb, VN, nat.VS_NONE), build(ca, VN), 0.5, 2.0, "fp16")


@pytest.mark.parametrize("n_rows", [4096, 4097])
def test_row_pointers_from_unions_of_0_8_and_9_cells(n_rows):
    """the scan from the union counts to the row pointers: one scan block, and a second block of one row; unions of no packet, exactly one packet
    and one cell more"""
    rng = np.random.default_rng(n_rows)
    uni = rng.choice([0, 8, 9], size=n_rows)
    uni[-1] = 9                                                                              # the row of the second block holds two packets
    base = np.argsort(rng.random((n_rows, 60)), axis=1)
    ca = from_rows([base[r, :min(uni[r], 5)] for r in range(n_rows)], rng)                   # 5 cells of a, cells 3 .. u of b: two shared columns
    cb = from_rows([base[r, 3:uni[r]] for r in range(n_rows)], rng)
    new, _ = check(build(ca, VN), build(cb, VN), 1.0, -0.5)
    assert np.array_equal(new.export_csr()[0], np.concatenate([[0], np.cumsum(uni)]))
    assert new.info().n_packets == int(((uni + 7) // 8).sum())


def test_an_index_without_a_packet():
    rng = np.random.default_rng(4)
    full = build(from_rows(random_rows([3] * 70, VN, rng), rng), VN)
    none, _ = full.prune(keep_cols=[])                                                       # every cell dropped: 70 rows, no packet
    assert none.info().n_packets == 0 and none.n_rows == 70
    new, want = check(none, none)
    assert new.info().n_packets == 0 and new.n_rows == 70
    _, want = check(none, full, 1.0, 2.0)
    assert np.array_equal(want[0], np.arange(71) * 3)
    check(full, none, 3.0, 1.0, "fp16")


# ---- weights and values ----------------------------------------------------------------------------------------------------------------------------------
WEIGHTS = [(1.0, 1.0), (1.0, -1.0), (-1.0, 0.0), (0.0, 0.0), (0.3, 1.0), (1.0, 0.3), (np.inf, 1.0), (1.0, -np.inf), (np.nan, 1.0), (0.0, np.inf)]


@pytest.mark.parametrize("out", list(OUTS))
def test_weights_are_data(shapes, out):
    a, b = shapes["fp32"][0], shapes["fp16"][1]
    for wa, wb in WEIGHTS:
        check(a, b, wa, wb, out)
    check(a, shapes["binary"][1], np.nan, np.inf, out)


@pytest.mark.parametrize("store", list(STORES))
def test_a_minus_a_keeps_every_cell_at_plus_zero(shapes, store):
    a = shapes[store][0]
    for out in OUTS:
        new, want = check(a, a, 1.0, -1.0, out)
        src = a.export_csr()
        order = np.concatenate([s + np.argsort(src[1][s:e], kind="stable") for s, e in zip(src[0][:-1], src[0][1:])] + [np.zeros(0, np.int64)]).astype(np.int64)
        assert np.array_equal(want[0], src[0]) and np.array_equal(want[1], src[1][order])    # the sparsity is the source's, sorted
        assert not bits(new.export_csr()[2]).any()                                           # +0 everywhere, never -0
    twice, want = check(a, a, 1.0, 1.0)                                                      # a is b: 2 a
    if store != "binary":
        assert np.array_equal(bits(want[2]), bits(2 * src[2][order]))


SPECIAL = [  # (a, b): wa = 1, wb = 1
    (0.0, 0.0), (-0.0, -0.0), (-0.0, 0.0), (5.0, -5.0), (1e-40, 1e-40), (1e-40, -1e-40), (3e38, 3e38), (-3e38, -3e38),       # zeros, fp32 subnormals, overflow
    (2.0 ** -24, 0.0), (2.0 ** -25, 0.0), (2.0 ** -25, 2.0 ** -26), (-(2.0 ** -25), 0.0), (2.0 ** -14, -(2.0 ** -25)),       # fp16 subnormals, underflow to +-0
    (1.0, 2.0 ** -11), (1.0, 3 * 2.0 ** -11), (65504.0, 15.0), (65504.0, 16.0), (-65504.0, -16.0),                           # fp16 ties to even, the overflow
    (1 + 2.0 ** -11, 2.0 ** -40),       # float32 takes the sum onto the fp16 tie, which goes to 1; ONE rounding would give 1 + 2^-10
    (1.0, 2.0 ** -24), (1.0, 3 * 2.0 ** -25), (np.inf, -np.inf), (np.inf, 1.0), (np.nan, 1.0), (1.0, np.nan),                # float32 ties, inf - inf, NaN
]


@pytest.mark.parametrize("out", list(OUTS))
def test_special_values(out):
    n = len(SPECIAL)
    ip = np.array([0, n, n + 2], dtype=np.int64)
    ix = np.concatenate([np.arange(n), [7, 2]]).astype(np.int64)
    da = np.array([x for x, _ in SPECIAL] + [1.0, -2.0], dtype=np.float32)
    db = np.array([y for _, y in SPECIAL] + [0.5, 0.25], dtype=np.float32)
    back = np.concatenate([np.arange(n)[::-1], [n + 1, n]])                                  # b stores its rows back to front
    a, b = build((ip, ix, da), VN), build((ip, ix[back], db[back]), VN)
    assert np.array_equal(bits(a.export_csr()[2]), bits(da))                                 # subnormals, NaN and -0.0 are stored as given
    _, want = check(a, b, 1.0, 1.0, out)
    v = want[2][:n]
    assert bits(v[:4]).tolist() == [0, 0x80000000, 0, 0] and np.isnan(v[[21, 23, 24]]).all() and v[22] == np.inf
    if out == "fp16":
        assert v[8] == 2.0 ** -24 and bits(v[9:12]).tolist() == [0, bits(np.float32(2.0 ** -24))[0], 0x80000000] and v[12] == 2.0 ** -14
        assert v[13] == 1.0 and v[14] == 1 + 2.0 ** -9 and v[15] == 65504.0 and v[16] == np.inf and v[17] == -np.inf and v[18] == 1.0
    else:
        assert v[4] == np.float32(1e-40) + np.float32(1e-40) and v[5] == 0 and v[6] == np.inf and v[7] == -np.inf and v[18] == np.float32(1 + 2.0 ** -11)
        assert v[19] == 1.0 and v[20] == np.float32(1 + 2.0 ** -23)
    for wa, wb in ((0.5, 0.5), (2.0 ** -10, 3.0), (-1.0, np.inf), (0.0, 1.0)):
        check(a, b, wa, wb, out)
    check(build((ip, ix, da), VN, nat.VS_F16), b, 2.0 ** -10, 2.0 ** -12, out)


# ---- repeated columns ------------------------------------------------------------------------------------------------------------------------------------
def test_a_repeated_column_is_refused_naming_the_lowest_row():
    rng = np.random.default_rng(5)
    ok = from_rows([[1, 2], [3, 4, 5], [], [6, 7], [8, 9, 10], [11]], rng)
    rep4 = from_rows([[1, 2], [3, 4, 5], [], [6, 7], [8, 9, 8], [11]], rng)
    rep1 = from_rows([[1, 2], [5, 4, 5], [], [6, 7], [8, 9, 10], [7, 7]], rng)
    far = from_rows([[1, 2], [3, 4, 5], [], [6, 7], [8, 9, 10], list(range(20, 90)) + [20]], rng)       # the repeat sits nine packets apart
    idx = {name: build(csr, VN, store) for name, csr, store in (("ok", ok, nat.VS_F32), ("rep4", rep4, nat.VS_F16), ("rep1", rep1, nat.VS_NONE), ("far", far, nat.VS_F32))}
    for a, b, source, row in (("rep4", "ok", "a", 4), ("ok", "rep4", "b", 4), ("rep4", "rep1", "b", 1), ("rep1", "rep4", "a", 1), ("rep1", "rep1", "a", 1),
                              ("far", "ok", "a", 5), ("ok", "far", "b", 5)):
        with pytest.raises(ValueError, match=f"row {row} of index {source} stores a column twice"):
            idx[a].combine(idx[b])
        with pytest.raises(ref.RepeatedColumn) as e:
            ref.combine_ref(exported(idx[a]), exported(idx[b]))
        assert (e.value.source, e.value.row) == (source, row)
    h = C.c_void_p()
    rc = nat.lib().vs_index_combine(idx["ok"]._h, idx["rep1"]._h, C.c_float(1.0), C.c_float(1.0), nat.VS_F32, 0, 0, 0, C.byref(h))
    assert rc == nat.VS_EINVAL and not h.value
    check(idx["ok"], idx["ok"])                                                              # the same column in a and in b is no repeat


# ---- tombstones, capacity, devices, arguments ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow():
    rng = np.random.default_rng(9)
    n = 2100
    la, lb = rng.integers(0, 120, size=n), rng.integers(0, 40, size=n)
    la[:4], lb[:4] = [0, 1, 8, 9], [9, 0, 8, 1]
    ca, cb = from_rows(random_rows(la, VN, rng), rng), from_rows(random_rows(lb, VN, rng), rng)
    return ca, cb


def test_tombstones_are_ored_and_restore_brings_rows_back_combined(narrow):
    ca, cb = narrow
    a, b = build(ca, VN), build(cb, VN, nat.VS_NONE)
    n = a.n_rows
    dead_a, dead_b = np.array([0, 5, 31, 1000], dtype=np.int64), np.array([5, 32, n - 1], dtype=np.int64)
    a.delete_rows(dead_a)
    new, want = check(a, b, 1.0, 0.5)                                                        # deletions on one side only
    assert new.n_live == n - 4 and torch.equal(new.live_mask(), a.live_mask())
    b.delete_rows(dead_b)
    new, want = check(a, b, 1.0, 0.5)                                                        # cells come from the stored rows, deleted or not
    dead = np.union1d(dead_a, dead_b)
    assert new.n_live == n - len(dead) and torch.equal(new.live_mask(), a.live_mask() & b.live_mask())
    assert a.n_live == n - 4 and b.n_live == n - 3
    q = torch.from_numpy((np.random.default_rng(10).random((4, VN)) < 0.1).astype(np.float32)).to("cuda:0")
    ids, _ = new.search(q, 50)
    assert not np.isin(ids.cpu().numpy(), dead).any()
    new.restore_rows()
    assert new.n_live == n
    twin = DeviceIndex.from_csr(*want, VN)
    x, y = new.search(q, 50), twin.search(q, 50)
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    only_b, _ = check(build(ca, VN), b)
    assert only_b.n_live == n - 3


def test_spare_capacity_then_append(narrow):
    ca, cb = narrow
    a, b = build(ca, VN), build(cb, VN, nat.VS_F16)
    rng = np.random.default_rng(12)
    new, want = check(a, b, 1.0, -1.0, rows_extra=3, packets_extra=10)
    more = from_rows(random_rows([5, 0, 70], VN, rng, "sorted"), rng)
    new.append_csr(*more)
    got = new.export_csr()
    assert np.array_equal(got[0], np.concatenate([want[0], want[0][-1] + more[0][1:]]))
    assert np.array_equal(got[1], np.concatenate([want[1], more[1]])) and ref.same_values(got[2], np.concatenate([want[2], more[2]]))
    with pytest.raises(ValueError, match="exceeds the reserved"):
        check(a, b, 1.0, -1.0)[0].append_csr(*more)                                          # without the spare capacity there is no room
    for bad in (dict(rows_extra=-1), dict(packets_extra=-1)):
        with pytest.raises(ValueError):
            a.combine(b, **bad)


def test_arguments(narrow):
    ca, cb = narrow
    a, b = build(ca, VN), build(cb, VN)
    with pytest.raises(TypeError, match="other must be a DeviceIndex"):
        a.combine(cb)
    with pytest.raises(TypeError, match="must be a number"):
        a.combine(b, "1")
    with pytest.raises(ValueError, match="dtype must be"):
        a.combine(b, dtype="binary")
    with pytest.raises(ValueError, match=f"index a is 2100 x {VN}, index b 2099 x {VN}"):
        a.combine(b.slice_rows(0, 2099))
    with pytest.raises(ValueError, match=f"index b 2100 x {VN + 1}"):
        a.combine(build(cb, VN + 1))
    h = C.c_void_p()
    one = C.c_float(1.0)
    assert nat.lib().vs_index_combine(a._h, b._h, one, one, nat.VS_NONE, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and not h.value
    assert nat.lib().vs_index_combine(a._h, b._h, one, one, nat.VS_F32, 0, 0, 99, C.byref(h)) == nat.VS_EINVAL and "device" in nat.last_error()
    assert nat.lib().vs_index_combine(a._h, None, one, one, nat.VS_F32, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "NULL" in nat.last_error()


def test_onto_another_gpu(narrow):
    if nat.device_count() < 2:
        pytest.skip("one GPU")
    ca, cb = narrow
    a, b = build(ca, VN), build(cb, VN)
    a.delete_rows(np.array([3, 4], dtype=np.int64))
    new, _ = check(a, b, 1.0, 0.3, "fp16", device=1, rows_extra=2, packets_extra=2)
    assert new.device == 1 and new.n_live == a.n_rows - 2
    other = DeviceIndex.from_csr(*cb, VN, device=1)
    with pytest.raises(ValueError, match="index a lives on device 0, index b on device 1"):
        a.combine(other)


def test_dense_indexes():
    """a dense index stored as packets is combined like any other; the matrix-core kind is refused"""
    rng = np.random.default_rng(8)
    mat = (rng.standard_normal((70, 256)) * (rng.random((70, 256)) < 0.2)).astype(np.float32)
    other = (rng.standard_normal((70, 256)) * (rng.random((70, 256)) < 0.1)).astype(np.float32)
    pa, pb = DeviceIndex.from_dense(mat, max_density=1.0), DeviceIndex.from_dense(other, max_density=1.0)
    assert pa.info().kind == nat.VS_KIND_DENSE and pa.info().n_packets > 0
    new, _ = check(pa, pb, 1.0, 2.0)
    assert new.info().kind == nat.VS_KIND_DENSE
    for x, y in ((DeviceIndex.from_dense(mat), pb), (pa, DeviceIndex.from_dense(other))):
        with pytest.raises(NotImplementedError, match="dense"):
            x.combine(y)


# ---- sharding -----------------------------------------------------------------------------------------------------------------------------------------------
def test_shard_group_of_uneven_shards(narrow):
    ca, cb = narrow
    a, b = build(ca, VN), build(cb, VN, nat.VS_NONE)
    n = a.n_rows
    cuts = [0, 700, 1500, n]
    ga = ShardGroup([a.slice_rows(cuts[i], cuts[i + 1] - cuts[i], device=0) for i in range(3)])
    gb = ShardGroup([b.slice_rows(cuts[i], cuts[i + 1] - cuts[i], device=0) for i in range(3)])
    whole, want = check(a, b, 1.0, 0.3, "fp16")
    new = ga.combine(gb, 1.0, 0.3, "fp16")
    assert isinstance(new, ShardGroup) and new.n_rows == n
    parts = [s.export_csr() for s in new._shards]
    assert [len(p[0]) - 1 for p in parts] == [700, 800, n - 1500]
    assert np.array_equal(np.concatenate([np.diff(p[0]) for p in parts]), np.diff(want[0]))
    assert np.array_equal(np.concatenate([p[1] for p in parts]), want[1]) and ref.same_values(np.concatenate([p[2] for p in parts]), want[2])
    q = torch.from_numpy((np.random.default_rng(4).random((4, VN)) < 0.1).astype(np.float32)).to("cuda:0")
    x, y = new.search(q, 30), whole.search(q, 30)
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    assert [p.wave_cells for p in ga.combine_plan(gb)] == [2048] * 3
    other_cuts = [0, 701, 1500, n]
    gc = ShardGroup([b.slice_rows(other_cuts[i], other_cuts[i + 1] - other_cuts[i], device=0) for i in range(3)])
    with pytest.raises(ValueError, match="shard i is combined with shard i"):
        ga.combine(gc)
    with pytest.raises(TypeError, match="other must be a ShardGroup"):
        ga.combine(b)


# ---- the point of the feature: the exact top k of the weighted sum of two scores -----------------------------------------------------------------------------
def dyadic_pair(n, cells_a, cells_b, rng):
    """A: cells_a values i / 16 (i = 1 .. 32) a row, B: cells_b binary cells a row, columns drawn one from each of cells_a (cells_b) equal
    ranges of V and stored shuffled.  With weights and query values on the same dyadic grid every score below is exact in float32."""
    def cols(cells):
        w = V // cells
        c = np.arange(cells)[None, :] * w + rng.integers(0, w, size=(n, cells))
        return np.take_along_axis(c, np.argsort(rng.random((n, cells)), axis=1), 1).reshape(-1)
    ip_a, ip_b = np.arange(n + 1, dtype=np.int64) * cells_a, np.arange(n + 1, dtype=np.int64) * cells_b
    da = (rng.integers(1, 33, size=n * cells_a) / 16.0).astype(np.float32)
    return (ip_a, cols(cells_a), da), (ip_b, cols(cells_b), None)


def dyadic_queries(B, nnz, rng):
    q = np.zeros((B, V), np.float32)
    for b in range(B):
        q[b, rng.permutation(V)[:nnz]] = rng.integers(1, 17, size=nnz) / 8.0
    return torch.from_numpy(q).to("cuda:0")


@pytest.mark.parametrize("n,cells_a,postings", [(16500, 288, True), (3000, 96, False)])
def test_search_of_the_combined_index_is_the_exact_top_k_of_the_summed_score(n, cells_a, postings):
    """set_scores of the combined index is wa * set_scores(A) + wb * set_scores(B) bit for bit, and search() returns the brute-force top k of
    that sum by (score descending, id ascending) -- on an index large enough for a postings copy (16 384 rows of 256 cells) and on one below
    that gate"""
    rng = np.random.default_rng(n)
    ca, cb = dyadic_pair(n, cells_a, 40, rng)
    a = DeviceIndex.from_csr(*ca, V)
    b = DeviceIndex.from_csr(cb[0], cb[1], None, V)
    wa, wb, k = 1.0, 0.25, 100
    q = dyadic_queries(6, 120, rng)
    new = a.combine(b, wa, wb).prepare()
    info = new.info()
    assert (info.postings_state == 1 and info.aux_bytes > 0) if postings else info.postings_state != 1
    sa, sb, sc = a.set_scores(q), b.set_scores(q), new.set_scores(q)
    want = wa * sa + wb * sb                                                                 # exact in float32: dyadic values, small sums
    assert torch.equal(sc, want) and bool((want == (wa * sa.double() + wb * sb.double()).float()).all())
    top_sc, top_ids = torch.sort(want, dim=1, descending=True, stable=True)                  # stable: equal scores keep ascending ids
    ids, scores = new.search(q, k)
    assert (new.info().last_path >= 2) == postings
    assert torch.equal(ids, top_ids[:, :k]) and torch.equal(scores, top_sc[:, :k])
    assert bool((top_sc[:, k - 1] > 0).all())                                                 # k real hits a query


# ---- the facade ------------------------------------------------------------------------------------------------------------------------------------------------------
def _eq(x, y):
    if isinstance(x, tuple):
        return len(x) == len(y) and all(_eq(p, q) for p, q in zip(x, y))
    if isinstance(x, torch.Tensor):
        return x.shape == y.shape and bool(((x == y) | ((x != x) & (y != y))).all())
    return x == y


@pytest.fixture()
def pair(narrow):
    from vsearch_amd.ir import BoTIndex, SparseIndex
    ca, cb = narrow
    n = len(ca[0]) - 1
    sp = SparseIndex(device="cuda:0", fp16=False)
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ca[0]), torch.from_numpy(ca[1]), torch.from_numpy(ca[2]), size=(n, VN))
    sp.move_to_device("cuda:0")
    sp.data = [{"text": f"doc {i}"} for i in range(n)]
    sp.set_groups(np.arange(n) // 3)
    sp.set_facet("lang", np.arange(n) % 5, names=["a", "b", "c", "d", "e"])
    sp.set_values("year", (1990 + np.arange(n) % 30).astype(np.float32))
    bot = BoTIndex(device="cuda:0", fp16=False)
    bot.vector = torch.sparse_csr_tensor(torch.from_numpy(cb[0]), torch.from_numpy(cb[1]), torch.ones(len(cb[1])), size=(n, VN))
    bot.move_to_device("cuda:0")
    bot.data = [{"text": f"lexical {i}"} for i in range(n)]
    return sp, bot


def test_facade_exact_hybrid_recipe(pair):
    from vsearch_amd.ir import SparseIndex
    sp, bot = pair
    n = len(sp)
    sp.delete([10, 11])
    bot.delete([11, 12])
    idf = bot.idf_weights()
    lexical = bot.rescaled(col_scale=idf)
    before = exported(sp._device_index())
    new = sp.combined(lexical, 1.0, 0.3)
    assert type(new) is SparseIndex and new is not sp and len(new) == n and new.n_live == n - 3
    assert same_export(exported(sp._device_index()), before) and sp.n_live == n - 2 and bot.n_live == n - 2
    want = ref.combine_ref(before, exported(lexical._device_index()), 1.0, 0.3)
    assert ref.same_csr(new._device_index().export_csr(), want)
    assert new.get_sample(7) == sp.get_sample(7) and torch.equal(new.groups, sp.groups)      # texts, groups and fields are this index's
    new.set_facet("other", np.zeros(n, dtype=np.int64))                                      # the registries are the new index's own
    assert "other" in new.facet_fields and "other" not in sp.facet_fields
    q = torch.from_numpy((np.random.default_rng(30).random((4, VN)) < 0.1).astype(np.float32)).to("cuda:0")
    res = new.search(q, 20)
    twin = DeviceIndex.from_csr(*want, VN)
    twin.delete_rows(np.array([10, 11, 12], dtype=np.int64))
    ids, scores = twin.search(q, 20)
    assert torch.equal(res.ids, ids) and torch.equal(res.scores, scores)
    raw = bot.combined(sp, 2.0, 1.0, dtype="fp16")                                           # a BoTIndex comes back valued
    assert type(raw) is SparseIndex and raw._device_index().info().store_dtype == nat.VS_F16 and raw.get_sample(7) == bot.get_sample(7)
    assert ref.same_csr(raw._device_index().export_csr(), ref.combine_ref(exported(bot._device_index()), before, 2.0, 1.0, "fp16"))
    with pytest.raises(TypeError, match="other must be an index"):
        sp.combined(np.zeros(3))
    sp.delete([12])                                                                          # now sp's live documents are the combined index's
    assert _eq(tuple(new.facets("lang")), tuple(sp.facets("lang"))) and _eq(tuple(new.value_stats("year")), tuple(sp.value_stats("year")))


def test_facade_row_sharded(pair):
    sp, bot = pair
    q = torch.from_numpy((np.random.default_rng(31).random((4, VN)) < 0.1).astype(np.float32)).to("cuda:0")
    want = sp.combined(bot, 1.0, 0.5).search(q, 20)
    with_one = sp.combined(bot, 1.0, 0.5)
    sp.shard_rows([0, 0, 0])
    with pytest.raises(ValueError, match="row-sharded exactly as this index"):
        sp.combined(bot)
    bot.shard_rows([0, 0, 0])
    new = sp.combined(bot, 1.0, 0.5)
    assert new.shards is not None and len(new.shards) == 3 and new.shards[0] is not sp.shards[0] and torch.equal(new.groups, with_one.groups)
    got = new.search(q, 20)
    assert torch.equal(got.ids, want.ids) and torch.equal(got.scores, want.scores)


def test_retriever_combine_index(pair):
    from vsearch_amd.ir import Retriever
    sp, bot = pair

    class Fake:                                  # (the method as a class attribute: no reference cycle through the instance)
        combine_index = Retriever.combine_index
    fake = Fake()
    fake.index = sp
    new = fake.combine_index(bot, 1.0, 0.3)
    assert fake.index is sp                                                                  # inplace defaults to False
    want = ref.combine_ref(exported(sp._device_index()), exported(bot._device_index()), 1.0, 0.3)
    assert ref.same_csr(new._device_index().export_csr(), want)
    swapped = fake.combine_index(bot, 1.0, 0.3, inplace=True)
    assert fake.index is swapped and swapped is not sp
    fake.index = None
    with pytest.raises(RuntimeError, match="no index"):
        fake.combine_index(bot, 1.0, 1.0)


def test_facade_dense_index_is_refused(pair):
    from vsearch_amd.ir import Index
    sp, _ = pair
    idx = Index(device="cuda:0")
    idx.vector = torch.randn(len(sp), VN)
    idx.move_to_device("cuda:0")
    with pytest.raises(NotImplementedError, match="dense"):
        idx.combined(sp)
    with pytest.raises(NotImplementedError, match="dense"):
        sp.combined(idx)
