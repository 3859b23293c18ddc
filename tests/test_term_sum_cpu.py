"""CPU checks of the term sums: the numpy reference against a plain double loop, the fixed-point image of the edge values, the
shard rule, id lists, the top-n reference on cases small enough to work out by hand, the plan rule (vs_term_sum_plan is pure host arithmetic),
the argument errors of the C ABI without a GPU, the facade's host logic, and the host-side checks (vsearch_amd/csrc/term_sum_check.h) run in a
stand-alone program under the host sanitizers.  No device is needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd import device_index as di

import _term_agg_ref as aref
import _term_sum_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = nat.TERM_SUM_TILE_COLS
F32 = np.float32


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit0", [0, 5, 37])
@pytest.mark.parametrize("with_live", [False, True])
def test_reference_equals_the_double_loop(bit0, with_live):
    n, V, B = 45, 13, 3
    rng = np.random.default_rng(bit0 + 7 * with_live)
    lens = rng.integers(0, V + 1, size=n)
    lens[:3] = (0, 1, V)                                                  # an empty row, one cell, every column
    ip, ix, va = aref.csr_case(lens, V, seed=bit0, zeros=0.2)
    va = (va * rng.random(va.size).astype(F32)).astype(F32)               # fp32 values that fx rounds
    masks = rng.random((B, n)) < 0.6
    words = ref.pack(masks, bit0, spare=1)                                # (every bit outside the rows set: it must not count)
    live = ref.pack(rng.random((1, n)) < 0.7, 0, spare=1)[0] if with_live else None
    got = ref.term_sums(words, words.shape[1], bit0, ref.Cells(ip, ix, va, V), live)
    want = ref.term_sums_loop(words, words.shape[1], bit0, ip, ix, va, V, live)
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and (g == w).all()
    assert (got[0] != 0).any() and (got[0] < 0).any() and (got[0] % 256 != 0).any()
    if not with_live:
        assert (got[1] == masks.sum(axis=1)).all()
    binary = ref.term_sums(words, words.shape[1], bit0, ref.Cells(ip, ix, None, V), live)
    counts = aref.term_counts(words, words.shape[1], bit0, aref.has_matrix(ip, ix, None, V), live)
    assert (binary[0] == counts[0] * ref.ONE).all() and (binary[1] == counts[1]).all()


def test_fx_edges():
    two = lambda e: F32(2.0) ** e
    cases = [(two(-25), 0), (3 * two(-25), 2), (-two(-25), 0), (-3 * two(-25), -2), (5 * two(-25), 2), (two(-24), 1), (F32(0.0), 0),
             (F32(-0.0), 0), (F32(np.nan), 0), (two(20), 1 << 44), (-two(20), -(1 << 44)), (two(21), 1 << 44), (-two(21), -(1 << 44)),
             (F32(np.inf), 1 << 44), (F32(-np.inf), -(1 << 44)), (F32(1.0), 1 << 24), (F32(3.4e38), 1 << 44), (two(-149), 0),
             (np.nextafter(two(20), F32(0)), (1 << 44) - (1 << 20))]
    vals = np.array([c[0] for c in cases], dtype=F32)
    got = ref.fx(vals)
    assert got.dtype == np.int64 and got.tolist() == [c[1] for c in cases]
    assert ref.fx(np.array([2.0 ** -24], dtype=np.float16)).tolist() == [1]          # fp16's smallest subnormal
    assert ref.fx(np.array([np.inf, -np.inf, np.nan, 65504.0], dtype=np.float16)).tolist() == [1 << 44, -(1 << 44), 0, 65504 << 24]
    assert ref.FX_SHIFT == nat.TERM_FX_SHIFT and ref.FX_CLAMP_LOG2 == nat.TERM_FX_CLAMP_LOG2 and di.TERM_FX_ONE == ref.ONE


def test_fp16_and_binary_stores_are_exact_against_fractions():
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 1 << 16, size=4000).astype(np.uint16)
    h = bits.view(np.float16)
    h = h[np.isfinite(h)]
    h = np.concatenate([h, np.array([2.0 ** -24, -(2.0 ** -24), 65504.0, -65504.0, 0.0, -0.0], dtype=np.float16)])
    exact = sum((Fraction(float(x)) for x in h), Fraction(0)) * (1 << 24)
    assert exact.denominator == 1 and int(ref.fx(h).sum()) == exact.numerator        # every fp16 value is a multiple of 2^-24
    V = 5
    ip = np.arange(0, h.size + 1, dtype=np.int64)
    ix = (np.arange(h.size) % V).astype(np.int32)
    sums, total = ref.term_sums(None, 0, 0, ref.Cells(ip, ix, h.astype(F32), V))
    for c in range(V):
        assert int(sums[0, c]) == sum((Fraction(float(x)) for x in h[c::V]), Fraction(0)) * (1 << 24)
    assert total.tolist() == [h.size]
    sums, _ = ref.term_sums(None, 0, 0, ref.Cells(ip, ix, None, V))
    assert sums[0].tolist() == [len(range(c, h.size, V)) << 24 for c in range(V)]


def test_the_padding_column_and_stored_zeros_add_nothing_and_sums_wrap():
    V = 4
    ip = np.array([0, 4, 6, 6], dtype=np.int64)
    ix = np.array([0, 2, 3, V, 2, 3], dtype=np.int32)                     # row 0 carries the padding id V
    va = np.array([1.5, 0.0, -0.0, 9.0, -0.25, np.nan], dtype=F32)
    sums, total = ref.term_sums(None, 0, 0, ref.Cells(ip, ix, va, V))
    assert sums.tolist() == [[3 << 23, 0, -(1 << 22), 0]] and total.tolist() == [3]
    # 2^19 saturated rows reach 2^63: the int64 wraps, as the loop's Python integers reduced modulo 2^64 do
    cells = ref.Cells(np.array([0, 1]), np.array([0]), np.array([np.inf], dtype=F32), 1)
    assert cells.rows_sum(np.array([(1 << 19) - 1]))[0] == (1 << 63) - (1 << 44) and cells.rows_sum(np.array([1 << 19]))[0] == -(1 << 63)


@pytest.mark.parametrize("cut", [1, 31, 32, 33])
def test_shard_rule_sums_over_row_ranges_add_to_the_whole(cut):
    """every shard sums its own rows, reading them from bit `row0` of the global bitmap, and its own live bitmap from bit 0"""
    n, V, B = 150, 17, 4
    rng = np.random.default_rng(cut)
    ip, ix, va = aref.csr_case(rng.integers(0, 9, size=n), V, seed=cut, zeros=0.1)
    va = (va * rng.random(va.size).astype(F32)).astype(F32)
    cells = ref.Cells(ip, ix, va, V)
    masks = rng.random((B, n)) < 0.7
    alive = rng.random(n) < 0.8
    words = ref.pack(masks)
    whole = ref.term_sums(words, words.shape[1], 0, cells, ref.pack(alive[None, :])[0])
    bounds = [0, cut, cut + 64 + cut, n]
    parts = [ref.term_sums(words, words.shape[1], r0, cells.slice(r0, r1), ref.pack(alive[None, r0:r1])[0]) for r0, r1 in zip(bounds[:-1], bounds[1:])]
    for i in range(2):
        assert (sum(p[i] for p in parts) == whole[i]).all()
    ids = np.stack([rng.integers(-1, n, size=20) for _ in range(B)]).astype(np.int64)
    whole_ids = ref.term_sums_ids(ids, 0, cells, alive)
    parts = [ref.term_sums_ids(ids, r0, cells.slice(r0, r1), alive[r0:r1]) for r0, r1 in zip(bounds[:-1], bounds[1:])]
    for i in range(2):
        assert (sum(p[i] for p in parts) == whole_ids[i]).all()


def test_reference_id_lists():
    ip = np.array([0, 1, 2, 3, 5], dtype=np.int64)
    ix = np.array([0, 1, 2, 0, 3], dtype=np.int32)
    va = np.array([1.0, 2.0, 4.0, 0.5, 8.0], dtype=F32)
    cells = ref.Cells(ip, ix, va, 4)
    live = np.array([True, True, False, True])
    sums, total = ref.term_sums_ids(np.array([[0, 0, -1, 3, 2, 9, -7]]), 0, cells, live)
    assert total.tolist() == [3] and sums.tolist() == [[5 << 23, 0, 0, 8 << 24]]   # 0 twice, 3 once; -1, the deleted 2 and the outsiders skipped
    sums, total = ref.term_sums_ids(np.array([[10, 13, 9]]), 10, cells)
    assert total.tolist() == [2] and sums.tolist() == [[3 << 23, 0, 0, 8 << 24]]
    assert ref.check_strict(np.array([[0, 3, -1]]), 0, 4) and not ref.check_strict(np.array([[0, 4]]), 0, 4)     # strict: a host list is refused
    assert not ref.check_strict(np.array([[-2]]), 0, 4) and ref.check_strict(np.array([[13]]), 10, 4)


# ---- the top-n of the reference ------------------------------------------------------------------------------------------------------------
def test_topn_order_exclusions_and_ties():
    #                col:   0         1        2   3        4          5
    sums = np.array([[3 << 24, 6 << 24, -(1 << 24), 0, 6 << 24, 1 << 24]])
    cols, sc, sm = ref.topn(sums, [3], 6)
    assert cols.tolist() == [[1, 4, 0, 5, -1, -1]] and sc[0, :4].tolist() == [2.0, 2.0, 1.0, F32(1 / 3)] and np.isneginf(sc[0, 4:]).all()
    assert sm.tolist() == [[6 << 24, 6 << 24, 3 << 24, 1 << 24, 0, 0]]            # sum <= 0 is no candidate
    assert cols.dtype == np.int32 and sc.dtype == F32 and sm.dtype == np.int64
    assert ref.topn(sums, [3], 1)[0].tolist() == [[1]]                           # n cuts inside the tie: the smallest column
    assert (ref.topn(sums, [0], 4)[0] == -1).all()                               # total = 0 lists nothing
    # two fp64 scores that differ but round to the same fp32: the column decides
    s2 = np.array([[(1 << 40) + 1, 1 << 40, (1 << 40) + 2]])
    m = ref.mean(s2, [1])
    assert m[0, 0] == m[0, 1] == m[0, 2] and float(((1 << 40) + 1) * 2.0 ** -24) != float(2.0 ** 16)
    assert ref.topn(s2, [1], 3)[0].tolist() == [[0, 1, 2]]
    # min_count acts only through counts
    counts = np.array([[3, 1, 9, 9, 2, 0]])
    assert ref.topn(sums, [3], 6, None, 5)[0].tolist() == cols.tolist()
    assert ref.topn(sums, [3], 6, counts, 2)[0].tolist() == [[4, 0, -1, -1, -1, -1]]
    assert ref.topn(sums, [3], 6, counts, 0)[0].tolist() == cols.tolist()
    out = ref.topn(sums[:, :2], [3], 9)                                           # n > n_cols
    assert out[0].tolist() == [[1, 0] + [-1] * 7] and np.isneginf(out[1][0, 2:]).all() and (out[2][0, 2:] == 0).all()


def test_mean_is_the_fp64_chain():
    sums = np.array([[1, (1 << 53) + 1, -3, 7 << 24], [5, 5, 5, 5]], dtype=np.int64)
    m = ref.mean(sums, [3, 0])
    assert m.dtype == F32 and (m[1] == 0).all()
    for c in range(4):
        assert m[0, c] == F32((float(int(sums[0, c])) * 2.0 ** -24) / 3.0)
    ts = di.TermSums(sums, np.array([3, 0]))
    assert (ts.mean().view(np.uint32) == m.view(np.uint32)).all() and ts.mean().dtype == F32
    assert (ts.values() == sums.astype(np.float64) * 2.0 ** -24).all()
    tt = di.TermSums(torch.from_numpy(sums), torch.tensor([3, 0]))
    assert (tt.mean().numpy().view(np.uint32) == m.view(np.uint32)).all() and tt.values().dtype == torch.float64


# ---- the plan rule ---------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_constants():
    text = open(os.path.join(REPO, "include", "vsearch_hip.h")).read()
    get = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert get("VS_TERM_FX_SHIFT") == nat.TERM_FX_SHIFT == ref.FX_SHIFT == 24
    assert get("VS_TERM_FX_CLAMP_LOG2") == nat.TERM_FX_CLAMP_LOG2 == ref.FX_CLAMP_LOG2 == 20
    assert get("VS_TERM_SUM_TILE_COLS") == nat.TERM_SUM_TILE_COLS == ref.TILE_COLS == di.MAX_TERM_TILE_COLS
    assert nat.TERM_SUM_TILE_COLS * 8 + 1024 <= 160 * 1024                         # the bins and the counters fit a CU's LDS
    assert nat.TERM_FX_SHIFT + nat.TERM_FX_CLAMP_LOG2 + 19 == 63                   # 2^19 saturated rows before an int64 wraps


@pytest.mark.parametrize("V,tiles,tile_cols", [(1, 1, 1), (18432, 1, 18432), (18433, 2, 9217), (29523, 2, 14762), (36864, 2, 18432),
                                               (36865, 3, 12289), (65535, 4, 16384)])
def test_plan_tiles_are_balanced(V, tiles, tile_cols):
    for B, pq in ((9, True), (1, False)):
        got = di.term_sum_plan(10_000, B, V, pq)
        assert got[:2] == (tiles, tile_cols) and got == ref.plan(10_000, B, V)
    assert tiles * tile_cols >= V > (tiles - 1) * tile_cols and tile_cols <= TILE


def test_plan_takes_an_explicit_tile_as_given():
    for tc in (1, 7, 8, 40, 4096, TILE):
        got = di.term_sum_plan(5000, 3, 40, True, 0, tc)
        assert got[:2] == (-(-40 // tc), tc) and got == ref.plan(5000, 3, 40, 0, tc)
    assert di.term_sum_plan(5000, 3, 29523, True, 0, 4096)[:2] == (8, 4096)


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 2049, 10_000, 1_000_000, 21_000_000, (1 << 32) - 1])
@pytest.mark.parametrize("B,V", [(1, 1), (9, 29523), (64, 18433), (64, 65535)])
def test_plan_chunks_cover_the_rows(n_rows, B, V):
    for tc in (0, 4096):
        tiles = ref.plan(n_rows, B, V, 0, tc)[0]
        for rpc_in in (0, 64, 2048, 1 << 20):
            if rpc_in and -(-n_rows // rpc_in) * B * tiles > 0x7FFFFFFF:               # more work items than one grid holds
                with pytest.raises(ValueError, match="too many"):
                    di.term_sum_plan(n_rows, B, V, True, rpc_in, tc)
                continue
            got = di.term_sum_plan(n_rows, B, V, True, rpc_in, tc)
            assert got == ref.plan(n_rows, B, V, rpc_in, tc)
            _, _, chunks, rpc = got
            assert rpc > 0 and rpc % 64 == 0 and chunks * rpc >= n_rows > (chunks - 1) * rpc
            if rpc_in:
                assert rpc == rpc_in                                                   # an explicit value is taken as given
            else:
                assert rpc % 2048 == 0 and B * tiles * chunks <= max(1024, B * tiles)  # a few workgroups per CU over the batch


def test_plan_argument_errors():
    for args in [(0, 1, 4, True, 0, 0), (1 << 32, 1, 4, True, 0, 0), (100, 0, 4, True, 0, 0), (100, 1, 0, True, 0, 0), (100, 1, 65536, True, 0, 0),
                 (100, 1, 4, True, 100, 0), (100, 1, 4, True, -64, 0), (100, 2, 4, False, 0, 0), (100, 1, 4, True, 0, -1),
                 (100, 1, 4, True, 0, TILE + 1)]:
        with pytest.raises(ValueError):
            di.term_sum_plan(*args)
    with pytest.raises(ValueError, match="tile_cols"):
        di.term_sum_plan(100, 1, 4, True, 0, TILE + 1)
    with pytest.raises(ValueError, match="multiple of 64"):
        di.term_sum_plan(100, 1, 4, True, 100, 0)
    with pytest.raises(ValueError, match="too many"):                               # 2^26 chunks x 16 queries x 2 tiles = 2^31 work items
        di.term_sum_plan((1 << 32) - 1, 16, 8, True, 64, 4)
    assert di.term_sum_plan((1 << 32) - 1, 15, 8, True, 64, 4)[:3] == (2, 4, 1 << 26)
    o32, o64 = C.c_int32(0), C.c_int64(0)
    assert nat.lib().vs_term_sum_plan(100, 1, 4, 1, 0, 0, None, C.byref(o32), C.byref(o64), C.byref(o64)) == nat.VS_EINVAL
    assert nat.lib().vs_term_sum_plan(100, 1, 4, 1, 0, 0, C.byref(o32), C.byref(o32), C.byref(o64), C.byref(o64)) == nat.VS_OK


# ---- argument errors of the C ABI, checked before the device is touched ----------------------------------------------------------------------
def test_index_calls_refuse_a_null_handle_without_a_device():
    sums, total, ids = np.zeros((1, 4), np.int64), np.zeros(1, np.int64), np.zeros((1, 3), np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert nat.lib().vs_index_term_sums(None, None, 0, 0, 1, 0, 0, p(sums), 4, p(total), None) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert nat.lib().vs_index_term_sums_ids(None, p(ids), 1, 3, 3, 0, 1, 0, p(sums), 4, p(total), None) == nat.VS_EINVAL
    assert "NULL" in nat.last_error()


def test_topn_argument_errors_without_a_device(have_gpu):
    good = nat.VS_OK if have_gpu else nat.VS_ENODEVICE
    sums, total, counts = np.ones((2, 6), np.int64), np.full(2, 3, np.int64), np.ones((2, 6), np.int64)

    def call(n=3, V=6, ld=6, ldc=6, B=2, null=()):
        outs = dict(cols=np.zeros((2, max(n, 1)), np.int32), score=np.zeros((2, max(n, 1)), F32), out=np.zeros((2, max(n, 1)), np.int64))
        p = {k: C.c_void_p(v.ctypes.data) for k, v in dict(sums=sums, total=total, counts=counts, **outs).items()}
        for k in null:
            p[k] = None
        return nat.lib().vs_term_sum_topn(p["sums"], ld, p["total"], p["counts"], ldc, B, V, n, 1, p["cols"], p["score"], p["out"], 0, None)
    assert call() == good
    assert call(null=("counts",)) == good                                         # counts may be NULL ...
    assert call(null=("counts",), ldc=0) == good                                  # ... and then ld_counts is not looked at
    assert call(n=nat.TERM_MAX_TOPN + 1) == nat.VS_EINVAL and "1024" in nat.last_error()
    assert call(n=0) == nat.VS_EINVAL
    assert call(V=0) == nat.VS_EINVAL
    assert call(ld=5) == nat.VS_EINVAL and "ld_sums" in nat.last_error()
    assert call(ldc=5) == nat.VS_EINVAL and "ld_counts" in nat.last_error()
    assert call(B=0) == nat.VS_EINVAL
    for k in ("sums", "total", "cols", "score", "out"):
        assert call(null=(k,)) == nat.VS_EINVAL and "NULL" in nat.last_error()


# ---- the facade's host logic -----------------------------------------------------------------------------------------------------------------
def test_facade_validation_needs_no_device():
    from vsearch_amd.ir import SparseIndex
    from vsearch_amd.ir.retriever.retriever import Retriever
    assert di._weight_topn_args(20, 0) == (20, 0) and di._weight_topn_args(np.int64(1), np.int32(3)) == (1, 3)
    for bad in (dict(topn=0), dict(topn=1025)):
        with pytest.raises(ValueError):
            di._weight_topn_args(**{"topn": 5, "min_count": 0, **bad})
    for bad in (dict(topn=2.0), dict(topn=True), dict(min_count="1")):
        with pytest.raises(TypeError):
            di._weight_topn_args(**{"topn": 5, "min_count": 0, **bad})
    assert di._term_sum_args(0, 0) == (0, 0) and di._term_sum_args(np.int64(128), TILE) == (128, TILE)
    for bad in ((100, 0), (-64, 0), (True, 0), (0, -1), (0, TILE + 1), (0, 2.0), (64.0, 0)):
        with pytest.raises(ValueError):
            di._term_sum_args(*bad)
    sums = np.ones((2, 6), np.int64)
    with pytest.raises(ValueError, match="total"):
        di.term_sum_topn(sums, np.ones(3, np.int64), 3)
    with pytest.raises(ValueError, match="counts"):
        di.term_sum_topn(sums, np.ones(2, np.int64), 3, counts=np.ones((2, 5), np.int64))
    with pytest.raises(ValueError, match="topn"):
        di.term_sum_topn(sums, np.ones(2, np.int64), 0)
    idx = SparseIndex()
    with pytest.raises(ValueError, match="topn"):
        idx.centroid_terms(topn=0)
    with pytest.raises(ValueError, match="go together"):
        idx.term_sums(q_embs=torch.zeros(1, 6))
    with pytest.raises(ValueError, match="go together"):
        idx.centroid(min_score=0.5)
    with pytest.raises(ValueError, match="ids name the set"):
        idx.term_sums(filter=torch.ones(3, dtype=torch.bool), ids=torch.zeros(1, 2, dtype=torch.int64))
    for kwargs in (dict(), dict(min_score=0.5, k=3)):                             # the retriever: exactly one of min_score and k
        with pytest.raises(ValueError, match="exactly one"):
            Retriever.centroid_terms(None, ["q"], **kwargs)


# ---- the host-side checks under the host sanitizers ------------------------------------------------------------------------------------------
def test_host_checks_under_a_host_sanitizer(tmp_path):
    """term_sum_check.h (the plan rule with its column tiles, every limit of the three calls, and what vs_index_term_sums_ids checks in a host id
    list before it stages it) in a stand-alone program built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "term_sum_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "term_sum_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "term_sum_check: ok" in run.stdout, run.stdout + run.stderr
