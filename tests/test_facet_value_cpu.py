"""CPU checks of the breakdowns: the numpy reference against plain loops and, label by label, against the references of the
numeric fields and of the facet counts; the invariants; the shard rule; the plan rule (vs_facet_value_plan is pure host arithmetic); the
argument errors of the C ABI without a GPU; the facade's host logic; and the host-side code (vsearch_amd/csrc/facet_value_check.h) run in a
stand-alone program under the host sanitizers.  No device is needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd import device_index as di

import _facet_ref as fref
import _facet_value_ref as ref
import _value_ref as vref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, I32 = np.float32, np.int32
DTYPES = [F32, I32]


def _all_same(got, want):
    return len(got) == len(want) and all(ref.same(g, w) for g, w in zip(got, want))


def _case(dtype, n, B, L, bit0, seed, kind="mixed", with_live=False):
    v = ref.values_case(n, dtype, seed=seed, frac_missing=0.15, frac_special=0.2, spread=20)
    labels = ref.labels_shape(kind, n, L, seed + 1)
    masks = ref.masks_case(B, n, seed=seed + 2, density=0.9)
    words = ref.pack(masks, bit0, spare=1)
    aw = ref.pack((np.random.default_rng(seed + 3).random(n) < 0.8)[None, :], bit0, spare=1)[0] if with_live else None
    edges = ref.edges_case(3, dtype) if dtype == F32 else np.array([-5, 0, 3, 17], I32)
    return v, labels, masks, words, aw, edges


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bit0", [0, 5, 37])
@pytest.mark.parametrize("with_live", [False, True])
def test_reference_equals_the_loops(dtype, bit0, with_live):
    n, B, L = 150, 3, 4
    v, labels, _, words, aw, edges = _case(dtype, n, B, L, bit0, seed=bit0 + 1, with_live=with_live)
    want_s, want_h = ref.loops(words, bit0, n, labels, L, v, list(edges), aw)
    assert _all_same(ref.stats(words, words.shape[1], bit0, n, labels, L, v, aw), want_s)
    assert _all_same(ref.histogram(words, words.shape[1], bit0, n, labels, L, v, edges, aw), want_h)
    want_s, want_h = ref.loops(None, 0, n, labels, L, v, list(edges))                                # words = NULL: every row
    assert _all_same(ref.stats(None, 0, 0, n, labels, L, v), want_s) and _all_same(ref.histogram(None, 0, 0, n, labels, L, v, edges), want_h)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ref.LABEL_SHAPES)
def test_reference_against_the_existing_references(dtype, kind):
    """per label l: the stats / histogram of the numeric fields over set & (labels == l); count + missing: the facet counts"""
    n, B, L, bit0 = 700, 4, 7, 33
    v, labels, masks, words, aw, _ = _case(dtype, n, B, L, bit0, seed=11, kind=kind, with_live=True)
    edges = ref.edges_case(6, dtype, spread=20)
    ld = words.shape[1]
    count, missing, lo, hi, sm, total, other = ref.stats(words, ld, bit0, n, labels, L, v, aw)
    counts, below, above, hmiss, htotal, hother = ref.histogram(words, ld, bit0, n, labels, L, v, edges, aw)
    for l in range(L):
        wl = ref.pack(masks & (labels == l)[None, :], bit0)
        assert _all_same((count[:, l], missing[:, l], lo[:, l], hi[:, l], sm[:, l]), vref.stats(wl, ld, bit0, n, v, aw)), l
        assert _all_same((counts[:, l], below[:, l], above[:, l], hmiss[:, l]), vref.histogram(wl, ld, bit0, n, v, edges, aw)), l
    fc, ft, fo = fref.facet_counts(words, ld, bit0, n, labels, L, aw)
    assert (count + missing == fc).all() and (total == ft).all() and (other == fo).all() and (htotal == ft).all() and (hother == fo).all()
    assert (counts.sum(axis=2) + below + above + hmiss == fc).all()
    # the invariants
    assert (count.sum(axis=1) + missing.sum(axis=1) + other == total).all()
    assert (counts.sum(axis=(1, 2)) + below.sum(axis=1) + above.sum(axis=1) + hmiss.sum(axis=1) + hother == htotal).all()
    empty = count == 0
    assert vref.is_missing(lo[empty]).all() and vref.is_missing(hi[empty]).all() and (sm[empty] == 0).all()
    if dtype == F32 and empty.any():
        assert (vref.bits(lo[empty]) == vref.NAN_BITS).all() and (vref.bits(hi[empty]) == vref.NAN_BITS).all()
    if kind == "none":
        assert (other == total).all() and not count.any() and not missing.any() and not counts.any()


def test_zeros_missing_and_wrapping_sums():
    labels = np.array([0, 0, 1, 1, 2, -1, 3, 3], I32)
    v = np.array([-0.0, 0.0, np.nan, -np.nan, np.inf, 5.0, 2.0 ** 21, -3e38], F32)
    count, missing, lo, hi, sm, total, other = ref.stats(None, 0, 0, 8, labels, 5, v)
    assert count[0].tolist() == [2, 0, 1, 2, 0] and missing[0].tolist() == [0, 2, 0, 0, 0] and total[0] == 8 and other[0] == 1
    assert vref.bits(lo[0, :1])[0] == 0 and vref.bits(hi[0, :1])[0] == 0                                      # +0.0 of either zero
    assert np.isnan(lo[0, 1]) and np.isnan(lo[0, 4]) and hi[0, 2] == np.inf and sm[0, 2] == 1 << 44           # clamped to 2^20
    assert sm[0, 3] == 0 and lo[0, 3] == F32(-3e38) and hi[0, 3] == F32(2.0 ** 21)                             # +2^44 - 2^44
    big = np.full(6, (1 << 31) - 1, I32)
    big[5] = ref.INT32_MIN
    st = ref.stats(None, 0, 0, 6, np.zeros(6, I32), 1, big)
    assert st[0][0, 0] == 5 and st[1][0, 0] == 1 and st[4][0, 0] == 5 * ((1 << 31) - 1)
    assert ref.unkey(vref.key(v), F32)[[0, 4, 7]].tolist() == [0.0, np.inf, F32(-3e38)] and ref.unkey(vref.key(big), I32).tolist() == big.tolist()
    st = di.FacetValueStats(np.array([[2, 0]]), np.array([[0, 1]]), np.array([[1.0, np.nan]], F32), np.array([[2.0, np.nan]], F32),
                            np.array([[3 << 24, 0]]), np.array([3]), np.array([0]))
    m = st.mean()
    assert m.dtype == np.float64 and m.shape == (1, 2) and m[0, 0] == 1.5 and np.isnan(m[0, 1])              # an empty cell: NaN
    st = di.FacetValueStats(torch.tensor([[4, 0]]), torch.tensor([[0, 0]]), torch.tensor([[1, ref.INT32_MIN]], dtype=torch.int32),
                            torch.tensor([[9, ref.INT32_MIN]], dtype=torch.int32), torch.tensor([[18, 0]]), torch.tensor([4]), torch.tensor([0]))
    assert st.mean().dtype == torch.float64 and float(st.mean()[0, 0]) == 4.5 and bool(torch.isnan(st.mean()[0, 1]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cut", [1, 31, 32, 33])
def test_shard_rule(dtype, cut):
    """every shard works on its slice of the labels and the values and its bit range [cut, n) of the bitmap; merged = the whole"""
    n, B, L = 300, 4, 5
    v, labels, masks, _, _, _ = _case(dtype, n, B, L, 0, seed=cut)
    if dtype == I32:
        v[[0, n - 1]] = ((1 << 24) + 1, (1 << 30) + 3)                                                        # values fp32 cannot hold
    words = ref.pack(masks)
    ld = words.shape[1]
    parts = [(0, cut), (cut, n)]
    got = ref.merge_stats([ref.stats(words, ld, r0, r1 - r0, labels[r0:r1], L, v[r0:r1]) for r0, r1 in parts])
    assert _all_same(got, ref.stats(words, ld, 0, n, labels, L, v))
    edges = ref.edges_case(9, dtype, spread=15)
    got = ref.merge_histogram([ref.histogram(words, ld, r0, r1 - r0, labels[r0:r1], L, v[r0:r1], edges) for r0, r1 in parts])
    assert _all_same(got, ref.histogram(words, ld, 0, n, labels, L, v, edges))


# ---- the plan rule ---------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_constants():
    text = open(os.path.join(REPO, "include", "vsearch_hip.h")).read()
    get = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert get("VS_FACET_VALUE_LDS_RECORDS") == nat.FACET_VALUE_LDS_RECORDS == 2048
    assert get("VS_FACET_VALUE_MAX_CELLS") == nat.FACET_VALUE_MAX_CELLS == 1 << 22
    assert 24 * nat.FACET_VALUE_LDS_RECORDS == 48 * 1024
    for name in ("vs_facet_value_plan", "vs_facet_value_stats", "vs_index_facet_value_stats", "vs_facet_value_histogram",
                 "vs_index_facet_value_histogram"):
        assert name in nat.EXPORTED_SYMBOLS and ("VS_API int %s(" % name) in text


def _plan_rule(n_rows, B, L, n_slots, per_query, rpc):
    cells = L * (n_slots or 1)
    cap = nat.FACET_LDS_BINS if n_slots else nat.FACET_VALUE_LDS_RECORDS
    regime = 1 if cells > cap else 0
    qt = 8 if per_query else 1
    while not regime and qt > 1 and qt * cells > cap:
        qt //= 2
    if rpc == 0:
        want = max(1, 1024 // -(-B // qt))
        rpc = max(-(-n_rows // want), 8192, 0 if regime else 16 * cells)
        rpc = -(-rpc // 2048) * 2048
    return regime, qt, -(-n_rows // rpc), rpc


@pytest.mark.parametrize("n_rows", [1, 65, 10_000, 21_015_324, (1 << 32) - 1])
@pytest.mark.parametrize("B,per_query", [(1, False), (1, True), (8, True), (9, True), (1000, True)])
def test_plan_against_its_rule(n_rows, B, per_query):
    shapes = [(L, 0) for L in (1, 12, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 70_000)]
    shapes += [(1, 4), (512, 4), (513, 4), (4096, 4), (4097, 4), (2, 1027), (15, 1027), (16, 1027), (1 << 20, 4)]
    for L, n_slots in shapes:
        for rpc_in in (0, 64, 1 << 20):
            got = di.facet_value_plan(n_rows, B, L, n_slots, per_query, rpc_in)
            assert got == _plan_rule(n_rows, B, L, n_slots, per_query, rpc_in), (L, n_slots, rpc_in)
            regime, qt, chunks, rpc = got
            assert rpc % 64 == 0 and chunks * rpc >= n_rows > (chunks - 1) * rpc and (rpc == rpc_in or not rpc_in)
    assert [di.facet_value_plan(10_000, 8, L, 0, True)[:2] for L in (256, 257, 512, 513, 1024, 1025, 2048, 2049)] == \
        [(0, 8), (0, 4), (0, 4), (0, 2), (0, 2), (0, 1), (0, 1), (1, 8)]


def test_plan_argument_errors():
    for args in [(0, 1, 4, 0, True, 0), (1 << 32, 1, 4, 0, True, 0), (100, 0, 4, 0, True, 0), (100, 1, 0, 0, True, 0), (100, 1, 4, 3, True, 0),
                 (100, 1, 4, 1028, True, 0), (100, 1, 4, -1, True, 0), (100, 1, 4, 0, True, 100), (100, 1, 4, 0, True, -64), (100, 2, 4, 0, False, 0),
                 (100, 8 * 65536, 1, 0, True, 0), (100, 1, (1 << 20) + 1, 4, True, 0), (100, 1 << 16, 1 << 15, 0, True, 0)]:
        with pytest.raises(ValueError):
            di.facet_value_plan(*args)
    with pytest.raises(ValueError, match="cells"):
        di.facet_value_plan(100, 1, 4085, 1027, True)
    o32, o64 = C.c_int32(0), C.c_int64(0)
    assert nat.lib().vs_facet_value_plan(100, 1, 4, 0, 1, 0, None, C.byref(o32), C.byref(o64), C.byref(o64)) == nat.VS_EINVAL
    assert nat.lib().vs_facet_value_plan(100, 1, 4, 0, 1, 0, C.byref(o32), C.byref(o32), C.byref(o64), C.byref(o64)) == nat.VS_OK


# ---- argument errors of the C ABI, checked before the device is touched ----------------------------------------------------------------------
def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def test_index_calls_refuse_a_null_handle_without_a_device():
    v, lab, o64, o32 = np.zeros(64, F32), np.zeros(64, I32), np.zeros(8, np.int64), np.zeros(8, F32)
    e = np.array([0, 1], F32)
    L = nat.lib()
    assert L.vs_index_facet_value_stats(None, None, 0, 0, 1, _p(lab), 2, _p(v), 0, 0, _p(o64), _p(o64), _p(o32), _p(o32), _p(o64), 2, _p(o64), _p(o64),
                                        None) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert L.vs_index_facet_value_histogram(None, None, 0, 0, 1, _p(lab), 2, _p(v), 0, _p(e), 2, 0, _p(o64), 1, _p(o64), _p(o64), _p(o64), _p(o64),
                                            _p(o64), None) == nat.VS_EINVAL and "NULL" in nat.last_error()


def test_argument_errors_without_a_device(have_gpu):
    good = nat.VS_OK if have_gpu else nat.VS_ENODEVICE
    n, nl = 100, 3
    L = nat.lib()
    vals = {0: ref.values_case(n, F32, 1), 1: ref.values_case(n, I32, 1)}
    labels = ref.labels_shape("mixed", n, nl, 2)
    words = np.full((3, 5), -1, np.int32)
    names = ("count", "missing", "lo", "hi", "sum", "total", "other")

    def stats(dt=0, B=3, bit0=0, ld=5, rpc=0, w=words, n_rows=n, n_labels=nl, ld_out=4, null=()):
        o = dict(count=np.zeros((3, 4), np.int64), missing=np.zeros((3, 4), np.int64), lo=np.zeros((3, 4), F32), hi=np.zeros((3, 4), F32),
                 sum=np.zeros((3, 4), np.int64), total=np.zeros(3, np.int64), other=np.zeros(3, np.int64))
        o = {k: (None if k in null else a) for k, a in o.items()}
        return L.vs_facet_value_stats(_p(w), bit0, ld, None, B, None if "labels" in null else _p(labels), n_labels,
                                      None if "values" in null else _p(vals[dt & 1]), dt, n_rows, rpc, _p(o["count"]), _p(o["missing"]), _p(o["lo"]),
                                      _p(o["hi"]), _p(o["sum"]), ld_out, _p(o["total"]), _p(o["other"]), 0, None)
    assert stats() == good and stats(dt=1) == good and stats(bit0=33) == good and stats(w=None, B=1, ld=0) == good and stats(rpc=64) == good
    assert stats(dt=2) == nat.VS_EINVAL and "dtype" in nat.last_error()
    assert stats(B=0) == nat.VS_EINVAL
    assert stats(bit0=-1) == nat.VS_EINVAL and "bit0" in nat.last_error()
    assert stats(bit0=64) == nat.VS_EINVAL and "ld_words" in nat.last_error()
    assert stats(ld=0) == nat.VS_EINVAL and "B = 1" in nat.last_error()
    assert stats(rpc=100) == nat.VS_EINVAL and "multiple of 64" in nat.last_error()
    assert stats(n_rows=0) == nat.VS_EINVAL and stats(n_labels=0) == nat.VS_EINVAL and "n_labels" in nat.last_error()
    assert stats(ld_out=2) == nat.VS_EINVAL and "ld_out" in nat.last_error()
    for k in ("labels", "values") + names:
        assert stats(null=(k,)) == nat.VS_EINVAL and "NULL" in nat.last_error()

    def hist(dt=0, edges=(0.0, 1.0, 2.0), ldc=4, B=3, ld=5, n_labels=nl, null=(), n_edges=None):
        o = dict(counts=np.zeros((3, nl, 4), np.int64), below=np.zeros((3, nl), np.int64), above=np.zeros((3, nl), np.int64),
                 missing=np.zeros((3, nl), np.int64), total=np.zeros(3, np.int64), other=np.zeros(3, np.int64))
        o = {k: (None if k in null else a) for k, a in o.items()}
        e = np.asarray(edges, dtype=F32 if dt == 0 else I32)
        return L.vs_facet_value_histogram(_p(words), 0, ld, None, B, None if "labels" in null else _p(labels), n_labels, _p(vals[dt]), dt, n,
                                          None if "edges" in null else _p(e), len(e) if n_edges is None else n_edges, 0, _p(o["counts"]), ldc,
                                          _p(o["below"]), _p(o["above"]), _p(o["missing"]), _p(o["total"]), _p(o["other"]), 0, None)
    assert hist() == good and hist(dt=1, edges=(-5, 0, 7)) == good and hist(edges=(-np.inf, np.inf)) == good
    assert hist(edges=(0.0,)) == nat.VS_EINVAL and "n_edges" in nat.last_error()
    assert hist(edges=np.arange(1026)) == nat.VS_EINVAL and "n_edges" in nat.last_error()
    assert hist(ldc=1) == nat.VS_EINVAL and "ld_counts" in nat.last_error()
    assert hist(edges=(0.0, 0.0, 1.0)) == nat.VS_EINVAL and "ascending" in nat.last_error()
    assert hist(edges=(-0.0, 0.0)) == nat.VS_EINVAL and "ascending" in nat.last_error()
    assert hist(edges=(0.0, np.nan)) == nat.VS_EINVAL and "missing" in nat.last_error()
    assert hist(dt=1, edges=(ref.INT32_MIN, 0)) == nat.VS_EINVAL and "missing" in nat.last_error()
    assert hist(n_labels=(1 << 20) + 1, B=1) == nat.VS_EINVAL and "cells" in nat.last_error()
    for k in ("labels", "edges", "counts", "below", "above", "missing", "total", "other"):
        assert hist(null=(k,)) == nat.VS_EINVAL and "NULL" in nat.last_error()


# ---- the facade's host logic -----------------------------------------------------------------------------------------------------------------
def test_python_argument_checks():
    lab, v = np.zeros(10, I32), np.zeros(10, F32)
    assert di._facet_value_args(lab, 3, v, 10, 128) == (3, nat.VAL_F32, 128, None)
    n_labels, dt, rpc, e = di._facet_value_args(torch.zeros(10, dtype=torch.int64), np.int64(2), torch.zeros(10, dtype=torch.int32), 10, 0, [1, 5])
    assert (n_labels, dt, rpc) == (2, nat.VAL_I32, 0) and e.dtype == I32 and e.tolist() == [1, 5]
    with pytest.raises(ValueError, match="one entry per row"):
        di._facet_value_args(lab, 3, np.zeros(11, F32), 10)                                                   # label / value length mismatch
    with pytest.raises(ValueError, match="one entry per row"):
        di._facet_value_args(np.zeros(11, I32), 3, v, 10)
    with pytest.raises(ValueError, match="n_labels"):
        di._facet_value_args(lab, 0, v, 10)
    with pytest.raises(TypeError):
        di._facet_value_args(lab.astype(F32), 3, v, 10)
    with pytest.raises(TypeError, match="float32 or int32"):
        di._facet_value_args(lab, 3, v.astype(np.float64), 10)
    with pytest.raises(ValueError, match="multiple of 64"):
        di._facet_value_args(lab, 3, v, 10, 100)
    for bad in ([1], [0, 0], [1, 0], [0, np.nan]):
        with pytest.raises(ValueError):
            di._facet_value_args(lab, 3, v, 10, 0, bad)
    with pytest.raises(ValueError, match="cells"):
        di._facet_value_args(lab, (1 << 20) + 1, v, 10, 0, [0, 1])


def test_index_facade_host_checks():
    from vsearch_amd.ir import SparseIndex
    idx = SparseIndex()
    idx._n_rows = lambda: 4
    idx._values = {"year": torch.tensor([1990, 2000, 2010, ref.INT32_MIN], dtype=torch.int32)}
    idx._facets = {"topic": (torch.zeros(4, dtype=torch.int32), 1, None)}
    for call in (lambda **kw: idx.stats_by_facet("nope", "topic", **kw), lambda **kw: idx.histogram_by_facet("nope", "topic", [0, 1], **kw)):
        with pytest.raises(KeyError, match="no value field"):
            call()
    for call in (lambda **kw: idx.stats_by_facet("year", "nope", **kw), lambda **kw: idx.histogram_by_facet("year", "nope", [0, 1], **kw)):
        with pytest.raises(KeyError, match="no facet field"):
            call()
    with pytest.raises(RuntimeError, match="no groups"):
        idx.stats_by_facet("year", "groups")
    with pytest.raises(ValueError, match="go together"):
        idx.stats_by_facet("year", "topic", q_embs=torch.zeros(1, 6))
    with pytest.raises(ValueError, match="go together"):
        idx.histogram_by_facet("year", "topic", [0, 1], min_score=0.5)
    for bad in ([1, 0], [0], [0.5, 1], [0, 1 << 31]):
        with pytest.raises(ValueError):
            idx.histogram_by_facet("year", "topic", bad)


# ---- the host-side code under the host sanitizers --------------------------------------------------------------------------------------------
def test_host_checks_under_a_host_sanitizer(tmp_path):
    """facet_value_check.h (every limit, the tile and regime boundaries at 256 / 257 .. 2048 / 2049 labels, the bins boundary, the 2^22-cell
    cap, the automatic chunk, strides too short) in a stand-alone program built with the host compiler under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "facet_value_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "facet_value_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "facet_value_check: ok" in run.stdout, run.stdout + run.stderr
