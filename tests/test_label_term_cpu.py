"""CPU tests of the per-label term aggregations: the numpy reference against a plain double loop and against the per-label
composition it replaces, the plan rule and its limits, the C ABI's argument errors without a device, the facades' host-side errors, and the
host-only checks (label_term_check.h) in a stand-alone program under the host sanitizers.  No GPU is needed."""
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

import _label_term_ref as ref
import _term_agg_ref as aref
import _term_sum_ref as tref
from _facet_ref import masks_case

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
TILE = nat.TERM_SUM_TILE_COLS
ONE = ref.ONE


def _case(n, V, L, seed, binary=False):
    rng = np.random.default_rng(seed)
    ip, ix, va = aref.csr_case(rng.integers(0, 9, size=n), V, seed=seed + 1, zeros=0.15, binary=binary)
    if va is not None:
        va = (va * (0.5 + rng.random(va.size)).astype(F32)).astype(F32)
        va[rng.random(va.size) < 0.05] = np.nan                                       # a NaN is had and adds nothing
    lab = rng.integers(-1, L + 2, size=n).astype(np.int32)                            # -1 and L, L + 1: outside
    return ip, ix, va, lab


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit0,with_live,binary", [(0, False, False), (5, True, False), (37, True, True), (0, False, True)])
def test_reference_equals_the_double_loop(bit0, with_live, binary):
    n, V, L = 150, 23, 5
    ip, ix, va, lab = _case(n, V, L, 7 + bit0, binary)
    mask = masks_case(1, n, seed=3, density=0.8)[0]
    words = ref.pack(mask[None, :], bit0, spare=1)[0]
    live = np.random.default_rng(4).random(n) < 0.9
    lw = ref.pack(live[None, :])[0] if with_live else None
    cells, has = tref.Cells(ip, ix, va, V), aref.has_matrix(ip, ix, va, V)
    s, t, o = ref.label_term_sums(words, bit0, lab, L, cells, lw)
    c, t2, o2 = ref.label_term_counts(words, bit0, lab, L, has, lw)
    ls, lc, lt, lo = ref.label_terms_loop(words, bit0, lab, L, ip, ix, va, V, lw)
    assert (s == ls).all() and (c == lc).all() and (t == lt).all() and (t2 == lt).all() and o == lo == o2
    size = int((mask & live).sum()) if with_live else int(mask.sum())
    assert int(t.sum()) + o == size and o > 0 and (t > 0).all()                       # total.sum() + other == the size of the set
    if binary:
        assert (s == c * ONE).all()                                                   # a binary index's sums are its counts x 2^24
    # words = None: every row
    s0, t0, o0 = ref.label_term_sums(None, 0, lab, L, cells, lw)
    l0 = ref.label_terms_loop(None, 0, lab, L, ip, ix, va, V, lw)
    assert (s0 == l0[0]).all() and (t0 == l0[2]).all() and o0 == l0[3] and int(t0.sum()) + o0 == (int(live.sum()) if with_live else n)


def test_every_row_is_the_composition_it_replaces():
    """row l == term_sums / term_counts over label_bitmap(l) & set, the contract's first consequence"""
    n, V, L = 300, 40, 7
    ip, ix, va, lab = _case(n, V, L, 11)
    lab[lab == 3] = 2                                                                 # a label with no row: an all-zero row, total 0
    mask = masks_case(1, n, seed=12, density=0.8)[0]
    live = np.random.default_rng(13).random(n) < 0.9
    cells, has = tref.Cells(ip, ix, va, V), aref.has_matrix(ip, ix, va, V)
    lw = ref.pack(live[None, :])[0]
    s, t, o = ref.label_term_sums(ref.pack(mask[None, :])[0], 0, lab, L, cells, lw)
    c = ref.label_term_counts(ref.pack(mask[None, :])[0], 0, lab, L, has, lw)[0]
    sets = ref.pack((lab[None, :] == np.arange(L)[:, None]) & mask[None, :])
    ws, wt = tref.term_sums(sets, sets.shape[1], 0, cells, lw)
    wc, _ = aref.term_counts(sets, sets.shape[1], 0, has, lw)
    assert (s == ws).all() and (t == wt).all() and (c == wc).all() and t[3] == 0 and (s[3] == 0).all() and (c[3] == 0).all()
    assert (tref.mean(s, t)[3] == 0).all()                                            # .mean() of a label without rows: zeros


def test_the_label_order_and_its_sorted_segments():
    n, L = 200, 6
    lab = np.random.default_rng(21).integers(-1, L + 1, size=n).astype(np.int32)
    mask = masks_case(1, n, seed=22, density=0.8)[0]
    ptr, rows, other = ref.label_order(ref.pack(mask[None, :], 5, spare=1)[0], 5, lab, L)
    assert ptr[0] == 0 and ptr[-1] == rows.size and other == int((mask & ((lab < 0) | (lab >= L))).sum())
    for l in range(L):
        assert rows[ptr[l]:ptr[l + 1]].tolist() == np.flatnonzero(mask & (lab == l)).tolist()
    shuffled = rows.copy()
    rng = np.random.default_rng(23)
    for l in range(L):
        shuffled[ptr[l]:ptr[l + 1]] = rng.permutation(shuffled[ptr[l]:ptr[l + 1]])
    assert (ref.sorted_segments(ptr, shuffled) == rows).all() and (shuffled != rows).any()


def test_result_tuples_share_the_term_sums_chain():
    sums = np.array([[3 * ONE, -ONE // 2, 0], [0, 0, 0], [1, 2, 3]], dtype=np.int64)
    total = np.array([3, 0, 1 << 30], dtype=np.int64)
    r = di.LabelTermSums(sums, total, np.array([4]))
    m = tref.mean(sums, total)
    assert (r.mean().view(np.uint32) == m.view(np.uint32)).all() and r.mean().dtype == F32 and (r.mean()[1] == 0).all()
    assert (r.values() == sums.astype(np.float64) * 2.0 ** -24).all()
    rt = di.LabelTermSums(torch.from_numpy(sums), torch.from_numpy(total), torch.tensor([4]))
    assert (rt.mean().numpy().view(np.uint32) == m.view(np.uint32)).all() and rt.values().dtype == torch.float64


# ---- the plan rule ---------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_limits():
    text = open(os.path.join(REPO, "include", "vsearch_hip.h")).read()
    assert int(re.search(r"#define\s+VS_LABEL_TERM_MAX_LABELS\s+(\d+)", text).group(1)) == nat.LABEL_TERM_MAX_LABELS == ref.MAX_LABELS == 65536
    assert int(re.search(r"#define\s+VS_LABEL_TERM_MAX_CELLS\s+\(1ll << (\d+)\)", text).group(1)) == 27
    assert nat.LABEL_TERM_MAX_CELLS == ref.MAX_CELLS == di.MAX_LABEL_TERM_CELLS == 1 << 27
    assert int(re.search(r"#define\s+VS_LABEL_TERM_MAX_WORK_ITEMS\s+(\d+)", text).group(1)) == nat.LABEL_TERM_MAX_WORK_ITEMS == ((1 << 32) - 1) // 1024
    assert nat.FACET_LDS_BINS == ref.LDS_BINS and ref.LDS_BINS * 4 + 1024 <= 160 * 1024       # the label histogram fits a CU's LDS
    for name in ("vs_label_term_plan", "vs_label_order", "vs_index_label_term_sums", "vs_index_label_term_counts"):
        assert re.search(r"VS_API int %s\(" % name, text) and name in nat._SIGNATURES
    assert 4546 * 29523 <= ref.MAX_CELLS < 4547 * 29523 and 4546 > nat.ASSIGN_MAX_K


@pytest.mark.parametrize("V,tiles,tile_cols", [(1, 1, 1), (18432, 1, 18432), (18433, 2, 9217), (29523, 2, 14762), (65535, 4, 16384)])
def test_plan_tiles_are_the_term_sums(V, tiles, tile_cols):
    got = di.label_term_plan(10_000, 64, V)
    assert got[:2] == (tiles, tile_cols) == di.term_sum_plan(10_000, 1, V, False)[:2] and got == ref.plan(10_000, 64, V)
    for tc in (1, 7, 4096, TILE):
        assert di.label_term_plan(5000, 3, V, 0, tc)[:2] == (-(-V // tc), tc)


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 2049, 10_000, 1_000_000, 21_000_000, (1 << 32) - 1])
@pytest.mark.parametrize("L,V", [(1, 1), (12, 29523), (4096, 18433), (65536, 2048)])
def test_plan_items_and_their_bound(n_rows, L, V):
    for tc in (0, 1024):
        tiles = ref.plan(n_rows, L, V, 0, tc)[0]
        for rpi_in in (0, 64, 2048, 1 << 20):
            want = ref.plan(n_rows, L, V, rpi_in, tc)
            if want[3] > nat.LABEL_TERM_MAX_WORK_ITEMS // tiles:                      # more 1024-thread workgroups than one launch holds
                with pytest.raises(ValueError, match="too many"):
                    di.label_term_plan(n_rows, L, V, rpi_in, tc)
                continue
            got = di.label_term_plan(n_rows, L, V, rpi_in, tc)
            assert got == want
            _, _, rpi, max_items = got
            assert rpi > 0 and rpi % 64 == 0 and max_items == -(-n_rows // rpi) + L
            if rpi_in:
                assert rpi == rpi_in                                                  # an explicit value is taken as given
            else:
                assert rpi % 2048 == 0 and (max_items - L) * tiles <= max(1024, tiles)
            # the bound holds however the rows spread over the labels: even, one label, one row a label
            even = np.full(L, n_rows // L, dtype=np.int64)
            even[: n_rows % L] += 1
            lone = np.zeros(L, dtype=np.int64)
            lone[0] = n_rows
            thin = np.ones(L, dtype=np.int64) if n_rows >= L else even
            thin[-1] += n_rows - int(thin.sum())
            for split in (even, lone, thin):
                assert int(split.sum()) == n_rows and ref.n_items(split, rpi) <= max_items


def test_plan_and_facade_limits_at_their_last_valid_and_first_invalid_value():
    assert di.label_term_plan(100, 65536, 8)[3] == 1 + 65536
    with pytest.raises(ValueError, match="n_labels"):
        di.label_term_plan(100, 65537, 8)
    with pytest.raises(ValueError, match="n_labels"):
        di.label_term_plan(100, 0, 8)
    for args in [(0, 1, 4, 0, 0), (1 << 32, 1, 4, 0, 0), (100, 1, 0, 0, 0), (100, 1, 65536, 0, 0), (100, 1, 4, 100, 0), (100, 1, 4, -64, 0),
                 (100, 1, 4, 0, -1), (100, 1, 4, 0, TILE + 1)]:
        with pytest.raises(ValueError):
            di.label_term_plan(*args)
    with pytest.raises(ValueError, match="multiple of 64"):
        di.label_term_plan(100, 1, 4, 100, 0)
    # max_items x tiles <= (2^32 - 1) / 1024: a launch of 1024-thread workgroups holds fewer than 2^32 threads
    W = nat.LABEL_TERM_MAX_WORK_ITEMS
    assert W * 1024 < 1 << 32 <= (W + 1) * 1024
    assert di.label_term_plan((W - 1) * 64, 1, 8, 64, 0)[3] == W                      # the last valid grid, one tile
    with pytest.raises(ValueError, match="too many"):
        di.label_term_plan(W * 64, 1, 8, 64, 0)
    assert di.label_term_plan((W // 2 - 1) * 64, 1, 8, 64, 4)[::3] == (2, W // 2)     # ... and two tiles
    with pytest.raises(ValueError, match="too many"):
        di.label_term_plan((W // 2) * 64, 1, 8, 64, 4)
    with pytest.raises(ValueError, match="too many"):                                 # 15 626 items x 29 523 one-column tiles
        di.label_term_plan(1_000_000, 1, 29523, 64, 1)
    o32, o64 = C.c_int32(0), C.c_int64(0)
    assert nat.lib().vs_label_term_plan(100, 1, 4, 0, 0, None, C.byref(o32), C.byref(o64), C.byref(o64)) == nat.VS_EINVAL
    assert nat.lib().vs_label_term_plan(100, 1, 4, 0, 0, C.byref(o32), C.byref(o32), C.byref(o64), C.byref(o64)) == nat.VS_OK
    # the facade's own checks: both limits, the knobs, the labels
    lab = np.zeros(10, np.int32)
    assert di._label_term_args(lab, 65536, 10, 2048) == (65536, 0, 0) and di._label_term_args(lab, 4546, 10, 29523, 128, 7) == (4546, 128, 7)
    for bad in (dict(n_labels=65537), dict(n_labels=0), dict(n_labels=4547, n_cols=29523), dict(n_labels=65536, n_cols=2049),
                dict(rows_per_item=100), dict(rows_per_item=-64), dict(rows_per_item=True), dict(tile_cols=TILE + 1), dict(tile_cols=-1),
                dict(labels=np.zeros(9, np.int32)), dict(labels=np.zeros((2, 5), np.int32))):
        with pytest.raises(ValueError):
            di._label_term_args(**{"labels": lab, "n_labels": 3, "n_rows": 10, "n_cols": 8, **bad})
    for bad in (dict(labels=np.zeros(10, F32)), dict(n_labels=3.0)):
        with pytest.raises(TypeError):
            di._label_term_args(**{"labels": lab, "n_labels": 3, "n_rows": 10, "n_cols": 8, **bad})


def test_callers_slice_the_labels_where_k_times_v_is_more_than_one_call_holds():
    """k-means and cluster_terms accept any K <= 4096 at any V <= 65 535, as they did 64 clusters a call: beyond 2^27 cells they take a slice
    of the labels a call (label_term_slices), every slice inside both limits, the slices covering [0, K) once, in order"""
    cells, most = di.MAX_LABEL_TERM_CELLS, di.MAX_LABEL_TERM_LABELS
    for K, V, want in [(4096, 65535, [(0, 2048), (2048, 2048)]), (2048, 65535, [(0, 2048)]), (2049, 65535, [(0, 2048), (2048, 1)]),
                       (3355, 40000, [(0, 3355)]), (3356, 40000, [(0, 3355), (3355, 1)]), (4096, 29523, [(0, 4096)]), (64, 29523, [(0, 64)]),
                       (4096, 32768, [(0, 4096)]), (4096, 32769, [(0, 4095), (4095, 1)]), (1, 1, [(0, 1)]), (70, 200, [(0, 70)])]:
        got = di.label_term_slices(K, V)
        assert got == want, (K, V, got)
        assert all(1 <= n <= most and n * V <= cells for _, n in got)
        assert [l0 for l0, _ in got] == [sum(n for _, n in got[:i]) for i in range(len(got))] and sum(n for _, n in got) == K
        if len(got) > 1:
            assert K * V > cells and (got[0][1] + 1) * V > cells                       # sliced only where one call cannot hold it, slices as large as fit
    for V in (1, 7, 2048, 29523, 65535):                                              # every K of a k-means, every width: the facade's own check passes
        for K in (1, 64, 4095, nat.ASSIGN_MAX_K):
            for _, n in di.label_term_slices(K, V):
                di._label_term_args(np.zeros(3, np.int32), n, 3, V)
    assert di.label_term_slices(70000, 8) == [(0, 65536), (65536, 4464)]               # the label limit cuts as well
    # what a slice does to the labels: l - l0 falls outside [0, n) exactly for the labels outside the slice, -1 included
    lab = np.array([-1, 0, 2047, 2048, 4095], dtype=np.int32)
    for l0, n in di.label_term_slices(4096, 65535):
        sl = lab - l0
        assert ((sl >= 0) & (sl < n)).tolist() == ((lab >= l0) & (lab < l0 + n)).tolist()


# ---- argument errors of the C ABI, checked before the device is touched ----------------------------------------------------------------------
def test_index_calls_refuse_a_null_handle_without_a_device():
    out, total, other, lab = np.zeros((2, 4), np.int64), np.zeros(2, np.int64), np.zeros(1, np.int64), np.zeros(5, np.int32)
    ptr, rows = np.zeros(3, np.int64), np.zeros(5, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    for fn in ("vs_index_label_term_sums", "vs_index_label_term_counts"):
        assert getattr(nat.lib(), fn)(None, None, 0, p(lab), 2, 0, 0, p(out), 4, p(total), p(other), None) == nat.VS_EINVAL
        assert "NULL" in nat.last_error()
    assert nat.lib().vs_label_order(None, None, 0, p(lab), 2, p(ptr), p(rows), p(other), None) == nat.VS_EINVAL and "NULL" in nat.last_error()


# ---- the facades' host logic -----------------------------------------------------------------------------------------------------------------
def test_facade_validation_needs_no_device():
    from vsearch_amd.ir import SparseIndex
    from vsearch_amd.ir.retriever.index import Index
    from vsearch_amd.ir.retriever.retriever import Retriever
    idx = SparseIndex()
    with pytest.raises(KeyError, match="no facet field"):                              # an unknown field
        idx.term_sums_by_facet("nope")
    with pytest.raises(KeyError, match="no facet field"):
        idx.centroid_terms_by_facet("nope", topn=3)
    with pytest.raises(ValueError, match="ONE document set"):                          # a per-query filter
        idx.term_sums_by_facet("kind", filter=np.ones((2, 5), bool))
    with pytest.raises(ValueError, match="ONE document set"):                          # more than one query
        idx.centroids_by_facet("kind", torch.zeros(2, 6), np.zeros(2, F32))
    with pytest.raises(ValueError, match="go together"):
        idx.term_counts_by_facet("kind", q_embs=torch.zeros(1, 6))
    with pytest.raises(ValueError, match="topn"):
        idx.centroid_terms_by_facet("kind", topn=0)
    with pytest.raises(ValueError, match="method"):
        idx.significant_terms_by_facet("kind", method="tfidf")
    dense = Index()                                                                    # a dense index is not covered
    for call in (lambda: dense.term_sums_by_facet("kind"), lambda: dense.term_counts_by_facet("kind"), lambda: dense.centroids_by_facet("kind"),
                 lambda: dense.centroid_terms_by_facet("kind"), lambda: dense.significant_terms_by_facet("kind")):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError, match="method"):
        Retriever.facet_terms(None, "kind", method="tfidf")
    with pytest.raises(ValueError, match="go together"):
        Retriever.facet_terms(None, "kind", ["q"])
    with pytest.raises(ValueError, match="ONE document set"):
        Retriever.facet_terms(None, "kind", ["q", "r"], 0.5)
    assert di.KMEANS_UPDATE_BATCH == 64


# ---- the host-side checks under the host sanitizers ------------------------------------------------------------------------------------------
def test_host_checks_under_a_host_sanitizer(tmp_path):
    """label_term_check.h (the plan rule, the item bound, both limits of the calls and the chunk of the label order) in a stand-alone program
    built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "label_term_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "label_term_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "label_term_check: ok" in run.stdout, run.stdout + run.stderr
