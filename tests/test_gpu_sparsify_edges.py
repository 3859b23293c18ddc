"""The encoder tail -- mask_rows_fast_kernel<G, CSR> (G = 4 / 8 / 15 / 16, mask mode and fused CSR mode), mask_rows_kernel,
count_nz / scan_counts / fill_csr, elu1p and head_pool -- against the plain references of tests/_sparsify_ref.py (pinned on the CPU by
tests/test_sparsify_ref_cpu.py), at the widths where run_mask changes the instantiation, at the list / histogram bands of the candidate
phase, at the fused kernel's staging limits and around the CU count.  Run on MI355X.

Bars.  Every comparison is bit for bit (uint32 views; NaN on both sides matches: a NaN's payload is the multiplier's) except elu1p of
x <= 0 (rtol 2e-7, atol 1.2e-7 against float64 expm1: the bound of test_elu1p) and the normalised bag-of-words value (rtol 1e-6: the
bound of test_build_bow_mask).  Which path of the candidate phase a row takes is computed from the reference's keys (ref.paths_of) and
asserted per width, never read from the kernel.  Calls go through the C ABI with 4 rows each (device pointers into one uploaded batch)
unless a test is about the batch size; outputs are pre-filled with a sentinel, pad columns and guard words must keep it."""
import ctypes as C

import numpy as np
import pytest
import torch

import _sparsify_ref as ref
from vsearch_amd import _native as nat

pytestmark = pytest.mark.gpu

SENT_F = np.float32(-77.25)
SENT_I = -7777


@pytest.fixture(scope="module")
def cu():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t, elem_offset=0):
    """pointer to element `elem_offset` of a CUDA tensor or a numpy array (None: NULL)"""
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        return C.c_void_p(t.data_ptr() + elem_offset * t.element_size())
    return C.c_void_p(t.ctypes.data + elem_offset * t.itemsize)


def _u32(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32) if a.dtype in (np.float32, np.int32) else a


def _assert_bits(got, want, what, names=None):
    got, want = _u32(got), _u32(want)
    ok = ref.same_bits(got, want)
    if not ok.all():
        at = np.argwhere(~ok)
        rows = sorted({int(r[0]) for r in at})[:6]
        label = [names[r % len(names)] for r in rows] if names else rows
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} differ, rows {label}, first at {at[:4].tolist()}: "
                             f"got {[hex(v) for v in got[~ok][:4]]} want {[hex(v) for v in want[~ok][:4]]}")


def _topk_mask(xd, V, k, ld=None, chunk=4):
    """vs_topk_mask over the rows of xd (CUDA [R, ld]) `chunk` rows a call -> uint8 [R, V] (numpy)"""
    R = xd.shape[0]
    ld = ld or V
    mask = torch.full((R, V), 7, dtype=torch.uint8, device="cuda")
    for r0 in range(0, R, chunk):
        n = min(chunk, R - r0)
        nat.check(nat.lib().vs_topk_mask(_p(xd, r0 * ld), n, V, ld, k, _p(mask, r0 * V), 0, None))
    return mask.cpu().numpy()


def _embed_mask(xd, idsd, V, shift, topk, lexical, bow=0, ld=None, chunk=4):
    """vs_embed_mask in place on a clone of xd, `chunk` rows a call -> the clone"""
    R = xd.shape[0]
    ld = ld or V
    L = idsd.shape[1] if idsd is not None else 0
    e = xd.clone()
    torch.cuda.synchronize()
    for r0 in range(0, R, chunk):
        n = min(chunk, R - r0)
        nat.check(nat.lib().vs_embed_mask(_p(e, r0 * ld), ld, _p(idsd, r0 * L) if idsd is not None else None, n, L, V + shift, shift, topk,
                                          int(lexical), bow, 0, None))
    torch.cuda.synchronize()
    return e


def _lex_combos(t):
    """the two (L, shift) pairs run with the t-th top-k value: over five values every L meets every shift"""
    return [(ref.LEX_L[(t + 2 * s) % len(ref.LEX_L)], shift) for s, shift in enumerate(ref.SHIFTS)]


# ---- a. the mask stage at every width ------------------------------------------------------------------------------------------------
def _mask_case(V, topk, t, x, names, tk):
    xd = _dev(x)
    got = _topk_mask(xd, V, topk)
    bad = got != tk.astype(np.uint8)
    assert not bad.any(), f"vs_topk_mask V={V} k={topk}: rows {[names[r] for r in sorted(set(np.argwhere(bad)[:, 0].tolist()))[:6]]} differ"
    _assert_bits(_embed_mask(xd, None, V, 0, topk, False), ref.masked_bits(x, tk), f"vs_embed_mask V={V} topk={topk}", names)
    for L, shift in _lex_combos(t):
        ids = ref.token_batch(x, V + shift, shift, L, seed=t)
        keep = ref.keep_mask_ref(x, ids, V + shift, shift, topk, True, topk_mask=tk)
        _assert_bits(_embed_mask(xd, _dev(ids), V, shift, topk, True), ref.masked_bits(x, keep),
                     f"vs_embed_mask V={V} topk={topk} lexical L={L} shift={shift}", names)
    _assert_bits(xd, x, "the input batch")


@pytest.mark.parametrize("V", ref.MASK_WIDTHS + (ref.slow_max_v(),))
def test_mask_stage_at_the_switch_widths(V):
    """vs_topk_mask and vs_embed_mask (with and without lexical, L in {1, 511, 512, 513, 1100}, shift in {0, 999}) over every row family,
    topk in {1, 2, V / 2, V - 1, V}: V <= 32768 runs mask_rows_fast_kernel<4 | 8 | 15 | 16>, beyond it mask_rows_kernel up to the
    widest row its LDS image admits"""
    seen = set()
    for t, topk in enumerate(ref.mask_topks(V)):
        x, names = ref.mask_rows(V, topk)
        tk = ref.topk_mask_ref(x, topk)
        seen |= set(ref.paths_of(x, topk))
        _mask_case(V, topk, t, x, names, tk)
    assert {p for p, _ in seen} == set(ref.PATHS), f"V={V}: paths {seen}"
    assert {p for p, zero in seen if zero} >= {"take_all", "list_128"}, "the P == 0 rows did not reach both of their paths"


def test_mask_stage_refuses_the_first_width_beyond_the_lds_image():
    V = ref.slow_max_v() + 1
    assert V == 36557
    x = _dev(np.ones((1, V), dtype=np.float32))
    mask = torch.zeros((1, V), dtype=torch.uint8, device="cuda")
    with pytest.raises(NotImplementedError):
        nat.check(nat.lib().vs_topk_mask(_p(x), 1, V, V, 5, _p(mask), 0, None))
    with pytest.raises(NotImplementedError):
        nat.check(nat.lib().vs_embed_mask(_p(x), V, None, 1, 0, V, 0, 5, 0, 0, 0, None))
    assert (x == 1).all() and (mask == 0).all()


@pytest.mark.parametrize("V", ref.PREFETCH_WIDTHS)
def test_mask_stage_more_rows_than_workgroups(V, cu):
    """B = CUs + 3 in ONE call: three workgroups take a second row, whose loads and tokens they issued during the first"""
    B = cu + 3
    for t, topk in ((2, V // 2), (3, V - 1)):
        x4, names = ref.mask_rows(V, topk)
        pick = (np.arange(B) * 5 + t) % x4.shape[0]           # (neighbouring rows of a workgroup come from different families)
        x, tk = x4[pick], ref.topk_mask_ref(x4, topk)[pick]
        names = [names[i] for i in pick]
        xd = _dev(x)
        got = _topk_mask(xd, V, topk, chunk=B)
        assert (got == tk.astype(np.uint8)).all(), f"vs_topk_mask V={V} k={topk} B={B}"
        L, shift = ((513, 999), (1100, 0))[t - 2]             # (1100: the second row's tokens beyond the 512 prefetched ones are read in place)
        ids = ref.token_batch(x, V + shift, shift, L, seed=t)
        keep = ref.keep_mask_ref(x, ids, V + shift, shift, topk, True, topk_mask=tk)
        _assert_bits(_embed_mask(xd, _dev(ids), V, shift, topk, True, chunk=B), ref.masked_bits(x, keep), f"vs_embed_mask V={V} topk={topk} B={B} L={L}", names)
        if t == 2:
            _assert_bits(_embed_mask(xd, None, V, 0, topk, False, chunk=B), ref.masked_bits(x, tk), f"vs_embed_mask V={V} topk={topk} B={B}", names)


def test_mask_stage_topk_zero_all_and_bag_of_words():
    """topk = 0 (lexical columns only), topk < 0 (everything), bow, vs_bow_mask with and without norm: mask_rows_kernel at a narrow row"""
    V, shift, L = 8193, 999, 513
    x, names = ref.mask_rows(V, 2)
    xd = _dev(x)
    ids = ref.token_batch(x, V + shift, shift, L, seed=9)
    idsd = _dev(ids)
    for topk, lexical in ((0, True), (0, False), (-1, True), (-1, False)):
        want = ref.embed_mask_ref(x, ids, V + shift, shift, topk, lexical)
        _assert_bits(_embed_mask(xd, idsd, V, shift, topk, lexical), want, f"vs_embed_mask topk={topk} lexical={lexical}", names)
    assert (_topk_mask(xd, V, 0) == 0).all()
    _assert_bits(_embed_mask(xd, idsd, V, shift, 5, False, bow=1), ref.embed_mask_ref(x, ids, V + shift, shift, 5, False, bow=True), "vs_embed_mask bow", names)
    R = x.shape[0]
    for norm in (0, 1):
        out = torch.full((R, V), float(SENT_F), dtype=torch.float32, device="cuda")
        nat.check(nat.lib().vs_bow_mask(_p(idsd), R, L, V + shift, shift, norm, _p(out), 0, None))
        want = ref.bow_mask_ref(ids, V + shift, shift, bool(norm))
        if norm:
            np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-6)
            assert ((out.cpu().numpy() != 0) == (want != 0)).all()
        else:
            _assert_bits(out, want.astype(np.float32), "vs_bow_mask")


def test_signed_zeros_and_non_finite_input_follow_the_stated_contract(cu):
    """include/vsearch_hip.h: selection compares order keys -- +0.0 ranks above -0.0 -- on both mask kernels; the fused call drops an
    unselected +-inf / NaN where vs_embed_mask + vs_dense_to_csr store the NaN of x * 0"""
    row = np.float32([[-0.0, 0.0, -1.0]])
    assert ref.topk_mask_ref(row, 1).tolist() == [[False, True, False]]
    assert _topk_mask(_dev(row), 3, 1).tolist() == [[0, 1, 0]]                                 # mask_rows_fast_kernel<4>
    wide = np.full((1, ref.MR_COLS + 1), -1.0, dtype=np.float32)
    wide[0, :2] = [-0.0, 0.0]
    got = _topk_mask(_dev(wide), wide.shape[1], 1)                                             # mask_rows_kernel
    assert got[0, :3].tolist() == [0, 1, 0] and got.sum() == 1
    zz = np.float32([[-0.0, 0.0, -0.0, 0.0, -1.0]])
    assert _topk_mask(_dev(zz), 5, 3).tolist() == ref.topk_mask_ref(zz, 3).astype(np.uint8).tolist() == [[1, 1, 0, 1, 0]]
    y = np.float32([[3.0, -np.inf, 2.0, 1.0, -np.inf], [1.0, 2.0, np.inf, 0.5, 0.25]])
    keep = ref.topk_mask_ref(y, 2)
    fused, two = ref.masked_csr_ref(y, keep), ref.two_call_csr_ref(y, keep)
    assert fused.cols.tolist() == [0, 2, 1, 2] and two.cols.tolist() == [0, 1, 2, 4, 1, 2]
    yd = _dev(y)
    _check_fused(yd, None, 5, 0, 2, False, fused, "fused CSR of the contract's rows")
    masked = _embed_mask(yd, None, 5, 0, 2, False, chunk=2)
    _assert_bits(masked, ref.masked_bits(y, keep), "vs_embed_mask of the contract's rows")
    masked = masked.cpu().numpy()
    stored = ref.dense_to_csr_ref(masked)                      # (the NaNs' payloads are the GPU multiplier's: the values come from `masked`)
    assert stored.cols.tolist() == two.cols.tolist() and np.isnan(stored.vals[[1, 3]]).all()
    _check_dense_to_csr(masked, stored, device=True)


# ---- b. lexical tokens out of range, leading dimensions, staging ----------------------------------------------------------------------
@pytest.mark.parametrize("pos,bad", [(3, -1), (700, "vocab")])
def test_a_token_out_of_range_raises_on_every_kernel(pos, bad):
    V, shift, L, B = 8193, 999, 1100, 4
    vocab = V + shift
    x = np.stack([ref.distinct_values(np.random.default_rng(i), V) for i in range(B)])
    ids = ref.token_batch(x, vocab, shift, L, seed=3)
    ids[2, pos] = vocab if bad == "vocab" else bad
    xd, idsd = _dev(x), _dev(ids)
    e = xd.clone()
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="token id out of range"):                 # mask_rows_fast_kernel<8>
        nat.check(nat.lib().vs_embed_mask(_p(e), V, _p(idsd), B, L, vocab, shift, 50, 1, 0, 0, None))
    with pytest.raises(ValueError, match="token id out of range"):                 # mask_rows_kernel (topk = 0)
        nat.check(nat.lib().vs_embed_mask(_p(e), V, _p(idsd), B, L, vocab, shift, 0, 1, 0, 0, None))
    out = torch.zeros((B, V), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="token id out of range"):                 # mask_rows_kernel (bow)
        nat.check(nat.lib().vs_bow_mask(_p(idsd), B, L, vocab, shift, 0, _p(out), 0, None))
    rowptr = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
    cols = torch.zeros(B * (50 + L), dtype=torch.int32, device="cuda")
    vals = torch.zeros(B * (50 + L), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="token id out of range"):                 # mask_rows_fast_kernel<8, 1>
        nat.check(nat.lib().vs_embed_mask_to_csr(_p(xd), V, _p(idsd), B, L, vocab, shift, 50, 1, _p(rowptr), _p(cols), _p(vals), cols.numel(), 0, None))
    # ... and the same batch without the bad token passes on all of them
    ids[2, pos] = vocab - 1
    keep = ref.keep_mask_ref(x, ids, vocab, shift, 50, True)
    _assert_bits(_embed_mask(xd, _dev(ids), V, shift, 50, True), ref.masked_bits(x, keep), "vs_embed_mask after the repair")


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("V", [8193, ref.MR_COLS, ref.MR_COLS + 1], ids=["fast-G8", "fast-G16", "slow"])
def test_mask_stage_leading_dimension_and_staging(V, on_device):
    """ld = V + 5 for vs_embed_mask and vs_topk_mask, host and device pointers: the pad columns are never read (they hold huge values
    that would win every top-k) nor written"""
    shift, L, pad = 999, 513, 5
    topk = V // 2
    x4, names = ref.mask_rows(V, topk)
    x, names = np.ascontiguousarray(x4[::6]), names[::6]        # eight rows of different families
    B, ld = x.shape[0], V + pad
    tk = ref.topk_mask_ref(x, topk)
    ids = ref.token_batch(x, V + shift, shift, L, seed=2)
    keep = ref.keep_mask_ref(x, ids, V + shift, shift, topk, True, topk_mask=tk)
    host = np.full((B, ld), 3e38, dtype=np.float32)
    host[:, :V] = x
    src = _dev(host) if on_device else host.copy()
    ids_in = _dev(ids) if on_device else ids
    mask = torch.full((B, V), 7, dtype=torch.uint8, device="cuda") if on_device else np.full((B, V), 7, dtype=np.uint8)
    nat.check(nat.lib().vs_topk_mask(_p(src), B, V, ld, topk, _p(mask), 0, None))
    got = mask.cpu().numpy() if on_device else mask
    assert (got == tk.astype(np.uint8)).all(), "vs_topk_mask, ld > V"
    nat.check(nat.lib().vs_embed_mask(_p(src), ld, _p(ids_in), B, L, V + shift, shift, topk, 1, 0, 0, None))
    out = src.cpu().numpy() if on_device else src
    _assert_bits(np.ascontiguousarray(out[:, :V]), ref.masked_bits(x, keep), "vs_embed_mask, ld > V", names)
    assert (out[:, V:] == np.float32(3e38)).all(), "vs_embed_mask wrote into the pad columns"


# ---- c. the fused mask -> CSR call ---------------------------------------------------------------------------------------------------
GUARD = 8


def _fused_call(xd, idsd, r0, n, V, shift, topk, lexical, rowptr, rp_at, cols, vals, at, cap, ld=None):
    ld = ld or V
    L = idsd.shape[1] if idsd is not None else 0
    return nat.lib().vs_embed_mask_to_csr(_p(xd, r0 * ld), ld, _p(idsd, r0 * L) if lexical else None, n, L, V + shift, shift, topk, int(lexical),
                                          _p(rowptr, rp_at), _p(cols, at), _p(vals, at), cap, 0, None)


def _check_fused(xd, idsd, V, shift, topk, lexical, want, what, chunk=4, ld=None, names=None):
    """vs_embed_mask_to_csr over the rows of xd, `chunk` rows a call with cap = the chunk's exact nnz, LAST chunk first: every chunk's
    entries lie right behind the one before it, so a store past cap lands in entries already checked in (or in the guard behind all)"""
    R = xd.shape[0]
    nnz = int(want.rowptr[-1])
    n_chunks = (R + chunk - 1) // chunk
    rowptr = torch.full((n_chunks * (chunk + 1) + GUARD,), SENT_I, dtype=torch.int64, device="cuda")
    cols = torch.full((nnz + GUARD,), SENT_I, dtype=torch.int32, device="cuda")
    vals = torch.full((nnz + GUARD,), float(SENT_F), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for c in reversed(range(n_chunks)):
        r0 = c * chunk
        n = min(chunk, R - r0)
        at, end = int(want.rowptr[r0]), int(want.rowptr[r0 + n])
        rc = _fused_call(xd, idsd, r0, n, V, shift, topk, lexical, rowptr, c * (chunk + 1), cols, vals, at, end - at, ld)
        assert rc == 0, f"{what}: rows {r0}..{r0 + n} with cap = their reference nnz {end - at}: {nat.last_error()}"
    torch.cuda.synchronize()
    rp = rowptr.cpu().numpy()
    assert (rp[n_chunks * (chunk + 1):] == SENT_I).all(), f"{what}: the words behind rowptr were written"
    for c in range(n_chunks):
        r0 = c * chunk
        n = min(chunk, R - r0)
        got = rp[c * (chunk + 1):c * (chunk + 1) + n + 1]
        exp = want.rowptr[r0:r0 + n + 1] - want.rowptr[r0]
        assert (got == exp).all(), f"{what}: rowptr of rows {r0}..{r0 + n} ({names[r0:r0 + n] if names else ''}): got {got.tolist()} want {exp.tolist()}"
    gc, gv = cols.cpu().numpy(), vals.cpu().numpy()
    assert (gc[nnz:] == SENT_I).all() and (gv[nnz:] == SENT_F).all(), f"{what}: the guard behind cap was written"
    bad = gc[:nnz] != want.cols
    assert not bad.any(), f"{what}: {int(bad.sum())} of {nnz} columns differ, first at entry {int(np.argmax(bad))}"
    ok = ref.same_bits(gv[:nnz], want.vals)
    assert ok.all(), f"{what}: {int((~ok).sum())} of {nnz} values differ, first at entry {int(np.argmax(~ok))}"


@pytest.mark.parametrize("V", ref.MASK_WIDTHS[:-1])
def test_fused_csr_at_the_switch_widths(V):
    """vs_embed_mask_to_csr against masked_csr_ref over every row family: topk in {1, 2, V / 2, V - 1, V} while a row's kept elements fit
    the stage (V <= 8192), else up to topk + L = 8192 exactly; with and without lexical.  mask_rows_fast_kernel<4 | 8 | 15 | 16, 1>."""
    seen = set()
    for t in range(5):
        topk = ref.csr_topks(V)[t]
        x, names = ref.mask_rows(V, topk)
        xd = _dev(x)
        tk = ref.topk_mask_ref(x, topk)
        seen |= set(ref.paths_of(x, topk))
        _check_fused(xd, None, V, 0, topk, False, ref.masked_csr_ref(x, tk), f"fused CSR V={V} topk={topk}", names=names)
        for L, shift in _lex_combos(t):
            tl = ref.csr_topks(V, L)[t]
            if tl != topk:
                x, names = ref.mask_rows(V, tl)
                xd = _dev(x)
                tk = ref.topk_mask_ref(x, tl)
            ids = ref.token_batch(x, V + shift, shift, L, seed=t)
            keep = ref.keep_mask_ref(x, ids, V + shift, shift, tl, True, topk_mask=tk)
            assert min(V, tl + L) <= ref.MR_STAGE
            _check_fused(xd, _dev(ids), V, shift, tl, True, ref.masked_csr_ref(x, keep), f"fused CSR V={V} topk={tl} lexical L={L} shift={shift}", names=names)
        _assert_bits(xd, x, "the input batch")
    assert {p for p, _ in seen} == set(ref.PATHS), f"V={V}: paths {seen}"
    p0 = {p for p, zero in seen if zero}
    assert "hist_all_eq" in p0 and (V > ref.MR_STAGE or p0 >= {"take_all", "list_128"}), f"V={V}: the P == 0 rows of the fused call reach only {p0}"


@pytest.mark.parametrize("V", ref.PREFETCH_WIDTHS)
def test_fused_csr_more_rows_than_workgroups(V, cu):
    B = cu + 3
    t, topk = 2, ref.csr_topks(V)[2]
    x4, names = ref.mask_rows(V, topk)
    pick = (np.arange(B) * 5 + t) % x4.shape[0]
    x, tk = x4[pick], ref.topk_mask_ref(x4, topk)[pick]
    xd = _dev(x)
    _check_fused(xd, None, V, 0, topk, False, ref.masked_csr_ref(x, tk), f"fused CSR V={V} topk={topk} B={B}", chunk=B)
    L, shift = 513, 999
    ids = ref.token_batch(x, V + shift, shift, L, seed=t)
    keep = ref.keep_mask_ref(x, ids, V + shift, shift, topk, True, topk_mask=tk)
    _check_fused(xd, _dev(ids), V, shift, topk, True, ref.masked_csr_ref(x, keep), f"fused CSR V={V} topk={topk} B={B} L={L}", chunk=B)


def test_fused_csr_row_split_around_the_cu_count(cu):
    """V = 8193, B in {1, 2, CUs - 1, CUs, CUs + 1, 2 CUs + 3} in one call each: the per / rem split of the rows over the workgroups and
    the ticketed prefix of their totals; an all-zero row and a row whose kept elements are all zeros in the middle of a run"""
    V, shift, L, topk = 8193, 999, 5, 37
    x4, _ = ref.mask_rows(V, topk)
    tk4 = ref.topk_mask_ref(x4, topk)
    for B in (1, 2, cu - 1, cu, cu + 1, 2 * cu + 3):
        pick = (np.arange(B) * 7) % x4.shape[0]
        x, tk = x4[pick].copy(), tk4[pick].copy()
        ids = ref.token_batch(x, V + shift, shift, L, seed=B)
        if B >= 4:
            for r in (B // 2, B - 2):
                x[r] = 0.0
                x[r + 1] = np.where(np.arange(V) < 60, np.float32(0.0), -np.float32(1.5))       # the top 37 are zeros: nothing stored
                x[r + 1, 1:60:2] = -0.0
                ids[r:r + 2] = shift + 3                                                      # (their lexical column is a zero too)
            tk = ref.topk_mask_ref(x, topk)
        keep = ref.keep_mask_ref(x, ids, V + shift, shift, topk, True, topk_mask=tk)
        want = ref.masked_csr_ref(x, keep)
        if B >= 4:
            assert want.rowptr[B // 2] == want.rowptr[B // 2 + 2] and want.rowptr[B // 2] > 0
        _check_fused(_dev(x), _dev(ids), V, shift, topk, True, want, f"fused CSR V={V} B={B}", chunk=B)


def test_fused_csr_limits(cu):
    """topk + L = 8192 runs and 8193 is refused; slot_cap = V where V < topk + L (V = 8191, topk = 8191; topk = V = 8192);
    cap = nnz - 1 is VS_ERANGE; ld = V + 5"""
    V, shift = 8193, 999
    x = np.stack([ref.distinct_values(np.random.default_rng(40 + i), V) for i in range(4)])
    xd = _dev(x)
    for L in (513, 1100):
        ids = ref.token_batch(x, V + shift, shift, L, seed=L)
        idsd = _dev(ids)
        for topk, runs in ((ref.MR_STAGE - L, True), (ref.MR_STAGE - L + 1, False)):
            if runs:
                keep = ref.keep_mask_ref(x, ids, V + shift, shift, topk, True)
                _check_fused(xd, idsd, V, shift, topk, True, ref.masked_csr_ref(x, keep), f"fused CSR topk + L = {topk + L}")
            else:
                rowptr = torch.zeros(5, dtype=torch.int64, device="cuda")
                cols = torch.zeros(4 * V, dtype=torch.int32, device="cuda")
                vals = torch.zeros(4 * V, dtype=torch.float32, device="cuda")
                with pytest.raises(NotImplementedError):
                    nat.check(_fused_call(xd, idsd, 0, 4, V, shift, topk, True, rowptr, 0, cols, vals, 0, 4 * V))
    rowptr = torch.zeros(5, dtype=torch.int64, device="cuda")
    cols = torch.zeros(4 * V, dtype=torch.int32, device="cuda")
    vals = torch.zeros(4 * V, dtype=torch.float32, device="cuda")
    with pytest.raises(NotImplementedError):                                        # no lexical: topk alone beyond the stage
        nat.check(_fused_call(xd, None, 0, 4, V, 0, ref.MR_STAGE + 1, False, rowptr, 0, cols, vals, 0, 4 * V))
    with pytest.raises(RuntimeError):                                               # topk > V
        nat.check(_fused_call(xd, None, 0, 4, V, 0, V + 1, False, rowptr, 0, cols, vals, 0, 4 * V))
    for Vs in (8191, 8192):                                                         # V the smaller: every element kept, + 1100 tokens
        xs = np.ascontiguousarray(x[:, :Vs])
        xs[1, ::5] = 0.0
        ids = ref.token_batch(xs, Vs + shift, shift, 1100, seed=1)
        keep = ref.keep_mask_ref(xs, ids, Vs + shift, shift, Vs, True)
        assert keep.all()
        _check_fused(_dev(xs), _dev(ids), Vs, shift, Vs, True, ref.masked_csr_ref(xs, keep), f"fused CSR V = topk = {Vs}")
    # cap one short of the batch's non-zeros
    ids = ref.token_batch(x, V + shift, shift, 40, seed=4)
    idsd = _dev(ids)
    keep = ref.keep_mask_ref(x, ids, V + shift, shift, 300, True)
    want = ref.masked_csr_ref(x, keep)
    nnz = int(want.rowptr[-1])
    cols = torch.full((nnz + GUARD,), SENT_I, dtype=torch.int32, device="cuda")
    vals = torch.full((nnz + GUARD,), float(SENT_F), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="the batch has more non-zeros"):
        nat.check(_fused_call(xd, idsd, 0, 4, V, shift, 300, True, rowptr, 0, cols, vals, 0, nnz - 1))
    assert (cols[nnz - 1:] == SENT_I).all() and (vals[nnz - 1:] == float(SENT_F)).all(), "a refused call wrote behind cap"
    # ld = V + 5, pads that would win every top-k
    host = np.full((4, V + 5), 3e38, dtype=np.float32)
    host[:, :V] = x
    _check_fused(_dev(host), idsd, V, shift, 300, True, want, "fused CSR ld = V + 5", ld=V + 5)
    xw = np.stack([ref.distinct_values(np.random.default_rng(50 + i), ref.MR_COLS) for i in range(4)])
    host = np.full((4, ref.MR_COLS + 5), 3e38, dtype=np.float32)
    host[:, :ref.MR_COLS] = xw
    _check_fused(_dev(host), None, ref.MR_COLS, 0, 768, False, ref.masked_csr_ref(xw, ref.topk_mask_ref(xw, 768)), "fused CSR V = 32768, ld = V + 5",
                 ld=ref.MR_COLS + 5)


# ---- d. dense -> CSR -----------------------------------------------------------------------------------------------------------------
def _check_dense_to_csr(x, want, device, pad=0):
    """the two-call protocol of vs_dense_to_csr with ld = V + pad (pads hold non-zeros), cap = nnz and a guard behind cols / vals"""
    B, V = x.shape
    ld = V + pad
    host = np.full((B, ld), 5.0, dtype=np.float32)
    host[:, :V] = x
    nnz = int(want.rowptr[-1])
    if device:
        src = _dev(host)
        rowptr = torch.full((B + 1 + GUARD,), SENT_I, dtype=torch.int64, device="cuda")
        cols = torch.full((nnz + GUARD,), SENT_I, dtype=torch.int32, device="cuda")
        vals = torch.full((nnz + GUARD,), float(SENT_F), dtype=torch.float32, device="cuda")
    else:
        src = host
        rowptr = np.full(B + 1 + GUARD, SENT_I, dtype=np.int64)
        cols = np.full(nnz + GUARD, SENT_I, dtype=np.int32)
        vals = np.full(nnz + GUARD, SENT_F, dtype=np.float32)
    torch.cuda.synchronize()
    nat.check(nat.lib().vs_dense_to_csr(_p(src), B, V, ld, _p(rowptr), None, None, 0, 0, None))
    torch.cuda.synchronize()
    rp = rowptr.cpu().numpy() if device else rowptr
    assert (rp[:B + 1] == want.rowptr).all(), f"rowptr B={B} V={V}: first difference at row {int(np.argmax(rp[:B + 1] != want.rowptr))}"
    assert (rp[B + 1:] == SENT_I).all(), "the words behind rowptr were written"
    nat.check(nat.lib().vs_dense_to_csr(_p(src), B, V, ld, _p(rowptr), _p(cols), _p(vals), nnz, 0, None))
    torch.cuda.synchronize()
    gc, gv = (cols.cpu().numpy(), vals.cpu().numpy()) if device else (cols, vals)
    assert (gc[nnz:] == SENT_I).all() and (gv[nnz:] == SENT_F).all(), "the guard behind cap was written"
    assert (gc[:nnz] == want.cols).all(), f"cols B={B} V={V}"
    assert (gv[:nnz].view(np.uint32) == want.vals.view(np.uint32)).all(), f"vals B={B} V={V} (stored as they are: NaN payloads included)"
    got_src = src.cpu().numpy() if device else src
    assert (got_src.view(np.uint32) == host.view(np.uint32)).all(), "the input was modified"


@pytest.mark.parametrize("B,V", [(3, V) for V in ref.DENSE_V] + [(B, 70) for B in ref.DENSE_B])
def test_dense_to_csr_edges(B, V):
    """count_nz's 8-deep unroll (V around 8192), fill_csr's second chunk of 32768 columns, scan_counts with more than a row a thread
    (B > 1024), the grid-stride loops (B > 2048); NaN, +-inf, subnormals are stored, +-0.0 are not"""
    x = ref.dense_rows(B, V, seed=1)
    want = ref.dense_to_csr_ref(x)
    _check_dense_to_csr(x, want, device=True)
    _check_dense_to_csr(x, want, device=True, pad=3)
    _check_dense_to_csr(x, want, device=False, pad=3 if V % 2 else 0)


# ---- e. elu1p and head_pool ------------------------------------------------------------------------------------------------------------
def _check_elu(got, x, what):
    got = np.asarray(got)
    e32, exact = ref.elu1p_exact(x)
    ok = ref.same_bits(np.ascontiguousarray(got[exact]), np.ascontiguousarray(e32[exact]))
    assert ok.all(), f"{what}: {int((~ok).sum())} results of x > 0 / +-0 / +-inf / NaN are not the exact ones, first x = {x[exact][~ok][:4]}"
    np.testing.assert_allclose(got[~exact], ref.elu1p_ref(x)[~exact], rtol=2e-7, atol=1.2e-7, err_msg=what)


def test_elu1p_grid_stride_and_exact_cases():
    x = ref.elu_input(ref.ELU_N, seed=1)
    assert x.size > 8192 * 256
    out = torch.full((x.size + GUARD,), float(SENT_F), dtype=torch.float32, device="cuda")
    xd = _dev(x)
    nat.check(nat.lib().vs_elu1p(_p(xd), x.size, _p(out), 0, None))
    got = out.cpu().numpy()
    assert (got[x.size:] == SENT_F).all()
    _check_elu(got[:x.size], x, "vs_elu1p, device pointers")
    small = ref.elu_input(1000, seed=2)
    host_out = np.full(1000 + GUARD, SENT_F, dtype=np.float32)
    nat.check(nat.lib().vs_elu1p(_p(small), 1000, _p(host_out), 0, None))
    assert (host_out[1000:] == SENT_F).all()
    _check_elu(host_out[:1000], small, "vs_elu1p, host pointers")


@pytest.mark.parametrize("B,L,V", [(3, 2, 699051), (2, 1, 1000), (5, 7, 333)], ids=["grid-stride", "one-position", "small"])
def test_head_pool_grid_stride_and_exact_cases(B, L, V):
    if B * V > 1000000:
        assert 8192 * 256 < B * V < 8192 * 256 + 256
    lg = ref.pool_logits(B, L, V, seed=3)
    m, _ = ref.head_pool_ref(lg)
    out = torch.full((B * V + GUARD,), float(SENT_F), dtype=torch.float32, device="cuda")
    lgd = _dev(lg)
    nat.check(nat.lib().vs_head_pool(_p(lgd), B, L, V, _p(out), 0, None))
    got = out.cpu().numpy()
    assert (got[B * V:] == SENT_F).all()
    _check_elu(got[:B * V].reshape(B, V), m, f"vs_head_pool B={B} L={L} V={V}")
    assert (got[:B * V].reshape(B, V)[:, 0] == 0).all() and (got[:B * V].reshape(B, V)[:, 1] == 1).all()
    if B * V < 10000:
        host_out = np.full((B, V), SENT_F, dtype=np.float32)
        nat.check(nat.lib().vs_head_pool(_p(lg), B, L, V, _p(host_out), 0, None))
        _check_elu(host_out, m, f"vs_head_pool B={B} L={L} V={V}, host pointers")
