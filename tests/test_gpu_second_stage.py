"""The kernels behind the search walks -- vs_rerank_scores, vs_rerank_topk, vs_merge_topk, vs_head_pool_mean_topk, vs_head_pool --
through their C entry points, against the plain numpy references of tests/_second_stage_ref.py (pinned on the CPU by
tests/test_second_stage_ref_cpu.py) at the widths, leading dimensions, k and batch sizes where their loops end.  Run on MI355X.

Bars.  Order results (ids, score bits): exact.  Scores on dyadic inputs, where every product and sum is exact: bit-equal.  Scores on
general inputs: at most 1 float32 ulp from the float64 sum of the float32 products, and |got - hi| <= 2^-24 abs_sum + ulp32(hi) (one
rounding per product plus the final cast) -- derived, not measured.  Mixed-sign pooling keeps the tolerance the operation already
has in test_gpu_facade.py (rtol 1e-5, atol 1e-6)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _second_stage_ref as ref
from vsearch_amd import _native as nat
from vsearch_amd.device_index import current_stream

pytestmark = pytest.mark.gpu

F32, F16 = nat.VS_F32, nat.VS_F16
NP_OF = {F32: np.float32, F16: np.float16}
DTYPES = pytest.mark.parametrize("p_dtype", [F32, F16], ids=["f32", "f16"])
SENTINEL = np.float32(-7.5e33)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    bad = ref.bits32(got) != ref.bits32(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} scores differ, first at {np.argwhere(bad)[:4].tolist()}: " \
                          f"got {got[bad][:4]} want {want[bad][:4]}"


def _same_ids(got, want, what=""):
    bad = np.asarray(got) != np.asarray(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} ids differ, first at {np.argwhere(bad)[:4].tolist()}: " \
                          f"got {np.asarray(got)[bad][:4]} want {np.asarray(want)[bad][:4]}"


# ---- vs_rerank_scores ------------------------------------------------------------------------------------------------------------
def _strided(a, pad, misalign):
    """Device copy of the rows of `a` at leading dimension n_cols + pad; the padding holds NaN (a kernel that reads it shows).
    `misalign`: the rows start one element into the allocation (flatten()[1:]: a 4-byte aligned base for fp32)."""
    n, v = a.shape
    host = np.full((n, v + pad), np.nan, dtype=a.dtype)
    host[:, :v] = a
    flat = np.concatenate([np.full(1, np.nan, dtype=a.dtype), host.reshape(-1)]) if misalign else host.reshape(-1)
    t = _dev(flat)
    return (t.flatten()[1:] if misalign else t), v + pad


def _rerank_scores(p, q, k, p_dtype, ldp_pad=0, ldq_pad=0, misalign=False):
    """All B * k rows in one call -> float32 [B * k] (host)."""
    B, V = q.shape
    assert p.shape == (B * k, V)
    pt, ldp = _strided(p.astype(NP_OF[p_dtype]), ldp_pad, misalign)
    qt, ldq = _strided(q, ldq_pad, misalign)
    out = torch.full((B * k,), float(SENTINEL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    nat.check(nat.lib().vs_rerank_scores(_ptr(pt), p_dtype, ldp, B * k, 0, _ptr(qt), ldq, B, k, V, _ptr(out), 0, None))
    return out.cpu().numpy()


WIDTHS = ref.RERANK_WIDTHS                                # every width at which a lane leaves one of the kernel's loops


@DTYPES
@pytest.mark.parametrize("V", WIDTHS)
def test_rerank_scores_dyadic_every_width_and_stride(V, p_dtype):
    """dense signed dyadic rows: every column counts and every sum is exact -> bit-equal, at every leading dimension and alignment"""
    p, q, k = ref.rerank_dyadic_case(V, NP_OF[p_dtype])   # (test_dyadic_inputs_sum_exactly proves these very arrays sum exactly)
    want = ref.rerank_scores_ref(p, q, k).exact32
    for ldp_pad, ldq_pad, misalign in ((0, 0, False), (1, 0, False), (0, 1, False), (3, 5, False), (5, 3, False), (0, 0, True), (1, 3, True)):
        got = _rerank_scores(p, q, k, p_dtype, ldp_pad, ldq_pad, misalign)
        _same_bits(got, want, f"V={V} ldp=V+{ldp_pad} ldq=V+{ldq_pad} misalign={misalign}")


@DTYPES
@pytest.mark.parametrize("V", WIDTHS)
def test_rerank_scores_general_values(V, p_dtype):
    """signed randn, ~97 % zeros in p (dense at the narrow widths): <= 1 ulp from exact32 and inside the derived bound around hi"""
    rng = np.random.default_rng(2000 + V)
    B, k = 4, 16
    p = ref.sparse_randn(rng, (B * k, V), 0.97 if V > 100 else 0.3, NP_OF[p_dtype])
    q = ref.sparse_randn(rng, (B, V), 0.2)
    r = ref.rerank_scores_ref(p, q, k)
    got = _rerank_scores(p, q, k, p_dtype, ldp_pad=3, ldq_pad=1)
    d = ref.ulp_distance32(got, r.exact32)
    err = np.abs(got.astype(np.float64) - r.hi)
    bound = 2.0 ** -24 * r.abs_sum + ref.ulp32(r.hi)
    print(f"V={V} dtype={p_dtype}: max ulp distance {d.max()}, max err/bound {np.max(err / bound):.3f}")
    assert d.max() <= 1, f"{int((d > 1).sum())} scores more than 1 ulp from the float64 sum of float32 products (max {d.max()})"
    assert (err <= bound).all(), f"max err/bound {np.max(err / bound):.3f}"


@DTYPES
def test_rerank_scores_streaming_chunks(p_dtype):
    """chunks of 1, 7, k - 1, k + 1 rows and all at once, crossing query boundaries, the last one short: the assembled array equals the
    single call bit for bit; a call writes [row0, row0 + n_rows) only; n_rows == 0 writes nothing"""
    rng = np.random.default_rng(77)
    B, k, V = 5, 9, 773
    n = B * k
    p = ref.sparse_randn(rng, (n, V), 0.9, NP_OF[p_dtype])
    q = ref.sparse_randn(rng, (B, V), 0.2)
    single = _rerank_scores(p, q, k, p_dtype)
    assert ref.ulp_distance32(single, ref.rerank_scores_ref(p, q, k).exact32).max() <= 1
    pt, qt = _dev(p), _dev(q)
    for chunk in (1, 7, k - 1, k + 1, n):
        out = torch.full((n,), float(SENTINEL), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        want = np.full(n, SENTINEL, dtype=np.float32)
        for r0 in range(0, n, chunk):
            rows = min(chunk, n - r0)
            nat.check(nat.lib().vs_rerank_scores(_ptr(pt[r0:]), p_dtype, V, 0, r0, _ptr(qt), V, B, k, V, _ptr(out), 0, None))
            _same_bits(out.cpu().numpy(), want, f"chunk={chunk} row0={r0}: n_rows == 0 wrote")
            nat.check(nat.lib().vs_rerank_scores(_ptr(pt[r0:]), p_dtype, V, rows, r0, _ptr(qt), V, B, k, V, _ptr(out), 0, None))
            want[r0:r0 + rows] = single[r0:r0 + rows]
            _same_bits(out.cpu().numpy(), want, f"chunk={chunk} row0={r0} n_rows={rows}")       # (sentinels outside the chunk included)


@DTYPES
def test_rerank_scores_grid_stride_loop(p_dtype):
    """more than 4 x 8192 rows: B * k = 40 x 1000 at V = 260"""
    rng = np.random.default_rng(5)
    B, k, V = 40, 1000, 260
    p = ref.dyadic_signed(rng, (B * k, V), NP_OF[p_dtype])
    q = ref.dyadic_signed(rng, (B, V))
    _same_bits(_rerank_scores(p, q, k, p_dtype), ref.rerank_scores_ref(p, q, k).exact32, "40 x 1000 rows")


@DTYPES
def test_rerank_scores_special_values(p_dtype):
    """a zero passage element (+0.0 or -0.0) contributes nothing whatever the query holds (inf, NaN); a non-zero one against inf gives
    inf with the product's sign"""
    rng = np.random.default_rng(9)
    B, k, V = 2, 6, 1029
    p = ref.dyadic_signed(rng, (B * k, V), NP_OF[p_dtype])
    q = ref.dyadic_signed(rng, (B, V))
    cols = [0, 3, 255, 256, 771, 1027, 1028]              # unrolled loop, single-step loop and the V % 4 tail
    p[:, cols] = 0
    p[1::2, cols] = -0.0
    q[0, cols] = (np.inf, np.nan, -np.inf, np.nan, np.inf, np.nan, -np.inf)
    q[1, cols] = (np.nan, np.inf, np.nan, -np.inf, np.nan, np.inf, np.nan)
    plain = q.copy()
    plain[:, cols] = 0
    want = ref.rerank_scores_ref(p, plain, k).exact32
    assert np.isfinite(want).all()
    _same_bits(_rerank_scores(p, q, k, p_dtype, ldp_pad=1), want, "zero passage elements against inf / NaN")
    # non-zero passage elements against +inf (query 0) and -inf (query 1)
    q2 = plain.copy()
    q2[0, 1028], q2[1, 4] = np.inf, -np.inf
    p2 = p.copy()
    p2[0, 1028], p2[1, 1028], p2[2, 1028], p2[3, 1028] = 2.0, -2.0, 0.0, -0.0
    p2[k:, 4] = 0.0
    p2[k + 0, 4], p2[k + 1, 4], p2[k + 3, 4] = 2.0, -2.0, -0.0
    r = ref.rerank_scores_ref(p2, q2, k).exact32
    assert r[0] == np.inf and r[1] == -np.inf and np.isfinite(r[2:k]).all()
    assert r[k] == -np.inf and r[k + 1] == np.inf and np.isfinite(r[k + 2:]).all()
    _same_bits(_rerank_scores(p2, q2, k, p_dtype), r, "non-zero passage elements against inf")


def test_rerank_scores_errors():
    B, k, V = 2, 4, 64
    p = torch.zeros((B * k, V), device="cuda")
    q = torch.zeros((B, V), device="cuda")
    out = torch.full((B * k,), float(SENTINEL), device="cuda")
    host = np.zeros((B * k, V), dtype=np.float32)
    torch.cuda.synchronize()

    def call(p_ptr=None, p_dtype=F32, ldp=V, n_rows=B * k, row0=0, ldq=V):
        return nat.lib().vs_rerank_scores(p_ptr or _ptr(p), p_dtype, ldp, n_rows, row0, _ptr(q), ldq, B, k, V, _ptr(out), 0, None)

    assert call() == nat.VS_OK
    assert call(n_rows=B * k, row0=1) == nat.VS_ERANGE
    assert call(n_rows=1, row0=B * k) == nat.VS_ERANGE
    assert call(n_rows=0, row0=B * k) == nat.VS_OK
    assert call(ldp=V - 1) == nat.VS_EINVAL
    assert call(ldq=V - 1) == nat.VS_EINVAL
    assert call(p_dtype=nat.VS_I32) == nat.VS_EINVAL
    assert call(p_ptr=C.c_void_p(host.ctypes.data)) == nat.VS_EINVAL
    assert (out.cpu().numpy() == 0).all()


# ---- vs_rerank_topk --------------------------------------------------------------------------------------------------------------
def _rerank_topk(scores, ids):
    B, k = scores.shape
    st, it = _dev(scores), _dev(ids)
    out_ids = torch.full((B, k), -77, dtype=torch.int64, device="cuda")
    out_sc = torch.full((B, k), float(SENTINEL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    nat.check(nat.lib().vs_rerank_topk(_ptr(st), _ptr(it), B, k, _ptr(out_ids), _ptr(out_sc), 0, None))
    return out_ids.cpu().numpy(), out_sc.cpu().numpy()


def _check_rerank_topk(scores, ids, what):
    got_ids, got_sc = _rerank_topk(scores, ids)
    want_ids, want_sc = ref.rerank_topk_ref(scores, ids)
    _same_ids(got_ids, want_ids, what)
    _same_bits(got_sc, want_sc, what)
    # every output row is a permutation of its input row (pairs: id with score, zeros as +0.0)
    pairs_in = np.stack([ids, ref.bits32(scores + np.float32(0)).astype(np.int64)], axis=-1)
    pairs_out = np.stack([got_ids, ref.bits32(got_sc).astype(np.int64)], axis=-1)
    for b in range(ids.shape[0]):
        assert sorted(map(tuple, pairs_in[b].tolist())) == sorted(map(tuple, pairs_out[b].tolist())), f"{what}: row {b} is no permutation"
    return got_ids, got_sc


@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 100, 127, 128, 129, 1000, 1024, 1025, 2047, 2048])
def test_rerank_topk_order(k, B):
    """(score descending, first-stage rank ascending) around every sort width; 64-bit ids (>= 2^40) pass through; -inf / id -1 padding
    stays last in its order; -0.0 ties +0.0"""
    rng = np.random.default_rng(k * 8 + B)
    for pattern in ref.RERANK_PATTERNS:
        sc, ids = ref.rerank_case(rng, pattern, B, k)
        got_ids, got_sc = _check_rerank_topk(sc, ids, f"k={k} B={B} {pattern}")
        if pattern == "all_equal":
            assert (got_ids == ids).all(), "equal scores: the first-stage order must come back unchanged"
        if pattern == "pad_tail" and k >= 3:
            n_pad = k // 3
            assert (got_ids[:, k - n_pad:] == -1).all() and (got_sc[:, k - n_pad:] == -np.inf).all() and (got_ids[:, :k - n_pad] >= 2 ** 40).all()


def test_rerank_topk_block_stride_loop():
    """B = 5000 > the 4096-block grid"""
    rng = np.random.default_rng(3)
    sc, ids = ref.rerank_case(rng, "three_values", 5000, 5)
    _check_rerank_topk(sc, ids, "B=5000 k=5")


def test_rerank_topk_errors():
    sc = torch.zeros((1, 2049), device="cuda")
    ids = torch.zeros((1, 2049), dtype=torch.int64, device="cuda")
    o_ids, o_sc = torch.empty_like(ids), torch.empty_like(sc)
    host = np.zeros((1, 2049), dtype=np.float32)
    torch.cuda.synchronize()
    assert nat.lib().vs_rerank_topk(_ptr(sc), _ptr(ids), 1, 2049, _ptr(o_ids), _ptr(o_sc), 0, None) == nat.VS_EUNSUPPORTED
    assert nat.lib().vs_rerank_topk(_ptr(sc), _ptr(ids), 1, 2048, _ptr(o_ids), _ptr(o_sc), 0, None) == nat.VS_OK
    assert nat.lib().vs_rerank_topk(C.c_void_p(host.ctypes.data), _ptr(ids), 1, 2048, _ptr(o_ids), _ptr(o_sc), 0, None) == nat.VS_EINVAL


# ---- vs_merge_topk ---------------------------------------------------------------------------------------------------------------
def _merge_host(ids, sc, k):
    B, n = ids.shape
    ids, sc = np.ascontiguousarray(ids, dtype=np.int64), np.ascontiguousarray(sc, dtype=np.float32)
    o_ids = np.full((B, k), -77, dtype=np.int64)
    o_sc = np.full((B, k), SENTINEL, dtype=np.float32)
    nat.check(nat.lib().vs_merge_topk(C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data), B, n, k, C.c_void_p(o_ids.ctypes.data),
                                      C.c_void_p(o_sc.ctypes.data), 0, None))
    return o_ids, o_sc


def _check_merge(ids, sc, k, what, merge=_merge_host):
    got_ids, got_sc = merge(ids, sc, k)
    want_ids, want_sc = ref.merge_topk_ref(ids, sc, k)
    _same_ids(got_ids, want_ids, what)
    _same_bits(got_sc, want_sc, what)


MERGE_K = [1, 100, 128, 129, 2048]


@pytest.mark.parametrize("k", MERGE_K)
@pytest.mark.parametrize("n_cand", ["k", "k+1", 4095, 4096, 4097, 6145, 8192, 16384, 100000])
def test_merge_topk_laws(n_cand, k):
    """one fill of the 4096-key buffer, and 2 to 48 streaming rounds of merge_select, under every score law"""
    n = {"k": k, "k+1": k + 1}.get(n_cand, n_cand)
    assert n >= k
    rng = np.random.default_rng(n * 7 + k)
    B = 2 if n >= 100000 else 3
    for law in ref.MERGE_LAWS:
        _check_merge(ref.merge_ids(rng, B, n), ref.merge_scores(rng, law, B, n, k), k, f"n_cand={n} k={k} {law}")


@pytest.mark.parametrize("n_cand", [300, 5000, 8192])
def test_merge_topk_drops_ids_outside_32_bits(n_cand):
    """ids -1, 2^32 - 1, 2^32 and 2^40 carry the best scores and are dropped, never aliased; 2^32 - 2 and 0 are kept"""
    rng = np.random.default_rng(n_cand)
    B, k = 3, 100
    ids = ref.merge_ids(rng, B, n_cand)
    sc = ref.merge_scores(rng, "few", B, n_cand, k)
    for b in range(B):
        bad = rng.choice(np.flatnonzero((ids[b] != 0) & (ids[b] != ref.ID_LIMIT - 1)), size=40, replace=False)
        ids[b, bad] = np.resize(np.array([-1, 2 ** 32 - 1, 2 ** 32, 2 ** 40, 2 ** 32 + 5, -2 ** 40], dtype=np.int64), 40)
        sc[b, bad] = 50.0
        sc[b, ids[b] == ref.ID_LIMIT - 1] = 40.0
        sc[b, ids[b] == 0] = 40.0
    want_ids, _ = ref.merge_topk_ref(ids, sc, k)
    assert (want_ids[:, 0] == 0).all() and (want_ids[:, 1] == 2 ** 32 - 2).all()
    _check_merge(ids, sc, k, f"n_cand={n_cand}")


@pytest.mark.parametrize("n_cand", [200, 5000, 12289])
def test_merge_topk_short_rows_get_a_padded_tail(n_cand):
    """fewer than k real candidates -> id -1 / score -inf behind them; a row of only pads; a full row beside them"""
    rng = np.random.default_rng(n_cand + 1)
    B, k = 4, 100
    ids = ref.merge_ids(rng, B, n_cand)
    sc = ref.merge_scores(rng, "few", B, n_cand, k)
    keep = rng.permutation(n_cand)[:37]                   # row 0: 37 real candidates, spread over the rounds
    row0 = np.full(n_cand, -1, dtype=np.int64)
    row0[keep] = ids[0, keep]
    ids[0] = row0
    ids[1] = -1                                           # row 1: only pads
    ids[2, :n_cand - 99] = 2 ** 32 - 1                    # row 2: 99 real ones, all in the last slots
    sc[2, -1] = -np.inf                                   # (a real candidate may score -inf: it precedes the pads)
    want_ids, want_sc = ref.merge_topk_ref(ids, sc, k)
    assert (want_ids[0, 37:] == -1).all() and (want_ids[1] == -1).all() and (want_sc[1] == -np.inf).all() and (want_ids[3] >= 0).all()
    assert want_ids[2, 98] == ids[2, -1] and want_ids[2, 99] == -1
    _check_merge(ids, sc, k, f"n_cand={n_cand}")


def test_merge_topk_signed_zeros_tie():
    """-0.0 == +0.0: the id decides, and the zero comes back as +0.0"""
    rng = np.random.default_rng(8)
    for n_cand, k in ((64, 64), (300, 100), (5000, 129)):
        ids = ref.merge_ids(rng, 3, n_cand)
        sc = rng.choice(np.array([0.0, -0.0, -1.0, -0.0, 0.0, 1.0], dtype=np.float32), size=(3, n_cand))
        if n_cand > 4096:
            sc[sc > 0] = -2.0                             # the zeros are the winners, across the round boundary
        _check_merge(ids, sc, k, f"n_cand={n_cand} k={k}")


def test_merge_topk_many_rows():
    """B = 600 > the 512-block grid (block-stride loop), and B * n_cand > 4096 * 256 (the key builder's grid-stride loop)"""
    rng = np.random.default_rng(6)
    B, n, k = 600, 2048, 100
    ids = np.stack([rng.permutation(50000)[:n] for _ in range(B)]).astype(np.int64)
    _check_merge(ids, ref.merge_scores(rng, "few", B, n, k), k, "B=600")
    _check_merge(ids[:1], ref.merge_scores(rng, "few", 1, n, k), k, "B=1")


@pytest.mark.parametrize("side_stream", [False, True], ids=["default-stream", "side-stream"])
def test_merge_topk_device_tensors(side_stream):
    """device inputs and outputs with a stream: only enqueued; read after synchronising the stream"""
    rng = np.random.default_rng(12)
    stream = torch.cuda.Stream() if side_stream else torch.cuda.default_stream()
    with torch.cuda.stream(torch.cuda.default_stream()):
        default_handle = current_stream(0)

    def merge(ids, sc, k):
        B, n = ids.shape
        it, st = _dev(ids), _dev(sc)
        o_ids = torch.full((B, k), -77, dtype=torch.int64, device="cuda")
        o_sc = torch.full((B, k), float(SENTINEL), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            handle = current_stream(0)
            assert (handle.value != default_handle.value) == side_stream
            nat.check(nat.lib().vs_merge_topk(_ptr(it), _ptr(st), B, n, k, _ptr(o_ids), _ptr(o_sc), 0, handle))
        stream.synchronize()
        return o_ids.cpu().numpy(), o_sc.cpu().numpy()

    for n, k in ((800, 100), (6145, 129), (16384, 2048)):
        for law in ("few", "runs8"):
            _check_merge(ref.merge_ids(rng, 3, n), ref.merge_scores(rng, law, 3, n, k), k, f"device n_cand={n} k={k} {law}", merge)
    # mixed: device inputs, host outputs (blocking)
    ids, sc = ref.merge_ids(rng, 3, 5000), ref.merge_scores(rng, "few", 3, 5000, 100)
    it, st = _dev(ids), _dev(sc)
    o_ids, o_sc = np.empty((3, 100), dtype=np.int64), np.empty((3, 100), dtype=np.float32)
    torch.cuda.synchronize()
    nat.check(nat.lib().vs_merge_topk(_ptr(it), _ptr(st), 3, 5000, 100, C.c_void_p(o_ids.ctypes.data), C.c_void_p(o_sc.ctypes.data), 0, None))
    want = ref.merge_topk_ref(ids, sc, 100)
    _same_ids(o_ids, want[0], "device in, host out")
    _same_bits(o_sc, want[1], "device in, host out")


def test_merge_topk_errors():
    ids = np.zeros((1, 4096), dtype=np.int64)
    sc = np.zeros((1, 4096), dtype=np.float32)
    o_ids, o_sc = np.zeros((1, 4096), dtype=np.int64), np.zeros((1, 4096), dtype=np.float32)

    def call(n, k):
        return nat.lib().vs_merge_topk(C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data), 1, n, k, C.c_void_p(o_ids.ctypes.data),
                                       C.c_void_p(o_sc.ctypes.data), 0, None)

    assert call(4096, 2049) == nat.VS_EUNSUPPORTED
    assert call(4096, 2048) == nat.VS_OK
    for k in MERGE_K:
        assert call(k - 1, k) == nat.VS_ERANGE
        assert call(k, k) == nat.VS_OK


# ---- vs_head_pool_mean_topk, vs_head_pool ----------------------------------------------------------------------------------------
def _mean_topk(x, t):
    B, L, V = x.shape
    xt = _dev(x)
    out = torch.full((B, V), float(SENTINEL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    nat.check(nat.lib().vs_head_pool_mean_topk(_ptr(xt), B, L, V, t, _ptr(out), 0, None))
    return out.cpu().numpy()


def _head_pool(x):
    B, L, V = x.shape
    xt = _dev(x)
    out = torch.full((B, V), float(SENTINEL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    nat.check(nat.lib().vs_head_pool(_ptr(xt), B, L, V, _ptr(out), 0, None))
    return out.cpu().numpy()


@pytest.mark.parametrize("L", ["t", "t+1", 33, 512])
@pytest.mark.parametrize("t", [1, 2, 31, 32])
def test_pooling_dyadic_bit_exact(t, L):
    """positive dyadic logits: elu1p is x + 1 and every sum is exact in float32 -> bit-equal, for ascending, descending, equal and
    duplicated logits along L and with -inf among them (the insertion sort's paths); V odd"""
    L = {"t": t, "t+1": t + 1}.get(L, L)
    rng = np.random.default_rng(100 * t + L)
    B, V = 2, 67
    for pattern in ref.POOL_PATTERNS:
        x = ref.pool_logits_dyadic(rng, pattern, B, L, V)
        _same_bits(_mean_topk(x, t), ref.mean_topk_ref(x, t).astype(np.float32), f"mean of top {t}, L={L} {pattern}")
        _same_bits(_head_pool(x), ref.head_pool_ref(x).astype(np.float32), f"max pool, L={L} {pattern}")


def test_pooling_single_position():
    rng = np.random.default_rng(1)
    for pattern in ("duplicates", "neg_inf"):
        x = ref.pool_logits_dyadic(rng, pattern, 3, 1, 129)
        _same_bits(_mean_topk(x, 1), ref.mean_topk_ref(x, 1).astype(np.float32), f"L=1 t=1 {pattern}")
        _same_bits(_head_pool(x), ref.head_pool_ref(x).astype(np.float32), f"L=1 {pattern}")


@pytest.mark.parametrize("t", [1, 2, 31, 32])
def test_pooling_mixed_sign(t):
    """general logits: the tolerance of test_mean_pooling_with_pooling_topk (rtol 1e-5, atol 1e-6), against float64"""
    rng = np.random.default_rng(40 + t)
    for L in sorted({t, t + 1, 33, 512}):
        x = (rng.standard_normal((2, L, 1001)) * 2).astype(np.float32)
        x[rng.random(x.shape) < 0.05] = -np.inf
        np.testing.assert_allclose(_mean_topk(x, t), ref.mean_topk_ref(x, t), rtol=1e-5, atol=1e-6, err_msg=f"t={t} L={L}")
        np.testing.assert_allclose(_head_pool(x), ref.head_pool_ref(x), rtol=1e-5, atol=1e-6, err_msg=f"max pool L={L}")


def test_pooling_grid_stride_loops():
    """B * V = 150 x 29 523 > 256 x 16 384 outputs: both kernels go round their grid-stride loop"""
    rng = np.random.default_rng(2)
    B, L, V = 150, 4, 29523
    x = ref.pool_logits_dyadic(rng, "duplicates", B, L, V)
    x[:, :, ::7] = np.sort(x[:, :, ::7], axis=1)
    _same_bits(_mean_topk(x, 3), ref.mean_topk_ref(x, 3).astype(np.float32), "mean of top 3, 150 x 4 x 29523")
    _same_bits(_head_pool(x), ref.head_pool_ref(x).astype(np.float32), "max pool, 150 x 4 x 29523")


def test_pooling_errors():
    x = torch.zeros((2, 8, 67), device="cuda")
    out = torch.zeros((2, 67), device="cuda")
    torch.cuda.synchronize()
    assert nat.lib().vs_head_pool_mean_topk(_ptr(x), 2, 8, 67, 9, _ptr(out), 0, None) == nat.VS_ERANGE
    assert nat.lib().vs_head_pool_mean_topk(_ptr(x), 2, 8, 67, 33, _ptr(out), 0, None) == nat.VS_EUNSUPPORTED
    assert nat.lib().vs_head_pool_mean_topk(_ptr(x), 2, 8, 67, 0, _ptr(out), 0, None) == nat.VS_EUNSUPPORTED
    assert nat.lib().vs_head_pool_mean_topk(_ptr(x), 2, 8, 67, 8, _ptr(out), 0, None) == nat.VS_OK
