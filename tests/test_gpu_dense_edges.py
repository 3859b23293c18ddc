"""The dense index -- pad_rows_kernel, dense_scores_kernel (128 x 128 main blocks, 32 x 128 quarter blocks, split-K slices),
splitk_reduce_kernel, the launch plan, the batch slices and selectors of vs_dense_search, fp16 storage, leading dimensions, the
sparsity-aware build (count_nz_kernel / fill_csr_kernel) and the pool mode of the same GEMM kernel (vs_head_project_pool) -- against the
plain references of tests/_dense_ref.py (pinned on the CPU by tests/test_dense_ref_cpu.py), at the tile, K, batch and dtype edges where
their loops end.  Run on MI355X.

Bars.  Unless a test says otherwise its data is small-dyadic (matrix k / 4 in [0, 1.75], queries k / 2 in [-2, 1.5]): every fp32 sum is
exact in any order, so scores are bit-equal to the fp64 reference and ids / scores of a search equal the canonical top-k (score descending,
id ascending) exactly.  Non-dyadic scores: inside ref.err_bound, derived from one rounding per product and per addition.  Shapes come from
the device's CU count through ref.dense_plan, the test-side mirror of launch_dense_scores; a test first asserts that the mirror reports
the branch it is there for."""
import ctypes as C

import numpy as np
import pytest
import torch

import _dense_ref as ref
from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex

pytestmark = pytest.mark.gpu

F32, F16 = nat.VS_F32, nat.VS_F16


@pytest.fixture(scope="module")
def cu():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _same_bits(got, want, what):
    got, want = _np(got), _np(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} scores differ, first at {np.argwhere(bad)[:4].tolist()}: " \
                          f"got {got[bad][:4]} want {want[bad][:4]}"


def _same_ids(got, want, what):
    got, want = _np(got), _np(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.int64, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} ids differ, first at {np.argwhere(bad)[:4].tolist()}: " \
                          f"got {got[bad][:4]} want {want[bad][:4]}"


def _check(idx, q, want, ks, what, filter=None, allowed=None):
    """idx.scores(q) is `want` bit for bit (unfiltered), idx.search(q, k) the canonical top-k of `want` for every k"""
    if filter is None:
        _same_bits(idx.scores(q), want, f"{what} scores")
    for k in ks:
        ids, sc = idx.search(q, k, filter=filter)
        w_ids, w_sc = ref.canonical_topk(want, k, allowed)
        _same_ids(ids, w_ids, f"{what} k={k} ids")
        _same_bits(sc, w_sc, f"{what} k={k} scores")


# ---- a. the quarter-block kernel alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,N,B", ref.QUARTER_CASES)
def test_quarter_block_kernel_sweep(cu, V, N, B):
    """N small: no full round of main blocks, every document goes through the 32 x 128 kernel.  One K chunk, V around the 32- and
    512-column boundaries, partial document and query tiles.  Host (numpy) matrix and queries."""
    p = ref.dense_plan(N, B, V, cu)
    assert (p.main_doc_tiles, p.kind) == (0, "quarter") and ref.dyadic_ok(V)
    mat, q = ref.dyadic_np(V * 1000 + N + B, N, B, V)
    idx = DeviceIndex.from_dense(mat)
    _check(idx, q, ref.exact32(q, mat), sorted({1, min(N, 7), N}), f"V={V} N={N} B={B}")
    idx.close()


# ---- b. main kernel + quarter-block tail ---------------------------------------------------------------------------------------------
def _plant(mat, q, positions):
    """row positions[j] becomes the best possible document of query j % B: 1.75 where the query is positive, 0 elsewhere"""
    for j, n in enumerate(positions):
        mat[n] = (q[j % q.shape[0]] > 0).float() * 1.75


def _main_case(cu, V, B, N, kind, seed, host=False):
    p = ref.dense_plan(N, B, V, cu)
    assert p.main_doc_tiles > 0 and p.kind == kind and ref.dyadic_ok(V), f"V={V} B={B} N={N}: the mirror plans {p}"
    mat, q = ref.dyadic_dev(seed, N, B, V)
    planted = sorted({5, p.n_begin - 1, min(p.n_begin, N - 1), N - 1})            # first tile, last main tile, first tail document, the last one
    _plant(mat, q, planted)
    want = ref.exact32(q, mat)
    w_ids = ref.canonical_topk(want, 4)[0].cpu().numpy()
    if V >= 33:                                                                   # (narrower rows tie with random ones: the reference still decides)
        for j, n in enumerate(planted):
            assert n in w_ids[j % B], f"document {n} was planted as a top document of query {j % B}"
    idx = DeviceIndex.from_dense(mat.cpu().numpy() if host else mat)
    _check(idx, q, want, (1, 7), f"V={V} B={B} N={N} ({p.main_doc_tiles} main tiles, {p.kind} tail of {p.n_tail})")
    idx.close()


def test_main_kernel_with_quarter_block_tail(cu):
    """One and two full rounds of 128 x 128 blocks; V <= 992 is too short to split, so the 0, 1, 127 or 129 documents behind the rounds go
    to quarter blocks.  One K chunk (V = 1: both prefetches clamp to chunk 0), V just past a 32- and a 512-column boundary, B = 1, 127, 129
    and three query tiles.  The expected top documents sit in the first tile, the last main tile, at the first tail document and at N - 1."""
    for i, (V, B, N, rounds, r) in enumerate(ref.main_quarter_cases(cu)):
        q_tiles = ref.ceil_div(B, 128)
        kind = "none" if r == 0 and (2 * cu) % q_tiles == 0 else "quarter"
        assert ref.dense_plan(N, B, V, cu).main_doc_tiles == rounds * 2 * cu // q_tiles
        _main_case(cu, V, B, N, kind, 100 + i)


def test_main_tiles_clamped_to_whole_tiles(cu):
    """doc_tiles * q_tiles is a multiple of the slot count while N % 128 != 0: the full rounds must give the partial tile to the tail"""
    for i, ((V, B, N), kind) in enumerate(zip(ref.clamp_cases(cu), ("quarter", "split"))):
        p = ref.dense_plan(N, B, V, cu)
        assert (ref.ceil_div(N, 128) * ref.ceil_div(B, 128)) % (2 * cu) == 0 and (p.main_doc_tiles, p.n_tail) == (N // 128, N % 128)
        _main_case(cu, V, B, N, kind, 200 + i)


# ---- c. split-K tail --------------------------------------------------------------------------------------------------------------------
def test_split_k_tail(cu):
    """Chunk counts 32, 32, 35 and 65: two and three slices, cps rounded up to whole summation blocks, a last slice of 16, 3 and 1 chunks;
    one and two query tiles; a tail of 1 and of 200 documents.  One matrix comes from host memory in two upload chunks."""
    for i, (V, B, N, r, host) in enumerate(ref.split_cases(cu)):
        p = ref.dense_plan(N, B, V, cu)
        assert p.n_tail == r and p.S >= 2 and p.cps % 16 == 0
        if host:
            assert ((256 << 20) // (V * 4)) < N
        _main_case(cu, V, B, N, "split", 300 + i, host=host)


def test_split_k_tail_non_dyadic_invariance(cu):
    """Every fp32 sum rounds (values in [0.01, 3.01)), V = 1100: 35 chunks, a last summation block of 3.  Tail rows that are copies of
    main-round rows score bit-identically to them; 128 queries score bit-identically inside a batch of 256 (another plan); every score is
    inside err_bound of the fp64 product."""
    V, n_main, n_copy = ref.invariance_case(cu)
    for B in (128, 256):
        p = ref.dense_plan(n_main + n_copy, B, V, cu)
        assert (p.n_begin, p.n_tail, p.kind) == (n_main, n_copy, "split"), f"B={B}: the mirror plans {p}"
    g = torch.Generator(device="cuda").manual_seed(5)
    mat = torch.rand((n_main + n_copy, V), device="cuda", generator=g) * 3 + 0.01
    mat[n_main:] = mat[n_main - n_copy - 77:n_main - 77]                          # (rows of the last main tiles)
    mat[n_main + 1] = mat[3]
    q = torch.rand((256, V), device="cuda", generator=g) * 3 + 0.01
    idx = DeviceIndex.from_dense(mat)
    s256 = idx.scores(q)
    _same_bits(s256[:, n_main:][:, [0] + list(range(2, n_copy))], s256[:, n_main - n_copy - 77:n_main - 77][:, [0] + list(range(2, n_copy))],
               "tail documents against their copies in a main round")
    _same_bits(s256[:, n_main + 1], s256[:, 3], "tail document against its copy in the first tile")
    _same_bits(idx.scores(q[:128]), s256[:128], "a batch of 128 against the same queries inside a batch of 256")
    idx.close()
    err = (torch.from_numpy(s256).cuda().double() - ref.scores64(q, mat)).abs()
    bound = ref.err_bound(q, mat, ldp=ref.ldp_of(V))
    print(f"V={V}: max err / bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} scores outside the derived bound, max err / bound {float((err / bound).max()):.3f}"


# ---- d. workspace fallback ----------------------------------------------------------------------------------------------------------------
def test_split_workspace_fallback(cu):
    """A tail that could be split (S >= 2) but whose block sums would take more than 256 MB goes to quarter blocks; one document tile
    fewer stays inside the limit and is split.  Same matrix, the shorter index its first rows."""
    V, B, n_over, n_under = ref.fallback_cases(cu)
    over, under = ref.dense_plan(n_over, B, V, cu), ref.dense_plan(n_under, B, V, cu)
    assert over.kind == "quarter" and over.S >= 2 and over.main_doc_tiles > 0 and over.ws_bytes > ref.WS_LIMIT, f"the mirror plans {over}"
    assert under.kind == "split" and under.ws_bytes <= ref.WS_LIMIT, f"the mirror plans {under}"
    mat, q = ref.dyadic_dev(41, n_over, B, V)
    _plant(mat, q, (5, over.n_begin - 1, over.n_begin, n_under - 1, n_over - 1))
    want = ref.exact32(q, mat)
    torch.cuda.empty_cache()                                                      # (the reference's fp64 blocks: the index takes 3 GB of its own)
    for N in (n_over, n_under):
        idx = DeviceIndex.from_dense(mat[:N])
        _check(idx, q, want[:, :N].contiguous(), (1, 7), f"V={V} B={B} N={N}")
        idx.close()


# ---- e. selection ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", ref.SELECT_N)
def test_selectors_of_the_dense_search(N):
    """V = 8 around the switch from merge_topk_kernel to select_topk_kernel (8192 / 8193 rows) and k around the 2048 of one select pass, up
    to k = N.  A constant matrix ties every score of a query: ids 0 .. k - 1.  A zero query (all scores +0.0), all-negative scores and
    mixed signs on one random matrix."""
    V = 8
    rng = np.random.default_rng(N)
    const = np.full((N, V), 0.5, dtype=np.float32)
    qc = np.stack([np.full(V, 1.5), np.full(V, -2.0), np.zeros(V), rng.integers(-4, 4, size=V) / 2]).astype(np.float32)
    idx = DeviceIndex.from_dense(const)
    want = ref.exact32(qc, const)
    assert (want == want[:, :1]).all()
    for k in ref.select_ks(N):
        ids, sc = idx.search(qc, k)
        _same_ids(ids, np.tile(np.arange(k, dtype=np.int64), (4, 1)), f"constant matrix N={N} k={k} ids")
        _same_bits(sc, np.repeat(want[:, :1], k, axis=1), f"constant matrix N={N} k={k} scores")
    idx.close()
    mat = rng.integers(1, 8, size=(N, V)).astype(np.float32) / 4                    # strictly positive
    q = np.stack([np.zeros(V), -rng.integers(1, 5, size=V) / 2, rng.integers(-4, 4, size=V) / 2, rng.integers(-4, 4, size=V) / 2]).astype(np.float32)
    want = ref.exact32(q, mat)
    assert (want[0] == 0).all() and (want[1] < 0).all() and (want[2:] > 0).any() and (want[2:] < 0).any()
    idx = DeviceIndex.from_dense(mat)
    _check(idx, q, want, ref.select_ks(N), f"zero / negative / mixed N={N}")
    _check(idx, torch.from_numpy(q).cuda(), torch.from_numpy(want).cuda(), (2049,), f"device queries N={N}")
    idx.close()


@pytest.mark.parametrize("N", [ref.SELECT_ABOVE, ref.SELECT_ABOVE + 1], ids=["merge_topk", "select_topk"])
def test_selectors_filtered_with_fewer_allowed_rows_than_k(N):
    """one filtered search per selector: 100 (shared mask) and 0 .. 120 (per-query masks) allowed rows, k = 150 and, over two select
    passes, 2049: the allowed rows in canonical order, then id -1 / score -inf"""
    V, B = 8, 4
    mat, q = ref.dyadic_np(N, N, B, V)
    want = ref.exact32(q, mat)
    rng = np.random.default_rng(N + 1)
    shared = np.zeros(N, dtype=bool)
    shared[rng.choice(N, size=100, replace=False)] = True
    shared[[0, N - 1]] = True
    per_q = np.zeros((B, N), dtype=bool)
    for b, n_allowed in enumerate((0, 1, 120, 64)):
        per_q[b, rng.choice(N, size=n_allowed, replace=False)] = True
    idx = DeviceIndex.from_dense(mat)
    for mask in (shared, per_q):
        for k in (150, 2049):
            ids, sc = idx.search(q, k, filter=mask)
            n_allowed = np.broadcast_to(mask, (B, N)).sum(axis=1)
            assert all((ids[b, n_allowed[b]:] == -1).all() and np.isneginf(sc[b, n_allowed[b]:]).all() for b in range(B))
            w_ids, w_sc = ref.canonical_topk(want, k, mask)
            _same_ids(ids, w_ids, f"N={N} k={k} mask{mask.shape} ids")
            _same_bits(sc, w_sc, f"N={N} k={k} mask{mask.shape} scores")
    idx.close()


# ---- f. batch slicing -------------------------------------------------------------------------------------------------------------------------
def test_batch_slices_of_the_dense_search(cu):
    """B * N * 8 bytes of keys pass 1 GiB: vs_dense_search runs the batch in two slices and must move the queries, the outputs and the
    per-query filter along.  Query bs_max - 1 allows every row, query bs_max five rows, the others each a random half.  Compared on
    the device."""
    N, B, V = ref.slice_case()
    p = ref.dense_plan(N, B, V, cu)
    assert 1 < p.bs_max < B and B * N * 8 > ref.SLICE_BYTES
    mat, q = ref.dyadic_dev(61, N, B, V)
    g = torch.Generator(device="cuda").manual_seed(62)
    mask = torch.rand((B, N), device="cuda", generator=g) < 0.5
    mask[p.bs_max - 1] = True
    mask[p.bs_max] = False
    mask[p.bs_max, [0, 77, 4096, N - 2, N - 1]] = True
    assert not bool((mask[p.bs_max - 1] == mask[p.bs_max]).all()) and not bool((mask[:B - p.bs_max] == mask[p.bs_max:]).all())
    want = ref.exact32(q, mat)
    idx = DeviceIndex.from_dense(mat)
    k = 10
    for allowed in (None, mask):
        ids, sc = idx.search(q, k, filter=allowed)
        w_ids, w_sc = ref.canonical_topk(want, k, allowed)
        what = "unfiltered" if allowed is None else "per-query mask"
        bad = (ids != w_ids).any(dim=1) | (sc.view(torch.int32) != w_sc.view(torch.int32)).any(dim=1)
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {B} queries differ, first {bad.nonzero()[:4].flatten().tolist()} (bs_max = {p.bs_max})"
        del w_ids, w_sc
    assert (ids[p.bs_max, 5:] == -1).all() and torch.isneginf(sc[p.bs_max, 5:]).all()
    idx.close()


# ---- g. dtypes and leading dimensions -------------------------------------------------------------------------------------------------------------
def _wide_case(seed=7, N=300, B=9, V=333):
    """fp32 values fp16 rounding changes, whose sums stay exact before and after it.  Even columns: matrix 1 + k / 4096 (13 significant
    bits, fp16 keeps 11: a grid of 2^-10 in [1, 2]) against queries k / 2; odd columns: matrix k / 4 against queries +-(1 + k / 4096).
    Every product lies on a grid of 2^-13 (2^-12 after rounding) and is below 4, so 333 of them sum exactly in fp32.  The last three rows
    and the last three queries hold only 2^-25 (a tie: rounds to 0), 3 * 2^-26 (rounds to 2^-24) and 2^-26 (rounds to 0): against a
    normal operand their products lie on a grid of 2^-38 below 2^-23, against each other on 2^-52 below 2^-49 -- exact again."""
    rng = np.random.default_rng(seed)
    mat = np.empty((N, V), dtype=np.float32)
    q = np.empty((B, V), dtype=np.float32)
    ev, od = np.arange(0, V, 2), np.arange(1, V, 2)
    mat[:, ev] = 1 + rng.integers(0, 4096, size=(N, ev.size)) / 4096
    mat[:, od] = rng.integers(0, 8, size=(N, od.size)) / 4
    q[:, ev] = rng.integers(-4, 4, size=(B, ev.size)) / 2
    q[:, od] = rng.choice([-1.0, 1.0], size=(B, od.size)) * (1 + rng.integers(0, 4096, size=(B, od.size)) / 4096)
    tiny = np.array([2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -26], dtype=np.float32)
    mat[-3:] = tiny[rng.integers(0, 3, size=(3, V))]
    q[-3:] = tiny[rng.integers(0, 3, size=(3, V))] * rng.choice([-1.0, 1.0], size=(3, V)).astype(np.float32)
    assert (ref.round_f16(mat) != mat).mean() > 0.3 and (ref.round_f16(q) != q).mean() > 0.3
    return mat, q


def _exact_or_fail(q, mat):
    """exact32, with the proof that the fp32 sums are exact in any order: the float32 cumulative sums forwards and backwards agree
    with the fp64 sum"""
    want = ref.exact32(q, mat)
    prod = q[:, None, :].astype(np.float32) * mat[None].astype(np.float32)
    for p in (prod, prod[..., ::-1]):
        assert (np.cumsum(p, axis=2, dtype=np.float32)[..., -1] == want).all()
    return want


DTYPE_COMBOS = [("f32-matrix-stored-f16", np.float32, F16, np.float32), ("f16-matrix", np.float16, None, np.float16),
                ("f16-queries-on-f32-index", np.float32, None, np.float16), ("f32-queries-on-f16-index", np.float16, None, np.float32)]


@pytest.mark.parametrize("name,mat_dtype,store,q_dtype", DTYPE_COMBOS, ids=[c[0] for c in DTYPE_COMBOS])
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_fp16_storage_and_inputs(name, mat_dtype, store, q_dtype, on_device):
    """round_f16 where the library documents it: an fp16-stored index rounds its matrix and the queries it is given; an fp32 index takes
    fp16 queries as they are.  Bit-exact scores and top-k; export_dense returns the stored values in both dtypes."""
    mat32, q32 = _wide_case()
    mat_in, q_in = mat32.astype(mat_dtype), q32.astype(q_dtype)
    f16_index = store == F16 or mat_dtype == np.float16
    stored = ref.round_f16(mat32) if f16_index else mat32
    q_used = ref.round_f16(q32) if (f16_index or q_dtype == np.float16) else q32
    want = _exact_or_fail(q_used, stored)
    assert (want != ref.exact32(q32, mat32)).mean() > 0.5                          # the rounding shows in the scores
    dev = (lambda a: torch.from_numpy(a).cuda()) if on_device else (lambda a: a)
    idx = DeviceIndex.from_dense(dev(mat_in), store_dtype=store)
    assert idx.info().store_dtype == (F16 if f16_index else F32)
    _check(idx, dev(q_in), want, (1, 7, mat32.shape[0]), name)
    e32, e16 = idx.export_dense(np.float32), idx.export_dense(np.float16)
    assert (e32.view(np.uint32) == stored.view(np.uint32)).all()
    assert (e16.view(np.uint16) == stored.astype(np.float16).view(np.uint16)).all()
    idx.close()


def _strided(a, pad, on_device, fill=np.nan):
    """the rows of `a` at leading dimension n_cols + pad, the padding holding NaN (a read of it shows) -> (array | CUDA tensor, ld)"""
    n, v = a.shape
    host = np.full((n, v + pad), fill, dtype=a.dtype)
    host[:, :v] = a
    return (torch.from_numpy(host).cuda() if on_device else host), v + pad


def _ptr(x):
    return C.c_void_p(x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data)


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_leading_dimensions_through_the_c_abi(dtype, on_device):
    """vs_index_create_dense / vs_index_export_dense with ld > n_cols, vs_index_search / vs_index_scores with ldq > n_cols, host and
    device pointers.  The padding columns of the inputs hold NaN; the padding of an export target keeps what it held."""
    N, B, V, k = 130, 5, 45, 9
    mat32, q32 = ref.dyadic_np(77, N, B, V)
    want = ref.exact32(q32, mat32)
    vs_dt = F32 if dtype == np.float32 else F16
    m, ld = _strided(mat32.astype(dtype), 3, on_device)
    h = C.c_void_p()
    torch.cuda.synchronize()
    nat.check(nat.lib().vs_index_create_dense(_ptr(m), vs_dt, vs_dt, N, V, ld, 0, C.byref(h)))
    idx = DeviceIndex(h)
    qs, ldq = _strided(q32.astype(dtype), 5, on_device)
    alloc = (lambda shape, dt, fill: torch.full(shape, fill, dtype=dt, device="cuda")) if on_device else \
            (lambda shape, dt, fill: np.full(shape, fill, dtype={torch.float32: np.float32, torch.int64: np.int64}[dt]))
    sc_all = alloc((B, N), torch.float32, -7.0)
    torch.cuda.synchronize()
    nat.check(nat.lib().vs_index_scores(h, _ptr(qs), vs_dt, ldq, B, _ptr(sc_all), None))
    _same_bits(sc_all, want, "vs_index_scores, ldq > n_cols")
    ids, sc = alloc((B, k), torch.int64, -9), alloc((B, k), torch.float32, -7.0)
    nat.check(nat.lib().vs_index_search(h, _ptr(qs), vs_dt, ldq, B, k, 1000, _ptr(ids), _ptr(sc), None))
    w_ids, w_sc = ref.canonical_topk(want, k)
    _same_ids(ids, w_ids + 1000, "vs_index_search, ldq > n_cols (id_offset 1000)")
    _same_bits(sc, w_sc, "vs_index_search, ldq > n_cols")
    h2 = C.c_void_p()                                                               # the same rows stored as packets: the other export kernel
    nat.check(nat.lib().vs_index_create_dense_auto(_ptr(m), vs_dt, vs_dt, N, V, ld, 1.0, 0, C.byref(h2)))
    packets = DeviceIndex(h2)
    assert packets.info().n_packets > 0 and idx.info().n_packets == 0
    for kind, handle in (("matrix", h), ("packets", h2)):
        for out_dtype in (np.float32, np.float16):
            out, ldo = _strided(np.zeros((N, V), dtype=out_dtype), 4, on_device, fill=-3.0)
            torch.cuda.synchronize()
            nat.check(nat.lib().vs_index_export_dense(handle, _ptr(out), F32 if out_dtype == np.float32 else F16, ldo))
            torch.cuda.synchronize()
            out = _np(out)
            assert (out[:, :V] == mat32.astype(out_dtype)).all(), f"{kind}: export as {out_dtype.__name__}, ld > n_cols"
            assert (out[:, V:] == -3.0).all(), f"{kind}: export as {out_dtype.__name__} wrote into the padding columns of its target"
    idx.close()
    packets.close()


# ---- h. the sparsity-aware build ----------------------------------------------------------------------------------------------------------------------
def _csr_equal(got, want, what):
    (g_ip, g_ix, g_d), (w_ip, w_ix, w_d) = got, want
    assert (g_ip == w_ip).all(), f"{what}: indptr differs, first row {int(np.argmax(g_ip != w_ip))}"
    assert (g_ix == w_ix).all(), f"{what}: {int((g_ix != w_ix).sum())} column ids differ, first at {int(np.argmax(g_ix != w_ix))}"
    assert (g_d.view(np.uint32) == w_d.view(np.uint32))[~np.isnan(w_d)].all() and (np.isnan(g_d) == np.isnan(w_d)).all(), f"{what}: values differ"


@pytest.mark.parametrize("n_cols", ref.AUTO_COLS)
def test_sparsity_aware_build(n_cols):
    """count_nz_kernel's 8-way head (from 7169 columns) and remainder, fill_csr_kernel's 1024-column steps and its second 32 Ki-column
    pass: export_csr is Tensor.to_sparse_csr of the matrix exactly (-0.0 dropped, NaN kept), export_dense the matrix, search and scores
    those of the MFMA index of the same matrix -- under dense queries, which from 32 764 columns on no longer fit the LDS image of the
    one-query CSR scan (it then reads them from memory)."""
    mat = ref.auto_matrix(n_cols)
    idx = DeviceIndex.from_dense(mat, max_density=1.0)
    info = idx.info()
    ip, ix, d = ref.nonzeros_csr(mat)
    assert info.kind == nat.VS_KIND_DENSE and info.nnz == ip[-1] and info.n_packets == int(((np.diff(ip) + 7) // 8).sum())
    _csr_equal(idx.export_csr(), (ip, ix, d), f"n_cols={n_cols}")
    assert (idx.export_dense() == mat).all()
    rng = np.random.default_rng(n_cols)
    q = rng.integers(-4, 4, size=(5, n_cols)).astype(np.float32) / 2
    want = ref.exact32(q, mat)
    ks = (1, 7, ref.AUTO_ROWS)
    _check(idx, q, want, ks, f"packets n_cols={n_cols}")
    mfma = DeviceIndex.from_dense(mat)
    assert mfma.info().n_packets == 0
    _check(mfma, q, want, ks, f"MFMA n_cols={n_cols}")
    for k in ks:
        (a_ids, a_sc), (m_ids, m_sc) = idx.search(q, k), mfma.search(q, k)
        _same_ids(a_ids, m_ids, f"packets against MFMA n_cols={n_cols} k={k}")
        _same_bits(a_sc, m_sc, f"packets against MFMA n_cols={n_cols} k={k}")
    idx.close()
    mfma.close()
    with_nan = ref.auto_matrix(n_cols, nan=True)                                 # (through the exports only: its scores are NaN)
    idx = DeviceIndex.from_dense(torch.from_numpy(with_nan).cuda(), max_density=1.0)
    assert idx.info().n_packets > 0
    _csr_equal(idx.export_csr(), ref.nonzeros_csr(with_nan), f"NaN n_cols={n_cols}")
    e = idx.export_dense()
    assert (np.isnan(e) == np.isnan(with_nan)).all() and (np.nan_to_num(e, nan=0.0) == np.nan_to_num(with_nan, nan=0.0)).all()
    idx.close()


@pytest.mark.parametrize("n_cols", [1025, 32769])
def test_sparsity_aware_build_fp16_storage_drops_what_rounds_to_zero(n_cols):
    mat = ref.auto_matrix(n_cols)
    rng = np.random.default_rng(n_cols + 1)
    tiny = np.array([2.0 ** -25, 2.0 ** -26, 3 * 2.0 ** -26, -(2.0 ** -25)], dtype=np.float32)      # -> 0, 0, 2^-24, -0
    spots = rng.random(mat.shape) < 0.05
    mat[spots] = tiny[rng.integers(0, 4, size=int(spots.sum()))]
    idx = DeviceIndex.from_dense(mat, store_dtype=F16, max_density=1.0)
    stored = ref.round_f16(mat)
    assert ((stored == 0) & (mat != 0)).sum() > 10 and idx.info().n_packets > 0
    _csr_equal(idx.export_csr(), ref.nonzeros_csr(stored), f"fp16 storage n_cols={n_cols}")
    assert (idx.export_dense(np.float16) == stored.astype(np.float16)).all() and (idx.export_dense() == stored).all()
    idx.close()


def test_sparsity_aware_build_stays_dense_beyond_16_bit_columns():
    mat = ref.auto_matrix(65_536)
    idx = DeviceIndex.from_dense(mat, max_density=1.0)
    assert idx.info().n_packets == 0 and idx.info().kind == nat.VS_KIND_DENSE
    q = np.random.default_rng(8).integers(-4, 4, size=(5, 65_536)).astype(np.float32) / 2
    _check(idx, q, ref.exact32(q, mat), (1, 7, ref.AUTO_ROWS), "n_cols=65536")
    assert (idx.export_dense() == mat).all()
    idx.close()


def test_sparsity_aware_build_density_threshold():
    """nnz == max_density * N * V keeps packets, one more non-zero makes the index dense"""
    N, V, dens = 16, 64, 0.25
    rng = np.random.default_rng(9)
    mat = np.zeros(N * V, dtype=np.float32)
    mat[rng.choice(N * V, size=int(dens * N * V), replace=False)] = 0.5
    mat = mat.reshape(N, V)
    assert int((mat != 0).sum()) == dens * N * V == 256
    idx = DeviceIndex.from_dense(mat, max_density=dens)
    assert idx.info().n_packets > 0 and idx.info().nnz == 256
    idx.close()
    mat[np.unravel_index(np.flatnonzero(mat.reshape(-1) == 0)[0], mat.shape)] = 0.25
    idx = DeviceIndex.from_dense(mat, max_density=dens)
    assert idx.info().n_packets == 0
    assert (idx.export_dense() == mat).all()
    idx.close()


def test_sparsity_aware_build_row_chunks():
    """2^20 + 5 rows of 4 columns: the build runs in chunks of 2^20 rows; rows 2^20 - 1 .. 2^20 + 4 straddle the cut"""
    N, V = (1 << 20) + 5, 4
    g = torch.Generator(device="cuda").manual_seed(10)
    mat = torch.randint(0, 3, (N, V), device="cuda", generator=g).float() / 2           # a third of the rows of a column are zero
    mat[0] = 0
    mat[(1 << 20) - 1] = torch.tensor([0.0, 1.0, 0.0, 0.5])
    mat[1 << 20] = torch.tensor([1.0, 0.0, 0.0, 1.0])
    mat[N - 1] = torch.tensor([0.5, 1.0, 1.0, 1.0])
    idx = DeviceIndex.from_dense(mat, max_density=1.0)
    host = mat.cpu().numpy()
    ip, ix, d = ref.nonzeros_csr(host)
    assert idx.info().n_packets == int((np.diff(ip) > 0).sum())
    _csr_equal(idx.export_csr(), (ip, ix, d), "2^20 + 5 rows")
    q = torch.tensor([[1.0, -0.5, 1.5, 0.5], [-1.0, 1.0, 0.0, -2.0]], device="cuda")
    _check(idx, q, ref.exact32(q, mat), (1, 100), "2^20 + 5 rows")
    idx.close()


@pytest.mark.parametrize("store", [F32, F16, nat.VS_NONE], ids=["f32", "f16", "binary"])
def test_one_query_scan_of_an_index_too_wide_for_its_lds_image(store):
    """65 535 columns: the fp32 image of a dense query (256 KB) does not fit the LDS, so the one-query CSR scan -- the path of a
    packet-stored dense index under dense queries, and of vs_index_scores -- reads the weights from memory.  All three value modes (the
    binary one ADDS the pad column's weight, which must be 0), the wave-private (k <= 128) and the shared (k > 128) top-k kernels, and
    their filtered instantiations."""
    n_cols, N = 65_535, ref.AUTO_ROWS
    mat = ref.auto_matrix(n_cols)
    ip, ix, d = ref.nonzeros_csr(mat)
    if store == nat.VS_NONE:
        mat, d = (mat != 0).astype(np.float32), None
    idx = DeviceIndex.from_csr(ip, ix.astype(np.int32), d, n_cols, store_dtype=store)
    q = np.random.default_rng(12).integers(-4, 4, size=(3, n_cols)).astype(np.float32) / 2
    want = ref.exact32(q, mat)
    _check(idx, q, want, (1, 7, 39, N), f"CSR n_cols={n_cols}")
    allowed = np.zeros(N, dtype=bool)
    allowed[[1, 4, 5, 8, 20, 38]] = True
    _check(idx, q, want, (3, N), f"CSR n_cols={n_cols}, filtered", filter=allowed, allowed=allowed)
    idx.close()
    big = np.tile(mat, (8, 1))                                                      # 320 rows: k = 129 .. 320 runs the shared-buffer kernel
    ip, ix, d = ref.nonzeros_csr(big)
    idx = DeviceIndex.from_csr(ip, ix.astype(np.int32), None if store == nat.VS_NONE else d, n_cols, store_dtype=store)
    want = ref.exact32(q, big)
    _check(idx, q, want, (129, 320), f"CSR n_cols={n_cols}, 320 rows")
    allowed = np.arange(320) % 3 == 0
    _check(idx, q, want, (129,), f"CSR n_cols={n_cols}, 320 rows, filtered", filter=allowed, allowed=allowed)
    idx.close()


# ---- i. pool mode ------------------------------------------------------------------------------------------------------------------------------------------
def _pool(hidden, W):
    B, L, H = hidden.shape
    V = W.shape[0]
    h, w = torch.from_numpy(hidden).cuda(), torch.from_numpy(W).cuda()
    out = torch.full((B, V), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    nat.check(nat.lib().vs_head_project_pool(_ptr(h), _ptr(w), B, L, H, V, _ptr(out), 0, None))
    return out.cpu().numpy()


@pytest.mark.parametrize("L,B,H,V", ref.POOL_CASES)
def test_pool_mode_of_the_gemm_kernel(L, B, H, V):
    """vs_head_project_pool == elu1p(max_l hidden @ W^T): L = 64 / 65 switches from 32-row to 128-row blocks, 128 / 129 to two blocks a
    sequence; rows past a sequence's end repeat its last row, never the next sequence's first.  Dyadic inputs: the logits and their max
    are exact, so where the max is positive (elu1p = x + 1, exact) the output is bit-equal; elsewhere exp() is inside the tolerance of
    test_fused_head_project_pool."""
    rng = np.random.default_rng(L * 1000 + B * 100 + H + V)
    hidden = rng.integers(-4, 4, size=(B, L, H)).astype(np.float32) / 2
    W = rng.integers(-8, 8, size=(V, H)).astype(np.float32) / 4
    if B > 1:                                                                       # the best row of a sequence would win the one before it too
        hidden[1:, 0] = np.where(W[0] > 0, 1.5, -2.0)
    m, want = ref.pool_ref(hidden, W)
    got = _pool(hidden, W)
    pos = m > 0
    assert pos.any() or V == 1
    _same_bits(got[pos], want[pos].astype(np.float32), f"L={L} B={B} H={H} V={V}, positive maxima")
    np.testing.assert_allclose(got[~pos], want[~pos], rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("L", [33, 129])
def test_pool_mode_all_logits_negative(L):
    """hidden > 0 against W < 0: every logit is negative, the output is exp(max) (the expm1 branch of pool_finish_kernel)"""
    rng = np.random.default_rng(L)
    B, H, V = 3, 96, 129
    hidden = rng.integers(1, 8, size=(B, L, H)).astype(np.float32) / 8
    W = -rng.integers(1, 8, size=(V, H)).astype(np.float32) / 8
    m, want = ref.pool_ref(hidden, W)
    assert (m < 0).all()
    np.testing.assert_allclose(_pool(hidden, W), want, rtol=2e-5, atol=2e-6)

