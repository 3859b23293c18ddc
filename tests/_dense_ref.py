"""Plain references of the dense index (vsearch_amd/csrc/dense.hip, dense_csr.h) and the shape tables its tests share.  numpy / torch
only, no library call: tests/test_dense_ref_cpu.py pins these functions to brute force and checks the shape tables on a machine without
a GPU, tests/test_gpu_dense_edges.py pins the HIP kernels to them.

Rules restated here (include/vsearch_hip.h, dense.hip):
  scores[b, n] = <q[b], mat[n]>; the accumulators start at +0.0, so a sum of zeros is +0.0 whatever the signs of its terms;
  top-k: score descending, id ascending; a filtered search holds id -1 / score -inf behind the allowed rows;
  fp16 storage rounds the matrix AND the queries to fp16 (round to nearest even); the sums stay fp32.
"""
from collections import namedtuple

import numpy as np
import torch

KC = 32                    # columns per K chunk: rows are padded to a multiple of it
SUM_BLOCK = 512            # columns per summation block (16 chunks)
WS_LIMIT = 256 << 20       # the split-K workspace limit
SLICE_BYTES = 1 << 30      # vs_dense_search keeps at most this many bytes of keys: the batch is cut into slices of bs_max queries
SELECT_ABOVE = 8192        # merge_topk_kernel up to this many rows, select_topk_kernel beyond


def ceil_div(a, b):
    return -(-a // b)


def ldp_of(V):
    return ceil_div(V, KC) * KC


# ---- references ----------------------------------------------------------------------------------------------------------------
def scores64(q, mat, block_bytes=1 << 30):
    """fp64 products q @ mat.T -> float64 [B, N].  numpy in -> numpy out; torch in -> torch out on the inputs' device, the matrix
    converted in row blocks of at most block_bytes of fp64."""
    if isinstance(mat, np.ndarray):
        return np.asarray(q, dtype=np.float64) @ np.asarray(mat, dtype=np.float64).T
    q64 = q.double()
    n, v = mat.shape
    rows = max(1, block_bytes // (8 * v))
    out = torch.empty((q.shape[0], n), dtype=torch.float64, device=mat.device)
    for r in range(0, n, rows):
        out[:, r:r + rows] = q64 @ mat[r:r + rows].double().t()
    return out


def exact32(q, mat):
    """scores64 as float32, for inputs whose sums are exact: what any summation order from +0.0 gives, -0.0 included (x + 0.0)."""
    s = scores64(q, mat)
    if isinstance(s, np.ndarray):
        return s.astype(np.float32) + np.float32(0)
    return s.float() + 0.0


def canonical_topk(all_scores, k, allowed=None):
    """Per row of float32 scores [B, N]: (ids int64 [B, k], scores float32 [B, k]) by score descending, id ascending -- a stable
    descending sort.  allowed: bool [N] or [B, N]; rows it excludes never appear, the positions behind the allowed ones hold -1 / -inf.
    numpy in -> numpy out; torch in -> torch out."""
    as_np = isinstance(all_scores, np.ndarray)
    s = torch.from_numpy(np.ascontiguousarray(all_scores, dtype=np.float32)) if as_np else all_scores
    assert s.dtype == torch.float32 and s.dim() == 2
    val, idx = torch.sort(s, dim=1, descending=True, stable=True)
    if allowed is not None:
        a = torch.from_numpy(np.ascontiguousarray(allowed)) if isinstance(allowed, np.ndarray) else allowed
        a = a.to(s.device).expand(s.shape)
        ok = torch.gather(a, 1, idx)
        front = torch.sort((~ok).to(torch.uint8), dim=1, stable=True)[1]          # allowed first, score order kept
        val, idx, ok = torch.gather(val, 1, front), torch.gather(idx, 1, front), torch.gather(ok, 1, front)
        val = torch.where(ok, val, torch.full_like(val, float("-inf")))
        idx = torch.where(ok, idx, torch.full_like(idx, -1))
    ids, sc = idx[:, :k].contiguous(), val[:, :k].contiguous()
    return (ids.numpy(), sc.numpy()) if as_np else (ids, sc)


def round_f16(x):
    return np.asarray(x).astype(np.float16).astype(np.float32)


def nonzeros_csr(mat):
    """Tensor.to_sparse_csr of a dense matrix: the elements with x != 0 in row-major order -- -0.0 is dropped, NaN is kept.
    -> (indptr int64 [N + 1], indices int64, data float32)"""
    mat = np.asarray(mat, dtype=np.float32)
    nz = mat != 0
    indptr = np.zeros(mat.shape[0] + 1, dtype=np.int64)
    np.cumsum(nz.sum(axis=1), out=indptr[1:])
    return indptr, np.nonzero(nz)[1].astype(np.int64), mat[nz]


Plan = namedtuple("Plan", "main_doc_tiles n_begin n_tail kind S cps n_sum_blocks ws_bytes bs_max chunks")


def dense_plan(N, B, V, cu):
    """Test-side mirror of launch_dense_scores for a batch of B queries (kind: 'none' | 'quarter' | 'split'; S, cps are 0 unless the tail
    is split), and bs_max as vs_dense_search computes it for a search of B queries."""
    ldp = ldp_of(V)
    doc_tiles, q_tiles = ceil_div(N, 128), ceil_div(B, 128)
    slots = cu * 2
    full_rounds = (doc_tiles * q_tiles) // slots
    main_doc_tiles = min(doc_tiles, (full_rounds * slots) // q_tiles)
    if main_doc_tiles * 128 > N:
        main_doc_tiles = N // 128
    n_begin = main_doc_tiles * 128
    n_tail = max(N - n_begin, 0)
    chunks = ldp // KC
    n_sum_blocks = ceil_div(chunks, 16)
    kind, S, cps, ws_bytes = "none", 0, 0, 0
    if n_tail > 0:
        tail_tiles = ceil_div(n_tail, 128) * q_tiles
        S = min(slots // max(tail_tiles, 1), chunks // 16)
        ws_bytes = n_sum_blocks * B * n_tail * 4
        if main_doc_tiles > 0 and S >= 2 and ws_bytes <= WS_LIMIT:
            kind = "split"
            cps = ceil_div(ceil_div(chunks, S), 16) * 16
            S = ceil_div(chunks, cps)
        else:
            kind, cps = "quarter", 0
    bs_max = max(1, min(B, SLICE_BYTES // (N * 8)))
    return Plan(main_doc_tiles, n_begin, n_tail, kind, S, cps, n_sum_blocks, ws_bytes, bs_max, chunks)


def err_bound(q, mat, ldp=None, nnz_row=None):
    """Tolerance of a score on non-dyadic data, derived: every product and every addition rounds at most once (relative 2^-24); a score
    is a sum of at most 512 terms a summation block plus one addition a block:
        (2 min(ldp, 512) + ceil(ldp / 512) + 2) 2^-24 (|q| @ |mat|^T),
    and for a packet-stored (logical dense) index, which adds a row's nnz_row products in one chain, (2 nnz_row + 2) 2^-24 (|q| @ |mat|^T).
    -> float64 [B, N], the kind of its inputs."""
    if nnz_row is not None:
        ops = 2 * nnz_row + 2
    else:
        ops = 2 * min(ldp, SUM_BLOCK) + ceil_div(ldp, SUM_BLOCK) + 2
    return scores64(abs(q), abs(mat)) * (ops * 2.0 ** -24)


def elu1p64(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x > 0, x + 1.0, np.expm1(np.minimum(x, 0.0)) + 1.0)


def pool_ref(hidden, W):
    """vs_head_project_pool: max over the L positions of hidden[b] @ W.T in fp64 -> (max float64 [B, V], elu1p of it)"""
    m = (np.asarray(hidden, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T).max(axis=1)
    return m, elu1p64(m)


# ---- data ------------------------------------------------------------------------------------------------------------------------
def dyadic_ok(V):
    """the small-dyadic laws below (matrix k / 4 in [0, 1.75], queries k / 2 in [-2, 1.5]: products on a grid of 1/8) sum exactly in
    fp32 in any order while V * 1.75 * 2 * 8 < 2^24"""
    return V * 1.75 * 2 * 8 < 2 ** 24


def dyadic_np(seed, N, B, V):
    rng = np.random.default_rng(seed)
    mat = rng.integers(0, 8, size=(N, V)).astype(np.float32) / 4
    q = rng.integers(-4, 4, size=(B, V)).astype(np.float32) / 2
    return mat, q


def dyadic_dev(seed, N, B, V, device="cuda"):
    g = torch.Generator(device=device).manual_seed(seed)
    mat = torch.randint(0, 8, (N, V), device=device, generator=g, dtype=torch.int8).float().div_(4)       # (int8: a 3 GB matrix stays 3 GB)
    q = torch.randint(-4, 4, (B, V), device=device, generator=g, dtype=torch.int8).float().div_(2)
    return mat, q


# ---- shape tables: built from the CU count through dense_plan, never from literals ----------------------------------------------------
def n_after_rounds(rounds, B, cu, r):
    """N whose plan for B queries has `rounds` full rounds of 128 x 128 blocks and r documents (N % 128 == r % 128) behind the main tiles
    -- where the main tiles of `rounds` rounds alone do not fill the rounds (q_tiles does not divide the slots), up to one tile more."""
    slots, q_tiles = 2 * cu, ceil_div(B, 128)
    main = (rounds * slots) // q_tiles
    need = ceil_div(rounds * slots, q_tiles)
    N = main * 128 + r
    if ceil_div(N, 128) < need:
        N = (need - 1) * 128 + (r % 128 or 128)
    return N


# a. quarter-block kernel alone (N small: no full round): a covering subset of V x N x B, every value of each list at least twice
QUARTER_CASES = [
    # (V, N, B)
    (1, 1, 1), (1, 129, 33), (1, 300, 129), (31, 127, 31), (31, 128, 1), (32, 128, 32), (32, 1, 129), (33, 129, 33), (33, 300, 1),
    (33, 127, 32), (511, 300, 31), (511, 1, 32), (512, 127, 129), (512, 129, 1), (513, 128, 33), (513, 300, 32), (513, 129, 129),
    (1055, 1, 31), (1055, 127, 1), (1055, 128, 129), (1055, 300, 33), (1, 128, 31),
]


def main_quarter_cases(cu):
    """b. main kernel + quarter-block tail (V <= 992: K too short to split) -> (V, B, N, rounds, r); r = 0 has no tail at all where the
    main tiles fill the rounds."""
    table = [(1, 1, 1, 0), (1, 129, 1, 129), (33, 127, 1, 1), (33, 257, 1, 127), (33, 128, 2, 129), (96, 128, 1, 127), (96, 1, 2, 1),
             (96, 257, 1, 0), (513, 129, 1, 0), (513, 1, 1, 129), (513, 127, 2, 127), (992, 128, 1, 1), (992, 257, 1, 129),
             (992, 129, 2, 1), (992, 127, 1, 0)]
    return [(V, B, n_after_rounds(rounds, B, cu, r), rounds, r) for V, B, rounds, r in table]


def clamp_cases(cu):
    """b. the clamp: doc_tiles * q_tiles is a multiple of the slot count and N % 128 != 0, so the full rounds would cover a partial tile
    -> (V, B, N), with a quarter-block and a split-K tail.  At 256 CUs N = 65 531."""
    return [(96, 128, 2 * cu * 128 - 5), (1100, 127, 2 * cu * 128 - 5)]


def split_cases(cu):
    """c. split-K tail -> (V, B, N, r, host matrix).  chunks 32, 32, 35, 65: S = 2 | 2 | 2 | 3, the last slice 16 | 16 | 3 | 1 chunks."""
    out = []
    for V in (993, 1024, 1100, 2049):
        for B, r in ((1, 1), (130, 200)):
            out.append((V, B, n_after_rounds(1, B, cu, r), r, False))
    out.append((993, 1, n_after_rounds(1, 1, cu, 200), 200, False))
    out.append((2049, 130, n_after_rounds(1, 130, cu, 1), 1, False))
    out.append((1100, 1, n_after_rounds(1, 1, cu, 200), 200, True))             # 4400-byte rows: two 256 MB upload chunks from 61 009 rows on
    return out


def invariance_case(cu):
    """c. non-dyadic: N = n_main + n_copy; a batch of 256 (two rounds) and one of 128 (one round) both end their main tiles at n_main and
    split the tail -> (V, n_main, n_copy)"""
    return 1100, 2 * cu * 128, 200


def fallback_cases(cu, B=128):
    """d. -> (V, B, N_over, N_under): both tails can be split (S >= 2); N_over's workspace passes 256 MB by less than one 128-document
    tile, N_under = N_over - 128 stays inside it.  The smallest V from 8200 up (in summation blocks) whose tail fits half the slots."""
    V = 8200
    while True:
        nsb = ceil_div(ldp_of(V) // KC, 16)
        n_tail = ceil_div(WS_LIMIT // (nsb * B * 4) + 1, 128) * 128
        if ceil_div(n_tail, 128) * ceil_div(B, 128) * 2 <= 2 * cu:
            N = n_after_rounds(1, B, cu, 0) + n_tail
            return V, B, N, N - 128
        V += SUM_BLOCK


SELECT_N = (4096, 4097, 8192, 8193, 12289)


def select_ks(N):
    return (1, 2048, 2049, N)


def slice_case():
    """f. B * N * 8 just over 1 GiB -> (N, B, V)"""
    return 70_000, 2000, 16


AUTO_COLS = (1, 1023, 1024, 1025, 8191, 8192, 8193, 32768, 32769, 40_000, 65_535)

POOL_L = (1, 32, 33, 64, 65, 128, 129)
POOL_CASES = [(L, B, H, V) for L in POOL_L for B, H, V in (((1, 32, 129), (3, 96, 127)) if L % 2 else ((3, 32, 1), (1, 96, 129)))] + \
             [(33, 3, 96, 1), (64, 1, 32, 127), (129, 3, 32, 127)]


# ---- matrices of the sparsity-aware build -------------------------------------------------------------------------------------------
AUTO_ROWS = 40


def auto_matrix(n_cols, seed=0, nan=False):
    """AUTO_ROWS x n_cols fp32, values k / 4 (k = 1 .. 7): first and last rows empty, an empty row inside, a full row, rows with the only
    non-zeros at column 0, at column n_cols - 1 and at both, a row with non-zeros on both sides of every column 1024 j (and so of 8192 and
    32 768), a row of -0.0 with a few non-zeros among them, random rows of ~2 % and ~30 % density.  nan: one NaN in the -0.0 row."""
    rng = np.random.default_rng(1000 + n_cols + seed)
    m = np.zeros((AUTO_ROWS, n_cols), dtype=np.float32)
    val = lambda size: rng.integers(1, 8, size=size).astype(np.float32) / 4
    m[1] = val(n_cols)                                                      # full
    m[2, 0] = 0.75
    m[3, n_cols - 1] = 1.25
    m[4, 0], m[4, n_cols - 1] = 0.5, 1.5
    edges = np.arange(1024, n_cols + 1, 1024)
    cols = np.unique(np.concatenate([edges - 1, edges[edges < n_cols]]))
    m[5, cols] = val(cols.size)
    m[6] = -0.0
    some = rng.choice(n_cols, size=min(n_cols, 5), replace=False)
    m[6, some[1:]] = val(some.size - 1)
    if nan:
        m[6, some[0]] = np.nan
    # row 7 stays empty
    for r in range(8, AUTO_ROWS - 1):
        dens = 0.3 if r % 4 == 0 else 0.02
        on = rng.random(n_cols) < dens
        m[r, on] = val(int(on.sum()))
    return m
