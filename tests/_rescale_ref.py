"""numpy reference of the reweighted index (vs_index_row_stats, vs_index_rescale; the arithmetic is pinned in include/vsearch_hip.h).

A CSR is (indptr, indices, data): row r holds the cells indptr[r]:indptr[r + 1] in STORED order, data float32 (an fp16 store widened exactly),
or None for a binary index (every cell holds 1).  Plain loops: the lane / packet / butterfly order of the sums is written out, nothing is
vectorised across cells."""
import numpy as np

LANES = 64            # lanes of the wave that sums a row
CELLS = 8             # cells of a packet
NO_VALUE = np.uint32(0x7FC00000)


def _butterfly(lane_sums):
    """the xor butterfly o = 32 .. 1 over 64 float64 lane sums -> the value every lane ends with"""
    s = np.array(lane_sums, dtype=np.float64)
    o = LANES // 2
    while o > 0:
        s = np.array([s[l] + s[l ^ o] for l in range(LANES)], dtype=np.float64)
        o //= 2
    return s[0]


def row_stats_ref(indptr, data, n_rows=None):
    """-> (cells int32, nonzero int32, l1 float64, sumsq float64, max float32) per row, in the pinned order: lane l adds the cells of the row's
    packets l, l + 64, ... (packet j = cells 8j .. 8j + 7 of the row) one by one from +0.0, then the butterfly"""
    indptr = np.asarray(indptr, dtype=np.int64)
    n = len(indptr) - 1 if n_rows is None else n_rows
    cells = np.zeros(n, np.int32)
    nonzero = np.zeros(n, np.int32)
    l1 = np.zeros(n, np.float64)
    sumsq = np.zeros(n, np.float64)
    mx = np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        for r in range(n):
            a, b = int(indptr[r]), int(indptr[r + 1])
            w = np.ones(b - a, np.float32) if data is None else np.asarray(data[a:b], dtype=np.float32)
            cells[r] = b - a
            nonzero[r] = int(np.count_nonzero(w != 0))
            lane_l1 = [np.float64(0.0)] * LANES
            lane_sq = [np.float64(0.0)] * LANES
            n_packets = (b - a + CELLS - 1) // CELLS
            for j in range(n_packets):
                lane = j % LANES
                for t in range(j * CELLS, min((j + 1) * CELLS, b - a)):
                    x = np.float64(w[t])
                    lane_l1[lane] = lane_l1[lane] + np.abs(x)
                    lane_sq[lane] = lane_sq[lane] + x * x
            l1[r] = _butterfly(lane_l1)
            sumsq[r] = _butterfly(lane_sq)
            ok = w[~np.isnan(w)]
            if ok.size == 0:
                mx[r] = NO_VALUE.view(np.float32)
            else:
                m = np.float32(ok.max())
                mx[r] = np.float32(0.0) if m == 0 else m          # a zero maximum is +0.0
    return cells, nonzero, l1, sumsq, mx


def rescale_ref(indptr, indices, data, row_scale=None, col_scale=None, out="fp32"):
    """-> the new values as float32 (an fp16 result widened exactly): float64 products left to right, a None scale skipped, rounded once to
    float32 and then, for out = "fp16", to float16.  data None: a binary source, 1 in every cell.  With no scale and the same dtype numpy's
    casts are the identity on the bits, NaN payloads aside."""
    indptr = np.asarray(indptr, dtype=np.int64)
    nnz = int(indptr[-1])
    w = np.ones(nnz, np.float32) if data is None else np.asarray(data, dtype=np.float32)
    x = w.astype(np.float64)
    with np.errstate(all="ignore"):
        if row_scale is not None:
            rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
            x = x * np.asarray(row_scale, dtype=np.float32).astype(np.float64)[rows]
        if col_scale is not None:
            x = x * np.asarray(col_scale, dtype=np.float32).astype(np.float64)[np.asarray(indices, dtype=np.int64)]
        y = x.astype(np.float32)
        if out == "fp16":
            y = y.astype(np.float16).astype(np.float32)
    return y


def same_values(got, want):
    """value bits equal; where the reference holds a NaN any NaN will do"""
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def same_f64(got, want):
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return bool(got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]))
