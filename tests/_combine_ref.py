"""numpy reference of the combined index (vs_index_combine; the semantics are pinned in include/vsearch_hip.h).

A CSR is (indptr, indices, data): row r holds the cells indptr[r]:indptr[r + 1] in STORED order (any order), data float32 (an fp16 store
widened exactly), or None for a binary index (every cell holds 1).  A plain loop over the rows and the cells: nothing is vectorised."""
import numpy as np


class RepeatedColumn(ValueError):
    """a source row stores one column twice: .source is "a" or "b", .row the lowest such row (a before b at the same row)"""

    def __init__(self, source, row):
        super().__init__(f"row {row} of index {source} stores a column twice")
        self.source, self.row = source, row


def _row(indptr, indices, data, r):
    a, b = int(indptr[r]), int(indptr[r + 1])
    cols = [int(c) for c in indices[a:b]]
    vals = [np.float32(1.0)] * (b - a) if data is None else [np.float32(v) for v in data[a:b]]
    return cols, vals


def combine_ref(csr_a, csr_b, wa=1.0, wb=1.0, out="fp32"):
    """-> (indptr int64, indices int64, values float32 -- an fp16 result widened exactly).  Result row r: the columns either source row stores,
    each once, ascending; a column in both rows holds fl32(fp64(wa) * fp64(a) + fp64(wb) * fp64(b)), a column in one row fl32 of the one
    product; out = "fp16" rounds that float32 to float16.  A stored zero is a cell; a sum that cancels stays a cell.  Raises RepeatedColumn for
    the lowest row that stores a column twice."""
    n = len(csr_a[0]) - 1
    assert len(csr_b[0]) - 1 == n, "the sources have the same rows"
    wa64, wb64 = np.float64(np.float32(wa)), np.float64(np.float32(wb))
    indptr, indices, values = [0], [], []
    rows = []
    for r in range(n):                                  # repeats first: the lowest row over both sources is the one named
        ca, va = _row(*csr_a, r)
        cb, vb = _row(*csr_b, r)
        if len(set(ca)) != len(ca):
            raise RepeatedColumn("a", r)
        if len(set(cb)) != len(cb):
            raise RepeatedColumn("b", r)
        rows.append((dict(zip(ca, va)), dict(zip(cb, vb))))
    with np.errstate(all="ignore"):
        for da, db in rows:
            for c in sorted(set(da) | set(db)):
                if c in da and c in db:
                    x = wa64 * np.float64(da[c]) + wb64 * np.float64(db[c])
                elif c in da:
                    x = wa64 * np.float64(da[c])
                else:
                    x = wb64 * np.float64(db[c])
                y = np.float32(x)
                if out == "fp16":
                    y = np.float32(np.float16(y))
                indices.append(c)
                values.append(y)
            indptr.append(len(indices))
    return np.array(indptr, np.int64), np.array(indices, np.int64), np.array(values, np.float32)


def same_values(got, want):
    """value bits equal; where the reference holds a NaN any NaN will do"""
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def same_csr(got, want):
    return bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_values(got[2], want[2]))
