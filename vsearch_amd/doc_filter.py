"""DocFilter: the allowed-document set of a filtered search (``vs_index_search_filtered``, ``vs_shard_group_search_filtered``).

A filter is a bitmap over the rows of an index -- bit ``r`` (bit ``r & 31`` of word ``r >> 5``) set = row ``r`` may be returned --
either ONE bitmap for the whole batch or one per query.  The words live on a GPU as a torch ``int32`` tensor ([W] or [B, W]) and are
packed there by ``vs_filter_pack``.  A filtered search returns exactly the top-k of the allowed rows (what an unfiltered search over
the index of only those rows returns, with the full index's ids); positions beyond the allowed rows hold id -1, score -inf.

    f = DocFilter.from_mask(visible)                          # bool [N] or [B, N]
    f = DocFilter.from_ids(deleted_ids, n_rows, allow=False)  # everything but these rows
    res = index.search(q, k, filter=f)

Term constraints build the bitmap from the index's own columns on the GPU (``vs_index_term_bitmaps`` + ``vs_term_filter_combine``):

    f = DocFilter.from_terms(index, must=[c1], must_not=[c2], should=[c3, c4, c5], min_should=2)
    res = index.search(q, k, filter=visible & f)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from typing import NamedTuple

from . import _native as nat


def _torch():
    import torch
    return torch


def _device_of(device):
    torch = _torch()
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    d = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
    if d.type != "cuda":
        raise ValueError(f"a DocFilter lives on a GPU, not on {d}")
    return torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())


# ---- term programs: pure argument normalisation (no GPU, no torch) ------------------------------------------------------------------
class TermProgram(NamedTuple):
    """A must / must_not / should program in the form vs_term_filter_combine takes: `cols` the union of distinct columns in order of first
    appearance, `thr` their thresholds (NaN: none) or None, the lists as indices into `cols` ([B, n], padded with -1; B = 1 for a program
    shared by the batch), `min_should` [B], and whether the program is one per query."""
    cols: np.ndarray          # int32 [T]
    thr: object               # float32 [T] or None
    must: np.ndarray          # int32 [B, n_must]
    must_not: np.ndarray      # int32 [B, n_must_not]
    should: np.ndarray        # int32 [B, n_should]
    min_should: np.ndarray    # int32 [B]
    per_query: bool


def _is_seq(x) -> bool:
    return isinstance(x, (list, tuple, np.ndarray)) or type(x).__module__.startswith("torch")


def _as_column(x, name) -> int:
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
        if type(x).__module__.startswith("torch") and getattr(x, "ndim", 1) == 0 and not x.is_floating_point() and str(x.dtype) != "torch.bool":
            x = int(x)
        else:
            raise TypeError(f"{name}: a term is an integer column id, got {type(x).__name__} {x!r}")
    x = int(x)
    if x < 0:
        raise ValueError(f"{name}: column id {x} is negative")
    return x


def _term_lists(x, name):
    """one list argument -> (list of per-query lists of ints, per_query)"""
    if x is None:
        return [[]], False
    if not _is_seq(x):
        raise TypeError(f"{name}: a sequence of column ids, or one sequence per query; got {type(x).__name__}")
    items = list(x)
    nested = [_is_seq(it) and getattr(it, "ndim", 1) != 0 for it in items]
    if items and all(nested):
        return [[_as_column(c, name) for c in it] for it in items], True
    if any(nested):
        raise TypeError(f"{name}: either column ids, or one sequence per query -- not a mix of both")
    return [[_as_column(c, name) for c in items]], False


def normalize_terms(must=None, must_not=None, should=None, min_should=None, thr=None, max_list: int = nat.TERM_FILTER_LIST,
                    max_terms: int = nat.TERM_FILTER_TERMS) -> TermProgram:
    """The arguments of DocFilter.from_terms -> a TermProgram.  Each list: None, a flat sequence of column ids (the same for every query)
    or a list of B sequences (one per query, ragged).  Duplicate terms collapse -- inside a list, and across lists to one slot of the
    union.  min_should: None (1 for a query whose should list is non-empty, else 0), an int, or B ints.  thr: {column: threshold}.
    Raises TypeError / ValueError for non-integer or negative terms, lists of different batch sizes, a list of more than `max_list` terms, more
    than `max_terms` distinct terms, a negative min_should."""
    parsed = {}
    B = None
    for name, x in (("must", must), ("must_not", must_not), ("should", should)):
        lists, per = _term_lists(x, name)
        parsed[name] = (lists, per)
        if per:
            if B is not None and B != len(lists):
                raise ValueError(f"{name} holds lists for {len(lists)} queries, another list for {B}")
            B = len(lists)
    ms_seq = None
    if min_should is not None:
        if _is_seq(min_should) and getattr(min_should, "ndim", 1) != 0:
            ms_seq = [m for m in min_should]
            if B is not None and B != len(ms_seq):
                raise ValueError(f"min_should holds {len(ms_seq)} entries, the lists are for {B} queries")
            B = len(ms_seq)
        else:
            ms_seq = None
        for m in (ms_seq if ms_seq is not None else [min_should]):
            if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)):
                raise TypeError(f"min_should must be an int, got {type(m).__name__}")
            if int(m) < 0:
                raise ValueError(f"min_should must be >= 0, got {int(m)}")
    per_query = B is not None
    if B == 0:
        raise ValueError("per-query lists for zero queries")
    B = B or 1
    if thr is not None and not isinstance(thr, dict):
        raise TypeError("thr: a dict {column: threshold}")
    slot = {}
    out = {}
    for name in ("must", "must_not", "should"):
        lists, per = parsed[name]
        rows = []
        for b in range(B):
            seen = []
            for c in (lists[b] if per else lists[0]):
                if c not in slot:
                    slot[c] = len(slot)
                if slot[c] not in seen:
                    seen.append(slot[c])
            if len(seen) > max_list:
                raise ValueError(f"{name}: {len(seen)} terms for query {b}, at most {max_list}")
            rows.append(seen)
        width = max(len(r) for r in rows)
        arr = np.full((B, width), -1, dtype=np.int32)
        for b, r in enumerate(rows):
            arr[b, :len(r)] = r
        out[name] = arr
    if len(slot) > max_terms:
        raise ValueError(f"{len(slot)} distinct terms, at most {max_terms} a filter")
    cols = np.array(list(slot), dtype=np.int64)
    if cols.size and int(cols.max()) > 0x7FFFFFFF:
        raise ValueError(f"column id {int(cols.max())} is not a column of an index")
    n_should = (out["should"] >= 0).sum(axis=1)
    if min_should is None:
        ms = (n_should > 0).astype(np.int32)
    elif ms_seq is not None:
        ms = np.array([int(m) for m in ms_seq], dtype=np.int32)
    else:
        ms = np.full(B, int(min_should), dtype=np.int32)
    t = None
    if thr:
        t = np.array([float(thr.get(int(c), np.nan)) for c in cols], dtype=np.float32)
        if bool(np.isnan(t).all()):
            t = None
    return TermProgram(cols.astype(np.int32), t, out["must"], out["must_not"], out["should"], np.minimum(ms, max_list + 1).astype(np.int32), per_query)


def terms_to_columns(terms, vocab, shift: int, name: str = "terms"):
    """Terms given as column ids or vocabulary tokens (strings) -> column ids; nesting (one list per query) is kept.  A string is looked up in
    `vocab` (the tokenizer's token -> id mapping); its column is token id - shift.  A string that is not one vocabulary entry, or whose id
    is below the shift, raises ValueError naming it."""
    if terms is None:
        return None
    if isinstance(terms, str):
        terms = [terms]
    def one(t):
        if isinstance(t, str):
            tid = vocab.get(t) if hasattr(vocab, "get") else None
            if tid is None:
                raise ValueError(f"{name}: {t!r} is not one entry of the vocabulary (pass the word pieces of a longer word one by one)")
            if int(tid) < int(shift):
                raise ValueError(f"{name}: {t!r} (token id {int(tid)}) lies below the vocabulary shift {int(shift)}: the index has no column for it")
            return int(tid) - int(shift)
        return t
    return [[one(t) for t in it] if (_is_seq(it) and getattr(it, "ndim", 1) != 0) else one(it) for it in terms]


class DocFilter:
    """Packed allowed-row bitmap(s) of an index of `n_rows` rows: `words` is int32 [W] (shared by the batch) or [B, W] (one per query),
    W = ceil(n_rows / 32), on a GPU."""

    def __init__(self, words, n_rows: int):
        torch = _torch()
        if not isinstance(words, torch.Tensor) or words.dtype != torch.int32 or words.dim() not in (1, 2) or not words.is_cuda:
            raise TypeError("DocFilter words: an int32 CUDA tensor [W] or [B, W]")
        n_rows = int(n_rows)
        if n_rows <= 0 or words.shape[-1] != (n_rows + 31) // 32:
            raise ValueError(f"DocFilter: {words.shape[-1]} words do not hold {n_rows} rows")
        self.words = words.contiguous()
        self.n_rows = n_rows

    @property
    def per_query(self) -> bool:
        return self.words.dim() == 2

    @property
    def n_queries(self):
        """queries of a per-query filter (None: one bitmap for any batch)"""
        return int(self.words.shape[0]) if self.per_query else None

    @property
    def ld(self) -> int:
        """words between two queries' bitmaps (the C ABI's filter_ld): 0 for a shared filter"""
        return int(self.words.shape[1]) if self.per_query else 0

    @property
    def device(self):
        return self.words.device

    # ---- construction --------------------------------------------------------------------------------
    @classmethod
    def from_mask(cls, mask, device=None) -> "DocFilter":
        """bool [N] (one set for the batch) or [B, N] (one per query) tensor or ndarray; True = allowed."""
        torch = _torch()
        if isinstance(mask, np.ndarray):
            mask = torch.from_numpy(np.ascontiguousarray(mask))
        if not isinstance(mask, torch.Tensor) or mask.dim() not in (1, 2):
            raise TypeError("DocFilter.from_mask takes a bool tensor / ndarray [N] or [B, N]")
        if mask.dtype != torch.bool:
            raise TypeError(f"DocFilter.from_mask takes a bool mask, not {mask.dtype} (integer ids: DocFilter.from_ids)")
        dev = _device_of(device if device is not None else (mask.device if mask.is_cuda else None))
        m = mask.to(dev).to(torch.uint8).contiguous()
        n = int(m.shape[-1])
        if n <= 0:
            raise ValueError("an empty mask: the index has rows")
        B = int(m.shape[0]) if m.dim() == 2 else 1
        nw = (n + 31) // 32
        words = torch.empty((B, nw) if m.dim() == 2 else (nw,), dtype=torch.int32, device=dev)
        from .device_index import current_stream
        nat.require_device()
        nat.check(nat.lib().vs_filter_pack(C.c_void_p(m.data_ptr()), B, n, n, C.c_void_p(words.data_ptr()), nw, dev.index,
                                           current_stream(dev.index)))
        return cls(words, n)

    @classmethod
    def from_ids(cls, ids, n_rows: int, allow: bool = True, device=None) -> "DocFilter":
        """Row ids to allow (allow=True) or to exclude (allow=False): a 1-D tensor / ndarray / list for the whole batch, or [B, m] for one
        set per query (entries < 0 are ignored there: ragged sets padded with -1).  The ids are scattered into the packed words on the GPU
        (vs_set_from_ids): no [B, N] mask is formed."""
        torch = _torch()
        n_rows = int(n_rows)
        if n_rows <= 0:
            raise ValueError("no rows: the index has rows")
        if isinstance(ids, np.ndarray) or isinstance(ids, (list, tuple)):
            ids = torch.as_tensor(np.asarray(ids, dtype=np.int64))
        if not isinstance(ids, torch.Tensor) or ids.dtype.is_floating_point or ids.dtype == torch.bool or ids.dim() not in (1, 2):
            raise TypeError("DocFilter.from_ids takes integer ids [m] or [B, m]")
        dev = _device_of(device if device is not None else (ids.device if ids.is_cuda else None))
        ids = ids.to(dev).to(torch.int64)
        if ids.numel() and int(ids.max()) >= n_rows:
            raise ValueError(f"row id {int(ids.max())} is out of range for {n_rows} rows")
        if ids.dim() == 1 and ids.numel() and int(ids.min()) < 0:
            raise ValueError("row ids must be >= 0")
        if ids.dim() == 2 and int(ids.shape[0]) < 1:
            raise ValueError("id sets for zero queries")
        from .device_index import set_from_ids
        nat.require_device()
        with torch.cuda.device(dev):
            words = set_from_ids(ids.reshape(1, -1) if ids.dim() == 1 else ids, n_rows, allow=allow, device=dev.index)
        return cls(words[0] if ids.dim() == 1 else words, n_rows)

    @classmethod
    def from_terms(cls, index, must=None, must_not=None, should=None, min_should=None, thr=None) -> "DocFilter":
        """The rows of `index` that have every `must` term, no `must_not` term and at least `min_should` of the `should` terms (default 1
        when `should` is given).  A row has term c -- a column id -- iff it stores column c with a non-zero value; with thr = {c: t}, iff
        the stored value is >= t.  Each list is a flat sequence of column ids (one program for the batch) or a list of B sequences (one per
        query, ragged).  index: a DeviceIndex, a ShardGroup, or a facade Index (columns in its vector's space).  The union of the distinct
        terms is scanned once on the GPU (vs_index_term_bitmaps), then combined (vs_term_filter_combine); deleted rows are not special
        here -- every search ANDs the live rows itself."""
        prog = normalize_terms(must, must_not, should, min_should, thr)
        target = index._explain_target()[0] if hasattr(index, "_explain_target") else index
        if not hasattr(target, "_term_words"):
            raise TypeError(f"DocFilter.from_terms takes a DeviceIndex, a ShardGroup or an Index, not {type(index).__name__}")
        torch = _torch()
        from .device_index import current_stream
        n = int(target.n_rows)
        if n <= 0:
            raise ValueError("the index has no rows")
        nat.require_device()
        dev = torch.device("cuda", int(target.device))
        W = (n + 31) // 32
        T = int(prog.cols.shape[0])
        ld = (W + 3) // 4 * 4
        terms = target._term_words(prog.cols, prog.thr, ld=ld)[0] if T else None
        B = int(prog.min_should.shape[0])
        lists = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a.shape[1] else None for a in (prog.must, prog.must_not, prog.should)]
        ms = torch.from_numpy(prog.min_should).to(dev)
        words = torch.empty((B, W), dtype=torch.int32, device=dev)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        nat.check(nat.lib().vs_term_filter_combine(ptr(terms), ld, n, T, ptr(lists[0]), int(prog.must.shape[1]), ptr(lists[1]), int(prog.must_not.shape[1]),
                                                   ptr(lists[2]), int(prog.should.shape[1]), ptr(ms), B, ptr(words), W, dev.index,
                                                   current_stream(dev.index)))
        return cls(words if prog.per_query else words[0], n)

    @classmethod
    def from_labels(cls, labels, values, device=None) -> "DocFilter":
        """The rows whose label equals a value: `labels` an int array / tensor [N] (facet codes, cluster labels of ``assign``), `values` an
        int (one set for the batch) or a sequence of B ints (one set per query, at most 4096) -> row r is allowed for query b iff
        labels[r] == values[b].  Built in one pass over the labels on the GPU (vs_label_bitmaps); a value no row carries gives an empty
        set.  The drill-down filter of a facet field, and the K cluster sets ``term_sums`` takes."""
        torch = _torch()
        from .device_index import _label_values, current_stream
        vals, scalar = _label_values(values)
        if isinstance(labels, (np.ndarray, list, tuple)):
            labels = torch.from_numpy(np.ascontiguousarray(np.asarray(labels)))
        if not isinstance(labels, torch.Tensor) or labels.dim() != 1:
            raise TypeError("DocFilter.from_labels takes an integer tensor / ndarray [N]")
        if labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
            raise TypeError(f"DocFilter.from_labels takes integer labels, not {labels.dtype}")
        n = int(labels.shape[0])
        if n <= 0:
            raise ValueError("no labels: the index has rows")
        dev = _device_of(device if device is not None else (labels.device if labels.is_cuda else None))
        nat.require_device()
        lab = labels.detach().to(dev)
        if lab.dtype != torch.int32:
            if lab.dtype == torch.int64 and n and (int(lab.min()) < -0x80000000 or int(lab.max()) > 0x7FFFFFFF):
                raise ValueError("a label does not fit 32 bits")
            lab = lab.to(torch.int32)
        lab = lab.contiguous()
        B, nw = int(vals.shape[0]), (n + 31) // 32
        v = torch.from_numpy(vals).to(dev)
        words = torch.empty((B, nw), dtype=torch.int32, device=dev)
        nat.check(nat.lib().vs_label_bitmaps(C.c_void_p(lab.data_ptr()), n, C.c_void_p(v.data_ptr()), B, 0, C.c_void_p(words.data_ptr()), nw,
                                             dev.index, current_stream(dev.index)))
        return cls(words[0] if scalar else words, n)

    @classmethod
    def from_values(cls, values, lo=None, hi=None, device=None) -> "DocFilter":
        """The rows whose value lies in a range: `values` a float32 / int32 array / tensor [N] (NaN / INT32_MIN = the row has no value;
        ``device_index.value_column`` converts other types), `lo` / `hi` numbers (one set for the batch) or sequences of B of them (one set
        per query, at most 4096); None is an open end -> row r is allowed for query b iff it has a value and lo[b] <= values[r] <= hi[b].
        Built in one pass over the values on the GPU (vs_value_range_bitmaps); lo > hi gives an empty set."""
        torch = _torch()
        from .device_index import _value_bounds, _value_dtype, value_range_bitmaps
        if isinstance(values, np.ndarray):
            values = torch.from_numpy(np.ascontiguousarray(values))
        if not isinstance(values, torch.Tensor) or values.dim() != 1 or int(values.shape[0]) < 1:
            raise TypeError("DocFilter.from_values takes a non-empty float32 / int32 tensor / ndarray [N]")
        _, _, scalar = _value_bounds(lo, hi, _value_dtype(values))
        dev = _device_of(device if device is not None else (values.device if values.is_cuda else None))
        nat.require_device()
        words = value_range_bitmaps(values.detach().to(dev).contiguous(), lo, hi, device=dev.index)
        return cls(words[0] if scalar else words, int(values.shape[0]))

    # ---- set algebra on the packed words --------------------------------------------------------------
    def _pair(self, other):
        if not isinstance(other, DocFilter):
            return None
        if other.n_rows != self.n_rows:
            raise ValueError(f"filters over {self.n_rows} and {other.n_rows} rows do not combine")
        if self.per_query and other.per_query and self.n_queries != other.n_queries:
            raise ValueError(f"per-query filters for {self.n_queries} and {other.n_queries} queries do not combine")
        return self.words, other.words.to(self.words.device)         # (a shared filter [W] broadcasts against a per-query one [B, W])

    def __and__(self, other):
        p = self._pair(other)
        return NotImplemented if p is None else DocFilter(p[0] & p[1], self.n_rows)

    def __or__(self, other):
        p = self._pair(other)
        return NotImplemented if p is None else DocFilter(p[0] | p[1], self.n_rows)

    def __invert__(self):
        w = ~self.words
        if self.n_rows & 31:                                         # the bits past n_rows stay 0
            w[..., -1] &= (1 << (self.n_rows & 31)) - 1
        return DocFilter(w, self.n_rows)

    def to(self, device) -> "DocFilter":
        dev = _device_of(device)
        return self if self.words.device == dev else DocFilter(self.words.to(dev), self.n_rows)

    # ---- the way out: count, list, page and sample the set (vs_set_count / vs_set_ids / vs_set_sample) ------------------------------------------
    # These read the bitmap as it is: an index's deleted rows are taken out by DeviceIndex.set_ids / Index.list_ids, not here.
    def count(self):
        """The number of rows in the set -> int64 tensor [B] on the filter's GPU (B = 1 for a shared filter)."""
        from .device_index import _doc_filter_count
        return _doc_filter_count(self)

    def ids(self, offset=0, limit=None):
        """The rows of the set in ascending order -> SetIds(ids int64 [B, limit], counts int64 [B]): ranks [offset, offset + limit) of each
        query's list, -1 behind its last member; counts is the full size whatever the window.  offset: an int or one per query.  limit=None
        takes the largest count, which costs one count round first.  B x limit <= 2^27: ``pages`` walks a longer list."""
        from .device_index import _doc_filter_ids
        return _doc_filter_ids(self, offset, limit)

    def pages(self, page_size: int):
        """The whole list in pages of `page_size` ids: a generator of SetIds, until every query's list is exhausted (at least one page)."""
        if isinstance(page_size, bool) or not isinstance(page_size, (int, np.integer)) or page_size < 1:
            raise ValueError(f"page_size must be a positive int, got {page_size!r}")
        offset = 0
        while True:
            page = self.ids(offset, int(page_size))
            yield page
            offset += int(page_size)
            if offset >= int(page.counts.max()):
                return

    def sample(self, n: int, seed: int = 0):
        """n rows of the set, uniformly and without replacement -> SetSample(ids int64 [B, n], counts int64 [B]): query b's n rows with the
        smallest (hash(seed + b, row), row), in that order; -1 behind the last when the set holds fewer.  Reproducible under the seed.
        n in 1..1024."""
        from .device_index import _doc_filter_sample
        return _doc_filter_sample(self, n, seed)

    def __repr__(self):
        kind = f"per-query x {self.n_queries}" if self.per_query else "shared"
        return f"DocFilter({self.n_rows} rows, {kind}, {self.words.device})"


def as_doc_filter(filter, n_rows: int, device=None, batch=None) -> DocFilter:
    """`filter=` of the search entry points -> a DocFilter on `device`: a DocFilter, a bool mask [N] / [B, N], or integer ids to allow.
    A mask / filter whose row count is not the index's, or a per-query filter for another batch size, raises ValueError."""
    torch = _torch()
    if isinstance(filter, DocFilter):
        f = filter
    else:
        if isinstance(filter, (list, tuple)):
            filter = np.asarray(filter)
        is_bool = (isinstance(filter, np.ndarray) and filter.dtype == np.bool_) or (isinstance(filter, torch.Tensor) and filter.dtype == torch.bool)
        if is_bool:
            if filter.shape[-1] != n_rows:
                raise ValueError(f"filter mask has {filter.shape[-1]} rows, the index has {n_rows}")
            f = DocFilter.from_mask(filter, device=device)
        elif isinstance(filter, (np.ndarray, torch.Tensor)):
            f = DocFilter.from_ids(filter, n_rows, device=device)
        else:
            raise TypeError(f"filter: a DocFilter, a bool mask or integer row ids, not {type(filter).__name__}")
    if f.n_rows != n_rows:
        raise ValueError(f"filter covers {f.n_rows} rows, the index has {n_rows}")
    if batch is not None and f.per_query and f.n_queries != int(batch):
        raise ValueError(f"per-query filter for {f.n_queries} queries, the batch has {batch}")
    return f.to(device) if device is not None else f
