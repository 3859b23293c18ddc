"""DocFilter: the allowed-document set of a filtered search (``vs_index_search_filtered``, ``vs_shard_group_search_filtered``).

A filter is a bitmap over the rows of an index -- bit ``r`` (bit ``r & 31`` of word ``r >> 5``) set = row ``r`` may be returned --
either ONE bitmap for the whole batch or one per query.  The words live on a GPU as a torch ``int32`` tensor ([W] or [B, W]) and are
packed there by ``vs_filter_pack``.  A filtered search returns exactly the top-k of the allowed rows (what an unfiltered search over
the index of only those rows returns, with the full index's ids); positions beyond the allowed rows hold id -1, score -inf.

    f = DocFilter.from_mask(visible)                          # bool [N] or [B, N]
    f = DocFilter.from_ids(deleted_ids, n_rows, allow=False)  # everything but these rows
    res = index.search(q, k, filter=f)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

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
        set per query (entries < 0 are ignored there: ragged sets padded with -1).  The mask is built with torch on the device."""
        torch = _torch()
        n_rows = int(n_rows)
        if isinstance(ids, np.ndarray) or isinstance(ids, (list, tuple)):
            ids = torch.as_tensor(np.asarray(ids, dtype=np.int64))
        if not isinstance(ids, torch.Tensor) or ids.dtype.is_floating_point or ids.dtype == torch.bool or ids.dim() not in (1, 2):
            raise TypeError("DocFilter.from_ids takes integer ids [m] or [B, m]")
        dev = _device_of(device if device is not None else (ids.device if ids.is_cuda else None))
        ids = ids.to(dev).to(torch.int64)
        if ids.numel() and int(ids.max()) >= n_rows:
            raise ValueError(f"row id {int(ids.max())} is out of range for {n_rows} rows")
        if ids.dim() == 1:
            if ids.numel() and int(ids.min()) < 0:
                raise ValueError("row ids must be >= 0")
            mask = torch.zeros(n_rows, dtype=torch.bool, device=dev)
            mask[ids] = True
        else:
            mask = torch.zeros((ids.shape[0], n_rows), dtype=torch.bool, device=dev)
            r, c = (ids >= 0).nonzero(as_tuple=True)                     # only the real entries: a -1 pad writes nothing
            mask[r, ids[r, c]] = True
        return cls.from_mask(mask if allow else ~mask, device=dev)

    def to(self, device) -> "DocFilter":
        dev = _device_of(device)
        return self if self.words.device == dev else DocFilter(self.words.to(dev), self.n_rows)

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
