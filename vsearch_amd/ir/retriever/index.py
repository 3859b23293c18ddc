"""Index containers with the reference's interface (/root/reference/src/ir/retriever/index.py:16-218),
backed by the device-resident formats of libvsearch_hip.so.

Same names, constructor arguments and return conventions as ``src.ir.retriever.index``:
``Index`` (dense), ``SparseIndex`` (CSR), ``BoTIndex`` (binary bag-of-token CSR), ``SearchResults``,
``IndexType``.  Differences, all supersets:
  * ``search`` never materialises the [B, N] score matrix; ties are ordered (score desc, id asc);
  * compute always runs on an MI355X: an index whose ``device`` is "cpu" keeps its API tensors on
    the host but is searched on GPU 0 (there is no CPU fallback -- without a GPU it raises);
  * loading a dense index from ``.pt`` shards and ``low_memory=True`` work (broken upstream);
  * ``fp16=True`` is applied on the device (scipy >= 1.15 cannot ``astype(float16)`` a sparse array).
"""
from __future__ import annotations

import copy
import glob
import json
import logging
from enum import Enum
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from ... import _native as nat
from ...device_index import Assignment, KMeansResult, KMEANS_UPDATE_BATCH, kmeans_loop, term_sum_topn, _assign_args, _kmeans_args, DeviceIndex, DiverseResults, Explanation, FacetCounts, FusedResults, GroupedResults, TermCounts, TermSums, TopFacets, TopTerms, TopWeights, _term_topn_args, _weight_topn_args, fuse_topk, _fuse_args, MAX_FUSE_DEPTH, MAX_FUSE_ENTRIES, _topn_args, NotBinaryError, RangeResults, ShardGroup, _diverse_args, _range_args, _grouped_args, _by_example_args, _explain_args, _int64_ids, _k_a_args, resparsify, topk_exclude
from ...device_index import SortedResults, ValueHistogram, ValueStats, value_column, _value_bounds, _value_dtype, _value_edges, _value_topk_args
from ...device_index import ValuePercentiles, _percentile_args, quantile_lerp
from ...device_index import FacetValueHistogram, FacetValueStats
from ...device_index import FacetValuePercentiles, MAX_VALUE_RANKS
from ...device_index import SetIds, SetSample, _set_sample_args, _set_window_args, MAX_SET_IDS
from ...device_index import _select_ids, _value_keys
from ...device_index import RowStats, _rescale_dtype, _combine_dtype
from ...device_index import CONCAT_MAX_SOURCES, _concat_dtype
from ...device_index import BOOST_MODES, MAX_BOOST_FIELDS
from ...device_index import _col_mask
from ...device_index import LabelTermCounts, LabelTermSums, _label_top_terms, _label_top_weights

logger = logging.getLogger(__name__)


class _ScoreField:
    """the type of ``SCORE``"""
    __slots__ = ()

    def __repr__(self):
        return "SCORE"


# Pass as `field` / `value_field` of value_stats, histogram, percentiles, median, top_by_value, stats_by_facet and histogram_by_facet to describe
# a document set by its SCORES instead of a stored field.  An object of its own, not a reserved name: set_values("_score", ...) is a field like any.
SCORE = _ScoreField()
SCORE_SCRATCH_BYTES = 1 << 30                                        # the [Bt, N] float32 block of scores a SCORE call keeps at a time


class SearchResults(NamedTuple):
    ids: List[int]
    scores: List[float]


class IndexType(Enum):
    DENSE = "dense"
    SPARSE = "sparse"
    BAG_OF_TOKEN = "bag_of_token"


def _resolve_devices(devices):
    """`devices` of SparseIndex / BoTIndex / Retriever.load_index -> list of GPU ordinals to shard over, or None (one device).
    None: the index lives on `device` (the reference's behaviour); "all": every visible GPU; an int n: GPUs 0 .. n-1; a list."""
    if devices is None:
        return None
    if isinstance(devices, str):
        if devices != "all":
            raise ValueError('devices: None, "all", a count or a list of GPU ordinals')
        devices = torch.cuda.device_count()
    if isinstance(devices, int):
        devices = list(range(devices))
    out = [_gpu_ordinal(d) if not isinstance(d, int) else int(d) for d in devices]
    return out if len(out) > 1 else None


def _gpu_ordinal(device) -> int:
    d = torch.device(device) if not isinstance(device, torch.device) else device
    if d.type == "cuda":
        return d.index if d.index is not None else torch.cuda.current_device()
    return 0


def remap_text_store(data, offsets, old_ids):
    """The text store after a compaction: entry j of the result is entry old_ids[j] of the input, for the in-memory list (`data`) and for
    the line offsets of a low_memory store (`offsets`); either may be None.  Pure host work."""
    old = [int(i) for i in old_ids]
    new_data = [data[i] for i in old] if data is not None else None
    new_offsets = [offsets[i] for i in old] if offsets is not None else None
    return new_data, new_offsets


def _packets_of(indptr) -> int:
    """8-nnz packets the CSR rows of `indptr` take in the device format"""
    ip = indptr.cpu().numpy() if isinstance(indptr, torch.Tensor) else np.asarray(indptr)
    return int(((np.diff(ip.astype(np.int64)) + 7) // 8).sum())


def fuse_results(results_list, k: int, method: str = "rrf", weights=None, c: float = 60.0) -> FusedResults:
    """``Index.search_fused``'s fusion over hit lists already at hand: `results_list` holds L SearchResults (or (ids [B, kk_l], scores)
    pairs, kk_l <= 1024 and their sum <= 4096 a query) -- a reranked list next to the first-stage one, lists of different indexes.  Shorter
    lists are padded; a list ends at its first id -1.  The result lives where the first list lives (host lists: numpy arrays)."""
    lists = [(r[0], r[1]) for r in results_list]
    _fuse_args(k, method, c, None, len(lists))
    first = lists[0][0]
    on_dev = isinstance(first, torch.Tensor) and first.is_cuda
    if on_dev:
        lists = [(i, s.float()) for i, s in lists]
    else:
        lists = [(i.cpu() if isinstance(i, torch.Tensor) else i, s.float().cpu() if isinstance(s, torch.Tensor) else s) for i, s in lists]
    return fuse_topk(lists, None, int(k), method, weights, c, device=first.device.index or 0 if on_dev else 0)


class Index:
    index_type = IndexType.DENSE
    DENSE_AS_CSR_DENSITY = 0.05        # set to 0 to always use the dense (MFMA) search kernel

    def __init__(self, index_file: Optional[str] = None, data_file: Optional[str] = None, fp16: bool = True,
                 device: str = "cpu", low_memory: bool = False):
        self.data = None
        self.low_memory = low_memory
        self.device = device
        self._vector = None            # torch view of the index (dense tensor / sparse CSR tensor), lazily exported
        self._dev: Optional[DeviceIndex] = None
        self._dtype = torch.float32    # dtype the reference would report for `vector` (scores are returned in it)
        self._shape = None
        self.init_index(index_file, fp16)
        self.load_data(data_file)

    # ---- the `vector` attribute of the reference: assignable and readable ----------------------
    @property
    def vector(self):
        if self._vector is None and self._dev is not None:
            self._vector = self._export_vector()
        return self._vector

    @vector.setter
    def vector(self, value):
        self._drop_device()
        if value is not None and not isinstance(value, torch.Tensor):      # scipy CSR
            value = torch.sparse_csr_tensor(torch.from_numpy(value.indptr), torch.from_numpy(value.indices),
                                            torch.from_numpy(value.data), size=value.shape)
        self._vector = value
        if value is not None:
            self._dtype = value.dtype
            self._shape = tuple(value.shape)

    def _drop_device(self):
        if self._dev is not None:
            self._dev.close()
        self._dev = None

    def adopt_device_index(self, dev: DeviceIndex, dtype=torch.float32, device: Optional[str] = None):
        """Take ownership of an index already built in HBM (Retriever.build_index emits the CSR per batch straight into the
        device format): `vector` is exported from it on demand."""
        self._drop_device()
        info = dev.info()
        self._vector = None
        self._dev = dev
        self._dtype = dtype
        self._shape = (int(info.n_rows), int(info.n_cols))
        self.device = device or f"cuda:{info.device}"
        self._prepare()

    def _export_vector(self):
        mat = self._dev.export_dense(np.float16 if self._dtype == torch.float16 else np.float32)
        return torch.from_numpy(mat).to(self.device)

    def _build_device_index(self) -> DeviceIndex:
        v = self._vector
        if v is None:
            raise RuntimeError("index is empty: no vector to search")
        if v.layout != torch.strided:
            raise TypeError(f"{type(self).__name__} expects a dense tensor, got layout {v.layout}")
        if v.dtype not in (torch.float32, torch.float16):
            v = v.float()
        store = nat.VS_F16 if v.dtype == torch.float16 else nat.VS_F32
        # a dense index of VDR embeddings is > 97 % zeros: below DENSE_AS_CSR_DENSITY it is stored as CSR packets
        return DeviceIndex.from_dense(v.contiguous(), store_dtype=store, device=_gpu_ordinal(self.device),
                                      max_density=self.DENSE_AS_CSR_DENSITY)

    # The column-grouped copy sparse queries are searched on is built when the index reaches the device (move_to_device, load_index,
    # build_index) -- 0.5 s at 21 M docs that would otherwise sit inside a user's first retrieve().
    EAGER_POSTINGS = True

    def _prepare(self):
        if self._dev is not None and self.EAGER_POSTINGS:
            self._dev.prepare()

    def _device_index(self) -> DeviceIndex:
        if self._dev is None:
            self._dev = self._build_device_index()
            self._prepare()
        return self._dev

    # ---- loading -------------------------------------------------------------------------------
    def init_index(self, index_path: Optional[str], fp16: bool = True):
        if not index_path:
            return
        files = sorted(glob.glob(index_path))
        if not files:
            raise FileNotFoundError(f"no index file matches {index_path!r}")
        logger.info("***** Loading %s Index from %d files *****", self.index_type.value, len(files))
        shards = [torch.load(f, map_location="cpu") for f in files]
        vector = torch.cat(shards, dim=0) if len(shards) > 1 else shards[0]
        self.vector = vector.to(torch.float16) if fp16 else vector
        self.move_to_device(self.device)

    def load_data(self, data_file: Optional[str]):
        if not data_file:
            return
        if not self.low_memory:
            with open(data_file, "r") as fh:
                self.data = [json.loads(line) for line in fh]
        else:
            self.data_file = data_file
            self.offsets = self._calculate_offsets(data_file)

    def move_to_device(self, device: str):
        logger.info("Moving index to %s.", device)
        if self._vector is not None:
            self._vector = self._vector.to(device)
        same_gpu = self._dev is not None and self._dev.device == _gpu_ordinal(device)
        if not same_gpu and self._dev is not None and self._dev.n_live != self._dev.n_rows:
            raise RuntimeError("the index has deleted rows, which a move to another device would resurrect: compact() first")
        if not same_gpu:
            if self._vector is None and self._dev is not None:
                self._vector = self._export_vector()
            self._drop_device()
        self.device = device
        if self._vector is not None or self._dev is not None:
            self._device_index()
            if torch.device(device).type == "cuda" and self._vector is not None and self._keep_only_device_copy():
                self._vector = None            # re-exported on demand; avoids a second device copy

    def _keep_only_device_copy(self) -> bool:
        return True

    # ---- text store ----------------------------------------------------------------------------
    @staticmethod
    def _calculate_offsets(data_file: str):
        offsets, pos = [], 0
        with open(data_file, "rb") as fh:
            for line in fh:
                offsets.append(pos)
                pos += len(line)
        return offsets

    def _load_line(self, file_path: str, offset: int):
        with open(file_path, "rb") as fh:
            fh.seek(offset)
            return json.loads(fh.readline().decode("utf-8"))

    def get_sample(self, index: int):
        if not self.low_memory:
            return self.data[index]
        return self._load_line(self.data_file, self.offsets[index])

    # ---- search (index.py:88-94) -------------------------------------------------------------------
    def search(self, q_embs: torch.Tensor, k: int, filter=None) -> SearchResults:
        """`filter` (not in the reference): search only part of the index -- a vsearch_amd.doc_filter.DocFilter, a bool mask [N] or
        [B, N] (True = allowed) or an integer tensor of allowed row ids.  The result is the top k of the allowed rows; positions beyond
        them hold id -1 and score -inf.  A mask whose length is not the index's row count raises ValueError."""
        if isinstance(q_embs, np.ndarray):
            q_embs = torch.from_numpy(q_embs)
        dev_index = self._device_index()
        gpu = torch.device("cuda", dev_index.device)         # (cached: info() reads search statistics and synchronises)
        q = q_embs.detach().to(gpu)
        q = q.to(self._dtype) if self._dtype in (torch.float16, torch.float32) else q.float()   # `.type(self.vector.dtype)`
        if q.dim() == 1:
            q = q.unsqueeze(0)
        ids, scores = dev_index.search(q.contiguous(), int(k), filter=filter)
        scores = scores.to(self._dtype)
        if torch.device(self.device).type != "cuda":
            ids, scores = ids.cpu(), scores.cpu()
        return SearchResults(ids, scores)

    # ---- explain (not in the reference: ir.explain(q, p) read from the index rows) -----------------------------------------------
    def _n_rows(self) -> int:
        return int(self._device_index().info().n_rows)

    def _explain_target(self):
        """(object with .explain(q, ids, topn), its first GPU)"""
        dev = self._device_index()
        return dev, dev.device

    def explain(self, q_embs, ids, topn: int = 10) -> Explanation:
        """Why document ids[b, j] is a hit of query b: the top `topn` columns by contribution q_w * p_w (largest first), the pair's
        score (a sparse index: bit-identical to its search score) and the number of matched terms, all read from the stored rows --
        nothing is re-embedded.  ids: int64 [B, k] (e.g. ``search(...).ids``); -1 is a filtered search's padding (cols -1, score -inf).
        Columns are in the index file's column space (+ ``shift``).  An id outside [-1, N) raises IndexError."""
        return self._explain(q_embs, ids, topn)

    def disentangle(self, ids, topn: int = 10) -> Explanation:
        """The top `topn` stored values of each listed row (no query, no encoder): contrib = the value (1 for a bag-of-token index),
        score = the row's sum, n_matched = its non-zeros.  ids: int64 [B, k] (or [k]: one row of ids)."""
        return self._explain(None, ids, topn)

    def _explain(self, q_embs, ids, topn):
        if isinstance(ids, np.ndarray):
            ids = torch.from_numpy(ids)
        if not isinstance(ids, torch.Tensor):
            raise TypeError(f"ids must be a tensor or an ndarray, got {type(ids).__name__}")
        if ids.dim() == 1:
            ids = ids.unsqueeze(0)
        q = None
        if q_embs is not None:
            if isinstance(q_embs, np.ndarray):
                q_embs = torch.from_numpy(q_embs)
            q = q_embs.detach()
            if q.dim() == 1:
                q = q.unsqueeze(0)
        _explain_args(q, ids.cpu() if q is None or not q.is_cuda else ids.to(q.device), topn)     # (argument errors before any device work)
        if ids.numel():
            lo, hi = int(ids.min()), int(ids.max())
            n = self._n_rows()
            if lo < -1 or hi >= n:
                raise IndexError(f"document id {lo if lo < -1 else hi} out of range [-1, {n})")
        target, gpu_ord = self._explain_target()
        gpu = torch.device("cuda", gpu_ord)
        if q is not None:
            q = q.to(gpu)
            q = q.to(self._dtype) if self._dtype in (torch.float16, torch.float32) else q.float()
            q = q.contiguous()
        ex = target.explain(q, ids.to(gpu).contiguous(), int(topn))
        shift = int(getattr(self, "shift", 0) or 0)
        cols = torch.where(ex.cols >= 0, ex.cols + shift, ex.cols) if shift else ex.cols
        ex = Explanation(cols, ex.contrib, ex.scores, ex.n_matched)
        if torch.device(self.device).type != "cuda":
            ex = Explanation(*(t.cpu() for t in ex))
        return ex

    # ---- query by example (not in the reference: stored rows as queries) -----------------------------------------------------------
    def _example_ids(self, ids, ndim):
        """ids (tensor | ndarray | list) -> int64 tensor of `ndim` dimensions; IndexError for an id outside [-1, N), before any device work"""
        if isinstance(ids, np.ndarray):
            ids = torch.from_numpy(ids)
        elif isinstance(ids, (list, tuple)):
            ids = torch.as_tensor(ids, dtype=torch.int64)
        if not isinstance(ids, torch.Tensor):
            raise TypeError(f"ids must be a tensor, an ndarray or a list, got {type(ids).__name__}")
        if ndim == 2 and ids.dim() == 1:
            ids = ids.unsqueeze(0)
        _int64_ids(ids, ndim)
        if ids.numel():
            lo, hi = int(ids.min()), int(ids.max())
            n = self._n_rows()
            if lo < -1 or hi >= n:
                raise IndexError(f"document id {lo if lo < -1 else hi} out of range [-1, {n})")
        return ids

    def _on_gpu(self, x, gpu, dtype=None):
        if x is None:
            return None
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(x)
        x = x.detach().to(gpu)
        if dtype is not None:
            x = x.to(dtype)
        return x.contiguous()

    def _to_api(self, t):
        return t if torch.device(self.device).type == "cuda" else t.cpu()

    def get_vectors(self, ids):
        """The stored vectors of documents ids (int64 [n]) -- what ``index.vector[ids]`` gives the reference, read from the device rows
        without exporting the index: a sparse / bag-of-token index gives a torch sparse-CSR [n, V], a dense Index a dense [n, V], in the
        index dtype, columns in the vector's space (no shift).  Id -1 gives an empty row; an id outside [-1, N) raises IndexError."""
        ids = self._example_ids(ids, 1)
        target, gpu_ord = self._explain_target()
        gpu = torch.device("cuda", gpu_ord)
        if self.index_type == IndexType.DENSE:
            rows = target.queries_from_rows(ids.to(gpu).unsqueeze(1).contiguous())       # (0 + 1 * v: the stored values, exactly)
            return self._to_api(rows.to(self._dtype))
        indptr, indices, values = target.get_rows(ids.to(gpu).contiguous())
        t = torch.sparse_csr_tensor(indptr, indices.to(torch.int64), values.to(self._dtype), size=(int(ids.numel()), int(self._vector_meta()[0][1])))
        return self._to_api(t)

    def queries_from_rows(self, ids, weights=None, q=None, alpha: float = 1.0):
        """Queries [B, V] (fp32) built from stored rows: fl32(alpha * q[b]) plus fl32(weights[b, j] * vector[ids[b, j]]) for j in order,
        every add rounded to fp32 (id -1 adds nothing).  ids: int64 [B, m] (or [m]: one query); weights [B, m] (default 1); q [B, V]."""
        return self._to_api(self._queries_from_rows(ids, weights, q, alpha)[0])

    def _queries_from_rows(self, ids, weights, q, alpha):
        ids = self._example_ids(ids, 2)
        if weights is not None and not isinstance(weights, (torch.Tensor, np.ndarray)):
            weights = torch.as_tensor(weights, dtype=torch.float32)
        w = self._on_gpu(weights, "cpu", torch.float32)
        if w is not None and w.dim() == 1:
            w = w.unsqueeze(0)
        qc = None
        if q is not None:
            qc = q if isinstance(q, torch.Tensor) else torch.from_numpy(np.asarray(q))
            qc = qc.detach()
            if qc.dim() == 1:
                qc = qc.unsqueeze(0)
            if qc.dtype not in (torch.float32, torch.float16):
                qc = qc.float()
        _by_example_args(ids.cpu(), w, qc.cpu() if qc is not None else None)  # (argument errors before any device work)
        target, gpu_ord = self._explain_target()
        gpu = torch.device("cuda", gpu_ord)
        ids = self._on_gpu(ids, gpu)
        out = target.queries_from_rows(ids, weights=self._on_gpu(w, gpu), q=self._on_gpu(qc, gpu), alpha=float(alpha))
        return out, ids, gpu_ord

    def search_by_example(self, ids, k: int, weights=None, q=None, alpha: float = 1.0, a: Optional[int] = None, exclude: bool = True,
                          filter=None) -> SearchResults:
        """Search with stored documents as queries (more-like-this, relevance feedback): the queries of ``queries_from_rows``, cut to
        their `a` largest entries when `a` is given, searched for the top k.  exclude=True leaves each query's own example ids out of its
        results (exact: the search takes k + m and drops them); exclude=False is exactly ``search(queries_from_rows(...), k)``.
        filter: as ``search``.  Fewer than k rows left: id -1, score -inf."""
        _k_a_args(k, a)
        qq, ids, gpu_ord = self._queries_from_rows(ids, weights, q, alpha)
        if a is not None:
            qq = resparsify(qq, int(a), gpu_ord)
        k = int(k)
        if not exclude:
            return self.search(qq, k, filter=filter)
        n = self._n_rows()
        kk = min(k + int(ids.shape[1]), n) if k <= n else k
        res = self.search(qq, kk, filter=filter)
        gpu = torch.device("cuda", gpu_ord)
        out_ids, out_sc = topk_exclude(res.ids.to(gpu).contiguous(), res.scores.to(gpu).float().contiguous(), ids, k, gpu_ord)
        return SearchResults(self._to_api(out_ids), self._to_api(out_sc.to(self._dtype)))

    # ---- grouped search (not in the reference: it searches a larger k on a guess and de-duplicates on the host) ---------------------
    def set_groups(self, groups):
        """Give every document a group id (an article, a source, a near-duplicate cluster): int array / tensor [N], values >= 0;
        documents with equal values form a group.  Kept as an int32 tensor on the index's GPU for ``search_grouped``; None removes it.
        Groups follow compact() and add(groups=); they are NOT written by save() -- call set_groups again after a load."""
        if groups is None:
            self._groups = None
            return
        g = groups.detach() if isinstance(groups, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(groups)))
        if g.dim() != 1:
            raise ValueError(f"groups must be 1-D (one id per document), got {g.dim()} dimensions")
        if g.is_floating_point() or g.is_complex() or g.dtype == torch.bool:
            raise TypeError(f"groups must be integer group ids, got {g.dtype}")
        n = self._n_rows()
        if int(g.shape[0]) != n:
            raise ValueError(f"groups holds {int(g.shape[0])} entries, the index has {n} documents")
        if n and int(g.min()) < 0:
            raise ValueError(f"group ids must be >= 0, got {int(g.min())}")
        if n and int(g.max()) > 0x7FFFFFFF:
            raise ValueError(f"group id {int(g.max())} does not fit 31 bits")
        gpu = torch.device("cuda", self._explain_target()[1])
        self._groups = g.to(torch.int32).to(gpu).contiguous()

    @property
    def groups(self):
        """the group id of every document (int32 tensor on the index's GPU), None when no groups are set"""
        return getattr(self, "_groups", None)

    def groups_from_samples(self, key: str = "title"):
        """Factorise field `key` of the data file into group ids (documents with equal values share a group, ids in order of first
        appearance) and set them -> the list of distinct values, indexed by group id.  Host work over the text store."""
        n = len(self)
        if n == 0:
            raise ValueError("the index has no data file to read groups from")
        if n != self._n_rows():
            raise ValueError(f"the data file holds {n} documents, the index {self._n_rows()}")
        seen, out = {}, np.empty(n, dtype=np.int32)
        for i in range(n):
            sample = self.get_sample(i)
            if not isinstance(sample, dict):
                raise TypeError(f"document {i} is a {type(sample).__name__}, not a record with fields: pass the group ids to set_groups()")
            if key not in sample:
                raise KeyError(f"document {i} has no field {key!r}")
            v = sample[key]
            out[i] = seen.setdefault(v if isinstance(v, (str, int, float, bool, tuple, type(None))) else json.dumps(v, sort_keys=True), len(seen))
        self.set_groups(out)
        return list(seen)

    def search_grouped(self, q_embs, k: int, per_group: int = 1, filter=None, depth: Optional[int] = None) -> GroupedResults:
        """The top k GROUPS per query (``set_groups``), each shown by its best `per_group` documents: the collapse of the complete
        ranking, exact -- not "de-duplicate whatever top-k' held".  -> GroupedResults(groups [B, k], ids [B, k, per_group], scores
        [B, k, per_group]); groups come in the order of their best document, unused slots hold group -1 / id -1 / score -inf.  Deleted
        documents and `filter` (as ``search``) apply.  depth: the first search's depth (default 2 k per_group); the result does not
        depend on it.  k <= 1024, per_group <= 64, k * per_group <= 8192.  Works on a row-sharded index as well."""
        _grouped_args(k, per_group, depth)
        if self.groups is None:
            raise RuntimeError("the index has no groups: set_groups(groups) or groups_from_samples(key) first")
        if isinstance(q_embs, np.ndarray):
            q_embs = torch.from_numpy(q_embs)
        target, gpu_ord = self._explain_target()
        gpu = torch.device("cuda", gpu_ord)
        if self._groups.device != gpu:
            self._groups = self._groups.to(gpu)
        q = q_embs.detach().to(gpu)
        q = q.to(self._dtype) if self._dtype in (torch.float16, torch.float32) else q.float()
        if q.dim() == 1:
            q = q.unsqueeze(0)
        res = target.search_grouped(q.contiguous(), int(k), self._groups, per_group=int(per_group), filter=filter, depth=depth)
        return GroupedResults(self._to_api(res.groups), self._to_api(res.ids), self._to_api(res.scores.to(self._dtype)))

    # ---- range search (not in the reference: every document scoring at least a threshold, counted) ------------------------------------------
    def _range_queries(self, q_embs, min_score, max_hits):
        """the argument checks (before any device call), then (search target, queries on its GPU in the index dtype)"""
        if isinstance(q_embs, np.ndarray):
            q_embs = torch.from_numpy(q_embs)
        q = q_embs.detach()
        if q.dim() == 1:
            q = q.unsqueeze(0)
        _range_args(q, min_score, max_hits)
        target, gpu_ord = self._explain_target()
        q = q.to(torch.device("cuda", gpu_ord))
        q = q.to(self._dtype) if self._dtype in (torch.float16, torch.float32) else q.float()
        return target, q.contiguous()

    def search_range(self, q_embs, min_score, max_hits: int = 100, filter=None) -> RangeResults:
        """Every document scoring at least `min_score` (one number, or one per query) -> RangeResults(ids, scores, counts): counts [B] is
        the exact number of matches whatever max_hits is; ids / scores [B, max_hits] hold them in the canonical order -- all of them when
        counts[b] <= max_hits, else the top max_hits -- with id -1 / score -inf behind.  One numerics decides membership on every path
        (the score ``explain`` reports).  max_hits in 0..2048.  Deleted documents and `filter` (as ``search``) apply.  Works on a
        row-sharded index as well."""
        target, q = self._range_queries(q_embs, min_score, max_hits)
        res = target.search_range(q, min_score, max_hits=int(max_hits), filter=filter)
        return RangeResults(self._to_api(res.ids), self._to_api(res.scores.to(self._dtype)), self._to_api(res.counts))

    def count_matches(self, q_embs, min_score, filter=None):
        """The number of documents scoring at least `min_score`, per query: int64 [B]."""
        target, q = self._range_queries(q_embs, min_score, 0)
        return self._to_api(target.count_matches(q, min_score, filter=filter))

    def match_filter(self, q_embs, min_score, filter=None):
        """The documents ``search_range`` matches, as a per-query DocFilter on the index's GPU: pass it to ``search(filter=)``, or combine it
        with other filters through ``&``, ``|``, ``~``."""
        target, q = self._range_queries(q_embs, min_score, 0)
        return target.match_filter(q, min_score, filter=filter)

    # ---- boosted search (not in the reference: rank by relevance and numeric fields together, exact) ----------------------------------------
    def _boost_fields(self, boosts, B):
        """the argument errors of `boosts` that need no device -> (field names, weights float32 [B, F])"""
        if not isinstance(boosts, dict) or not boosts:
            raise TypeError('boosts must be a non-empty dict of value field -> weight, e.g. {"recency": 0.3}')
        if len(boosts) > MAX_BOOST_FIELDS:
            raise ValueError(f"a boosted search takes at most {MAX_BOOST_FIELDS} fields, got {len(boosts)}")
        store = self._value_store()
        for name in boosts:
            if name not in store:
                raise KeyError(f"no value field {name!r}: set_values() or values_from_samples() first (fields: {list(store)})")
        w = np.empty((B, len(boosts)), dtype=np.float32)
        for j, (name, wj) in enumerate(boosts.items()):
            wj = np.asarray(wj.detach().cpu().numpy() if isinstance(wj, torch.Tensor) else wj, dtype=np.float32)
            if wj.ndim > 1 or (wj.ndim == 1 and wj.shape[0] != B):
                raise ValueError(f"the weight of {name!r}: a number, or one per query ({B}); got shape {tuple(wj.shape)}")
            w[:, j] = wj
        if not np.isfinite(w).all():
            raise ValueError("weights must be finite")
        return list(boosts), w

    def search_boosted(self, q_embs, k: int = 100, boosts=None, mode: str = "add", min_score=None, filter=None) -> RangeResults:
        """The exact top k by BOOSTED score: relevance plus (mode="add") or times (mode="mul") a weighted sum of up to 4 value fields
        (``set_values`` / ``values_from_samples``), e.g. boosts={"recency": 0.3, "views": 0.1}; a weight is a number or one per query.
        "add": score + sum_j w_j * value_j; "mul": score * (1 + sum_j w_j * value_j); a document without a value gets no boost from that
        field.  Every document is scored -- this is no rescore of a deeper top-k -- with one pinned numerics (``DeviceIndex.search_boosted``),
        so the result is reproducible bit for bit.  min_score: a floor on the boosted score.  -> RangeResults(ids, boosted scores, counts):
        counts [B] is the number of documents at or above the floor (all live, allowed ones without one).  k in 0..2048.  Deleted documents
        and `filter` (as ``search``) apply.  Works on a row-sharded index as well."""
        if mode not in BOOST_MODES:
            raise ValueError(f"mode must be one of {sorted(BOOST_MODES)}, got {mode!r}")
        names, w = self._boost_fields(boosts, 1 if q_embs.ndim == 1 else int(q_embs.shape[0]))      # (before any device work)
        target, q = self._range_queries(q_embs, -np.inf if min_score is None else min_score, k)
        res = target.search_boosted(q, [self._value_field(n) for n in names], w, mode=mode, min_score=min_score, max_hits=int(k), filter=filter)
        return RangeResults(self._to_api(res.ids), self._to_api(res.scores.to(self._dtype)), self._to_api(res.counts))

    # ---- facets (not in the reference: per-label counts of a document set, the summary beside a result list) ------------------------------
    def _facet_store(self):
        if getattr(self, "_facets", None) is None:
            self._facets = {}                                       # name -> (int32 codes on the index's GPU, n_labels, names | None)
        return self._facets

    @staticmethod
    def _facet_codes(codes, n, what="codes"):
        """codes of set_facet / add(facets=) -> int32 CPU tensor [n]; values >= 0 are labels, -1 = none"""
        c = codes.detach().cpu() if isinstance(codes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.atleast_1d(np.asarray(codes))))
        if c.dim() != 1:
            raise ValueError(f"{what} must be 1-D (one code per document), got {c.dim()} dimensions")
        if c.is_floating_point() or c.is_complex() or c.dtype == torch.bool:
            raise TypeError(f"{what} must be integer codes, got {c.dtype}")
        if int(c.shape[0]) != n:
            raise ValueError(f"{what} holds {int(c.shape[0])} entries for {n} documents")
        if n and int(c.min()) < -1:
            raise ValueError(f"{what} must be >= -1 (-1 = no label), got {int(c.min())}")
        if n and int(c.max()) >= 0x7FFFFFFF:
            raise ValueError(f"code {int(c.max())} does not fit 31 bits")
        return c.to(torch.int32)

    def set_facet(self, name: str, codes, names=None):
        """Give every document a label of facet field `name` (a category, a language, a year, an article): int array / tensor [N], values
        >= 0 are labels, -1 means none.  n_labels = max + 1, or len(names) when `names` (label -> display name) is given; a code >=
        len(names) raises.  Kept as an int32 tensor on the index's GPU for ``facets``; codes=None removes the field.  Facet fields follow
        compact() and add(facets=); they are NOT written by save() -- call set_facet again after a load."""
        if not isinstance(name, str) or not name:
            raise TypeError("a facet field is named by a non-empty string")
        if name == "groups":
            raise ValueError('"groups" names the group ids (set_groups): pick another field name')
        store = self._facet_store()
        if codes is None:
            store.pop(name, None)
            return
        c = self._facet_codes(codes, self._n_rows())
        top = int(c.max()) if c.numel() else -1
        if names is not None:
            names = list(names)
            if not names:
                raise ValueError("names is empty")
            if top >= len(names):
                raise ValueError(f"code {top} has no name: names holds {len(names)}")
            n_labels = len(names)
        else:
            n_labels = max(top + 1, 1)
        store[name] = (c.to(torch.device("cuda", self._explain_target()[1])).contiguous(), n_labels, names)

    @property
    def facet_fields(self):
        """the names of the facet fields set on this index"""
        return list(getattr(self, "_facets", None) or {})

    def facet_from_samples(self, key: str, name: Optional[str] = None):
        """Build facet field `name` (default: `key`) from field `key` of the data file: names are the sorted distinct values, a document
        without the key gets -1 -> the names.  Host work over the text store."""
        n = len(self)
        if n == 0:
            raise ValueError("the index has no data file to read facets from")
        if n != self._n_rows():
            raise ValueError(f"the data file holds {n} documents, the index {self._n_rows()}")
        vals = []
        for i in range(n):
            sample = self.get_sample(i)
            if not isinstance(sample, dict):
                raise TypeError(f"document {i} is a {type(sample).__name__}, not a record with fields: pass the codes to set_facet()")
            if key not in sample or sample[key] is None:
                vals.append(None)
                continue
            v = sample[key]
            vals.append(v if isinstance(v, (str, int, float, bool, tuple)) else json.dumps(v, sort_keys=True))
        names = sorted({v for v in vals if v is not None}, key=lambda v: (type(v).__name__, v))
        if not names:
            raise KeyError(f"no document has a field {key!r}")
        code = {(type(v).__name__, v): i for i, v in enumerate(names)}      # (1, 1.0 and True are different labels)
        codes = np.array([-1 if v is None else code[(type(v).__name__, v)] for v in vals], dtype=np.int32)
        self.set_facet(name or key, codes, names)
        return names

    def _facet_field(self, field):
        """-> (codes on the search target's GPU, n_labels, names | None)"""
        gpu = torch.device("cuda", self._explain_target()[1])
        if field == "groups":
            if self.groups is None:
                raise RuntimeError("the index has no groups: set_groups(groups) or groups_from_samples(key) first")
            if self._groups.device != gpu:
                self._groups = self._groups.to(gpu)
            return self._groups, int(self._groups.max()) + 1 if self._groups.numel() else 1, None
        store = self._facet_store()
        if field not in store:
            raise KeyError(f"no facet field {field!r}: set_facet() or facet_from_samples() first (fields: {list(store)})")
        codes, n_labels, names = store[field]
        if codes.device != gpu:
            codes = codes.to(gpu)
            store[field] = (codes, n_labels, names)
        return codes, n_labels, names

    def facet_names(self, field):
        """label -> display name of a facet field (None when it has none)"""
        return self._facet_field(field)[2]

    def facets(self, field: str, q_embs=None, min_score=None, filter=None, topn: Optional[int] = 10, min_count: int = 1):
        """How a document set spreads over the labels of facet field `field` (``set_facet`` / ``facet_from_samples``; "groups" = the group
        ids).  The set: with q_embs and min_score, per query the documents ``match_filter(q_embs, min_score, filter)`` matches; without
        them, `filter` alone (as in ``search``; None = every document).  Deleted documents never count.  -> TopFacets(labels [B, topn],
        counts [B, topn], total [B], other [B]): the topn labels with the most documents of the set (count descending, label ascending, at
        least max(min_count, 1) documents; unused slots label -1 / count 0), total = the size of the set, other = its documents without a
        label; topn=None: the dense FacetCounts(counts [B, n_labels], total, other).  Works on a row-sharded index as well (not on the
        one-process-per-GPU path of ``vsearch_amd.distributed``)."""
        if (q_embs is None) != (min_score is None):
            raise ValueError("q_embs and min_score go together: the set is match_filter(q_embs, min_score, filter), or the filter alone")
        if topn is not None:
            topn, min_count = _topn_args(topn, min_count)
        codes, n_labels, _ = self._facet_field(field)
        target = self._explain_target()[0]
        if q_embs is not None:
            filter = self.match_filter(q_embs, min_score, filter=filter)
        if topn is None:
            return FacetCounts(*(self._to_api(t) for t in target.facet_counts(codes, n_labels, filter=filter)))
        return TopFacets(*(self._to_api(t) for t in target.top_facets(codes, n_labels, topn, filter=filter, min_count=min_count)))

    # ---- set egress (not in the reference: the members of a document set as ids -- the whole list, a page, a uniform sample) ------------------
    def _egress_set(self, q_embs, min_score, filter):
        """the set of count_docs / list_ids / sample_ids, resolved exactly as ``facets`` resolves it"""
        if (q_embs is None) != (min_score is None):
            raise ValueError("q_embs and min_score go together: the set is match_filter(q_embs, min_score, filter), or the filter alone")
        return self.match_filter(q_embs, min_score, filter=filter) if q_embs is not None else filter

    def count_docs(self, filter=None):
        """The number of live documents in `filter` (as in ``search``; None = every document): int64 [B], B = 1 for a shared filter."""
        return self._to_api(self._explain_target()[0].set_count(filter=filter))

    def list_ids(self, q_embs=None, min_score=None, filter=None, offset=0, limit: Optional[int] = None) -> SetIds:
        """The documents of a set as ids in ascending order -> SetIds(ids [B, limit], counts [B]): ranks [offset, offset + limit) of each
        query's list, -1 behind its last member; counts is the full size of the set whatever the window.  The set as in ``facets``: with
        q_embs and min_score the documents ``match_filter`` matches, without them `filter` alone, None = every document; deleted documents
        are never listed.  limit=None takes the largest count; B x limit <= 2^27 -- page with `offset` through a longer list.  Works on a
        row-sharded index as well."""
        _set_window_args(offset, limit)
        filter = self._egress_set(q_embs, min_score, filter)
        return SetIds(*(self._to_api(t) for t in self._explain_target()[0].set_ids(filter=filter, offset=offset, limit=limit)))

    def sample_ids(self, n: int, q_embs=None, min_score=None, filter=None, seed: int = 0) -> SetSample:
        """n documents of a set, uniformly and without replacement -> SetSample(ids [B, n], counts [B]); query b samples under seed + b, the
        same seed gives the same documents on one GPU and on a row-sharded index alike; -1 behind the last when the set holds fewer.  The
        set as in ``list_ids``.  n in 1..1024."""
        _set_sample_args(n, seed)
        filter = self._egress_set(q_embs, min_score, filter)
        return SetSample(*(self._to_api(t) for t in self._explain_target()[0].set_sample(n, filter=filter, seed=seed)))

    # ---- numeric fields (not in the reference: a quantity per document -- a year, a timestamp, a length, a price -- to filter, describe and sort by)
    def _value_store(self):
        if getattr(self, "_values", None) is None:
            self._values = {}                                       # name -> float32 / int32 values on the index's GPU, the missing sentinel inside
        return self._values

    def set_values(self, name: str, values, missing=None):
        """Give every document a value of numeric field `name`: array / tensor [N].  Integer input becomes int32 (a value outside
        [-2^31 + 1, 2^31 - 1] raises); floating input becomes float32, and NaN means "no value".  missing: optional bool mask [N] of the
        documents without a value.  Kept on the index's GPU for ``value_filter``, ``value_stats``, ``histogram`` and ``top_by_value``;
        values=None removes the field.  A name of a facet field, or "groups", raises.  Value fields follow compact() and
        add(values=); they are NOT written by save() -- call set_values again after a load."""
        if not isinstance(name, str) or not name:
            raise TypeError("a value field is named by a non-empty string")
        if name == "groups":
            raise ValueError('"groups" names the group ids (set_groups): pick another field name')
        if name in (getattr(self, "_facets", None) or {}):
            raise ValueError(f"{name!r} is a facet field of this index: pick another field name")
        store = self._value_store()
        if values is None:
            store.pop(name, None)
            return
        v = value_column(values, missing)
        if int(v.shape[0]) != self._n_rows():
            raise ValueError(f"values holds {int(v.shape[0])} entries for {self._n_rows()} documents")
        store[name] = torch.from_numpy(v).to(torch.device("cuda", self._explain_target()[1])).contiguous()

    @property
    def value_fields(self):
        """the names of the value fields set on this index"""
        return list(getattr(self, "_values", None) or {})

    def values_from_samples(self, key: str, name: Optional[str] = None):
        """Build value field `name` (default: `key`) from field `key` of the data file: numbers only; all integers give an int32 field, else
        float32; a document without the key (or with None) has no value.  Host work over the text store."""
        n = len(self)
        if n == 0:
            raise ValueError("the index has no data file to read values from")
        if n != self._n_rows():
            raise ValueError(f"the data file holds {n} documents, the index {self._n_rows()}")
        vals, missing = [], np.zeros(n, dtype=bool)
        for i in range(n):
            sample = self.get_sample(i)
            if not isinstance(sample, dict):
                raise TypeError(f"document {i} is a {type(sample).__name__}, not a record with fields: pass the values to set_values()")
            v = sample.get(key)
            if v is None:
                missing[i] = True
                v = 0
            elif isinstance(v, bool) or not isinstance(v, (int, float)):
                raise TypeError(f"document {i}: field {key!r} holds {type(v).__name__} {v!r}, not a number")
            vals.append(v)
        if missing.all():
            raise KeyError(f"no document has a field {key!r}")
        ints = all(isinstance(v, int) for v in vals)
        self.set_values(name or key, np.asarray(vals, dtype=np.int64 if ints else np.float64), missing)

    def _value_check(self, field, q_embs=None, min_score=None):
        """the argument errors of a value call that need no device -> the field's vs dtype"""
        store = self._value_store()
        if field not in store:
            raise KeyError(f"no value field {field!r}: set_values() or values_from_samples() first (fields: {list(store)})")
        if (q_embs is None) != (min_score is None):
            raise ValueError("q_embs and min_score go together: the set is match_filter(q_embs, min_score, filter), or the filter alone")
        return _value_dtype(store[field])

    def _value_field(self, field):
        """-> the field's values on the search target's GPU"""
        store = self._value_store()
        self._value_check(field)
        gpu = torch.device("cuda", self._explain_target()[1])
        if store[field].device != gpu:
            store[field] = store[field].to(gpu)
        return store[field]

    def get_values(self, name: str):
        """the values of field `name` [N], float32 or int32, documents without a value as NaN / INT32_MIN"""
        return self._to_api(self._value_field(name))

    def value_filter(self, field: str, lo=None, hi=None):
        """A DocFilter of the documents with lo <= value <= hi of value field `field`, both ends inclusive; None is an open end; lists of B
        bounds give a per-query filter.  A document without a value never matches.  Built on the GPU in one pass over the values; for
        ``search(filter=)`` and ``&``, ``|``, ``~`` with any other filter (term_filter, match_filter, from_labels)."""
        v = self._value_field(field)
        return self._explain_target()[0].value_range_filter(v, lo, hi)

    def _value_set(self, q_embs, min_score, filter):
        return self.match_filter(q_embs, min_score, filter=filter) if q_embs is not None else filter

    # ---- scores as a field: SCORE in place of a field name ---------------------------------------------------------------------------------
    @staticmethod
    def _score_check(q_embs, score_scratch=SCORE_SCRATCH_BYTES):
        """the argument errors of a SCORE call, before any device work"""
        if q_embs is None:
            raise ValueError("field=SCORE needs q_embs: the scores are a query's")
        if isinstance(score_scratch, bool) or not isinstance(score_scratch, (int, np.integer)) or score_scratch < 1:
            raise ValueError(f"score_scratch must be a positive number of bytes, got {score_scratch!r}")

    def _score_set(self, q_embs, min_score, filter):
        """-> (search target, queries on its GPU, None or the set as a DocFilter there)"""
        target, q = self._range_queries(q_embs, 0.0 if min_score is None else min_score, 0)
        if min_score is not None:
            return target, q, target.match_filter(q, min_score, filter=filter)
        if filter is None:
            return target, q, None
        from ...doc_filter import as_doc_filter
        return target, q, as_doc_filter(filter, self._n_rows(), device=target.device, batch=int(q.shape[0]))

    def set_scores(self, q_embs, min_score=None, filter=None) -> torch.Tensor:
        """The exact score of every document of a set -> float32 [B, N] on the index's GPU: the score ``search_range`` decides by and
        ``explain`` reports, bit for bit, and NaN for every document outside the set and every deleted one.  The set: with min_score
        the documents ``match_filter(q_embs, min_score, filter)`` matches per query, else `filter` alone (None = every document).  A row is
        a float32 value array like any field's (``DeviceIndex.value_stats`` and the other value calls take it).  B x N x 4 bytes: for a
        large batch use ``histogram(SCORE, ...)`` and its siblings, which score a bounded block of queries at a time.  A dense ``Index``
        raises NotImplementedError."""
        self._score_check(q_embs)
        target, q, f = self._score_set(q_embs, min_score, filter)
        return target.set_scores(q, filter=f)

    def _over_scores(self, q_embs, min_score, filter, score_scratch, one):
        """one(search target, values [N], None or a one-set DocFilter) -> a result tuple of one query; the queries' results stacked.  The value calls take
        ONE [N] array for all queries, so a batch is served in two levels: a block of Bt queries is scored at once, [Bt, N] float32 within
        score_scratch bytes, then every query of it makes its own value call with its row of the scores and its bitmap."""
        from ...doc_filter import DocFilter
        self._score_check(q_embs, score_scratch)
        target, q, f = self._score_set(q_embs, min_score, filter)
        B, n = int(q.shape[0]), self._n_rows()
        bt = int(max(1, min(B, int(score_scratch) // max(4 * n, 1))))
        parts = []
        for b0 in range(0, B, bt):
            per_query = f is not None and f.per_query
            fb = DocFilter(f.words[b0:b0 + bt], n) if per_query else f
            block = target.set_scores(q[b0:b0 + bt], filter=fb)
            for i in range(int(block.shape[0])):
                parts.append(one(target, block[i], DocFilter(fb.words[i], n) if per_query else fb))
        return type(parts[0])(*(self._to_api(torch.cat(x)) for x in zip(*parts)))

    def value_stats(self, field: str, q_embs=None, min_score=None, filter=None, score_scratch: int = SCORE_SCRATCH_BYTES) -> ValueStats:
        """Count, missing, min, max and sum of value field `field` over a document set -> ValueStats, one entry per query; ``.mean()`` in
        fp64.  The set as in ``facets``: with q_embs and min_score the documents ``match_filter(q_embs, min_score, filter)`` matches per
        query, else `filter` alone (None = every document).  Deleted documents never count.
        field=SCORE describes the set by each query's scores (float32; ``set_scores``): q_embs is required, min_score optional -- without
        it the set is `filter` alone; score_scratch: bytes of the block of scores kept at a time (the queries are served in blocks)."""
        if field is SCORE:
            return self._over_scores(q_embs, min_score, filter, score_scratch, lambda t, v, f: ValueStats(*t.value_stats(v, filter=f)))
        self._value_check(field, q_embs, min_score)
        v = self._value_field(field)
        filter = self._value_set(q_embs, min_score, filter)
        return ValueStats(*(self._to_api(t) for t in self._explain_target()[0].value_stats(v, filter=filter)))

    def histogram(self, field: str, edges, q_embs=None, min_score=None, filter=None, score_scratch: int = SCORE_SCRATCH_BYTES) -> ValueHistogram:
        """How a document set spreads over the bins [edges[i], edges[i + 1]) of value field `field` -> ValueHistogram(counts [B, E - 1],
        below, above, missing, total).  edges: 2..1025 strictly ascending numbers.  The set as in ``value_stats``.  field=SCORE: the
        histogram of each query's scores -- counts[b, i] == count_matches(edges[i]) - count_matches(edges[i + 1]) over the same set."""
        if field is SCORE:
            self._score_check(q_embs, score_scratch)
            _value_edges(edges, nat.VAL_F32)
            return self._over_scores(q_embs, min_score, filter, score_scratch, lambda t, v, f: ValueHistogram(*t.value_histogram(v, edges, filter=f)))
        _value_edges(edges, self._value_check(field, q_embs, min_score))
        v = self._value_field(field)
        filter = self._value_set(q_embs, min_score, filter)
        return ValueHistogram(*(self._to_api(t) for t in self._explain_target()[0].value_histogram(v, edges, filter=filter)))

    def _facet_check(self, field):
        """the argument errors of naming a facet field, before any device work"""
        if field == "groups":
            if self.groups is None:
                raise RuntimeError("the index has no groups: set_groups(groups) or groups_from_samples(key) first")
        elif field not in self._facet_store():
            raise KeyError(f"no facet field {field!r}: set_facet() or facet_from_samples() first (fields: {list(self._facet_store())})")

    def stats_by_facet(self, value_field: str, facet_field: str, q_embs=None, min_score=None, filter=None,
                       score_scratch: int = SCORE_SCRATCH_BYTES) -> FacetValueStats:
        """Count, missing, min, max and sum of value field `value_field` per label of facet field `facet_field` ("groups" = the group ids) over
        a document set, in one pass over the index -> FacetValueStats(count, missing, min, max, sum [B, n_labels], total, other [B]);
        ``.mean()`` in fp64 -- "mean price per category of the matches".  A document without a label counts into `other` only.  The set as in
        ``value_stats``.  Works on a row-sharded index as well.  value_field=SCORE: the mean score per label (as in ``value_stats``)."""
        if value_field is SCORE:
            self._score_check(q_embs, score_scratch)
            self._facet_check(facet_field)
            codes, n_labels, _ = self._facet_field(facet_field)
            return self._over_scores(q_embs, min_score, filter, score_scratch,
                                     lambda t, v, f: FacetValueStats(*t.facet_value_stats(codes, n_labels, v, filter=f)))
        self._value_check(value_field, q_embs, min_score)
        self._facet_check(facet_field)
        v = self._value_field(value_field)
        codes, n_labels, _ = self._facet_field(facet_field)
        filter = self._value_set(q_embs, min_score, filter)
        return FacetValueStats(*(self._to_api(t) for t in self._explain_target()[0].facet_value_stats(codes, n_labels, v, filter=filter)))

    def histogram_by_facet(self, value_field: str, facet_field: str, edges, q_embs=None, min_score=None, filter=None,
                           score_scratch: int = SCORE_SCRATCH_BYTES) -> FacetValueHistogram:
        """How the documents of each label of `facet_field` spread over the bins [edges[i], edges[i + 1]) of `value_field`, over a document
        set (a cross-tab) -> FacetValueHistogram(counts [B, n_labels, E - 1], below, above, missing [B, n_labels], total, other [B]).
        edges: 2..1025 strictly ascending numbers.  The set as in ``value_stats``.  value_field=SCORE: score bands per label."""
        if value_field is SCORE:
            self._score_check(q_embs, score_scratch)
            _value_edges(edges, nat.VAL_F32)
            self._facet_check(facet_field)
            codes, n_labels, _ = self._facet_field(facet_field)
            return self._over_scores(q_embs, min_score, filter, score_scratch,
                                     lambda t, v, f: FacetValueHistogram(*t.facet_value_histogram(codes, n_labels, v, edges, filter=f)))
        _value_edges(edges, self._value_check(value_field, q_embs, min_score))
        self._facet_check(facet_field)
        v = self._value_field(value_field)
        codes, n_labels, _ = self._facet_field(facet_field)
        filter = self._value_set(q_embs, min_score, filter)
        return FacetValueHistogram(*(self._to_api(t) for t in self._explain_target()[0].facet_value_histogram(codes, n_labels, v, edges, filter=filter)))

    def top_by_value(self, field: str, k: int, descending: bool = True, q_embs=None, min_score=None, filter=None,
                     score_scratch: int = SCORE_SCRATCH_BYTES) -> SortedResults:
        """The k documents of a set with the largest (descending) or smallest values of `field`, ties by id ascending -- sort by a field
        instead of by score -> SortedResults(ids [B, k], values [B, k]); documents without a value are never listed, id -1 behind the last.
        k in 1..1024.  The set as in ``value_stats``.  field=SCORE: the best (``search_range``'s list) or the WORST k of the set by score."""
        if field is SCORE:
            self._score_check(q_embs, score_scratch)
            _value_topk_args(k, descending)
            return self._over_scores(q_embs, min_score, filter, score_scratch,
                                     lambda t, v, f: SortedResults(*t.value_topk(v, k, descending=descending, filter=f)))
        self._value_check(field, q_embs, min_score)
        _value_topk_args(k, descending)
        v = self._value_field(field)
        filter = self._value_set(q_embs, min_score, filter)
        return SortedResults(*(self._to_api(t) for t in self._explain_target()[0].value_topk(v, k, descending=descending, filter=filter)))

    def percentiles(self, field: str, pcts, q_embs=None, min_score=None, filter=None, method: str = "linear",
                    score_scratch: int = SCORE_SCRATCH_BYTES) -> ValuePercentiles:
        """Exact percentiles of value field `field` over a document set -> ValuePercentiles(values [B, P], count, missing).  pcts: numbers
        in 0..100.  With q = pct / 100 and pos = q * (count - 1): method "lower" gives the value at rank floor(pos), "higher" at ceil(pos),
        "nearest" at rint(pos) (half to even), in the field's type; "linear" (the default, numpy's) selects the values at floor(pos) and
        ceil(pos) exactly and interpolates lo + (hi - lo) * (pos - floor(pos)) in float64 (exactly lo where lo == hi).  A set without values
        gives NaN / the missing sentinel.  The set as in ``value_stats``; any number of percentiles (16 a pass).  field=SCORE: the median,
        p90, ... of each query's scores over its set."""
        if field is SCORE:
            self._score_check(q_embs, score_scratch)
            q = _percentile_args(pcts, method)
            return self._over_scores(q_embs, min_score, filter, score_scratch, lambda t, v, f: self._percentiles_of(t, v, q, method, f))
        self._value_check(field, q_embs, min_score)
        q = _percentile_args(pcts, method)
        v = self._value_field(field)
        filter = self._value_set(q_embs, min_score, filter)
        return ValuePercentiles(*(self._to_api(t) for t in self._percentiles_of(self._explain_target()[0], v, q, method, filter)))

    @staticmethod
    def _percentiles_of(target, v, q, method, filter):
        """the percentiles of one value array over one filter, on the target's GPU"""
        if method != "linear":
            res = target.value_quantiles(v, q=q, method=method, filter=filter)
            return ValuePercentiles(res.values, res.count, res.missing)
        lo, hi = target.value_quantiles(v, q=q, method="lower", filter=filter), target.value_quantiles(v, q=q, method="higher", filter=filter)
        pos = q[None, :] * (lo.count.cpu().numpy().astype(np.float64) - 1.0)[:, None]
        vals = quantile_lerp(lo.values.cpu().numpy(), hi.values.cpu().numpy(), pos - np.floor(pos))
        if v.dtype == torch.int32:                                  # (an int32 field's sentinel is a number: no answer is NaN here)
            vals = np.where(lo.ranks.cpu().numpy() < 0, np.nan, vals)
        return ValuePercentiles(torch.from_numpy(vals).to(lo.count.device), lo.count, lo.missing)

    def median(self, field: str, q_embs=None, min_score=None, filter=None, method: str = "linear",
               score_scratch: int = SCORE_SCRATCH_BYTES) -> ValuePercentiles:
        """``percentiles(field, [50], ...)``: the median of value field `field` (or of the scores: SCORE) over a document set, values [B, 1]."""
        return self.percentiles(field, [50], q_embs=q_embs, min_score=min_score, filter=filter, method=method, score_scratch=score_scratch)

    # (query, label, rank) cells a per-label percentile call may take: x 2048 bins = the 2^27 counts of the percentiles' 1 GiB rule
    FACET_QUANTILE_CELLS = 65536

    def percentiles_by_facet(self, value_field: str, facet_field: str, pcts, q_embs=None, min_score=None, filter=None, method: str = "linear",
                             score_scratch: int = SCORE_SCRATCH_BYTES) -> FacetValuePercentiles:
        """Exact percentiles of value field `value_field` per label of facet field `facet_field` ("groups" = the group ids) over a document
        set, three counting passes for all labels -> FacetValuePercentiles(values [B, n_labels, P], count, missing [B, n_labels], total,
        other [B]) -- "the median price per category of the matches".  pcts and method as in ``percentiles``, applied to each label's count;
        a label without values gives NaN / the missing sentinel; a document without a label counts into `other` only.  The set as in
        ``value_stats``.  The work is split so that queries x labels x ranks of a pass stay within 65536: first over the queries, then over
        the percentiles (16 a pass at most).  More than 65536 labels are not covered and raise ValueError.  Works on a row-sharded index as
        well.  value_field=SCORE: the median, p90, ... score per label."""
        if value_field is SCORE:
            self._score_check(q_embs, score_scratch)
            q = _percentile_args(pcts, method)
            self._facet_check(facet_field)
            codes, n_labels, _ = self._facet_field(facet_field)
            self._facet_quantile_check(n_labels)
            return self._over_scores(q_embs, min_score, filter, score_scratch,
                                     lambda t, v, f: self._percentiles_by_facet_of(t, codes, n_labels, v, q, method, f))
        self._value_check(value_field, q_embs, min_score)
        q = _percentile_args(pcts, method)
        self._facet_check(facet_field)
        v = self._value_field(value_field)
        codes, n_labels, _ = self._facet_field(facet_field)
        self._facet_quantile_check(n_labels)
        filter = self._value_set(q_embs, min_score, filter)
        target = self._explain_target()[0]
        if filter is not None:
            from ...doc_filter import as_doc_filter
            filter = as_doc_filter(filter, self._n_rows(), device=target.device)
        return FacetValuePercentiles(*(self._to_api(t) for t in self._percentiles_by_facet_of(target, codes, n_labels, v, q, method, filter)))

    def _facet_quantile_check(self, n_labels):
        if n_labels > self.FACET_QUANTILE_CELLS:
            raise ValueError(f"percentiles_by_facet: n_labels = {n_labels} is more than {self.FACET_QUANTILE_CELLS} labels, which is not covered "
                             f"(one query's counts of one rank would pass 2^27): break the facet field up, or filter by from_labels and use percentiles()")

    def _percentiles_by_facet_of(self, target, codes, n_labels, v, q, method, f):
        """the per-label percentiles of one value array over one DocFilter (or None), on the target's GPU, in passes within FACET_QUANTILE_CELLS"""
        from ...doc_filter import DocFilter
        n, P = self._n_rows(), int(q.shape[0])
        per_query = f is not None and f.per_query
        B = f.n_queries if per_query else 1
        bt = max(1, min(B, self.FACET_QUANTILE_CELLS // (n_labels * min(P, MAX_VALUE_RANKS))))
        rp = max(1, min(MAX_VALUE_RANKS, self.FACET_QUANTILE_CELLS // (bt * n_labels)))
        blocks = []
        for b0 in range(0, B, bt):
            fb = DocFilter(f.words[b0:b0 + bt], n) if per_query else f
            vals, first = [], None
            for j0 in range(0, P, rp):
                qj = np.ascontiguousarray(q[j0:j0 + rp])
                if method != "linear":
                    lo = target.facet_value_quantiles(codes, n_labels, v, q=qj, method=method, filter=fb)
                    vals.append(lo.values)
                else:
                    lo = target.facet_value_quantiles(codes, n_labels, v, q=qj, method="lower", filter=fb)
                    hi = target.facet_value_quantiles(codes, n_labels, v, q=qj, method="higher", filter=fb)
                    pos = qj[None, None, :] * (lo.count.cpu().numpy().astype(np.float64) - 1.0)[:, :, None]
                    x = quantile_lerp(lo.values.cpu().numpy(), hi.values.cpu().numpy(), pos - np.floor(pos))
                    if v.dtype == torch.int32:                      # (an int32 field's sentinel is a number: no answer is NaN here)
                        x = np.where(lo.ranks.cpu().numpy() < 0, np.nan, x)
                    vals.append(torch.from_numpy(x).to(lo.count.device))
                first = first or lo
            blocks.append((torch.cat(vals, dim=2), first.count, first.missing, first.total, first.other))
        return FacetValuePercentiles(*(torch.cat(x) for x in zip(*blocks)))

    def median_by_facet(self, value_field: str, facet_field: str, q_embs=None, min_score=None, filter=None, method: str = "linear",
                        score_scratch: int = SCORE_SCRATCH_BYTES) -> FacetValuePercentiles:
        """``percentiles_by_facet(value_field, facet_field, [50], ...)``: the median per label, values [B, n_labels, 1]."""
        return self.percentiles_by_facet(value_field, facet_field, [50], q_embs=q_embs, min_score=min_score, filter=filter, method=method,
                                         score_scratch=score_scratch)

    def _added_values(self, values, n_add):
        """values= of add() / update() -> {name: ndarray [n_add] in the field's type}, or None for an index without value fields.  Raises
        before anything changes: a missing or an extra field, a wrong length, a value the field's type does not hold."""
        have = getattr(self, "_values", None) or {}
        given = dict(values) if values is not None else {}
        if not have:
            if given:
                raise ValueError("the index has no value fields: set_values() first, then add(..., values=)")
            return None
        missing, extra = sorted(set(have) - set(given)), sorted(set(given) - set(have))
        if missing or extra:
            raise ValueError(f"the index has value fields {sorted(have)}: add(..., values=) must give values for exactly these"
                             f" (missing {missing}, unknown {extra})")
        out = {}
        for name, vals in given.items():
            v = value_column(vals, what=f"values[{name!r}]")
            if int(v.shape[0]) != n_add:
                raise ValueError(f"values[{name!r}] holds {int(v.shape[0])} entries for {n_add} added documents")
            if have[name].dtype == torch.int32 and v.dtype != np.int32:
                raise TypeError(f"values[{name!r}]: the field holds integers, got {v.dtype}")
            out[name] = v.astype(np.float32 if have[name].dtype == torch.float32 else np.int32)
        return out

    # ---- term aggregations (not in the reference: what a document set is about, in the vocabulary's own columns) --------------------------
    def _term_set(self, q_embs, min_score, filter, ids):
        """the set of a term aggregation -> (search target, filter, ids), argument errors before any device work"""
        if (q_embs is None) != (min_score is None):
            raise ValueError("q_embs and min_score go together: the set is match_filter(q_embs, min_score, filter), the filter alone, or ids")
        if ids is not None and (q_embs is not None or filter is not None):
            raise ValueError("ids name the set themselves: give them without q_embs / min_score / filter")
        if ids is not None:
            ids = self._example_ids(ids, 2)
        target, gpu_ord = self._explain_target()
        if q_embs is not None:
            filter = self.match_filter(q_embs, min_score, filter=filter)
        if ids is not None:
            ids = ids.to(torch.device("cuda", gpu_ord)).contiguous()
        return target, filter, ids

    def term_counts(self, q_embs=None, min_score=None, filter=None, ids=None) -> TermCounts:
        """For a document set, how many of its documents have each vocabulary column -> TermCounts(counts [B, V], total [B]), int64; columns
        in the vector's space (no shift).  The set: with q_embs and min_score, per query the documents ``match_filter(q_embs, min_score,
        filter)`` matches; `filter` alone (as in ``search``); or `ids`, int64 [B, m] hit lists (``search(...).ids``; -1 is skipped, an id
        listed twice counts twice, an id outside [-1, N) raises IndexError).  None of them: every live document -- the document frequency
        of the whole vocabulary in one pass.  Deleted documents never count.  Works on a row-sharded index as well (not on the
        one-process-per-GPU path of ``vsearch_amd.distributed``, and not on a dense index)."""
        target, filter, ids = self._term_set(q_embs, min_score, filter, ids)
        return TermCounts(*(self._to_api(t) for t in target.term_counts(filter=filter, ids=ids)))

    def significant_terms(self, q_embs=None, min_score=None, filter=None, ids=None, topn: int = 20, method: str = "jlh", min_count: int = 1,
                          background=None) -> TopTerms:
        """The columns over-represented in a document set (``term_counts``'s set) against a background -> TopTerms(cols [B, topn], scores
        [B, topn], df [B, topn], bg [B, topn], total [B]); cols in the index file's column space (+ ``shift``), as ``explain`` reports
        them.  With fgp = df / total and bgp = bg / background total: method "jlh" scores (fgp - bgp) * (fgp / bgp) over the columns with
        fgp > bgp, "lift" fgp / bgp, "count" lists the columns most documents of the set have (exact integer order).  Only columns at
        least max(min_count, 1) documents of the set have; score descending, then column ascending; unused slots -1 / -inf / 0 / 0.
        background=None counts every live document in the same call (one more pass; nothing is cached, so it is never stale); a caller
        who wants to pay once passes ``background=index.term_counts()``."""
        _term_topn_args(topn, method, min_count)
        target, filter, ids = self._term_set(q_embs, min_score, filter, ids)
        top = target.top_terms(filter=filter, ids=ids, topn=int(topn), method=method, min_count=int(min_count), background=background)
        shift = int(getattr(self, "shift", 0) or 0)
        cols = torch.where(top.cols >= 0, top.cols + shift, top.cols) if shift else top.cols
        return TopTerms(*(self._to_api(t) for t in (cols, top.scores, top.df, top.bg, top.total)))

    def term_sums(self, q_embs=None, min_score=None, filter=None, ids=None) -> TermSums:
        """For a document set (``term_counts``'s: q_embs + min_score, `filter`, `ids`, or every live document), how much weight it puts on
        each vocabulary column -> TermSums(sums [B, V], total [B]), int64; columns in the vector's space (no shift).  sums are fixed
        point -- every stored value (clamped to +-2^20) times 2^24, rounded to nearest even, added as integers: exact for an fp16 or a
        binary index, the same whatever the order and however the index is sharded.  ``.values()`` gives float64 sums, ``.mean()`` the
        centroid.  Deleted documents never contribute.  Not on the one-process-per-GPU path of ``vsearch_amd.distributed``, not on a
        dense index."""
        target, filter, ids = self._term_set(q_embs, min_score, filter, ids)
        return TermSums(*(self._to_api(t) for t in target.term_sums(filter=filter, ids=ids)))

    def centroid(self, q_embs=None, min_score=None, filter=None, ids=None) -> torch.Tensor:
        """The mean vector of a document set (``term_sums``'s set) -> float32 [B, V] in the vector's space: a query like any other,
        ``index.search(index.centroid(filter=f), k)``.  A query whose set is empty gets an all-zero row."""
        return self.term_sums(q_embs, min_score, filter=filter, ids=ids).mean()

    def centroid_terms(self, q_embs=None, min_score=None, filter=None, ids=None, topn: int = 20, min_count: int = 0) -> TopWeights:
        """The columns a document set (``term_sums``'s set) puts the most weight on -> TopWeights(cols [B, topn], scores [B, topn], sums
        [B, topn], total [B]); cols in the index file's column space (+ ``shift``), as ``explain`` reports them.  score = the column's mean
        weight over the set, float32((double(sum) * 2^-24) / double(total)); only columns with a positive sum; score descending, then
        column ascending; unused slots -1 / -inf / 0.  min_count > 0 takes ``term_counts`` of the same set as well and lists only columns
        at least min_count of its documents have."""
        _weight_topn_args(topn, min_count)
        target, filter, ids = self._term_set(q_embs, min_score, filter, ids)
        top = target.top_weight_terms(filter=filter, ids=ids, topn=int(topn), min_count=int(min_count))
        shift = int(getattr(self, "shift", 0) or 0)
        cols = torch.where(top.cols >= 0, top.cols + shift, top.cols) if shift else top.cols
        return TopWeights(*(self._to_api(t) for t in (cols, top.scores, top.sums, top.total)))

    # ---- term aggregations by facet label (not in the reference: the centroid and the terms of every cluster, category or article at once) -----
    def _facet_term_set(self, field, q_embs, min_score, filter):
        """the set and the labels of a by-facet term aggregation -> (search target, codes, n_labels, names, one shared DocFilter | None);
        argument errors before any device work"""
        if (q_embs is None) != (min_score is None):
            raise ValueError("q_embs and min_score go together: the set is match_filter(q_embs, min_score, filter), or the filter alone")
        if self.index_type == IndexType.DENSE:
            raise NotImplementedError("the term aggregations read the sparse rows: a dense Index is not covered")
        if q_embs is not None and (getattr(q_embs, "ndim", 2) != 2 or int(q_embs.shape[0]) != 1):
            raise ValueError("a by-facet term aggregation takes ONE document set: one query [1, V], not a batch")
        from ...doc_filter import DocFilter
        many = filter.n_queries if isinstance(filter, DocFilter) else (int(filter.shape[0]) if getattr(filter, "ndim", 1) == 2 else None)
        if many is not None and many != 1:
            raise ValueError("a by-facet term aggregation takes ONE document set, not a per-query filter")
        if field != "groups" and field not in self._facet_store():
            raise KeyError(f"no facet field {field!r}: set_facet() or facet_from_samples() first (fields: {list(self._facet_store())})")
        codes, n_labels, names = self._facet_field(field)
        target, gpu_ord = self._explain_target()
        if q_embs is not None:
            filter = self.match_filter(q_embs, min_score, filter=filter)
        if filter is not None:
            from ...doc_filter import as_doc_filter
            filter = as_doc_filter(filter, self._n_rows(), device=torch.device("cuda", gpu_ord))
            if filter.per_query:
                if filter.n_queries != 1:
                    raise ValueError("a by-facet term aggregation takes ONE document set, not a per-query filter")
                filter = DocFilter(filter.words[0], filter.n_rows)
        return target, codes, n_labels, names, filter

    def term_sums_by_facet(self, field: str, q_embs=None, min_score=None, filter=None) -> LabelTermSums:
        """``term_sums`` per label of facet field `field` (``set_facet`` / ``facet_from_samples``; "groups" = the group ids), for every label
        at once -> LabelTermSums(sums [n_labels, V], total [n_labels], other [1]), int64: row l is bit for bit ``term_sums`` of the set's
        documents with label l; other counts the set's documents without a label.  ONE set: one query [1, V] with min_score (the documents
        ``match_filter`` matches), `filter` alone, or neither: every live document -- a batch of queries or a per-query filter raises
        ValueError.  One pass over the stored cells whatever the number of labels (at most 65 536, and n_labels x V <= 2^27).  Works on a
        row-sharded index as well (not on the one-process-per-GPU path of ``vsearch_amd.distributed``, and not on a dense index)."""
        target, codes, n_labels, _, f = self._facet_term_set(field, q_embs, min_score, filter)
        return LabelTermSums(*(self._to_api(t) for t in target.label_term_sums(codes, n_labels, filter=f)))

    def term_counts_by_facet(self, field: str, q_embs=None, min_score=None, filter=None) -> LabelTermCounts:
        """``term_counts`` per label of facet field `field` -> LabelTermCounts(counts [n_labels, V], total [n_labels], other [1]); the set
        as in ``term_sums_by_facet``."""
        target, codes, n_labels, _, f = self._facet_term_set(field, q_embs, min_score, filter)
        return LabelTermCounts(*(self._to_api(t) for t in target.label_term_counts(codes, n_labels, filter=f)))

    def centroids_by_facet(self, field: str, q_embs=None, min_score=None, filter=None) -> torch.Tensor:
        """The mean vector of every label's documents -> float32 [n_labels, V] in the vector's space, ready for ``index.search``: the
        centroid of every cluster, category or article at once.  A label without documents in the set gets an all-zero row."""
        return self.term_sums_by_facet(field, q_embs, min_score, filter=filter).mean()

    def centroid_terms_by_facet(self, field: str, topn: int = 20, min_count: int = 0, q_embs=None, min_score=None, filter=None) -> TopWeights:
        """Per label the columns its documents put the most weight on -> TopWeights(cols [n_labels, topn], scores, sums, total [n_labels]),
        as ``centroid_terms`` lists them for one set; min_count > 0 takes the per-label counts as well."""
        _weight_topn_args(topn, min_count)
        target, codes, n_labels, _, f = self._facet_term_set(field, q_embs, min_score, filter)
        top = _label_top_weights(target, codes, n_labels, f, int(topn), int(min_count))
        shift = int(getattr(self, "shift", 0) or 0)
        cols = torch.where(top.cols >= 0, top.cols + shift, top.cols) if shift else top.cols
        return TopWeights(*(self._to_api(t) for t in (cols, top.scores, top.sums, top.total)))

    def significant_terms_by_facet(self, field: str, topn: int = 20, method: str = "jlh", min_count: int = 1, background=None, q_embs=None,
                                   min_score=None, filter=None) -> TopTerms:
        """Per label the columns over-represented in its documents against a background -> TopTerms(cols [n_labels, topn], scores, df, bg,
        total [n_labels]), as ``significant_terms`` lists them for one set (method "jlh" | "lift" | "count"); background=None counts every
        live document in the same call."""
        _term_topn_args(topn, method, min_count)
        target, codes, n_labels, _, f = self._facet_term_set(field, q_embs, min_score, filter)
        top = _label_top_terms(target, codes, n_labels, f, int(topn), method, int(min_count), background)
        shift = int(getattr(self, "shift", 0) or 0)
        cols = torch.where(top.cols >= 0, top.cols + shift, top.cols) if shift else top.cols
        return TopTerms(*(self._to_api(t) for t in (cols, top.scores, top.df, top.bg, top.total)))

    # ---- clustering (not in the reference: the nearest of K centroids for every document, and Lloyd's k-means around it) --------------------------
    def _cluster_target(self, filter):
        """-> (search target, its GPU, one shared DocFilter there | None); a dense index raises NotImplementedError before any device work"""
        if self.index_type == IndexType.DENSE:
            raise NotImplementedError("clustering reads the sparse rows: a dense Index is not covered")
        target, gpu_ord = self._explain_target()
        gpu = torch.device("cuda", gpu_ord)
        f = None
        if filter is not None:
            from ...doc_filter import as_doc_filter
            f = as_doc_filter(filter, self._n_rows(), device=gpu)
            if f.per_query:
                raise ValueError("clustering takes ONE document set, not a per-query filter")
        return target, gpu, f

    def _n_cols(self) -> int:
        return int(self._vector_meta()[0][1])

    def assign(self, centroids, metric: str = "dot", filter=None) -> Assignment:
        """For every live document (allowed by `filter`, as in ``search``: one set) the nearest of the K centroids [K, V] (float32, columns
        in the vector's space) -> Assignment(labels int32 [N], values float32 [N]).  metric "dot": the largest dot product, in the
        library's numerics (``explain``'s score where the sums are exact); "l2": the smallest Euclidean distance -- value = dot - ||c||^2 /
        2, so ||x||^2 - 2 value is the squared distance.  Ties go to the lowest centroid; a deleted or filtered-out document gets -1 /
        -inf.  One pass over the index on the GPU, no [K, N] matrix.  K <= 4096.  Works on a row-sharded index as well (not on the
        one-process-per-GPU path of ``vsearch_amd.distributed``, and not on a dense index)."""
        if metric not in ("dot", "l2"):
            raise ValueError(f'metric must be "dot" or "l2", got {metric!r}')
        if self.index_type == IndexType.DENSE:
            raise NotImplementedError("clustering reads the sparse rows: a dense Index is not covered")
        c, _, _ = _assign_args(centroids, None, self._n_cols())
        target, gpu, f = self._cluster_target(filter)
        c = c.to(gpu).contiguous()
        res = target.assign(c, bias=-target.half_norms(c) if metric == "l2" else None, filter=f)
        return Assignment(self._to_api(res.labels), self._to_api(res.values))

    def kmeans(self, n_clusters: int, iters: int = 10, metric: str = "l2", init=None, seed: int = 0, filter=None) -> KMeansResult:
        """Lloyd's k-means over the live documents (allowed by `filter`) -> KMeansResult(centroids float32 [K, V], labels int32 [N], values
        float32 [N], counts int64 [K], n_iter, changed).  init: int64 row ids [K] (those documents are the start centroids), float32
        centroids [K, V], or None: K distinct live, allowed documents drawn with ``torch.randperm`` under a CPU generator seeded with
        `seed`.  Each iteration assigns (``assign``) and, unless nothing changed, moves every centroid to the mean of its documents
        (``label_term_sums``: the sums of all K clusters in one pass); an empty cluster keeps its centroid.  The labels and values returned are
        the assignment under the centroids returned.  Deterministic, bit for bit: two runs are identical.  metric "l2" (Euclidean) or "dot"
        (the largest dot product: spherical k-means without the normalisation).  The centroids are queries for ``search``; the labels feed
        ``set_facet``, ``set_groups`` (see ``cluster``) and ``DocFilter.from_labels``."""
        K, iters = _kmeans_args(n_clusters, iters, metric)
        if self.index_type == IndexType.DENSE:
            raise NotImplementedError("clustering reads the sparse rows: a dense Index is not covered")
        V = self._n_cols()
        _kmeans_args(K, iters, metric, init, V)
        target, gpu, f = self._cluster_target(filter)
        n = self._n_rows()
        rows = None
        if init is not None and len(init.shape) == 1:
            rows = (init.detach().cpu() if isinstance(init, torch.Tensor) else torch.from_numpy(np.asarray(init))).to(torch.int64)
            if int(rows.min()) < 0 or int(rows.max()) >= n:
                raise IndexError(f"an init row lies outside [0, {n})")
        cand = None
        if init is None or f is not None:                               # the live, allowed documents: one pass against a single zero centroid
            ok = target.assign(torch.zeros((1, V), dtype=torch.float32, device=gpu), filter=f).labels >= 0
            cand = ok.nonzero().reshape(-1).cpu()
        n_ok = int(cand.numel()) if cand is not None else self.n_live
        if K > n_ok:
            raise ValueError(f"n_clusters = {K} exceeds the {n_ok} live, allowed documents")
        if init is None:
            g = torch.Generator(device="cpu")
            g.manual_seed(int(seed))
            rows = cand[torch.randperm(n_ok, generator=g)[:K]]
        if rows is not None:
            start = target.queries_from_rows(rows.to(gpu).unsqueeze(1).contiguous())        # (0 + 1 * v: the stored values, exactly)
        else:
            start = _assign_args(init, None, V)[0].to(gpu)
        C_, labels, values, n_iter, changed = kmeans_loop(target, start.to(torch.float32), iters, metric, f)
        counts = target.facet_counts(labels, K, filter=f).counts[0]
        return KMeansResult(self._to_api(C_), self._to_api(labels), self._to_api(values), self._to_api(counts), n_iter, changed)

    def cluster(self, n_clusters: int, field: str = "cluster", set_groups: bool = False, **kmeans_args) -> KMeansResult:
        """``kmeans``, with the labels stored as facet field `field` (``facets(field, q, min_score)`` then counts a result set per cluster;
        unassigned documents carry -1 = no label) and, with set_groups=True, as the group ids of ``search_grouped`` (one hit per cluster;
        documents without a cluster share the group id K, since group ids are >= 0) -> the KMeansResult."""
        res = self.kmeans(n_clusters, **kmeans_args)
        K = int(res.centroids.shape[0])
        self.set_facet(field, res.labels, names=[str(j) for j in range(K)])
        if set_groups:
            self.set_groups(torch.where(res.labels < 0, torch.full_like(res.labels, K), res.labels))
        return res

    def cluster_terms(self, labels, n_clusters: int, topn: int = 10) -> TopWeights:
        """Per cluster the columns its documents put the most weight on -> TopWeights(cols [K, topn], scores, sums, total [K]); cols in the
        index file's column space (+ ``shift``), scores the mean weight, total the cluster's size.  labels: ``kmeans(...).labels``."""
        _weight_topn_args(topn, 0)
        target, gpu, _ = self._cluster_target(None)
        lab = (labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.asarray(labels))).to(gpu)
        K = _kmeans_args(n_clusters, 0, "l2")[0]
        cols, scores, sums, total = _label_top_weights(target, lab, K, None, int(topn), 0)     # all K clusters in one pass
        shift = int(getattr(self, "shift", 0) or 0)
        cols = torch.where(cols >= 0, cols + shift, cols) if shift else cols
        return TopWeights(*(self._to_api(t) for t in (cols, scores, sums, total)))

    def _added_facets(self, facets, n_add):
        """facets= of add() / update() -> {name: int32 CPU codes [n_add]}, or None for an index without facet fields.  Raises before
        anything changes: a missing or an extra field, a code without a name."""
        have = getattr(self, "_facets", None) or {}
        given = dict(facets) if facets is not None else {}
        if not have:
            if given:
                raise ValueError("the index has no facet fields: set_facet() first, then add(..., facets=)")
            return None
        missing, extra = sorted(set(have) - set(given)), sorted(set(given) - set(have))
        if missing or extra:
            raise ValueError(f"the index has facet fields {sorted(have)}: add(..., facets=) must give codes for exactly these"
                             f" (missing {missing}, unknown {extra})")
        out = {}
        for name, codes in given.items():
            c = self._facet_codes(codes, n_add, f"facets[{name!r}]")
            if have[name][2] is not None and n_add and int(c.max()) >= len(have[name][2]):
                raise ValueError(f"facets[{name!r}]: code {int(c.max())} has no name (the field has {len(have[name][2])})")
            out[name] = c
        return out

    # ---- diversified search (not in the reference: Maximal Marginal Relevance over the top hits, similarities from the stored rows) -------
    def _diverse_out(self, res) -> DiverseResults:
        return DiverseResults(self._to_api(res.ids), self._to_api(res.scores.to(self._dtype)), self._to_api(res.pos), self._to_api(res.mmr))

    def search_diverse(self, q_embs, k: int, lam=0.5, depth: Optional[int] = None, sim: str = "cosine", filter=None) -> DiverseResults:
        """The top k with near-duplicates pushed down: Maximal Marginal Relevance over the top `depth` hits of ``search`` -- every pick
        maximises lam * relevance - (1 - lam) * (its largest similarity to a hit already picked), the similarities taken between the stored
        rows on the GPU.  -> DiverseResults(ids, scores, pos, mmr), all [B, k] in pick order: scores are the search's own, pos the hit's
        rank in the plain search, mmr the value it was picked at; unused slots hold id -1 / score -inf / pos -1 / mmr -inf.  lam in [0, 1],
        one number or one per query (1: exactly ``search(q, k)``); sim: "cosine" | "dot"; depth: k <= depth <= 1024 (default
        min(N, 1024, max(4 k, k + 16))).  Deleted documents and `filter` (as ``search``) apply.  Works on a row-sharded index as well."""
        _diverse_args(k, depth, sim)
        if isinstance(q_embs, np.ndarray):
            q_embs = torch.from_numpy(q_embs)
        target, gpu_ord = self._explain_target()
        q = q_embs.detach().to(torch.device("cuda", gpu_ord))
        q = q.to(self._dtype) if self._dtype in (torch.float16, torch.float32) else q.float()
        if q.dim() == 1:
            q = q.unsqueeze(0)
        return self._diverse_out(target.search_diverse(q.contiguous(), int(k), lam=lam, depth=depth, sim=sim, filter=filter))

    def diversify(self, results, k: int, lam=0.5, sim: str = "cosine") -> DiverseResults:
        """``search_diverse``'s selection over hit lists already at hand: `results` is a SearchResults (or any (ids [B, kk], scores) pair,
        kk <= 1024) -- a reranked list, a filtered search's list with its trailing padding.  Rows are read as stored."""
        _diverse_args(k, None, sim)
        ids = self._example_ids(results[0], 2)
        scores = results[1] if isinstance(results[1], torch.Tensor) else torch.as_tensor(np.asarray(results[1]))
        if scores.dim() == 1:
            scores = scores.unsqueeze(0)
        target, gpu_ord = self._explain_target()
        gpu = torch.device("cuda", gpu_ord)
        return self._diverse_out(target.diversify(ids.to(gpu).contiguous(), scores.detach().to(gpu).float().contiguous(), int(k), lam=lam, sim=sim))

    # ---- fused search (not in the reference: several hit lists of a query merged by rank or score on the GPU, vs_fuse_topk) ---------------
    def _fused_out(self, res) -> FusedResults:
        return FusedResults(*(self._to_api(t) for t in res))

    def _query_batch(self, q_embs, gpu):
        """queries as search() takes them -> a contiguous [B, V] tensor of the index's dtype on `gpu`"""
        if isinstance(q_embs, np.ndarray):
            q_embs = torch.from_numpy(q_embs)
        q = q_embs.detach().to(gpu)
        q = q.to(self._dtype) if self._dtype in (torch.float16, torch.float32) else q.float()
        if q.dim() == 1:
            q = q.unsqueeze(0)
        return q.contiguous()

    def search_fused(self, q_embs_list, k: int, method: str = "rrf", weights=None, c: float = 60.0, depth: Optional[int] = None,
                     filter=None) -> FusedResults:
        """One answer to several queries: every batch of `q_embs_list` (a list of L batches [B, V], or [L, B, V]: paraphrases, sub-questions,
        a feedback query next to the original) is searched at depth `depth` and the L hit lists of a query are fused on the GPU.  method:
        "rrf" reciprocal rank fusion sum_l w_l / (c + rank_l) | "sum" weighted CombSUM of min-max normalised scores | "mnz" that times the
        number of lists holding the document | "raw" the weighted sum of the raw scores.  weights: None, [L] or [B, L].  -> FusedResults(ids,
        fused, ranks, scores, n): per hit its 0-based rank and score in every list (-1 / -inf where absent), n the size of the union.  depth:
        default min(N, 1024, 4096 / L, max(4 k, k + 16)).  Deleted documents and `filter` (as ``search``) apply to every search.  Works on a
        row-sharded index as well.  A fusion of the lists' candidates, not a proven top k of a summed score over the whole corpus."""
        qs = list(q_embs_list) if isinstance(q_embs_list, (list, tuple)) else [q_embs_list[l] for l in range(int(q_embs_list.shape[0]))]
        _fuse_args(k, method, c, depth, len(qs))
        target, gpu_ord = self._explain_target()
        gpu = torch.device("cuda", gpu_ord)
        return self._fused_out(target.search_fused([self._query_batch(q, gpu) for q in qs], int(k), method, weights, c, depth, filter))

    def search_hybrid(self, q_embs, others, k: int, method: str = "rrf", weights=None, c: float = 60.0, depth: Optional[int] = None, filter=None,
                      missing: str = "zero") -> FusedResults:
        """This index and others over the SAME rows searched together: the valued index next to the bag-of-token index, a sparse index next
        to a dense one.  `others`: a list of (index, queries for it | None = the same `q_embs`); list 0 is this index.  Every index is
        searched at depth `depth` (`filter` applies to each) and the lists are fused as in ``search_fused``.  missing="zero": the lists as
        they are -- a document outside an index's top `depth` gets nothing from it.  missing="score" (method "raw" only): the union of the
        lists (at most 1024 documents a query, ValueError beyond) is scored on EVERY index from its stored rows (``explain``: on a sparse
        index the search's own score bit for bit) and those complete lists are fused: every returned document carries its true weighted sum.
        Still a fusion of candidates, not a proven top k of the summed score over the corpus."""
        pairs = [(self, q_embs)] + [(idx, q_embs if q is None else q) for idx, q in others]
        L = len(pairs)
        _fuse_args(k, method, c, depth, L)
        if missing not in ("zero", "score"):
            raise ValueError(f"missing must be 'zero' or 'score', got {missing!r}")
        if missing == "score" and method != "raw":
            raise ValueError("missing='score' sums true scores: it goes with method='raw' only")
        rows = [idx._n_rows() for idx, _ in pairs]
        if len(set(rows)) != 1:
            raise ValueError(f"hybrid search needs indexes over the same rows, got row counts {rows}")
        if depth is None:
            depth = max(1, min(rows[0], MAX_FUSE_DEPTH, MAX_FUSE_ENTRIES // L, max(4 * int(k), int(k) + 16)))
        gpu_ord = self._explain_target()[1]
        gpu = torch.device("cuda", gpu_ord)
        lists = []
        for idx, q in pairs:
            r = idx.search(q, int(depth), filter=filter)
            lists.append((r.ids.to(gpu), r.scores.to(gpu).float()))
        if missing == "zero":
            return self._fused_out(fuse_topk(lists, None, int(k), method, weights, c, device=gpu_ord))
        union = fuse_topk(lists, None, min(MAX_FUSE_DEPTH, L * int(depth)), "rrf", device=gpu_ord)
        n_max = int(union.n.max())
        if n_max > MAX_FUSE_DEPTH:
            raise ValueError(f"the lists of a query hold {n_max} different documents, missing='score' scores at most {MAX_FUSE_DEPTH}: lower depth")
        full = [(union.ids, idx.explain(q, union.ids, topn=0).scores.to(gpu).float()) for idx, q in pairs]
        return self._fused_out(fuse_topk(full, None, int(k), "raw", weights, c, device=gpu_ord))

    def _added_groups(self, groups, n_add):
        """groups= of add() / update() -> int32 CPU tensor [n_add], or None for an index without groups"""
        if self.groups is None:
            if groups is not None:
                raise ValueError("the index has no groups: set_groups() first, then add(..., groups=)")
            return None
        if groups is None:
            raise ValueError("the index has groups: add(..., groups=) must give one group id per added document")
        g = groups.detach().cpu() if isinstance(groups, torch.Tensor) else torch.from_numpy(np.atleast_1d(np.asarray(groups)))
        if g.is_floating_point() or g.dtype == torch.bool:
            raise TypeError(f"groups must be integer group ids, got {g.dtype}")
        if g.dim() != 1 or int(g.shape[0]) != n_add:
            raise ValueError(f"groups holds {tuple(g.shape)} entries for {n_add} added documents")
        if n_add and (int(g.min()) < 0 or int(g.max()) > 0x7FFFFFFF):
            raise ValueError("group ids must be in [0, 2^31)")
        return g.to(torch.int32)

    # ---- term constraints (not in the reference: must / must-not / should filters from the index's own columns) --------------------
    def term_filter(self, must=None, must_not=None, should=None, min_should=None, thr=None):
        """A DocFilter of the documents that have every `must` term, no `must_not` term and at least `min_should` of the `should` terms
        (default 1 when `should` is given) -- for ``search(..., filter=)``.  Terms are column ids of the vector (no shift); a document has
        a term iff it stores a non-zero value there, with thr = {column: t} iff the value is >= t.  Each list: column ids (one program for
        the batch) or one list per query.  Built on the GPU from the index rows (DocFilter.from_terms), on every shard of a row-sharded
        index; combine with other filters by ``&``, ``|``, ``~``."""
        from ...doc_filter import DocFilter
        return DocFilter.from_terms(self, must=must, must_not=must_not, should=should, min_should=min_should, thr=thr)

    def doc_freq(self, cols, thr=None, live_only: bool = True):
        """Documents that have each term of `cols` (column ids of the vector) -> int64 tensor [T]; deleted documents do not count unless
        live_only=False."""
        return self._to_api(self._explain_target()[0].doc_freq(cols, thr=thr, live_only=live_only))

    # ---- mutable index (not in the reference: its index is rebuilt) ------------------------------------------------------------------
    def _mutable_target(self):
        """DeviceIndex, or the ShardGroup of a row-sharded index: both have delete_rows / restore_rows / n_live / compact"""
        return self._explain_target()[0]

    def delete(self, ids):
        """Delete documents by id: no search of this index (retrieve, rerank, more_like_this, feedback, every shard) returns them from now
        on.  Ids do not move and len(index) stays the stored row count; explain / get_vectors still answer for a deleted id and restore()
        brings it back, until compact() drops the rows for good.  ids: integers (list / numpy / torch), -1 ignored."""
        self._mutable_target().delete_rows(ids.detach() if isinstance(ids, torch.Tensor) else ids)

    def restore(self, ids=None):
        """Undo delete() for `ids`; None restores every document."""
        self._mutable_target().restore_rows(ids.detach() if isinstance(ids, torch.Tensor) else ids)

    @property
    def n_live(self) -> int:
        """documents not deleted"""
        return int(self._mutable_target().n_live)

    def _check_no_deletions(self, what):
        if (self._dev is not None or getattr(self, "_group", None) is not None) and self.n_live != self._n_rows():
            raise ValueError(f"the index has {self._n_rows() - self.n_live} deleted documents that {what} cannot record: compact() first"
                             " (a .vsx file keeps them)")

    def _swap_compacted(self, rows_extra=0, packets_extra=0):
        """replace the device index (or every shard) by its compaction -> old ids (numpy)"""
        group = getattr(self, "_group", None)
        if group is not None:
            new_group, old = group.compact(rows_extra, packets_extra)
            group.close()
            for sh in self._shards:
                sh.close()
            self._adopt_shards(list(new_group._shards))
            new_group.close()
        else:
            new, old = self._device_index().compact(rows_extra, packets_extra)
            self._dev.close()
            self._dev = new
            self._prepare()
        self._vector = None                                         # re-exported from the new rows on demand
        self._parts = None                                          # (the sources of a joined index no longer lie at their places)
        if self._shape is not None:
            self._shape = (int(old.shape[0]), self._shape[1])
        if self.groups is not None:                                 # new document j keeps the group of old_ids[j]
            g = self._groups
            self._groups = g.index_select(0, torch.from_numpy(old).to(g.device)).to(torch.device("cuda", self._explain_target()[1]))
        for name, (c, n_labels, names) in list((getattr(self, "_facets", None) or {}).items()):     # and the label of old_ids[j]
            c = c.index_select(0, torch.from_numpy(old).to(c.device)).to(torch.device("cuda", self._explain_target()[1]))
            self._facets[name] = (c, n_labels, names)
        for name, v in list((getattr(self, "_values", None) or {}).items()):                        # and the value
            self._values[name] = v.index_select(0, torch.from_numpy(old).to(v.device)).to(torch.device("cuda", self._explain_target()[1]))
        return old

    def compact(self):
        """Drop the deleted rows for good (vs_index_compact on the GPU) -> old_ids: new document j was document old_ids[j].  The text store
        follows: get_sample(j) returns the text that belonged to old_ids[j]."""
        old = self._swap_compacted()
        self.data, offsets = remap_text_store(self.data, getattr(self, "offsets", None) if self.low_memory else None, old)
        if offsets is not None:
            self.offsets = offsets
        return torch.from_numpy(old)

    def pruned(self, topk=None, min_value=None, drop_columns=None, keep_columns=None, max_df=None, protect=None):
        """A NEW index of the same class holding, for every document, a subset of its stored cells (vs_index_prune on the GPU; this index is
        left exactly as it was): the cells whose column is in keep_columns (ids or a bool mask [V]; None: all), not in drop_columns and not
        more frequent than max_df, whose value is >= min_value, and that are among the document's `topk` largest such cells -- or that the
        same document of `protect` stores (a BoTIndex / SparseIndex of the same rows: the reference's bow_mask | topk_mask at topk = m,
        vdr.py:152-169, made from the index built at topk = 768).  max_df: a fraction of the live documents (float in (0, 1]) or a count
        (int): the columns more than that many live documents have are dropped, taken from term_counts().  Ids do not move: the new index
        shares the text store, the groups, the facet and the value fields, and carries the deletions; a row-sharded index is pruned shard by
        shard on its GPUs (protect row-sharded the same way).  A dense index on the matrix cores raises NotImplementedError."""
        target, gpu_ord = self._explain_target()
        sharded = isinstance(target, ShardGroup)
        n_cols = int((target._shards[0] if sharded else target).info().n_cols)
        drop = None if drop_columns is None else _col_mask(drop_columns, n_cols, "drop_columns")
        if max_df is not None:
            if isinstance(max_df, bool) or not isinstance(max_df, (int, float, np.integer, np.floating)):
                raise TypeError(f"max_df must be a fraction (float) or a count (int), got {type(max_df).__name__}")
            if isinstance(max_df, (float, np.floating)):
                if not 0.0 < max_df <= 1.0:
                    raise ValueError(f"a fractional max_df must be in (0, 1], got {max_df}")
                limit = float(max_df) * self.n_live
            else:
                if max_df < 0:
                    raise ValueError(f"max_df must be >= 0, got {max_df}")
                limit = int(max_df)
            frequent = (self.term_counts().counts[0] > limit).cpu().numpy()
            drop = frequent if drop is None else (drop | frequent)
        p_target = None
        if protect is not None:
            if not isinstance(protect, Index):
                raise TypeError(f"protect must be an index of the same rows, got {type(protect).__name__}")
            p_target = protect._explain_target()[0]
            if isinstance(p_target, ShardGroup) != sharded:
                raise ValueError("protect must be row-sharded exactly as this index is (or neither)")
        new_target, _ = target.prune(topk, min_value, keep_cols=keep_columns, drop_cols=drop, protect=p_target)
        new = copy.copy(self)                                       # the text store (data / offsets) is shared: ids did not move
        new._vector = None                                          # re-exported from the pruned rows on demand
        new._dev = None
        for name in ("_facets", "_values"):                         # the columns are shared, the registries are the new index's own
            if getattr(self, name, None) is not None:
                setattr(new, name, dict(getattr(self, name)))
        if sharded:
            new._shards, new._group = None, None
            new._adopt_shards(list(new_target._shards))
            new_target.close()
        else:
            new._dev = new_target
            new._prepare()
        return new

    # ---- reweighted index (not in the reference: row norms, and the stored values times a scale per document and per column) -------------------
    def row_stats(self) -> RowStats:
        """Per stored document (deleted ones included): RowStats(cells int32, nonzero int32, l1 float64, sumsq float64, max float32) -- the
        stored cells, those with a non-zero value, the sum of |value|, the sum of value^2 and the largest value (NaN: no value), read from the
        stored rows on the GPU (vs_index_row_stats).  The sums are float64 in the pinned order of the exact scores: bit-reproducible, and
        the same sharded or not.  Each is ready to be a value field (set_values).  A dense index on the matrix cores raises
        NotImplementedError."""
        return RowStats(*[self._to_api(t) for t in self._explain_target()[0].row_stats()])

    def row_norms(self, p=2):
        """float32 [N]: the L1 (p = 1) or L2 (p = 2) norm of every stored document; the float64 root of row_stats().sumsq is taken on the
        device and cast to float32."""
        if isinstance(p, bool) or p not in (1, 2):
            raise ValueError(f"p must be 1 or 2, got {p!r}")
        st = self._explain_target()[0].row_stats()
        return self._to_api((st.l1 if p == 1 else torch.sqrt(st.sumsq)).to(torch.float32))

    def rescaled(self, row_scale=None, col_scale=None, dtype=None):
        """A NEW index of the same documents and cells whose stored values are value * row_scale[document] * col_scale[column]
        (vs_index_rescale on the GPU; this index is left exactly as it was): products in float64, rounded once to float32 and then, for dtype
        "fp16", to float16.  row_scale [N], col_scale [V]: numbers, numpy or torch; None = 1.  dtype: "fp32" | "fp16" | None = the stored
        dtype (a bag-of-token index, whose cells hold 1: the dtype it reports for its vector).  Ids do not move: the new index shares the text store, the groups, the
        facet and the value fields, and carries the deletions, as ``pruned`` does; a row-sharded index is rescaled shard by shard on its
        GPUs.  A BoTIndex comes back as a SparseIndex.  A dense index on the matrix cores raises NotImplementedError."""
        target, gpu_ord = self._explain_target()
        sharded = isinstance(target, ShardGroup)
        first = target._shards[0] if sharded else target
        src_dtype = int(first.info().store_dtype)
        if dtype is None and src_dtype == nat.VS_NONE:               # binary rows: the dtype the index reports for its vector
            dtype = "fp16" if self._dtype == torch.float16 else "fp32"
        out_dtype = _rescale_dtype(dtype, src_dtype)
        new_target = target.rescale(row_scale, col_scale, out_dtype)
        new = copy.copy(self)                                       # the text store (data / offsets) is shared: ids did not move
        if isinstance(new, BoTIndex):
            new.__class__ = SparseIndex                             # a valued index now (BoTIndex adds nothing to SparseIndex but _binary(): see there)
        new._vector = None                                          # re-exported from the rescaled rows on demand
        new._dev = None
        new._dtype = torch.float16 if out_dtype == nat.VS_F16 else torch.float32
        for name in ("_facets", "_values"):                         # the columns are shared, the registries are the new index's own
            if getattr(self, name, None) is not None:
                setattr(new, name, dict(getattr(self, name)))
        if sharded:
            new._shards, new._group = None, None
            new._adopt_shards(list(new_target._shards))
            new_target.close()
        else:
            new._dev = new_target
            new._prepare()
        return new

    # ---- combined index (not in the reference: the weighted cell-wise sum of two indexes of the same documents) -------------------------------
    def combined(self, other, weight=1.0, other_weight=1.0, dtype=None):
        """A NEW SparseIndex whose document r is weight * (document r of this index) + other_weight * (document r of `other`), cell by cell
        over the union of the two documents' stored columns (vs_index_combine on the GPU; both indexes are left exactly as they were).  A
        score is linear in the stored cells, so ``combined.search(q, k)`` is the exact top k of weight * score + other_weight * other's score
        over the whole corpus -- the hybrid ranking that search_hybrid only approximates from candidate lists:
        ``sparse.combined(bot.rescaled(col_scale=bot.idf_weights()), 1.0, 0.3).search(q, k)``.  other: any SparseIndex / BoTIndex of the
        same length and width (a bag-of-token cell counts 1).  dtype: "fp32" | "fp16" | None = fp32 unless both store fp16.  Ids do not
        move: the new index shares this index's text store, groups, facet and value fields, as ``rescaled`` does; a document deleted in
        either index is deleted.  A BoTIndex comes back valued, as a SparseIndex.  Row-sharded indexes are combined shard by shard on
        their GPUs and have to be cut at the same rows.  A document that stores a column twice raises ValueError; a dense Index
        NotImplementedError."""
        if not isinstance(other, Index):
            raise TypeError(f"other must be an index of the same documents, got {type(other).__name__}")
        if not isinstance(self, SparseIndex) or not isinstance(other, SparseIndex):
            raise NotImplementedError("combined() adds the stored cells of two SparseIndex / BoTIndex: a dense Index has none (build it sparse)")
        target, gpu_ord = self._explain_target()
        o_target = other._explain_target()[0]
        sharded = isinstance(target, ShardGroup)
        if isinstance(o_target, ShardGroup) != sharded:
            raise ValueError("other must be row-sharded exactly as this index is (or neither)")
        first, o_first = (target._shards[0], o_target._shards[0]) if sharded else (target, o_target)
        if len(self) != len(other) or int(first.info().n_cols) != int(o_first.info().n_cols):
            raise ValueError(f"this index is {len(self)} x {int(first.info().n_cols)}, other {len(other)} x {int(o_first.info().n_cols)}: "
                             f"document r is combined with document r, column by column")
        out_dtype = _combine_dtype(dtype, int(first.info().store_dtype), int(o_first.info().store_dtype))
        new_target = target.combine(o_target, weight, other_weight, out_dtype)
        new = copy.copy(self)                                       # the text store (data / offsets) is shared: ids did not move
        if isinstance(new, BoTIndex):
            new.__class__ = SparseIndex                             # a valued index now
        new._vector = None                                          # re-exported from the combined rows on demand
        new._dev = None
        new._dtype = torch.float16 if out_dtype == nat.VS_F16 else torch.float32
        for name in ("_facets", "_values"):                         # the columns are shared, the registries are the new index's own
            if getattr(self, name, None) is not None:
                setattr(new, name, dict(getattr(self, name)))
        if sharded:
            new._shards, new._group = None, None
            new._adopt_shards(list(new_target._shards))
            new_target.close()
        else:
            new._dev = new_target
            new._prepare()
        return new

    def normalized(self, p=2):
        """``rescaled`` to unit L1 / L2 length: row_scale = float32(1 / norm) with the norm in float64; a document whose norm is 0 or not
        finite keeps scale 1.  Searched by the fast path, a unit-length index ranks by cosine for any one query."""
        if isinstance(p, bool) or p not in (1, 2):
            raise ValueError(f"p must be 1 or 2, got {p!r}")
        st = self._explain_target()[0].row_stats()
        norm = st.l1 if p == 1 else torch.sqrt(st.sumsq)
        ok = torch.isfinite(norm) & (norm > 0)
        scale = torch.where(ok, 1.0 / torch.where(ok, norm, torch.ones_like(norm)), torch.ones_like(norm)).to(torch.float32)
        return self.rescaled(row_scale=scale)

    def astype(self, dtype):
        """A NEW index with the same cells stored as "fp16" or "fp32" (``rescaled`` without a scale: float32 -> float16 rounds to nearest
        even, float16 -> float32 is exact), converted on the GPU."""
        if dtype is None:
            raise ValueError("astype needs a dtype: 'fp16' or 'fp32'")
        return self.rescaled(dtype=dtype)

    def idf_weights(self, k: float = 0.5):
        """float32 [V]: log(1 + (N - df + k) / (df + k)) per column, N the live documents and df the live documents that store the column
        with a non-zero value (term_counts()), computed in float64 on the device; 0 where df is 0.  ``rescaled(col_scale=idf_weights())``
        of a BoTIndex is the IDF-weighted lexical index."""
        df = self.term_counts().counts[0].to(torch.float64)
        n = float(self.n_live)
        w = torch.log(1.0 + (n - df + float(k)) / (df + float(k)))
        return self._to_api(torch.where(df > 0, w, torch.zeros_like(w)).to(torch.float32))

    # ---- sub-index (not in the reference: a document set, or the whole index in another order, as a new index) ----------------------------------
    def _set_member_ids(self, filter):
        """every live document of ONE set (a shared filter, or None = all) in ascending order: int64 tensor on the search target's GPU, listed
        by set_ids in pages of MAX_SET_IDS"""
        target = self._explain_target()[0]
        counts = target.set_count(filter=filter)
        if int(counts.numel()) != 1:
            raise ValueError(f"a sub-index is made of ONE document set: a shared filter or the match set of one query, got a batch of {int(counts.numel())}")
        total = int(counts[0])
        if total == 0:
            raise ValueError("empty selection: the set holds no live document")
        pages = [target.set_ids(filter=filter, offset=o, limit=min(MAX_SET_IDS, total - o)).ids[0] for o in range(0, total, MAX_SET_IDS)]
        return pages[0] if len(pages) == 1 else torch.cat(pages)

    def _selected(self, ids):
        """the new index of documents `ids` (int64, host numpy or a tensor on the search target's GPU) in that order, everything attached"""
        target, gpu_ord = self._explain_target()
        gpu = torch.device("cuda", gpu_ord)
        sharded = isinstance(target, ShardGroup)
        new_target = target.select_rows(ids)
        src = (ids if isinstance(ids, torch.Tensor) else torch.from_numpy(ids)).to(gpu)
        new = copy.copy(self)
        new._vector = None                                          # re-exported from the selected rows on demand
        new._dev = None
        new._source_ids = src
        new._parts = None
        if self._shape is not None:
            new._shape = (int(src.shape[0]), self._shape[1])
        if self.data is not None or (self.low_memory and getattr(self, "offsets", None) is not None):
            new.data, offsets = remap_text_store(self.data, getattr(self, "offsets", None) if self.low_memory else None, src.cpu().numpy())
            if offsets is not None:
                new.offsets = offsets
        if self.groups is not None:                                 # new document j keeps the group of source_ids[j]
            new._groups = self._groups.index_select(0, src.to(self._groups.device)).to(gpu)
        if getattr(self, "_facets", None) is not None:              # ... its label of every facet field, with the field's n_labels and names
            new._facets = {name: (c.index_select(0, src.to(c.device)).to(gpu), n_labels, names) for name, (c, n_labels, names) in self._facets.items()}
        if getattr(self, "_values", None) is not None:              # ... and its value of every value field
            new._values = {name: v.index_select(0, src.to(v.device)).to(gpu) for name, v in self._values.items()}
        if sharded:
            new._shards, new._group = None, None
            new._adopt_shards(list(new_target._shards))
            new_target.close()
        else:
            new._dev = new_target
            new._prepare()
        return new

    def subset(self, q_embs=None, min_score=None, filter=None, ids=None):
        """A NEW index of the same class holding a document set of this one (vs_index_select_rows on the GPU; this index is left exactly as
        it was).  The set as in ``list_ids``: `filter` alone (what ``search(filter=)`` accepts, shared by the batch), or with q_embs and
        min_score the documents ``match_filter`` matches for ONE query (B = 1); the documents come in ascending id order and deleted ones are
        never selected.  Or ids=: exactly these documents in exactly this order, repeats kept (an oversample, a bootstrap, ``sample_ids(...)
        .ids[0]``), a deleted id carried as deleted; -1 raises.  Rows are copied whole, so a document scores bit for bit what it scores here.
        The new index carries the texts, the groups, every facet field (n_labels and names) and every value field of its documents, and
        ``source_ids``.  A row-sharded index is selected shard by shard on its GPUs and keeps its sharding (a shard left without documents
        is dropped); there ids= must not go back to an earlier shard (ValueError): a selection does not move rows across shards."""
        if ids is not None:
            if q_embs is not None or min_score is not None or filter is not None:
                raise ValueError("ids= names the documents itself: it goes without q_embs, min_score and filter")
            picked, on_dev = _select_ids(ids.detach() if isinstance(ids, torch.Tensor) else ids)
            if on_dev:
                picked = picked.to(torch.device("cuda", self._explain_target()[1]))
            return self._selected(picked)
        if q_embs is not None and min_score is not None:
            q = torch.from_numpy(q_embs) if isinstance(q_embs, np.ndarray) else q_embs
            if q.dim() == 2 and int(q.shape[0]) != 1:
                raise ValueError(f"a sub-index is made of ONE document set: the match set of one query, got a batch of {int(q.shape[0])}")
        return self._selected(self._set_member_ids(self._egress_set(q_embs, min_score, filter)))

    @property
    def source_ids(self):
        """int64 [len]: document j of this index is document source_ids[j] of the index ``subset`` / ``sorted_by`` made it from (None for
        an index that was not made by them)"""
        src = getattr(self, "_source_ids", None)
        return None if src is None else self._to_api(src)

    def sorted_by(self, field, descending: bool = False):
        """A NEW index holding the LIVE documents of this one ordered by a field (this index is untouched): a facet field (or "groups") orders
        by (label, id) with the documents without a label last; a value field by (value, id) on the order keys of the numeric fields -- -0.0
        and +0.0 tie -- with the documents without a value last; descending reverses the field's order only: ties still go by ascending id
        and the missing stay last.  The order is a stable argsort on the GPU; everything ``subset`` carries is carried, ``source_ids``
        included.  This supplies the operation -- documents of a label in one run of rows --, not a recommendation when to use it.  A
        row-sharded index raises NotImplementedError (the order would move rows across shards); SCORE is not a field."""
        if field is SCORE:
            raise ValueError("SCORE is not a field of sorted_by: scores belong to a query, not to the index")
        target, gpu_ord = self._explain_target()
        if isinstance(target, ShardGroup):
            raise NotImplementedError("sorted_by moves documents across the shards of a row-sharded index: sort before shard_rows()")
        if field == "groups" or field in (getattr(self, "_facets", None) or {}):
            keys = self._facet_field(field)[0].to(torch.int64) + 1    # 0 = no label
        else:
            keys = _value_keys(self._value_field(field))             # 0 = no value
        live = self._set_member_ids(None)
        k = keys.index_select(0, live)
        missing = k == 0
        if descending:
            k = 0xFFFFFFFF - k
        k = torch.where(missing, torch.full_like(k, 1 << 32), k)
        return self._selected(live.index_select(0, torch.argsort(k, stable=True)))

    # ---- joined index (the reference's load step, vstack(shards) at index.py:172-175, for indexes that are on the GPU already) -------------------
    @staticmethod
    def _concat_fields(sources):
        """The field rules of ``concatenated`` over the source indexes, raised before any device work -> (grouped, {facet field: (n_labels,
        names)}, [value fields]).  Groups: every source has them or none does.  A facet or value field of one source must exist in every
        source; a facet field with equal names (or none anywhere: n_labels is the maximum), a value field with equal dtype."""
        grouped = [getattr(s, "_groups", None) is not None for s in sources]
        if any(grouped) and not all(grouped):
            raise ValueError(f"groups: source {grouped.index(False)} has no groups, source {grouped.index(True)} has: every source has them or none does")
        facets, values = {}, []
        stores = [getattr(s, "_facets", None) or {} for s in sources]
        for name in [n for st in stores for n in st]:
            if name in facets:
                continue
            lacking = [i for i, st in enumerate(stores) if name not in st]
            if lacking:
                raise ValueError(f"facet field {name!r} is missing in source {lacking[0]}: a carried field must exist in every source")
            names = [st[name][2] for st in stores]
            if any(nm != names[0] for nm in names[1:]):
                bad = next(i for i, nm in enumerate(names) if nm != names[0])
                raise ValueError(f"facet field {name!r}: the label names of source {bad} differ from source 0's (codes are not remapped by name)")
            facets[name] = (len(names[0]) if names[0] is not None else max(st[name][1] for st in stores), names[0])
        stores = [getattr(s, "_values", None) or {} for s in sources]
        for name in [n for st in stores for n in st]:
            if name in values:
                continue
            lacking = [i for i, st in enumerate(stores) if name not in st]
            if lacking:
                raise ValueError(f"value field {name!r} is missing in source {lacking[0]}: a carried field must exist in every source")
            dts = [st[name].dtype for st in stores]
            if any(dt != dts[0] for dt in dts[1:]):
                bad = next(i for i, dt in enumerate(dts) if dt != dts[0])
                raise ValueError(f"value field {name!r} is {dts[0]} in source 0 and {dts[bad]} in source {bad}: the dtypes must be equal")
            values.append(name)
        return all(grouped), facets, values

    def concatenated(self, *others, dtype=None):
        """A NEW index of the class of this one holding this index's documents, then those of others[0], and so on (vs_index_concat on the
        GPU; every source is left exactly as it was): document j of source s is document ``parts[s] + j`` of the result.  Rows are copied
        whole, so a document scores bit for bit what it scored in a source of the result's dtype.  others: SparseIndex / BoTIndex of the same
        width on this index's GPU, stored as fp32, fp16 or bag-of-token in any mix (up to 256 sources; the same index may appear twice).
        dtype: "fp32" | "fp16" | None = bag-of-token if all are, fp16 if all valued sources store fp16, else fp32; a BoTIndex joined with a
        valued index comes back a SparseIndex, its cells 1.  Carried: the texts, the `data` lists one behind the other, when EVERY source
        holds its texts in memory -- otherwise the result has no text store, as an index built without a data file --; the groups (every
        source has them or none does); the facet fields (a field must exist in every source with equal names; without names n_labels is
        the maximum) and the value fields (in every source, of equal dtype) -- anything else raises ValueError naming the field before any
        device work --; deletions travel with their documents.  Group ids and facet codes are taken as they are: not offset, not remapped.
        A dense Index on the matrix cores raises NotImplementedError, as does a row-sharded source: ``unsharded()`` it first."""
        sources = [self] + list(others)
        for o in sources:
            if not isinstance(o, Index):
                raise TypeError(f"concatenated() joins indexes, got {type(o).__name__}")
            if getattr(o, "_group", None) is not None:
                raise NotImplementedError("a row-sharded index is not joined as it is: unsharded() makes it one index on one GPU first")
        if not all(isinstance(o, SparseIndex) for o in sources):
            raise NotImplementedError("concatenated() joins the stored rows of SparseIndex / BoTIndex: a dense Index has none (build it sparse)")
        if len(sources) > CONCAT_MAX_SOURCES:
            raise ValueError(f"a join takes at most {CONCAT_MAX_SOURCES} sources, got {len(sources)} (join in stages)")
        grouped, facets, values = self._concat_fields(sources)
        targets = [s._explain_target()[0] for s in sources]
        gpu = torch.device("cuda", targets[0].device)
        out_dtype = _concat_dtype(dtype, [int(t.info().store_dtype) for t in targets])
        new_target = targets[0].concat(targets[1:], dtype=out_dtype)
        counts = [int(t.n_rows) for t in targets]
        new = copy.copy(self)
        if out_dtype != nat.VS_NONE and isinstance(new, BoTIndex):
            new.__class__ = SparseIndex                             # a valued index now
        new._vector = None                                          # re-exported from the joined rows on demand
        new._dev = None
        new._source_ids = None
        new._parts = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64)
        if out_dtype != nat.VS_NONE:
            new._dtype = torch.float16 if out_dtype == nat.VS_F16 else torch.float32
        new._shape = (int(sum(counts)), int(targets[0].info().n_cols))
        for gone in ("offsets", "data_file"):                       # texts on disk are not carried: the result has no text store then
            new.__dict__.pop(gone, None)
        new.low_memory = False
        new.data = [x for s in sources for x in s.data] if all(s.data is not None and not s.low_memory for s in sources) else None
        new._groups = torch.cat([s._groups.to(gpu) for s in sources]) if grouped else None
        new._facets = {name: (torch.cat([s._facets[name][0].to(gpu) for s in sources]), n_labels, names) for name, (n_labels, names) in facets.items()} or None
        new._values = {name: torch.cat([s._values[name].to(gpu) for s in sources]) for name in values} or None
        new._dev = new_target
        new._prepare()
        return new

    @property
    def parts(self):
        """int64 [S + 1] of an index ``concatenated`` made: document j of source s is document parts[s] + j (None for any other index, and
        once ``subset`` / ``sorted_by`` / ``compact`` have moved the documents)"""
        return getattr(self, "_parts", None)

    def _add_csr(self, vectors):
        """vectors -> (indptr, indices, data) of the rows to append"""
        if isinstance(vectors, np.ndarray):
            vectors = torch.from_numpy(vectors)
        if isinstance(vectors, torch.Tensor) and vectors.layout == torch.strided:
            if vectors.dim() == 1:
                vectors = vectors.unsqueeze(0)
            vectors = vectors.detach().cpu().float().to_sparse_csr()
        indptr, indices, data, shape = SparseIndex._csr_parts(vectors)
        return indptr, indices, data, shape

    def add(self, vectors, samples=None, groups=None, facets=None, values=None):
        """Append documents -> their new ids (int64 tensor).  vectors: a sparse CSR tensor / scipy CSR (or a dense [n, V] tensor) whose
        columns match the index.  When the index has no spare capacity it is compacted with room to grow (at least the rows asked for, at
        least a quarter of its size); that moves ids if rows are deleted, so then add() raises and asks for compact().  samples: the
        documents' texts, appended to `data`.  groups: their group ids -- required when the index has groups (set_groups), refused
        when it has none.  facets: {field: codes} for every facet field of the index (set_facet), under the same rule; a field without
        names grows its n_labels with the new codes.  values: {field: values} for every value field of the index (set_values), under the
        same rule; NaN (a float field) marks a document without a value."""
        indptr, indices, data, shape = self._add_csr(vectors)
        n_add = int(indptr.shape[0]) - 1
        new_groups = self._added_groups(groups, n_add)
        new_facets = self._added_facets(facets, n_add)
        new_values = self._added_values(values, n_add)
        target = self._shards[-1] if getattr(self, "_shards", None) else self._device_index()
        info = target.info()
        if info.kind != nat.VS_KIND_CSR and not (info.kind == nat.VS_KIND_DENSE and info.n_packets > 0):
            raise NotImplementedError("a dense index on the matrix cores has no append: build it below DENSE_AS_CSR_DENSITY or rebuild it")
        if int(shape[1]) != int(info.n_cols):
            raise ValueError(f"vectors have {int(shape[1])} columns, the index has {int(info.n_cols)}")
        if samples is not None and (self.low_memory or len(samples) != n_add):
            raise ValueError("samples must hold one text per added vector (and the text store must be in memory: low_memory=False)")
        n0 = self._n_rows()
        if isinstance(data, torch.Tensor) and data.dtype not in (torch.float32, torch.float16):
            data = data.float()
        if isinstance(data, np.ndarray) and data.dtype not in (np.float32, np.float16):
            data = data.astype(np.float32)
        if info.store_dtype == nat.VS_NONE:
            if not bool((data == 1).all()):
                raise ValueError("a bag-of-token (binary) index takes only values of 1")
            data = None
        def append():
            tgt = self._shards[-1] if getattr(self, "_shards", None) else self._dev
            tgt.append_csr(indptr, indices, data)
        try:
            append()
        except ValueError as e:
            if "exceeds the reserved" not in str(e):
                raise
            if self.n_live != n0:
                raise RuntimeError("the index is full and has deleted rows: growing it compacts it, which moves ids -- call compact() first, "
                                   "then add()") from None
            self._swap_compacted(max(n_add, n0 // 4), max(_packets_of(indptr), int(info.n_packets) // 4))
            append()
        if getattr(self, "_shards", None):
            self._group.close()                                     # (the group caches its shards' row ranges)
            self._group = ShardGroup(self._shards)
            if self.EAGER_POSTINGS:
                self._shards[-1].prepare()
        else:
            self._prepare()
        self._vector = None
        if self._shape is not None:
            self._shape = (n0 + n_add, self._shape[1])
        if samples is not None:
            self.data = (self.data or []) + list(samples)
        if new_groups is not None:
            self._groups = torch.cat([self._groups, new_groups.to(self._groups.device)])
        for name, c_new in (new_facets or {}).items():
            c, n_labels, names = self._facets[name]
            if names is None and n_add:
                n_labels = max(n_labels, int(c_new.max()) + 1)
            self._facets[name] = (torch.cat([c, c_new.to(c.device)]), n_labels, names)
        for name, v_new in (new_values or {}).items():
            v = self._values[name]
            self._values[name] = torch.cat([v, torch.from_numpy(v_new).to(v.device)])
        return torch.arange(n0, n0 + n_add, dtype=torch.int64)

    def update(self, ids, vectors, samples=None, groups=None, facets=None, values=None):
        """delete(ids) + add(vectors, samples, groups, facets, values) -> the new ids of the replacements"""
        if (self.groups is None) != (groups is None):               # (before anything is deleted)
            self._added_groups(groups, 0)
        have = getattr(self, "_facets", None) or {}
        if set(have) != set(facets or {}):
            self._added_facets(facets, 0)
        if set(getattr(self, "_values", None) or {}) != set(values or {}):
            self._added_values(values, 0)
        self.delete(ids)
        return self.add(vectors, samples, groups, facets, values)

    # ---- persistence -------------------------------------------------------------------------------
    def save(self, path):
        """Dense index -> ``.pt`` (torch.save of the CPU tensor), like index.py:96-109.  Groups, facet fields and value
        fields (set_groups, set_facet, set_values) are not written: set them again after a load."""
        self._check_no_deletions("a .pt file")
        try:
            torch.save(self.vector.cpu(), path)
            logger.info("Index successfully saved to %s", path)
        except Exception as exc:
            logger.error("Failed to save index to %s: %s", path, exc)
            raise

    def __len__(self):
        if self.data:
            return len(self.data)
        return len(getattr(self, "offsets", [])) if self.low_memory else 0

    def __repr__(self):
        return repr(self.vector)

    def _vector_meta(self):
        if self._vector is not None:
            return self._vector.shape, self._vector.dtype, self._vector.layout
        if self._dev is not None:
            info = self._dev.info()
            layout = torch.strided if info.kind == nat.VS_KIND_DENSE else torch.sparse_csr
            return torch.Size([info.n_rows, info.n_cols]), self._dtype, layout
        if getattr(self, "_shards", None):
            return torch.Size(self._shape), self._dtype, torch.sparse_csr
        return None, None, None

    def __str__(self):
        shape, dtype, layout = self._vector_meta()
        rows = [("Index Type", type(self).__name__), ("Vector Shape", shape), ("Vector Dtype", dtype),
                ("Vector Layout", layout), ("Number of Texts", len(self.data) if self.data else 0), ("Device", self.device)]
        return "".join(f"{name:<18}: {value}\n" for name, value in rows)


def _vsx_rows(path: str) -> int:
    """rows of a native .vsx shard, from its header (csr_index.hip VsxHeader: magic[8], int32 store_dtype, n_cols, int64 n_rows, ...)"""
    import struct
    with open(path, "rb") as fh:
        hdr = fh.read(24)
    if len(hdr) < 24 or hdr[:7] != b"VSXCSR1":
        raise ValueError(f"{path} is not a vsearch native shard file")
    return int(struct.unpack_from("<q", hdr, 16)[0])


class SparseIndex(Index):
    index_type = IndexType.SPARSE

    def __init__(self, index_file: Optional[str] = None, data_file: Optional[str] = None, fp16: bool = True,
                 device: str = "cpu", low_memory: bool = False, shift: int = 0, devices=None):
        """`devices` (not in the reference: its index lives on one device) row-shards the index over several GPUs of this process:
        the shard files matched by `index_file` are dealt to the GPUs in row order (whole files; the reference builds Wiki21M as
        per-shard .npz files, examples/inference_sparse/README.md:90-107, and re-joins them with vstack at index.py:172-175),
        `search` scores the batch on every GPU and merges the per-shard top-k on the first (vs_shard_group_*).  Results are
        identical to the unsharded index."""
        self.shift = shift
        self._devices = _resolve_devices(devices)
        self._shards: Optional[List[DeviceIndex]] = None
        self._group: Optional[ShardGroup] = None
        super().__init__(index_file, data_file, fp16, device, low_memory)

    # -- row shards over several GPUs ------------------------------------------------------------------
    def _drop_device(self):
        if self._group is not None:
            self._group.close()
        for sh in (self._shards or []):
            sh.close()
        self._group, self._shards = None, None
        super()._drop_device()

    def _adopt_shards(self, shards: List[DeviceIndex]):
        self._shards = shards
        self._group = ShardGroup(shards)
        self._dev = None
        if self.EAGER_POSTINGS:
            for sh in shards:
                sh.prepare()
        self.device = f"cuda:{shards[0].device}"

    def shard_rows(self, devices):
        """Deal this (unsharded, device-resident) index over `devices` in contiguous, equal row ranges ("per-shard npz
        or row ranges"): one .npz / .vsx file -- what SparseIndex.save writes, index.py:181-202 -- or an index built in memory
        (Retriever.build_index, retriever.py:284-317) then uses more than one GPU.  Device-to-device copies of the packets
        (vs_index_slice_rows); results stay bit-identical to the unsharded index."""
        gpus = _resolve_devices(devices)
        if not gpus:
            return self
        if self._shards:
            raise NotImplementedError("the index is row-sharded already")
        from vsearch_amd.distributed import shard_rows as _range
        whole = self._device_index()
        info = whole.info()
        if info.kind != nat.VS_KIND_CSR:
            raise NotImplementedError("row sharding serves the sparse and bag-of-token indexes")
        self._shape = (int(info.n_rows), int(info.n_cols))
        built = []
        try:
            for r, gpu in enumerate(gpus):
                row0, n = _range(int(info.n_rows), len(gpus), r)
                built.append(whole.slice_rows(row0, n, gpu))
        except Exception:
            for dev in built:
                dev.close()
            raise
        self._dev = None
        self._vector = None
        whole.close()
        self._devices = gpus
        self._adopt_shards(built)
        return self

    @property
    def shards(self):
        """the DeviceIndex of every row shard, in row order (None: the index is not sharded)"""
        return list(self._shards) if self._shards else None

    @property
    def shard_devices(self):
        """GPU ordinal of every row shard (None: the index is not sharded)"""
        return [sh.device for sh in self._shards] if self._shards else None

    def unsharded(self, device=None):
        """A NEW index holding this row-sharded index as ONE index on one GPU (ShardGroup.gathered: every shard is brought to the target GPU
        by a device-to-device copy, then one vs_index_concat joins them; this index is left exactly as it was).  device: a GPU ordinal or
        "cuda:i", default the first shard's.  Ids do not move: the new index shares the text store, the groups, the facet and the value
        fields, and carries the deletions, as ``rescaled`` does.  During the call the target GPU holds the moved shards and the result at
        once.  ``index.unsharded().sorted_by(field)`` is the sorted order a sharded index cannot be given; the result can be cut into
        another number of shards (shard_rows) or saved as one file.  An index that is not sharded raises ValueError."""
        if self._group is None:
            raise ValueError("the index is not row-sharded: there is nothing to gather")
        gpu_ord = self._shards[0].device if device is None else (int(device) if isinstance(device, int) else _gpu_ordinal(device))
        new_target = self._group.gathered(device=gpu_ord)
        new = copy.copy(self)                                       # the text store (data / offsets) is shared: ids did not move
        new._vector = None                                          # re-exported from the gathered rows on demand
        new._shards, new._group, new._devices = None, None, None
        for name in ("_facets", "_values"):                         # the columns are shared, the registries are the new index's own
            if getattr(self, name, None) is not None:
                setattr(new, name, dict(getattr(self, name)))
        new.device = f"cuda:{gpu_ord}"
        new._dev = new_target
        new._prepare()
        return new

    def search(self, q_embs: torch.Tensor, k: int, filter=None) -> SearchResults:
        if self._group is None:
            return super().search(q_embs, k, filter=filter)
        if isinstance(q_embs, np.ndarray):
            q_embs = torch.from_numpy(q_embs)
        gpu = torch.device("cuda", self._shards[0].device)
        q = q_embs.detach().to(gpu)
        q = q.to(self._dtype) if self._dtype in (torch.float16, torch.float32) else q.float()
        if q.dim() == 1:
            q = q.unsqueeze(0)
        ids, scores = self._group.search(q.contiguous(), int(k), filter=filter)
        return SearchResults(ids, scores.to(self._dtype))

    def _n_rows(self) -> int:
        return self._group.n_rows if self._group is not None else super()._n_rows()

    def _explain_target(self):
        if self._group is None:
            return super()._explain_target()
        return self._group, self._shards[0].device

    def move_to_device(self, device: str):
        if self._group is not None:
            if torch.device(device).type == "cuda" and _gpu_ordinal(device) in self.shard_devices:
                return                                              # (already there: the shards stay where they are)
            raise NotImplementedError("a row-sharded index stays on its GPUs; reload it with device= / devices= to move it")
        super().move_to_device(device)

    # -- conversions ---------------------------------------------------------------------------------
    @staticmethod
    def _csr_parts(v):
        """torch sparse CSR tensor | scipy CSR -> (indptr, indices, data, (n_rows, n_cols))."""
        if isinstance(v, torch.Tensor):
            if v.layout != torch.sparse_csr:
                v = v.to_sparse_csr()
            return v.crow_indices(), v.col_indices(), v.values(), tuple(v.shape)
        return v.indptr, v.indices, v.data, tuple(v.shape)         # scipy.sparse.csr_array / csr_matrix

    def _binary(self) -> bool:
        return False

    def _build_device_index(self) -> DeviceIndex:
        v = self._vector
        if v is None:
            raise RuntimeError("index is empty: no vector to search")
        indptr, indices, data, shape = self._csr_parts(v)
        if isinstance(data, torch.Tensor) and data.dtype not in (torch.float32, torch.float16):
            data = data.float()
        if isinstance(data, np.ndarray) and data.dtype not in (np.float32, np.float16):
            data = data.astype(np.float32)
        if self._binary() and bool((data == 1).all()):
            store, data = nat.VS_NONE, None                          # ids only: 2 bytes per non-zero, integer-exact scores
        else:
            # (a BoTIndex over a VALUED matrix: the reference searches it like any sparse index, index.py:205-218 -- so do we)
            store = nat.VS_F16 if self._dtype == torch.float16 else nat.VS_F32
        return DeviceIndex.from_csr(indptr, indices, data, shape[1], store_dtype=store, device=_gpu_ordinal(self.device))

    def _export_vector(self):
        parts = self._shards if self._shards else [self._dev]
        ip_all, ix_all, d_all, rows, nnz0, n_cols = [np.zeros(1, np.int64)], [], [], 0, 0, 0
        for dev in parts:
            indptr, indices, data = dev.export_csr(np.float16 if self._dtype == torch.float16 else np.float32)
            info = dev.info()
            ip_all.append(indptr[1:] + nnz0)
            ix_all.append(indices)
            d_all.append(data)
            rows += info.n_rows
            nnz0 += int(indptr[-1])
            n_cols = info.n_cols
        t = torch.sparse_csr_tensor(torch.from_numpy(np.concatenate(ip_all)), torch.from_numpy(np.concatenate(ix_all)),
                                    torch.from_numpy(np.concatenate(d_all)), size=(rows, n_cols))
        return t.to(self.device)

    @property
    def vector(self):
        if self._vector is None and (self._dev is not None or self._shards):
            self._vector = self._export_vector()
        return self._vector

    @vector.setter
    def vector(self, value):
        Index.vector.fset(self, value)

    def _scipy_csr_to_torch_csr(self, mat) -> torch.Tensor:
        t = torch.sparse_csr_tensor(torch.from_numpy(mat.indptr), torch.from_numpy(mat.indices), torch.from_numpy(mat.data), size=mat.shape)
        return t.to(self.device)

    # -- loading (index.py:163-179) ------------------------------------------------------------------
    def init_index(self, index_file: Optional[str], fp16: bool = True):
        if not index_file:
            return
        from scipy.sparse import load_npz
        files = sorted(glob.glob(index_file))
        if not files:
            raise FileNotFoundError(f"no index file matches {index_file!r}")
        logger.info("***** Loading %s Index from %d files *****", self.index_type.value, len(files))
        if all(f.endswith(".vsx") for f in files) and self._devices and len(files) < len(self._devices):
            # fewer native files than GPUs: row ranges.  The files are joined on the first GPU (device-to-device), then dealt out
            if self.shift:
                raise ValueError(f"a native .vsx shard stores the columns after the shift was applied: load it with shift=0 (got shift={self.shift})")
            self._drop_device()
            self._vector = None
            gpus, self._devices = self._devices, None
            try:
                if len(files) == 1:
                    self.init_index(files[0], fp16)
                    self.shard_rows(gpus)
                else:
                    # every file's rows, sliced at the GPUs' range boundaries; a GPU whose range spans two files holds two shards
                    # (a shard group takes any number of shards per device, in row order).  ONE file at a time (all files at
                    # once on the first GPU needed room for the whole index there): the row counts come from the files' headers, a file
                    # is loaded on the GPU that gets most of its rows, cut into the ranges it overlaps (peer copies) and closed
                    from vsearch_amd.distributed import shard_rows as _range
                    rows = [_vsx_rows(f) for f in files]
                    total, built, start = sum(rows), [], 0
                    bounds = [_range(total, len(gpus), r) for r in range(len(gpus))]
                    try:
                        for f, n in zip(files, rows):
                            cuts = [(gpu, max(start, b0), min(start + n, b0 + bn)) for gpu, (b0, bn) in zip(gpus, bounds)]
                            cuts = [(gpu, lo, hi) for gpu, lo, hi in cuts if hi > lo]
                            home = max(cuts, key=lambda c: c[2] - c[1])[0] if cuts else gpus[0]
                            dev = DeviceIndex.load_native(f, device=home)
                            try:
                                if int(dev.info().n_rows) != n:
                                    raise ValueError(f"{f}: header says {n} rows, the file holds {int(dev.info().n_rows)}")
                                for gpu, lo, hi in cuts:
                                    built.append(dev.slice_rows(lo - start, hi - lo, gpu))
                            finally:
                                dev.close()
                            start += n
                    except Exception:
                        for d in built:
                            d.close()
                        raise
                    info = built[0].info()
                    self._dtype = torch.float32 if info.store_dtype == nat.VS_F32 else torch.float16
                    self._shape = (total, int(info.n_cols))
                    self._adopt_shards(built)
            finally:
                self._devices = gpus
            return
        if all(f.endswith(".vsx") for f in files) and (len(files) == 1 or self._devices):
            # native shard files: the device format verbatim.  One file -> this device; several (with `devices`) -> one row shard each,
            # dealt to the GPUs in order
            if self.shift:
                raise ValueError("a native .vsx shard stores the columns after the shift was applied: load it with shift=0 "
                                 f"(got shift={self.shift}); convert from .npz shards to change it")
            self._drop_device()
            self._vector = None
            gpus = self._devices or [_gpu_ordinal(self.device)]
            loaded = []
            try:
                for i, f in enumerate(files):
                    dev = DeviceIndex.load_native(f, device=gpus[i * len(gpus) // len(files)])
                    loaded.append(dev)
                    info = dev.info()
                    # the file holds the device format verbatim: it must be the kind of index this class searches
                    if info.kind != nat.VS_KIND_CSR:
                        raise ValueError(f"{f} holds a dense index (sparsity-aware dense store): load it with Index, not {type(self).__name__}")
                    if not self._binary() and info.store_dtype == nat.VS_NONE:   # (a BoTIndex may hold a valued matrix, like the reference's)
                        raise ValueError(f"{f} holds a binary (bag-of-token) index: it cannot be loaded as {type(self).__name__}")
                    if loaded[0].info().store_dtype != info.store_dtype or loaded[0].info().n_cols != info.n_cols:
                        raise ValueError(f"{f}: shards of one index must agree in value type and column count")
            except Exception:
                for dev in loaded:
                    dev.close()
                raise
            info = loaded[0].info()
            if not fp16 and info.store_dtype == nat.VS_F16:
                logger.warning("%s stores fp16 values; fp16=False cannot restore fp32 precision", files[0])
            self._dtype = torch.float32 if info.store_dtype == nat.VS_F32 else torch.float16
            self._shape = (sum(d.info().n_rows for d in loaded), info.n_cols)
            if len(loaded) == 1:
                self._dev = loaded[0]
                self._prepare()                                     # (after the checks: a rejected file costs no second copy in HBM)
            else:
                self._adopt_shards(loaded)
            return
        # pass 1: sizes only.  CSR shards are inspected by the library (zip + npy parsed natively, the column shift applied);
        # other scipy formats go through scipy (bound by nnz).
        from vsearch_amd.device_index import npz_inspect
        rows_total, packets_cap, n_cols = 0, 0, None
        native, f_rows, f_packets = {}, {}, {}
        for f in files:
            try:
                n_r, n_c, _, pk = npz_inspect(f, self.shift)
                native[f] = True
                shape = (n_r, n_c + self.shift)
            except NotImplementedError:                             # not a CSR file
                native[f] = False
                with np.load(f) as z:
                    shape = tuple(int(x) for x in z["shape"])
                    pk = int(z["data"].shape[0]) if "data" in z.files else shape[0] * shape[1]
            f_rows[f], f_packets[f] = shape[0], pk
            packets_cap += pk
            rows_total += shape[0]
            if n_cols is None:
                n_cols = shape[1]
            elif n_cols != shape[1]:
                raise ValueError(f"shard {f} has {shape[1]} columns, expected {n_cols}")
        self._drop_device()
        self._vector = None
        self._dtype = torch.float16 if fp16 else torch.float32
        self._shape = (rows_total, n_cols - self.shift)
        logger.info("***** Converting Sparse index to the device CSR format *****")

        # pass 2: one shard at a time -- the reference's vstack(shards) (index.py:175) never exists on the host.  With `devices` the
        # files are dealt to the GPUs in row order, whole files, as evenly in rows as their boundaries allow.
        gpus = self._devices or [_gpu_ordinal(self.device)]
        split_rows = bool(self._devices) and len(files) < len(gpus)      # fewer files than GPUs (one .npz: what `save` writes): row ranges
        all_gpus = gpus
        if split_rows and len(files) == 1:
            gpus = gpus[:1]
        groups, start, g_row0 = [[] for _ in gpus], 0, [None] * len(gpus)
        for f in files:
            # (row ranges: a file goes to the GPU whose range holds its middle row -- converted there, then cut into the ranges it overlaps;
            #  whole files: to the GPUs in row order, as evenly in rows as the files' boundaries allow)
            at = (start + f_rows[f] // 2) if split_rows else start
            g = min(len(gpus) - 1, at * len(gpus) // max(rows_total, 1))
            if g_row0[g] is None:
                g_row0[g] = start
            groups[g].append(f)
            start += f_rows[f]
        plan = [(g, fs) for g, fs in zip(gpus, groups) if fs]
        plan_row0 = [r0 for r0, fs in zip(g_row0, groups) if fs]

        def convert(store):
            built = []
            try:
                for gpu, fs in plan:
                    dev = DeviceIndex.reserved(sum(f_rows[f] for f in fs), sum(f_packets[f] for f in fs), n_cols - self.shift, store, device=gpu)
                    built.append(dev)
                    for f in fs:
                        if native[f]:
                            dev.append_npz(f, self.shift)           # file -> rows, no scipy object in between
                            continue
                        mat = load_npz(f).tocsr()[:, self.shift:]
                        mat.sort_indices()
                        data = mat.data.astype(np.float32, copy=False)
                        if store == nat.VS_NONE:
                            if not bool((data == 1).all()):
                                raise NotBinaryError("BoTIndex expects a binary matrix (every stored value == 1)")
                            data = None
                        dev.append_csr(mat.indptr, mat.indices, data)
            except Exception:
                for dev in built:                                   # (nothing reserved survives a failed conversion)
                    dev.close()
                raise
            return built

        valued = nat.VS_F16 if fp16 else nat.VS_F32                  # fp32 -> fp16 happens on the device
        if self._binary():
            try:
                built = convert(nat.VS_NONE)
            except NotBinaryError:
                built = None
            if built is None:
                # shards with values other than 1: the reference's BoTIndex searches them like any sparse index (index.py:205-218)
                logger.info("%s: the shards hold values other than 1 -- stored as a valued sparse index", type(self).__name__)
                built = convert(valued)
        else:
            built = convert(valued)
        if len(built) == 1 and split_rows:
            self._dev = built[0]
            self.shard_rows(all_gpus)                                # joined on the first GPU, dealt out in row ranges (device to device)
        elif split_rows:
            # several files, fewer than GPUs: every converted group is cut into the GPUs' row ranges (peer copies) and closed; when a GPU has
            # no room for a range beside the group it holds, the groups stay as they are -- whole files as shards (the dealing before round 5)
            from vsearch_amd.distributed import shard_rows as _range
            bounds = [_range(rows_total, len(all_gpus), r) for r in range(len(all_gpus))]
            cut, ok = [], True
            try:
                for dev, r0 in zip(built, plan_row0):
                    n = int(dev.info().n_rows)
                    for gpu, (b0, bn) in zip(all_gpus, bounds):
                        lo, hi = max(r0, b0), min(r0 + n, b0 + bn)
                        if hi > lo:
                            cut.append(dev.slice_rows(lo - r0, hi - lo, gpu))
            except nat.VsearchNativeError as e:
                logger.warning("row ranges over %d GPUs did not fit (%s): keeping %d whole-file shards", len(all_gpus), e, len(built))
                ok = False
                for d in cut:
                    d.close()
            if ok:
                for dev in built:
                    dev.close()
                built = cut
            self._adopt_shards(built)
        elif len(built) == 1:
            self._dev = built[0]
            self._prepare()
        else:
            self._adopt_shards(built)

    # -- persistence (index.py:181-202) --------------------------------------------------------------
    def save(self, path):
        """CSR index -> scipy ``.npz`` (keys indices, indptr, data, shape, format; int64 indices).  Groups, facet fields and value fields
        (set_groups, set_facet, set_values) are not written: set them again after a load."""
        from scipy.sparse import csr_array, save_npz
        if str(path).endswith(".vsx"):                              # native shard file (loads without a CSR round trip)
            if self._shards:
                raise NotImplementedError("a row-sharded index is saved shard by shard: index.shards[i].save_native(path_i)")
            self._device_index().save_native(path)
            logger.info("Index successfully saved to %s", path)
            return
        self._check_no_deletions("an .npz file")
        try:
            # values go to disk as float32: scipy.sparse has no float16, and the loader re-applies fp16 (fp16=True)
            if self._dev is not None and not self._shards:
                # written by the library (csrc/npz.hip): the same keys / dtypes scipy.sparse.save_npz writes for the reference's
                # int64 torch CSR, stored (uncompressed) members; numpy's savez appends ".npz" to a bare name, so does this
                target = str(path) if str(path).endswith(".npz") else str(path) + ".npz"
                self._dev.save_npz(target, compressed=False)
                logger.info("Index successfully saved to %s", target)
                return
            else:
                ip, ix, d, shape = self._csr_parts(self.vector)        # (a row-sharded index: its shards' rows re-joined)
                indptr, indices, data = ip.cpu().numpy(), ix.cpu().numpy(), d.float().cpu().numpy()
            save_npz(path, csr_array((data, indices, indptr), shape=shape))
            logger.info("Index successfully saved to %s", path)
        except Exception as exc:
            logger.error("Failed to save index to %s: %s", path, exc)
            raise


class BoTIndex(SparseIndex):
    index_type = IndexType.BAG_OF_TOKEN

    def __init__(self, index_file: Optional[str] = None, data_file: Optional[str] = None, fp16: bool = True,
                 device: str = "cpu", low_memory: bool = False, shift: int = 0, devices=None):
        super().__init__(index_file, data_file, fp16, device, low_memory, shift, devices)

    def _binary(self) -> bool:                                      # the ONLY difference from SparseIndex: rescaled() relies on it when it hands
        return True                                                 # a copy of a BoTIndex back as a SparseIndex
