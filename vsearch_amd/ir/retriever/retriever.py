"""Retriever with the reference's interface (/root/reference/src/ir/retriever/retriever.py:20-348):
``retrieve / process_query / build_index / save_index / load_index`` with the same signatures, on
top of the device-resident indexes of ``index.py``.

Deviations (supersets): ``retrieve(index=...)`` really uses the passed index;
``load_index`` accepts ``IndexType`` as well as ``str``; ``build_index(SPARSE)`` emits CSR batch by
batch on the GPU instead of materialising the dense [N, V] matrix; the bag-of-token builder
implements the intended per-document semantics for any batch size (upstream aliases batches).
Training-time methods (``forward`` with negatives, ``retireve_negatives``: hard-negative mining for the training loop,
retriever.py:150-205) are out of scope and absent.
"""
from __future__ import annotations

import logging
from typing import Dict, List, Union

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor as T

from ... import _native as nat
from ..biencoder.biencoder import BiEncoder, BiEncoderConfig
from ..utils import sparse as sp
from .index import BoTIndex, DiverseResults, FusedResults, GroupedResults, Index, IndexType, RangeResults, SCORE, SearchResults, SparseIndex

logger = logging.getLogger(__name__)


class RetrieverConfig(BiEncoderConfig):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)


class Retriever(BiEncoder):
    config_class = RetrieverConfig

    def __init__(self, config: RetrieverConfig, index: Index = None, **kwargs):
        super().__init__(config, **kwargs)
        self.config = config
        self.index = index

    # ---- queries (retriever.py:74-104) -------------------------------------------------------------
    def process_query(self, queries: Union[str, List[str], np.ndarray, T], dropout: float = 0, a: int = None,
                      batch_size: int = 32) -> T:
        """str / list of str -> encoder_q.embed(topk=a); ndarray -> tensor; tensor -> as is; optional dropout."""
        active = a or self.encoder_q.config.topk
        if isinstance(queries, str):
            q_emb = self.encoder_q.embed([queries], batch_size=batch_size, topk=active)
        elif isinstance(queries, list) and len(queries) > 0 and isinstance(queries[0], str):
            q_emb = self.encoder_q.embed(queries, batch_size=batch_size, topk=active)
        elif isinstance(queries, np.ndarray):
            q_emb = torch.Tensor(queries)
        elif isinstance(queries, T):
            q_emb = queries
        else:
            raise NotImplementedError(f"Query type {type(queries)} not supported")
        if dropout:
            q_emb = F.dropout(q_emb, p=dropout)
        return q_emb

    # ---- retrieval (retriever.py:107-148) ----------------------------------------------------------
    def retrieve(self, queries: Union[List[str], np.ndarray, T], k: int = 5, dropout: float = 0, a: int = None,
                 index: Index = None, rerank: bool = False, batch_size: int = 32, filter=None, must=None, must_not=None, should=None,
                 min_should: int = None) -> SearchResults:
        """`filter` (not in the reference): restrict the hits to part of the index (Index.search); hits beyond the allowed rows are
        padding (id -1, score -inf), stay last through the rerank and are not re-embedded.  `must` / `must_not` / `should` / `min_should`:
        term constraints (``term_filter``), ANDed with `filter` when both are given."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        if must is not None or must_not is not None or should is not None or min_should is not None:
            terms = self.term_filter(must=must, must_not=must_not, should=should, min_should=min_should, index=index)
            if filter is not None:
                from ...doc_filter import as_doc_filter
                filter = as_doc_filter(filter, terms.n_rows, device=terms.device) & terms
            else:
                filter = terms
        a = a or self.encoder_q.config.topk
        q_emb = self.process_query(queries, dropout, a, batch_size=batch_size)
        results = index.search(q_emb, k=k, filter=filter) if filter is not None else index.search(q_emb, k=k)
        if rerank and index.index_type == IndexType.BAG_OF_TOKEN:
            results = self._rerank(index, q_emb, results, k, batch_size)
        return results

    def retrieve_grouped(self, queries: Union[List[str], np.ndarray, T], k: int = 5, per_group: int = 1, dropout: float = 0, a: int = None,
                         index: Index = None, batch_size: int = 32, filter=None, must=None, must_not=None, should=None,
                         min_should: int = None, depth: int = None) -> GroupedResults:
        """The top k GROUPS of documents per query (``index.set_groups`` / ``groups_from_samples``: the articles of a passage index),
        each with its best `per_group` documents -- ``Index.search_grouped`` behind the query encoder.  Exact: the collapse of the complete
        ranking, not of a deeper top-k.  `filter` and the term constraints as in ``retrieve``."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        if must is not None or must_not is not None or should is not None or min_should is not None:
            terms = self.term_filter(must=must, must_not=must_not, should=should, min_should=min_should, index=index)
            if filter is not None:
                from ...doc_filter import as_doc_filter
                filter = as_doc_filter(filter, terms.n_rows, device=terms.device) & terms
            else:
                filter = terms
        a = a or self.encoder_q.config.topk
        q_emb = self.process_query(queries, dropout, a, batch_size=batch_size)
        return index.search_grouped(q_emb, k=k, per_group=per_group, filter=filter, depth=depth)

    def retrieve_range(self, queries: Union[List[str], np.ndarray, T], min_score, max_hits: int = 100, dropout: float = 0, a: int = None,
                       index: Index = None, batch_size: int = 32, filter=None, must=None, must_not=None, should=None,
                       min_should: int = None) -> RangeResults:
        """Every document scoring at least `min_score` per query, counted -- ``Index.search_range`` behind the query encoder: the exact
        number of matches and the first `max_hits` of them in the canonical order.  `filter` and the term constraints as in ``retrieve``."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        if must is not None or must_not is not None or should is not None or min_should is not None:
            terms = self.term_filter(must=must, must_not=must_not, should=should, min_should=min_should, index=index)
            if filter is not None:
                from ...doc_filter import as_doc_filter
                filter = as_doc_filter(filter, terms.n_rows, device=terms.device) & terms
            else:
                filter = terms
        a = a or self.encoder_q.config.topk
        q_emb = self.process_query(queries, dropout, a, batch_size=batch_size)
        return index.search_range(q_emb, min_score, max_hits=max_hits, filter=filter)

    def retrieve_boosted(self, queries: Union[List[str], np.ndarray, T], k: int = 5, boosts=None, mode: str = "add", min_score=None,
                         dropout: float = 0, a: int = None, index: Index = None, batch_size: int = 32, filter=None, must=None, must_not=None,
                         should=None, min_should: int = None) -> RangeResults:
        """The exact top k by relevance and value fields together -- ``Index.search_boosted`` behind the query encoder:
        boosts={"recency": 0.3, "views": 0.1} adds (mode="add") or multiplies in (mode="mul") a weighted sum of the documents' values.
        Every document is scored, so no hit is lost behind a rescore window.  `filter` and the term constraints as in ``retrieve``."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        if must is not None or must_not is not None or should is not None or min_should is not None:
            terms = self.term_filter(must=must, must_not=must_not, should=should, min_should=min_should, index=index)
            if filter is not None:
                from ...doc_filter import as_doc_filter
                filter = as_doc_filter(filter, terms.n_rows, device=terms.device) & terms
            else:
                filter = terms
        a = a or self.encoder_q.config.topk
        q_emb = self.process_query(queries, dropout, a, batch_size=batch_size)
        return index.search_boosted(q_emb, k=k, boosts=boosts, mode=mode, min_score=min_score, filter=filter)

    def retrieve_facets(self, queries: Union[List[str], np.ndarray, T], field: str, min_score, topn: int = 10, min_count: int = 1,
                        dropout: float = 0, a: int = None, index: Index = None, batch_size: int = 32, filter=None, must=None, must_not=None,
                        should=None, min_should: int = None):
        """How each query's matches spread over facet field `field` (``index.set_facet`` / ``facet_from_samples``) -- ``Index.facets`` behind
        the query encoder: the matches are the documents scoring at least `min_score`, exactly as in ``retrieve_range``; `filter` and the
        term constraints act through that match set.  -> (facets, totals): facets[b] is the list of (name, count) of query b's `topn`
        labels with the most matches (the label's code where the field has no names), count descending; totals[b] the number of matches."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        if must is not None or must_not is not None or should is not None or min_should is not None:
            terms = self.term_filter(must=must, must_not=must_not, should=should, min_should=min_should, index=index)
            if filter is not None:
                from ...doc_filter import as_doc_filter
                filter = as_doc_filter(filter, terms.n_rows, device=terms.device) & terms
            else:
                filter = terms
        a = a or self.encoder_q.config.topk
        q_emb = self.process_query(queries, dropout, a, batch_size=batch_size)
        top = index.facets(field, q_emb, min_score, filter=filter, topn=topn, min_count=min_count)
        names = index.facet_names(field)
        labels, counts, totals = top.labels.cpu().tolist(), top.counts.cpu().tolist(), top.total.cpu().tolist()
        facets = [[(names[l] if names is not None else l, c) for l, c in zip(ls, cs) if l >= 0] for ls, cs in zip(labels, counts)]
        return facets, totals

    def _match_set(self, queries, index, filter, must, must_not, should, min_should, dropout, a, batch_size):
        """the index, the query embeddings and the filter (term constraints ANDed in) of a retrieve_* call over the match set"""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        if must is not None or must_not is not None or should is not None or min_should is not None:
            terms = self.term_filter(must=must, must_not=must_not, should=should, min_should=min_should, index=index)
            if filter is not None:
                from ...doc_filter import as_doc_filter
                filter = as_doc_filter(filter, terms.n_rows, device=terms.device) & terms
            else:
                filter = terms
        a = a or self.encoder_q.config.topk
        return index, self.process_query(queries, dropout, a, batch_size=batch_size), filter

    def value_filter(self, field: str, lo=None, hi=None, index: Index = None):
        """``Index.value_filter``: the documents with lo <= value <= hi of value field `field` (None: an open end) as a DocFilter, to be passed
        as ``filter=`` to any retrieve_* call; it composes with ``term_filter`` through ``&``."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        return index.value_filter(field, lo, hi)

    def retrieve_sorted(self, queries: Union[List[str], np.ndarray, T], field: str, k: int = 5, min_score=0.0, descending: bool = True,
                        dropout: float = 0, a: int = None, index: Index = None, batch_size: int = 32, filter=None, must=None, must_not=None,
                        should=None, min_should: int = None):
        """The k matches of each query with the largest (descending) or smallest values of value field `field` -- sort by a field instead
        of by score, ``Index.top_by_value`` behind the query encoder: the matches are the documents scoring at least `min_score`, exactly
        as in ``retrieve_range``; `filter` and the term constraints as in ``retrieve``.  -> SortedResults(ids [B, k], values [B, k])."""
        index, q_emb, filter = self._match_set(queries, index, filter, must, must_not, should, min_should, dropout, a, batch_size)
        return index.top_by_value(field, k, descending=descending, q_embs=q_emb, min_score=min_score, filter=filter)

    def retrieve_ids(self, queries: Union[List[str], np.ndarray, T], min_score, offset=0, limit: int = None, dropout: float = 0, a: int = None,
                     index: Index = None, batch_size: int = 32, filter=None, must=None, must_not=None, should=None, min_should: int = None):
        """EVERY match of each query as ids in ascending order -- ``Index.list_ids`` behind the query encoder, where ``retrieve_range`` stops
        at 2048 hits: the matches are the documents scoring at least `min_score`; `filter` and the term constraints as in ``retrieve``.
        -> SetIds(ids [B, limit], counts [B]); limit=None: the largest count; `offset` pages through a longer list."""
        index, q_emb, filter = self._match_set(queries, index, filter, must, must_not, should, min_should, dropout, a, batch_size)
        return index.list_ids(q_embs=q_emb, min_score=min_score, filter=filter, offset=offset, limit=limit)

    def sample_band(self, queries: Union[List[str], np.ndarray, T], lo, hi, n: int, seed: int = 0, dropout: float = 0, a: int = None,
                    index: Index = None, batch_size: int = 32, filter=None, must=None, must_not=None, should=None, min_should: int = None,
                    return_texts: bool = True):
        """n documents per query scoring in [lo, hi) -- the hard-negative band as one call: match_filter(lo) & ~match_filter(hi), sampled
        uniformly and reproducibly under `seed` (``Index.sample_ids``).  -> (SetSample(ids [B, n], counts [B]), texts): texts[b] lists the
        samples' documents (``index.get_sample``) in the order of ids[b], without the -1 padding; None when return_texts is False or the
        index has no data file."""
        index, q_emb, filter = self._match_set(queries, index, filter, must, must_not, should, min_should, dropout, a, batch_size)
        band = index.match_filter(q_emb, lo, filter=filter) & ~index.match_filter(q_emb, hi)
        res = index.sample_ids(n, filter=band, seed=seed)
        texts = None
        if return_texts and len(index):
            texts = [[index.get_sample(int(i)) for i in row if i >= 0] for row in res.ids.cpu().tolist()]
        return res, texts

    def retrieve_histogram(self, queries: Union[List[str], np.ndarray, T], field: str, edges, min_score=0.0, dropout: float = 0, a: int = None,
                           index: Index = None, batch_size: int = 32, filter=None, must=None, must_not=None, should=None,
                           min_should: int = None):
        """How each query's matches spread over the bins of value field `field` -- ``Index.histogram`` behind the query encoder, the match
        set as in ``retrieve_sorted`` -> ValueHistogram(counts [B, E - 1], below, above, missing, total)."""
        index, q_emb, filter = self._match_set(queries, index, filter, must, must_not, should, min_should, dropout, a, batch_size)
        return index.histogram(field, edges, q_embs=q_emb, min_score=min_score, filter=filter)

    def retrieve_score_histogram(self, queries: Union[List[str], np.ndarray, T], edges, min_score=None, **filters):
        """How each query's SCORES spread over the bins [edges[i], edges[i + 1]) -- ``retrieve_histogram(queries, SCORE, edges, ...)``: where a
        relevance cut-off should sit, counts at every threshold from one call.  min_score=None: over every document `filters` (filter=,
        must=, ... and the other keywords of ``retrieve_histogram``) leave; else over the matches.  ``retrieve_percentiles``,
        ``retrieve_sorted``, ``retrieve_stats_by_facet`` and ``retrieve_histogram_by_facet`` take SCORE as their field the same way."""
        return self.retrieve_histogram(queries, SCORE, edges, min_score=min_score, **filters)

    def retrieve_stats_by_facet(self, queries: Union[List[str], np.ndarray, T], value_field: str, facet_field: str, min_score=0.0, topn: int = 10,
                                min_count: int = 1, dropout: float = 0, a: int = None, index: Index = None, batch_size: int = 32, filter=None,
                                must=None, must_not=None, should=None, min_should: int = None):
        """The stats of value field `value_field` per label of `facet_field` over each query's matches -- ``Index.stats_by_facet`` behind the
        query encoder, the match set as in ``retrieve_histogram`` -> (rows, totals): rows[b] lists (name, docs, count, min, max, mean) for the
        `topn` labels with the most documents of the set (docs = count + missing, at least max(min_count, 1)), docs descending then label
        ascending; name is the label's code where the field has no names; min / max are None and mean is NaN where no document of the label
        has a value; totals[b] is the number of matches."""
        from ...device_index import facet_topn, _topn_args
        topn, min_count = _topn_args(topn, min_count)
        index, q_emb, filter = self._match_set(queries, index, filter, must, must_not, should, min_should, dropout, a, batch_size)
        st = index.stats_by_facet(value_field, facet_field, q_embs=q_emb, min_score=min_score, filter=filter)
        docs = st.count + st.missing
        top_l, top_c = facet_topn(docs if docs.is_cuda else docs.numpy(), topn, min_count, device=index._explain_target()[1])
        top_l, top_c = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (top_l, top_c))
        names = index.facet_names(facet_field)
        count, lo, hi, mean = st.count.cpu().numpy(), st.min.cpu().numpy(), st.max.cpu().numpy(), st.mean().cpu().numpy()
        rows = []
        for b in range(top_l.shape[0]):
            out = []
            for l, d in zip(top_l[b].tolist(), top_c[b].tolist()):
                if l < 0:
                    continue
                c = int(count[b, l])
                out.append((names[l] if names is not None else l, d, c, lo[b, l].item() if c else None, hi[b, l].item() if c else None,
                            float(mean[b, l])))
            rows.append(out)
        return rows, st.total.cpu().tolist()

    def retrieve_histogram_by_facet(self, queries: Union[List[str], np.ndarray, T], value_field: str, facet_field: str, edges, min_score=0.0,
                                    dropout: float = 0, a: int = None, index: Index = None, batch_size: int = 32, filter=None, must=None,
                                    must_not=None, should=None, min_should: int = None):
        """How each query's matches spread over (label of `facet_field`, bin of `value_field`) -- ``Index.histogram_by_facet`` behind the query
        encoder, the match set as in ``retrieve_histogram`` -> FacetValueHistogram(counts [B, n_labels, E - 1], below, above, missing, total,
        other)."""
        index, q_emb, filter = self._match_set(queries, index, filter, must, must_not, should, min_should, dropout, a, batch_size)
        return index.histogram_by_facet(value_field, facet_field, edges, q_embs=q_emb, min_score=min_score, filter=filter)

    def retrieve_percentiles_by_facet(self, queries: Union[List[str], np.ndarray, T], value_field: str, facet_field: str, pcts, min_score=0.0,
                                      topn: int = 10, min_count: int = 1, method: str = "linear", dropout: float = 0, a: int = None,
                                      index: Index = None, batch_size: int = 32, filter=None, must=None, must_not=None, should=None,
                                      min_should: int = None):
        """Exact percentiles of value field `value_field` per label of `facet_field` over each query's matches --
        ``Index.percentiles_by_facet`` behind the query encoder, the match set as in ``retrieve_histogram`` -> (rows, totals): rows[b] lists
        (name, docs, count, percentiles) for the `topn` labels with the most documents of the set (docs = count + missing, at least
        max(min_count, 1)), docs descending then label ascending; name is the label's code where the field has no names; percentiles is the
        list of the P values (NaN / the missing sentinel where no document of the label has a value); totals[b] is the number of matches."""
        from ...device_index import facet_topn, _topn_args
        topn, min_count = _topn_args(topn, min_count)
        index, q_emb, filter = self._match_set(queries, index, filter, must, must_not, should, min_should, dropout, a, batch_size)
        res = index.percentiles_by_facet(value_field, facet_field, pcts, q_embs=q_emb, min_score=min_score, filter=filter, method=method)
        docs = res.count + res.missing
        top_l, top_c = facet_topn(docs if docs.is_cuda else docs.numpy(), topn, min_count, device=index._explain_target()[1])
        top_l, top_c = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (top_l, top_c))
        names = index.facet_names(facet_field)
        count, vals = res.count.cpu().numpy(), res.values.cpu().numpy()
        rows = []
        for b in range(top_l.shape[0]):
            out = []
            for l, d in zip(top_l[b].tolist(), top_c[b].tolist()):
                if l < 0:
                    continue
                out.append((names[l] if names is not None else l, d, int(count[b, l]), vals[b, l].tolist()))
            rows.append(out)
        return rows, res.total.cpu().tolist()

    def retrieve_percentiles(self, queries: Union[List[str], np.ndarray, T], field: str, pcts, min_score=0.0, method: str = "linear",
                             dropout: float = 0, a: int = None, index: Index = None, batch_size: int = 32, filter=None, must=None, must_not=None,
                             should=None, min_should: int = None):
        """Exact percentiles of value field `field` over each query's matches -- ``Index.percentiles`` behind the query encoder, the match
        set as in ``retrieve_sorted`` -> ValuePercentiles(values [B, P], count, missing); pcts in 0..100."""
        index, q_emb, filter = self._match_set(queries, index, filter, must, must_not, should, min_should, dropout, a, batch_size)
        return index.percentiles(field, pcts, q_embs=q_emb, min_score=min_score, filter=filter, method=method)

    def significant_terms(self, queries: Union[List[str], np.ndarray, T], min_score=None, k: int = None, topn: int = 20, method: str = "jlh",
                          min_count: int = 1, background=None, dropout: float = 0, a: int = None, index: Index = None, batch_size: int = 32,
                          filter=None, must=None, must_not=None, should=None, min_should: int = None):
        """What each query's results are about -- ``Index.significant_terms`` behind the query encoder: the vocabulary tokens
        over-represented in the result set against the whole index.  Exactly one of `min_score` (the set is every document scoring at
        least it, as in ``retrieve_range``) and `k` (the set is ``retrieve``'s top k hits) must be given.  -> per query the list of
        (token, score, df, bg), most significant first: df documents of the set and bg documents of the background have the token.
        `method`, `min_count`, `background` as in ``Index.significant_terms``; `filter` and the term constraints as in ``retrieve_facets``."""
        if (min_score is None) == (k is None):
            raise ValueError("exactly one of min_score (the match set) and k (the top-k hits) must be given")
        if method not in ("jlh", "lift", "count"):
            raise ValueError(f'method must be "jlh", "lift" or "count", got {method!r}')
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        if must is not None or must_not is not None or should is not None or min_should is not None:
            terms = self.term_filter(must=must, must_not=must_not, should=should, min_should=min_should, index=index)
            if filter is not None:
                from ...doc_filter import as_doc_filter
                filter = as_doc_filter(filter, terms.n_rows, device=terms.device) & terms
            else:
                filter = terms
        a = a or self.encoder_q.config.topk
        q_emb = self.process_query(queries, dropout, a, batch_size=batch_size)
        if k is not None:
            hits = index.search(q_emb, k=k, filter=filter) if filter is not None else index.search(q_emb, k=k)
            top = index.significant_terms(ids=hits.ids, topn=topn, method=method, min_count=min_count, background=background)
        else:
            top = index.significant_terms(q_emb, min_score, filter=filter, topn=topn, method=method, min_count=min_count, background=background)
        shift = int(self.encoder_p.config.shift_vocab_num)
        tok = self.encoder_p.tokenizer
        cols, scores, df, bg = (t.cpu().numpy() for t in (top.cols, top.scores, top.df, top.bg))
        out = []
        for b in range(cols.shape[0]):
            live = cols[b] >= 0
            names = tok.convert_ids_to_tokens([int(x) + shift for x in cols[b][live]])
            out.append([(name, float(s), int(d), int(g)) for name, s, d, g in zip(names, scores[b][live], df[b][live], bg[b][live])])
        return out

    def centroid_terms(self, queries: Union[List[str], np.ndarray, T], min_score=None, k: int = None, topn: int = 20, min_count: int = 0,
                       dropout: float = 0, a: int = None, index: Index = None, batch_size: int = 32, filter=None, must=None, must_not=None,
                       should=None, min_should: int = None):
        """What each query's results weigh most -- ``Index.centroid_terms`` behind the query encoder: the vocabulary tokens with the
        largest mean weight over the result set (its centroid's largest coordinates).  Exactly one of `min_score` (the set is every
        document scoring at least it, as in ``retrieve_range``) and `k` (the set is ``retrieve``'s top k hits) must be given.  -> per query
        the list of (token, mean_weight, sum), heaviest first: sum is the fixed-point column sum (weights times 2^24).  `min_count` as in
        ``Index.centroid_terms``; `filter` and the term constraints as in ``retrieve_facets``."""
        if (min_score is None) == (k is None):
            raise ValueError("exactly one of min_score (the match set) and k (the top-k hits) must be given")
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        if must is not None or must_not is not None or should is not None or min_should is not None:
            terms = self.term_filter(must=must, must_not=must_not, should=should, min_should=min_should, index=index)
            if filter is not None:
                from ...doc_filter import as_doc_filter
                filter = as_doc_filter(filter, terms.n_rows, device=terms.device) & terms
            else:
                filter = terms
        a = a or self.encoder_q.config.topk
        q_emb = self.process_query(queries, dropout, a, batch_size=batch_size)
        if k is not None:
            hits = index.search(q_emb, k=k, filter=filter) if filter is not None else index.search(q_emb, k=k)
            top = index.centroid_terms(ids=hits.ids, topn=topn, min_count=min_count)
        else:
            top = index.centroid_terms(q_emb, min_score, filter=filter, topn=topn, min_count=min_count)
        shift = int(self.encoder_p.config.shift_vocab_num)
        tok = self.encoder_p.tokenizer
        cols, scores, sums = (t.cpu().numpy() for t in (top.cols, top.scores, top.sums))
        out = []
        for b in range(cols.shape[0]):
            live = cols[b] >= 0
            names = tok.convert_ids_to_tokens([int(x) + shift for x in cols[b][live]])
            out.append([(name, float(s), int(d)) for name, s, d in zip(names, scores[b][live], sums[b][live])])
        return out

    def facet_terms(self, field: str, queries: Union[List[str], np.ndarray, T] = None, min_score=None, topn: int = 10, method: str = "weight",
                    min_count: int = None, background=None, dropout: float = 0, a: int = None, index: Index = None, batch_size: int = 32,
                    filter=None):
        """What every label of facet field `field` is about, for all labels at once -- ``Index.centroid_terms_by_facet`` (method "weight":
        the tokens the label's documents put the most weight on) or ``Index.significant_terms_by_facet`` ("jlh" | "lift" | "count": the
        tokens over-represented in them) behind the query encoder -> {label name: (docs, [(token, score), ...])}, docs the documents of
        the set with that label; name is the label's code where the field has no names.  The set: ONE query with `min_score` (its matches),
        `filter` alone, or neither: every live document.  min_count: None = the method's default (0 for "weight", 1 otherwise)."""
        if method not in ("weight", "jlh", "lift", "count"):
            raise ValueError(f'method must be "weight", "jlh", "lift" or "count", got {method!r}')
        if (queries is None) != (min_score is None):
            raise ValueError("queries and min_score go together: the set is one query's matches, the filter alone, or every live document")
        if queries is not None and not isinstance(queries, str) and len(queries) != 1:
            raise ValueError("facet_terms takes ONE document set: one query, not a batch")
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        q_emb = None
        if queries is not None:
            q_emb = self.process_query([queries] if isinstance(queries, str) else queries, dropout, a or self.encoder_q.config.topk,
                                       batch_size=batch_size)
        if method == "weight":
            top = index.centroid_terms_by_facet(field, topn=topn, min_count=0 if min_count is None else min_count, q_embs=q_emb,
                                                min_score=min_score, filter=filter)
        else:
            top = index.significant_terms_by_facet(field, topn=topn, method=method, min_count=1 if min_count is None else min_count,
                                                   background=background, q_embs=q_emb, min_score=min_score, filter=filter)
        names = index.facet_names(field)
        shift = int(self.encoder_p.config.shift_vocab_num)
        tok = self.encoder_p.tokenizer
        cols, scores, total = (t.cpu().numpy() for t in (top.cols, top.scores, top.total))
        out = {}
        for l in range(cols.shape[0]):
            live = cols[l] >= 0
            toks = tok.convert_ids_to_tokens([int(x) + shift for x in cols[l][live]])
            out[names[l] if names is not None else l] = (int(total[l]), [(t, float(s)) for t, s in zip(toks, scores[l][live])])
        return out

    def cluster_documents(self, n_clusters: int, topn: int = 10, index: Index = None, **args):
        """Partition the indexed documents into `n_clusters` clusters (``Index.cluster``: Lloyd's k-means on the GPU, the labels stored as
        facet field "cluster") and name every cluster by its tokens -> per cluster (size, [(token, mean weight), ...]), the vocabulary
        tokens its documents put the most weight on, heaviest first.  **args go to ``Index.cluster`` (iters, metric, init, seed, filter,
        field, set_groups)."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        res = index.cluster(n_clusters, **args)
        top = index.cluster_terms(res.labels, n_clusters, topn=topn)
        shift = int(self.encoder_p.config.shift_vocab_num)
        tok = self.encoder_p.tokenizer
        cols, scores, total = (t.cpu().numpy() for t in (top.cols, top.scores, top.total))
        out = []
        for j in range(cols.shape[0]):
            live = cols[j] >= 0
            names = tok.convert_ids_to_tokens([int(x) + shift for x in cols[j][live]])
            out.append((int(total[j]), [(name, float(s)) for name, s in zip(names, scores[j][live])]))
        return out

    def retrieve_diverse(self, queries: Union[List[str], np.ndarray, T], k: int = 5, lam: float = 0.5, depth: int = None, sim: str = "cosine",
                         dropout: float = 0, a: int = None, index: Index = None, batch_size: int = 32, filter=None, must=None, must_not=None,
                         should=None, min_should: int = None) -> DiverseResults:
        """The top k documents per query with near-duplicates pushed down -- ``Index.search_diverse`` (Maximal Marginal Relevance over the
        top `depth` hits, similarities between the stored rows) behind the query encoder.  lam = 1 is ``retrieve``; `filter` and the term
        constraints as in ``retrieve``."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        if must is not None or must_not is not None or should is not None or min_should is not None:
            terms = self.term_filter(must=must, must_not=must_not, should=should, min_should=min_should, index=index)
            if filter is not None:
                from ...doc_filter import as_doc_filter
                filter = as_doc_filter(filter, terms.n_rows, device=terms.device) & terms
            else:
                filter = terms
        a = a or self.encoder_q.config.topk
        q_emb = self.process_query(queries, dropout, a, batch_size=batch_size)
        return index.search_diverse(q_emb, k=k, lam=lam, depth=depth, sim=sim, filter=filter)

    def retrieve_fused(self, query_variants, k: int = 5, method: str = "rrf", weights=None, c: float = 60.0, depth: int = None,
                       dropout: float = 0, a: int = None, index: Index = None, batch_size: int = 32, filter=None, must=None, must_not=None,
                       should=None, min_should: int = None) -> SearchResults:
        """One answer to several phrasings: `query_variants` is a list of L query lists (or embedding tensors), each of length B -- variant l
        of query b is query_variants[l][b].  Every variant batch is searched and the L hit lists of a query are fused on the GPU
        (``Index.search_fused``: "rrf" by default).  -> SearchResults(ids, scores), the fused value as the score.  `filter` and the term
        constraints as in ``retrieve``: they apply to every variant's search."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        if must is not None or must_not is not None or should is not None or min_should is not None:
            terms = self.term_filter(must=must, must_not=must_not, should=should, min_should=min_should, index=index)
            if filter is not None:
                from ...doc_filter import as_doc_filter
                filter = as_doc_filter(filter, terms.n_rows, device=terms.device) & terms
            else:
                filter = terms
        a = a or self.encoder_q.config.topk
        q_embs = [self.process_query(q, dropout, a, batch_size=batch_size) for q in query_variants]
        res = index.search_fused(q_embs, k=k, method=method, weights=weights, c=c, depth=depth, filter=filter)
        return SearchResults(res.ids, res.fused)

    def retrieve_hybrid(self, queries: Union[List[str], np.ndarray, T], k: int = 5, indexes: List[Index] = None, weights=None, method: str = "rrf",
                        c: float = 60.0, depth: int = None, missing: str = "zero", dropout: float = 0, a: int = None, batch_size: int = 32,
                        filter=None, must=None, must_not=None, should=None, min_should: int = None) -> FusedResults:
        """The same queries against several indexes over the same documents (`indexes`: the valued index and the bag-of-token index of a
        corpus; default: the retriever's own alone), fused on the GPU -- ``Index.search_hybrid`` behind the query encoder.  `missing`:
        "zero" | "score" (method "raw": every hit carries its true weighted sum).  `filter` and the term constraints as in ``retrieve``."""
        indexes = list(indexes) if indexes else [self.index]
        if indexes[0] is None:
            raise RuntimeError("no index: call build_index / load_index first")
        first = indexes[0]
        if must is not None or must_not is not None or should is not None or min_should is not None:
            terms = self.term_filter(must=must, must_not=must_not, should=should, min_should=min_should, index=first)
            if filter is not None:
                from ...doc_filter import as_doc_filter
                filter = as_doc_filter(filter, terms.n_rows, device=terms.device) & terms
            else:
                filter = terms
        a = a or self.encoder_q.config.topk
        q_emb = self.process_query(queries, dropout, a, batch_size=batch_size)
        return first.search_hybrid(q_emb, [(idx, None) for idx in indexes[1:]], k, method=method, weights=weights, c=c, depth=depth, filter=filter,
                                   missing=missing)

    def term_filter(self, must=None, must_not=None, should=None, min_should: int = None, thr=None, index: Index = None):
        """Index.term_filter with terms given as column ids or as vocabulary tokens (strings): a string is looked up in the passage
        tokenizer's vocabulary and its column is token id - shift.  A string that is not one vocabulary entry (a longer word: pass its word
        pieces), or whose id lies below the shift, raises ValueError.  thr: {column id or token: threshold}."""
        from ...doc_filter import terms_to_columns
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        vocab = self.encoder_p.tokenizer.vocab
        shift = int(self.encoder_p.config.shift_vocab_num)
        cols = {name: terms_to_columns(x, vocab, shift, name) for name, x in (("must", must), ("must_not", must_not), ("should", should))}
        if thr is not None:
            thr = dict(zip(terms_to_columns(list(thr), vocab, shift, "thr"), thr.values()))
        return index.term_filter(must=cols["must"], must_not=cols["must_not"], should=cols["should"], min_should=min_should, thr=thr)

    def explain_results(self, queries: Union[List[str], np.ndarray, T], results: SearchResults, topn: int = 10, index: Index = None,
                        a: int = None, batch_size: int = 32) -> List[List[Dict[str, float]]]:
        """Why each hit of `results` (from ``retrieve``) was returned: per query, per hit, token -> contribution q_w * p_w, largest
        first -- the shape ``explain`` returns -- read from the index rows on the device (Index.explain), not re-embedded.  `queries`:
        texts or embeddings, as ``retrieve`` takes them.  Padding hits (id -1) give {}."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        a = a or self.encoder_q.config.topk
        q_emb = self.process_query(queries, 0, a, batch_size=batch_size)
        ex = index.explain(q_emb, results.ids, topn=topn)
        cols, contrib = ex.cols.cpu().numpy(), ex.contrib.cpu().numpy()
        ids = results.ids.cpu().numpy() if isinstance(results.ids, T) else np.asarray(results.ids)
        shift = int(self.encoder_p.config.shift_vocab_num)
        tok = self.encoder_p.tokenizer
        out: List[List[Dict[str, float]]] = []
        for b in range(cols.shape[0]):
            row = []
            for j in range(cols.shape[1]):
                live = cols[b, j] >= 0
                if ids.ndim == 2 and ids[b, j] < 0 or not live.any():
                    row.append({})
                    continue
                c = cols[b, j][live]
                names = tok.convert_ids_to_tokens([int(x) + shift for x in c])
                row.append({name: float(v) for name, v in zip(names, contrib[b, j][live])})
            out.append(row)
        return out

    def more_like_this(self, ids, k: int = 5, exclude: bool = True, filter=None, a: int = None, index: Index = None) -> SearchResults:
        """Documents like the given ones, with no encoder: ids [B] (one query per document) or [B, m] (the sum of m documents' rows a
        query) are searched as queries (Index.search_by_example); `exclude` leaves each query's own documents out of its hits, `a` keeps
        only the a largest entries of each query."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        if isinstance(ids, (list, tuple)):
            ids = torch.as_tensor(ids, dtype=torch.int64)
        elif isinstance(ids, np.ndarray):
            ids = torch.from_numpy(ids)
        if isinstance(ids, T) and ids.dim() == 1:
            ids = ids.unsqueeze(1)
        return index.search_by_example(ids, k, a=a, exclude=exclude, filter=filter)

    def retrieve_with_feedback(self, queries: Union[List[str], np.ndarray, T], k: int = 5, fb_docs: int = 10, fb_weight: float = 0.75,
                               a: int = None, filter=None, rerank: bool = False, batch_size: int = 32, index: Index = None) -> SearchResults:
        """Rocchio pseudo-relevance feedback: retrieve the top `fb_docs` hits of each query, form q' = q + (fb_weight / m_b) * (sum of
        their stored rows) -- m_b the query's real (non-padding) hits; every add rounded to fp32, Index.queries_from_rows --, keep the `a`
        largest entries of q' (default: the encoder's topk, so q' costs what an encoded query costs) and search the top k.  The feedback
        documents stay eligible.  `filter` restricts both searches; `rerank` as in ``retrieve`` (against the original query)."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        a = a or self.encoder_q.config.topk
        q_emb = self.process_query(queries, 0, a, batch_size=batch_size)
        if q_emb.dim() == 1:
            q_emb = q_emb.unsqueeze(0)
        first = index.search(q_emb, k=fb_docs, filter=filter) if filter is not None else index.search(q_emb, k=fb_docs)
        fb_ids = first.ids
        m_b = (fb_ids >= 0).sum(dim=1, keepdim=True).clamp(min=1).to(torch.float64)
        w = (float(fb_weight) / m_b).to(torch.float32).expand(fb_ids.shape).contiguous()
        q_fb = index.queries_from_rows(fb_ids, weights=w, q=q_emb, alpha=1.0)
        q_fb = q_fb.masked_fill(~sp.build_topk_mask(q_fb, k=int(a)), 0.0)
        results = index.search(q_fb, k=k, filter=filter) if filter is not None else index.search(q_fb, k=k)
        if rerank and index.index_type == IndexType.BAG_OF_TOKEN:
            results = self._rerank(index, q_emb, results, k, batch_size)
        return results

    def _rerank(self, index: Index, q_emb: T, results: SearchResults, k: int, batch_size: int) -> SearchResults:
        """Re-embed the k hits with encoder_p, score against q, re-sort (retriever.py:137-147) -- on the device:
        ``vs_rerank_scores`` per re-embedding batch (the reference's dense [B*k, V] tensor is never held) and
        ``vs_rerank_topk`` for the order (score descending; equal scores keep their first-stage order)."""
        import ctypes as C
        from ... import _native as nat
        from ...device_index import current_stream
        hit_ids = results.ids
        B = int(hit_ids.shape[0])
        flat_ids = hit_ids.flatten().tolist()
        texts = [index.get_sample(i) if i >= 0 else None for i in flat_ids]         # (id -1: a filtered search's padding, never re-embedded)
        nat.require_device()
        dev = hit_ids.device if hit_ids.is_cuda else torch.device("cuda", 0)
        ordinal = dev.index or 0
        stream = current_stream(ordinal)
        q = q_emb.to(dev).to(torch.float32).contiguous()
        ids_dev = hit_ids.to(dev).contiguous()
        scores = torch.empty((B, k), dtype=torch.float32, device=dev)
        chunk = max(int(batch_size), 1) * 32               # re-embedded passages held at a time
        for r0 in range(0, B * k, chunk):
            part = texts[r0:r0 + chunk]
            live = [i for i, t in enumerate(part) if t is not None]
            if not live:
                continue                                    # (all padding: its scores are set to -inf below)
            p_emb = self.encoder_p.embed([part[i] for i in live], batch_size=batch_size, require_grad=False)
            if p_emb.dtype not in (torch.float32, torch.float16):
                p_emb = p_emb.to(torch.float32)
            p_emb = p_emb.to(dev)
            if len(live) < len(part):                       # padding rows: zeros in the batch, their scores overwritten below
                full = torch.zeros((len(part), p_emb.shape[1]), dtype=p_emb.dtype, device=dev)
                full[torch.as_tensor(live, device=dev)] = p_emb
                p_emb = full
            p_emb = p_emb.contiguous()
            nat.check(nat.lib().vs_rerank_scores(C.c_void_p(p_emb.data_ptr()), nat.VS_F16 if p_emb.dtype == torch.float16 else nat.VS_F32,
                                                 int(p_emb.shape[1]), int(p_emb.shape[0]), r0, C.c_void_p(q.data_ptr()), int(q.shape[1]), B, int(k),
                                                 int(q.shape[1]), C.c_void_p(scores.data_ptr()), ordinal, stream))
        if (ids_dev < 0).any():
            scores = scores.masked_fill(ids_dev < 0, float("-inf"))   # padding stays behind every real hit (and keeps its order)
        out_ids = torch.empty_like(ids_dev)
        out_scores = torch.empty_like(scores)
        nat.check(nat.lib().vs_rerank_topk(C.c_void_p(scores.data_ptr()), C.c_void_p(ids_dev.data_ptr()), B, int(k), C.c_void_p(out_ids.data_ptr()),
                                           C.c_void_p(out_scores.data_ptr()), ordinal, stream))
        return SearchResults(out_ids, out_scores)

    def retireve_negatives(self, *args, **kwargs):
        """Hard-negative mining for the reference's TRAINING loop (retriever.py:150-205, called from forward() at :51): out of this
        build's scope (the retrieval hot path, no training).  Present so that a caller gets a clear message, not an
        AttributeError."""
        raise NotImplementedError("Retriever.retireve_negatives (hard-negative mining for training, reference retriever.py:150-205) is not part of "
                                  "the MI355X retrieval path; use retrieve() and filter the hits")

    retrieve_negatives = retireve_negatives

    # ---- index build (retriever.py:208-317) ----------------------------------------------------------
    def _tokenize_for_bot(self, texts: List[str], max_len: int):
        return self.encoder_p.tokenizer(texts, max_length=max_len, truncation=True)["input_ids"]

    def _build_bot_vectors(self, texts: List[str], batch_size: int = 32, max_len: int = 128, max_token: int = None,
                           num_shift: int = 999, fp16: int = True):
        """Binary bag-of-token CSR of the corpus (retriever.py:208-253): per document the set of token ids
        >= num_shift (optionally only the first `max_token` distinct ids, [CLS] included in the count)."""
        import ctypes as C
        vocab = len(self.encoder_p.tokenizer.vocab)
        token_lists = []
        for s in range(0, len(texts), batch_size):
            token_lists.extend(self._tokenize_for_bot(texts[s:s + batch_size], max_len))
        offsets = np.zeros(len(token_lists) + 1, dtype=np.int64)
        np.cumsum([len(t) for t in token_lists], out=offsets[1:])
        tokens = (np.concatenate([np.asarray(t, dtype=np.int32) for t in token_lists]) if token_lists else np.zeros(0, np.int32))
        tokens = np.ascontiguousarray(tokens)
        n = len(token_lists)
        indptr = np.empty(n + 1, dtype=np.int64)
        args = (C.c_void_p(tokens.ctypes.data), C.c_void_p(offsets.ctypes.data), n, int(vocab), int(num_shift), int(max_token or 0))
        try:
            nat.check(nat.lib().vs_bot_build(*args, C.c_void_p(indptr.ctypes.data), None))
        except ValueError as e:
            raise IndexError(str(e)) from None
        indices = np.empty(max(int(indptr[-1]), 1), dtype=np.int32)
        nat.check(nat.lib().vs_bot_build(*args, C.c_void_p(indptr.ctypes.data), C.c_void_p(indices.ctypes.data)))
        indices = indices[:int(indptr[-1])]
        values = torch.ones(indices.shape[0], dtype=torch.float16 if fp16 else torch.float32)
        return torch.sparse_csr_tensor(torch.from_numpy(indptr), torch.from_numpy(indices.astype(np.int64)), values,
                                       size=(n, vocab - num_shift))

    def _build_embedding_vectors(self, texts: List[str], batch_size: int = 32, max_len: int = 128, num_shift: int = 0) -> T:
        """Dense [N, V] passage embeddings (retriever.py:256-282)."""
        parts = []
        for s in range(0, len(texts), batch_size):
            emb = self.encode_corpus(texts[s:s + batch_size], batch_size=batch_size, max_len=max_len, convert_to_tensor=True)
            parts.append(emb[:, num_shift:])
        return torch.cat(parts, dim=0)

    def _build_embedding_csr(self, texts: List[str], batch_size: int = 32, max_len: int = 128):
        """Same embeddings as `_build_embedding_vectors(...).to_sparse_csr()` (retriever.py:303-304), emitted as CSR per batch
        on the GPU and appended to the index IN HBM (``vs_index_append_csr`` takes the device pointers): neither the dense
        [N, V] fp32 matrix (118 KB per passage) nor a host copy of the CSR pieces is ever held.  -> DeviceIndex."""
        from ...device_index import DeviceIndex
        from ... import _native as nat
        n = len(texts)
        dev_index, row_cap, pk_cap = None, n, 0
        pending = []                                        # batches embedded before the first reservation / beyond it
        # the mask stage and to_sparse_csr() fused (encoder.embed_csr -> vs_embed_mask_to_csr: the masked dense batch is never written) when
        # the encoder offers it; else embed + vs_dense_to_csr
        fused = hasattr(self.encoder_p, "embed_csr") and type(self).encode_corpus is BiEncoder.encode_corpus
        batches = self.encode_corpus_csr(texts, batch_size=batch_size, max_len=max_len) if fused else None
        for s in range(0, n, batch_size):
            if fused:
                try:
                    rp, ci, va, n_cols = next(batches)
                except (nat.VsearchNativeError, ValueError):
                    # (a native error of the fused kernel -- raised here, outside the append below: the same host fallback serves it)
                    if dev_index is not None:
                        dev_index.close()
                    return None
            else:
                emb = self.encode_corpus(texts[s:s + batch_size], batch_size=batch_size, max_len=max_len, convert_to_tensor=True)
                rp, ci, va = sp.dense_to_csr(emb.float().contiguous())        # device tensors
                n_cols = int(emb.shape[1])
            if dev_index is None:
                # reserve from the first batch: the encoder keeps at most topk (+ the lexical tokens) non-zeros per passage
                per_row = int((rp[1:] - rp[:-1]).max().item()) if rp.numel() > 1 else 0
                bound = max(per_row, int(getattr(getattr(self.encoder_p, "config", None), "topk", 0) or 0)) + int(max_len)
                pk_cap = n * ((min(bound, n_cols) + 7) // 8)
                dev_index = DeviceIndex.reserved(row_cap, max(pk_cap, 1), n_cols, nat.VS_F32, device=rp.device.index or 0)
            try:
                dev_index.append_csr(rp, ci, va)
            except (nat.VsearchNativeError, ValueError):
                pending.append((rp.cpu(), ci.cpu(), va.cpu(), s))          # a passage denser than the bound: rebuild with exact sizes
                break
        if pending:
            return None
        return dev_index

    def _build_embedding_csr_host(self, texts: List[str], batch_size: int = 32, max_len: int = 128):
        """Fallback of `_build_embedding_csr` (a passage denser than the reservation bound): CSR pieces gathered on the host."""
        ptrs, cols, vals, base, V = [torch.zeros(1, dtype=torch.int64)], [], [], 0, None
        for s in range(0, len(texts), batch_size):
            emb = self.encode_corpus(texts[s:s + batch_size], batch_size=batch_size, max_len=max_len, convert_to_tensor=True)
            V = emb.shape[1]
            rp, ci, va = sp.dense_to_csr(emb.float().contiguous())
            ptrs.append(rp[1:].cpu() + base)
            base += int(rp[-1].item())
            cols.append(ci.cpu())
            vals.append(va.cpu())
        return torch.sparse_csr_tensor(torch.cat(ptrs), torch.cat(cols).to(torch.int64), torch.cat(vals), size=(len(texts), V))

    def build_index(self, texts: List[str], batch_size=32, index_type=IndexType.DENSE, bag_of_token=False, devices=None):
        """retriever.py:284-317.  `devices` (not in the reference): deal the built sparse / bag-of-token index over several GPUs of this
        process in contiguous row ranges (SparseIndex.shard_rows) -- None, "all", a count, or a list of GPU ordinals."""
        if isinstance(index_type, str):
            index_type = IndexType(index_type.lower())
        elif not isinstance(index_type, IndexType):
            raise TypeError("index_type must be an instance of IndexType, int, or str.")
        self.index_type = index_type
        if index_type == IndexType.DENSE:
            self.index = Index()
            self.index.data = texts
            self.index.vector = self._build_embedding_vectors(texts, batch_size=batch_size)
        elif index_type == IndexType.SPARSE:
            self.index = SparseIndex()
            self.index.data = texts
            built = self._build_embedding_csr(texts, batch_size=batch_size) if len(texts) else None
            if built is not None:
                self.index.adopt_device_index(built, dtype=torch.float32)
            else:
                self.index.vector = self._build_embedding_csr_host(texts, batch_size=batch_size)
        elif index_type == IndexType.BAG_OF_TOKEN:
            self.index = BoTIndex()
            self.index.data = texts
            self.index.vector = self._build_bot_vectors(texts, batch_size=batch_size)
        else:
            raise NotImplementedError
        self.index.move_to_device(self.device)
        if devices is not None:
            if index_type == IndexType.DENSE:
                raise NotImplementedError("devices=: row sharding serves the sparse and bag-of-token indexes")
            self.index.shard_rows(devices)

    def delete_documents(self, ids, index: Index = None):
        """Delete documents of the index by id (Index.delete): retrieve, rerank, more_like_this and retrieve_with_feedback never return
        them again; ids do not move until compact_index()."""
        (index or self.index).delete(ids)

    def compact_index(self, index: Index = None):
        """Drop deleted documents for good (Index.compact) -> old_ids: document j of the index was document old_ids[j] before."""
        return (index or self.index).compact()

    def prune_index(self, topk=None, min_value=None, drop_tokens=None, keep_tokens=None, max_df=None, protect_lexical: Index = None,
                    inplace: bool = True, index: Index = None) -> Index:
        """Index.pruned with the columns given as column ids or vocabulary tokens (resolved the way must= is: a string is one entry of the
        passage tokenizer's vocabulary, its column is token id - shift) -> the pruned index; inplace: it replaces retriever.index (the old
        index object stays valid for whoever holds it).  protect_lexical: the bag-of-token index of the same documents."""
        from ...doc_filter import terms_to_columns
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        vocab = self.encoder_p.tokenizer.vocab
        shift = int(self.encoder_p.config.shift_vocab_num)
        drop = None if drop_tokens is None else terms_to_columns(drop_tokens, vocab, shift, "drop_tokens")
        keep = None if keep_tokens is None else terms_to_columns(keep_tokens, vocab, shift, "keep_tokens")
        new = index.pruned(topk=topk, min_value=min_value, drop_columns=drop, keep_columns=keep, max_df=max_df, protect=protect_lexical)
        if inplace:
            self.index = new
        return new

    def normalize_index(self, p=2, inplace: bool = False, index: Index = None) -> Index:
        """Index.normalized -> the index with every document at unit length (cosine ranking on the fast path); inplace: it replaces
        retriever.index (the old index object stays valid for whoever holds it)."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        new = index.normalized(p)
        if inplace:
            self.index = new
        return new

    def reweight_index(self, token_weights=None, idf: bool = False, dtype=None, inplace: bool = False, index: Index = None) -> Index:
        """Index.rescaled by column -> the reweighted index.  token_weights: {column id or vocabulary token: weight} (tokens resolved the way
        prune_index resolves drop_tokens; the columns not named keep weight 1); idf: multiply in Index.idf_weights() (float32 product).  With
        neither the index is only converted to `dtype`.  inplace: it replaces retriever.index."""
        from ...doc_filter import terms_to_columns
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        scale = None
        if idf:
            scale = index.idf_weights().cpu().numpy()
        if token_weights is not None:
            if not hasattr(token_weights, "items"):
                raise TypeError(f"token_weights must be a dict of token -> weight, got {type(token_weights).__name__}")
            keys = list(token_weights.keys())
            cols = terms_to_columns(keys, self.encoder_p.tokenizer.vocab, int(self.encoder_p.config.shift_vocab_num), "token_weights")
            n_cols = int(index._vector_meta()[0][1])
            if scale is None:
                scale = np.ones(n_cols, dtype=np.float32)
            for c, key in zip(cols, keys):
                if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) < n_cols:
                    raise ValueError(f"token_weights: {key!r} is not a column in [0, {n_cols})")
                scale[int(c)] = np.float32(scale[int(c)]) * np.float32(token_weights[key])
        new = index.rescaled(col_scale=scale, dtype=dtype)
        if inplace:
            self.index = new
        return new

    def combine_index(self, other: Index, weight=1.0, other_weight=1.0, inplace: bool = False, dtype=None, index: Index = None) -> Index:
        """Index.combined -> the index of weight * retriever.index + other_weight * other, cell by cell: its search is the exact hybrid
        ranking by the weighted sum of the two scores.  other: an index of the same documents (e.g. the bag-of-token index, rescaled by
        idf_weights()).  inplace: it replaces retriever.index (the old index object stays valid for whoever holds it)."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        new = index.combined(other, weight, other_weight, dtype=dtype)
        if inplace:
            self.index = new
        return new

    def merge_index(self, other, inplace: bool = True, index: Index = None, dtype=None) -> Index:
        """Index.concatenated -> the index of retriever.index's documents with those of `other` (an index, or a sequence of them) behind
        them: last night's documents, embedded and indexed as a small index of their own, join the main one without leaving the GPU.
        inplace: it replaces retriever.index (the old index object stays valid for whoever holds it)."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        others = [other] if isinstance(other, Index) else list(other)
        new = index.concatenated(*others, dtype=dtype)
        if inplace:
            self.index = new
        return new

    def subset_index(self, filter=None, query=None, min_score=None, ids=None, inplace: bool = True, index: Index = None) -> Index:
        """Index.subset -> the new index of a document set: `filter`, or the documents one `query` (a text, or its embedding [1, V]) scores at
        least `min_score`, or the documents `ids` in that order; inplace: it replaces retriever.index (the old index object stays valid for
        whoever holds it)."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        q_embs = None if query is None else self.process_query(query)
        new = index.subset(q_embs=q_embs, min_score=min_score, filter=filter, ids=ids)
        if inplace:
            self.index = new
        return new

    def sort_index_by(self, field, descending: bool = False, inplace: bool = True, index: Index = None) -> Index:
        """Index.sorted_by -> the new index of the live documents ordered by a facet or value field (e.g. the labels ``cluster`` stored);
        inplace: it replaces retriever.index."""
        index = index or self.index
        if index is None:
            raise RuntimeError("no index: call build_index / load_index first")
        new = index.sorted_by(field, descending=descending)
        if inplace:
            self.index = new
        return new

    def save_index(self, path):
        self.index.save(path)

    def load_index(self, index_file=None, data_file=None, index_type=None, devices=None):
        """retriever.py:322-348.  `devices` (not in the reference): row-shard a sparse / bag-of-token index over several GPUs of this
        process -- None (one device, the reference's behaviour), "all", a count, or a list of GPU ordinals (SparseIndex docstring)."""
        if index_type is None:
            if index_file.endswith(".pt"):
                index_type = IndexType.DENSE
            elif index_file.endswith(".npz"):
                index_type = IndexType.SPARSE
            else:
                raise ValueError("Cannot infer index type from file extension. Please provide 'index_type' explicitly.")
        elif isinstance(index_type, str):
            index_type = IndexType(index_type.lower())
        elif not isinstance(index_type, IndexType):
            raise TypeError("index_type must be an instance of IndexType, int, or str.")
        self.index_type = index_type
        cls = {IndexType.DENSE: Index, IndexType.SPARSE: SparseIndex, IndexType.BAG_OF_TOKEN: BoTIndex}[index_type]
        if devices is not None and index_type == IndexType.DENSE:
            raise NotImplementedError("devices=: row sharding serves the sparse and bag-of-token indexes")
        self.index = cls(index_file, data_file, device=self.device) if devices is None else cls(index_file, data_file, device=self.device, devices=devices)
