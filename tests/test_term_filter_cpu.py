"""Host-side checks of the term filters that need no GPU: the numpy references agree with each other and with a dense brute force, the
argument normalisation of DocFilter.from_terms, the token -> column mapping of Retriever.term_filter, and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

from conftest import REPO, SHIFT, VOCAB
from _term_filter_ref import allowed_mask_ref, combine_ref, pack_bits, term_bitmaps_ref, term_masks_ref, unpack_words
from vsearch_amd import _native as nat
from vsearch_amd.doc_filter import TermProgram, normalize_terms, terms_to_columns


def random_csr(rng, n, V, max_len=12, binary=False):
    """CSR with empty rows, explicit zeros and negative values (all fp16-exact)"""
    lens = rng.integers(0, max_len + 1, n)
    lens[rng.random(n) < 0.2] = 0
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(V, l, replace=False)) for l in lens] + [np.zeros(0, np.int64)]).astype(np.int64)
    data = None
    if not binary:
        data = rng.choice(np.array([0.0, 0.0, -1.5, -0.25, 0.125, 0.5, 1.0, 2.0], np.float32), indices.shape[0])
    return indptr, indices, data


def dense_brute(indptr, indices, data, n, V, cols, thr):
    """the semantics on a dense value matrix and a dense stored-mask"""
    val = np.zeros((n, V), np.float32)
    stored = np.zeros((n, V), bool)
    for r in range(n):
        sl = slice(indptr[r], indptr[r + 1])
        stored[r, indices[sl]] = True
        val[r, indices[sl]] = 1.0 if data is None else data[sl]
    out = np.zeros((len(cols), n), bool)
    for t, c in enumerate(cols):
        out[t] = stored[:, c] & ((val[:, c] >= np.float32(thr[c])) if c in thr else (val[:, c] != 0))
    return out


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("n", [1, 33, 200])
def test_references_agree(n, binary):
    V = 40
    rng = np.random.default_rng(n + binary)
    ip, ix, d = random_csr(rng, n, V, binary=binary)
    cols = list(range(V))
    thr = {3: 0.5, 4: 0.0, 5: -0.25, 6: 1.0, 7: -3.0}
    masks = term_masks_ref(ip, ix, d, n, cols, thr)
    assert (masks == dense_brute(ip, ix, d, n, V, cols, thr)).all()
    words = term_bitmaps_ref(ip, ix, d, n, cols, thr)
    assert words.shape == (V, (n + 31) // 32) and (unpack_words(words, n) == masks).all()
    assert not np.unpackbits(words.view(np.uint8), bitorder="little").reshape(V, -1)[:, n:].any()
    programs = [dict(must=[1, 2]), dict(must_not=[3, 9]), dict(should=[4, 5, 6, 7, 8], min_should=2), dict(should=[4, 5], min_should=0),
                dict(should=[4, 5], min_should=3), dict(), dict(must=[[1], [2, 3], []], must_not=[[4], [], [5, 6]], should=[[7, 8, 9], [], [10]]),
                dict(must=[1], should=[[2, 3], [4, 5, 6]], min_should=[2, 1])]
    for kw in programs:
        prog = normalize_terms(thr=thr, **kw)
        tw = term_bitmaps_ref(ip, ix, d, n, prog.cols, prog.thr)
        got = combine_ref(tw, n, prog.must, prog.must_not, prog.should, prog.min_should)
        want = allowed_mask_ref(ip, ix, d, n, thr=thr, **kw)
        assert (got == pack_bits(want)).all(), kw
    if not binary:
        assert (masks[4] != term_masks_ref(ip, ix, d, n, [4])[0]).any() or n == 1      # (explicit zeros count under thr = 0 only)
    assert pack_bits(allowed_mask_ref(ip, ix, d, n))[0].tolist() == pack_bits(np.ones(n, bool)).tolist()   # all-empty program


def test_normalize_terms():
    p = normalize_terms(must=[7, 5, 7], must_not=[5], should=(9, 7))
    assert isinstance(p, TermProgram) and not p.per_query
    assert p.cols.dtype == np.int32 and p.cols.tolist() == [7, 5, 9] and p.thr is None       # duplicates collapse to one slot
    assert p.must.tolist() == [[0, 1]] and p.must_not.tolist() == [[1]] and p.should.tolist() == [[2, 0]]
    assert p.min_should.tolist() == [1]                                                     # default with should given
    assert normalize_terms(must=[3]).min_should.tolist() == [0] and normalize_terms().cols.shape == (0,)
    assert normalize_terms(should=[3, 4], min_should=0).min_should.tolist() == [0]
    assert normalize_terms(should=[3, 4], min_should=5).min_should.tolist() == [5]
    # ragged per-query lists, a flat list broadcast against them, -1 padding, per-query default of min_should
    p = normalize_terms(must=[[1, 2, 3], [], [2]], should=[[], [8], [8, 9]], must_not=[4])
    assert p.per_query and p.must.tolist() == [[0, 1, 2], [-1, -1, -1], [1, -1, -1]]
    assert p.must_not.tolist() == [[3]] * 3 and p.should.tolist() == [[-1, -1], [4, -1], [4, 5]]
    assert p.min_should.tolist() == [0, 1, 1] and p.cols.tolist() == [1, 2, 3, 4, 8, 9]
    p = normalize_terms(must=np.array([[1, 2], [2, 3]]), min_should=[0, 0], thr={2: 0.5, 99: 1.0})
    assert p.per_query and p.cols.tolist() == [1, 2, 3] and np.isnan(p.thr[[0, 2]]).all() and p.thr[1] == 0.5
    assert normalize_terms(must=[[1]], thr={}).thr is None and normalize_terms(must=[1], thr={5: 1.0}).thr is None
    # bad inputs
    with pytest.raises(ValueError):
        normalize_terms(must=[[1], [2]], should=[[1], [2], [3]])          # batch sizes differ
    with pytest.raises(ValueError):
        normalize_terms(must=[[1], [2]], min_should=[1, 1, 1])
    with pytest.raises(ValueError):
        normalize_terms(must=[-1])
    with pytest.raises(ValueError):
        normalize_terms(should=[1], min_should=-1)
    with pytest.raises(ValueError):
        normalize_terms(should=list(range(nat.TERM_FILTER_LIST + 1)))
    assert normalize_terms(should=list(range(nat.TERM_FILTER_LIST)) * 2).should.shape == (1, nat.TERM_FILTER_LIST)
    for bad in (dict(must=[1.5]), dict(must=["a"]), dict(must=[True]), dict(must=5), dict(must=[1, [2]]), dict(should=[1], min_should=1.0),
                dict(must=[1], thr=[0.5])):
        with pytest.raises(TypeError):
            normalize_terms(**bad)


class DictTokenizer:
    """the id tokenizer of the facade tests (token i is spelled "tok<i>") with a token -> id vocabulary"""
    vocab = {f"tok{i}": i for i in range(VOCAB)}


def test_tokens_to_columns():
    vocab = DictTokenizer.vocab
    assert terms_to_columns(["tok1000", 5, "tok30521"], vocab, SHIFT) == [1, 5, VOCAB - 1 - SHIFT]
    assert terms_to_columns([["tok999"], [7, "tok2000"]], vocab, SHIFT) == [[0], [7, 1001]]
    assert terms_to_columns("tok1234", vocab, SHIFT) == [235] and terms_to_columns(None, vocab, SHIFT) is None
    with pytest.raises(ValueError, match="einstein"):
        terms_to_columns(["einstein"], vocab, SHIFT)                       # not one vocabulary entry
    with pytest.raises(ValueError, match="tok998"):
        terms_to_columns(["tok998"], vocab, SHIFT)                         # below the shift: no column
    with pytest.raises(ValueError):
        terms_to_columns(["tok5"], range(VOCAB), SHIFT)                    # a vocabulary without a token -> id mapping
    from vsearch_amd.ir import Retriever
    assert callable(Retriever.term_filter)
    import inspect
    assert {"must", "must_not", "should", "min_should", "filter"} <= set(inspect.signature(Retriever.retrieve).parameters)


def test_abi_declares_and_binds_the_entry_points():
    header = open(os.path.join(REPO, "include", "vsearch_hip.h")).read()
    for name in ("vs_index_term_bitmaps", "vs_term_filter_combine", "vs_shard_group_term_bitmaps"):
        assert re.search(r"VS_API\s+int\s+" + name + r"\(", header), name
        assert name in nat.EXPORTED_SYMBOLS
        assert getattr(nat.lib(), name).restype is not None
    for macro, value in (("VS_TERM_FILTER_SLOTS", nat.TERM_FILTER_SLOTS), ("VS_TERM_FILTER_TERMS", nat.TERM_FILTER_TERMS),
                         ("VS_TERM_FILTER_LIST", nat.TERM_FILTER_LIST)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", header).group(1)) == value
    assert "term_filter.hip" in open(os.path.join(REPO, "vsearch_amd", "csrc", "Makefile")).read()
    from vsearch_amd.device_index import DeviceIndex, ShardGroup
    from vsearch_amd.doc_filter import DocFilter
    from vsearch_amd.ir import Index
    for cls in (DeviceIndex, ShardGroup):
        assert callable(cls.term_bitmaps) and callable(cls.doc_freq)
    assert callable(DocFilter.from_terms) and callable(Index.term_filter) and callable(Index.doc_freq)
