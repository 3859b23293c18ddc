"""GPU tests of the term filters (vs_index_term_bitmaps, vs_term_filter_combine, vs_shard_group_term_bitmaps; DocFilter.from_terms) -- run
on MI355X.

The contract: bitmap t holds exactly the rows that store column cols[t] with a non-zero value (>= the threshold, when one is given), a
program combines them as must / must_not / should, and every comparison here is exact equality of words.  Expected values come from the
numpy references of tests/_term_filter_ref.py applied to what the index itself exports (index.export_csr())."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import oracle
from conftest import SHIFT, V, VOCAB
from _term_filter_ref import allowed_mask_ref, combine_ref, pack_bits, term_bitmaps_ref, term_masks_ref
from vsearch_amd import _native as nat
from vsearch_amd import synth
from vsearch_amd.device_index import DeviceIndex, ShardGroup
from vsearch_amd.doc_filter import DocFilter, normalize_terms

pytestmark = pytest.mark.gpu

EVERY, NEVER = 777, 12345                     # a column every non-empty row stores, a column no row stores
VALUES = np.array([0.0, -1.5, -0.25, 0.125, 0.5, 0.5, 1.0, 2.0, 3.0], np.float32)     # fp16-exact; explicit zeros and negatives


def make_csr(n, seed, empty=True, long_row=None):
    """Rows of 0 (when `empty`), 1, 7, 8, 9, 16 and random lengths -- no pad, one pad, full packets --, optionally one row of about 2000
    entries; column 0 and column V - 1 in some rows, EVERY in every non-empty row, NEVER in none."""
    rng = np.random.default_rng(seed)
    pool = np.setdiff1d(np.arange(1, V - 1), [EVERY, NEVER])
    hot = pool[:40]                                  # columns frequent enough to meet in programs
    lens = np.array([(0, 1, 7, 8, 9, 16)[r % 6] if r % 3 else int(rng.integers(1, 41)) for r in range(n)])
    if not empty:
        lens = np.maximum(lens, 1)
    if long_row is not None and long_row < n:
        lens[long_row] = 2000
    rows = []
    for r, l in enumerate(lens):
        if l == 0:
            rows.append(np.zeros(0, np.int64))
            continue
        c = {EVERY}
        if r % 5 == 0:
            c.add(0)
        if r % 7 == 0:
            c.add(V - 1)
        c.update(rng.choice(hot, min(l, 6), replace=False).tolist())
        c = list(c)[:l] if l < len(c) else list(c) + rng.choice(pool[40:], l - len(c), replace=False).tolist()
        if EVERY not in c:
            c[0] = EVERY
        rows.append(np.unique(np.asarray(c, np.int64)))
    indptr = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int64)
    data = rng.choice(VALUES, indices.shape[0]).astype(np.float32)
    return indptr, indices, data


def build(ip, ix, d, store):
    if store == "binary":
        return DeviceIndex.from_csr(ip, ix, None, V)
    return DeviceIndex.from_csr(ip, ix, d.astype(np.float16) if store == "fp16" else d, V)


def words_of(t):
    return t.cpu().numpy().view(np.uint32)


def expect(idx, cols, thr=None):
    ip, ix, d = idx.export_csr()
    return term_bitmaps_ref(ip, ix, d, int(idx.n_rows), cols, thr)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000, 1025, 2049])
def test_row_counts_cross_word_line_and_run(n):
    """n_rows across a word, a 128-byte line and the kernel's run of 1024 rows; tail bits 0; words beyond W of a wider row are untouched"""
    ip, ix, d = make_csr(n, n, empty=False)
    cols = [0, V - 1, EVERY, NEVER, int(ix[0]), int(ix[-1]), EVERY]
    W = (n + 31) // 32
    for store in ("fp32", "fp16", "binary"):
        idx = build(ip, ix, d, store)
        want = expect(idx, cols)
        assert (words_of(idx.term_bitmaps(cols)) == want).all(), store
        if store == "binary":
            assert (want[2] == pack_bits(np.ones(n, bool))).all() and not want[3].any()       # every row / no row
        # the C ABI with ld_words > W: the words behind a bitmap are not written
        ld = W + 3
        buf = torch.full((len(cols), ld), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        c = np.asarray(cols, np.int32)
        nat.check(nat.lib().vs_index_term_bitmaps(idx._h, C.c_void_p(c.ctypes.data), None, len(cols), C.c_void_p(buf.data_ptr()), ld, None, 1, None))
        got = words_of(buf)
        assert (got[:, :W] == want).all() and (got[:, W:] == 0x5A5A5A5A).all(), store
        # host outputs
        hw = np.zeros((len(cols), W), np.uint32)
        hdf = np.zeros(len(cols), np.int64)
        nat.check(nat.lib().vs_index_term_bitmaps(idx._h, C.c_void_p(c.ctypes.data), None, len(cols), C.c_void_p(hw.ctypes.data), W,
                                                  C.c_void_p(hdf.ctypes.data), 1, None))
        assert (hw == want).all() and hdf.tolist() == [int(np.unpackbits(w.view(np.uint8)).sum()) for w in want], store


@pytest.fixture(scope="module")
def mixed():
    """the mixed corpus (empty rows, 1 / 7 / 8 / 9 / 16 entries, one row of 2000) on the three stores, with its exported CSR"""
    n = 2500
    ip, ix, d = make_csr(n, 5, empty=True, long_row=1300)
    out = {}
    for store in ("fp32", "fp16", "binary"):
        idx = build(ip, ix, d, store)
        out[store] = (idx, idx.export_csr())
    return n, out


@pytest.mark.parametrize("store", ["fp32", "fp16", "binary"])
def test_mixed_corpus_terms_and_thresholds(mixed, store):
    n, by_store = mixed
    idx, (ip, ix, d) = by_store[store]
    present = np.unique(ix)
    rng = np.random.default_rng(3)
    base = [0, V - 1, EVERY, NEVER]
    for T in (1, 2, 300, nat.TERM_FILTER_SLOTS + 1):
        cols = (base + rng.choice(np.setdiff1d(present, base), max(T - 4, 0), replace=False).tolist())[:T]
        assert len(set(cols)) == T
        assert (words_of(idx.term_bitmaps(cols)) == term_bitmaps_ref(ip, ix, d, n, cols)).all(), T
    dup = [EVERY, 0, EVERY, int(present[50]), 0]                                           # duplicate columns: identical bitmaps
    got = words_of(idx.term_bitmaps(dup))
    assert (got == term_bitmaps_ref(ip, ix, d, n, dup)).all() and (got[0] == got[2]).all() and (got[1] == got[4]).all()
    # thresholds: v == thr, a threshold below a negative stored value, thr <= 0 (a stored zero counts), per-term lists and dicts, the
    # same column under two thresholds and under none
    cols = [EVERY, EVERY, EVERY, EVERY, EVERY, 0, V - 1, NEVER] + present[40:60].tolist()
    thr = [0.5, -1.5, 0.0, None, 3.5, 2.0, -0.25, 0.0] + [0.125] * 20
    want = term_bitmaps_ref(ip, ix, d, n, cols, thr)
    assert (words_of(idx.term_bitmaps(cols, thr=thr)) == want).all()
    if store != "binary":
        masks = term_masks_ref(ip, ix, d, n, [EVERY] * 4, [0.5, None, -1.5, 0.0])
        v = np.zeros(n, np.float32)
        sel = ix == EVERY
        v[np.repeat(np.arange(n), np.diff(ip))[sel]] = d[sel]
        assert masks[0][v == 0.5].all() and not masks[0][v == 0.125].any()                  # v == thr is in
        assert masks[1][v == -1.5].all() and masks[2][v == -1.5].all() and not masks[3][v == -1.5].any()   # a negative value
    d_thr = {int(present[41]): 0.5, EVERY: 1.0}
    cols2 = [EVERY, int(present[41]), int(present[42])]
    assert (words_of(idx.term_bitmaps(cols2, thr=d_thr)) == term_bitmaps_ref(ip, ix, d, n, cols2, d_thr)).all()
    df = idx.doc_freq(cols, thr=thr).cpu().numpy()
    assert df.dtype == np.int64 and df.tolist() == [int(np.unpackbits(w.view(np.uint8)).sum()) for w in want]
    for bad in ([-1], [V], [0, V]):
        with pytest.raises(ValueError):
            idx.term_bitmaps(bad)
    c = np.asarray([V], np.int32)
    buf = torch.zeros((1, (n + 31) // 32), dtype=torch.int32, device="cuda")
    for bad in (V, -1):
        c[0] = bad
        assert nat.lib().vs_index_term_bitmaps(idx._h, C.c_void_p(c.ctypes.data), None, 1, C.c_void_p(buf.data_ptr()), buf.shape[1], None, 1,
                                               None) == nat.VS_EINVAL


def test_grown_sliced_and_deleted_index():
    n = 1500
    ip, ix, d = make_csr(n, 9, long_row=700)
    cols = [0, V - 1, EVERY, NEVER] + np.unique(ix)[40:60].tolist()
    want = term_bitmaps_ref(ip, ix, d, n, cols)
    grown = DeviceIndex.reserved(n + 100, int(((np.diff(ip) + 7) // 8).sum()) + 50, V, nat.VS_F32)
    for r0, r1 in ((0, 400), (400, 1025), (1025, n)):
        grown.append_csr(ip[r0:r1 + 1] - ip[r0], ix[ip[r0]:ip[r1]], d[ip[r0]:ip[r1]])
    assert (words_of(grown.term_bitmaps(cols)) == want).all()
    part = grown.slice_rows(333, 777)
    sip, six, sd = part.export_csr()
    assert (words_of(part.term_bitmaps(cols)) == term_bitmaps_ref(sip, six, sd, 777, cols)).all()
    assert (term_masks_ref(sip, six, sd, 777, cols) == term_masks_ref(ip, ix, d, n, cols)[:, 333:333 + 777]).all()
    # deletions: bitmaps unchanged, doc_freq(live_only=True) drops the deleted rows, live_only=False does not; compact: both agree
    masks = term_masks_ref(ip, ix, d, n, cols)
    dead = np.unique(np.random.default_rng(1).choice(n, 200, replace=False))
    grown.delete_rows(dead)
    live = np.ones(n, bool)
    live[dead] = False
    assert (words_of(grown.term_bitmaps(cols)) == want).all()
    assert grown.doc_freq(cols).cpu().numpy().tolist() == (masks & live).sum(axis=1).tolist()
    assert grown.doc_freq(cols, live_only=False).cpu().numpy().tolist() == masks.sum(axis=1).tolist()
    packed, old = grown.compact()
    assert (words_of(packed.term_bitmaps(cols)) == pack_bits(masks[:, old])).all()
    assert packed.doc_freq(cols).cpu().numpy().tolist() == packed.doc_freq(cols, live_only=False).cpu().numpy().tolist() == masks[:, old].sum(axis=1).tolist()


def test_dense_indexes():
    """the matrix kind (a plain kernel: one thread a row) and a dense index stored as packets (the scan)"""
    n, Cn = 1100, 512
    rng = np.random.default_rng(2)
    mat = np.where(rng.random((n, Cn)) < 0.03, rng.choice(VALUES[1:], (n, Cn)), 0).astype(np.float32)
    cols = [0, Cn - 1, 5, 17, 17, 300]
    thr = [None, 0.5, 0.125, None, 2.0, -0.25]
    has = np.stack([(mat[:, c] != 0) if t is None else ((mat[:, c] >= np.float32(t)) & (mat[:, c] != 0)) for c, t in zip(cols, thr)])
    for max_density, kind_packets in ((0.0, False), (0.05, True)):
        idx = DeviceIndex.from_dense(mat, max_density=max_density)
        assert (idx.info().n_packets > 0) == kind_packets
        assert (words_of(idx.term_bitmaps(cols)) == pack_bits(np.stack([mat[:, c] != 0 for c in cols]))).all(), max_density
        assert (words_of(idx.term_bitmaps(cols, thr=thr)) == pack_bits(has)).all(), max_density       # (a zero element is not stored)
        assert idx.doc_freq(cols, thr=thr).cpu().numpy().tolist() == has.sum(axis=1).tolist()
        for bad in ([-1], [Cn]):
            with pytest.raises(ValueError):
                idx.term_bitmaps(bad)
    fp16 = DeviceIndex.from_dense(mat.astype(np.float16))
    assert (words_of(fp16.term_bitmaps(cols, thr=thr)) == pack_bits(has)).all()


def _program_cases(present):
    h = [int(c) for c in present[:70]]
    return {
        "shared": dict(must=[EVERY, h[1]], must_not=[h[2]], should=[h[3], h[4], h[5]], min_should=2),
        "per-query-ragged": dict(must=[[EVERY], [h[1], h[2]], []], must_not=[[h[3]], [], [h[4], h[5], 0]], should=[[h[6], h[7], h[8]], [], [h[9]]]),
        "must-not-only": dict(must_not=[h[1], V - 1]),
        "all-empty": dict(),
        "should-64": dict(should=h[:64], min_should=3),
        "mixed-shared-and-per-query": dict(must=[EVERY], should=[[h[1], h[2]], [h[3], h[4], h[5]], [h[6]]], min_should=[2, 1, 0]),
        "thresholds": dict(must=[EVERY], should=[h[1], h[2]], thr={EVERY: 0.5, h[1]: 0.0}),
    }


@pytest.mark.parametrize("store", ["fp32", "binary"])
def test_programs_equal_the_brute_force(mixed, store):
    n, by_store = mixed
    idx, (ip, ix, d) = by_store[store]
    hot = np.unique(ix)
    hot = hot[np.argsort(-np.bincount(ix, minlength=V)[hot], kind="stable")]
    cases = _program_cases(hot)
    should = [int(c) for c in hot[2:7]]
    for ms in (0, 1, 2, len(should), len(should) + 1):
        cases[f"min-should-{ms}"] = dict(should=should, min_should=ms)
    for name, kw in cases.items():
        f = DocFilter.from_terms(idx, **kw)
        want = allowed_mask_ref(ip, ix, d, n, **kw)
        B = want.shape[0]
        per_query = any(isinstance(v, list) and v and isinstance(v[0], list) for v in kw.values()) or isinstance(kw.get("min_should"), list)
        assert f.n_rows == n and f.per_query == per_query, name
        got = words_of(f.words).reshape(B, -1)
        assert (got == pack_bits(want)).all(), name
        prog = normalize_terms(**kw)                                       # and the word-level reference
        tw = term_bitmaps_ref(ip, ix, d, n, prog.cols, prog.thr)
        assert (got == combine_ref(tw, n, prog.must, prog.must_not, prog.should, prog.min_should)).all(), name
    assert (words_of(DocFilter.from_terms(idx).words) == pack_bits(np.ones(n, bool))).all()            # every row, tail bits 0
    assert not words_of(DocFilter.from_terms(idx, should=should, min_should=len(should) + 1).words).any()
    # the C ABI with host pointers, out_ld > W, and an index outside [-1, T)
    prog = normalize_terms(**cases["per-query-ragged"])
    tw = term_bitmaps_ref(ip, ix, d, n, prog.cols, prog.thr)
    W = tw.shape[1]
    out = np.full((3, W + 1), 0xA5A5A5A5, np.uint32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    args = lambda must: (p(tw), W, n, len(prog.cols), p(must), must.shape[1], p(prog.must_not), prog.must_not.shape[1], p(prog.should),
                         prog.should.shape[1], p(prog.min_should), 3, p(out), W + 1, 0, None)
    nat.check(nat.lib().vs_term_filter_combine(*args(prog.must)))
    assert (out[:, :W] == combine_ref(tw, n, prog.must, prog.must_not, prog.should, prog.min_should)).all() and (out[:, W] == 0xA5A5A5A5).all()
    bad = prog.must.copy()
    bad[0, 0] = len(prog.cols)
    assert nat.lib().vs_term_filter_combine(*args(bad)) == nat.VS_EINVAL


def test_three_unaligned_shards():
    """shards of 33, 64 and 5 rows on one GPU: the seam words hold bits of two shards"""
    n = 102
    ip, ix, d = make_csr(n, 21)
    full = DeviceIndex.from_csr(ip, ix, d, V)
    shards = []
    for r0, r1 in ((0, 33), (33, 97), (97, 102)):
        shards.append(DeviceIndex.from_csr(ip[r0:r1 + 1] - ip[r0], ix[ip[r0]:ip[r1]], d[ip[r0]:ip[r1]], V))
    group = ShardGroup(shards)
    cols = [0, V - 1, EVERY, NEVER] + np.unique(ix)[40:50].tolist() + [EVERY]
    thr = {EVERY: 0.5}
    for t in (None, thr):
        assert (words_of(group.term_bitmaps(cols, thr=t)) == words_of(full.term_bitmaps(cols, thr=t))).all()
        assert group.doc_freq(cols, thr=t).cpu().numpy().tolist() == full.doc_freq(cols, thr=t).cpu().numpy().tolist()
    assert (words_of(full.term_bitmaps(cols)) == term_bitmaps_ref(ip, ix, d, n, cols)).all()
    dead = [0, 32, 33, 96, 97, 101]
    group.delete_rows(np.asarray(dead))
    full.delete_rows(np.asarray(dead))
    assert group.doc_freq(cols).cpu().numpy().tolist() == full.doc_freq(cols).cpu().numpy().tolist()
    assert group.doc_freq(cols, live_only=False).cpu().numpy().tolist() == full.doc_freq(cols, live_only=False).cpu().numpy().tolist()
    kw = dict(must=[EVERY], must_not=[0], should=[[int(c)] for c in np.unique(ix)[40:43]])
    want = pack_bits(allowed_mask_ref(ip, ix, d, n, **kw))
    assert (words_of(DocFilter.from_terms(group, **kw).words) == want).all() and (words_of(DocFilter.from_terms(full, **kw).words) == want).all()


def _narrow_program(ip, ix, d, n, k):
    """must terms, most frequent columns first, until fewer than k (but some) rows are left"""
    order = np.argsort(-np.bincount(ix, minlength=V), kind="stable")
    must, left = [], np.ones(n, bool)
    for c in order[:200]:
        m = term_masks_ref(ip, ix, d, n, [int(c)])[0]
        if (left & m).sum() >= 3:
            must.append(int(c))
            left &= m
        if left.sum() < k:
            break
    assert 0 < left.sum() < k
    return must


@pytest.mark.parametrize("kind", ["valued-quad", "binary"])
def test_search_under_term_filters(kind):
    B, k = 4, 100
    if kind == "valued-quad":
        n = 20000
        ip, ix, d = oracle.synth_csr(3, 0, n, V, 768)
        idx = DeviceIndex.from_csr(ip, ix, d, V)
        idx.set_option("blocked_postings", 1)
        idx.set_option("postings_walk", 4)
        q = oracle.synth_queries(2, B)
    else:
        n = 3000
        ip, ix, _ = oracle.synth_csr(5, 0, n, V, 86, synth.KIND_BOT)
        d = None
        idx = DeviceIndex.from_csr(ip, ix, None, V)
        idx.set_option("blocked_postings", 1)
        idx.set_option("postings_walk", 6)
        q = oracle.synth_queries(6, B, V, 776, synth.VAL_DYADIC)
    must = _narrow_program(ip, ix, d, n, k)
    hot = np.argsort(-np.bincount(ix, minlength=V), kind="stable")
    programs = [dict(must=must), dict(must=must[:1], must_not=[int(hot[5])], should=[int(c) for c in hot[6:12]], min_should=2),
                dict(should=[[int(hot[1])], [int(hot[2]), int(hot[3])], [], [int(hot[4])]], must_not=[int(hot[0])])]
    masks = [allowed_mask_ref(ip, ix, d, n, **kw) for kw in programs]       # (computed once, shared below)
    for kw, mask in zip(programs, masks):
        f = DocFilter.from_terms(idx, **kw)
        ids, sc = idx.search(q, k, filter=f)
        info = idx.info()
        assert info.last_path == 3 and (kind != "valued-quad" or info.postings_walk == 4)
        e_ids, e_sc = idx.search(q, k, filter=DocFilter.from_mask(mask if mask.shape[0] > 1 else mask[0]))
        assert (np.asarray(ids) == np.asarray(e_ids)).all() and (np.asarray(sc) == np.asarray(e_sc)).all()
    ids, sc = map(np.asarray, idx.search(q, k, filter=DocFilter.from_terms(idx, must=must)))
    left = int(masks[0].sum())
    assert (ids[:, :left] >= 0).all() and (ids[:, left:] == -1).all() and np.isneginf(sc[:, left:]).all()      # the padding appears
    # set algebra on the packed words
    f1 = DocFilter.from_terms(idx, **programs[1])
    f2 = DocFilter.from_terms(idx, **programs[2])
    m1, m2 = pack_bits(masks[1])[0], pack_bits(masks[2])
    tail = pack_bits(np.ones(n, bool))
    assert (words_of((f1 & f2).words) == (m1 & m2)).all() and (words_of((f2 | f1).words) == (m1 | m2)).all()
    assert (words_of((~f1).words) == (~m1 & tail)).all() and (words_of((~f2).words) == (~m2 & tail)).all()
    assert (f1 & f2).per_query and not (f1 & ~f1).per_query and not words_of((f1 & ~f1).words).any()
    visible = DocFilter.from_mask(np.arange(n) % 2 == 0)
    assert (words_of((visible & f1).words) == (pack_bits(np.arange(n) % 2 == 0) & m1)).all()
    with pytest.raises(ValueError):
        f1 & DocFilter.from_mask(np.ones(n - 1, bool))
    with pytest.raises(ValueError):
        f2 & DocFilter.from_mask(np.ones((3, n), bool))


def test_retrieve_with_token_constraints():
    """Retriever.retrieve(must=[token]) through a fake encoder: only rows that store the token's column come back; filter= is ANDed in"""
    from vsearch_amd.ir import Retriever, SparseIndex
    n, B, k = 3000, 4, 50
    ip, ix, d = oracle.synth_csr(11, 0, n, V, 768)
    sp = SparseIndex(device="cuda:0")
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(d), size=(n, V))
    sp.move_to_device("cuda:0")
    hot = np.argsort(-np.bincount(ix, minlength=V), kind="stable")
    col, col2 = int(hot[0]), int(hot[1])
    tok = types.SimpleNamespace(vocab={f"tok{i}": i for i in range(VOCAB)})
    class Fake:                                  # (methods as class attributes: no reference cycle through the instance)
        process_query, term_filter = Retriever.process_query, Retriever.term_filter
    fake = Fake()
    fake.index, fake.device = sp, "cuda"
    fake.encoder_q = types.SimpleNamespace(config=types.SimpleNamespace(topk=768))
    fake.encoder_p = types.SimpleNamespace(tokenizer=tok, config=types.SimpleNamespace(shift_vocab_num=SHIFT))
    q = torch.from_numpy(oracle.synth_queries(7, B))
    has = term_masks_ref(ip, ix, d, n, [col, col2])
    res = Retriever.retrieve(fake, q, k=k, must=[f"tok{col + SHIFT}"])
    ids = res.ids.cpu().numpy()
    assert (ids >= 0).any() and has[0][ids[ids >= 0]].all()
    want = sp.search(q, k, filter=torch.from_numpy(has[0]))
    assert (ids == want.ids.cpu().numpy()).all() and (res.scores.cpu().numpy() == want.scores.cpu().numpy()).all()
    even = np.arange(n) % 2 == 0
    res = Retriever.retrieve(fake, q, k=k, must=[f"tok{col + SHIFT}"], must_not=[col2], filter=torch.from_numpy(even))
    want = sp.search(q, k, filter=torch.from_numpy(has[0] & ~has[1] & even))
    assert (res.ids.cpu().numpy() == want.ids.cpu().numpy()).all()
    with pytest.raises(ValueError, match="einstein"):
        Retriever.retrieve(fake, q, k=k, must=["einstein"])
    with pytest.raises(ValueError, match="tok5"):
        Retriever.term_filter(fake, must_not=["tok5"])
    assert sp.doc_freq([col, col2]).cpu().numpy().tolist() == has.sum(axis=1).tolist()
    sp.shard_rows([0, 0, 0])                                             # the facade's row sharding goes through the group call
    f = sp.term_filter(must=[col], must_not=[col2])
    assert (words_of(f.words) == pack_bits(has[0] & ~has[1])).all()
    assert sp.doc_freq([col, col2]).cpu().numpy().tolist() == has.sum(axis=1).tolist()
