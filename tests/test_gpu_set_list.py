"""GPU tests of the set egress (vs_set_count / vs_set_ids / vs_set_sample / vs_set_from_ids and their vs_index_* variants; DocFilter.count /
.ids / .pages / .sample / .from_ids, DeviceIndex / ShardGroup .set_count / .set_ids / .set_sample, Index.count_docs / .list_ids / .sample_ids,
Retriever.retrieve_ids / .sample_band) -- run on MI355X.

The contract is tests/_set_list_ref.py.  Every result is an integer, so everything compares with ==.  The raw calls go into
junk-filled outputs, once on host buffers and once on device buffers: a slot that is not written shows."""
import ctypes as C

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, SetIds, SetSample, ShardGroup, set_list_plan
from vsearch_amd.doc_filter import DocFilter
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

import _set_list_ref as ref
import _term_agg_ref as taref

pytestmark = pytest.mark.gpu

JUNK = -0x5A5A5A5A5A5A5A5B
JUNK32 = 0x5A5A5A5A
N_ROWS = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4097]
BIT0 = [0, 1, 31, 32, 37, 101]
RPC = [64, 2048, 0]


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


class _Bufs:
    """inputs and junk-filled outputs of a raw call, host or device buffers throughout"""

    def __init__(self, on_dev, ins, outs):
        self.on_dev = on_dev
        ins = {k: np.ascontiguousarray(v) for k, v in ins.items() if v is not None}
        ins = {k: (v.view(np.int32) if v.dtype == np.uint32 else v.view(np.int64) if v.dtype == np.uint64 else v) for k, v in ins.items()}
        outs = {k: v for k, v in outs.items() if v is not None}
        if on_dev:
            self.ins = {k: torch.from_numpy(v).cuda() for k, v in ins.items()}
            self.outs = {k: torch.from_numpy(v).cuda() for k, v in outs.items()}
            torch.cuda.synchronize()
        else:
            self.ins, self.outs = ins, outs

    def p(self, name):
        t = self.ins.get(name, self.outs.get(name))
        if t is None:
            return None
        return C.c_void_p(t.data_ptr() if self.on_dev else t.ctypes.data)

    def out(self, name):
        if self.on_dev:
            torch.cuda.synchronize()
        return _np(self.outs[name])


def _raw_count(words, bit0, ld, aw, B, n, rpc, on_dev, index=None):
    b = _Bufs(on_dev, dict(words=words, aw=aw), dict(counts=np.full(B, JUNK, np.int64)))
    if index is None:
        nat.check(nat.lib().vs_set_count(b.p("words"), bit0, ld, b.p("aw"), B, n, rpc, b.p("counts"), 0, None))
    else:
        nat.check(nat.lib().vs_index_set_count(index._h, b.p("words"), bit0, ld, B, rpc, b.p("counts"), None))
    return b.out("counts")


def _raw_ids(words, bit0, ld, aw, B, n, offsets, limit, id_offset, rpc, on_dev, index=None):
    off = None if offsets is None else np.asarray(offsets, np.int64)
    b = _Bufs(on_dev, dict(words=words, aw=aw, off=off), dict(ids=np.full((B, limit), JUNK, np.int64) if limit else None, counts=np.full(B, JUNK, np.int64)))
    if index is None:
        nat.check(nat.lib().vs_set_ids(b.p("words"), bit0, ld, b.p("aw"), B, n, b.p("off"), limit, id_offset, rpc, b.p("ids"), b.p("counts"), 0, None))
    else:
        nat.check(nat.lib().vs_index_set_ids(index._h, b.p("words"), bit0, ld, B, b.p("off"), limit, id_offset, rpc, b.p("ids"), b.p("counts"), None))
    return (b.out("ids") if limit else np.zeros((B, 0), np.int64)), b.out("counts")


def _raw_sample(words, bit0, ld, aw, B, n, seeds, k, id_offset, rpc, on_dev, index=None, want_hash=True):
    b = _Bufs(on_dev, dict(words=words, aw=aw, seeds=np.asarray(seeds, np.uint64)),
              dict(ids=np.full((B, k), JUNK, np.int64), hs=np.full((B, k), JUNK32, np.int32) if want_hash else None, counts=np.full(B, JUNK, np.int64)))
    if index is None:
        nat.check(nat.lib().vs_set_sample(b.p("words"), bit0, ld, b.p("aw"), B, n, b.p("seeds"), k, id_offset, rpc, b.p("ids"), b.p("hs"), b.p("counts"),
                                          0, None))
    else:
        nat.check(nat.lib().vs_index_set_sample(index._h, b.p("words"), bit0, ld, B, b.p("seeds"), k, id_offset, rpc, b.p("ids"), b.p("hs"),
                                                b.p("counts"), None))
    return b.out("ids"), (b.out("hs").view(np.uint32) if want_hash else None), b.out("counts")


def _raw_from_ids(ids, m, n, bit0, allow, ld_words, on_dev):
    B = ids.shape[0]
    b = _Bufs(on_dev, dict(ids=ids), dict(words=np.full((B, ld_words), JUNK32, np.int32)))
    nat.check(nat.lib().vs_set_from_ids(b.p("ids"), B, m, ids.shape[1], n, bit0, allow, b.p("words"), ld_words, 0, None))
    return b.out("words").view(np.uint32)


def _sets(n, rng):
    """the nine sets of the grid, bool [9, n]: empty, every row, only the first row, only the last, only the last bit of a word, alternating,
    1 %, 50 %, another 50 %"""
    m = np.zeros((9, n), bool)
    m[1] = True
    m[2, 0] = True
    m[3, n - 1] = True
    m[4, min(n - 1, 31)] = True
    m[5, ::2] = True
    m[6] = rng.random(n) < 0.01
    m[7] = rng.random(n) < 0.5
    m[8] = rng.random(n) < 0.5
    return m


def _windows(counts, variant):
    """per-query offsets that differ, and a limit: offset 0, inside the list, equal to the count, beyond it; limit 0, 1, above the count"""
    B = counts.shape[0]
    kinds = [(variant + b) % 4 for b in range(B)]
    off = np.array([0 if k == 0 else int(c) // 2 if k == 1 else int(c) if k == 2 else int(c) + 5 for k, c in zip(kinds, counts)], np.int64)
    limit = [0, 1, int(counts.max()) + 3, 7, 64][variant % 5]
    return off, limit


# ---- count and ids: the grid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", N_ROWS)
def test_count_and_ids_grid(n):
    rng = np.random.default_rng(n)
    variant = n
    for bit0 in BIT0:
        masks = _sets(n, rng)
        words = ref.pack(masks, bit0, spare=1, garbage=rng)                                       # garbage below bit0 and past the rows
        ld = words.shape[1]
        amask = rng.random(n) < 0.8
        aw = ref.pack(amask[None, :], bit0, spare=1, garbage=rng)[0]
        for rpc in RPC:
            for on_dev in (False, True):
                variant += 1
                a, am = (aw, masks & amask) if variant % 2 else (None, masks)
                id_offset = [0, 1000, 1 << 40][variant % 3]
                # B = 9: every set, per-query offsets that differ
                counts = ref.set_count(am)
                assert (_raw_count(words, bit0, ld, a, 9, n, rpc, on_dev) == counts).all(), (bit0, rpc, on_dev)
                off, limit = _windows(counts, variant)
                got = _raw_ids(words, bit0, ld, a, 9, n, off, limit, id_offset, rpc, on_dev)
                want = ref.set_ids(am, off, limit, id_offset)
                assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), (bit0, rpc, on_dev, off, limit)
                # B = 3: the alternating, the 1 % and a 50 % set, the whole list and one slot more
                sub, wsub = am[5:8], words[5:8]
                got = _raw_ids(wsub, bit0, ld, a, 3, n, None, int(sub.sum(1).max()) + 1, id_offset, rpc, on_dev)
                want = ref.set_ids(sub, None, int(sub.sum(1).max()) + 1, id_offset)
                assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), (bit0, rpc, on_dev)
                # B = 1 shared (ld_words = 0), and words == NULL: every row (under the and-words when given)
                one = am[8:9]
                off1, limit1 = _windows(ref.set_count(one), variant + 1)
                got = _raw_ids(words[8], bit0, 0, a, 1, n, off1, limit1, id_offset, rpc, on_dev)
                want = ref.set_ids(one, off1, limit1, id_offset)
                assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), (bit0, rpc, on_dev)
                every = (amask if a is not None else np.ones(n, bool))[None, :]
                got = _raw_ids(None, bit0, 0, a, 1, n, None, n, id_offset, rpc, on_dev)
                want = ref.set_ids(every, None, n, id_offset)
                assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), (bit0, rpc, on_dev)


@pytest.mark.parametrize("on_dev", [False, True])
def test_windows_that_straddle_span_and_chunk_boundaries(on_dev):
    rng = np.random.default_rng(17)
    n, bit0 = 20000, 37                                                                            # three automatic chunks of 8192 rows
    assert set_list_plan(n, 2, True, 0) == (3, 8192, 10) and set_list_plan(n, 2, True, 2048)[0] == 10
    masks = np.stack([rng.random(n) < 0.5, rng.random(n) < 0.01])
    words = ref.pack(masks, bit0, garbage=rng)
    ld = words.shape[1]
    cum = masks.cumsum(axis=1)
    for rpc in (0, 2048, 4096):
        for edge in (2048, 4096, 8192, 16384):                                                     # span, chunk and automatic-chunk boundaries
            off = np.array([cum[0, edge - 1] - 3, max(int(cum[1, edge - 1]) - 1, 0)], np.int64)    # the window starts just below the boundary
            got = _raw_ids(words, bit0, ld, None, 2, n, off, 7, 5, rpc, on_dev)
            want = ref.set_ids(masks, off, 7, 5)
            assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), (rpc, edge)
            assert (want[0][0] - 5 < edge).any() and (want[0][0] - 5 >= edge).any()                # it does straddle
        got = _raw_ids(words, bit0, ld, None, 2, n, None, int(cum[:, -1].max()), 0, rpc, on_dev)   # and the whole lists
        want = ref.set_ids(masks, None, int(cum[:, -1].max()))
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), rpc
    if on_dev:                                                                                     # a negative device offset reads as 0
        got = _raw_ids(words, bit0, ld, None, 2, n, [-4, 0], 7, 0, 0, True)
        assert (got[0] == ref.set_ids(masks, None, 7)[0]).all()
    else:                                                                                          # a negative host offset is refused
        with pytest.raises(ValueError, match="offsets"):
            _raw_ids(words, bit0, ld, None, 2, n, [0, -1], 7, 0, 0, False)


# ---- sample --------------------------------------------------------------------------------------------------------------------------------------
def _check_sample(got, want, what=None):
    assert (got[0] == want[0]).all(), what
    if got[1] is not None:
        assert (got[1] == want[1]).all(), what
    assert (got[2] == want[2]).all(), what


@pytest.mark.parametrize("on_dev", [False, True])
def test_sample_sizes_and_seeds(on_dev):
    rng = np.random.default_rng(23)
    n, bit0 = 4097, 37
    masks = np.stack([rng.random(n) < 0.01, rng.random(n) < 0.01, rng.random(n) < 0.5, np.zeros(n, bool)])
    words = ref.pack(masks, bit0, spare=1, garbage=rng)
    ld = words.shape[1]
    amask = rng.random(n) < 0.8
    aw = ref.pack(amask[None, :], bit0, spare=1, garbage=rng)[0]
    seeds = [0, 1, 12345, (1 << 64) - 1]                                                           # per-query seeds
    count0 = int(masks[0].sum())
    for k in (1, count0, count0 + 7, 64):                                                          # n = 1, n = count, n > count
        for rpc, id_offset in ((0, 0), (64, 1000), (2048, 1 << 33)):
            got = _raw_sample(words, bit0, ld, None, 4, n, seeds, k, id_offset, rpc, on_dev)
            _check_sample(got, ref.set_sample(masks, seeds, k, id_offset), (k, rpc))
    got = _raw_sample(words, bit0, ld, aw, 4, n, seeds, 32, 7, 0, on_dev, want_hash=False)          # and-words; no out_hash
    _check_sample(got, ref.set_sample(masks & amask, seeds, 32, 7))
    got = _raw_sample(words[2], bit0, 0, None, 1, n, [5], 100, 0, 2048, on_dev)                     # one shared bitmap
    _check_sample(got, ref.set_sample(masks[2:3], [5], 100))
    got = _raw_sample(None, 0, 0, None, 1, 65, [9], 70, 0, 0, on_dev)                               # words == NULL: every row
    _check_sample(got, ref.set_sample(np.ones((1, 65), bool), [9], 70))
    assert (got[0][0, 65:] == -1).all() and (got[1][0, 65:] == ref.NO_HASH).all()


@pytest.mark.parametrize("rpc,chunks", [(6144, 1), (2048, 3)])
def test_sample_1024_of_6000_cuts_and_merges(rpc, chunks):
    """n = 1024 over 6000 set rows: in ONE chunk more than 2048 candidates enter the stream, so the cut runs; in three chunks the merge runs"""
    rng = np.random.default_rng(29)
    n = 6144
    assert set_list_plan(n, 2, True, rpc)[:2] == (chunks, rpc)
    mask = np.zeros((2, n), bool)
    mask[0, rng.choice(n, 6000, replace=False)] = True
    mask[1, rng.choice(n, 6000, replace=False)] = True
    words = ref.pack(mask)
    want = ref.set_sample(mask, [3, 4], 1024, 77)
    for on_dev in (False, True):
        _check_sample(_raw_sample(words, 0, words.shape[1], None, 2, n, [3, 4], 1024, 77, rpc, on_dev), want, on_dev)


# ---- from ids --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_dev", [False, True])
@pytest.mark.parametrize("n,bit0", [(100, 0), (100, 37), (2049, 37), (33, 31), (1, 32)])
def test_from_ids_round_trip(on_dev, n, bit0):
    rng = np.random.default_rng(n + bit0)
    B, m = 3, 40
    ids = rng.integers(0, n, size=(B, m + 2)).astype(np.int64)                                     # ld_ids = m + 2: the last two columns are not read
    ids[:, m:] = n - 1 if n > 1 else 0
    ids[0, ::3] = -1                                                                               # padding
    ids[1, 1::2] = ids[1, 0]                                                                       # duplicates
    ids[2, :m] = -7                                                                                # an empty list
    nw = ref.n_words(bit0, n)
    for allow in (1, 0):
        want = ref.from_ids(ids[:, :m], n, bool(allow))
        words = _raw_from_ids(ids, m, n, bit0, allow, nw + 2, on_dev)
        assert (words[:, :nw] == ref.pack(want, bit0)).all(), allow                                 # whole words: 0 below bit0 and past the rows
        assert (words[:, nw:] == JUNK32).all()                                                     # behind them nothing is touched
        back = _raw_ids(words, bit0, nw + 2, None, B, n, None, n, 0, 0, on_dev)                    # the round trip with vs_set_ids
        assert (back[0] == ref.set_ids(want, None, n)[0]).all() and (back[1] == want.sum(1)).all()
    empty = _raw_from_ids(np.zeros((2, 0), np.int64), 0, n, bit0, 0, nw, on_dev)                   # m = 0, allow = 0: every row
    assert (empty == ref.pack(np.ones((2, n), bool), bit0)).all()


def test_from_ids_device_id_past_the_rows_changes_nothing():
    n, bit0 = 100, 37
    ids = np.array([[5, 100, 99, 1 << 40, -1, 101, 0x7FFFFFFFFFFFFFFF]], np.int64)
    nw = ref.n_words(bit0, n)
    words = _raw_from_ids(ids, ids.shape[1], n, bit0, 1, nw + 4, True)
    assert (words[:, :nw] == ref.pack(ref.from_ids(np.array([[5, 99]]), n), bit0)).all() and (words[:, nw:] == JUNK32).all()
    with pytest.raises(ValueError, match="out of range"):
        _raw_from_ids(ids, ids.shape[1], n, bit0, 1, nw + 4, False)                                # the same list on the host is refused


def test_doc_filter_from_ids_equals_the_mask_path():
    n = 3000
    rng = np.random.default_rng(31)
    ids = rng.integers(0, n, size=(4, 50)).astype(np.int64)
    ids[1, 10:] = -1
    for allow in (True, False):
        f = DocFilter.from_ids(torch.from_numpy(ids), n, allow=allow)
        want = ref.from_ids(ids, n, allow)
        assert f.per_query and (_np(f.words).view(np.uint32) == ref.pack(want)).all()
        assert (_np(DocFilter.from_mask(torch.from_numpy(want)).words) == _np(f.words)).all()
        g = DocFilter.from_ids(ids[0], n, allow=allow)
        assert not g.per_query and (_np(g.words).view(np.uint32) == ref.pack(want[:1])[0]).all()
    assert int(DocFilter.from_ids(np.zeros(0, np.int64), n).count()[0]) == 0 and int(DocFilter.from_ids([], n, allow=False).count()[0]) == n
    with pytest.raises(ValueError, match="out of range"):
        DocFilter.from_ids([0, n], n)
    with pytest.raises(ValueError, match=">= 0"):
        DocFilter.from_ids([0, -1], n)


# ---- index level: tombstones, a group of one, a group of row shards ---------------------------------------------------------------------------------
N, V = 300, 40
CUTS = (0, 5, 101, N)
DEAD = np.array([2, 100, 101, 299])                    # one in the short shard, one on either side of a cut, the last row
_case = {}


def _targets():
    if not _case:
        lens = np.random.default_rng(7).integers(0, 12, size=N)
        ip, ix, va = taref.csr_case(lens, V, seed=71, zeros=0.05)
        whole = DeviceIndex.from_csr(ip, ix, va, V, store_dtype=nat.VS_F32)
        cut = ShardGroup([whole.slice_rows(CUTS[i], CUTS[i + 1] - CUTS[i], device=0) for i in range(3)])
        one = ShardGroup([whole])
        whole.delete_rows(DEAD)
        cut.delete_rows(DEAD)
        live = np.ones(N, bool)
        live[DEAD] = False
        rng = np.random.default_rng(11)
        masks = rng.random((3, N)) < np.array([0.9, 0.5, 0.05])[:, None]
        masks[0, :] = True                                                                         # every row, the dead ones among them
        masks[1, CUTS[1]:CUTS[2]] = False                                                          # no row in the middle shard
        masks[2, [4, 5, 100, 101, 102]] = True                                                     # members on both sides of the cuts, two of them dead
        _case["v"] = ((whole, one, cut), live, masks)
    return _case["v"]


@pytest.mark.parametrize("kind", ["none", "shared", "per_query"])
def test_index_group_of_one_and_row_shards_agree(kind):
    (whole, one, cut), live, masks = _targets()
    if kind == "none":
        f, m = None, live[None, :]
    elif kind == "shared":
        f, m = DocFilter.from_mask(torch.from_numpy(masks[1])), (masks[1] & live)[None, :]
    else:
        f, m = DocFilter.from_mask(torch.from_numpy(masks)), masks & live
    B = m.shape[0]
    counts = ref.set_count(m)
    seeds = [(5 + b) for b in range(B)]
    for name, t in (("whole", whole), ("one", one), ("cut", cut)):
        assert (_np(t.set_count(filter=f)) == counts).all(), name
        res = t.set_ids(filter=f)                                                                  # limit=None: the largest count
        assert isinstance(res, SetIds) and (_np(res.ids) == ref.set_ids(m, None, int(counts.max()))[0]).all() and (_np(res.counts) == counts).all(), name
        assert not np.isin(_np(res.ids), DEAD).any()                                               # deleted rows never appear
        for off, limit in ((0, 4), (2, 5), (3, 200), (90, 30), (int(counts.max()), 3), (1000, 2), (0, 0)):      # (2, 5), (3, 200): over a cut
            res = t.set_ids(filter=f, offset=off, limit=limit)
            want = ref.set_ids(m, [off] * B, limit)
            assert (_np(res.ids) == want[0]).all() and (_np(res.counts) == counts).all(), (name, off, limit)
        if B == 3:
            per = np.array([1, 40, 0], np.int64)                                                   # per-query offsets
            assert (_np(t.set_ids(filter=f, offset=per, limit=60).ids) == ref.set_ids(m, per, 60)[0]).all(), name
        for k in (1, 7, 64, 400):
            res = t.set_sample(k, filter=f, seed=5)
            want = ref.set_sample(m, seeds, k)
            assert isinstance(res, SetSample) and (_np(res.ids) == want[0]).all() and (_np(res.counts) == counts).all(), (name, k)
            assert not np.isin(_np(res.ids), DEAD).any()
    want = ref.set_sample(m, seeds, 7)                                                             # the raw index call returns the hashes as well
    got = _raw_sample(None if f is None else _np(f.words).view(np.uint32), 0, 0 if f is None or not f.per_query else f.ld, None, B, N, seeds, 7, 0, 0,
                      True, index=whole)
    _check_sample(got, want)
    assert (_raw_count(None, 0, 0, None, 1, N, 0, False, index=whole) == N - DEAD.size).all()
    got = _raw_ids(None, 0, 0, None, 1, N, [N - DEAD.size - 2], 4, 10, 64, False, index=whole)
    assert got[0].tolist() == [[307, 308, -1, -1]] and got[1].tolist() == [N - DEAD.size]


# ---- facades ---------------------------------------------------------------------------------------------------------------------------------------
def test_doc_filter_count_ids_pages_sample():
    rng = np.random.default_rng(37)
    n = 5000
    masks = rng.random((3, n)) < np.array([0.3, 0.01, 0.0])[:, None]
    f = DocFilter.from_mask(torch.from_numpy(masks))
    counts = masks.sum(1)
    assert (_np(f.count()) == counts).all()
    res = f.ids()
    assert isinstance(res, SetIds) and tuple(res.ids.shape) == (3, int(counts.max())) and (_np(res.ids) == ref.set_ids(masks, None, int(counts.max()))[0]).all()
    assert (_np(f.ids(offset=[5, 1, 0], limit=9).ids) == ref.set_ids(masks, [5, 1, 0], 9)[0]).all()
    for page_size in (1000, int(counts.max()), 4096):
        pages = list(f.pages(page_size))
        assert len(pages) == -(-int(counts.max()) // page_size) and all((_np(p.counts) == counts).all() for p in pages)
        got = np.concatenate([_np(p.ids) for p in pages], axis=1)
        for b in range(3):                                                                         # the pages, concatenated, are the whole list
            assert (got[b, :counts[b]] == np.nonzero(masks[b])[0]).all() and (got[b, counts[b]:] == -1).all()
    shared = DocFilter.from_mask(torch.from_numpy(masks[1]))
    assert (_np(shared.ids().ids) == np.nonzero(masks[1])[0][None, :]).all() and len(list((~shared & shared).pages(10))) == 1
    s = f.sample(32, seed=9)
    want = ref.set_sample(masks, [9, 10, 11], 32)
    assert isinstance(s, SetSample) and (_np(s.ids) == want[0]).all() and (_np(s.counts) == counts).all()
    assert (_np(f.sample(32, seed=9).ids) == want[0]).all() and (_np(shared.sample(5, seed=10).ids) == want[0][1:2, :5]).all()
    with pytest.raises(ValueError):
        f.sample(0)
    with pytest.raises(ValueError):
        f.ids(offset=[0, 0], limit=1)                                                              # two offsets, three queries


def test_index_list_ids_and_retriever_sample_band(tiny_retriever):
    from vsearch_amd.ir.retriever.index import IndexType
    r = tiny_retriever
    n = 80
    texts = make_texts(n, 5)
    r.build_index(texts, index_type=IndexType.SPARSE)
    idx = r.index
    idx.data = [dict(text=t) for t in texts]
    queries = make_texts(4, 9)
    q_emb = r.process_query(queries, 0, r.encoder_q.config.topk)
    sc = _np(idx.explain(q_emb, torch.arange(n).repeat(4, 1), topn=0).scores).astype(np.float32)
    uniq = [np.unique(sc[b]) for b in range(4)]
    lo = np.array([u[u.size // 4] for u in uniq], np.float32)
    hi = np.array([u[3 * u.size // 4] for u in uniq], np.float32)
    match = sc >= lo[:, None]
    counts = match.sum(1)
    res = idx.list_ids(q_embs=q_emb, min_score=lo)
    assert isinstance(res, SetIds) and (_np(res.ids) == ref.set_ids(match, None, int(counts.max()))[0]).all() and (_np(res.counts) == counts).all()
    assert (_np(idx.list_ids(q_embs=q_emb, min_score=lo, offset=3, limit=5).ids) == ref.set_ids(match, [3] * 4, 5)[0]).all()
    assert (_np(r.retrieve_ids(queries, lo).ids) == _np(res.ids)).all()
    assert _np(idx.count_docs()).tolist() == [n] and (_np(idx.count_docs(idx.match_filter(q_emb, lo))) == counts).all()
    assert _np(idx.list_ids().ids).tolist() == [list(range(n))]
    band = match & ~(sc >= hi[:, None])
    got, got_texts = r.sample_band(queries, lo, hi, 6, seed=3)
    want = ref.set_sample(band, [3, 4, 5, 6], 6)
    assert isinstance(got, SetSample) and (_np(got.ids) == want[0]).all() and (_np(got.counts) == band.sum(1)).all()
    for b in range(4):                                                                             # ids inside the band, texts in their order
        ids_b = [i for i in _np(got.ids)[b].tolist() if i >= 0]
        assert all(lo[b] <= sc[b, i] < hi[b] for i in ids_b) and got_texts[b] == [idx.data[i] for i in ids_b]
    again, _ = r.sample_band(queries, lo, hi, 6, seed=3)                                           # reproducible under the seed
    assert (_np(again.ids) == _np(got.ids)).all()
    assert (_np(idx.sample_ids(6, q_embs=q_emb, min_score=lo, seed=3).ids) == ref.set_sample(match, [3, 4, 5, 6], 6)[0]).all()
    idx.delete([int(_np(got.ids)[0, 0])])                                                          # a deleted document is never sampled or listed
    gone = int(_np(got.ids)[0, 0])
    assert gone not in _np(r.sample_band(queries, lo, hi, 6, seed=3)[0].ids)[0].tolist()
    assert gone not in _np(idx.list_ids().ids)[0].tolist() and _np(idx.count_docs()).tolist() == [n - 1]
