"""GPU tests of fused search (vs_fuse_topk; fuse_topk, DeviceIndex / ShardGroup .search_fused, Index.search_fused / .search_hybrid,
fuse_results, Retriever.retrieve_fused / .retrieve_hybrid) -- run on MI355X.

The contract is tests/_fuse_ref.py.  Everything compares BITS: ids, ranks, n, and view(uint32) of fused and scores.  Every
kernel case runs on host and on device buffers, into outputs filled with junk so that an unwritten slot shows."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import V
from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, FusedResults, ShardGroup, fuse_topk
from vsearch_amd.doc_filter import DocFilter
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

import _fuse_ref as ref
import _mmr_ref as mref

pytestmark = pytest.mark.gpu

F32 = np.float32
MODE_CODE = {"rrf": nat.FUSE_RRF, "sum": nat.FUSE_SUM, "mnz": nat.FUSE_MNZ, "raw": nat.FUSE_RAW}
JUNK = (77, 1.5, 9, -2.5, 5)


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _junk(B, k, L, on_dev):
    out = (np.full((B, k), JUNK[0], np.int64), np.full((B, k), JUNK[1], F32), np.full((B, k, L), JUNK[2], np.int32),
           np.full((B, k, L), JUNK[3], F32), np.full((B,), JUNK[4], np.int32))
    return tuple(torch.from_numpy(o).cuda() for o in out) if on_dev else out


def _p(x):
    if x is None:
        return None
    return C.c_void_p(x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data)


def _native(ids, scores, k, mode, on_dev, weights=None, fill=None, c=60.0, ld=None, stride=None, out=None, L=None, kk=None):
    """vs_fuse_topk itself over lists [L, B, kk] laid out with row stride ld and list stride `stride` -> (return code, outputs)"""
    Lr, B, kkr = ids.shape
    L, kk = Lr if L is None else L, kkr if kk is None else kk               # (0 is an argument to pass on, not a default)
    ld = kkr if ld is None else ld
    stride = B * ld if stride is None else stride
    flat_i, flat_s = ref.layout(ids, scores, max(ld, kkr), max(stride, (B - 1) * max(ld, kkr) + kkr))
    w = None if weights is None else np.ascontiguousarray(weights, dtype=F32)
    f = None if fill is None else np.ascontiguousarray(fill, dtype=F32)
    ldw = 0 if w is None or w.ndim == 1 else w.shape[1]
    ldf = 0 if f is None else f.shape[1]
    args = [flat_i, flat_s, w, f]
    if on_dev:
        args = [None if a is None else torch.from_numpy(a).cuda() for a in args]
    out = _junk(B, max(k, 1), L, on_dev) if out is None else out
    rc = nat.lib().vs_fuse_topk(_p(args[0]), _p(args[1]), L, B, kk, ld, stride, _p(args[2]), ldw, _p(args[3]), ldf, MODE_CODE.get(mode, mode), c, k,
                                *[_p(o) for o in out], 0, None)
    if on_dev:
        torch.cuda.synchronize()
    return rc, out


def _run(ids, scores, k, mode, on_dev, **kw):
    rc, out = _native(ids, scores, k, mode, on_dev, **kw)
    nat.check(rc)
    return dict(zip(ref.NAMES, (_np(o) for o in out)))


def _weights(kind, L, B, seed):
    """None | [L] for the batch | [B, L + 2] per query; small dyadic values, so that sums of them tie"""
    rng = np.random.default_rng(seed)
    if kind == "none":
        return None
    if kind == "batch":
        return rng.choice([0.5, 1.0, 2.0], size=L).astype(F32)
    return rng.choice([0.25, 0.5, 1.0, 2.0], size=(B, L + 2)).astype(F32)


SHAPES = [(1, 1), (1, 1024), (2, 1), (2, 63), (2, 64), (2, 65), (3, 341), (3, 342), (4, 1024), (8, 512), (8, 511), (5, 7)]


# ---- the kernel alone -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,kk", SHAPES)
def test_kernel_equals_the_reference(L, kk):
    B = 3
    ids, sc = ref.kernel_case(L, kk, seed=100 * L + kk, B=B)
    small = L * kk <= 200                                                        # (larger shapes: every mode once, the weight kinds in turn)
    kinds = ("none", "batch", "query")
    combos = [(m, w) for m in ref.MODES for w in kinds] if small else [(m, kinds[(i + L) % 3]) for i, m in enumerate(ref.MODES)]
    union = L * kk                                                               # query 0: the lists are disjoint
    ks = sorted({k for k in (1, union, union + 3, 1024) if k <= 1024})
    ties = 0
    for n, (mode, kind) in enumerate(combos):
        w = _weights(kind, L, B, n)
        fill = None if mode != "raw" or n % 2 else np.full((B, L), -0.125, dtype=F32)
        ld, stride = (kk, B * kk) if n % 2 == 0 else (kk + 3, B * (kk + 3) + 5)
        full = ref.fuse_all(ids, sc, mode, w, 60.0, fill)
        assert len(full[0]) == union and len(full[1]) == kk
        for k in ks:
            want = ref.cut(full, k, L)
            if mode != "rrf" and k == ks[-1]:
                ties += ref.tied_neighbours(want)
            for on_dev in (False, True):
                got = _run(ids, sc, k, mode, on_dev, weights=w, fill=fill, ld=ld, stride=stride)
                ref.assert_equal_bits(got, want, (L, kk, mode, kind, k, on_dev))
    assert ties > 0 or L * kk < 8                                                # the score modes did tie, and the id decided


def _edge_lists():
    """L = 8, kk = 6, seven queries, one edge each"""
    L, kk, B = 8, 6, 7
    ids, sc = ref.kernel_case(L, kk, seed=5, B=B, levels=4)
    ids[:, 0, :] = -1                                                            # 0: nothing at all
    ids[0, 1, 2], ids[0, 1, 3:] = -1, (60_001, 60_002, 60_003)                   # 1: list 0 padded from the middle, live-looking ids behind it
    ids[3, 1, 0] = -1                                                            #    and list 3 empty with a full row of them
    ids[2, 2, 4], ids[2, 2, 5] = ids[2, 2, 1], ids[2, 2, 1]                      # 2: an id three times in one list
    ids[:, 3, 3] = 123_456                                                       # 3: an id in all 8 lists
    ids[0, 4, 0], ids[1, 4, 5], ids[5, 4, 2] = 0, 2 ** 32 - 2, 0                 # 4: the smallest and the largest id
    sc[4, 5, :] = F32(0.375)                                                     # 5: a flat list (mx == mn)
    sc[6, 5, :1], ids[6, 5, 1:] = F32(-2.0), -1                                  #    and a list of one entry
    ids[1, 6, :], sc[1, 6, :] = ids[0, 6, ::-1], sc[0, 6, :]                     # 6: the symmetric case, lists 0 and 1 mirrored
    return ids, sc


def test_kernel_at_its_edges():
    ids, sc = _edge_lists()
    L, B, kk = ids.shape
    k = L * kk + 2
    w0 = np.array([1, 0, 1, 0.5, 0, 2, 1, 1], dtype=F32)
    fill = np.tile(np.array([-1, 0, 0.25, -0.5, 0, 1, 0.125, -2], dtype=F32), (B, 1))
    cases = [("rrf", dict(c=60.0)), ("rrf", dict(c=0.0)), ("rrf", dict(c=0.0, weights=w0)), ("sum", {}), ("sum", dict(weights=w0)),
             ("mnz", {}), ("raw", {}), ("raw", dict(fill=fill)), ("raw", dict(fill=fill, weights=w0))]
    for mode, kw in cases:
        want = ref.fuse(ids, sc, k, mode, **kw)
        # the reference first: the case holds what it claims
        assert want["n"][0] == 0 and (want["ids"][0] == -1).all() and (want["ranks"][0] == -1).all() and np.isneginf(want["fused"][0]).all()
        assert not set(want["ids"][1].tolist()) & {60_001, 60_002, 60_003} and (want["ranks"][1][:, 0] < 2).all() and (want["ranks"][1][:, 3] == -1).all()
        twice = int(ids[2, 2, 1])
        assert (want["ids"][2] == twice).sum() == 1 and want["ranks"][2][want["ids"][2] == twice][0, 2] == 1
        everywhere = want["ranks"][3][want["ids"][3] == 123_456]
        assert everywhere.shape == (1, L) and (everywhere == 3).all()
        assert {0, 2 ** 32 - 2} <= set(want["ids"][4].tolist())
        zero = want["ranks"][4][want["ids"][4] == 0][0]
        assert zero[0] == 0 and zero[5] == 2
        if mode == "sum" and not kw:
            flat = want["ranks"][5][:, 4] >= 0
            assert flat.sum() == kk and (want["ranks"][5][:, 6] == 0).sum() == 1
        if mode == "rrf" and "weights" not in kw:
            assert ref.tied_neighbours(want) > 0
        if "weights" in kw and mode == "rrf":                                    # documents that only the silent lists hold: in the union, fused 0
            only_silent = (want["ranks"][6][:, [0, 2, 3, 5, 6, 7]] < 0).all(axis=1) & (want["ids"][6] >= 0)
            assert only_silent.any() and (want["fused"][6][only_silent] == 0).all()
        for on_dev in (False, True):
            ref.assert_equal_bits(_run(ids, sc, k, mode, on_dev, **kw), want, (mode, sorted(kw), on_dev))
            ref.assert_equal_bits(_run(ids, sc, 5, mode, on_dev, **kw), ref.fuse(ids, sc, 5, mode, **kw), (mode, sorted(kw), on_dev, "k = 5"))


def test_rrf_does_not_read_scores():
    ids, sc = ref.kernel_case(3, 20, seed=9)
    wild = sc.copy()
    wild[0, :, ::3], wild[1, :, 1::4], wild[2, :, 5] = np.nan, np.inf, -np.inf
    wild.view(np.uint32)[2, 0, 7] = 0x7FC12345                                   # a NaN with a payload: the bits pass through
    want, plain = ref.fuse(ids, wild, 64, "rrf"), ref.fuse(ids, sc, 64, "rrf")
    ref.assert_equal_bits(want, plain, "reference", ("ids", "fused", "ranks", "n"))
    assert np.isnan(want["scores"]).any() and np.isposinf(want["scores"]).any() and (want["scores"].view(np.uint32) == 0x7FC12345).any()
    for on_dev in (False, True):
        ref.assert_equal_bits(_run(ids, wild, 64, "rrf", on_dev), want, on_dev)


def test_device_ids_outside_the_range_end_their_list():
    ids, sc = ref.kernel_case(2, 12, seed=4)
    ids[0, 0, 5], ids[1, 1, 0], ids[0, 2, 11], ids[1, 2, 3] = 2 ** 32 - 1, -7, 2 ** 40, 2 ** 63 - 1
    want = ref.fuse(ids, sc, 30, "sum")
    assert want["n"].tolist()[0] == 5 + 12 and (want["ranks"][1][:, 1] == -1).all()
    ref.assert_equal_bits(_run(ids, sc, 30, "sum", True), want, "device")
    rc, out = _native(ids, sc, 30, "sum", False)
    assert rc == nat.VS_EINVAL and "outside" in nat.last_error() and (out[0] == JUNK[0]).all()


def test_kernel_rejects_what_it_cannot_take():
    ids, sc = ref.kernel_case(2, 8, seed=3, B=2)
    big_i, big_s = np.zeros((1, 1, 1025), np.int64), np.zeros((1, 1, 1025), F32)
    five_i, five_s = np.zeros((5, 1, 1024), np.int64), np.zeros((5, 1, 1024), F32)
    bad_id = ids.copy()
    bad_id[1, 1, 7] = 2 ** 32 - 1
    cases = [dict(L=0), dict(L=9), dict(kk=0), dict(big=(big_i, big_s)), dict(big=(five_i, five_s)), dict(k=0), dict(k=1025), dict(ld=7),
             dict(stride=2 * 8 - 1), dict(mode=4), dict(mode=-1), dict(c=-1.0), dict(c=float("inf")), dict(c=float("nan")),
             dict(weights=np.ones((2, 1), F32)), dict(fill=np.zeros((2, 1), F32), mode="raw"), dict(weights=np.array([1, np.inf], F32)),
             dict(fill=np.full((2, 2), np.nan, F32), mode="raw"), dict(ids=bad_id)]
    for kw in cases:
        for on_dev in (False, True):
            kw2 = dict(kw)
            i, s = kw2.pop("big", (kw2.pop("ids", ids), sc))
            if on_dev and ("ids" in kw or any(isinstance(v, np.ndarray) and not np.isfinite(v).all() for v in kw.values())):
                continue                                                         # (the contents of device arrays are not read on the host)
            k, mode = kw2.pop("k", 4), kw2.pop("mode", "rrf")
            out = _junk(i.shape[1], 4, max(i.shape[0], 1), on_dev)
            rc, _ = _native(i, s, k, mode, on_dev, out=out, **kw2)
            assert rc == nat.VS_EINVAL and nat.last_error(), (kw, on_dev)
            with pytest.raises(ValueError):
                nat.check(rc)
            for o, v in zip(out, JUNK):                                          # nothing is written
                assert (_np(o) == v).all(), (kw, on_dev)
    rc, _ = _native(five_i, five_s, 4, "rrf", False)
    assert rc == nat.VS_EINVAL and "4096" in nat.last_error()
    rc, _ = _native(bad_id, sc, 4, "rrf", False)
    assert rc == nat.VS_EINVAL and "4294967295" in nat.last_error()
    dev_i, dev_s = torch.from_numpy(ids).cuda(), torch.from_numpy(sc).cuda()
    with pytest.raises(ValueError, match="host or all"):                         # device lists, host outputs
        fuse_topk(dev_i, dev_s, 4, out=_junk(2, 4, 2, False))
    for bad in (dict(k=0), dict(k=1025), dict(mode="borda"), dict(c=-1.0), dict(weights=np.ones(3, F32)), dict(fill=np.ones((3, 2), F32))):
        with pytest.raises(ValueError):
            fuse_topk(ids, sc, **{"k": 4, **bad})
    with pytest.raises(ValueError, match="4096"):
        fuse_topk(five_i, five_s, 4)


def test_nothing_leaks_between_calls():
    big_i, big_s = ref.kernel_case(4, 1000, seed=21)
    small_i, small_s = ref.kernel_case(2, 9, seed=22, B=5)
    dev = lambda a: torch.from_numpy(a).cuda()
    bi, bs, si, ss = dev(big_i), dev(big_s), dev(small_i), dev(small_s)
    runs = [fuse_topk(bi, bs, 300, "mnz"), fuse_topk(si, ss, 30, "mnz"), fuse_topk(bi, bs, 300, "mnz"), fuse_topk(si, ss, 30, "rrf")]
    torch.cuda.synchronize()
    want_big, want_small = ref.fuse(big_i, big_s, 300, "mnz"), ref.fuse(small_i, small_s, 30, "mnz")
    res = lambda r: dict(zip(ref.NAMES, (_np(t) for t in r)))
    ref.assert_equal_bits(res(runs[0]), want_big, "first")
    ref.assert_equal_bits(res(runs[1]), want_small, "second, smaller")
    ref.assert_equal_bits(res(runs[2]), want_big, "the first again")
    ref.assert_equal_bits(res(runs[3]), ref.fuse(small_i, small_s, 30, "rrf"), "another mode")


def test_fuse_topk_takes_arrays_and_pairs():
    ids, sc = ref.kernel_case(3, 12, seed=8, B=4)
    w = np.array([[1, 2, 0.5, 9]] * 4, dtype=F32)
    want = ref.fuse(ids, sc, 10, "sum", w)
    for conv in (lambda a: a, lambda a: torch.from_numpy(a), lambda a: torch.from_numpy(a).cuda()):
        got = fuse_topk(conv(ids), conv(sc), 10, "sum", weights=w)
        on_dev = isinstance(conv(ids), torch.Tensor) and conv(ids).is_cuda           # device in -> device out; anything else -> numpy
        assert isinstance(got, FusedResults) and (got.ids.is_cuda if on_dev else isinstance(got.ids, np.ndarray))
        ref.assert_equal_bits(dict(zip(ref.NAMES, (_np(t) for t in got))), want, "arrays")
    short = [(ids[0], sc[0]), (ids[1][:, :5], sc[1][:, :5]), (ids[2][:, :9], sc[2][:, :9])]         # lists of different depths
    padded_i, padded_s = ids.copy(), sc.copy()
    padded_i[1, :, 5:], padded_i[2, :, 9:] = -1, -1
    want = ref.fuse(padded_i, padded_s, 40, "rrf", [1, 0.5, 2])
    for conv in (lambda a: a, lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()):
        got = fuse_topk([(conv(i), conv(s)) for i, s in short], None, 40, weights=[1, 0.5, 2])
        ref.assert_equal_bits(dict(zip(ref.NAMES, (_np(t) for t in got))), want, "pairs")
    got = fuse_topk(ids, sc, 7, "raw", fill=np.array([0.5, -1, 0], dtype=F32))                       # fill [L]: every query's
    ref.assert_equal_bits(dict(zip(ref.NAMES, (_np(t) for t in got))), ref.fuse(ids, sc, 7, "raw", fill=np.array([0.5, -1, 0], F32)), "fill")


# ---- search_fused, end to end -----------------------------------------------------------------------------------------------------------
_made = {}


def _rows():
    if "rows" not in _made:
        _made["rows"] = mref.e2e_rows("fp32", V)
    return _made["rows"]


def _index():
    """the unchanging DeviceIndex of the end-to-end cases: mref.N_E2E rows of exact values"""
    if "dev" not in _made:
        _made["dev"] = DeviceIndex.from_csr(*_rows(), V)
    return _made["dev"]


def _variants():
    """three query batches [B_E2E, V] that rank alike but not equally: the queries, the queries without every other term, and with the next
    query's terms mixed in at half weight (dyadic values: the search's scores stay exact sums)"""
    q = mref.e2e_queries(V)
    half = q.copy()
    for b in range(q.shape[0]):
        half[b, np.flatnonzero(q[b])[::2]] = 0
    return [q, half, (q + 0.5 * np.roll(q, 1, axis=0)).astype(F32)]


def _searched(obj, qs, depth, flt=None):
    lists = [obj.search(q, depth, filter=flt) if flt is not None else obj.search(q, depth) for q in qs]
    return np.stack([_np(i) for i, _ in lists]), np.stack([_np(s).astype(F32) for _, s in lists])


def _res(r):
    return dict(zip(ref.NAMES, (_np(t) for t in r)))


def test_search_fused_equals_the_reference():
    dev, qs = _index(), _variants()
    B, k, depth = qs[0].shape[0], 10, 40
    ids, sc = _searched(dev, qs, depth)
    wq = np.random.default_rng(1).choice([0.5, 1.0, 2.0], size=(B, 3)).astype(F32)
    for mode, w in (("rrf", None), ("sum", [1.0, 0.5, 2.0]), ("rrf", wq), ("mnz", None)):
        want = ref.fuse(ids, sc, k, mode, w)
        got = dev.search_fused(qs, k, mode, weights=w, depth=depth)
        assert isinstance(got, FusedResults) and isinstance(got.ids, np.ndarray)
        ref.assert_equal_bits(_res(got), want, (mode, "numpy"))
    assert (want["n"] < 3 * depth).all() and (want["n"] > depth).all()           # the variants' lists overlap, and differ
    stacked = torch.from_numpy(np.stack(qs)).cuda()                              # [L, B, V], torch in -> torch out; the default depth max(4 k, k + 16) = 40
    got = dev.search_fused(stacked, k)
    assert got.ids.is_cuda and got.ranks.dtype == torch.int32 and tuple(got.ranks.shape) == (B, k, 3)
    ref.assert_equal_bits(_res(got), ref.fuse(ids, sc, k, "rrf"), "torch, default depth")
    one = dev.search_fused(qs[:1], k, depth=depth)                               # one list under RRF: the search itself
    top = dev.search(qs[0], k)
    assert (one.ids == top[0]).all() and (one.ranks[:, :, 0] == np.arange(k)).all() and (one.scores[:, :, 0].view(np.uint32) == top[1].view(np.uint32)).all()
    with pytest.raises(ValueError, match="4096"):
        dev.search_fused(qs + qs[:2], k, depth=1000)
    with pytest.raises(ValueError):
        dev.search_fused([], k)


def test_search_fused_under_a_filter_and_deletions():
    dev, qs = DeviceIndex.from_csr(*_rows(), V), _variants()
    k, depth = 10, 32
    allowed = np.random.default_rng(5).random(mref.N_E2E) < 0.5
    few = np.zeros(mref.N_E2E, dtype=bool)
    few[::211] = True                                                            # 10 rows allowed: the lists end in padding
    for mask in (allowed, few):
        flt = DocFilter.from_mask(torch.from_numpy(mask))
        ids, sc = _searched(dev, qs, depth, flt)
        assert mask[ids[ids >= 0]].all() and ((ids == -1).any() or mask is allowed)
        got = _res(dev.search_fused(qs, k, "sum", depth=depth, filter=flt))
        assert mask[got["ids"][got["ids"] >= 0]].all() and (got["ids"] >= 0).any()
        ref.assert_equal_bits(got, ref.fuse(ids, sc, k, "sum"), "filter")
    dead = np.unique(_searched(dev, qs, 5)[0])
    dev.delete_rows(dead)
    ids, sc = _searched(dev, qs, depth)
    got = _res(dev.search_fused(qs, k, depth=depth))
    assert not np.isin(got["ids"], dead).any() and not np.isin(ids, dead).any()
    ref.assert_equal_bits(got, ref.fuse(ids, sc, k, "rrf"), "deleted")
    dev.close()


def test_row_shards_equal_the_unsharded_index():
    whole, qs = _index(), _variants()
    k, depth = 10, 40
    cut_at = 777
    group = ShardGroup([whole.slice_rows(0, cut_at, device=0), whole.slice_rows(cut_at, mref.N_E2E - cut_at, device=0)])
    ids, _ = _searched(whole, qs, depth)
    assert ((ids < cut_at).any(axis=(0, 2)) & (ids >= cut_at).any(axis=(0, 2))).all()     # every query draws rows from both shards
    for mode in ("rrf", "sum"):
        want = _res(whole.search_fused(qs, k, mode, depth=depth))
        ref.assert_equal_bits(_res(group.search_fused(qs, k, mode, depth=depth)), want, ("group", mode))
        got = group.search_fused([torch.from_numpy(q).cuda() for q in qs], k, mode, depth=depth)
        assert got.ids.is_cuda
        ref.assert_equal_bits(_res(got), want, ("group, torch", mode))
    group.close()


def _hybrid_pair():
    """a valued SparseIndex and a BoTIndex over the same rows (the same columns, all values 1)"""
    if "pair" not in _made:
        from vsearch_amd.ir import BoTIndex, SparseIndex
        ip, ix, va = _rows()
        pair = []
        for cls, vals in ((SparseIndex, va), (BoTIndex, np.ones_like(va))):
            idx = cls(device="cuda:0", fp16=False)
            idx.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(vals), size=(mref.N_E2E, V))
            idx.move_to_device("cuda:0")
            pair.append(idx)
        _made["pair"] = tuple(pair)
    return _made["pair"]


def test_index_search_fused_and_fuse_results():
    sp, _ = _hybrid_pair()
    qs = [torch.from_numpy(q) for q in _variants()]
    k, depth = 8, 24
    lists = [sp.search(q, depth) for q in qs]
    ids, sc = np.stack([_np(r.ids) for r in lists]), np.stack([_np(r.scores).astype(F32) for r in lists])
    want = ref.fuse(ids, sc, k, "rrf", [1.0, 0.5, 0.5])
    got = sp.search_fused(qs, k, weights=[1.0, 0.5, 0.5], depth=depth)
    assert got.ids.is_cuda
    ref.assert_equal_bits(_res(got), want, "Index.search_fused")
    from vsearch_amd.ir.retriever.index import fuse_results
    ref.assert_equal_bits(_res(fuse_results(lists, k, weights=[1.0, 0.5, 0.5])), want, "fuse_results")
    short = [lists[0], (lists[1].ids[:, :10], lists[1].scores[:, :10])]          # lists of different depths, on the host
    short = [(i.cpu(), s.cpu()) for i, s in short]
    pad_i, pad_s = ids[:2].copy(), sc[:2].copy()
    pad_i[1, :, 10:] = -1
    ref.assert_equal_bits(_res(fuse_results(short, k, "mnz")), ref.fuse(pad_i, pad_s, k, "mnz"), "fuse_results, host, padded")
    sp.shard_rows([0, 0])
    try:
        ref.assert_equal_bits(_res(sp.search_fused(qs, k, weights=[1.0, 0.5, 0.5], depth=depth)), want, "Index.search_fused, row shards")
    finally:
        _made.pop("pair")                                                        # (the pair's first index is sharded now: the next test builds its own)


def test_search_hybrid_over_a_valued_and_a_binary_index():
    sp, bot = _hybrid_pair()
    q = torch.from_numpy(mref.e2e_queries(V))
    k, depth = 10, 40
    a, b = sp.search(q, depth), bot.search(q, depth)
    ids, sc = np.stack([_np(a.ids), _np(b.ids)]), np.stack([_np(a.scores).astype(F32), _np(b.scores).astype(F32)])
    assert not (ids[0] == ids[1]).all()
    for method, w in (("rrf", None), ("sum", [2.0, 1.0]), ("raw", [1.0, 0.25])):
        got = sp.search_hybrid(q, [(bot, None)], k, method=method, weights=w, depth=depth)
        ref.assert_equal_bits(_res(got), ref.fuse(ids, sc, k, method, w), ("zero", method))
    w = np.array([1.0, 0.25], dtype=F32)
    got = _res(sp.search_hybrid(q, [(bot, q)], k, method="raw", weights=w, depth=depth, missing="score"))
    assert (got["ids"] >= 0).all() and (got["ranks"] >= 0).all()                # every hit is scored on both indexes
    hit_ids = torch.from_numpy(got["ids"]).cuda()
    for l, idx in enumerate((sp, bot)):
        own = _np(idx.explain(q.cuda(), hit_ids, topn=0).scores).astype(F32)
        assert (got["scores"][:, :, l].view(np.uint32) == own.view(np.uint32)).all(), l
    s0, s1 = got["scores"][:, :, 0], got["scores"][:, :, 1]
    assert (got["fused"].view(np.uint32) == ((w[0] * s0).astype(F32) + (w[1] * s1).astype(F32)).astype(F32).view(np.uint32)).all()
    order = np.lexsort((got["ids"], -got["fused"].astype(np.float64)), axis=1)
    assert (order == np.arange(k)).all()
    union = ref.fuse(ids, sc, 2 * depth, "rrf")                                  # and they are the best of the union under the true sums
    ex = [_np(idx.explain(q.cuda(), torch.from_numpy(union["ids"]).cuda(), topn=0).scores).astype(F32) for idx in (sp, bot)]
    want = ref.fuse(np.stack([union["ids"]] * 2), np.stack(ex), k, "raw", w)
    assert (want["ids"] == got["ids"]).all() and (want["fused"].view(np.uint32) == got["fused"].view(np.uint32)).all()
    with pytest.raises(ValueError, match="raw"):
        sp.search_hybrid(q, [(bot, None)], k, method="rrf", missing="score")
    with pytest.raises(ValueError, match="missing"):
        sp.search_hybrid(q, [(bot, None)], k, missing="drop")
    with pytest.raises(ValueError, match="different documents"):
        sp.search_hybrid(q, [(bot, None)], k, method="raw", depth=1024, missing="score")
    from vsearch_amd.ir import SparseIndex
    ip, ix, va = _rows()
    fewer = SparseIndex(device="cuda:0", fp16=False)
    fewer.vector = torch.sparse_csr_tensor(torch.from_numpy(ip[:101]), torch.from_numpy(ix[:ip[100]].astype(np.int64)), torch.from_numpy(va[:ip[100]]), size=(100, V))
    fewer.move_to_device("cuda:0")
    with pytest.raises(ValueError, match="same rows"):
        sp.search_hybrid(q, [(fewer, None)], k)


def test_retriever_retrieve_fused_and_hybrid(tiny_retriever):
    from vsearch_amd.ir.retriever.index import IndexType
    r = tiny_retriever
    n, k = 80, 6
    texts = make_texts(n, 5)
    r.build_index(texts, index_type=IndexType.SPARSE)
    idx = r.index
    variants = [make_texts(4, 9), make_texts(4, 10)]
    embs = [r.process_query(v, 0, r.encoder_q.config.topk) for v in variants]
    got = r.retrieve_fused(variants, k=k, depth=30)
    want = idx.search_fused(embs, k, depth=30)
    assert (_np(got.ids) == _np(want.ids)).all() and (_np(got.scores).view(np.uint32) == _np(want.fused).view(np.uint32)).all()
    lists = [r.retrieve(v, k=30) for v in variants]
    ids, sc = np.stack([_np(x.ids) for x in lists]), np.stack([_np(x.scores).astype(F32) for x in lists])
    ref.assert_equal_bits(_res(want), ref.fuse(ids, sc, k, "rrf"), "retriever, reference")
    cols = _np(idx.get_vectors(torch.tensor([3])).col_indices())                # must=: only documents with document 3's rarest term
    df = _np(idx.doc_freq(cols))
    col = int(cols[df.argmin()])
    assert 0 < df.min() < n
    narrowed = r.retrieve_fused(variants, k=k, depth=30, must=[col])
    lists = [r.retrieve(v, k=30, must=[col]) for v in variants]
    ids, sc = np.stack([_np(x.ids) for x in lists]), np.stack([_np(x.scores).astype(F32) for x in lists])
    assert not np.array_equal(_np(narrowed.ids), _np(got.ids))
    assert (_np(narrowed.ids) == ref.fuse(ids, sc, k, "rrf")["ids"]).all()
    hits = np.unique(_np(narrowed.ids)[_np(narrowed.ids) >= 0])
    rp, ix, _ = idx._device_index().get_rows(hits)
    assert hits.size and all(col in ix[rp[i]:rp[i + 1]] for i in range(hits.size))
    r.build_index(texts, index_type=IndexType.BAG_OF_TOKEN)                      # the same documents as a bag-of-token index
    bot = r.index
    hyb = r.retrieve_hybrid(variants[0], k=k, indexes=[idx, bot], depth=20)
    a, b = idx.search(embs[0], 20), bot.search(embs[0], 20)
    ids, sc = np.stack([_np(a.ids), _np(b.ids)]), np.stack([_np(a.scores).astype(F32), _np(b.scores).astype(F32)])
    ref.assert_equal_bits(_res(hyb), ref.fuse(ids, sc, k, "rrf"), "retrieve_hybrid")
