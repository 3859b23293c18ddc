"""GPU tests of boosted search (vs_index_search_boosted; DeviceIndex / ShardGroup / Index .search_boosted, Retriever.retrieve_boosted) -- run on
MI355X.

The contract is tests/_boost_ref.py: the fp64 row sum of range search before its rounding, plus or times the weighted field
values in fp64, in field order, rounded once.  Everything compares BITS -- ids, counts, bitmap words and scores.view(uint32); no tolerance
anywhere.  The inputs are checked for what makes the comparison mean something: row sums that do not depend on the order of the adds, a boost
that changes every query's top 16, and tied boosted scores in every query."""
import ctypes as C

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, RangeResults, ShardGroup
from vsearch_amd.doc_filter import DocFilter
from test_gpu_facade import FakeTokenizer, make_texts, tiny_retriever  # noqa: F401  (the tiny retriever fixture and its tokenizer)

import _boost_ref as ref
import _range_ref as rr

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
VR = 2000
B_MAX = 9
ALL_HITS = (0, 1, 129, 512, 513, 2048)                               # (512 | 513: the tile scan's limit)
STORES = {"fp32": nat.VS_F32, "fp16": nat.VS_F16, "bin": nat.VS_NONE}
MODES = {ref.ADD: nat.BOOST_ADD, ref.MUL: nat.BOOST_MUL}


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


_cases = {}


def _case(n_rows, store="fp32"):
    """-> (DeviceIndex, queries [B_MAX, VR], fp64 row sums [B_MAX, n_rows], fields); built once, never changed by a test.  fields: two float32
    columns (every 13th value missing; twins as _boost_ref.field_f32 arranges them) and two int32 ones"""
    key = (n_rows, store)
    if key not in _cases:
        ip, ix, va = rr.csr_case(n_rows, VR, seed=n_rows + 40)
        q = rr.sparse_queries(B_MAX, VR, seed=n_rows + 1)
        data = None if store == "bin" else (va.astype(np.float16) if store == "fp16" else va)
        dev = DeviceIndex.from_csr(ip, ix, data, VR, store_dtype=STORES[store])
        fields = [ref.field_f32(n_rows, n_rows + 7), ref.field_i32(n_rows, n_rows + 8), ref.field_f32(n_rows, n_rows + 9, twins=False),
                  ref.field_i32(n_rows, n_rows + 10, lo=0, hi=40)]
        if n_rows >= 1000:
            rows = np.random.default_rng(0).choice(n_rows, size=40, replace=False)
            assert ref.exact_sums(q, ip, ix, va, store, rows, b=n_rows % B_MAX)          # the reference is exact: no order of adds can differ
        _cases[key] = (dev, q, ref.sums(q, ip, ix, va, store), fields)
    return _cases[key]


# the boost configurations: (fields of the case, weights [9, F] or [F], mode)
W4 = np.array([[0.05, -0.002, 0.25, 0.01], [0.0, 0.001, 0.0, -0.02], [0.0, 0.0, 0.0, 0.0], [-0.3, 0.004, 0.1, 0.0], [0.25, 0.0, -0.05, 0.03],
               [1.5, -0.01, 0.0, 0.5], [0.05, 0.0, 0.0, 0.0], [-0.05, -0.001, -0.25, -0.01], [0.125, 0.002, 0.5, 0.02]], F32)
CONFIGS = [((0,), W4[:, :1], ref.ADD), ((0,), W4[:, :1], ref.MUL), ((1,), W4[:, 1:2], ref.ADD), ((0, 1), W4[:, :2], ref.MUL),
           ((1, 2), W4[:, 1:3], ref.ADD), ((0, 1, 2, 3), W4, ref.ADD), ((3, 2, 1, 0), W4, ref.MUL), ((0,), np.array([0.05], F32), ref.ADD),
           ((0,), np.array([0.25], F32), ref.ADD)]
assert {len(c[0]) for c in CONFIGS} == {1, 2, 4} and (W4 == 0).any() and (W4 < 0).any()


def _call(dev, q, fields, w, mode, thr, max_hits, on_dev, flt=None, want_words=True, id_offset=0):
    """vs_index_search_boosted into junk-filled outputs, host or device buffers throughout -> dict of numpy arrays.  thr None: a NULL pointer"""
    n, B, K = int(dev.info().n_rows), q.shape[0], max_hits
    W = (n + 31) // 32
    outs = dict(ids=np.full((B, K), 77, np.int64), scores=np.full((B, K), 1.5, F32), counts=np.full(B, -5, np.int64),
                words=np.full((B, W), 0xA5A5A5A5, np.uint32).view(np.int32))
    ins = dict(q=np.ascontiguousarray(q), w=ref.weights(w, B, len(fields)))
    if thr is not None:
        ins["thr"] = rr.thresholds(thr, B)
    for j, f in enumerate(fields):
        ins[f"f{j}"] = np.ascontiguousarray(f)
    fld = 0
    if flt is not None:
        ins["flt"] = _np(flt.words)
        fld = flt.ld
    if on_dev:
        outs = {k: torch.from_numpy(v).cuda() for k, v in outs.items()}
        ins = {k: torch.from_numpy(v).cuda() for k, v in ins.items()}
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
        torch.cuda.synchronize()
    else:
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
    F = len(fields)
    tab = (C.c_void_p * F)(*[ptr(ins[f"f{j}"]) for j in range(F)])
    dts = (C.c_int32 * F)(*[nat.VAL_F32 if f.dtype == F32 else nat.VAL_I32 for f in fields])
    dt = nat.VS_F16 if q.dtype == np.float16 else nat.VS_F32
    nat.check(nat.lib().vs_index_search_boosted(dev._h, ptr(ins["q"]), dt, q.shape[1], B, ptr(ins["thr"]) if thr is not None else None, K,
                                                ptr(ins["flt"]) if flt is not None else None, 0, fld, id_offset, ptr(outs["ids"]), ptr(outs["scores"]),
                                                ptr(outs["counts"]), ptr(outs["words"]) if want_words else None, W, tab, dts, F, ptr(ins["w"]),
                                                MODES[mode], None))
    return {k: _np(v) for k, v in outs.items()}


def _check(dev, q, S, fields, w, mode, thr, max_hits, allowed=None, flt=None, what=None, on_devs=(False, True)):
    want = ref.search(S, fields, w, mode, thr, max_hits, allowed)
    for on_dev in on_devs:
        rr.assert_equal_bits(_call(dev, q, fields, w, mode, thr, max_hits, on_dev, flt), want, (what, mode, max_hits, on_dev))
    return want


def _mid(X, valid, B, want_hits):
    """per-query floors that about `want_hits` rows pass"""
    out = []
    for b in range(B):
        v = np.sort(X[b][valid[b]])[::-1]
        out.append(v[min(v.size - 1, max(0, want_hits - 1 + 3 * b))] if v.size else 0.0)
    return np.array(out, dtype=F32)


def _pick(case_fields, w, B, cfg):
    idxs, wc, mode = CONFIGS[cfg % len(CONFIGS)]
    return [case_fields[i] for i in idxs], (wc[:B] if wc.ndim == 2 else wc), mode


# ---- rows x batch x max_hits x boost configurations: every slot of junk-filled host and device buffers ----------------------------------------
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 1000, 20000])
def test_equals_the_reference_across_rows_batches_hits_and_boosts(n_rows):
    dev, q, S, cf = _case(n_rows)
    if n_rows >= 1000:
        # the inputs: a field of random() * 10 under weights 0.05 and 0.25 changes every query's top 16, and every query has tied boosted scores
        for w in (0.05, 0.25):
            X, valid = ref.boosted(S, [cf[0]], [w], ref.ADD)
            assert ref.tops_differ(S, X).all() and all(ref.has_ties(X, valid, b) for b in range(B_MAX))
        pairs = [(0, 1), (1, 9), (129, 8), (129, 1), (512, 9), (513, 9), (513, 8), (2048, 1), (512, 8)]
    else:
        pairs = [(mh, B) for mh in ALL_HITS for B in (1, 8, 9)]
    assert {mh for mh, _ in pairs} == set(ALL_HITS) and {B for _, B in pairs} == {1, 8, 9}
    seen = set()
    for i, (max_hits, B) in enumerate(pairs):
        fields, w, mode = _pick(cf, None, B, i)
        seen.add(i % len(CONFIGS))
        X, valid = ref.boosted(S[:B], fields, w, mode)
        thr = _mid(X, valid, B, (5, 140, 600)[i % 3])
        want = _check(dev, q[:B], S[:B], fields, w, mode, thr, max_hits, what=(n_rows, B, i),
                      on_devs=(False, True) if n_rows < 20000 or i % 2 else (True,))
        assert (want["counts"] >= 1).all()
        info = dev.info()
        assert info.queries_per_pass == (8 if max_hits <= 512 else 1) and info.last_path == (1 if max_hits <= 512 else 0)
        if n_rows == 20000:                                          # several chunks, and a ragged last one
            nchunk, rpc = dev.last_range_plan()
            assert nchunk > 1 and (nchunk - 1) * rpc < n_rows <= nchunk * rpc, (max_hits, B, nchunk, rpc)
            assert n_rows % rpc != 0 or (max_hits, B) == (513, 8), (max_hits, B, nchunk, rpc)
    assert seen == set(range(len(CONFIGS)))                          # F = 1, 2, 4; fp32, int32 and mixed fields; both modes
    fields, w, mode = _pick(cf, None, B_MAX, 5)
    want = _check(dev, q, S, fields, w, mode, None, 16, what="no floor")                  # thr NULL: every row; the list is the exact top 16
    assert (want["counts"] == n_rows).all()
    got = _call(dev, q, fields, w, mode, 0.25, 3, on_dev=False, want_words=False)          # no bitmap asked for: the junk stays
    assert (got["words"].view(np.uint32) == 0xA5A5A5A5).all()
    rr.assert_equal_bits(got, ref.search(S, fields, w, mode, 0.25, 3), "no words", ("ids", "scores", "counts"))


# ---- the two scans and the three stores --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["fp32", "fp16", "bin"])
def test_tile_scan_and_one_query_scan_give_identical_bits(store):
    dev, q, S, cf = _case(1000, store)
    for cfg in (3, 5, 6):
        fields, w, mode = _pick(cf, None, B_MAX, cfg)
        X, valid = ref.boosted(S, fields, w, mode)
        thr = _mid(X, valid, B_MAX, 200)
        got = {}
        for qpp in (0, 1):
            dev.set_queries_per_pass(qpp)
            try:
                got[qpp] = _call(dev, q, fields, w, mode, thr, 129, on_dev=True)
                assert dev.info().queries_per_pass == (8 if qpp == 0 else 1)
            finally:
                dev.set_queries_per_pass(0)
        rr.assert_equal_bits(got[0], got[1], ("tile == one query", store, cfg))
        want = ref.search(S, fields, w, mode, thr, 129)
        assert (want["counts"] > 129).all()
        rr.assert_equal_bits(got[0], want, (store, cfg))
    if store == "fp16":                                              # fp16 queries are widened, fp32 ones rounded to the index dtype
        rr.assert_equal_bits(_call(dev, q.astype(np.float16), fields, w, mode, thr, 129, on_dev=True), want, "fp16 queries")


# ---- ties ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qpp", [0, 1])
def test_twin_rows_tie_by_id_or_flip_by_value(qpp):
    n = 1000
    dev, q, S, cf = _case(n)
    f = cf[0]
    src = ref.twin_sources(n)
    live = lambda r: not np.isnan(f[r])
    same = [(s, r) for r, s in src.items() if live(r) and live(s) and f[r] == f[s]]
    flip = [(s, r) for r, s in src.items() if live(r) and live(s) and f[r] > f[s]]       # the later row has the larger value
    assert len(same) > 20 and len(flip) > 10 and all((S[:, r] == S[:, s]).all() for s, r in same + flip)
    dev.set_queries_per_pass(qpp)
    try:
        for mode, w in ((ref.ADD, 0.25), (ref.MUL, 0.25)):
            want = _check(dev, q, S, [f], [w], mode, None, 2048, what=("twins", qpp), on_devs=(True,))
            plain = rr.search(S.astype(F32), -np.inf, 2048)
            flipped = 0
            for b in range(B_MAX):
                pos = {int(i): p for p, i in enumerate(want["ids"][b])}
                ppos = {int(i): p for p, i in enumerate(plain["ids"][b])}
                for s, r in same:                                    # equal S, equal values: the boosted scores tie and the id decides
                    assert pos[s] < pos[r] and (want["scores"][b, pos[s]:pos[r] + 1] == want["scores"][b, pos[s]]).all()
                    assert (np.diff(want["ids"][b, pos[s]:pos[r] + 1]) > 0).all()
                for s, r in flip:                                    # equal S: the plain search lists s first; the boost may put r first
                    assert ppos[s] < ppos[r]
                    flipped += pos[r] < pos[s]
            # "add": S + 0.25 * value is larger for the larger value (but for a rounding tie); "mul": only a pair with S > 0 flips
            assert flipped > (8 * len(flip) if mode == ref.ADD else 0), (mode, flipped, len(flip))
    finally:
        dev.set_queries_per_pass(0)


# ---- thresholds ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qpp", [0, 1])
def test_thresholds(qpp):
    n, B = 1000, 8
    dev, q, S, cf = _case(n)
    qs, Ss = q[:B], S[:B]
    fields, w, mode = [cf[0], cf[1]], W4[:B, :2], ref.ADD
    X, valid = ref.boosted(Ss, fields, w, mode)
    assert valid.all()
    dev.set_queries_per_pass(qpp)
    try:
        want = _check(dev, qs, Ss, fields, w, mode, -np.inf, 129, what="-inf")
        assert (want["counts"] == n).all() and (want["words"][:, -1] == (1 << (n & 31)) - 1).all()
        want = _check(dev, qs, Ss, fields, w, mode, np.inf, 129, what="+inf")
        assert (want["counts"] == 0).all() and (want["ids"] == -1).all() and np.isneginf(want["scores"]).all()
        for zero in (0.0, -0.0):
            want = _check(dev, qs, Ss, fields, w, mode, zero, 2048, what="zero")
            assert (want["counts"] < n).any() and (want["counts"] > 0).all()
        tie, shared = rr.tie_threshold(X, 4)                         # exactly a boosted score several rows share: >= keeps them all, ids ascending
        assert shared >= 2
        want = _check(dev, qs, Ss, fields, w, mode, tie, 2048, what="tie")
        last = want["ids"][4, want["counts"][4] - shared:want["counts"][4]]
        assert (X[4, last] == tie).all() and (np.diff(last) > 0).all()
        half, above = rr.halfway(X, 5, 30)                           # halfway between two adjacent boosted scores
        want = _check(dev, qs, Ss, fields, w, mode, half, 513, what="halfway")
        assert want["counts"][5] == above
        per_q = np.array([-np.inf, np.inf, 0.0, 1.0, tie, half, -1.0, X[7].max()], dtype=F32)
        want = _check(dev, qs, Ss, fields, w, mode, per_q, 128, what="per query")
        assert want["counts"][0] == n and want["counts"][1] == 0 and want["counts"][7] >= 1
        assert dev.info().queries_per_pass == (8 if qpp == 0 else 1)
        nan_q = per_q.copy()                                         # a NaN floor: VS_EINVAL for a host array; on the device it matches no row
        nan_q[3] = np.nan
        with pytest.raises(ValueError, match="NaN"):
            _call(dev, qs, fields, w, mode, nan_q, 5, on_dev=False)
        got = _call(dev, qs, fields, w, mode, nan_q, 5, on_dev=True)
        want = ref.search(Ss, fields, w, mode, nan_q, 5)
        assert want["counts"][3] == 0 and (want["words"][3] == 0).all()
        rr.assert_equal_bits(got, want, "NaN floor on the device")
    finally:
        dev.set_queries_per_pass(0)


@pytest.mark.parametrize("qpp", [0, 1])
def test_weight_errors_and_the_nan_rule(qpp):
    n = 1000
    dev, q, S, cf = _case(n)
    fields, mode = [cf[0], cf[1]], ref.ADD
    w = W4[:, :2].copy()
    w[4, 1] = np.nan
    dev.set_queries_per_pass(qpp)
    try:
        with pytest.raises(ValueError, match="not finite"):
            _call(dev, q, fields, w, mode, None, 5, on_dev=False)
        got = _call(dev, q, fields, w, mode, None, 5, on_dev=True)   # on the device: that query matches nothing, the others are served
        want = ref.search(S, fields, w, mode, None, 5)
        assert want["counts"][4] == 0 and (np.delete(want["counts"], 4) == n).all()
        rr.assert_equal_bits(got, want, "NaN weight on the device")
        # infinite values: +inf - inf and 0 * inf match nothing; other non-finite results go through
        f, g = cf[0].copy(), cf[2].copy()
        empty = np.arange(8, n, 9)
        f[[0, 1, empty[0]]] = [np.inf, -np.inf, np.inf]
        g[[0, 1, 2]] = [-np.inf, -np.inf, np.inf]
        for m in (ref.ADD, ref.MUL):
            want = _check(dev, q, S, [f, g], [1.0, 1.0], m, None, 16, what=("inf", m))
            assert (want["counts"] < n).all() and (want["counts"] >= n - 4).all()
    finally:
        dev.set_queries_per_pass(0)
    for args, match in ((dict(F=0), "n_fields"), (dict(F=5), "n_fields"), (dict(mode=2), "mode"), (dict(dt=7), "field_dtypes"), (dict(null=True), "NULL")):
        cnt = np.zeros(B_MAX, np.int64)
        col = np.ascontiguousarray(cf[0])
        F = args.get("F", 1)
        tab = (C.c_void_p * 5)(*[None if args.get("null") else C.c_void_p(col.ctypes.data)] * 5)
        dts = (C.c_int32 * 5)(*[args.get("dt", nat.VAL_F32)] * 5)
        w1 = np.ones((B_MAX, 5), F32)
        with pytest.raises(ValueError, match=match):
            nat.check(nat.lib().vs_index_search_boosted(dev._h, C.c_void_p(q.ctypes.data), nat.VS_F32, VR, B_MAX, None, 0, None, 0, 0, 0, None, None,
                                                        C.c_void_p(cnt.ctypes.data), None, 0, tab, dts, F, C.c_void_p(w1.ctypes.data),
                                                        args.get("mode", nat.BOOST_ADD), None))


# ---- all weights 0: vs_index_search_range, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["fp32", "fp16", "bin"])
def test_all_weights_zero_is_range_search(store):
    n = 1000
    dev, q, S, cf = _case(n, store)
    f = cf[0].copy()
    f[[0, 1, 2, 8, 17]] = [np.inf, -np.inf, np.inf, -np.inf, np.inf]                      # (row 8 and 17 have no packets)
    plain = S.astype(F32)
    thr = np.sort(plain, axis=1)[:, -150].astype(F32)
    W = (n + 31) // 32
    for qpp in (0, 1):
        dev.set_queries_per_pass(qpp)
        try:
            for max_hits in (0, 129, 600):
                ids, sc, cnt, words = dev._range_call(torch.from_numpy(q).cuda(), thr, max_hits, None, 0, True)     # vs_index_search_range itself
                base = dict(ids=_np(ids), scores=_np(sc), counts=_np(cnt), words=_np(words))
                rr.assert_equal_bits(base, rr.search(plain, thr, max_hits), "range search")
                for mode in (ref.ADD, ref.MUL):
                    for on_dev in (False, True):
                        got = _call(dev, q, [f, cf[1]], np.zeros((B_MAX, 2), F32), mode, thr, max_hits, on_dev)
                        rr.assert_equal_bits(got, base, ("weight 0", store, qpp, mode, max_hits, on_dev))
                got = _call(dev, q, [f], np.full((B_MAX, 1), -0.0, F32), ref.MUL, thr, max_hits, True)
                rr.assert_equal_bits(got, base, ("weight -0.0", store, qpp, max_hits))
        finally:
            dev.set_queries_per_pass(0)
    assert W == base["words"].shape[1]


# ---- filters, deleted rows, id_offset ---------------------------------------------------------------------------------------------------------------
def test_filters_deleted_rows_and_id_offset():
    n = 1000
    ip, ix, va = rr.csr_case(n, VR, seed=n + 40)
    dev, (_, q, S, cf) = DeviceIndex.from_csr(ip, ix, va, VR), _case(n)
    rng = np.random.default_rng(9)
    shared, per_q = rng.random(n) < 0.5, rng.random((B_MAX, n)) < 0.5
    fields, w, mode = _pick(cf, None, B_MAX, 5)
    X, valid = ref.boosted(S, fields, w, mode)
    thr = _mid(X, valid, B_MAX, 200)
    dead = rng.choice(n, size=300, replace=False)
    live = np.ones(n, dtype=bool)
    live[dead] = False
    for deleted in (False, True):
        if deleted:
            dev.delete_rows(dead)
        for qpp in (0, 1):
            dev.set_queries_per_pass(qpp)
            for allowed in (None, shared, per_q):
                flt = DocFilter.from_mask(torch.from_numpy(allowed)) if allowed is not None else None
                a = (live if deleted else None) if allowed is None else (allowed & live if deleted else allowed)
                for max_hits in (0, 64, 600):
                    _check(dev, q, S, fields, w, mode, thr, max_hits, a, flt, what=("filter", qpp, deleted), on_devs=(True,))
                want = _check(dev, q, S, fields, w, mode, None, 7, a, flt, what="filter, no floor", on_devs=(True,))
                assert (want["counts"] == (np.broadcast_to(a, (B_MAX, n)).sum(axis=1) if a is not None else n)).all()
    dev.set_queries_per_pass(0)
    got = _call(dev, q, fields, w, mode, thr, 40, on_dev=True, id_offset=123456789012)
    rr.assert_equal_bits(got, ref.search(S, fields, w, mode, thr, 40, live, id_offset=123456789012), "id_offset")
    dev.close()


# ---- the Python methods and the shard rule ------------------------------------------------------------------------------------------------------------
def test_methods():
    n = 1000
    dev, q, S, cf = _case(n)
    fields, w, mode = [cf[0], cf[3]], W4[:, :2], "mul"
    X, valid = ref.boosted(S, fields, w, mode)
    thr = _mid(X, valid, B_MAX, 150)
    want = ref.search(S, fields, w, mode, thr, 100)
    for kind in ("numpy", "cpu", "cuda"):
        conv = (lambda a: a) if kind == "numpy" else (lambda a: torch.from_numpy(np.ascontiguousarray(a))) if kind == "cpu" else \
               (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
        qq = conv(q)
        res = dev.search_boosted(qq, [conv(f) for f in fields], conv(w) if kind != "cpu" else w, mode=mode, min_score=thr)
        assert isinstance(res, RangeResults) and type(res.ids) is type(qq) and (not isinstance(qq, torch.Tensor) or res.ids.device == qq.device)
        rr.assert_equal_bits(dict(ids=_np(res.ids), scores=_np(res.scores), counts=_np(res.counts)), want, ("search_boosted", kind), ("ids", "scores", "counts"))
        assert (_np(dev.count_boosted(qq, fields, w, mode=mode, min_score=thr)) == want["counts"]).all()
    res = dev.search_boosted(q, [torch.from_numpy(fields[0]).cuda(), fields[1]], w, mode=mode, min_score=thr, max_hits=5, id_offset=1000)
    assert isinstance(res.ids, np.ndarray) and (res.ids == want["ids"][:, :5] + 1000).all()         # (a device column with host queries)
    bf = dev.boosted_filter(q, fields, w, mode=mode, min_score=thr)
    assert isinstance(bf, DocFilter) and bf.per_query and bf.n_queries == B_MAX and (_np(bf.words).view(np.uint32) == want["words"]).all()
    top = dev.search_boosted(q, fields, w, mode=mode, max_hits=10)                                  # no floor: the exact top 10
    rr.assert_equal_bits(dict(ids=top.ids, scores=top.scores, counts=top.counts), ref.search(S, fields, w, mode, None, 10), "top 10", ("ids", "scores", "counts"))
    with pytest.raises(ValueError, match="finite"):
        dev.search_boosted(q, fields, np.full(2, np.nan, F32))
    with pytest.raises(ValueError, match="one entry per row"):
        dev.search_boosted(q, [fields[0][:-1]], [1.0])


@pytest.mark.parametrize("store", ["fp32", "bin"])
def test_row_shards_equal_the_unsharded_index(store):
    n = 1000
    whole, q, S, cf = _case(n, store)
    ndev = torch.cuda.device_count()
    bounds = [0, 437, 438, n]                                        # three uneven shards; two of them do not start on a word
    shards = [whole.slice_rows(bounds[i], bounds[i + 1] - bounds[i], device=i % ndev) for i in range(3)]
    group = ShardGroup(shards)
    allowed = np.random.default_rng(2).random((B_MAX, n)) < 0.7
    flt = DocFilter.from_mask(torch.from_numpy(allowed))
    for cfg in (4, 6):
        fields, w, mode = _pick(cf, None, B_MAX, cfg)
        X, valid = ref.boosted(S, fields, w, mode)
        thr = _mid(X, valid, B_MAX, 120)
        for a, f in ((None, None), (allowed, flt)):
            for max_hits in (0, 30, 600):
                want = ref.search(S, fields, w, mode, thr, max_hits, a)
                for qq in (q, torch.from_numpy(q).cuda()):
                    res = group.search_boosted(qq, fields, w, mode=mode, min_score=thr, max_hits=max_hits, filter=f)
                    assert type(res.ids) is type(qq)
                    rr.assert_equal_bits(dict(ids=_np(res.ids), scores=_np(res.scores), counts=_np(res.counts)), want, ("group", max_hits),
                                          ("ids", "scores", "counts"))
                one = whole.search_boosted(q, fields, w, mode=mode, min_score=thr, max_hits=max_hits, filter=f)
                rr.assert_equal_bits(dict(ids=one.ids, scores=one.scores, counts=one.counts), want, "whole", ("ids", "scores", "counts"))
            assert (_np(group.count_boosted(q, fields, w, mode=mode, min_score=thr, filter=f)) == want["counts"]).all()
            bf = group.boosted_filter(q, fields, w, mode=mode, min_score=thr, filter=f)
            assert bf.n_rows == n and (_np(bf.words).view(np.uint32) == want["words"]).all()
    group.close()


# ---- the matrix cores ------------------------------------------------------------------------------------------------------------------------------------
def test_dense_matrix_index():
    n, V, B = 1500, 96, 9
    mat, q = rr.dense_case(n, V, B, seed=2)
    S = (q.astype(F64) @ mat.astype(F64).T)
    assert (S == S.astype(F32)).all() and (S.astype(F32) == rr.scores(q, *rr.dense_to_csr(mat))).all()   # sums of m / 65536: exact in fp32 and fp64 alike
    dense = DeviceIndex.from_dense(mat)
    assert dense.info().kind == nat.VS_KIND_DENSE and dense.info().n_packets == 0
    cf = [ref.field_f32(n, 3, twins=False) / F32(64), ref.field_i32(n, 4, lo=-3, hi=4)]
    cf[0][[0, 1]] = [np.inf, -np.inf]
    allowed = np.random.default_rng(1).random((B, n)) < 0.6
    flt = DocFilter.from_mask(torch.from_numpy(allowed))
    for fields, w, mode in (([cf[0]], W4[:, :1], ref.ADD), (cf, W4[:, :2], ref.MUL), (cf[::-1], np.zeros(2, F32), ref.ADD)):
        X, valid = ref.boosted(S, fields, w, mode)
        for max_hits in (0, 1, 129, 2048):
            for thr in (None, np.inf, _mid(X, valid, B, 40)):
                _check(dense, q, S, fields, w, mode, thr, max_hits, what="dense")
        want = _check(dense, q, S, fields, w, mode, _mid(X, valid, B, 300), 129, allowed, flt, what="dense, filtered", on_devs=(True,))
        assert (want["counts"] > 100).all()
    ids, sc, cnt, words = dense._range_call(torch.from_numpy(q).cuda(), np.full(B, 0.01, F32), 129, None, 0, True)
    got = _call(dense, q, cf[::-1], np.zeros(2, F32), ref.MUL, 0.01, 129, True)                     # weight 0: the range search of the matrix cores
    rr.assert_equal_bits(got, dict(ids=_np(ids), scores=_np(sc), counts=_np(cnt), words=_np(words)), "dense, weight 0")
    dense.delete_rows(np.arange(0, n, 3))
    live = np.ones(n, dtype=bool)
    live[::3] = False
    _check(dense, q, S, cf, W4[:, :2], ref.ADD, None, 513, allowed & live, flt, what="dense, filtered, deleted", on_devs=(True,))
    dense.close()


def test_a_csr_index_wider_than_the_query_image_is_unsupported():
    V = 32764
    ip, ix, va = rr.csr_case(64, V, seed=1)
    dev = DeviceIndex.from_csr(ip, ix, va, V)
    with pytest.raises(NotImplementedError, match="too wide"):
        dev.search_boosted(rr.sparse_queries(2, V, seed=2), [np.zeros(64, F32)], [1.0])
    dev.close()


# ---- the facade -------------------------------------------------------------------------------------------------------------------------------------------
def test_retriever_and_index_facade(tiny_retriever):
    from vsearch_amd.ir import SparseIndex
    from vsearch_amd.ir.retriever.index import IndexType
    r = tiny_retriever
    n = 80
    r.build_index(make_texts(n, 5), index_type=IndexType.SPARSE)
    idx = r.index
    rng = np.random.default_rng(5)
    recency, views = (rng.random(n) * 10).astype(F32), rng.integers(0, 1000, n)
    recency[::13] = np.nan
    idx.set_values("recency", recency)
    idx.set_values("views", views)
    queries = make_texts(4, 9)
    q_emb = r.process_query(queries, 0, r.encoder_q.config.topk)
    boosts = {"recency": 0.3, "views": [0.001, 0.0, -0.002, 0.01]}
    got = r.retrieve_boosted(queries, k=20, boosts=boosts)
    assert isinstance(got, RangeResults) and (_np(got.counts) == n).all() and (_np(got.ids) >= 0).all()
    same = idx.search_boosted(q_emb, 20, boosts=boosts)
    assert (_np(same.ids) == _np(got.ids)).all() and (_np(same.scores) == _np(got.scores)).all()
    # ... which is the device index's call on the stored columns
    target, gpu = idx._explain_target()
    qd = q_emb.to(f"cuda:{gpu}")
    qd = qd.to(idx._dtype) if idx._dtype in (torch.float16, torch.float32) else qd.float()
    w = np.array([[0.3, 0.001], [0.3, 0.0], [0.3, -0.002], [0.3, 0.01]], F32)
    direct = target.search_boosted(qd.contiguous(), [idx._value_field("recency"), idx._value_field("views")], w, max_hits=20)
    assert (_np(direct.ids) == _np(got.ids)).all() and (_np(direct.scores.to(idx._dtype)) == _np(got.scores)).all()
    plain = idx.search_range(q_emb, -np.inf, max_hits=20)
    assert (_np(plain.ids) != _np(got.ids)).any()                                                   # the boost changes the list
    zero = idx.search_boosted(q_emb, 20, boosts={"recency": 0.0, "views": 0}, mode="mul")           # weight 0 is search_range
    assert (_np(zero.ids) == _np(plain.ids)).all() and (_np(zero.scores) == _np(plain.scores)).all()
    heavy = idx.search_boosted(q_emb, 1, boosts={"views": 1e6})                                     # a heavy boost ranks by the field
    assert (views[_np(heavy.ids)[:, 0]] == views.max()).all()
    cols = _np(idx.get_vectors(torch.tensor([3])).col_indices())                                    # must=: only the documents with that term
    col = int(cols[_np(idx.doc_freq(cols)).argmin()])
    df = int(_np(idx.doc_freq(np.array([col])))[0])
    narrowed = r.retrieve_boosted(queries, k=n, boosts=boosts, must=[col])
    assert 0 < df < n and (_np(narrowed.counts) == df).all()
    with pytest.raises(KeyError, match="year"):
        r.retrieve_boosted(queries, k=5, boosts={"year": 1.0})
    # a row-sharded SparseIndex against the reference
    ip, ix, va = rr.csr_case(1000, VR, seed=1040)
    _, q, S, cf = _case(1000)
    sp = SparseIndex(device="cuda:0", fp16=False)
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(va), size=(1000, VR))
    sp.move_to_device("cuda:0")
    sp.set_values("a", cf[0])
    sp.set_values("b", np.where(ref.missing(cf[1]), 0, cf[1]), missing=ref.missing(cf[1]))          # (INT32_MIN is said through missing=)
    assert (_np(sp.get_values("b")) == cf[1]).all()
    want = ref.search(S, [cf[0], cf[1]], W4[:, :2], ref.ADD, None, 150)
    for sharded in (False, True):
        if sharded:
            sp.shard_rows([0, 0, 0])
            assert sp.shards is not None and len(sp.shards) == 3
        res = sp.search_boosted(torch.from_numpy(q), 150, boosts={"a": W4[:, 0], "b": W4[:, 1]})
        rr.assert_equal_bits(dict(ids=_np(res.ids), scores=_np(res.scores), counts=_np(res.counts)), want, ("SparseIndex", sharded), ("ids", "scores", "counts"))
