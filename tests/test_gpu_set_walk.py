"""GPU tests of the shared set walkers (vsearch_amd/csrc/set_walk.h) and of the entry points in front of them (agg_call.h).  ONE set goes
through every consumer of walk_tile, walk_rows and the top-n stream -- facet counts, term counts, term sums, value stats and histogram, the
radix counts of the percentiles, value top-k, the per-label stats, histogram and radix counts, set count, ids and sample -- and each must see
exactly the members a numpy popcount sees.  The features' own suites pin what they compute; this one fails in one obvious place when the walk
changes.  The same set then goes through both forms of every entry point that takes a set as a bitmap: the free form, given the index's live
rows as its second bitmap, must write the very bytes the index-bound form writes; and both forms report errors in one order.

The shape hits every edge of the walk at once: 4161 rows = 2 x 2048 + 65 in chunks of 2048 (three chunks, the last one a full 64-row step and
a one-row step), 9 per-query bitmaps (one full tile of 8 queries and one more), rows 2048 .. 4095 cleared in every query (an all-zero span),
three set rows deleted (the live bitmap is ANDed in), and the same set once more 37 bits into a longer filter, as a shard of a group reads it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex
from vsearch_amd.doc_filter import DocFilter

pytestmark = pytest.mark.gpu

N, V, B, RPC = 2 * 2048 + 65, 40, 9, 2048
N_LABELS, K = 5, 1024
BIT0 = 37
EDGES = [-1.0, -0.25, 0.5, 2.0]                                             # of the histograms: three bins, rows below and above them

_case = {}


def _setup():
    """the index, the per-row payloads and the set, built once: (index, labels, values, masks [B, N] bool, reference member counts [B])"""
    if not _case:
        rng = np.random.default_rng(20)
        nnz = rng.integers(1, 6, N)                                         # every row stores 1..5 non-zero cells
        ip = np.zeros(N + 1, np.int64)
        ip[1:] = np.cumsum(nnz)
        ix = np.concatenate([np.sort(rng.choice(V, k, replace=False)) for k in nnz]).astype(np.int32)
        va = (rng.integers(1, 64, ix.size) / 16.0).astype(np.float16)
        dev = DeviceIndex.from_csr(ip, ix, va, V, store_dtype=nat.VS_F16)
        masks = rng.random((B, N)) < 0.3
        masks[:, 2048:4096] = False                                         # an all-zero span in every query
        masks[:, N - 1] = True                                              # the one-row step holds a set row, deleted below
        dead = np.array([np.flatnonzero(masks[0])[0], 4096 + np.flatnonzero(masks[4, 4096:])[0], N - 1], np.int64)
        assert len(set(dead.tolist())) == 3
        dev.delete_rows(dead)
        live = np.ones(N, bool)
        live[dead] = False
        want = (masks & live).sum(1).astype(np.int64)
        assert (want > 0).all() and (want < K).all()
        labels = torch.from_numpy(rng.integers(0, N_LABELS, N).astype(np.int32)).cuda()
        values = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).cuda()      # every row has a value
        _case["v"] = (dev, labels, values, masks, want)
        _case["live"] = live
    return _case["v"]


def _filter(masks, bit0):
    """the set packed `bit0` bits into a filter that is `bit0` rows longer; the bits in front of it belong to someone else"""
    full = np.ones((B, bit0 + N), bool)
    full[:, bit0:] = masks
    return DocFilter.from_mask(full)


@pytest.mark.parametrize("bit0", [0, BIT0])
def test_every_consumer_sees_the_members_a_popcount_sees(bit0):
    dev, labels, values, masks, want = _setup()
    f = _filter(masks, bit0)
    got = {}
    _, total, _ = dev._facet_call(labels, N_LABELS, f, bit0, RPC)
    got["facet total"] = total
    got["term-counts total"] = dev._term_counts_call(f, bit0, RPC)[1]
    got["term-sums total"] = dev._term_sums_call(f, bit0, RPC, 0)[1]
    count, missing, _, _, _ = dev._value_stats_call(values, nat.VAL_F32, f, bit0, RPC)
    got["value-stats count + missing"] = count + missing
    counts, _ = dev._value_radix_counts_call(values, nat.VAL_F32, 0, 1, None, None, f, bit0, RPC)
    got["radix-count total at level 0"] = counts.sum((1, 2))                # (no row is missing its value)
    ids, _ = dev._value_topk_call(values, nat.VAL_F32, K, 1, 0, f, bit0, RPC)
    got["value_topk ids"] = (ids != -1).sum(1)
    edges = torch.tensor(EDGES, dtype=torch.float32, device=values.device)
    counts, below, above, missing = dev._value_hist_call(values, nat.VAL_F32, edges, f, bit0, RPC)
    got["value-histogram bins + below + above + missing"] = counts.sum(1) + below + above + missing
    count, missing, _, _, _, total, other = dev._facet_value_stats_call(labels, N_LABELS, values, nat.VAL_F32, f, bit0, RPC)
    got["facet-value-stats total"] = total
    got["facet-value-stats count + missing + other"] = count.sum(1) + missing.sum(1) + other
    counts, below, above, missing, total, other = dev._facet_value_hist_call(labels, N_LABELS, values, nat.VAL_F32, edges, f, bit0, RPC)
    got["facet-value-histogram total"] = total
    got["facet-value-histogram cells + other"] = counts.sum((1, 2)) + (below + above + missing).sum(1) + other
    counts, missing, total, other = dev._facet_value_radix_counts_call(labels, N_LABELS, values, nat.VAL_F32, 0, 1, None, None, f, bit0, RPC)
    got["facet-radix-count total at level 0"] = total
    got["facet-radix-count cells + missing + other at level 0"] = counts.sum((1, 2, 3)) + missing.sum(1) + other
    got["set count"] = dev._set_count_call(f, bit0, RPC)[0]
    ids, counts = dev._set_ids_call(f, bit0, None, K, 0, RPC)               # (K is above the largest set: every member is listed)
    got["set ids"] = (ids != -1).sum(1)
    got["set-ids counts"] = counts
    seeds = torch.arange(B, dtype=torch.int64, device=values.device)
    ids, _, counts = dev._set_sample_call(f, bit0, seeds, K, 0, RPC)         # (and every member is sampled)
    got["set sample"] = (ids != -1).sum(1)
    got["set-sample counts"] = counts
    for name, g in got.items():
        g = g.cpu().numpy()
        print(name, g.tolist(), "reference", want.tolist())
        assert (g == np.minimum(K, want) if name == "value_topk ids" else g == want).all(), (name, bit0, g.tolist(), want.tolist())


# ---- the two forms of an entry point: vs_X(words, ..., and_words, ..., n_rows, ..., device) and vs_index_X(idx, words, ...) -------------------
_N = object()                                                               # where the free form takes n_rows
I64, I32, F32 = np.int64, np.int32, np.float32
BINS = nat.VALUE_RADIX_BINS
R = 3


def _pairs(x, out):
    """name of X -> the arguments of vs_X between B and device (vs_index_X: the same without n_rows).  x: the inputs of the call, out(shape,
    dtype): a fresh zeroed output buffer of the call's kind"""
    lab, val, edg, q, seeds, dt = x["labels"], x["values"], x["edges"], x["q"], x["seeds"], nat.VAL_F32
    E, L, low = len(EDGES), N_LABELS, nat.QUANTILE_LOWER
    vec, cell = (lambda d=I64: out((B,), d)), (lambda d=I64: out((B, L), d))
    return {
        "facet_counts": lambda: [lab, _N, L, RPC, cell(), L, vec(), vec()],
        "value_stats": lambda: [val, dt, _N, RPC, vec(), vec(), vec(F32), vec(F32), vec()],
        "value_histogram": lambda: [val, dt, _N, edg, E, RPC, out((B, E - 1), I64), E - 1, vec(), vec(), vec()],
        "value_topk": lambda: [val, dt, _N, 16, 1, 7, RPC, out((B, 16), I64), out((B, 16), F32)],
        "value_quantiles": lambda: [val, dt, _N, q, low, None, R, RPC, out((B, R), F32), out((B, R), I64), vec(), vec()],
        "value_radix_counts": lambda: [val, dt, _N, 0, R, None, None, RPC, out((B, 1, BINS), I64), vec()],
        "facet_value_stats": lambda: [lab, L, val, dt, _N, RPC, cell(), cell(), cell(F32), cell(F32), cell(), L, vec(), vec()],
        "facet_value_histogram": lambda: [lab, L, val, dt, _N, edg, E, RPC, out((B, L, E - 1), I64), E - 1, cell(), cell(), cell(), vec(), vec()],
        "facet_value_quantiles": lambda: [lab, L, val, dt, _N, q, low, None, R, RPC, out((B, L, R), F32), out((B, L, R), I64), cell(), cell(), vec(),
                                          vec()],
        "facet_value_radix_counts": lambda: [lab, L, val, dt, _N, 0, R, None, None, RPC, out((B, L, 1, BINS), I64), cell(), vec(), vec()],
        "set_count": lambda: [_N, RPC, vec()],
        "set_ids": lambda: [_N, None, K, 7, RPC, out((B, K), I64), vec()],
        "set_sample": lambda: [_N, seeds, K, 7, RPC, out((B, K), I64), out((B, K), I32), vec()],
    }


HOST_PAIRS = ["facet_counts", "value_stats", "value_quantiles", "facet_value_stats", "facet_value_radix_counts", "set_sample"]      # one a unit


def _p(a):
    if a is None or isinstance(a, int):
        return a
    return C.c_void_p(a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)


def _both_forms(dev, name, x, words, and_words, ld, bit0, host):
    """-> (bytes the free form wrote, bytes the index-bound form wrote), output by output"""
    written = []
    for free in (True, False):
        outs = []

        def out(shape, dtype):
            outs.append(np.zeros(shape, dtype) if host else torch.zeros(shape, dtype=getattr(torch, np.dtype(dtype).name), device=x["values"].device))
            return outs[-1]
        args = _pairs(x, out)[name]()
        stream = torch.cuda.current_stream(dev.device).cuda_stream or 1
        if free:
            args = [N if a is _N else _p(a) for a in args]
            rc = getattr(nat.lib(), "vs_" + name)(_p(words), bit0, ld, _p(and_words), B, *args, dev.device, stream)
        else:
            args = [_p(a) for a in args if a is not _N]
            rc = getattr(nat.lib(), "vs_index_" + name)(dev._h, _p(words), bit0, ld, B, *args, stream)
        nat.check(rc)
        torch.cuda.synchronize()
        written.append([(o if host else o.cpu().numpy()).tobytes() for o in outs])
    return written


@pytest.mark.parametrize("bit0", [0, BIT0])
def test_free_form_with_the_live_mask_writes_what_the_index_form_writes(bit0):
    dev, labels, values, masks, want = _setup()
    f = _filter(masks, bit0)
    bits = np.zeros(((bit0 + N + 31) // 32) * 32, bool)
    bits[bit0:bit0 + N] = _case["live"]                                     # the live rows packed at bit0, as the free form reads its second bitmap
    live_words = np.packbits(bits, bitorder="little").view(np.uint32).view(np.int32)
    cuda = values.device
    on_dev = {"labels": labels, "values": values, "edges": torch.tensor(EDGES, dtype=torch.float32, device=cuda),
              "q": torch.tensor([0.0, 0.5, 1.0], dtype=torch.float64, device=cuda), "seeds": torch.arange(B, dtype=torch.int64, device=cuda)}
    on_host = {k: v.cpu().numpy() for k, v in on_dev.items()}
    names = list(_pairs(on_dev, None))
    assert len(names) == 13
    for host in (False, True):
        x = on_host if host else on_dev
        words = f.words.cpu().numpy() if host else f.words
        and_words = live_words if host else torch.from_numpy(live_words).to(cuda)
        for name in (HOST_PAIRS if host else names):
            a, b = _both_forms(dev, name, x, words, and_words, f.ld, bit0, host)
            print(name, "host" if host else "device", "bit0", bit0, [len(o) for o in a], "bytes; equal:", [p == q for p, q in zip(a, b)])
            assert a == b, (name, host, bit0)
            assert any(any(o) for o in a), (name, "wrote nothing")
    # the shared reference, through one of the pairs: the forms agree on the right thing
    outs = []
    args = _pairs(on_dev, lambda shape, dtype: outs.append(torch.zeros(shape, dtype=torch.int64, device=cuda)) or outs[-1])["set_count"]()
    nat.check(nat.lib().vs_set_count(_p(f.words), bit0, f.ld, _p(torch.from_numpy(live_words).to(cuda)), B, N, *[_p(a) for a in args[1:]], dev.device,
                                     torch.cuda.current_stream(dev.device).cuda_stream or 1))
    assert (outs[0].cpu().numpy() == want).all()


# a free call with two errors at once -- a device out of range and an argument the device-free checks catch -- reports the argument; a NULL
# index is reported whatever else is wrong.  No kernel is launched.
def _error_cases():
    z = np.zeros(B * N_LABELS * 8, np.int64)                                # any host buffer: no call gets as far as reading it
    bad_edges = np.array([0.0, 1.0, 1.0], np.float32)
    bad_q = np.array([0.5, 1.5], np.float64)
    bad_off = np.array([-2], np.int64)
    L, E, dt = N_LABELS, 3, nat.VAL_F32
    return {
        "facets": ("facet_counts", [z, _N, L, 0, z, L - 1, z, z], "ld_counts = 4 is shorter than n_labels = 5"),
        "values": ("value_histogram", [z, dt, _N, bad_edges, E, 0, z, E - 1, z, z, z], "edges must be strictly ascending"),
        "quantiles": ("value_quantiles", [z, dt, _N, bad_q, 0, None, 2, 0, z, z, z, z], "q[1] = 1.5 is outside [0, 1]"),
        "facet_values": ("facet_value_histogram", [z, L, z, dt, _N, bad_edges, E, 0, z, E - 1, z, z, z, z, z], "edges must be strictly ascending"),
        "facet_quantiles": ("facet_value_radix_counts", [z, L, z, dt, _N, 0, 1, None, None, 0, z, None, z, z],
                            "NULL argument: level 0 needs missing, total and other"),
        "set_list": ("set_ids", [_N, bad_off, 4, 0, 0, z, z], "offsets[0] = -2 is negative"),
    }


@pytest.mark.parametrize("unit", ["facets", "values", "quantiles", "facet_values", "facet_quantiles", "set_list"])
def test_argument_errors_come_before_the_device_and_a_null_index_before_all(unit):
    name, args, message = _error_cases()[unit]
    rc = getattr(nat.lib(), "vs_" + name)(None, 0, 0, None, 1, *[N if a is _N else _p(a) for a in args], 1 << 20, None)
    print(unit, "free form:", rc, nat.last_error())
    assert rc == nat.VS_EINVAL and message in nat.last_error() and "device" not in nat.last_error()
    # the index-bound form with the same bad argument, a negative bit0 and B = 0 on top, and no index
    rc = getattr(nat.lib(), "vs_index_" + name)(None, None, -1, 0, 0, *[_p(a) for a in args if a is not _N], None)
    print(unit, "index form:", rc, nat.last_error())
    assert rc == nat.VS_EINVAL and nat.last_error() == "NULL argument"
