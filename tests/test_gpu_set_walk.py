"""GPU tests of the shared set walkers (vsearch_amd/csrc/set_walk.h): ONE set goes through every consumer of walk_tile, walk_rows and the
top-n stream -- facet counts, term counts, term sums, value stats, the radix counts of the percentiles, value top-k -- and each must see exactly
the members a numpy popcount sees.  The features' own suites pin what they compute; this one fails in one obvious place when the walk changes.

The shape hits every edge of the walk at once: 4161 rows = 2 x 2048 + 65 in chunks of 2048 (three chunks, the last one a full 64-row step and
a one-row step), 9 per-query bitmaps (one full tile of 8 queries and one more), rows 2048 .. 4095 cleared in every query (an all-zero span),
three set rows deleted (the live bitmap is ANDed in), and the same set once more 37 bits into a longer filter, as a shard of a group reads it.
"""
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
    for name, g in got.items():
        g = g.cpu().numpy()
        print(name, g.tolist(), "reference", want.tolist())
        assert (g == np.minimum(K, want) if name == "value_topk ids" else g == want).all(), (name, bit0, g.tolist(), want.tolist())
