"""query by example without a GPU: no CPU fallback (every new entry point raises VsearchNativeError), and argument errors raised before
the library is called."""
import ctypes as C

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, ShardGroup, resparsify, topk_exclude


def _no_gpu_index():
    return DeviceIndex(C.c_void_p())            # (a handle that never reaches the library: the device check comes first)


def test_new_symbols_are_bound():
    for name in ("vs_index_get_rows", "vs_index_queries_from_rows", "vs_topk_exclude", "vs_shard_group_get_rows",
                 "vs_shard_group_queries_from_rows"):
        assert name in nat.EXPORTED_SYMBOLS


def test_by_example_fails_loudly_without_gpu(have_gpu):
    if have_gpu:
        pytest.skip("GPU present")
    from vsearch_amd.ir import BoTIndex, Index, SparseIndex
    ids = np.zeros((1, 2), np.int64)
    idx = _no_gpu_index()
    with pytest.raises(nat.VsearchNativeError):
        idx.get_rows(np.zeros(2, np.int64))
    with pytest.raises(nat.VsearchNativeError):
        idx.queries_from_rows(ids)
    with pytest.raises(nat.VsearchNativeError):
        idx.search_by_example(ids, 3)
    with pytest.raises(nat.VsearchNativeError):
        topk_exclude(np.zeros((1, 4), np.int64), np.zeros((1, 4), np.float32), ids, 2)
    # the C entry points themselves: VS_ENODEVICE before anything else (no host computation)
    lib = nat.lib()
    assert lib.vs_index_get_rows(None, None, 0, 0, None, None, None, None) == nat.VS_ENODEVICE
    assert lib.vs_index_queries_from_rows(None, None, 1, 1, 1, None, 0, None, 0, 0, 1.0, None, 0, None) == nat.VS_ENODEVICE
    assert lib.vs_topk_exclude(None, None, 1, 1, 1, None, 1, 1, 1, None, None, 0, None) == nat.VS_ENODEVICE
    assert lib.vs_shard_group_get_rows(None, None, 0, None, None, None) == nat.VS_ENODEVICE
    assert lib.vs_shard_group_queries_from_rows(None, None, 1, 1, 1, None, 0, None, 0, 0, 1.0, None, 0) == nat.VS_ENODEVICE
    sp = SparseIndex()
    sp.vector = torch.eye(4).to_sparse_csr()
    for call in (lambda: sp.get_vectors(torch.tensor([0, 1])), lambda: sp.queries_from_rows(torch.tensor([[0, 1]])),
                 lambda: sp.search_by_example(torch.tensor([[0]]), 2)):
        with pytest.raises(nat.VsearchNativeError):
            call()
    bot = BoTIndex()
    bot.vector = torch.eye(4).to_sparse_csr()
    with pytest.raises(nat.VsearchNativeError):
        bot.get_vectors(torch.tensor([0]))
    dense = Index()
    dense.vector = torch.eye(4)
    with pytest.raises(nat.VsearchNativeError):
        dense.get_vectors(torch.tensor([0]))


@pytest.mark.parametrize("cls", [DeviceIndex, ShardGroup])
def test_by_example_argument_errors_before_the_library(cls):
    obj = cls.__new__(cls)                      # no handle: every case below must fail before one is needed
    ids = np.zeros((2, 3), np.int64)
    with pytest.raises(ValueError):
        obj.get_rows(ids)                                                   # get_rows takes [n]
    with pytest.raises(TypeError):
        obj.get_rows(ids[0].astype(np.int32))
    with pytest.raises(ValueError):
        obj.queries_from_rows(ids[0])                                       # [B, m]
    with pytest.raises(ValueError):
        obj.queries_from_rows(np.zeros((2, 0), np.int64))                   # m >= 1
    with pytest.raises(TypeError):
        obj.queries_from_rows(ids.astype(np.int32))
    with pytest.raises(TypeError):
        obj.queries_from_rows(torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError):
        obj.queries_from_rows(ids, weights=np.ones((2, 2), np.float32))     # weights shaped like ids
    with pytest.raises(ValueError):
        obj.queries_from_rows(ids, weights=np.ones(3, np.float32))
    with pytest.raises(ValueError):
        obj.queries_from_rows(ids, q=np.ones((3, 4), np.float32))           # one query row per ids row
    for k in (0, -1):
        with pytest.raises(ValueError):
            obj.search_by_example(ids, k)
    for k in (2.0, True):
        with pytest.raises(TypeError):
            obj.search_by_example(ids, k)
    for a in (0, -5):
        with pytest.raises(ValueError):
            obj.search_by_example(ids, 3, a=a)
    with pytest.raises(TypeError):
        obj.search_by_example(ids, 3, a=1.5)


def test_resparsify_checks_a_before_the_library():
    q = np.ones((2, 5), np.float32)
    for a in (0, 6):
        with pytest.raises(ValueError):
            resparsify(q, a, 0)


def test_index_by_example_argument_errors():
    from vsearch_amd.ir import SparseIndex
    sp = SparseIndex()
    sp.vector = torch.eye(4).to_sparse_csr()
    with pytest.raises(TypeError):
        sp.get_vectors("0")
    with pytest.raises(TypeError):
        sp.queries_from_rows(torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(ValueError):
        sp.search_by_example(torch.zeros(1, 2, dtype=torch.int64), 0)
    with pytest.raises(ValueError):
        sp.search_by_example(torch.zeros(1, 2, dtype=torch.int64), 2, a=0)
