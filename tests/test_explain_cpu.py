"""explain without a GPU: no CPU fallback (the rule test_boundary.py applies to search), and argument errors raised before the library
is called."""
import ctypes as C

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, Explanation, ShardGroup


def _no_gpu_index():
    return DeviceIndex(C.c_void_p())            # (a handle that never reaches the library: the device check comes first)


def test_explain_fails_loudly_without_gpu(have_gpu):
    if have_gpu:
        pytest.skip("GPU present")
    from vsearch_amd.ir import BoTIndex, Index, SparseIndex
    with pytest.raises(nat.VsearchNativeError):
        _no_gpu_index().explain(np.ones((1, 4), np.float32), np.zeros((1, 2), np.int64), topn=2)
    with pytest.raises(nat.VsearchNativeError):
        _no_gpu_index().explain(None, np.zeros((1, 2), np.int64), topn=2)
    sp = SparseIndex()
    sp.vector = torch.eye(4).to_sparse_csr()
    with pytest.raises(nat.VsearchNativeError):
        sp.explain(torch.ones(1, 4), torch.zeros(1, 2, dtype=torch.int64))
    with pytest.raises(nat.VsearchNativeError):
        sp.disentangle(torch.zeros(1, 2, dtype=torch.int64))
    bot = BoTIndex()
    bot.vector = torch.eye(4).to_sparse_csr()
    with pytest.raises(nat.VsearchNativeError):
        bot.disentangle(torch.zeros(1, 2, dtype=torch.int64))
    dense = Index()
    dense.vector = torch.eye(4)
    with pytest.raises(nat.VsearchNativeError):
        dense.explain(torch.ones(1, 4), torch.zeros(1, 2, dtype=torch.int64))


@pytest.mark.parametrize("cls", [DeviceIndex, ShardGroup])
def test_explain_argument_errors_before_the_library(cls):
    obj = cls.__new__(cls)                      # no handle: every case below must fail before one is needed
    q = np.ones((2, 4), np.float32)
    ids = np.zeros((2, 3), np.int64)
    for topn in (-1, 1025):
        with pytest.raises(ValueError):
            obj.explain(q, ids, topn=topn)
    for topn in (2.0, True, "3"):
        with pytest.raises(TypeError):
            obj.explain(q, ids, topn=topn)
    with pytest.raises(ValueError):
        obj.explain(q, ids[0], topn=1)
    with pytest.raises(ValueError):
        obj.explain(q, np.zeros((3, 3), np.int64), topn=1)
    with pytest.raises(ValueError):
        obj.explain(q[0], ids, topn=1)
    with pytest.raises(TypeError):
        obj.explain(q, ids.astype(np.int32), topn=1)
    with pytest.raises(TypeError):
        obj.explain(q, torch.zeros(2, 3, dtype=torch.int32), topn=1)


def test_index_explain_argument_errors_and_explanation_fields():
    from vsearch_amd.ir import SparseIndex
    sp = SparseIndex()
    sp.vector = torch.eye(4).to_sparse_csr()
    with pytest.raises(ValueError):
        sp.explain(torch.ones(1, 4), torch.zeros(1, 2, dtype=torch.int64), topn=2000)
    with pytest.raises(TypeError):
        sp.explain(torch.ones(1, 4), torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(TypeError):
        sp.disentangle([[0, 1]])
    assert Explanation._fields == ("cols", "contrib", "scores", "n_matched")
