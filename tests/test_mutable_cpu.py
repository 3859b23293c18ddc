"""CPU-side checks of the mutable index (delete / restore / compact): the boundary (header, exports, struct layout), the loud failure
without a GPU, the argument checks that run before the library is reached, and the text-store remap of compact() as a pure unit."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO
from vsearch_amd import _native as nat
from vsearch_amd import device_index as di

HEADER = os.path.join(REPO, "include", "vsearch_hip.h")
NEW_SYMBOLS = ("vs_index_delete_rows", "vs_index_restore_rows", "vs_index_live_rows", "vs_index_live_bitmap", "vs_index_compact",
               "vs_shard_group_delete_rows", "vs_shard_group_restore_rows")


def test_new_symbols_declared_exported_and_bound():
    text = open(HEADER).read()
    declared = set(re.findall(r"VS_API\s+[\w\s\*]+?\b(vs_\w+)\s*\(", text))
    handle = C.CDLL(nat.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/vsearch_hip.h"
        assert s in nat.EXPORTED_SYMBOLS, f"{s} has no ctypes signature"
        assert hasattr(handle, s), f"{s} is not exported by the library"


def test_index_info_ends_with_n_live_and_matches_the_header(tmp_path):
    names = [f[0] for f in nat.IndexInfo._fields_]
    assert names[-1] == "n_live" and nat.IndexInfo._fields_[-1][1] is C.c_int64

    class Before(C.Structure):
        _fields_ = nat.IndexInfo._fields_[:-1]
    assert C.sizeof(nat.IndexInfo) == C.sizeof(Before) + 8
    # the header's own field order: every member of vs_index_info_t, in order, is a field of IndexInfo
    body = re.search(r"typedef struct vs_index_info_t \{(.*?)\} vs_index_info_t;", open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = re.findall(r"\bint(?:32|64)_t\s+(\w+)\s*;", body)
    assert members == names
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:                                                   # and the size a C compiler gives the header's struct
        src = tmp_path / "sz.c"
        src.write_text('#include <stdio.h>\n#include "vsearch_hip.h"\nint main(void) { printf("%zu %zu", sizeof(vs_index_info_t), '
                       '__builtin_offsetof(vs_index_info_t, n_live)); return 0; }\n')
        exe = tmp_path / "sz"
        subprocess.check_call([cc, "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
        size, off = map(int, subprocess.check_output([str(exe)], text=True).split())
        assert size == C.sizeof(nat.IndexInfo) and off == nat.IndexInfo.n_live.offset


def test_new_entry_points_fail_loudly_without_gpu(have_gpu):
    if have_gpu:
        pytest.skip("GPU present")
    lib = nat.lib()
    assert lib.vs_index_delete_rows(None, None, 0, 0, None) == nat.VS_ENODEVICE
    assert "no CPU fallback" in nat.last_error()
    assert lib.vs_index_restore_rows(None, None, 0, 0, None) == nat.VS_ENODEVICE
    assert lib.vs_index_live_rows(None, None) == nat.VS_ENODEVICE
    assert lib.vs_index_live_bitmap(None, None, 0) == nat.VS_ENODEVICE
    assert lib.vs_index_compact(None, 0, 0, 0, None, None) == nat.VS_ENODEVICE
    assert lib.vs_shard_group_delete_rows(None, None, 0) == nat.VS_ENODEVICE
    assert lib.vs_shard_group_restore_rows(None, None, 0) == nat.VS_ENODEVICE
    dev = di.DeviceIndex(C.c_void_p())
    with pytest.raises(nat.VsearchNativeError, match="no CPU fallback"):
        dev.delete_rows([1, 2])
    with pytest.raises(nat.VsearchNativeError, match="no CPU fallback"):
        dev.restore_rows()
    with pytest.raises(nat.VsearchNativeError, match="no CPU fallback"):
        dev.compact()


def test_argument_errors_come_before_the_library(monkeypatch):
    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(nat, "lib", boom)
    monkeypatch.setattr(nat, "require_device", boom)
    dev = di.DeviceIndex(C.c_void_p())
    group = di.ShardGroup.__new__(di.ShardGroup)
    for obj in (dev, group):
        for bad in (np.array([1.0, 2.0]), [0.5], torch.tensor([1.5]), np.array([True, False]), ["a"]):
            with pytest.raises(TypeError, match="integer"):
                obj.delete_rows(bad)
            with pytest.raises(TypeError, match="integer"):
                obj.restore_rows(bad)
        for bad in (np.zeros((2, 2), dtype=np.int64), torch.zeros((1, 3), dtype=torch.int64), np.int64(3)):
            with pytest.raises(ValueError, match="1-D"):
                obj.delete_rows(bad)
        with pytest.raises(ValueError, match="rows_extra"):
            obj.compact(rows_extra=-1)
        with pytest.raises(ValueError, match="packets_extra"):
            obj.compact(packets_extra=-5)
        with pytest.raises(TypeError, match="rows_extra"):
            obj.compact(rows_extra=1.5)
    ids, on_dev = di._row_ids([3, 1, -1])
    assert ids.dtype == np.int64 and ids.tolist() == [3, 1, -1] and not on_dev
    ids, _ = di._row_ids(torch.tensor([4, 2], dtype=torch.int32))
    assert ids.dtype == np.int64 and ids.tolist() == [4, 2]
    assert di._row_ids([])[0].shape == (0,)
    dev._h = None
    group._h = None


def test_text_store_remap_of_compact():
    from vsearch_amd.ir.retriever.index import remap_text_store
    data = ["d0", "d1", {"text": "d2"}, "d3", "d4"]
    offsets = [0, 10, 25, 40, 77]
    old = np.array([0, 2, 4], dtype=np.int64)
    new_data, new_off = remap_text_store(data, offsets, old)
    assert new_data == ["d0", {"text": "d2"}, "d4"] and new_off == [0, 25, 77]
    assert remap_text_store(data, None, torch.tensor([3]))[0] == ["d3"] and remap_text_store(None, offsets, [1, 3]) == (None, [10, 40])
    assert remap_text_store(data, offsets, []) == ([], [])
    assert data[1] == "d1" and offsets[1] == 10                 # inputs untouched


def test_low_memory_text_store_follows_a_compaction(tmp_path):
    """Index.compact()'s host half on a real data_file, both low_memory modes: what get_sample returns after the remap"""
    import json
    from vsearch_amd.ir import SparseIndex
    from vsearch_amd.ir.retriever.index import remap_text_store
    docs = [f"doc {i} é" for i in range(6)]
    p = tmp_path / "corpus.jsonl"
    p.write_text("".join(json.dumps(d) + "\n" for d in docs), encoding="utf-8")
    old = [1, 2, 5]
    for low in (False, True):
        idx = SparseIndex(None, str(p), low_memory=low)
        idx.data, offsets = remap_text_store(idx.data, idx.offsets if low else None, old)
        if low:
            idx.offsets = offsets
        assert [idx.get_sample(j) for j in range(3)] == [docs[i] for i in old] and len(idx) == 3


def test_facade_has_the_mutable_methods():
    from vsearch_amd.ir import Index, SparseIndex, BoTIndex, Retriever
    for cls in (Index, SparseIndex, BoTIndex):
        for name in ("delete", "restore", "compact", "add", "update"):
            assert callable(getattr(cls, name))
        assert isinstance(cls.n_live, property)
    assert callable(Retriever.delete_documents) and callable(Retriever.compact_index)
