"""CPU checks of the sub-index: the numpy reference (tests/_select_ref.py) against itself, the per-shard split rule in numpy
and in the library (vs_select_split is pure host arithmetic), the order of sorted_by, the plan rule (vs_select_plan), the argument errors of
the C ABI and of the Python layer without a GPU, and the host-only code (vsearch_amd/csrc/select_check.h) run in a stand-alone program under
the host sanitizers.  No device is needed; nothing is loaded into Python under a sanitizer."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from vsearch_amd import _native as nat
from vsearch_amd import device_index as di

import _select_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _csr(rng, lengths, n_cols=50):
    ip = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ix = np.concatenate([np.sort(rng.permutation(n_cols)[:n]) for n in lengths] + [np.zeros(0, np.int64)]).astype(np.int64)
    return ip, ix, rng.standard_normal(int(ip[-1])).astype(np.float32)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


# ---- the reference against itself --------------------------------------------------------------------------------------------------------------------
def test_a_permutation_and_its_inverse_is_the_identity():
    rng = np.random.default_rng(1)
    csr = _csr(rng, [0, 1, 7, 8, 9, 0, 30, 2, 0])
    perm = rng.permutation(9)
    inv = np.argsort(perm)
    once = ref.select_ref(*csr, perm)
    assert not _same(once, csr)
    assert _same(ref.select_ref(*once, inv), csr)


def test_arange_is_the_identity():
    csr = _csr(np.random.default_rng(2), [3, 0, 9, 1])
    assert _same(ref.select_ref(*csr, np.arange(4)), csr)
    part = ref.select_ref(*csr, np.arange(1, 3))
    assert part[0].tolist() == [0, 0, 9] and np.array_equal(part[1], csr[1][3:12])


def test_duplicates_are_kept():
    csr = _csr(np.random.default_rng(3), [2, 0, 5])
    ip, ix, d = ref.select_ref(*csr, [2, 2, 0, 1, 2])
    assert ip.tolist() == [0, 5, 10, 12, 12, 17]
    assert np.array_equal(ix[0:5], ix[5:10]) and np.array_equal(ix[0:5], ix[12:17]) and np.array_equal(ix[0:5], csr[1][2:7])
    assert np.array_equal(d[10:12], csr[2][0:2])
    assert ref.select_ref(csr[0], csr[1], None, [1, 0])[2] is None            # a binary index has no values
    for bad in ([-1], [3], [0, 3]):
        with pytest.raises(IndexError):
            ref.select_ref(*csr, bad)
    with pytest.raises(ValueError):
        ref.select_ref(*csr, [])


# ---- the shard rule: the reference and the library agree -----------------------------------------------------------------------------------------------
CUTS = [0, 10, 25, 40]


def _lib_split(ids, cuts):
    begin = di.split_by_shard(ids, cuts)
    ids = np.asarray(ids, dtype=np.int64)
    return [(s, ids[begin[s]:begin[s + 1]] - cuts[s]) for s in range(len(cuts) - 1) if begin[s + 1] > begin[s]]


def _same_split(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def test_split_ascending_ids():
    ids = [0, 3, 9, 10, 24, 25, 39]
    want = ref.split_by_shard(ids, CUTS)
    assert [(s, l.tolist()) for s, l in want] == [(0, [0, 3, 9]), (1, [0, 14]), (2, [0, 14])]
    assert _same_split(_lib_split(ids, CUTS), want)
    inside = [9, 0, 9, 24, 10, 10, 39]                                        # any order and repeats INSIDE a shard are fine
    assert _same_split(_lib_split(inside, CUTS), ref.split_by_shard(inside, CUTS))
    assert [l.tolist() for _, l in ref.split_by_shard(inside, CUTS)] == [[9, 0, 9], [14, 0, 0], [14]]


def test_split_a_decreasing_shard_sequence_raises():
    for ids in ([3, 12, 9], [30, 24], [39, 0]):
        with pytest.raises(ValueError, match="earlier shard"):
            ref.split_by_shard(ids, CUTS)
        with pytest.raises(ValueError, match="earlier shard"):
            di.split_by_shard(ids, CUTS)
    for ids in ([40], [-1], [3, 99]):
        with pytest.raises(ValueError, match="outside"):
            ref.split_by_shard(ids, CUTS)
        with pytest.raises(ValueError, match="outside"):
            di.split_by_shard(ids, CUTS)


def test_split_an_empty_shard_is_dropped():
    ids = [1, 2, 30, 26]
    want = ref.split_by_shard(ids, CUTS)
    assert [s for s, _ in want] == [0, 2]
    assert _same_split(_lib_split(ids, CUTS), want)
    assert di.split_by_shard(ids, CUTS).tolist() == [0, 2, 2, 4]
    assert [s for s, _ in ref.split_by_shard([12], CUTS)] == [1] and di.split_by_shard([12], CUTS).tolist() == [0, 0, 1, 1]
    assert _same_split(_lib_split([5], [0, 3, 3, 9]), ref.split_by_shard([5], [0, 3, 3, 9]))        # a shard without rows gets nothing


# ---- the order of sorted_by -----------------------------------------------------------------------------------------------------------------------------
def test_sort_order_ties_go_by_id():
    labels = np.array([2, 0, 2, 1, 0, 2])
    assert ref.sort_order(ref.order_key(labels, labels=True), np.ones(6, bool)).tolist() == [1, 4, 3, 0, 2, 5]
    live = np.array([1, 0, 1, 1, 1, 1], bool)                                  # a deleted document is absent
    assert ref.sort_order(ref.order_key(labels, labels=True), live).tolist() == [4, 3, 0, 2, 5]


def test_sort_order_missing_last():
    labels = np.array([-1, 3, 0, -1, 3])
    assert ref.sort_order(ref.order_key(labels, labels=True), np.ones(5, bool)).tolist() == [2, 1, 4, 0, 3]
    years = np.array([1990.0, np.nan, -5.0, np.inf, -np.inf, np.nan], np.float32)
    assert ref.sort_order(ref.order_key(years), np.ones(6, bool)).tolist() == [4, 2, 0, 3, 1, 5]
    ints = np.array([7, np.iinfo(np.int32).min, -3, 7], np.int32)              # INT32_MIN is the missing sentinel of an int32 field
    assert ref.sort_order(ref.order_key(ints), np.ones(4, bool)).tolist() == [2, 0, 3, 1]
    with pytest.raises(TypeError):
        ref.order_key(np.zeros(3, np.float64))


def test_sort_order_zero_signs_tie():
    v = np.array([0.0, -0.0, -1.0, 0.0, -0.0], np.float32)
    key = ref.order_key(v)
    assert key[0] == key[1] == key[3] == key[4] and key[2] < key[0]
    assert ref.sort_order(key, np.ones(5, bool)).tolist() == [2, 0, 1, 3, 4]


def test_sort_order_descending():
    v = np.array([1.0, 3.0, np.nan, 3.0, -2.0, 1.0], np.float32)
    assert ref.sort_order(ref.order_key(v), np.ones(6, bool), descending=True).tolist() == [1, 3, 0, 5, 4, 2]      # ids ascend in a tie, missing last
    labels = np.array([0, 2, -1, 2, 1])
    assert ref.sort_order(ref.order_key(labels, labels=True), np.ones(5, bool), descending=True).tolist() == [1, 3, 4, 0, 2]
    # the keys the facade sorts by on the GPU are the same numbers
    import torch
    assert np.array_equal(di._value_keys(torch.from_numpy(v)).numpy(), ref.order_key(v))
    ints = np.array([5, -5, np.iinfo(np.int32).min, 0], np.int32)
    assert np.array_equal(di._value_keys(torch.from_numpy(ints)).numpy(), ref.order_key(ints))


# ---- the plan rule and the C ABI without a device ---------------------------------------------------------------------------------------------------------
def test_plan_is_pure_host_arithmetic():
    assert di.select_plan(1) == 8 + 8 * 2 + 32
    assert di.select_plan(4096) == 8 * 4096 + 8 * 2 + 32                       # one scan block of 4096 ids
    assert di.select_plan(4097) == 8 * 4097 + 8 * 3 + 32
    assert di.select_plan(21015324) == 8 * 21015324 + 8 * 5132 + 32            # the staged ids dominate: 168 MB at 21 M
    assert nat.lib().vs_select_plan(5, None) == nat.VS_OK                      # the output may be NULL
    for bad, needle in ((0, "empty selection"), (-1, "n must be"), ((1 << 32) - 1, "n must be")):
        with pytest.raises(ValueError, match=needle):
            di.select_plan(bad)


def test_c_abi_argument_errors_without_a_handle():
    L = nat.lib()
    h = C.c_void_p()
    ids = np.array([0, 1], dtype=np.int64)
    p = C.c_void_p(ids.ctypes.data)
    fake = C.c_void_p(1)                                                        # never dereferenced: every check below comes before the handle is read
    assert L.vs_index_select_rows(None, p, 2, 0, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert L.vs_index_select_rows(fake, p, 2, 0, 0, 0, 0, None) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert L.vs_index_select_rows(fake, None, 2, 0, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "ids is NULL" in nat.last_error()
    assert L.vs_index_select_rows(fake, p, 0, 0, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "empty selection" in nat.last_error()
    assert L.vs_index_select_rows(fake, p, -1, 0, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "n must be" in nat.last_error()
    assert L.vs_index_select_rows(fake, p, 2, 0, -1, 0, 0, C.byref(h)) == nat.VS_EINVAL and ">= 0" in nat.last_error()
    assert L.vs_index_select_rows(fake, p, 2, 0, 0, -1, 0, C.byref(h)) == nat.VS_EINVAL and ">= 0" in nat.last_error()
    assert not h.value
    begin = np.zeros(3, dtype=np.int64)
    cuts = np.array([0, 5, 9], dtype=np.int64)
    assert L.vs_select_split(p, 2, None, 2, C.c_void_p(begin.ctypes.data)) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert L.vs_select_split(p, 2, C.c_void_p(cuts.ctypes.data), 0, C.c_void_p(begin.ctypes.data)) == nat.VS_EINVAL and "n_shards" in nat.last_error()


def test_python_layer_argument_errors():
    """what select_rows() refuses before the library is reached.  (The range check of host ids -- an id of -1 and of n_rows -- reads the row count
    of a handle, which only a device makes: the stand-alone program below runs it on the CPU, tests/test_gpu_select.py through the call.)"""
    for bad in (np.zeros(0, np.int64), []):
        with pytest.raises(ValueError, match="empty selection"):
            di._select_ids(bad)
    for bad in (np.array([0.5]), np.array([True]), "3"):
        with pytest.raises(TypeError):
            di._select_ids(bad)
    with pytest.raises(ValueError, match="1-D"):
        di._select_ids(np.zeros((2, 2), np.int64))
    ids, on_dev = di._select_ids(np.array([3, 3, 1], dtype=np.int32))
    assert ids.dtype == np.int64 and ids.tolist() == [3, 3, 1] and not on_dev
    for bad in (dict(rows_extra=-1), dict(packets_extra=-1)):
        with pytest.raises(ValueError, match=">= 0"):
            di._compact_args(bad.get("rows_extra", 0), bad.get("packets_extra", 0))
    with pytest.raises(ValueError, match="1-D"):
        di.split_by_shard([[1, 2]], CUTS)


# ---- the host-only code under the host sanitizers ------------------------------------------------------------------------------------------------
def test_host_checks_under_a_host_sanitizer(tmp_path):
    """select_check.h (the plan rule, every argument check -- a host id of -1 and of n_rows among them --, the capacity rule on the 64-bit packet
    sum and the per-shard split rule against a recount on exact-size heap arrays) in a stand-alone program built with the host compiler under
    AddressSanitizer and UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "select_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "select_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "select_check: ok" in run.stdout, run.stdout + run.stderr
