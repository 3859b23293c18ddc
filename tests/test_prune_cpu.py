"""CPU checks of index pruning: the numpy reference (tests/_prune_ref.py) against the reference's own rule -- the oracle's
embed_mask at topk = m equals the pruned embed_mask at topk = 768 --, the reference's edges, the plan rule (vs_prune_plan is pure host
arithmetic), the argument errors of the C ABI and of the Python layer without a GPU, and the host-only code (vsearch_amd/csrc/prune_check.h)
run in a stand-alone program under the host sanitizers.  No device is needed; nothing is loaded into Python under a sanitizer."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from vsearch_amd import _native as nat
from vsearch_amd import device_index as di

import _prune_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB, SHIFT = 2999, 999                                # V = 2000 columns


# ---- the numpy reference against the reference's own rule -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def embedding():
    """E [32, 2000]: every row a scaled permutation of 1..2000 -- positive and tie-free --, and random token ids (some below the shift)"""
    rng = np.random.default_rng(11)
    V = VOCAB - SHIFT
    E = np.stack([(rng.permutation(V) + 1).astype(np.float32) * np.float32(2.0 ** rng.integers(-6, 3)) for _ in range(32)])
    ids = rng.integers(0, VOCAB, size=(32, 40)).astype(np.int64)
    for row in E:
        assert np.unique(row).size == V                 # tie-free: torch.topk leaves ties open, so the comparison stays inside the contract
    return E, ids


@pytest.mark.parametrize("lexical", [True, False])
@pytest.mark.parametrize("m", [1, 8, 100, 768])
def test_reference_equals_the_oracles_embed_mask(embedding, m, lexical):
    E, ids = embedding
    stored = ref.dense_to_csr(oracle.embed_mask(E, ids, VOCAB, SHIFT, topk=768, activate_lexical=lexical))
    protect = ref.dense_to_csr(oracle.bow_mask(ids, VOCAB, SHIFT))[:2] if lexical else None
    want = ref.dense_to_csr(oracle.embed_mask(E, ids, VOCAB, SHIFT, topk=m, activate_lexical=lexical))
    ip, ix, d, kept = ref.prune_ref(*stored, topk=m, protect=protect)
    assert np.array_equal(ip, want[0]) and np.array_equal(ix, want[1])
    assert np.array_equal(d.view(np.uint32), want[2].view(np.uint32))
    assert np.array_equal(kept, np.diff(want[0]))
    if lexical and m < 768:
        assert (kept > m).any()                         # protected cells were added on top of the m


# ---- the reference's edges ------------------------------------------------------------------------------------------------------------------------
def _one_row(vals, cols=None):
    vals = np.asarray(vals, dtype=np.float32)
    cols = np.arange(len(vals)) if cols is None else np.asarray(cols)
    return np.array([0, len(vals)]), cols, vals


def _kept_cols(*a, **k):
    return ref.prune_ref(*a, **k)[1].tolist()


def test_all_equal_rows_keep_the_first_m():
    assert _kept_cols(*_one_row([2.0] * 9, cols=[5, 3, 8, 1, 7, 0, 2, 6, 4]), topk=4) == [5, 3, 8, 1]


def test_zero_signs_tie_and_nan_ranks_last():
    ip, ix, d = _one_row([-0.0, 0.0, -1.0, 0.0])
    assert _kept_cols(ip, ix, d, topk=2) == [0, 1]      # -0.0 ties +0.0: stored order decides
    ip, ix, d = _one_row([np.nan, -np.inf, 1.0, -np.nan, np.inf])
    assert _kept_cols(ip, ix, d, topk=3) == [1, 2, 4]   # -inf above a NaN
    assert _kept_cols(ip, ix, d, topk=4) == [0, 1, 2, 4]   # then the NaNs in stored order
    assert _kept_cols(ip, ix, d, min_value=-np.inf) == [1, 2, 4]   # a NaN is never >=
    out = ref.prune_ref(ip, ix, d, topk=4)
    assert np.array_equal(out[2].view(np.uint32), d[[0, 1, 2, 4]].view(np.uint32))     # stored bits, the NaN's payload included


def test_m_at_least_n_is_the_identity():
    ip, ix, d = _one_row([3.0, 1.0, 2.0])
    for m in (3, 4, 65535, 0, None):
        out = ref.prune_ref(ip, ix, d, topk=m)
        assert np.array_equal(out[0], ip) and np.array_equal(out[1], ix) and np.array_equal(out[2], d) and out[3].tolist() == [3]


def test_protected_cells_are_added_and_ineligible_ones_dropped():
    ip, ix, d = _one_row([5.0, 1.0, 4.0, 0.5, 3.0], cols=[10, 11, 12, 13, 14])
    prot = (np.array([0, 3]), np.array([13, 10, 99]))
    assert _kept_cols(ip, ix, d, topk=2) == [10, 12]
    assert _kept_cols(ip, ix, d, topk=2, protect=prot) == [10, 12, 13]       # 13 survives, and 12 is not displaced by the protected 10
    keep = np.ones(100, dtype=bool)
    keep[13] = False
    assert _kept_cols(ip, ix, d, topk=2, protect=prot, col_keep=keep) == [10, 12]      # an ineligible protected cell is dropped
    assert _kept_cols(ip, ix, d, topk=2, protect=prot, min_value=1.0) == [10, 12]
    keep[10] = False
    assert _kept_cols(ip, ix, d, topk=2, protect=prot, col_keep=keep) == [12, 14]      # the top m is taken over the eligible cells


def test_empty_rows_and_binary_rows():
    ip, ix, d, kept = ref.prune_ref(np.array([0, 0, 2, 2]), np.array([4, 1]), np.array([1.0, 2.0], np.float32), topk=1)
    assert ip.tolist() == [0, 0, 1, 1] and ix.tolist() == [1] and kept.tolist() == [0, 1, 0]
    keep = np.array([True, False, True, True, False])
    ip, ix, d, kept = ref.prune_ref(np.array([0, 3, 3]), np.array([4, 0, 3]), None, col_keep=keep)
    assert ip.tolist() == [0, 2, 2] and ix.tolist() == [0, 3] and d is None
    with pytest.raises(AssertionError):
        ref.prune_ref(np.array([0, 1]), np.array([0]), None, topk=1)


# ---- the plan rule and the C ABI without a device -------------------------------------------------------------------------------------------------
def test_plan_values():
    reg, scratch, lds = di.prune_plan(21015324, 21015324 * 96, 29523, nat.VS_F32, 256, True)
    assert reg == 1024 and reg >= 768                   # the 96 packets of a 768-cell row are selected from registers
    assert scratch == 21015324 * 96 + 4 * 21015324 + 8 * (5131 + 1) + 8     # 2 GB of keep bytes, the kept counts, the block sums
    assert lds == 4 * (923 + 4 * 256 + 4 * 923)
    assert di.prune_plan(1000, 5000, 300, nat.VS_F16) == (1024, 5000 + 4000 + 16 + 8, 4 * (10 + 1024))
    assert di.prune_plan(10, 10, 65535, nat.VS_NONE, 0, True)[2] == 4 * (2048 + 1024 + 4 * 2048) <= 64 * 1024
    assert di.prune_plan(0, 0, 5, nat.VS_F32, 3)[0] == 1024
    L = nat.lib()
    assert L.vs_prune_plan(1, 1, 5, nat.VS_F32, 0, 0, None, None, None) == nat.VS_OK          # every output may be NULL


def test_plan_errors():
    for args, exc, needle in (((-1, 0, 5, nat.VS_F32), ValueError, "n_rows"), (((1 << 32) - 1, 0, 5, nat.VS_F32), ValueError, "n_rows"),
                              ((1, 1 << 32, 5, nat.VS_F32), ValueError, "n_packets"), ((1, 1, 0, nat.VS_F32), ValueError, "n_cols"),
                              ((1, 1, 65536, nat.VS_F32), NotImplementedError, "uint16"), ((1, 1, 5, nat.VS_F32, -1), ValueError, "topk must"),
                              ((1, 1, 5, nat.VS_F32, 65536), ValueError, "topk must"), ((1, 1, 5, nat.VS_NONE, 3), ValueError, "binary"),
                              ((1, 1, 5, nat.VS_I64), ValueError, "store_dtype")):
        with pytest.raises(exc, match=needle):
            di.prune_plan(*args)


def test_c_abi_argument_errors_without_a_handle():
    L = nat.lib()
    h = C.c_void_p()
    nan = C.c_float(float("nan"))
    assert L.vs_index_prune(None, 5, nan, None, None, 0, 0, 0, C.byref(h), None) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert L.vs_index_prune(None, -1, nan, None, None, 0, 0, 0, C.byref(h), None) == nat.VS_EINVAL and "topk must" in nat.last_error()
    assert L.vs_index_prune(None, 65536, nan, None, None, 0, 0, 0, C.byref(h), None) == nat.VS_EINVAL and "topk must" in nat.last_error()
    assert L.vs_index_prune(None, 5, nan, None, None, -1, 0, 0, C.byref(h), None) == nat.VS_EINVAL and ">= 0" in nat.last_error()
    assert L.vs_index_prune(None, 5, nan, None, None, 0, -1, 0, C.byref(h), None) == nat.VS_EINVAL and ">= 0" in nat.last_error()
    assert L.vs_index_prune(None, 5, nan, None, None, 0, 0, 0, None, None) == nat.VS_EINVAL
    assert not h.value


# ---- the Python layer's host logic -------------------------------------------------------------------------------------------------------------------
def test_prune_args():
    t, v = di._prune_args(None, None)
    assert t == 0 and np.isnan(v)
    assert di._prune_args(np.int64(7), 0.1) == (7, float(np.float32(0.1))) and di._prune_args(65535, -np.inf) == (65535, -np.inf)
    for bad in (-1, 65536):
        with pytest.raises(ValueError, match="topk"):
            di._prune_args(bad, None)
    for bad in (1.5, True, "3"):
        with pytest.raises(TypeError, match="topk"):
            di._prune_args(bad, None)
    with pytest.raises(ValueError, match="NaN"):
        di._prune_args(3, float("nan"))
    with pytest.raises(TypeError, match="min_value"):
        di._prune_args(3, "x")


def test_col_keep_words():
    assert di._col_keep_words(70) is None
    w = di._col_keep_words(70, keep_cols=[0, 31, 32, 69])
    assert w.dtype == np.uint32 and w.tolist() == [0x80000001, 1, 1 << 5]
    w = di._col_keep_words(70, drop_cols=np.array([1, 33]))
    assert w.tolist() == [0xFFFFFFFD, 0xFFFFFFFD, 0x3F]          # bits past n_cols stay clear
    mask = np.zeros(70, dtype=bool)
    mask[[2, 3, 64]] = True
    assert di._col_keep_words(70, keep_cols=mask, drop_cols=[3]).tolist() == [4, 0, 1]
    assert di._col_keep_words(70, keep_cols=[]).tolist() == [0, 0, 0]
    for bad in ([70], [-1]):
        with pytest.raises(ValueError, match="outside"):
            di._col_keep_words(70, keep_cols=bad)
    with pytest.raises(TypeError):
        di._col_keep_words(70, drop_cols=[0.5])
    with pytest.raises(ValueError, match="shape"):
        di._col_keep_words(70, keep_cols=np.ones(71, dtype=bool))
    with pytest.raises(ValueError, match="1-D"):
        di._col_keep_words(70, keep_cols=[[1, 2]])


# ---- the host-only code under the host sanitizers ------------------------------------------------------------------------------------------------
def test_host_checks_under_a_host_sanitizer(tmp_path):
    """prune_check.h (the order key, the digit and tie-bit functions, the radix select composed of them against a sort on exact-size heap
    arrays, the plan rule, every check) in a stand-alone program built with the host compiler under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "prune_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "prune_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "prune_check: ok" in run.stdout, run.stdout + run.stderr
