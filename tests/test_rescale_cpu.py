"""CPU checks of the reweighted index: the numpy reference (tests/_rescale_ref.py) against independent formulations, the plan
rule (vs_rescale_plan is pure host arithmetic), the argument errors of the C ABI and of the Python layer without a GPU, and the host-only code
(vsearch_amd/csrc/rescale_check.h) run in a stand-alone program under the host sanitizers.  No device is needed; nothing is loaded into Python
under a sanitizer."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from vsearch_amd import _native as nat
from vsearch_amd import device_index as di

import _rescale_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _csr(rng, lengths, n_cols=700, values=None):
    ip = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ix = np.concatenate([np.sort(rng.permutation(n_cols)[:n]) for n in lengths] + [np.zeros(0, np.int64)]).astype(np.int64)
    d = rng.standard_normal(int(ip[-1])) if values is None else values(int(ip[-1]))
    return ip, ix, d.astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the stats reference against independent formulations ---------------------------------------------------------------------------------------
def test_stats_on_dyadic_values_equal_reduceat():
    """values k / 8 with |k| <= 64: every partial sum of up to 600 of them and of their squares is exact in float64, so any order gives the
    same bits -- the lane / butterfly loop has to equal np.add.reduceat"""
    rng = np.random.default_rng(1)
    lengths = [1, 7, 8, 9, 504, 511, 512, 513, 520, 600, 3]
    ip, ix, d = _csr(rng, lengths, values=lambda n: rng.integers(-64, 65, size=n) / 8.0)
    cells, nonzero, l1, sumsq, mx = ref.row_stats_ref(ip, d)
    x = d.astype(np.float64)
    assert np.array_equal(cells, np.diff(ip)) and cells.dtype == np.int32
    assert np.array_equal(nonzero, np.add.reduceat((d != 0).astype(np.int32), ip[:-1]))
    assert np.array_equal(l1.view(np.uint64), np.add.reduceat(np.abs(x), ip[:-1]).view(np.uint64))
    assert np.array_equal(sumsq.view(np.uint64), np.add.reduceat(x * x, ip[:-1]).view(np.uint64))
    assert np.array_equal(_bits(mx), _bits(np.maximum.reduceat(d, ip[:-1]) + np.float32(0.0)))


def test_stats_edge_rows():
    nan = np.float32(np.nan)
    ip = np.array([0, 0, 2, 4, 5, 8, 8])
    d = np.array([-0.0, 0.0, nan, nan, -0.0, nan, -3.0, -7.0], np.float32)
    cells, nonzero, l1, sumsq, mx = ref.row_stats_ref(ip, d)
    assert cells.tolist() == [0, 2, 2, 1, 3, 0] and nonzero.tolist() == [0, 0, 2, 0, 3, 0]
    assert _bits(mx).tolist() == [0x7FC00000, 0, 0x7FC00000, 0, _bits(np.float32(-3.0))[0], 0x7FC00000]      # empty, +0.0 of the zeros, all NaN, -0.0 alone
    assert l1[0] == 0 and not np.signbit(l1[0]) and sumsq[5] == 0 and np.isnan(l1[2]) and np.isnan(sumsq[4]) and l1[1] == 0 and l1[3] == 0
    b = ref.row_stats_ref(np.array([0, 3, 3]), None)                              # a binary index: 1 everywhere
    assert b[0].tolist() == [3, 0] and b[1].tolist() == [3, 0] and b[2].tolist() == [3.0, 0.0] and b[3].tolist() == [3.0, 0.0]
    assert b[4][0] == 1.0 and np.isnan(b[4][1])


def test_stats_order_matters_and_is_the_pinned_one():
    """2^54 in lane 0 and a 1 in each of lanes 1 .. 7 (the ulp of 2^54 is 4): the butterfly adds the ones to each other first -- 2^54 + 1 and
    2^54 + 2 round back to 2^54 on the way, the last step adds 4 exactly -- while a left-to-right sum loses every one of them"""
    d = np.zeros(65 * 8, np.float32)
    d[0] = 2.0 ** 27
    d[8:64:8] = 1.0                                                               # the first cell of packets 1 .. 7
    ip = np.array([0, d.size])
    _, _, l1, sumsq, _ = ref.row_stats_ref(ip, d)
    assert sumsq[0] == 2.0 ** 54 + 4.0 and l1[0] == 2.0 ** 27 + 7.0
    seq = np.float64(0.0)
    for x in d.astype(np.float64):
        seq = seq + x * x
    assert seq == 2.0 ** 54
    # lane 0 holds packets 0 and 64 and adds them cell by cell before the butterfly: 2^54 + 4 is exact there
    d2 = np.zeros(65 * 8, np.float32)
    d2[0], d2[64 * 8] = 2.0 ** 27, 2.0
    d2[8:32:8] = 1.0                                                              # lanes 1 .. 3: (2^54 + 4) + 1 -> 2^54 + 4, then + 2 -> the tie goes to even: 2^54 + 8
    assert ref.row_stats_ref(ip, d2)[3][0] == 2.0 ** 54 + 8.0


# ---- the rescale reference against independent formulations ------------------------------------------------------------------------------------------
def test_one_scale_is_the_float32_product():
    rng = np.random.default_rng(3)
    ip, ix, d = _csr(rng, [0, 5, 40, 0, 9])
    d[:4] = [np.float32(1e-39), np.float32(-1e-20), np.float32(3e38), np.float32(-0.0)]
    rs = (rng.standard_normal(5) * 1e3).astype(np.float32)
    cs = np.exp(rng.standard_normal(700) * 20).astype(np.float32)
    rows = np.repeat(np.arange(5), np.diff(ip))
    with np.errstate(all="ignore"):
        assert np.array_equal(_bits(ref.rescale_ref(ip, ix, d, row_scale=rs)), _bits(d * rs[rows]))
        assert np.array_equal(_bits(ref.rescale_ref(ip, ix, d, col_scale=cs)), _bits(d * cs[ix]))
    assert np.array_equal(_bits(ref.rescale_ref(ip, ix, d)), _bits(d))
    assert np.array_equal(_bits(ref.rescale_ref(ip, ix, None, col_scale=cs)), _bits(cs[ix]))       # a binary source: the scale itself
    both = ref.rescale_ref(ip, ix, d, row_scale=rs, col_scale=cs)
    with np.errstate(all="ignore"):
        want = (d.astype(np.float64) * rs[rows].astype(np.float64) * cs[ix].astype(np.float64)).astype(np.float32)
    assert ref.same_values(both, want)


def test_fp16_halfway_cases():
    ip, ix = np.array([0, 10]), np.arange(10)
    d = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65519.0, 65520.0, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, -(2.0 ** -25), 2.0 ** -14 - 2.0 ** -25, 0.1],
                 np.float32)
    got = ref.rescale_ref(ip, ix, d, out="fp16")
    want = np.array([1.0, 1 + 2.0 ** -9, 65504.0, np.inf, 2.0 ** -24, 0.0, 2.0 ** -24, -0.0, 2.0 ** -14, np.float32(np.float16(0.1))], np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    # the two roundings are taken one after the other: 1 + 2^-11 + 2^-40 rounds to 1 + 2^-11 in float32 first, then ties to even
    x = ref.rescale_ref(np.array([0, 1]), np.array([0]), np.array([1 + 2.0 ** -11], np.float32), row_scale=[np.float32(1 + 2.0 ** -23)], out="fp16")
    assert x[0] == 1.0 + 2.0 ** -10                                               # (here the float32 value is above the tie)
    y = ref.rescale_ref(np.array([0, 1]), np.array([0]), np.array([2.0 ** -12], np.float32), row_scale=[np.float32(0.5 + 2.0 ** -24)], col_scale=[1.0], out="fp16")
    assert y[0] == np.float32(np.float16(np.float32(2.0 ** -13 + 2.0 ** -36)))


# ---- the plan rule and the C ABI without a device ---------------------------------------------------------------------------------------------------------
def test_plan_is_pure_host_arithmetic():
    F32, F16, BIN = nat.VS_F32, nat.VS_F16, nat.VS_NONE
    assert di.rescale_plan(10, 10, 1, F32, F32, False, True) == (4, 16, "lds")
    assert di.rescale_plan(10, 10, 300, F32, F16, True, True) == (40 + 1200, 1200, "lds")
    assert di.rescale_plan(21015324, 21015324 * 96, 29523, F32, F32, True, True) == (4 * 21015324 + 4 * 29523, 118096, "lds")
    limit = 160 * 1024 // 4                                                       # the image fills a CU's LDS
    assert di.rescale_plan(10, 10, limit, F16, F32, False, True) == (4 * limit, 160 * 1024, "lds")
    assert di.rescale_plan(10, 10, limit + 1, F16, F32, False, True) == (4 * (limit + 1), 0, "memory")
    assert di.rescale_plan(10, 10, 65535, BIN, F32, False, True) == (4 * 65535, 0, "memory")
    assert di.rescale_plan(10, 0, 65535, F32, F32, True, False) == (40, 0, "none")
    assert di.rescale_plan(0, 0, 300, F32, F32) == (0, 0, "none")
    assert nat.lib().vs_rescale_plan(5, 5, 5, F32, F32, 1, 1, None, None, None) == nat.VS_OK          # any output may be NULL
    with pytest.raises(NotImplementedError, match="uint16"):
        di.rescale_plan(1, 1, 65536, F32, F32)
    for bad, needle in (((1, 1, 0, F32, F32), "n_cols"), ((-1, 1, 5, F32, F32), "n_rows"), ((1, -1, 5, F32, F32), "n_packets"),
                        ((1, 1, 5, nat.VS_I32, F32), "source store_dtype"), ((1, 1, 5, F32, BIN), "binarising"), ((1, 1, 5, F32, nat.VS_I64), "out_dtype")):
        with pytest.raises(ValueError, match=needle):
            di.rescale_plan(*bad)


def test_c_abi_argument_errors_without_a_handle():
    L = nat.lib()
    h = C.c_void_p()
    fake = C.c_void_p(1)                                                        # never dereferenced: every check below comes before the handle is read
    assert L.vs_index_rescale(None, None, None, nat.VS_F32, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert L.vs_index_rescale(fake, None, None, nat.VS_F32, 0, 0, 0, None) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert L.vs_index_rescale(fake, None, None, nat.VS_NONE, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "binarising" in nat.last_error()
    assert L.vs_index_rescale(fake, None, None, nat.VS_I32, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "out_dtype" in nat.last_error()
    assert L.vs_index_rescale(fake, None, None, nat.VS_F32, -1, 0, 0, C.byref(h)) == nat.VS_EINVAL and ">= 0" in nat.last_error()
    assert L.vs_index_rescale(fake, None, None, nat.VS_F16, 0, -1, 0, C.byref(h)) == nat.VS_EINVAL and ">= 0" in nat.last_error()
    assert not h.value
    assert L.vs_index_row_stats(None, None, None, None, None, None) == nat.VS_EINVAL and "NULL" in nat.last_error()


def test_python_layer_argument_errors():
    for good, want in (("fp32", nat.VS_F32), ("fp16", nat.VS_F16), ("float16", nat.VS_F16), (np.float32, nat.VS_F32), (np.dtype("float16"), nat.VS_F16),
                       (nat.VS_F16, nat.VS_F16)):
        assert di._rescale_dtype(good, nat.VS_NONE) == want
    assert di._rescale_dtype(None, nat.VS_F16) == nat.VS_F16 and di._rescale_dtype(None, nat.VS_F32) == nat.VS_F32
    with pytest.raises(ValueError, match="binary index has no value dtype"):
        di._rescale_dtype(None, nat.VS_NONE)
    for bad in ("int8", "binary", True, nat.VS_NONE, np.int32):
        with pytest.raises(ValueError, match="dtype must be"):
            di._rescale_dtype(bad, nat.VS_F32)
    a, p = di._scale_arg([1, 2.5, -3], 3, "row_scale", 0)
    assert a.dtype == np.float32 and a.tolist() == [1.0, 2.5, -3.0] and p.value == a.ctypes.data
    assert di._scale_arg(None, 3, "row_scale", 0) == (None, None)
    with pytest.raises(ValueError, match=r"row_scale must have shape \(3,\)"):
        di._scale_arg(np.ones(4), 3, "row_scale", 0)
    with pytest.raises(ValueError, match="col_scale must have shape"):
        di._scale_arg(np.ones((3, 1)), 3, "col_scale", 0)
    with pytest.raises(TypeError, match="numbers"):
        di._scale_arg(np.array(["a", "b"]), 2, "col_scale", 0)
    with pytest.raises(TypeError, match="numbers"):
        di._scale_arg(np.array([True, False]), 2, "col_scale", 0)


# ---- the host-only code under the host sanitizers ------------------------------------------------------------------------------------------------
def test_host_checks_under_a_host_sanitizer(tmp_path):
    """rescale_check.h (every argument rule, the plan at n_cols = 1, 300, 29 523, the LDS-image limit and one past it, and 65 535, a packet
    count of 0, the capacity rule, the grids) in a stand-alone program built with the host compiler under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "rescale_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "rescale_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "rescale_check: ok" in run.stdout, run.stdout + run.stderr
