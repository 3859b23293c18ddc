"""CPU checks of the combined index: the numpy reference (tests/_combine_ref.py) against independent formulations, fp16
rounding, stored and cancelled zeros, the repeated-column error, the plan rule (vs_combine_plan is pure host arithmetic), the argument errors
of the C ABI and of the Python layer without a GPU, and the host-only code (vsearch_amd/csrc/combine_check.h) run in a stand-alone program
under the host sanitizers.  No device is needed; nothing is loaded into Python under a sanitizer."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from vsearch_amd import _native as nat
from vsearch_amd import device_index as di

import _combine_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_COLS = 90


def _csr(rng, lengths, n_cols=N_COLS, order="shuffled"):
    ip = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rows = []
    for n in lengths:
        c = rng.permutation(n_cols)[:n]
        rows.append(np.sort(c) if order == "sorted" else (np.sort(c)[::-1] if order == "descending" else c))
    ix = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int64)
    return ip, ix, rng.standard_normal(int(ip[-1])).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dense(csr, n_cols=N_COLS):
    ip, ix, d = csr
    n = len(ip) - 1
    rows = np.repeat(np.arange(n), np.diff(ip))
    m = np.zeros((n, n_cols), np.float32)
    mask = np.zeros((n, n_cols), bool)
    m[rows, ix] = 1.0 if d is None else d
    mask[rows, ix] = True
    return m, mask


# ---- the reference against independent formulations ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wa,wb", [(1.0, 1.0), (1.0, -1.0), (0.3, 0.7), (0.0, 2.5), (-3.0, 1e-3)])
def test_reference_equals_the_dense_formula_on_the_union_mask(wa, wb):
    rng = np.random.default_rng(1)
    lengths = [0, 1, 7, 8, 9, 40, 90, 0, 3]
    a, b = _csr(rng, lengths, order="descending"), _csr(rng, lengths[::-1])
    for binary_b in (False, True):
        bb = (b[0], b[1], None) if binary_b else b
        ip, ix, v = ref.combine_ref(a, bb, wa, wb)
        A, ma = _dense(a)
        B, mb = _dense(bb)
        xa, xb = np.float64(np.float32(wa)) * A.astype(np.float64), np.float64(np.float32(wb)) * B.astype(np.float64)
        # a column one side lacks takes the one product, not product + 0: 0 * -x stays -0
        want = np.float32(np.where(ma & mb, xa + xb, np.where(ma, xa, xb)))
        union = ma | mb
        assert np.array_equal(np.diff(ip), union.sum(1))
        rows = np.repeat(np.arange(len(lengths)), np.diff(ip))
        assert np.array_equal(np.stack([rows, ix], 1), np.argwhere(union))            # each union column once, ascending
        assert np.array_equal(_bits(v), _bits(want[union]))


def test_reference_equals_a_scipy_sum():
    sp = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(2)
    lengths = rng.integers(0, 30, size=50)
    a, b = _csr(rng, lengths, order="sorted"), _csr(rng, rng.permutation(lengths), order="sorted")
    # dyadic values and weights: every product and sum is exact, so the float64 sum scipy takes equals the reference's whatever its order
    a = (a[0], a[1], (rng.integers(-64, 65, size=len(a[2])) / 8.0).astype(np.float32))
    b = (b[0], b[1], (rng.integers(1, 65, size=len(b[2])) / 16.0).astype(np.float32))
    ip, ix, v = ref.combine_ref(a, b, 0.5, -0.25)
    A = sp.csr_matrix((a[2].astype(np.float64), a[1], a[0]), shape=(50, N_COLS))
    B = sp.csr_matrix((b[2].astype(np.float64), b[1], b[0]), shape=(50, N_COLS))
    S = (0.5 * A - 0.25 * B).toarray()
    mine = np.zeros((50, N_COLS))
    mine[np.repeat(np.arange(50), np.diff(ip)), ix] = v
    assert np.array_equal(mine, S)


# ---- fp16 rounding --------------------------------------------------------------------------------------------------------------------------------
def test_fp16_halfway_and_double_rounding_cases():
    one = (np.array([0, 10]), np.arange(10))
    d = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65519.0, 65520.0, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, -(2.0 ** -25), 2.0 ** -14 - 2.0 ** -25, 0.1],
                 np.float32)
    empty = (np.array([0, 0]), np.zeros(0, np.int64), np.zeros(0, np.float32))
    got = ref.combine_ref((*one, d), empty, 1.0, 1.0, "fp16")[2]
    want = np.array([1.0, 1 + 2.0 ** -9, 65504.0, np.inf, 2.0 ** -24, 0.0, 2.0 ** -24, -0.0, 2.0 ** -14, np.float32(np.float16(0.1))], np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    # two roundings: (1 + 2^-11) + 2^-40 is above the fp16 tie, float32 takes it onto the tie, and the tie goes to the even 1.0 -- one
    # rounding of the exact sum would give 1 + 2^-10
    cell = lambda v: (np.array([0, 1]), np.array([4]), np.array([v], np.float32))
    assert ref.combine_ref(cell(1 + 2.0 ** -11), cell(2.0 ** -40), 1.0, 1.0, "fp16")[2][0] == 1.0
    assert np.float16(np.float64(1 + 2.0 ** -11) + 2.0 ** -40) == np.float16(1 + 2.0 ** -10)
    # ... and a sum float32 keeps above the tie rounds up
    assert ref.combine_ref(cell(1 + 2.0 ** -11), cell(2.0 ** -20), 1.0, 1.0, "fp16")[2][0] == 1 + 2.0 ** -10
    # the float32 rounding itself: 1 + 2^-24 is a float32 tie, to even
    assert ref.combine_ref(cell(1.0), cell(2.0 ** -24), 1.0, 1.0)[2][0] == 1.0
    assert ref.combine_ref(cell(1.0), cell(2.0 ** -24), 1.0, 3.0)[2][0] == np.float32(1 + 2.0 ** -22)
    # weights scale before the sum: 0.3 is the float32 0.3
    x = ref.combine_ref(cell(3.0), cell(7.0), 1.0, 0.3)[2][0]
    assert x == np.float32(3.0 + np.float64(np.float32(0.3)) * 7.0)


# ---- stored and cancelled zeros ---------------------------------------------------------------------------------------------------------------------
def test_stored_zeros_and_cancelling_pairs_stay_cells():
    a = (np.array([0, 3, 3]), np.array([5, 2, 9]), np.array([0.0, 1.5, -2.0], np.float32))          # column 5 holds a stored zero
    b = (np.array([0, 2, 3]), np.array([9, 7, 1]), np.array([2.0, -0.0, 4.0], np.float32))          # 9 cancels; 7 holds a stored -0
    ip, ix, v = ref.combine_ref(a, b, 1.0, 1.0)
    assert ip.tolist() == [0, 4, 5] and ix.tolist() == [2, 5, 7, 9, 1]
    assert _bits(v).tolist() == _bits(np.array([1.5, 0.0, -0.0, 0.0, 4.0], np.float32)).tolist()   # -2 + 2 = +0; the lone -0 stays -0
    ip, ix, v = ref.combine_ref(a, a, 1.0, -1.0)                                                   # a - a: every cell stays, at +0
    assert ip.tolist() == [0, 3, 3] and ix.tolist() == [2, 5, 9] and _bits(v).tolist() == [0, 0, 0]
    ip, ix, v = ref.combine_ref(a, b, 0.0, 0.0)                                                    # zero weights keep the sparsity
    assert ip.tolist() == [0, 4, 5] and _bits(v).tolist() == _bits(np.array([0.0, 0.0, -0.0, 0.0, 0.0], np.float32)).tolist()
    ip, ix, v = ref.combine_ref(a, (b[0], b[1], None), np.inf, np.nan)                            # weights are data
    assert np.isnan(v[[1, 2, 3, 4]]).all() and v[0] == np.inf                                      # inf * 0 (column 5), NaN * 1


# ---- repeated columns ---------------------------------------------------------------------------------------------------------------------------------
def test_repeated_column_names_the_source_and_the_lowest_row():
    ok = (np.array([0, 2, 4, 6]), np.array([1, 2, 3, 4, 5, 6]), np.ones(6, np.float32))
    rep2 = (np.array([0, 2, 4, 6]), np.array([1, 2, 3, 4, 6, 6]), np.ones(6, np.float32))
    rep1 = (np.array([0, 2, 4, 6]), np.array([1, 2, 3, 3, 5, 5]), np.ones(6, np.float32))
    for a, b, source, row in ((rep2, ok, "a", 2), (ok, rep2, "b", 2), (rep2, rep1, "b", 1), (rep1, rep2, "a", 1), (rep1, rep1, "a", 1)):
        with pytest.raises(ref.RepeatedColumn) as e:
            ref.combine_ref(a, b)
        assert (e.value.source, e.value.row) == (source, row)
    assert ref.combine_ref(ok, ok)[1].tolist() == [1, 2, 3, 4, 5, 6]                               # the same column in a and in b is no repeat


# ---- the plan rule and the C ABI without a device -------------------------------------------------------------------------------------------------------
def test_plan_is_pure_host_arithmetic():
    F32, F16, BIN = nat.VS_F32, nat.VS_F16, nat.VS_NONE
    p = di.combine_plan(10, 10, 10, 300, F16, F16, F16)
    assert p == (2048, 32768, 4 * (3 * 10 + 2048) * 4, (3 * 10 + 304) * 4 + 128, 40 + 4 + 16 + 64)
    n = 21015324
    p = di.combine_plan(n, n * 96, n * 11, 29523, F32, BIN, F32)
    words, blocks, long_cap = 923, (n + 4095) // 4096, n * 107 // 256 + 1
    assert p.wave_lds_bytes == 4 * (3 * words + 2048) * 4 and p.group_lds_bytes == (3 * words + 29528) * 4 + 128
    assert p.scratch_bytes == 4 * n + 4 * long_cap + 8 * (blocks + 1) + 64
    p = di.combine_plan(10, 10, 10, 65535, BIN, F32, F16)
    assert p.wave_lds_bytes == 4 * (3 * 2048 + 2048) * 4 <= 160 * 1024 and p.group_lds_bytes == (3 * 2048 + 32768) * 4 + 128 <= 160 * 1024
    assert p.wave_cells == 2048 and p.group_cells == 32768
    assert di.combine_plan(0, 0, 0, 300, F32, F32, F32).scratch_bytes == 16 + 64
    assert nat.lib().vs_combine_plan(5, 5, 5, 5, F32, F32, F32, None, None, None, None, None) == nat.VS_OK      # any output may be NULL
    with pytest.raises(NotImplementedError, match="uint16"):
        di.combine_plan(1, 1, 1, 65536, F32, F32, F32)
    for bad, needle in (((1, 1, 1, 0, F32, F32, F32), "n_cols"), ((-1, 1, 1, 5, F32, F32, F32), "n_rows"), ((1, -1, 1, 5, F32, F32, F32), "n_packets"),
                        ((1, 1, 1 << 32, 5, F32, F32, F32), "n_packets"), ((1, 1, 1, 5, nat.VS_I32, F32, F32), "source store_dtype"),
                        ((1, 1, 1, 5, F32, nat.VS_U8, F32), "source store_dtype"), ((1, 1, 1, 5, F32, F32, BIN), "binarising"),
                        ((1, 1, 1, 5, F32, F32, nat.VS_I64), "out_dtype")):
        with pytest.raises(ValueError, match=needle):
            di.combine_plan(*bad)


def test_c_abi_argument_errors_without_a_handle():
    L = nat.lib()
    h = C.c_void_p()
    fake = C.c_void_p(1)                                                        # never dereferenced: every check below comes before a handle is read
    one = C.c_float(1.0)
    assert L.vs_index_combine(None, fake, one, one, nat.VS_F32, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert L.vs_index_combine(fake, None, one, one, nat.VS_F32, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert L.vs_index_combine(fake, fake, one, one, nat.VS_F32, 0, 0, 0, None) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert L.vs_index_combine(fake, fake, one, one, nat.VS_NONE, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "binarising" in nat.last_error()
    assert L.vs_index_combine(fake, fake, one, one, nat.VS_I32, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "out_dtype" in nat.last_error()
    assert L.vs_index_combine(fake, fake, one, one, nat.VS_F32, -1, 0, 0, C.byref(h)) == nat.VS_EINVAL and ">= 0" in nat.last_error()
    assert L.vs_index_combine(fake, fake, one, one, nat.VS_F16, 0, -1, 0, C.byref(h)) == nat.VS_EINVAL and ">= 0" in nat.last_error()
    assert not h.value


def test_python_layer_argument_errors():
    F32, F16, BIN = nat.VS_F32, nat.VS_F16, nat.VS_NONE
    assert di._combine_dtype(None, F16, F16) == F16                               # fp32, unless both sources are fp16
    for sa, sb in ((F32, F32), (F32, F16), (F16, BIN), (BIN, BIN), (BIN, F32)):
        assert di._combine_dtype(None, sa, sb) == F32
    assert di._combine_dtype("fp16", F32, BIN) == F16 and di._combine_dtype(np.float32, F16, F16) == F32
    for bad in ("int8", "binary", True, BIN):
        with pytest.raises(ValueError, match="dtype must be"):
            di._combine_dtype(bad, F32, F32)
    assert di._combine_weight(0.3, "wa") == float(np.float32(0.3)) and di._combine_weight(2, "wa") == 2.0
    assert np.isnan(di._combine_weight(float("nan"), "wb")) and di._combine_weight(np.float64(1e300), "wb") == np.inf
    for bad in ("1", None, True, [1.0]):
        with pytest.raises(TypeError, match="must be a number"):
            di._combine_weight(bad, "wb")


# ---- the host-only code under the host sanitizers ------------------------------------------------------------------------------------------------
def test_host_checks_under_a_host_sanitizer(tmp_path):
    """combine_check.h (every argument rule, the plan at n_cols = 1, 300, 29 523 and 65 535, the flags of the count step, the capacity rule,
    the grids) in a stand-alone program built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "combine_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "combine_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "combine_check: ok" in run.stdout, run.stdout + run.stderr
