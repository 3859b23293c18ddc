"""CPU checks of the joined index: the numpy reference (tests/_concat_ref.py) against scipy's vstack and its fp32 -> fp16
rounding against numpy's, the plan rule (vs_concat_plan), the argument errors of the C ABI and of the Python layers without a GPU, the facade's
field rules, and the host-only code (vsearch_amd/csrc/concat_check.h) run in a stand-alone program under the host sanitizers.  No device is
needed; nothing is loaded into Python under a sanitizer."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from vsearch_amd import _native as nat
from vsearch_amd import device_index as di

import _concat_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, NONE = nat.VS_F32, nat.VS_F16, nat.VS_NONE


def _csr(rng, lengths, n_cols=50):
    ip = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ix = np.concatenate([np.sort(rng.permutation(n_cols)[:n]) for n in lengths] + [np.zeros(0, np.int64)]).astype(np.int64)
    return ip, ix, rng.standard_normal(int(ip[-1])).astype(np.float32)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------------
def test_reference_equals_scipy_vstack_for_same_dtype_sources():
    sp = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(1)
    parts = [_csr(rng, l) for l in ([0, 3, 9, 0], [8], [0], [1, 0, 40, 7])]
    want = sp.vstack([sp.csr_matrix((d, ix, ip), shape=(len(ip) - 1, 50)) for ip, ix, d in parts]).tocsr()
    got = ref.concat_ref(parts, "fp32")
    assert np.array_equal(got[0], want.indptr) and np.array_equal(got[1], want.indices)
    assert np.array_equal(got[2].view(np.uint32), want.data.astype(np.float32).view(np.uint32))
    halves = [(ip, ix, d.astype(np.float16).astype(np.float32)) for ip, ix, d in parts]         # fp16 sources, widened as export_csr does
    got16 = ref.concat_ref(halves, "fp16")
    assert np.array_equal(got16[0], want.indptr) and np.array_equal(got16[2].view(np.uint32), np.concatenate([h[2] for h in halves]).view(np.uint32))
    binary = ref.concat_ref([(ip, ix, None) for ip, ix, _ in parts], "binary")
    assert binary[2] is None and np.array_equal(binary[0], want.indptr) and np.array_equal(binary[1], want.indices)
    assert ref.packets_of(got[0]) == sum(ref.packets_of(p[0]) for p in parts)
    pk = ref.rebased_packet_pointers([p[0] for p in parts])
    assert pk.tolist() == [0, 0, 1, 3, 3, 4, 4, 5, 5, 10, 11]                                   # R_s + r -> src_pk_s[r] + P_s; the last is the total


def test_reference_mixed_stores_and_empty_sources():
    rng = np.random.default_rng(2)
    a, b, c = _csr(rng, [2, 0]), _csr(rng, [3]), _csr(rng, [1, 1])
    empty = (np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32))
    got = ref.concat_ref([empty, a, empty, (b[0], b[1], None), c, empty], "fp16")
    assert got[0].tolist() == [0, 2, 2, 5, 6, 7]
    assert np.array_equal(got[2][2:5], np.ones(3, np.float32))                                  # a binary cell is 1
    assert np.array_equal(got[2][:2].view(np.uint32), a[2].astype(np.float16).astype(np.float32).view(np.uint32))
    assert ref.default_store(["binary", "binary"]) == "binary" and ref.default_store(["binary", "fp16"]) == "fp16"
    assert ref.default_store(["fp16", "fp32", "binary"]) == "fp32"
    with pytest.raises(ValueError, match="binarising"):
        ref.concat_ref([a, (b[0], b[1], None)], "binary")
    with pytest.raises(ValueError, match="empty join"):
        ref.concat_ref([empty, empty], "fp32")
    assert ref.concat_live([[True, False], [], [False]]).tolist() == [True, False, False]


def test_fp16_rounding_equals_numpy_at_ties_subnormals_overflow_and_nan():
    u = np.float32(2.0 ** -11)
    special = np.array([1.0 + u, 1.0 + 3 * u, 1.0 + u * (1 + 2.0 ** -12), 1.0 + u * (1 - 2.0 ** -12), -(1.0 + u), -(1.0 + 3 * u),       # ties, and just off them
                        2047.0 + 0.5, 2048.0 + 1.0, 2048.0 + 3.0,
                        2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -26, -(2.0 ** -25), 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25,   # subnormals
                        2.0 ** -14 - 2.0 ** -26, 1e-45, -1e-45, 1e-38, 0.0, -0.0,
                        65504.0, 65519.0, 65519.996, 65520.0, 65536.0, 1e30, -65520.0, -65519.996, np.inf, -np.inf], dtype=np.float32)      # overflow
    with np.errstate(over="ignore"):
        want = special.astype(np.float16)
    assert np.array_equal(ref.f16_bits(special), want.view(np.uint16))
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF], dtype=np.uint32).view(np.float32)
    got = ref.f16_bits(nans).view(np.float16)
    assert np.isnan(got).all() and np.isnan(nans.astype(np.float16)).all()
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 1 << 32, size=200_000, dtype=np.uint64).astype(np.uint32)            # every exponent, both signs
    x = bits.view(np.float32)
    x = x[~np.isnan(x)]
    with np.errstate(over="ignore"):
        assert np.array_equal(ref.f16_bits(x), x.astype(np.float16).view(np.uint16))
    near = (rng.integers(0, 0x7C00, size=50_000).astype(np.uint16).view(np.float16).astype(np.float32).view(np.uint32) + 0x1000).view(np.float32)   # exact ties
    with np.errstate(over="ignore"):
        assert np.array_equal(ref.f16_bits(near), near.astype(np.float16).view(np.uint16))
    assert ref.same_bits(ref.to_f16(np.float32([1.0 + u, np.nan])), np.float32([1.0, np.nan]))


# ---- the plan rule and the C ABI without a device ---------------------------------------------------------------------------------------------------------
def test_plan_is_pure_host_arithmetic():
    p = di.concat_plan([5], [7], 100, [F32], F32)
    assert p == di.ConcatPlan(5, 7, 48 + 16, 6152)
    p = di.concat_plan([3, 0, 9], [4, 0, 0], 100, [F32, F16, NONE], F16)
    assert (p.rows, p.packets, p.scratch_bytes) == (12, 4, 3 * 48 + 16)
    p = di.concat_plan([1000] * 256, [12000] * 256, 29523, [F16] * 256, F16)
    assert (p.rows, p.packets, p.scratch_bytes, p.lds_bytes) == (256000, 3072000, 256 * 48 + 16, 6152)
    assert di.concat_plan([3, 2], [4, 1], 100, [NONE, NONE], NONE).rows == 5                    # all binary: a binary result is allowed
    assert di.concat_plan([0x7FFFFFFF, 0x7FFFFFFF], [1, 1], 10, [F32, F32], F32).rows == (1 << 32) - 2
    L = nat.lib()
    one, dt = np.array([4], dtype=np.int64), np.array([F32], dtype=np.int32)
    assert L.vs_concat_plan(1, C.c_void_p(one.ctypes.data), C.c_void_p(one.ctypes.data), 10, C.c_void_p(dt.ctypes.data), F32, None, None, None, None) == nat.VS_OK
    for args, exc, needle in ((([3, 2], [4, 1], 100, [NONE, F16], NONE), ValueError, "binarising is not covered"),
                              (([3], [4], 100, [F32], 7), ValueError, "out_dtype must be"),
                              (([3, 2], [4, 1], 100, [F32, 5], F32), ValueError, "source 1: bad store_dtype"),
                              (([0, 0], [0, 0], 100, [F32, F32], F32), ValueError, "empty join"),
                              (([3, -1], [4, 1], 100, [F32, F32], F32), ValueError, "source 1: n_rows"),
                              (([3, 1], [-4, 1], 100, [F32, F32], F32), ValueError, "source 0: n_packets"),
                              (([3], [4], 0, [F32], F32), ValueError, "n_cols must be positive"),
                              (([3], [4], 65536, [F32], F32), NotImplementedError, "uint16"),
                              (([], [], 10, [], F32), ValueError, "n_src must be in 1..256"),
                              (([1] * 257, [1] * 257, 10, [F32] * 257, F32), ValueError, "n_src must be in 1..256"),
                              (([0x7FFFFFFF, 0x80000000], [1, 1], 10, [F32, F32], F32), NotImplementedError, "2\\^32"),      # 2^32 - 1 rows
                              (([5, 5], [0x80000000, 0x80000000], 10, [F32, F32], F32), NotImplementedError, "2\\^32")):    # 2^32 packets
        with pytest.raises(exc, match=needle):
            di.concat_plan(*args)
    with pytest.raises(ValueError, match="one entry a source"):
        di.concat_plan([1, 2], [1], 10, [F32, F32], F32)
    assert L.vs_concat_plan(1, None, C.c_void_p(one.ctypes.data), 10, C.c_void_p(dt.ctypes.data), F32, None, None, None, None) == nat.VS_EINVAL
    assert "NULL" in nat.last_error()


def test_c_abi_argument_errors_without_a_handle():
    L = nat.lib()
    h = C.c_void_p()
    fake = (C.c_void_p * 2)(1, 1)                                               # never dereferenced: every check below comes before a handle is read
    holes = (C.c_void_p * 2)(1, None)
    assert L.vs_index_concat(None, 2, F32, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert L.vs_index_concat(fake, 2, F32, 0, 0, 0, None) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert L.vs_index_concat(fake, 0, F32, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "n_src must be in 1..256" in nat.last_error()
    assert L.vs_index_concat(fake, 257, F32, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "n_src must be" in nat.last_error()
    assert L.vs_index_concat(fake, -1, F32, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "n_src must be" in nat.last_error()
    assert L.vs_index_concat(fake, 2, F32, -1, 0, 0, C.byref(h)) == nat.VS_EINVAL and ">= 0" in nat.last_error()
    assert L.vs_index_concat(fake, 2, F32, 0, -1, 0, C.byref(h)) == nat.VS_EINVAL and ">= 0" in nat.last_error()
    holes_first = (C.c_void_p * 2)(None, None)
    assert L.vs_index_concat(holes_first, 2, F32, 0, 0, 0, C.byref(h)) == nat.VS_EINVAL and "NULL argument: source 0" in nat.last_error()
    del holes
    assert not h.value


def test_python_layer_argument_errors():
    """what concat() refuses, and what it picks, before the library is reached"""
    assert di._concat_dtype(None, [NONE, NONE]) == NONE and di._concat_dtype(None, [NONE, F16]) == F16
    assert di._concat_dtype(None, [F16, F32, NONE]) == F32 and di._concat_dtype(None, [F32]) == F32 and di._concat_dtype(None, [F16, F16]) == F16
    assert di._concat_dtype("fp16", [F32, NONE]) == F16 and di._concat_dtype(np.float32, [F16]) == F32 and di._concat_dtype(torch.float16, [F32]) == F16
    assert di._concat_dtype("binary", [NONE]) == NONE and di._concat_dtype(NONE, [NONE, NONE]) == NONE
    with pytest.raises(ValueError, match="binarising"):
        di._concat_dtype("binary", [NONE, F32])
    for bad in ("int8", True, 3.5):
        with pytest.raises(ValueError):
            di._concat_dtype(bad, [F32])
    a = object.__new__(di.DeviceIndex)                                          # no handle: nothing below may reach it
    assert di._concat_sources(a, a, di.DeviceIndex) == [a, a] and di._concat_sources(a, [], di.DeviceIndex) == [a]
    assert len(di._concat_sources(a, [a] * 255, di.DeviceIndex)) == 256
    with pytest.raises(ValueError, match="at most 256"):
        di._concat_sources(a, [a] * 256, di.DeviceIndex)
    for bad in ([a, 3], ["x"], [None]):
        with pytest.raises(TypeError):
            di._concat_sources(a, bad, di.DeviceIndex)
    for bad in (dict(rows_extra=-1), dict(packets_extra=-1)):
        with pytest.raises(ValueError, match=">= 0"):
            a.concat([a], **bad)


# ---- the facade's rules, raised before any device work -------------------------------------------------------------------------------------------------------
def _bare(cls, n, groups=False, facets=None, values=None):
    idx = cls.__new__(cls)                                                      # no device index: nothing below may reach for one
    idx._group = None
    idx._groups = torch.zeros(n, dtype=torch.int32) if groups else None
    idx._facets = {k: (torch.zeros(n, dtype=torch.int32), nl, names) for k, (nl, names) in (facets or {}).items()} or None
    idx._values = {k: torch.zeros(n, dtype=dt) for k, dt in (values or {}).items()} or None
    return idx


def test_facade_field_rules():
    from vsearch_amd.ir import BoTIndex, Index, SparseIndex
    rules = Index._concat_fields
    a = _bare(SparseIndex, 3, True, {"lang": (3, ["x", "y", "z"]), "topic": (4, None)}, {"year": torch.float32, "pages": torch.int32})
    b = _bare(BoTIndex, 2, True, {"topic": (9, None), "lang": (3, ["x", "y", "z"])}, {"pages": torch.int32, "year": torch.float32})
    grouped, facets, values = rules([a, b, a])
    assert grouped and facets == {"lang": (3, ["x", "y", "z"]), "topic": (9, None)} and values == ["year", "pages"]
    assert rules([_bare(SparseIndex, 1), _bare(SparseIndex, 1)]) == (False, {}, [])
    with pytest.raises(ValueError, match="groups: source 1 has no groups"):
        rules([a, _bare(SparseIndex, 2, False, {"lang": (3, ["x", "y", "z"]), "topic": (4, None)}, {"year": torch.float32, "pages": torch.int32})])
    with pytest.raises(ValueError, match="facet field 'topic' is missing in source 1"):
        rules([a, _bare(SparseIndex, 2, True, {"lang": (3, ["x", "y", "z"])}, {"year": torch.float32, "pages": torch.int32})])
    with pytest.raises(ValueError, match="facet field 'extra' is missing in source 0"):
        rules([a, _bare(SparseIndex, 2, True, {"lang": (3, ["x", "y", "z"]), "topic": (4, None), "extra": (1, None)}, {"year": torch.float32, "pages": torch.int32})])
    with pytest.raises(ValueError, match="facet field 'lang': the label names of source 1 differ"):
        rules([a, _bare(SparseIndex, 2, True, {"lang": (3, ["x", "z", "y"]), "topic": (4, None)}, {"year": torch.float32, "pages": torch.int32})])
    with pytest.raises(ValueError, match="facet field 'topic': the label names of source 1 differ"):
        rules([a, _bare(SparseIndex, 2, True, {"lang": (3, ["x", "y", "z"]), "topic": (4, list("abcd"))}, {"year": torch.float32, "pages": torch.int32})])
    with pytest.raises(ValueError, match="value field 'year' is missing in source 1"):
        rules([a, _bare(SparseIndex, 2, True, {"lang": (3, ["x", "y", "z"]), "topic": (4, None)}, {"pages": torch.int32})])
    with pytest.raises(ValueError, match="value field 'pages' is torch.int32 in source 0 and torch.float32 in source 1"):
        rules([a, _bare(SparseIndex, 2, True, {"lang": (3, ["x", "y", "z"]), "topic": (4, None)}, {"year": torch.float32, "pages": torch.float32})])
    # through concatenated(): the same errors, and the sources it does not take, all before a device index is asked for
    with pytest.raises(ValueError, match="value field 'year' is missing"):
        a.concatenated(_bare(SparseIndex, 2, True, {"lang": (3, ["x", "y", "z"]), "topic": (4, None)}, {"pages": torch.int32}))
    with pytest.raises(TypeError, match="joins indexes"):
        a.concatenated(np.zeros(3))
    with pytest.raises(NotImplementedError, match="dense Index"):
        a.concatenated(_bare(Index, 2))
    with pytest.raises(NotImplementedError, match="dense Index"):
        _bare(Index, 2).concatenated(a)
    sharded = _bare(SparseIndex, 2)
    sharded._group = object()
    with pytest.raises(NotImplementedError, match=r"unsharded\(\)"):
        a.concatenated(sharded)
    with pytest.raises(NotImplementedError, match=r"unsharded\(\)"):
        sharded.concatenated(a)
    with pytest.raises(ValueError, match="at most 256"):
        a.concatenated(*[a] * 256)
    with pytest.raises(ValueError, match="not row-sharded"):
        a.unsharded()
    assert a.parts is None


def test_retriever_merge_index_needs_an_index():
    from vsearch_amd.ir import Retriever

    class Fake:
        merge_index = Retriever.merge_index
    fake = Fake()
    fake.index = None
    with pytest.raises(RuntimeError, match="no index"):
        fake.merge_index([])


# ---- the host-only code under the host sanitizers ------------------------------------------------------------------------------------------------
def test_host_checks_under_a_host_sanitizer(tmp_path):
    """concat_check.h (the plan rule, every argument check, the capacity rule on the 64-bit totals, the table's bases and the kernels' source
    search against a plain scan on exact-size heap arrays) in a stand-alone program built with the host compiler under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "concat_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "concat_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "concat_check: ok" in run.stdout, run.stdout + run.stderr
