"""CPU tests of fused search: the numpy reference of vs_fuse_topk (tests/_fuse_ref.py) pinned on cases small enough to work out by hand, and
the host-side argument checks (vsearch_amd/csrc/fuse_check.h) run in a stand-alone program under the host sanitizers.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _fuse_ref as ref

F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B_, C_, D = 11, 22, 33, 44


def _lists(*lists):
    """lists of (id, score) pairs of ONE query -> ids / scores [L, 1, kk], shorter lists padded with id -1 / score -inf"""
    kk = max(len(x) for x in lists)
    ids = np.full((len(lists), 1, kk), -1, dtype=np.int64)
    sc = np.full((len(lists), 1, kk), -np.inf, dtype=F32)
    for l, x in enumerate(lists):
        for j, (d, s) in enumerate(x):
            ids[l, 0, j], sc[l, 0, j] = d, s
    return ids, sc


def test_one_list_under_rrf_keeps_its_order():
    ids, sc = _lists([(C_, 9.0), (A, 7.0), (D, 7.0), (B_, 1.0)])
    got = ref.fuse(ids, sc, 6, "rrf")
    assert got["ids"].tolist() == [[C_, A, D, B_, -1, -1]] and got["n"].tolist() == [4]
    assert got["ranks"][0, :, 0].tolist() == [0, 1, 2, 3, -1, -1]
    want = [F32(1) / F32(F32(60) + F32(r + 1)) for r in range(4)]
    assert got["fused"][0, :4].view(np.uint32).tolist() == np.array(want, dtype=F32).view(np.uint32).tolist()
    assert np.isneginf(got["fused"][0, 4:]).all() and np.isneginf(got["scores"][0, 4:]).all()
    assert got["scores"][0, :4, 0].tolist() == [9.0, 7.0, 7.0, 1.0]


def test_the_symmetric_case_ties_and_the_id_decides():
    for first, second in ((A, B_), (B_, A)):                                     # whichever list order: the lower id comes first
        ids, sc = _lists([(first, 2.0), (second, 1.0)], [(second, 5.0), (first, 4.0)])
        got = ref.fuse(ids, sc, 2, "rrf")
        assert got["fused"][0, 0] == got["fused"][0, 1] and got["ids"].tolist() == [[A, B_]]
        assert ref.tied_neighbours(got) == 1
    assert sorted(got["ranks"][0].tolist()) == [[0, 1], [1, 0]]


def test_a_zero_weight_silences_a_list_but_keeps_its_documents():
    ids, sc = _lists([(A, 2.0), (B_, 1.0)], [(C_, 9.0), (B_, 8.0), (A, 7.0)])
    got = ref.fuse(ids, sc, 5, "rrf", weights=[1.0, 0.0])
    assert got["n"].tolist() == [3] and got["ids"].tolist() == [[A, B_, C_, -1, -1]]          # list 0's order; C only stands in the silent list
    assert got["fused"][0, 2] == 0 and got["ranks"][0, 2].tolist() == [-1, 0] and got["scores"][0, 2, 1] == 9.0
    one = ref.fuse(ids[:1], sc[:1], 5, "rrf")
    assert got["fused"][0, :2].view(np.uint32).tolist() == one["fused"][0, :2].view(np.uint32).tolist()


def test_mnz_multiplies_by_the_number_of_lists_holding_the_document():
    ids, sc = _lists([(A, 4.0), (B_, 2.0), (C_, 0.0)], [(B_, 3.0), (D, 1.0)], [(B_, 10.0), (A, 0.0)])
    s, m = ref.fuse(ids, sc, 4, "sum"), ref.fuse(ids, sc, 4, "mnz")
    count = {A: 2, B_: 3, C_: 1, D: 1}
    by_id = {int(d): f for d, f in zip(s["ids"][0], s["fused"][0])}
    assert by_id[B_] == F32(2.5) and by_id[A] == F32(1) and by_id[C_] == 0 and by_id[D] == 0     # B: 0.5 + 1 + 1
    for d, f in zip(m["ids"][0], m["fused"][0]):
        assert f == F32(by_id[int(d)] * F32(count[int(d)]))
    assert m["ids"][0].tolist() == [B_, A, C_, D] and m["fused"][0].tolist() == [7.5, 2.0, 0.0, 0.0]


def test_a_repeated_id_counts_once_at_its_lower_position():
    ids, sc = _lists([(A, 5.0), (B_, 4.0), (A, 3.0), (A, 1.0)], [(B_, 2.0), (B_, 1.0)])
    got = ref.fuse(ids, sc, 4, "rrf", c=0.0)
    assert got["n"].tolist() == [2] and got["ids"].tolist() == [[B_, A, -1, -1]]
    assert got["fused"][0, :2].tolist() == [1.5, 1.0]                            # B: 1/2 + 1/1, A: 1/1
    assert got["ranks"][0, :2].tolist() == [[1, 0], [0, -1]] and got["scores"][0, 1, 0] == 5.0
    raw = ref.fuse(ids, sc, 4, "raw")
    assert raw["ids"][0, :2].tolist() == [B_, A] and raw["fused"][0, :2].tolist() == [6.0, 5.0]
    norm = ref.fuse(ids, sc, 4, "sum")                                           # the ignored entries still stretch the list's score range: 1 .. 5
    assert norm["fused"][0, :2].tolist() == [1.75, 1.0]                          # B: (4 - 1) / 4 + 1, A: 1


def test_padding_ends_a_list_wherever_it_stands():
    ids, sc = _lists([(A, 3.0), (B_, 2.0), (C_, 1.0), (D, 0.5)], [(B_, 9.0)])
    ids[0, 0, 2] = -1                                                            # padded from the middle: C and D are ignored
    ids[1, 0, :] = -1                                                            # an all-padding list
    got = ref.fuse(ids, sc, 3, "sum")
    assert got["n"].tolist() == [2] and got["ids"].tolist() == [[A, B_, -1]]
    assert got["fused"][0, :2].tolist() == [1.0, 0.0]                            # the range is 2 .. 3, not 0.5 .. 3
    assert got["ranks"][0].tolist() == [[0, -1], [1, -1], [-1, -1]]
    ids[0, 0, 0] = -1                                                            # nothing at all
    got = ref.fuse(ids, sc, 3, "rrf")
    assert got["n"].tolist() == [0] and (got["ids"] == -1).all() and np.isneginf(got["fused"]).all() and (got["ranks"] == -1).all()
    ids, sc = _lists([(A, 3.0), (ref.ID_END, 2.0), (C_, 1.0)])                   # an id the keys cannot hold ends the list as -1 does
    assert ref.fuse(ids, sc, 3, "rrf")["ids"].tolist() == [[A, -1, -1]]


def test_a_flat_list_normalises_to_one():
    ids, sc = _lists([(A, 0.25), (B_, 0.25), (C_, 0.25)], [(C_, -3.0)])
    got = ref.fuse(ids, sc, 3, "sum", weights=[0.5, 2.0])
    assert got["ids"].tolist() == [[C_, A, B_]] and got["fused"].tolist() == [[2.5, 0.5, 0.5]]
    assert ref.tied_neighbours(got) == 1


def test_raw_with_fill_is_the_hand_computed_sum():
    ids, sc = _lists([(A, 0.75), (B_, 0.5)], [(B_, 0.25), (C_, 0.125)])
    w = np.array([[2.0, 4.0, 99.0]], dtype=F32)                                  # [B, ldw = 3]
    fill = np.array([[-1.0, 0.0625]], dtype=F32)
    got = ref.fuse(ids, sc, 3, "raw", weights=w, fill=fill)
    #   A: 2 * 0.75 + 4 * 0.0625 = 1.75   B: 2 * 0.5 + 4 * 0.25 = 2   C: 2 * -1 + 4 * 0.125 = -1.5
    assert got["ids"].tolist() == [[B_, A, C_]] and got["fused"].tolist() == [[2.0, 1.75, -1.5]]
    bare = ref.fuse(ids, sc, 3, "raw", weights=w)
    assert bare["ids"].tolist() == [[B_, A, C_]] and bare["fused"].tolist() == [[2.0, 1.5, 0.5]]
    assert np.isneginf(got["scores"][0, 1, 1]) and got["ranks"][0, 1].tolist() == [0, -1]       # fill stands in the sum, not in the detail rows


def test_cut_and_the_kernel_case_generator():
    ids, sc = ref.kernel_case(3, 10, seed=1)
    full = ref.fuse_all(ids, sc, "rrf")
    assert [len(q) for q in full] == [30, 10, 5 + 3 * 5]                         # disjoint, identical, half shared
    a, b = ref.cut(full, 4, 3), ref.cut(full, 40, 3)
    assert (a["ids"] == b["ids"][:, :4]).all() and (a["n"] == b["n"]).all() and (b["ids"][1, 10:] == -1).all()
    assert ref.tied_neighbours(b) > 0
    for mode in ("sum", "mnz", "raw"):
        assert ref.tied_neighbours(ref.fuse(ids, sc, 40, mode)) > 0
    flat_i, flat_s = ref.layout(ids, sc, 13, 50)
    assert flat_i.shape == (2 * 50 + 2 * 13 + 10,) and (flat_i[50 + 13:50 + 23] == ids[1, 1]).all() and (flat_s[100 + 26:] == sc[2, 2]).all()


def test_facade_argument_checks_need_no_device():
    from vsearch_amd import _native as nat
    from vsearch_amd.device_index import _fuse_args, _fuse_rows, _stack_lists
    assert _fuse_args(10, "rrf", 60, 100, 3) == (10, nat.FUSE_RRF, 60.0, 100) and _fuse_args(np.int64(1), "raw", 0)[1] == nat.FUSE_RAW
    for bad in (dict(k=0), dict(k=1025), dict(mode="borda"), dict(c=-1), dict(c=float("inf")), dict(c=float("nan")), dict(depth=0),
                dict(depth=1025), dict(L=0), dict(L=9), dict(L=5, depth=820)):
        with pytest.raises(ValueError):
            _fuse_args(**{"k": 5, **bad})
    for bad in (2.5, True, "3"):
        with pytest.raises(TypeError):
            _fuse_args(bad)
    assert _fuse_args(5, depth=819, L=5)[3] == 819                               # 4095 entries fit
    w, ldw = _fuse_rows([1, 2, 3], 4, 3, "weights")
    assert w.dtype == F32 and ldw == 0 and _fuse_rows(None, 4, 3, "weights") == (None, 0)
    w, ldw = _fuse_rows(np.ones((4, 5)), 4, 3, "weights")
    assert w.shape == (4, 5) and ldw == 5
    for bad in (np.ones(2), np.ones((3, 3)), np.ones((4, 2)), np.ones((4, 3, 1))):
        with pytest.raises(ValueError):
            _fuse_rows(bad, 4, 3, "weights")
    a, b = (np.arange(6, dtype=np.int64).reshape(2, 3), np.ones((2, 3), F32)), (np.full((2, 1), 7, np.int64), np.zeros((2, 1), F32))
    ids, sc = _stack_lists([a, b])
    assert ids.shape == (2, 2, 3) and ids[1].tolist() == [[7, -1, -1], [7, -1, -1]] and np.isneginf(sc[1, :, 1:]).all() and (sc[0] == 1).all()
    for bad in ([], [a, (np.zeros((3, 1), np.int64), np.zeros((3, 1), F32))], [(a[0], a[1][:, :2])], [a[0]]):
        with pytest.raises((ValueError, TypeError)):
            _stack_lists(bad)


def test_host_checks_under_a_host_sanitizer(tmp_path):
    """fuse_check.h (every limit of vs_fuse_topk, and what it checks in host arrays before it stages them) in a stand-alone program built
    with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path / "fuse_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "fuse_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and "fuse_check: ok" in run.stdout, run.stdout + run.stderr
