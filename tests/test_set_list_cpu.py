"""CPU checks of the set egress: the pinned hash against its known answers -- from the numpy reference, from the library's host
function and from the stand-alone program --, paging, the two shard rules composed on the reference, the uniformity of the hash's definition,
the plan rule (vs_set_list_plan is pure host arithmetic), the argument errors of the C ABI without a GPU, the facade's host logic, and the
host-only code (vsearch_amd/csrc/set_list_check.h) run in a stand-alone program under the host sanitizers.  No device is needed; nothing is
loaded into Python under a sanitizer."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from vsearch_amd import _native as nat
from vsearch_amd import device_index as di

import _set_list_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    """set_list_check_main.cpp built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    prog = str(tmp_path_factory.mktemp("set_list") / "set_list_check")
    src = os.path.join(REPO, "vsearch_amd", "csrc", "set_list_check_main.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.dirname(src), src, "-o", prog])
    return prog


# ---- the hash --------------------------------------------------------------------------------------------------------------------------------
def test_hash_known_answers_from_the_reference():
    for seed, id_, h in ref.KNOWN_HASHES:
        assert int(ref.sample_hash(seed, [id_])[0]) == h, (seed, id_)


def test_hash_known_answers_from_the_library():
    for seed, id_, h in ref.KNOWN_HASHES:
        assert di.set_sample_hash(seed, id_) == h, (seed, id_)
    rng = np.random.default_rng(1)
    for seed in (0, 1, 7, (1 << 63) + 5, (1 << 64) - 1):
        ids = np.concatenate([rng.integers(0, 1 << 40, size=50), [0, 1, (1 << 32) - 2, 21015323]]).astype(np.int64)
        assert [di.set_sample_hash(seed, int(i)) for i in ids] == ref.sample_hash(seed, ids).tolist()


def test_hash_known_answers_from_the_stand_alone_program(check_program):
    args = [str(x) for seed, id_, _ in ref.KNOWN_HASHES for x in (seed, id_)]
    run = subprocess.run([check_program, "hash"] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert [int(line, 16) for line in run.stdout.split()] == [h for _, _, h in ref.KNOWN_HASHES]


# ---- the window and the pages ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.0, 0.02, 0.5, 1.0])
def test_pages_concatenated_equal_the_whole_list(density):
    n = 517
    mask = np.random.default_rng(3).random(n) < density
    whole, counts = ref.set_ids(mask, None, n)
    assert counts[0] == mask.sum() and (whole[0, :counts[0]] == np.nonzero(mask)[0]).all() and (whole[0, counts[0]:] == -1).all()
    for page_size in (1, 2, 7, 64, 516, 517, 518, 2000):
        got = np.concatenate(list(ref.pages(mask, page_size)))
        assert (got[:counts[0]] == whole[0, :counts[0]]).all() and (got[counts[0]:] == -1).all() and got.shape[0] < counts[0] + page_size + 1


def test_window_edges_of_the_reference():
    mask = np.zeros((2, 100), bool)
    mask[0, [3, 50, 99]] = True
    ids, counts = ref.set_ids(mask, [1, 0], 4, id_offset=1000)
    assert counts.tolist() == [3, 0] and ids.tolist() == [[1050, 1099, -1, -1], [-1, -1, -1, -1]]
    assert ref.set_ids(mask, [3, 7], 2)[0].tolist() == [[-1, -1], [-1, -1]]                          # an offset at, and past, the count
    assert ref.set_ids(mask, None, 0)[0].shape == (2, 0)


# ---- the shard rules, on the reference ------------------------------------------------------------------------------------------------------------
CUTS = [5, 101]


def _shard_case(seed, B=3, n=300):
    rng = np.random.default_rng(seed)
    mask = rng.random((B, n)) < np.array([0.02, 0.5, 0.95])[:B, None]
    mask[0, [4, 5, 100, 101]] = True                                                               # members on both sides of each cut
    return mask


def test_window_rule_over_cuts_equals_the_unsharded_list():
    mask = _shard_case(5)
    total = mask.sum(axis=1)
    for limit in (0, 1, 3, 50, 400):
        for offset in (0, 1, 2, 4, 60, 150, 299, 300):
            want, counts = ref.set_ids(mask, [offset] * 3, limit)
            got, got_counts = ref.sharded_ids(mask, CUTS, offset, limit)
            assert (got == want).all() and (got_counts == counts).all() and (counts == total).all(), (offset, limit)
    per_query = np.array([0, 7, 280], np.int64)                                                    # windows that start in one shard and end in the next
    want, _ = ref.set_ids(mask, per_query, 40)
    assert (ref.sharded_ids(mask, CUTS, per_query, 40)[0] == want).all()
    one = np.zeros((1, 300), bool)
    one[0, [4, 5, 6, 100, 101, 102]] = True
    assert ref.sharded_ids(one, CUTS, 1, 4)[0].tolist() == [[5, 6, 100, 101]]                       # one window over all three shards


def test_sample_merge_over_cuts_equals_the_unsharded_sample():
    mask = _shard_case(6)
    seeds = [0, 1, (1 << 64) - 1]
    for n in (1, 5, 32, 299, 400):
        want = ref.set_sample(mask, seeds, n)
        got = ref.sharded_sample(mask, CUTS, seeds, n)
        assert all((g == w).all() for g, w in zip(got, want)), n
    ids, hs, counts = ref.set_sample(mask, seeds, 400)
    for b in range(3):
        real = ids[b] >= 0
        assert real.sum() == counts[b] and sorted(ids[b][real].tolist()) == np.nonzero(mask[b])[0].tolist()      # n > count: the whole set
        assert (hs[b][~real] == ref.NO_HASH).all() and (np.diff(hs[b][real].astype(np.int64)) >= 0).all()


# ---- the uniformity of the hash's definition ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,M,n,S", [(0, 64, 8, 4096), (1_000_000, 64, 8, 4096), (64, 64, 8, 4096), (0, 1000, 10, 4096), (5, 37, 1, 8192),
                                        (0, 256, 32, 2048)])
def test_sampling_frequencies_are_uniform(base, M, n, S):
    """Over seeds 0..S - 1, how often each of M rows is sampled, against the binomial variance: chi^2 / df < 1.5.  The inputs are fixed, so the
    outcome is deterministic (the reference gives 0.88 to 1.07 on these)."""
    stat = ref.chi2_per_df(base, M, n, S)
    print(f"chi2/df ({M} from {base}, n = {n}, S = {S}) = {stat:.4f}")
    assert stat < 1.5


# ---- the plan rule and the constants -----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_constants():
    text = open(os.path.join(REPO, "include", "vsearch_hip.h")).read()
    get = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert get("VS_SET_MAX_SAMPLE") == nat.SET_MAX_SAMPLE == ref.MAX_SAMPLE == di.MAX_SET_SAMPLE == 1024
    assert get("VS_SET_MAX_OUT_IDS") == nat.SET_MAX_OUT_IDS == ref.MAX_OUT_IDS == di.MAX_SET_IDS == 1 << 27
    for name in ("vs_set_list_plan", "vs_set_count", "vs_index_set_count", "vs_set_ids", "vs_index_set_ids", "vs_set_sample", "vs_index_set_sample",
                 "vs_set_from_ids"):
        assert name in nat.EXPORTED_SYMBOLS and ("VS_API int %s(" % name) in text
    assert "VS_API uint32_t vs_set_sample_hash(" in text and "vs_set_sample_hash" in nat.EXPORTED_SYMBOLS
    for seed, id_, h in ref.KNOWN_HASHES[:4]:
        assert ("(%d, %d) 0x%08x" % (seed, id_, h)) in text                                         # the header pins the known answers


@pytest.mark.parametrize("n_rows", [1, 64, 2049, 1_000_000, 21_015_324, (1 << 32) - 1])
@pytest.mark.parametrize("B,per_query", [(1, False), (1, True), (8, True), (9, True), (64, True)])
def test_plan_against_its_rule(n_rows, B, per_query):
    for rpc_in in (0, 64, 2048, 6144, 2048 * 3 + 64):
        got = di.set_list_plan(n_rows, B, per_query, rpc_in)
        assert got == ref.plan_rule(n_rows, B, rpc_in)
        chunks, rpc, spans = got
        assert rpc % 2048 == 0 and chunks * rpc >= n_rows > (chunks - 1) * rpc and spans * 2048 >= n_rows > (spans - 1) * 2048


def test_plan_argument_errors():
    for args in [(0, 1, True, 0), (1 << 32, 1, True, 0), (100, 0, True, 0), (100, 1, True, 100), (100, 1, True, -64), (100, 2, False, 0),
                 ((1 << 32) - 1, 65, True, 0), (100, 65536, True, 0)]:
        with pytest.raises(ValueError):
            di.set_list_plan(*args)
    o = C.c_int64(0)
    assert nat.lib().vs_set_list_plan(100, 1, 1, 0, None, C.byref(o), C.byref(o)) == nat.VS_EINVAL


# ---- argument errors of the C ABI, checked before the device is touched ----------------------------------------------------------------------
def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def test_argument_errors_without_a_device(have_gpu):
    good = nat.VS_OK if have_gpu else nat.VS_ENODEVICE
    n, L = 100, nat.lib()
    words = np.full((3, 5), -1, np.int32)

    def count(B=3, bit0=0, ld=5, rpc=0, w=words, n_rows=n, out=True):
        o = np.zeros(max(B, 1), np.int64) if out else None                                        # (held through the call: a good call writes it)
        return L.vs_set_count(_p(w), bit0, ld, None, B, n_rows, rpc, _p(o), 0, None)
    assert count() == good and count(bit0=37) == good and count(w=None, B=1, ld=0) == good and count(rpc=64) == good
    assert count(out=False) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert count(B=0) == nat.VS_EINVAL and count(bit0=-1) == nat.VS_EINVAL and count(bit0=64) == nat.VS_EINVAL and "ld_words" in nat.last_error()
    assert count(ld=0) == nat.VS_EINVAL and count(rpc=100) == nat.VS_EINVAL and "multiple of 64" in nat.last_error()
    assert count(n_rows=0) == nat.VS_EINVAL and count(n_rows=1 << 32) == nat.VS_EINVAL and count(w=None, B=2, ld=0) == nat.VS_EINVAL
    one, seed = np.zeros(1, np.int64), np.zeros(1, np.uint64)
    assert L.vs_index_set_count(None, None, 0, 0, 1, 0, _p(one), None) == nat.VS_EINVAL and "NULL" in nat.last_error()

    def ids(B=3, limit=7, offsets=None, ids_out=True, counts=True, ld=5, rpc=0):
        off = None if offsets is None else np.asarray(offsets, np.int64)
        # (a call that is refused never touches its buffers: the over-long limit gets a short one)
        o = np.zeros((B, min(max(limit, 1), 64)), np.int64) if ids_out else None
        c = np.zeros(B, np.int64) if counts else None
        return L.vs_set_ids(_p(words), 0, ld, None, B, n, _p(off), limit, 1000, rpc, _p(o), _p(c), 0, None)
    assert ids() == good and ids(limit=0, ids_out=False) == good and ids(offsets=[0, 5, 1 << 40]) == good and ids(rpc=2048) == good
    assert ids(offsets=[0, -1, 0]) == nat.VS_EINVAL and "offsets[1]" in nat.last_error()
    assert ids(limit=-1) == nat.VS_EINVAL and "limit" in nat.last_error()
    assert ids(limit=(1 << 27) // 3 + 1, ids_out=True) == nat.VS_EINVAL and "2^27" in nat.last_error()
    assert ids(ids_out=False) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert ids(counts=False) == nat.VS_EINVAL and ids(ld=3) == nat.VS_EINVAL and ids(rpc=1) == nat.VS_EINVAL
    assert L.vs_index_set_ids(None, None, 0, 0, 1, None, 1, 0, 0, _p(one), _p(one), None) == nat.VS_EINVAL

    def sample(B=3, k=5, seeds=True, ids_out=True, hs=True, counts=True, rpc=0, n_rows=n, w=words, ld=5):
        sd = np.zeros(B, np.uint64) if seeds else None
        o = np.zeros((B, max(k, 1)), np.int64) if ids_out else None
        h = np.zeros((B, max(k, 1)), np.uint32) if hs else None
        c = np.zeros(B, np.int64) if counts else None
        return L.vs_set_sample(_p(w), 0, ld, None, B, n_rows, _p(sd), k, 0, rpc, _p(o), _p(h), _p(c), 0, None)
    assert sample() == good and sample(hs=False) == good and sample(k=1024) == good and sample(k=1) == good
    assert sample(k=0) == nat.VS_EINVAL and "n must" in nat.last_error()
    assert sample(k=1025) == nat.VS_EINVAL and "n must" in nat.last_error()
    for k in ("seeds", "ids_out", "counts"):
        assert sample(**{k: False}) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert sample(rpc=100) == nat.VS_EINVAL
    assert sample(B=1, k=1024, n_rows=(1 << 32) - 1, w=None, ld=0, rpc=2048) == nat.VS_EINVAL and "scratch" in nat.last_error()
    assert L.vs_index_set_sample(None, None, 0, 0, 1, _p(seed), 1, 0, 0, _p(one), None, _p(one), None) == nat.VS_EINVAL

    def from_ids(lists=((0, 99, -1, 5), (7, 7, -5, 98)), B=2, m=4, ld_ids=4, n_rows=n, bit0=37, ld=5, out=True, null_ids=False):
        a = np.asarray(lists, np.int64)
        o = np.zeros((max(B, 1), 8), np.int32) if out else None
        return L.vs_set_from_ids(None if null_ids else _p(a), B, m, ld_ids, n_rows, bit0, 1, _p(o), ld, 0, None)
    assert from_ids() == good and from_ids(m=0, ld_ids=0, null_ids=True) == good and from_ids(bit0=0, ld=4) == good
    assert from_ids(n_rows=99) == nat.VS_EINVAL and "ids[0, 1] = 99" in nat.last_error()          # an id at n_rows in a host array
    assert from_ids(null_ids=True) == nat.VS_EINVAL and "NULL" in nat.last_error()
    assert from_ids(out=False) == nat.VS_EINVAL and from_ids(ld=4) == nat.VS_EINVAL and "ld_words" in nat.last_error()
    assert from_ids(ld_ids=3) == nat.VS_EINVAL and from_ids(B=0) == nat.VS_EINVAL and from_ids(m=-1) == nat.VS_EINVAL
    assert from_ids(bit0=-1) == nat.VS_EINVAL and from_ids(n_rows=0) == nat.VS_EINVAL


# ---- the facade's host logic -------------------------------------------------------------------------------------------------------------------
def test_window_and_sample_args():
    assert di._set_window_args(0, None) == (0, None) and di._set_window_args(np.int64(5), 7) == (5, 7)
    off, limit = di._set_window_args([1, 2, 3], 0)
    assert off.dtype == np.int64 and off.tolist() == [1, 2, 3] and limit == 0
    for bad in ((-1, 5), ([0, -1], 5), (0, -1), (0, 1.5), (0, True)):
        with pytest.raises(ValueError):
            di._set_window_args(*bad)
    for bad in (1.5, [0.5], [[1, 2]], []):
        with pytest.raises(TypeError):
            di._set_window_args(bad, 1)
    assert di._offsets_for(0, 4) is None and di._offsets_for(3, 2).tolist() == [3, 3]
    with pytest.raises(ValueError, match="3 offsets"):
        di._offsets_for(np.zeros(3, np.int64), 2)
    assert di._set_sample_args(1, 0) == (1, 0) and di._set_sample_args(1024, -5) == (1024, -5)
    for bad in (0, 1025, 1.5, True):
        with pytest.raises(ValueError):
            di._set_sample_args(bad, 0)
    with pytest.raises(TypeError):
        di._set_sample_args(5, 0.5)
    seeds = di._sample_seeds((1 << 64) - 1, 3).view(np.uint64)
    assert seeds.tolist() == [(1 << 64) - 1, 0, 1]                                                  # seed + b, modulo 2^64


def test_index_facade_host_checks():
    from vsearch_amd.ir import SparseIndex
    idx = SparseIndex()
    with pytest.raises(ValueError, match="go together"):
        idx.list_ids(q_embs=np.zeros((1, 6), np.float32))
    with pytest.raises(ValueError, match="offset"):
        idx.list_ids(offset=-1)
    with pytest.raises(ValueError, match="n must"):
        idx.sample_ids(0)
    with pytest.raises(ValueError, match="go together"):
        idx.sample_ids(5, min_score=1.0)


# ---- the host-only code under the host sanitizers ------------------------------------------------------------------------------------------------
def test_host_checks_under_a_host_sanitizer(check_program):
    """set_list_check.h (the hash's known answers, the sample key's order, the window arithmetic composed span by span against a plain list on
    exact-size heap arrays, the invert mask, the plan rule, every check) in a stand-alone program built with the host compiler under
    AddressSanitizer and UndefinedBehaviorSanitizer"""
    run = subprocess.run([check_program], capture_output=True, text=True)
    assert run.returncode == 0 and "set_list_check: ok" in run.stdout, run.stdout + run.stderr
