"""The pruned plane scan (RS_VT_PRUNE; prefilter, lists, passes B1 and B2) against
the oracle, bit for bit (index and score), on a 64 x 32 library of 130 templates
(blocks of 64, 64 and 2) at 1, 4, 37 and 300 queries: a ragged batch, G = 1 and
G = 8 query groups, several batches per group.  RS_VT_PRUNE=force prunes at any
size; prune_stats() tells how many (block, query) pairs each pass scanned."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import view_templates as V
from test_prune_bound import PF_UNITS, boundary_pair, lower_bounds

pytestmark = pytest.mark.gpu

T, NTB = 130, 3
COUNTS = [1, 4, 37, 300]
NQ_MAX = max(COUNTS)


@pytest.fixture(scope='module')
def vtmod():
    from pyratslam_amd import _build
    _build.build()
    import pyratslam_amd.view_templates as m
    return m


@functools.lru_cache(maxsize=None)
def base_library():
    lib = V.synthetic_library(T, 64, 32, seed=31)
    lib.setflags(write=False)
    return lib


def reference(lib, queries):
    sc = np.stack([V.vt_scores_library(lib, q) for q in queries])
    return sc.argmin(axis=1), sc.min(axis=1)


@functools.lru_cache(maxsize=None)
def mix_case(hit_frac):
    lib = base_library()
    queries, _ = V.synthetic_queries(lib, NQ_MAX, seed=32 + int(10 * hit_frac), hit_frac=hit_frac)
    return queries, reference(lib, queries)


def forced(vtmod, monkeypatch, lib):
    monkeypatch.setenv('RS_VT_PRUNE', 'force')
    h = vtmod.ViewTemplates._from_shape((64, 32), 45000)
    assert h.scan_form() == 'plane-pruned' and h.prune_stats() == (0, 0, 0, 0)
    h.add(lib)
    return h


def check(h, queries, ref, nq):
    idx, score, new = h.match_templates(queries[:nq], mode=0)
    assert not new.any()
    assert np.array_equal(score, ref[1][:nq])
    assert np.array_equal(idx, ref[0][:nq])
    l1, l2, pairs, passes = h.prune_stats()
    assert l1 == nq and pairs == NTB * nq and passes == 2 and 0 <= l2 <= (NTB - 1) * nq
    return l2


@pytest.mark.parametrize('nq', COUNTS)
def test_hits_scan_one_block_each(vtmod, monkeypatch, nq):
    """Every query re-sees a stored template: its block is the candidate and no other
    block's bound reaches the score found there, so pruning did happen."""
    queries, ref = mix_case(1.0)
    h = forced(vtmod, monkeypatch, base_library())
    assert check(h, queries, ref, nq) == 0
    h.close()


@pytest.mark.parametrize('nq', COUNTS)
def test_misses_scan_every_block(vtmod, monkeypatch, nq):
    queries, ref = mix_case(0.0)
    h = forced(vtmod, monkeypatch, base_library())
    assert check(h, queries, ref, nq) == (NTB - 1) * nq
    h.close()


@pytest.mark.parametrize('nq', COUNTS)
def test_mix_of_hits_and_misses(vtmod, monkeypatch, nq):
    queries, ref = mix_case(0.9)
    h = forced(vtmod, monkeypatch, base_library())
    l2 = check(h, queries, ref, nq)
    assert l2 == (NTB - 1) * int(np.count_nonzero(ref[1][:nq] > 45000))
    h.close()


@functools.lru_cache(maxsize=None)
def decoy_case(decoy_at):
    """Queries: noised copies of template 129.  The decoy equals template 129 on rows
    16..47 (every unit a prefilter may use) and is random elsewhere, so its bound equals
    the true match's while its score is large."""
    rng = np.random.default_rng(41)
    lib = base_library().copy()
    lib[decoy_at] = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
    lib[decoy_at, 16:48] = lib[129, 16:48]
    noise = rng.integers(0, 4, size=(NQ_MAX, 64, 32))
    queries = np.clip(lib[129].astype(np.int16)[None] - noise, 0, 255).astype(np.uint8)
    ref = reference(lib, queries)
    assert (ref[0] == 129).all()
    assert all((lower_bounds(lib[decoy_at], q) == lower_bounds(lib[129], q)).all() for q in queries[:4])
    return lib, queries, ref


@pytest.mark.parametrize('nq', COUNTS)
def test_decoy_in_a_lower_block_match_found_by_pass_b2(vtmod, monkeypatch, nq):
    lib, queries, ref = decoy_case(3)
    h = forced(vtmod, monkeypatch, lib)
    # block 0 (the decoy, lower on the tie of bounds) is every query's candidate; block 2
    # holds the match and is scanned by B2, and so is block 1 (B1 left a large score)
    assert check(h, queries, ref, nq) == 2 * nq
    h.close()


@pytest.mark.parametrize('nq', COUNTS)
def test_decoy_in_the_match_block(vtmod, monkeypatch, nq):
    lib, queries, ref = decoy_case(128)
    h = forced(vtmod, monkeypatch, lib)
    assert check(h, queries, ref, nq) == 0
    h.close()


@functools.lru_cache(maxsize=None)
def boundary_case():
    q = np.random.default_rng(43).integers(0, 256, size=(64, 32), dtype=np.uint8)
    lib = base_library().copy()
    lib[20], lib[100] = boundary_pair(q, units=PF_UNITS)
    queries = np.repeat(q[None], NQ_MAX, axis=0)
    ref = reference(lib, queries[:1])
    assert ref[0][0] == 20 and ref[1][0] == 40 and V.vt_score(lib[100], q) == 40
    return lib, queries, (np.repeat(ref[0], NQ_MAX), np.repeat(ref[1], NQ_MAX))


@pytest.mark.parametrize('nq', COUNTS)
def test_equal_score_at_a_lower_index_wins(vtmod, monkeypatch, nq):
    """X (index 20, block 0): bound = score = 40.  Y (index 100, block 1): score 40,
    bound 0, so block 1 is the candidate and leaves U = 40; block 0's bound equals U
    and must still be scanned (<=): the answer is X."""
    lib, queries, ref = boundary_case()
    h = forced(vtmod, monkeypatch, lib)
    assert check(h, queries, ref, nq) == nq      # block 0 only: block 2's bound is far above 40
    h.close()


@pytest.mark.parametrize('nq', COUNTS)
def test_identical_templates_first_index_wins(vtmod, monkeypatch, nq):
    lib = base_library().copy()
    lib[70] = lib[129] = lib[5]
    rng = np.random.default_rng(47)
    queries = np.clip(lib[5].astype(np.int16)[None] - rng.integers(0, 4, size=(nq, 64, 32)), 0, 255).astype(np.uint8)
    ref = reference(lib, queries)
    assert (ref[0] == 5).all()
    h = forced(vtmod, monkeypatch, lib)
    check(h, queries, ref, nq)
    h.close()


@pytest.mark.parametrize('nq', COUNTS)
def test_every_offset_as_the_unique_best(vtmod, monkeypatch, nq):
    lib = base_library()
    queries = np.stack([np.roll(lib[(37 * i) % T], (i % 15) - 7, axis=0) for i in range(nq)])
    ref = reference(lib, queries)
    assert (ref[1] == 0).all() and np.array_equal(ref[0], (37 * np.arange(nq)) % T)
    h = forced(vtmod, monkeypatch, lib)
    assert check(h, queries, ref, nq) == 0
    h.close()


@pytest.mark.parametrize('nq', COUNTS)
def test_all_zero_against_all_255(vtmod, monkeypatch, nq):
    lib = base_library().copy()
    lib[10], lib[90] = 0, 255
    queries = np.empty((nq, 64, 32), dtype=np.uint8)
    queries[0::2], queries[1::2] = 255, 0
    ref = reference(lib, queries[:2])
    ref = (np.resize(ref[0], nq), np.resize(ref[1], nq))
    h = forced(vtmod, monkeypatch, lib)
    check(h, queries, ref, nq)
    h.close()
    # ... and the only two templates: each direction of the wrap is some query's best
    two = np.stack([np.zeros((64, 32), np.uint8), np.full((64, 32), 255, np.uint8)])
    h = vtmod.ViewTemplates._from_shape((64, 32), 45000)
    h.add(two)
    idx, score, _ = h.match_templates(queries, mode=0)
    r2 = reference(two, queries[:2])
    assert np.array_equal(idx, np.resize(r2[0], nq)) and np.array_equal(score, np.resize(r2[1], nq))
    h.close()


# --- RS_VT_PRUNE=0 against 1 on random data: identical keys ----------------------
@functools.lru_cache(maxsize=None)
def random_case():
    lib = V.synthetic_library(400, 64, 32, seed=51)
    queries, _ = V.synthetic_queries(lib, 600, seed=52, hit_frac=0.8)
    return lib, queries


def pair_of_handles(vtmod, monkeypatch, make):
    out = []
    for v in ('0', '1'):
        monkeypatch.setenv('RS_VT_PRUNE', v)
        out.append(make())
    assert out[0].scan_form() == 'plane' and out[1].scan_form() == 'plane-pruned'
    return out


@pytest.mark.parametrize('where', ['device', 'host'])
def test_match_stream_same_keys_with_and_without_pruning(vtmod, monkeypatch, where):
    from pyratslam_amd import _lib
    lib, queries = random_case()
    dense, pruned = pair_of_handles(vtmod, monkeypatch, lambda: vtmod.ViewTemplates._from_shape((64, 32), 45000))
    res = []
    for h in (dense, pruned):
        h.add(lib)
        out = []
        for nb, nq in ((2, 300), (1, 560)):        # a second call with another query count
            q = np.ascontiguousarray(queries[:nb * nq].reshape(nb, nq, 64, 32))
            if where == 'device':
                buf = _lib.DeviceBuffer(q.nbytes).upload(q)
                out.append(h.match_stream((nb, nq, buf)))
                buf.close()
            else:
                out.append(h.match_stream(q))
        res.append(out)
    assert dense.prune_stats()[3] == 0
    l1, l2, pairs, passes = pruned.prune_stats()
    assert (l1, pairs, passes) == (560, 7 * 560, 2) and l2 < pairs - l1
    for a, b in zip(*res):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    ref = reference(lib, queries[:20])
    assert np.array_equal(res[1][0][0].ravel()[:20], ref[0]) and np.array_equal(res[1][0][1].ravel()[:20], ref[1])
    dense.close()
    pruned.close()


def test_scan_local_on_three_shards_same_keys(vtmod, monkeypatch):
    from pyratslam_amd import _lib
    lib, queries = random_case()
    keys = []
    for v in ('0', '1'):
        monkeypatch.setenv('RS_VT_PRUNE', v)
        shards = [vtmod.ShardedViewTemplates.from_shape((64, 32), 45000, r, 3, reducer=lambda k: k)
                  for r in range(3)]
        per_call = []
        for nq in (600, 520, 37):                  # the counters are left at zero; 37: dense launch
            local = []
            for s in shards:
                if not per_call:
                    s.add(lib)
                k = np.empty(nq, dtype=np.uint64)
                _lib.check(s._lib.rs_vt_scan_local(s._h, nq, _lib.ptr(np.ascontiguousarray(queries[:nq]), ctypes.c_uint8),
                                                   _lib.ptr(k, ctypes.c_uint64)))
                local.append(k)
            per_call.append(local)
        if v == '1':
            assert all(s.prune_stats() == (520, s.prune_stats()[1], 3 * 520, 2) for s in shards)
        keys.append(per_call)
        for s in shards:
            s.close()
    for a, b in zip(*keys):
        for ka, kb in zip(a, b):
            assert np.array_equal(ka, kb)
    glob = np.minimum.reduce(keys[1][0])
    ref = reference(lib, queries[:20])
    assert np.array_equal((glob & 0xFFFFFFFF)[:20].astype(np.int64), ref[0])
    assert np.array_equal((glob >> 32)[:20], ref[1])
