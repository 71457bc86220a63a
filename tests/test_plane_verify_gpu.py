"""The pruned plane scan's verification step (vt_prune_verify_kernel): before pass B1 the
one template that holds the candidate block's least bound is scored exactly, and where
every other bound of the block exceeds that score the query is settled without a block
scan.  Index and score against the oracle, bit for bit, with RS_VT_PRUNE=force on a
64 x 32 library of 130 templates (blocks of 64, 64 and 2) at 1, 4, 37 and 300 queries;
prune_verified() against the NumPy restatement of the rule (test_prune_verify_rule)."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import view_templates as V
from test_prune_bound import PF_UNITS, boundary_pair
from test_prune_verify_rule import settled_mask

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
    lib = V.synthetic_library(T, 64, 32, seed=71)
    lib.setflags(write=False)
    return lib


def reference(lib, queries):
    sc = np.stack([V.vt_scores_library(lib, q) for q in queries])
    return sc.argmin(axis=1), sc.min(axis=1)


def noised(t, n, seed):
    rng = np.random.default_rng(seed)
    return np.clip(t.astype(np.int16)[None] - rng.integers(0, 4, size=(n, 64, 32)), 0, 255).astype(np.uint8)


def forced(vtmod, monkeypatch, lib):
    monkeypatch.setenv('RS_VT_PRUNE', 'force')
    h = vtmod.ViewTemplates._from_shape((64, 32), 45000)
    assert h.scan_form() == 'plane-pruned' and h.prune_stats() == (0, 0, 0, 0) and h.prune_verified() == 0
    h.add(lib)
    return h


def check(h, queries, ref, nq, ntb=NTB):
    """Answers and the stats' contract; returns (pairs of pass B2, verified queries)."""
    idx, score, new = h.match_templates(queries[:nq], mode=0)
    assert not new.any()
    assert np.array_equal(score, ref[1][:nq])
    assert np.array_equal(idx, ref[0][:nq])
    l1, l2, pairs, passes = h.prune_stats()
    assert l1 == nq and pairs == ntb * nq and passes == 2 and 0 <= l2 <= (ntb - 1) * nq
    ver = h.prune_verified()
    assert 0 <= ver <= nq
    return l2, ver


@functools.lru_cache(maxsize=None)
def mix_case(hit_frac):
    lib = base_library()
    queries, _ = V.synthetic_queries(lib, NQ_MAX, seed=72 + int(10 * hit_frac), hit_frac=hit_frac)
    return queries, reference(lib, queries), settled_mask(lib, queries)


@pytest.mark.parametrize('nq', COUNTS)
def test_all_hits_are_settled_by_verification(vtmod, monkeypatch, nq):
    queries, ref, settled = mix_case(1.0)
    assert settled.all()
    h = forced(vtmod, monkeypatch, base_library())
    assert check(h, queries, ref, nq) == (0, nq)
    assert h.prune_stats() == (nq, 0, 3 * nq, 2)
    h.close()


@pytest.mark.parametrize('hit_frac', [0.0, 0.9])
@pytest.mark.parametrize('nq', COUNTS)
def test_verified_count_is_the_rules(vtmod, monkeypatch, nq, hit_frac):
    queries, ref, settled = mix_case(hit_frac)
    h = forced(vtmod, monkeypatch, base_library())
    l2, ver = check(h, queries, ref, nq)
    assert ver == int(np.count_nonzero(settled[:nq]))
    assert l2 == (NTB - 1) * int(np.count_nonzero(ref[1][:nq] > 45000))
    h.close()


@pytest.mark.parametrize('nq', COUNTS)
def test_identical_templates_in_one_block(vtmod, monkeypatch, nq):
    """Equal bounds: min2 = min1 <= U0, not settled; the block scan returns the lower index."""
    lib = base_library().copy()
    lib[40] = lib[5]
    queries = noised(lib[5], nq, 73)
    ref = reference(lib, queries)
    assert (ref[0] == 5).all()
    h = forced(vtmod, monkeypatch, lib)
    assert check(h, queries, ref, nq) == (0, 0)
    h.close()


@pytest.mark.parametrize('nq', COUNTS)
def test_identical_templates_in_two_blocks(vtmod, monkeypatch, nq):
    """Settled in block 0 (the lower block on the tie of bounds); block 1's bound does not
    exceed the score, so it is still on list2, and index 5 wins."""
    lib = base_library().copy()
    lib[70] = lib[5]
    queries = noised(lib[5], nq, 74)
    ref = reference(lib, queries)
    assert (ref[0] == 5).all()
    h = forced(vtmod, monkeypatch, lib)
    assert check(h, queries, ref, nq) == (nq, nq)
    h.close()


@pytest.mark.parametrize('nq', COUNTS)
def test_second_bound_equal_to_the_score_is_block_scanned(vtmod, monkeypatch, nq):
    """X (index 20): bound = score = 40.  Y (index 30, same block): bound 0, score 40.
    l^ = Y, U0 = 40 = min2: not settled (>), and the block scan returns X."""
    q = np.random.default_rng(75).integers(0, 256, size=(64, 32), dtype=np.uint8)
    lib = base_library().copy()
    lib[20], lib[30] = boundary_pair(q, units=PF_UNITS)
    queries = np.repeat(q[None], nq, axis=0)
    r = reference(lib, queries[:1])
    assert r[0][0] == 20 and r[1][0] == 40 and V.vt_score(lib[30], q) == 40
    assert not settled_mask(lib, queries[:1])[0]
    h = forced(vtmod, monkeypatch, lib)
    assert check(h, queries, (np.repeat(r[0], nq), np.repeat(r[1], nq)), nq) == (0, 0)
    h.close()


@pytest.mark.parametrize('nq', COUNTS)
def test_decoy_at_lane_zero_of_the_match_block(vtmod, monkeypatch, nq):
    """The decoy (index 128, lane 0 of block 2) equals template 129 on the prefilter's rows:
    l^ is the decoy, U0 is large, and the block scan finds the match."""
    rng = np.random.default_rng(76)
    lib = base_library().copy()
    lib[128] = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
    lib[128, 16:48] = lib[129, 16:48]
    queries = noised(lib[129], nq, 77)
    ref = reference(lib, queries)
    assert (ref[0] == 129).all() and not settled_mask(lib, queries[:4]).any()
    h = forced(vtmod, monkeypatch, lib)
    assert check(h, queries, ref, nq) == (0, 0)
    h.close()


@pytest.mark.parametrize('nq', COUNTS)
def test_block_of_one_template_has_no_second_bound(vtmod, monkeypatch, nq):
    lib = base_library()[:129]
    queries = noised(lib[128], nq, 78)
    ref = reference(lib, queries)
    assert (ref[0] == 128).all()
    h = forced(vtmod, monkeypatch, lib)
    assert check(h, queries, ref, nq) == (0, nq)
    h.close()


@pytest.mark.parametrize('nq', COUNTS)
def test_every_offset_as_the_best_of_a_settled_query(vtmod, monkeypatch, nq):
    lib = base_library()
    queries = np.stack([np.roll(lib[(37 * i) % T], (i % 15) - 7, axis=0) for i in range(nq)])
    ref = reference(lib, queries)
    assert (ref[1] == 0).all() and np.array_equal(ref[0], (37 * np.arange(nq)) % T)
    h = forced(vtmod, monkeypatch, lib)
    assert check(h, queries, ref, nq) == (0, nq)
    h.close()


@pytest.mark.parametrize('nq', COUNTS)
def test_all_zero_against_all_255(vtmod, monkeypatch, nq):
    lib = base_library().copy()
    lib[10], lib[90] = 0, 255
    queries = np.empty((nq, 64, 32), dtype=np.uint8)
    queries[0::2], queries[1::2] = 255, 0
    r = reference(lib, queries[:2])
    s = settled_mask(lib, queries[:2])
    h = forced(vtmod, monkeypatch, lib)
    _, ver = check(h, queries, (np.resize(r[0], nq), np.resize(r[1], nq)), nq)
    assert ver == int(np.count_nonzero(np.resize(s, nq)))
    h.close()


# --- keys equal to the dense launch's: streams and shards -------------------------
@functools.lru_cache(maxsize=None)
def random_case():
    lib = V.synthetic_library(400, 64, 32, seed=79)
    queries, _ = V.synthetic_queries(lib, 340, seed=80, hit_frac=0.8)
    return lib, queries


@functools.lru_cache(maxsize=None)
def shard_settled(rank, nranks):
    lib, queries = random_case()
    return settled_mask(lib[rank::nranks], queries[:300])   # template g lives on rank g % nranks


@pytest.mark.parametrize('where', ['device', 'host'])
def test_match_stream_same_keys_as_the_dense_launch(vtmod, monkeypatch, where):
    from pyratslam_amd import _lib
    lib, queries = random_case()
    res, handles = [], []
    for v in ('0', 'force'):
        monkeypatch.setenv('RS_VT_PRUNE', v)
        h = vtmod.ViewTemplates._from_shape((64, 32), 45000)
        h.add(lib)
        out = []
        for nb, nq in ((3, 37), (1, 300)):         # a second call with another query count
            q = np.ascontiguousarray(queries[:nb * nq].reshape(nb, nq, 64, 32))
            if where == 'device':
                buf = _lib.DeviceBuffer(q.nbytes).upload(q)
                out.append(h.match_stream((nb, nq, buf)))
                buf.close()
            else:
                out.append(h.match_stream(q))
        res.append(out)
        handles.append(h)
    dense, pruned = handles
    assert dense.prune_stats()[3] == 0 and dense.prune_verified() == 0
    l1, l2, pairs, passes = pruned.prune_stats()
    assert (l1, pairs, passes) == (300, 7 * 300, 2)
    assert pruned.prune_verified() == int(np.count_nonzero(shard_settled(0, 1)))
    for a, b in zip(*res):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    ref = reference(lib, queries[:20])
    assert np.array_equal(res[1][1][0].ravel()[:20], ref[0]) and np.array_equal(res[1][1][1].ravel()[:20], ref[1])
    dense.close()
    pruned.close()


def test_scan_local_on_three_shards_same_keys_as_the_dense_launch(vtmod, monkeypatch):
    from pyratslam_amd import _lib
    lib, queries = random_case()
    keys = []
    for v in ('0', 'force'):
        monkeypatch.setenv('RS_VT_PRUNE', v)
        shards = [vtmod.ShardedViewTemplates.from_shape((64, 32), 45000, r, 3, reducer=lambda k: k)
                  for r in range(3)]
        per_call = []
        for nq in (300, 37):
            local = []
            for r, s in enumerate(shards):
                if not per_call:
                    s.add(lib)
                k = np.empty(nq, dtype=np.uint64)
                _lib.check(s._lib.rs_vt_scan_local(s._h, nq, _lib.ptr(np.ascontiguousarray(queries[:nq]), ctypes.c_uint8),
                                                   _lib.ptr(k, ctypes.c_uint64)))
                local.append(k)
                if v == 'force':                   # the shard's own templates: lib[r::3]
                    assert s.prune_stats()[0] == nq and s.prune_stats()[2:] == (3 * nq, 2)
                    assert s.prune_verified() == int(np.count_nonzero(shard_settled(r, 3)[:nq]))
            per_call.append(local)
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


def test_further_calls_on_one_handle_report_the_last_call_only(vtmod, monkeypatch):
    queries, ref, settled = mix_case(0.9)
    h = forced(vtmod, monkeypatch, base_library())
    for nq in (300, 4, 37):
        l2, ver = check(h, queries, ref, nq)
        assert ver == int(np.count_nonzero(settled[:nq]))
        assert l2 == (NTB - 1) * int(np.count_nonzero(ref[1][:nq] > 45000))
        assert h.prune_verified() == ver and h.prune_stats() == (nq, l2, NTB * nq, 2)   # read twice: unchanged
    h.close()
