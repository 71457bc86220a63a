"""The pruned plane scan with the prefilter's bound taken over half a template unit
(columns 0..15 of rows 28..31) and four template blocks per wave: index and score against
the oracle, bit for bit, with RS_VT_PRUNE=force, at 1, 4, 37 and 300 queries against
libraries of 130 templates (blocks of 64, 64 and 2), 258 (5 blocks: a wave with one live
block of its four) and, at 4 and 37 queries, 1,030 (17 blocks: a second thread block in x
whose single live wave holds one block).  prune_verified() and the pairs of pass B2 are
counted against the NumPy restatement of the sub-unit bound (test_prune_subunit_bound)."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import view_templates as V
from test_prune_subunit_bound import PF_COLS, pruned_per_query, sub_min_bounds
from test_prune_verify_rule import score_matrix

pytestmark = pytest.mark.gpu

SHAPES = [(t, nq) for t in (130, 258) for nq in (1, 4, 37, 300)] + [(1030, 4), (1030, 37)]
NQ_MAX = {130: 300, 258: 300, 1030: 37}


@pytest.fixture(scope='module')
def vtmod():
    from pyratslam_amd import _build
    _build.build()
    import pyratslam_amd.view_templates as m
    return m


@functools.lru_cache(maxsize=None)
def base_library(t):
    lib = V.synthetic_library(t, 64, 32, seed=91)
    lib.setflags(write=False)
    return lib


class Case:
    """A library, its queries, the oracle's answers and the restatement's per-query counts."""

    def __init__(self, lib, queries):
        self.lib, self.queries = lib, queries
        sc = score_matrix(lib, queries)
        self.idx, self.score = sc.argmin(axis=1), sc.min(axis=1)
        self.settled, self.b2 = pruned_per_query(lib, queries, PF_COLS, scores=sc)
        self.ntb = (len(lib) + 63) // 64


def noised(t, n, seed, cols=slice(None)):
    """n copies of template t, each pixel of the columns `cols` lowered by 0..3."""
    rng = np.random.default_rng(seed)
    q = np.repeat(t[None], n, axis=0).astype(np.int16)
    q[:, :, cols] -= rng.integers(0, 4, size=q[:, :, cols].shape)
    return np.clip(q, 0, 255).astype(np.uint8)


def forced(vtmod, monkeypatch, lib):
    monkeypatch.setenv('RS_VT_PRUNE', 'force')
    h = vtmod.ViewTemplates._from_shape((64, 32), 45000)
    assert h.scan_form() == 'plane-pruned'
    h.add(lib)
    return h


def check(vtmod, monkeypatch, case, nq):
    h = forced(vtmod, monkeypatch, case.lib)
    idx, score, _ = h.match_templates(case.queries[:nq], mode=0)
    assert np.array_equal(score, case.score[:nq])
    assert np.array_equal(idx, case.idx[:nq])
    l1, l2, pairs, passes = h.prune_stats()
    assert (l1, pairs, passes) == (nq, case.ntb * nq, 2)
    ver = h.prune_verified()
    h.close()
    assert ver == int(np.count_nonzero(case.settled[:nq]))
    assert l2 == int(case.b2[:nq].sum())
    return l2, ver


@functools.lru_cache(maxsize=None)
def mix_case(t, hit_frac):
    lib = base_library(t)
    queries, _ = V.synthetic_queries(lib, NQ_MAX[t], seed=92 + int(10 * hit_frac), hit_frac=hit_frac)
    return Case(lib, queries)


@pytest.mark.parametrize('hit_frac', [1.0, 0.0, 0.9])
@pytest.mark.parametrize('t,nq', SHAPES)
def test_hits_misses_and_mixes(vtmod, monkeypatch, t, nq, hit_frac):
    case = mix_case(t, hit_frac)
    l2, ver = check(vtmod, monkeypatch, case, nq)
    if hit_frac == 0.0:
        assert ver == 0 and l2 == (case.ntb - 1) * nq      # a miss is scanned against every block


@functools.lru_cache(maxsize=None)
def side_noise_decoy_case(t):
    """Queries = the last template with noise in columns 16..31 only; template 3 (block 0)
    equals it on columns 0..15 of rows 16..47: both bounds are 0, block 0 is the candidate,
    its verification fails (the decoy's score is large), and pass B2 finds the match."""
    rng = np.random.default_rng(93)
    lib = base_library(t).copy()
    lib[3] = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
    lib[3, 16:48, :PF_COLS] = lib[t - 1, 16:48, :PF_COLS]
    case = Case(lib, noised(lib[t - 1], NQ_MAX[t], 94, cols=slice(PF_COLS, 32)))
    bounds = sub_min_bounds(lib, case.queries[:4])
    assert (bounds[:, 3] == 0).all() and (bounds[:, t - 1] == 0).all()
    assert (case.idx == t - 1).all() and (case.score > 0).all() and not case.settled.any()
    assert (case.b2 >= 1).all()
    return case


@pytest.mark.parametrize('t,nq', SHAPES)
def test_noise_beside_the_sub_unit_and_a_decoy_in_a_lower_block(vtmod, monkeypatch, t, nq):
    assert check(vtmod, monkeypatch, side_noise_decoy_case(t), nq)[1] == 0


@functools.lru_cache(maxsize=None)
def equal_on_the_sub_unit_case(t):
    """Templates a < b of the last whole block: b is a with 4 x 5 added in columns 20..23 of
    row 29 (the unit's rows, beside the sub-unit), a has them in row 10: equal bounds and
    equal scores for queries made from the unchanged template."""
    lib = base_library(t).copy()
    a = 64 * ((t // 64) - 1) + 7
    b = a + 30
    orig = lib[a].copy()
    lib[b] = orig
    lib[a, 10, 20:24] += 5                                  # uint8: wraps, (T - Q) mod 256 grows by 5
    lib[b, 29, 20:24] += 5
    case = Case(lib, noised(orig, NQ_MAX[t], 95))
    bounds = sub_min_bounds(lib, case.queries[:4])
    assert np.array_equal(bounds[:, a], bounds[:, b])
    assert (case.idx == a).all() and not case.settled.any()
    assert V.vt_score(lib[b], case.queries[0]) == case.score[0]
    return case


@pytest.mark.parametrize('t,nq', SHAPES)
def test_templates_equal_on_the_sub_unit_lower_index_wins(vtmod, monkeypatch, t, nq):
    assert check(vtmod, monkeypatch, equal_on_the_sub_unit_case(t), nq)[1] == 0


# --- keys equal to the dense launch's: streams and shards -------------------------
@functools.lru_cache(maxsize=None)
def random_case():
    lib = V.synthetic_library(258, 64, 32, seed=96)
    queries, _ = V.synthetic_queries(lib, 340, seed=97, hit_frac=0.8)
    return lib, queries


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
    assert dense.prune_stats()[3] == 0
    settled, b2 = pruned_per_query(lib, queries[:300])
    assert pruned.prune_stats() == (300, int(b2.sum()), 5 * 300, 2)
    assert pruned.prune_verified() == int(np.count_nonzero(settled))
    for a, b in zip(*res):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    sc = score_matrix(lib, queries[:20])
    assert np.array_equal(res[1][1][0].ravel()[:20], sc.argmin(axis=1))
    assert np.array_equal(res[1][1][1].ravel()[:20], sc.min(axis=1))
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
                if v == 'force':                   # the shard's own templates: lib[r::3], two blocks
                    settled, b2 = pruned_per_query(lib[r::3], queries[:nq])
                    assert s.prune_stats() == (nq, int(b2.sum()), 2 * nq, 2)
                    assert s.prune_verified() == int(np.count_nonzero(settled))
            per_call.append(local)
        keys.append(per_call)
        for s in shards:
            s.close()
    for a, b in zip(*keys):
        for ka, kb in zip(a, b):
            assert np.array_equal(ka, kb)
    glob = np.minimum.reduce(keys[1][0])
    sc = score_matrix(lib, queries[:20])
    assert np.array_equal((glob & 0xFFFFFFFF)[:20].astype(np.int64), sc.argmin(axis=1))
    assert np.array_equal((glob >> 32)[:20], sc.min(axis=1))
