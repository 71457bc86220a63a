"""The pruned plane scan's front in one launch (vt_front_kernel): a thread block walks every
template block for its groups of four queries, sixteen blocks to a chunk, folds each chunk's
bounds into the queries' picks and verifies in its tail.  Index and score against the
oracle, bit for bit, and prune_stats() / prune_verified() against the NumPy restatement of
the rule (test_prune_subunit_bound.pruned_per_query), with RS_VT_PRUNE=force, on

  * 130 templates: 3 template blocks, so waves 1-3 of a thread block hold no template block
    but still own a query; fused by the rule (RS_VT_FRONT unset);
  * 1,030 templates: 17 blocks, a second chunk with one live block of six templates; fused
    with RS_VT_FRONT=force (the rule keeps two launches beyond sixteen blocks),

at 1, 3, 4, 5, 37 and 300 queries (partial groups).  One library and one set of 300 queries
per size hold every case side by side, so the oracle's score matrix is computed once per
size; a test takes its case's queries, repeated up to the query count."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import view_templates as V
from test_prune_bound import PF_UNITS, boundary_pair
from test_prune_subunit_bound import PF_COLS, pruned_per_query
from test_prune_verify_rule import score_matrix

pytestmark = pytest.mark.gpu

COUNTS = [1, 3, 4, 5, 37, 300]
NQ = 300
LIBS = [pytest.param(130, None, id='130-rule'), pytest.param(1030, 'force', id='1030-force')]
THR = 45000
# templates the cases plant: twins, decoys, the boundary pair, all-0 and all-255
SPECIAL = {5, 40, 9, 70, 128, 129, 12, 100, 20, 30, 10, 90}


@pytest.fixture(scope='module')
def vtmod():
    from pyratslam_amd import _build
    _build.build()
    import pyratslam_amd.view_templates as m
    return m


def noised(t, n, seed):
    rng = np.random.default_rng(seed)
    return np.clip(t.astype(np.int16)[None] - rng.integers(0, 4, size=(n, 64, 32)), 0, 255).astype(np.uint8)


class World:
    """The library of t templates, the 300 queries, the cases' query indices, the oracle's
    answers and the rule's (settled by verification, blocks of pass B2) per query."""

    def __init__(self, t):
        rng = np.random.default_rng(700 + t)
        lib = V.synthetic_library(t, 64, 32, seed=71).copy()
        self.ntb = (t + 63) // 64
        qb = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)     # the boundary case's query
        lib[40] = lib[5]                                             # twin in the same block
        lib[70] = lib[9]                                             # twin in another block
        lib[128] = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
        lib[128, 16:48] = lib[129, 16:48]                            # decoy at lane 0 of the match block
        lib[12] = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
        lib[12, 16:48] = lib[100, 16:48]                             # decoy in a lower block
        lib[20], lib[30] = boundary_pair(qb, units=PF_UNITS)         # min2 == U0
        lib[10], lib[90] = 0, 255
        plain = [i for i in ((t - 3 - 37 * k) % t for k in range(200)) if i not in SPECIAL]
        last = [i for i in range(t - 3, 0, -1) if i not in SPECIAL]  # from the last block down
        parts, self.seg = [], {}

        def put(name, q):
            at = sum(len(p) for p in parts)
            parts.append(np.asarray(q, dtype=np.uint8))
            self.seg[name] = np.arange(at, at + len(q))

        hits, src = V.synthetic_queries(lib, 80, seed=72, hit_frac=1.0)
        hits = hits[~np.isin(src, list(SPECIAL))][:40]               # (a planted template's hit is its case's)
        assert len(hits) == 40
        tail_hits = np.concatenate([noised(np.roll(lib[last[k]], (k % 15) - 7, axis=0), 1, 800 + k) for k in range(20)])
        put('hits', np.concatenate([hits, tail_hits]))
        put('misses', rng.integers(0, 256, size=(40, 64, 32), dtype=np.uint8))
        put('twin_same_block', noised(lib[5], 20, 73))
        put('twin_other_block', noised(lib[9], 20, 74))
        put('decoy_same_block', noised(lib[129], 20, 75))
        put('decoy_lower_block', noised(lib[100], 20, 76))
        put('boundary', np.repeat(qb[None], 10, axis=0))
        put('offsets_settled', np.stack([np.roll(lib[plain[k]], (k % 15) - 7, axis=0) for k in range(30)]))
        put('offsets_unsettled', np.concatenate([noised(np.roll(lib[129], o, axis=0), 1, 900 + o)
                                                 for o in range(-7, 8)]))
        extremes = np.empty((10, 64, 32), dtype=np.uint8)
        extremes[0::2], extremes[1::2] = 0, 255
        put('extremes', extremes)
        mix, _ = V.synthetic_queries(lib, NQ - sum(len(p) for p in parts), seed=77, hit_frac=0.5)
        put('mix', mix)
        self.lib, self.queries = lib, np.concatenate(parts)
        assert len(self.queries) == NQ
        self.lib.setflags(write=False)
        self.queries.setflags(write=False)
        self.plain, self.last = plain, last
        sc = score_matrix(lib, self.queries)
        self.sc = sc
        self.idx, self.score = sc.argmin(axis=1), sc.min(axis=1).astype(np.uint64)
        self.settled, self.b2 = pruned_per_query(lib, self.queries, PF_COLS, scores=sc)


@functools.lru_cache(maxsize=None)
def world(t):
    return World(t)


def make(vtmod, monkeypatch, lib, front, prune='force'):
    monkeypatch.setenv('RS_VT_PRUNE', prune)
    if front is None:
        monkeypatch.delenv('RS_VT_FRONT', raising=False)
    else:
        monkeypatch.setenv('RS_VT_FRONT', front)
    h = vtmod.ViewTemplates._from_shape((64, 32), THR)
    h.add(lib)
    return h


def check(h, w, sel):
    """One frozen call over queries w.queries[sel]: answers, stats and the verified count, read twice."""
    nq = len(sel)
    idx, score, _ = h.match_templates(w.queries[sel], mode=0)
    print('nq %d: verified %d of rule %d, B2 pairs %d of rule %d' % (
        nq, h.prune_verified(), int(w.settled[sel].sum()), h.prune_stats()[1], int(w.b2[sel].sum())))
    assert np.array_equal(score, w.score[sel])
    assert np.array_equal(idx, w.idx[sel])
    for _ in range(2):
        assert h.prune_stats() == (nq, int(w.b2[sel].sum()), w.ntb * nq, 2)
        assert h.prune_verified() == int(w.settled[sel].sum())


# --- what each case is there for, stated on the oracle's side (no GPU) --------------
@pytest.mark.parametrize('t', [130, 1030])
def test_the_cases_are_what_they_claim(t):
    w = world(t)
    s = w.seg
    assert w.settled[s['hits']].all() and (w.score[s['hits']] <= THR).all()
    assert (w.idx[s['hits']][40:] == np.array(w.last[:20])).all()          # ... the last block's among them
    # (1,030: templates of block 16, the second chunk; 130: its last block holds the decoy pair only)
    assert t == 130 or (np.array(w.last[:4]) // 64 == w.ntb - 1).all()
    assert not w.settled[s['misses']].any() and (w.b2[s['misses']] == w.ntb - 1).all()
    assert (w.idx[s['twin_same_block']] == 5).all() and not w.settled[s['twin_same_block']].any()
    assert (w.idx[s['twin_other_block']] == 9).all() and w.settled[s['twin_other_block']].all()
    assert (w.b2[s['twin_other_block']] >= 1).all()
    assert (w.idx[s['decoy_same_block']] == 129).all() and not w.settled[s['decoy_same_block']].any()
    assert (w.idx[s['decoy_lower_block']] == 100).all() and not w.settled[s['decoy_lower_block']].any()
    assert (w.b2[s['decoy_lower_block']] >= 1).all()
    assert (w.idx[s['boundary']] == 20).all() and (w.score[s['boundary']] == 40).all()
    assert int(w.sc[s['boundary'][0], 30]) == 40 and not w.settled[s['boundary']].any()
    assert (w.score[s['offsets_settled']] == 0).all() and w.settled[s['offsets_settled']].all()
    assert (w.idx[s['offsets_settled']] == np.array(w.plain[:30])).all()
    assert (w.idx[s['offsets_unsettled']] == 129).all() and not w.settled[s['offsets_unsettled']].any()
    for q in np.concatenate([s['offsets_settled'], s['offsets_unsettled']]):  # the unique best
        assert np.count_nonzero(w.sc[q] == w.sc[q].min()) == 1
    for k, o in enumerate(range(-7, 8)):                                     # ... at the offset meant
        q = w.queries[s['offsets_unsettled'][k]]
        per_offset = [int(np.sum((w.lib[129][8 + d:56 + d] - q[8:56]).astype(np.uint8), dtype=np.uint64))
                      for d in range(-7, 8)]
        assert int(np.argmin(per_offset)) - 7 == -o and per_offset.count(min(per_offset)) == 1


CASES = ['hits', 'misses', 'twin_same_block', 'twin_other_block', 'decoy_same_block', 'decoy_lower_block',
         'boundary', 'offsets_settled', 'offsets_unsettled', 'extremes', 'mix']


@pytest.mark.parametrize('nq', COUNTS)
@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('t, front', LIBS)
def test_case_at_every_count(vtmod, monkeypatch, t, front, case, nq):
    w = world(t)
    h = make(vtmod, monkeypatch, w.lib, front)
    assert h.scan_form() == 'plane-pruned'
    check(h, w, np.resize(w.seg[case], nq))
    h.close()


@pytest.mark.parametrize('nq', COUNTS)
@pytest.mark.parametrize('t, front', LIBS)
def test_all_cases_side_by_side(vtmod, monkeypatch, t, front, nq):
    w = world(t)
    h = make(vtmod, monkeypatch, w.lib, front)
    check(h, w, np.random.default_rng(nq).permutation(NQ)[:nq])
    h.close()


@pytest.mark.parametrize('t, front', LIBS)
def test_all_zero_queries_against_an_all_255_library(vtmod, monkeypatch, t, front):
    """Every template equal: every bound ties, the lowest block and lane are picked, min2 == min1
    <= U0 settles nothing, and index 0 wins."""
    lib = np.full((t, 64, 32), 255, dtype=np.uint8)
    q = np.zeros((1, 64, 32), dtype=np.uint8)
    s = V.vt_scores_library(lib, q[0])
    assert int(np.argmin(s)) == 0 and (s == s[0]).all()
    h = make(vtmod, monkeypatch, lib, front)
    ntb = (t + 63) // 64
    for nq in (5, 300):
        idx, score, _ = h.match_templates(np.repeat(q, nq, axis=0), mode=0)
        assert (idx == 0).all() and (score == s[0]).all()
        assert h.prune_verified() == 0 and h.prune_stats() == (nq, (ntb - 1) * nq, ntb * nq, 2)
    h.close()


@pytest.mark.parametrize('t, front', LIBS)
def test_all_misses_then_hits_in_the_same_slots(vtmod, monkeypatch, t, front):
    """Every query expanded, then settled ones and unsettled ones in the same slots, then misses
    again: planes left by the call before cannot stand in for an expansion that is missing."""
    w = world(t)
    h = make(vtmod, monkeypatch, w.lib, front)
    unsettled = np.concatenate([w.seg['decoy_lower_block'], w.seg['twin_same_block'], w.seg['offsets_unsettled']])
    for name_sel in (w.seg['misses'], w.seg['hits'], unsettled, w.seg['misses'], w.seg['mix']):
        check(h, w, np.resize(name_sel, 37))
    h.close()


@pytest.mark.parametrize('nq', [5, 300])
@pytest.mark.parametrize('t', [130, 1030])
def test_two_launches_and_one_give_the_same(vtmod, monkeypatch, t, nq):
    w = world(t)
    sel = np.random.default_rng(5 * nq).permutation(NQ)[:nq]
    res = []
    for front in ('0', 'force'):
        h = make(vtmod, monkeypatch, w.lib, front)
        idx, score, new = h.match_templates(w.queries[sel], mode=0)
        res.append((idx, score, new, h.prune_stats(), h.prune_verified()))
        check(h, w, sel)
        h.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('where', ['device', 'host'])
@pytest.mark.parametrize('t, front', LIBS)
def test_match_stream(vtmod, monkeypatch, t, front, where):
    from pyratslam_amd import _lib
    w = world(t)
    h = make(vtmod, monkeypatch, w.lib, front)
    for nb, nq in ((3, 37), (1, 300), (2, 5)):         # further calls with other query counts
        q = np.ascontiguousarray(w.queries[:nb * nq].reshape(nb, nq, 64, 32))
        if where == 'device':
            buf = _lib.DeviceBuffer(q.nbytes).upload(q)
            idx, score = h.match_stream((nb, nq, buf))
            buf.close()
        else:
            idx, score = h.match_stream(q)
        assert np.array_equal(idx.ravel(), w.idx[:nb * nq]) and np.array_equal(score.ravel(), w.score[:nb * nq])
        if nb == 1:                                     # (host batches go in groups: the last group's stats)
            assert h.prune_stats() == (nq, int(w.b2[:nq].sum()), w.ntb * nq, 2)
            assert h.prune_verified() == int(w.settled[:nq].sum())
    h.close()


@pytest.mark.parametrize('t, front', LIBS)
def test_scan_local_on_three_shards_then_resolve(vtmod, monkeypatch, t, front):
    from pyratslam_amd import _lib
    w = world(t)
    monkeypatch.setenv('RS_VT_PRUNE', 'force')
    if front is None:
        monkeypatch.delenv('RS_VT_FRONT', raising=False)
    else:
        monkeypatch.setenv('RS_VT_FRONT', front)
    shards = [vtmod.ShardedViewTemplates.from_shape((64, 32), THR, r, 3, reducer=lambda k: k) for r in range(3)]
    for s in shards:
        s.add(w.lib)
    for nq in (300, 37):
        q = np.ascontiguousarray(w.queries[:nq])
        local = []
        for r, s in enumerate(shards):
            k = np.empty(nq, dtype=np.uint64)
            _lib.check(s._lib.rs_vt_scan_local(s._h, nq, _lib.ptr(q, ctypes.c_uint8), _lib.ptr(k, ctypes.c_uint64)))
            local.append(k)
            mine = w.lib[r::3]                                   # template g lives on rank g % 3
            settled, b2 = pruned_per_query(mine, q, PF_COLS, scores=w.sc[:nq, r::3])
            assert s.prune_stats() == (nq, int(b2.sum()), ((len(mine) + 63) // 64) * nq, 2)
            assert s.prune_verified() == int(settled.sum())
        glob = np.minimum.reduce(local)
        assert np.array_equal((glob & 0xFFFFFFFF).astype(np.int64), w.idx[:nq])
        assert np.array_equal(glob >> 32, w.score[:nq])
        for s in shards:
            idx, score = np.empty(nq, dtype=np.int64), np.empty(nq, dtype=np.uint64)
            new = np.zeros(nq, dtype=np.uint8)
            _lib.check(s._lib.rs_vt_resolve(s._h, nq, _lib.ptr(glob, ctypes.c_uint64), 0,
                                            _lib.ptr(score, ctypes.c_uint64), _lib.ptr(idx, ctypes.c_int64),
                                            _lib.ptr(new, ctypes.c_uint8)))
            assert np.array_equal(idx, w.idx[:nq]) and np.array_equal(score, w.score[:nq])
    for s in shards:
        s.close()


def test_a_thread_block_serving_two_query_groups(vtmod, monkeypatch):
    """16,388 queries are 4,097 groups for a grid capped at 4,096 thread blocks: the first block
    serves a second group.  Keys equal to the dense launch's (and, the queries being the 300
    of the other tests drawn again and again, to the oracle's)."""
    w = world(130)
    sel = np.random.default_rng(16388).integers(0, NQ, size=16388)
    q = w.queries[sel]
    dense = make(vtmod, monkeypatch, w.lib, None, prune='0')
    di, ds, _ = dense.match_templates(q, mode=0)
    assert dense.prune_stats()[3] == 0
    dense.close()
    h = make(vtmod, monkeypatch, w.lib, None)
    idx, score, _ = h.match_templates(q, mode=0)
    assert np.array_equal(idx, di) and np.array_equal(score, ds)
    assert np.array_equal(idx, w.idx[sel]) and np.array_equal(score, w.score[sel])
    assert h.prune_stats() == (16388, int(w.b2[sel].sum()), 3 * 16388, 2)
    assert h.prune_verified() == int(w.settled[sel].sum())
    h.close()


# --- other readers of the staged forms around a pruned call: a build ahead of a pruned scan
# is compact, so a matrix scan expands the planes first
@pytest.mark.parametrize('t, front', LIBS)
def test_score_matrix_right_after_staging(vtmod, monkeypatch, t, front):
    w = world(t)
    h = make(vtmod, monkeypatch, w.lib, front)
    for nq in (5, 300, 37):
        sel = np.random.default_rng(11 * nq).permutation(NQ)[:nq]
        m = h.scores(w.queries[sel], t0=64, nt=64)             # template block 1
        assert np.array_equal(np.asarray(m, dtype=np.int64), w.sc[sel][:, 64:128])
        check(h, w, sel)                                       # ... and a pruned call behind it
    h.close()


@pytest.mark.parametrize('t, front', LIBS)
def test_sequential_call_with_novel_queries(vtmod, monkeypatch, t, front):
    """Misses become templates in order (a candidate matrix scan reads the forms behind the pruned
    scan of the same staging); the same calls on a dense handle are the reference."""
    w = world(t)
    sel = np.concatenate([w.seg['misses'][:9], w.seg['hits'][:9], w.seg['misses'][:9], w.seg['mix'][:10]])
    later = np.random.default_rng(3).permutation(NQ)[:37]
    res = []
    for prune, f in (('0', None), ('force', front)):
        h = make(vtmod, monkeypatch, w.lib, f, prune=prune)
        a = h.match_templates(w.queries[sel])                  # SEQUENTIAL
        b = h.match_templates(w.queries[later], mode=0)
        res.append((a, b, len(h)))
        h.close()
    (da, db, dn), (pa, pb, pn) = res
    assert dn == pn and dn > t and da[2].any()
    for x, y in zip(da + db, pa + pb):
        assert np.array_equal(x, y)
