"""The pruned plane scan with ONE list pass (RS_VT_PASSES=1, the default): the
verification writes a query into the list of every template block it must be scanned against,
on its own score U0, and vt_scan_plane_kernel<64, false, true> runs once.  Against the two-pass
chain (RS_VT_PASSES=2) and the oracle, with RS_VT_PRUNE=force:

  * keys (index and score) equal the oracle's, bit for bit, in both modes;
  * prune_stats() and prune_verified() are the two-pass rule's counts in both modes, read twice,
    and equal the NumPy rule (test_prune_subunit_bound.pruned_per_query);
  * prune_scanned() equals the NumPy one-pass list size (test_single_pass_rule.rules), is at
    least the rule's pairs plus the unsettled queries, and strictly more for a decoy at lane 0
    of the match's block; with two passes it is exactly the rule's pairs plus the unsettled.

An equal score at a lower index in a block other than tb* whose bound equals U(q) has a library
of its own (test_single_pass_rule.Cross).  Libraries of 130 templates (3 blocks, the fused front) and 1,030 (17 blocks) with RS_VT_FRONT=0
(prefilter and verify kernels) and =force (the fused front's second chunk), at 1, 3, 4, 5, 37 and
300 queries.  The library, the queries and the oracle's matrix are test_plane_front_gpu's (one
per size); a pair of handles per library serves every test, so calls of different query counts
follow one another on one handle and the counters' parity flips all the way through."""
import ctypes
import os

import numpy as np
import pytest

from oracle import view_templates as V
from test_plane_front_gpu import CASES, COUNTS, NQ, THR, world
from test_prune_subunit_bound import PF_COLS, pruned_per_query, sub_min_bounds
from test_single_pass_rule import cross, rules

pytestmark = pytest.mark.gpu

LIBS = [pytest.param(130, None, id='130-rule'), pytest.param(1030, '0', id='1030-two-launches'),
        pytest.param(1030, 'force', id='1030-force')]
ENV = ('RS_VT_PRUNE', 'RS_VT_FRONT', 'RS_VT_PASSES')


def create(vtmod, lib, front, passes, prune='force', sharded=None):
    """A handle made under RS_VT_PRUNE / _FRONT / _PASSES (read at create), the environment put back."""
    old = {k: os.environ.get(k) for k in ENV}
    new = {'RS_VT_PRUNE': prune, 'RS_VT_FRONT': front, 'RS_VT_PASSES': passes}
    try:
        for k, v in new.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        if sharded is None:
            h = vtmod.ViewTemplates._from_shape((64, 32), THR)
        else:
            h = vtmod.ShardedViewTemplates.from_shape((64, 32), THR, sharded, 3, reducer=lambda k: k)
        h.add(lib)
        return h
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@pytest.fixture(scope='module')
def vtmod():
    from pyratslam_amd import _build
    _build.build()
    import pyratslam_amd.view_templates as m
    return m


@pytest.fixture(scope='module')
def pairs(vtmod):
    """(t, front) -> (one-pass handle, two-pass handle), made on first use."""
    made = {}

    def get(t, front):
        if (t, front) not in made:
            made[t, front] = (create(vtmod, world(t).lib, front, None), create(vtmod, world(t).lib, front, '2'))
        return made[t, front]

    yield get
    for one, two in made.values():
        one.close()
        two.close()


_rules = {}


def rule_of(t):
    if t not in _rules:
        w = world(t)
        _rules[t] = rules(sub_min_bounds(w.lib, w.queries, PF_COLS), w.sc)
    return _rules[t]


def check_both(hs, w, rs, sel, strictly_more=False):
    """One frozen call over w.queries[sel] on the one-pass and on the two-pass handle."""
    nq = len(sel)
    one = sum(len(rs[q].one) for q in sel)
    two = sum(len(rs[q].two) for q in sel)
    want = ((nq, int(w.b2[sel].sum()), w.ntb * nq, 2), int(w.settled[sel].sum()))
    assert two == want[0][1] + nq - want[1]             # the rule's pairs plus the unsettled queries
    got = []
    for h, scanned in zip(hs, (one, two)):
        idx, score, _ = h.match_templates(w.queries[sel], mode=0)
        assert np.array_equal(score, w.score[sel]) and np.array_equal(idx, w.idx[sel])
        for _ in range(2):
            assert (h.prune_stats(), h.prune_verified()) == want
            assert h.prune_scanned() == scanned
        got.append((idx, score))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    print('nq %d: scanned %d with one pass, %d with two' % (nq, one, two))
    assert one >= two and (one > two or not strictly_more)


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('t, front', LIBS)
def test_case_at_every_count(pairs, t, front, case):
    w, rs = world(t), rule_of(t)
    for nq in COUNTS:
        check_both(pairs(t, front), w, rs, np.resize(w.seg[case], nq), strictly_more=case == 'decoy_same_block')


@pytest.mark.parametrize('t, front', LIBS)
def test_equal_score_at_a_lower_index_in_another_block_whose_bound_equals_u(vtmod, t, front):
    """test_single_pass_rule.Cross: X in block 0 with bound = score = 40, Y in a higher block (the
    last one of 1,030 templates: the verify kernel's stride, the fused front's second chunk) with
    bound 0 and score 40, so U0 = U = 40 equals block 0's bound; once settled by the verification,
    once unsettled (Y has a twin).  Only the "<=" of the append and of the counting kernel finds X:
    keys, statistics and pairs scanned, one pass against two, at every query count, the two
    queries alone, alternating, and among misses and hits."""
    c = cross(t)
    hs = (create(vtmod, c.lib, front, None), create(vtmod, c.lib, front, '2'))
    for nq in COUNTS:
        for pick in ([0], [1], [0, 1], list(range(len(c.queries)))):
            sel = np.resize(np.array(pick), nq)
            check_both(hs, c, c.rules, sel)
            assert (c.idx[sel][sel == 0] == c.xa).all() and (c.idx[sel][sel == 1] == c.xb).all()
    for h in hs:
        h.close()


@pytest.mark.parametrize('t, front', LIBS)
def test_all_cases_side_by_side(pairs, t, front):
    w, rs = world(t), rule_of(t)
    for nq in COUNTS:
        check_both(pairs(t, front), w, rs, np.random.default_rng(nq).permutation(NQ)[:nq], strictly_more=nq == 300)


@pytest.mark.parametrize('t, front', LIBS)
def test_misses_then_hits_then_unsettled_then_misses_in_the_same_slots(pairs, t, front):
    w, rs = world(t), rule_of(t)
    unsettled = np.concatenate([w.seg['decoy_lower_block'], w.seg['twin_same_block'], w.seg['offsets_unsettled']])
    for sel in (w.seg['misses'], w.seg['hits'], unsettled, w.seg['misses'], w.seg['mix']):
        check_both(pairs(t, front), w, rs, np.resize(sel, 37))


@pytest.mark.parametrize('t, front', LIBS)
def test_query_counts_in_turn_with_a_dense_call_between(pairs, t, front):
    """The parity flips from call to call; a matrix scan (a dense launch, from template block 1)
    between two pruned calls touches neither the counters nor the statistics."""
    w, rs = world(t), rule_of(t)
    hs = pairs(t, front)
    for i, nq in enumerate((300, 1, 37, 5, 300, 4, 3, 37)):
        sel = np.random.default_rng(40 + i).permutation(NQ)[:nq]
        check_both(hs, w, rs, sel)
        if i % 2 == 0:
            for h in hs:
                before = (h.prune_stats(), h.prune_verified(), h.prune_scanned())
                k = min(nq, 5)
                m = h.scores(w.queries[sel[:k]], t0=64, nt=64)
                assert np.array_equal(np.asarray(m, dtype=np.int64), w.sc[sel[:k]][:, 64:128])
                assert (h.prune_stats(), h.prune_verified(), h.prune_scanned()) == before


@pytest.mark.parametrize('t, front', LIBS)
def test_all_zero_queries_against_an_all_255_library(vtmod, t, front):
    """Every bound ties: nothing settles, every block is listed in both modes, index 0 wins."""
    lib = np.full((t, 64, 32), 255, dtype=np.uint8)
    q = np.zeros((1, 64, 32), dtype=np.uint8)
    s = V.vt_scores_library(lib, q[0])
    ntb = (t + 63) // 64
    for passes in (None, '2'):
        h = create(vtmod, lib, front, passes)
        for nq in (5, 300):
            idx, score, _ = h.match_templates(np.repeat(q, nq, axis=0), mode=0)
            assert (idx == 0).all() and (score == s[0]).all()
            assert h.prune_verified() == 0 and h.prune_stats() == (nq, (ntb - 1) * nq, ntb * nq, 2)
            assert h.prune_scanned() == ntb * nq
        h.close()


@pytest.mark.parametrize('where', ['device', 'host'])
@pytest.mark.parametrize('t, front', LIBS)
def test_match_stream(pairs, t, front, where):
    from pyratslam_amd import _lib
    w, rs = world(t), rule_of(t)
    for h, field in zip(pairs(t, front), ('one', 'two')):
        for nb, nq in ((3, 37), (1, 300), (2, 5)):
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
                assert h.prune_scanned() == sum(len(getattr(r, field)) for r in rs[:nq])


@pytest.mark.parametrize('t, front', LIBS)
def test_scan_local_on_three_shards_then_resolve(vtmod, t, front):
    from pyratslam_amd import _lib
    w = world(t)
    nq = 37
    q = np.ascontiguousarray(w.queries[:nq])
    keys = []
    for passes, field in ((None, 'one'), ('2', 'two')):
        shards = [create(vtmod, w.lib, front, passes, sharded=r) for r in range(3)]
        local = []
        for r, s in enumerate(shards):
            k = np.empty(nq, dtype=np.uint64)
            _lib.check(s._lib.rs_vt_scan_local(s._h, nq, _lib.ptr(q, ctypes.c_uint8), _lib.ptr(k, ctypes.c_uint64)))
            local.append(k)
            mine, sc = w.lib[r::3], w.sc[:nq, r::3]              # template g lives on rank g % 3
            settled, b2 = pruned_per_query(mine, q, PF_COLS, scores=sc)
            assert s.prune_stats() == (nq, int(b2.sum()), ((len(mine) + 63) // 64) * nq, 2)
            assert s.prune_verified() == int(settled.sum())
            assert s.prune_scanned() == sum(len(getattr(x, field)) for x in rules(sub_min_bounds(mine, q, PF_COLS), sc))
        glob = np.minimum.reduce(local)
        assert np.array_equal((glob & 0xFFFFFFFF).astype(np.int64), w.idx[:nq]) and np.array_equal(glob >> 32, w.score[:nq])
        s = shards[0]
        idx, score, new = np.empty(nq, dtype=np.int64), np.empty(nq, dtype=np.uint64), np.zeros(nq, dtype=np.uint8)
        _lib.check(s._lib.rs_vt_resolve(s._h, nq, _lib.ptr(glob, ctypes.c_uint64), 0, _lib.ptr(score, ctypes.c_uint64),
                                        _lib.ptr(idx, ctypes.c_int64), _lib.ptr(new, ctypes.c_uint8)))
        assert np.array_equal(idx, w.idx[:nq]) and np.array_equal(score, w.score[:nq])
        keys.append(local)
        for s in shards:
            s.close()
    for a, b in zip(*keys):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('t, front', LIBS)
def test_sequential_call_right_behind_a_staging(vtmod, t, front):
    """Misses become templates in order (a candidate matrix scan reads the forms behind the pruned
    scan of the same staging): one pass, two passes and the dense handle agree."""
    w = world(t)
    sel = np.concatenate([w.seg['misses'][:9], w.seg['hits'][:9], w.seg['misses'][:9], w.seg['mix'][:10]])
    later = np.random.default_rng(3).permutation(NQ)[:37]
    res = []
    for prune, passes in (('0', None), ('force', None), ('force', '2')):
        h = create(vtmod, w.lib, front, passes, prune=prune)
        a = h.match_templates(w.queries[sel])                  # SEQUENTIAL
        b = h.match_templates(w.queries[later], mode=0)
        res.append((a + b, len(h)))
        h.close()
    assert res[0][1] == res[1][1] == res[2][1] > t
    for other in res[1:]:
        for x, y in zip(res[0][0], other[0]):
            assert np.array_equal(x, y)


def test_a_thread_block_serving_two_query_groups(vtmod):
    """16,388 queries are 4,097 groups for a grid capped at 4,096 thread blocks: the first block
    serves a second group, and appends for it."""
    w, rs = world(130), rule_of(130)
    sel = np.random.default_rng(16388).integers(0, NQ, size=16388)
    one = int(np.array([len(r.one) for r in rs])[sel].sum())
    two = int(np.array([len(r.two) for r in rs])[sel].sum())
    for passes, scanned in ((None, one), ('2', two)):
        h = create(vtmod, w.lib, None, passes)
        idx, score, _ = h.match_templates(w.queries[sel], mode=0)
        assert np.array_equal(idx, w.idx[sel]) and np.array_equal(score, w.score[sel])
        assert h.prune_stats() == (16388, int(w.b2[sel].sum()), 3 * 16388, 2)
        assert h.prune_verified() == int(w.settled[sel].sum())
        assert h.prune_scanned() == scanned
        h.close()
    assert one > two
