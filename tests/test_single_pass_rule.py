"""CPU check of the rule by which the pruned plane scan lists (block, query) pairs in ONE pass
(DESIGN section 34), restated on the oracle's score matrix and the half-unit bound:

    two passes   list1 = {tb*} for an unsettled query; then U(q) = the minimum of block tb* (U0
                 for a settled query) and list2 = {tb != tb* : minLB[tb][q] <= U(q)}
    one pass     the verification lists on its own score U0 = score(t^, q) >= U(q):
                 {tb* if unsettled} + {tb != tb* : minLB[tb][q] <= U0}

The one-pass list is a superset of the two lists, so no key changes (every scan meets in a
minimum over (score, index)); it holds the block of the first argmin; and it equals them
whenever t^ is its block's first argmin (then U0 = U).  The statistics stay the two-pass
rule's: the counting predicate tb != tb* and minlb[tb][q] <= ublk[q] over what a one-pass call
leaves (tbstar[q] = ~tb* where settled, ublk[q] = U(q)) reproduces them.  rules() is what
tests/test_plane_single_pass_gpu.py counts prune_scanned() against."""
import collections
import functools

import numpy as np
import pytest

from oracle import view_templates as V
from test_plane_front_gpu import world
from test_prune_bound import PF_UNITS, boundary_pair
from test_prune_subunit_bound import PF_COLS, pruned_per_query, sub_min_bounds
from test_prune_verify_rule import score_matrix, verify_rule

Rule = collections.namedtuple('Rule', 'tb that u0 u settled two one minlb')


def rules(bounds, scores):
    """Per query, from the min-bound and score matrices [nq][T]: candidate block, t^, U0, U(q),
    settled, the blocks of the two passes' lists together, the blocks of the one list, and
    minLB per block."""
    ntb = (bounds.shape[1] + 63) // 64
    out = []
    for q, (tb, that, u0, _, settled) in enumerate(verify_rule(bounds, scores)):
        minlb = [int(bounds[q, 64 * b:64 * b + 64].min()) for b in range(ntb)]
        u = u0 if settled else int(scores[q, 64 * tb:64 * tb + 64].min())
        own = set() if settled else {tb}
        two = own | {b for b in range(ntb) if b != tb and minlb[b] <= u}
        one = own | {b for b in range(ntb) if b != tb and minlb[b] <= u0}
        out.append(Rule(tb, that, u0, u, bool(settled), two, one, minlb))
    return out


def one_pass_pairs(bounds, scores):
    """The entries of the single pass's lists, per query."""
    return np.array([len(r.one) for r in rules(bounds, scores)])


@functools.lru_cache(maxsize=None)
def case130():
    """130 templates (3 blocks) with random, hit, decoy, twin, tie and boundary queries side by
    side (the library and the 300 queries of test_plane_front_gpu)."""
    w = world(130)
    return w, rules(sub_min_bounds(w.lib, w.queries, PF_COLS), w.sc)


class Cross:
    """An equal score at a lower index in a block other than tb*, whose bound equals U(q):
    test_plane_front_gpu's library of t templates with two boundary pairs planted across blocks.
    X (block 0) has bound = score = 40 and Y (block `hb`) bound 0 and score 40, so block hb is the
    candidate, U0 = 40, and block 0's bound equals it: only "<=" lists block 0, where the answer
    X is.  Query `qa`: Y alone in its block, so the verification settles it (U = U0 = 40).  Query
    `qb`: its Y twice (a twin right behind it), min2 = 0, so the query is unsettled and U = 40
    comes from the scan of block hb.  hb is block 1 of 130 templates and the last block of 1,030
    (the fused front's second chunk).  The queries: qa, qb, then four misses and four hits of
    the same world; w-like fields for the GPU test's check."""

    def __init__(self, t):
        w = world(t)
        rng = np.random.default_rng(4300 + t)
        self.ntb = w.ntb
        self.hb = 1 if t == 130 else w.ntb - 1
        self.xa, self.xb = 21, 22
        self.ya, self.yb = 64 * self.hb + 1, 64 * self.hb + 3
        qa, qb = (rng.integers(0, 256, size=(64, 32), dtype=np.uint8) for _ in range(2))
        lib = w.lib.copy()
        lib[self.xa], lib[self.ya] = boundary_pair(qa, units=PF_UNITS)
        lib[self.xb], lib[self.yb] = boundary_pair(qb, units=PF_UNITS)
        lib[self.yb + 1] = lib[self.yb]
        self.lib = lib
        self.queries = np.concatenate([qa[None], qb[None], w.queries[w.seg['misses'][:4]],
                                       w.queries[w.seg['offsets_settled'][1:5]]])
        self.sc = score_matrix(lib, self.queries)
        self.idx, self.score = self.sc.argmin(axis=1), self.sc.min(axis=1).astype(np.uint64)
        self.settled, self.b2 = pruned_per_query(lib, self.queries, PF_COLS, scores=self.sc)
        self.rules = rules(sub_min_bounds(lib, self.queries, PF_COLS), self.sc)
        self.lib.setflags(write=False)
        self.queries.setflags(write=False)


@functools.lru_cache(maxsize=None)
def cross(t):
    return Cross(t)


@pytest.mark.parametrize('t', [130, 1030])
def test_equal_score_at_a_lower_index_in_another_block_whose_bound_equals_u(t):
    c = cross(t)
    ra, rb = c.rules[0], c.rules[1]
    # settled: the verified template is Y, U = U0 = 40, block 0's bound is exactly 40
    assert ra.settled and ra.tb == c.hb and ra.that == c.ya and ra.u0 == ra.u == 40 and ra.minlb[0] == 40
    assert int(c.idx[0]) == c.xa and int(c.score[0]) == 40 and int(c.sc[0, c.ya]) == 40
    assert ra.one == ra.two == {0}
    # unsettled: min2 = 0 (the twin), U = 40 from the block, equal to U0 and to block 0's bound
    assert not rb.settled and rb.tb == c.hb and rb.that == c.yb and rb.u0 == rb.u == 40 and rb.minlb[0] == 40
    assert int(c.idx[1]) == c.xb and int(c.score[1]) == 40
    assert rb.one == rb.two == {0, c.hb}
    for q, r in ((0, ra), (1, rb)):
        # "<" in place of "<=" would leave block 0 out and answer Y, in either rule and in the count
        strict = {b for b in range(c.ntb) if b != r.tb and r.minlb[b] < r.u0}
        assert 0 not in strict and int(c.b2[q]) == len(strict) + 1 == 1
        assert 64 * r.tb + int(np.argmin(c.sc[q, 64 * r.tb:64 * r.tb + 64])) == r.that   # Y is its block's first argmin
    # the counting predicate at equality, over what a one-pass call leaves
    minlb = np.array([r.minlb for r in c.rules], dtype=np.uint32).T
    tbstar = np.array([~r.tb if r.settled else r.tb for r in c.rules], dtype=np.int32)
    ublk = np.array([r.u for r in c.rules], dtype=np.uint32)
    tbs = np.where(tbstar < 0, ~tbstar, tbstar)
    pairs = ((np.arange(c.ntb)[:, None] != tbs[None]) & (minlb <= ublk[None])).sum(axis=0)
    assert np.array_equal(pairs, c.b2) and np.array_equal(tbstar < 0, c.settled)
    # the other queries of the set are ordinary: misses list every block, hits are settled
    assert all(len(r.one) == c.ntb for r in c.rules[2:6]) and all(r.settled for r in c.rules[6:])


def test_one_pass_list_holds_the_two_pass_lists_and_the_first_argmin():
    w, rs = case130()
    for q, r in enumerate(rs):
        assert r.u <= r.u0
        assert r.two <= r.one
        if r.settled:       # the key is written by the verification itself
            assert int(w.idx[q]) == r.that and int(w.score[q]) == r.u0
        else:
            assert int(w.idx[q]) // 64 in r.one


def test_lists_are_equal_where_the_verified_template_is_its_blocks_first_argmin():
    w, rs = case130()
    seen = 0
    for q, r in enumerate(rs):
        blk = w.sc[q, 64 * r.tb:64 * r.tb + 64]
        if 64 * r.tb + int(np.argmin(blk)) == r.that:
            assert r.u == r.u0 and r.one == r.two
            seen += 1
    assert seen >= len(w.seg['hits']) + len(w.seg['misses'])       # hits and random queries among them
    for name in ('hits', 'misses', 'twin_other_block', 'offsets_settled'):
        assert all(rs[q].one == rs[q].two for q in w.seg[name])


def test_a_decoy_at_lane_0_of_the_match_block_lengthens_the_list():
    """lib[128] shares the bound's rows with lib[129] and nothing else: t^ is the decoy, U0 its
    large score, and every block's bound lies below it, while U(q) is the match's small score."""
    w, rs = case130()
    for q in w.seg['decoy_same_block']:
        r = rs[q]
        assert not r.settled and r.tb == 2 and r.that == 128 and int(w.idx[q]) == 129
        assert r.u < r.u0
        assert r.two < r.one and len(r.one) > len(r.two)            # strictly larger
        assert r.one == {0, 1, 2}
    # ... and the cases are not all alike: some lists hold the candidate block alone, some none
    sizes = {len(r.one) for r in rs}
    assert 0 in sizes and 1 in sizes and 3 in sizes


def test_ties_and_the_boundary_pair():
    w, rs = case130()
    for q in w.seg['twin_same_block']:          # equal bounds and scores in one block: block-scanned
        assert not rs[q].settled and rs[q].tb in rs[q].one and int(w.idx[q]) == 5
    for q in w.seg['boundary']:                 # min2 == U0: not settled, the lower index wins
        r = rs[q]
        assert not r.settled and r.u0 == 40 and r.u == 40 and int(w.idx[q]) == 20 and r.one == r.two
    # every template equal: every bound ties, nothing settles, every block is listed
    lib = np.full((130, 64, 32), 255, dtype=np.uint8)
    q0 = np.zeros((2, 64, 32), dtype=np.uint8)
    for r in rules(sub_min_bounds(lib, q0, PF_COLS), score_matrix(lib, q0)):
        assert not r.settled and r.tb == 0 and r.one == r.two == {0, 1, 2}


def test_the_counting_predicate_reproduces_the_two_pass_counts():
    w, rs = case130()
    nq, ntb = len(rs), w.ntb
    minlb = np.array([r.minlb for r in rs], dtype=np.uint32).T           # [ntb][nq], as the kernels keep it
    tbstar = np.array([~r.tb if r.settled else r.tb for r in rs], dtype=np.int32)
    ublk = np.array([r.u for r in rs], dtype=np.uint32)
    tbs = np.where(tbstar < 0, ~tbstar, tbstar)
    pairs = ((np.arange(ntb)[:, None] != tbs[None]) & (minlb <= ublk[None])).sum(axis=0)
    settled = tbstar < 0
    assert np.array_equal(settled, w.settled) and np.array_equal(pairs, w.b2)   # pruned_per_query's
    assert np.array_equal(pairs + ~settled, [len(r.two) for r in rs])
    assert settled.any() and (~settled).any() and pairs.any()
    # on another library, against an independent run of the two-pass restatement
    lib = V.synthetic_library(130, 64, 32, seed=91)
    qs, _ = V.synthetic_queries(lib, 24, seed=92, hit_frac=0.5)
    sc = score_matrix(lib, qs)
    ver, b2 = pruned_per_query(lib, qs, PF_COLS, scores=sc)
    rs2 = rules(sub_min_bounds(lib, qs, PF_COLS), sc)
    assert [r.settled for r in rs2] == list(ver)
    assert [len(r.two) - (not r.settled) for r in rs2] == list(b2)
    assert (one_pass_pairs(sub_min_bounds(lib, qs, PF_COLS), sc) >= b2 + ~ver).all()
