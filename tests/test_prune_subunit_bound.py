"""CPU check of the sub-unit bound the prefilter of the pruned plane scan prunes by
(vt_prefilter_kernel with VT_PF_CGS column groups of 8 columns):

    LB(t, q, o) = TS(t) - QS(q, 4J - o) + 256 * B(t, q, o)

over columns 0 .. PF_COLS-1 of template rows 4J..4J+3 only (J = the prefilter's unit):
TS and QS the byte sums of those columns, B the number of their byte pairs with T < Q.
It is the sum of (T - Q) mod 256 over a subset of the byte pairs of score(t, q, o), whose
terms are all >= 0: a lower bound of the score at every offset for any number of columns.
The restatement here (sub_min_bounds) is what tests/test_plane_prefilter_subunit_gpu.py
counts prune_verified() and the pairs of pass B2 against."""
import numpy as np
import pytest

from oracle import view_templates as V
from test_prune_bound import PF_UNITS, cases, lower_bounds, offset_scores
from test_prune_verify_rule import min_bounds, score_matrix, small_cases, verify_rule

M = V.MAX_OFFSET
H, W = 64, 32
# the columns of a unit the prefilter's bound covers (8 * VT_PF_CGS of
# pyratslam_amd/csrc/vt_planes.h)
PF_COLS = 16
J = PF_UNITS[0]
COLS = [8, 16, 32]      # 1, 2 and 4 column groups


def sub_lower_bounds(t, q, cols=PF_COLS):
    """LB(t, q, o) for o = -(M-1)..M-1 over columns < cols of the unit, by the kernel's formula."""
    out = []
    for o in range(-M + 1, M):
        s = 4 * J - o
        assert s >= M and s + 3 <= H - M - 1
        tu, qu = t[4 * J:4 * J + 4, :cols].astype(np.int64), q[s:s + 4, :cols].astype(np.int64)
        out.append(int(tu.sum()) - int(qu.sum()) + 256 * int(np.count_nonzero(tu < qu)))
    return np.array(out)


def sub_min_bounds(lib, queries, cols=PF_COLS):
    """min over the offsets of the sub-unit bound as int64[nq][T] (sub_lower_bounds, vectorised)."""
    lib, queries = np.asarray(lib), np.asarray(queries)
    tu = lib[:, 4 * J:4 * J + 4, :cols].reshape(len(lib), -1).astype(np.int16)
    tsum = tu.sum(axis=1, dtype=np.int64)
    best = None
    for o in range(-M + 1, M):
        s = 4 * J - o
        qu = queries[:, s:s + 4, :cols].reshape(len(queries), -1).astype(np.int16)
        borrows = (tu[None] < qu[:, None]).sum(axis=2, dtype=np.int64)
        lb = tsum[None] - qu.sum(axis=1, dtype=np.int64)[:, None] + 256 * borrows
        best = lb if best is None else np.minimum(best, lb)
    return best


def pruned_per_query(lib, queries, cols=PF_COLS, scores=None):
    """Per query: (settled by verification, blocks pass B2 scans) of the pruned scan with
    the sub-unit bound: a settled query's U is U0, any other's the candidate block's
    minimum, and every other block with minLB <= U is scanned."""
    bounds = sub_min_bounds(lib, queries, cols)
    scores = score_matrix(lib, queries) if scores is None else scores
    ntb = (len(lib) + 63) // 64
    ver, pairs = [], []
    for q, (tb, _, u0, _, settled) in enumerate(verify_rule(bounds, scores)):
        u = u0 if settled else int(scores[q, 64 * tb:64 * tb + 64].min())
        ver.append(bool(settled))
        pairs.append(sum(1 for b in range(ntb) if b != tb and int(bounds[q, 64 * b:64 * b + 64].min()) <= u))
    return np.array(ver), np.array(pairs)


def pruned_counts(lib, queries, cols=PF_COLS):
    """(verified queries, (block, query) pairs of pass B2)."""
    ver, pairs = pruned_per_query(lib, queries, cols)
    return int(ver.sum()), int(pairs.sum())


@pytest.mark.parametrize('cols', COLS)
def test_sub_unit_bound_below_every_offset_score(cols):
    for t, q in cases():     # random, hit, decoy, all-0 against all-255 and the reverse
        lb, sc = sub_lower_bounds(t, q, cols), offset_scores(t, q)
        assert (lb >= 0).all() and (lb <= sc).all()
        for k, o in enumerate(range(-M + 1, M)):
            part = int(np.sum((t[4 * J:4 * J + 4, :cols] - q[4 * J - o:4 * J - o + 4, :cols]).astype(np.uint8),
                              dtype=np.uint64))
            assert lb[k] == part
        assert lb.min() <= int(V.vt_score(t, q))
        assert (lb <= lower_bounds(t, q)).all()                      # never above the whole unit's
    t, q = cases()[0]
    assert np.array_equal(sub_lower_bounds(t, q, 32), lower_bounds(t, q))


@pytest.mark.parametrize('cols', COLS)
def test_vectorised_sub_unit_bounds(cols):
    lib = V.synthetic_library(5, H, W, seed=64)
    qs, _ = V.synthetic_queries(lib, 4, seed=65, hit_frac=0.5)
    mb = sub_min_bounds(lib, qs, cols)
    for i, q in enumerate(qs):
        for j, t in enumerate(lib):
            assert mb[i, j] == sub_lower_bounds(t, q, cols).min()
    assert np.array_equal(sub_min_bounds(lib, qs, 32), min_bounds(lib, qs))


def test_bound_meets_the_score_when_the_differences_lie_in_the_sub_unit():
    q = np.random.default_rng(9).integers(0, 256, size=(H, W), dtype=np.uint8)
    for o, c0 in ((3, 5), (-7, 0), (0, PF_COLS - 4), (7, 12)):
        t = np.roll(q, o, axis=0)
        t[4 * J + 1, c0:c0 + 4] += 10                                # uint8: wraps, (T - Q) mod 256 = 10
        assert c0 + 4 <= PF_COLS and int(V.vt_score(t, q)) == 40
        lb = sub_lower_bounds(t, q)
        assert lb.min() == lb[o + M - 1] == 40 == offset_scores(t, q)[o + M - 1]


def test_bound_is_zero_and_valid_when_the_differences_lie_beside_the_sub_unit():
    q = np.random.default_rng(10).integers(0, 256, size=(H, W), dtype=np.uint8)
    for o, c0 in ((3, PF_COLS), (-2, 20), (0, W - 4)):
        t = np.roll(q, o, axis=0)
        t[4 * J + 1, c0:c0 + 4] += 10
        lb, sc = sub_lower_bounds(t, q), offset_scores(t, q)
        assert int(V.vt_score(t, q)) == 40 and lb[o + M - 1] == 0 and lb.min() == 0
        assert (lb <= sc).all()
        assert lower_bounds(t, q).min() == 40                        # the whole unit sees them


@pytest.mark.parametrize('cols', COLS)
def test_settled_implies_first_argmin_and_score_with_sub_unit_bounds(cols):
    seen = {}
    for lib, queries, name in small_cases():
        bounds, scores = sub_min_bounds(lib, queries, cols), score_matrix(lib, queries)
        assert (bounds <= scores).all() and (bounds >= 0).all()
        rule = verify_rule(bounds, scores)
        for q, (tb, that, u0, min2, settled) in enumerate(rule):
            assert tb == 0
            if settled:
                assert int(np.argmin(scores[q])) == that and int(scores[q].min()) == u0
        seen[name] = [r[4] for r in rule]
    assert all(seen['single'])
    assert not any(seen['decoy']) and not any(seen['tie'])
    if cols >= PF_COLS:
        # (the boundary case's differences lie in columns 5..8: inside the sub-unit)
        assert all(seen['hit']) and not any(seen['boundary'])


def test_sub_unit_bound_settles_what_the_whole_unit_settles_on_hits():
    lib = V.synthetic_library(130, H, W, seed=71)
    queries, _ = V.synthetic_queries(lib, 40, seed=81, hit_frac=0.9)
    assert pruned_counts(lib, queries, PF_COLS) == pruned_counts(lib, queries, 32)
