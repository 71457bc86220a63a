"""CPU check of the rule by which the pruned plane scan settles a query in its candidate
block without scanning the block (vt_prune_verify_kernel):

    l^   = the block's template with the least bound min_o LB(t, q, o), lowest index on ties
    min2 = the least bound among the block's other templates (NONE if it has no other)
    U0   = the exact score of (l^, q)
    settled  <=>  min2 > U0

Every other template has score >= bound >= min2 > U0, so a settled block's first argmin
is l^ and its minimum is U0: what a scan of the block would return.  With >= a template
whose bound equals U0 could hold an equal score at a lower index.  The restatement here
(verify_rule) is what tests/test_plane_verify_gpu.py counts prune_verified() against."""
import numpy as np

from oracle import view_templates as V
from test_prune_bound import PF_UNITS, boundary_pair, lower_bounds

M = V.MAX_OFFSET
NONE = 0xFFFFFFFF


def min_bounds(lib, queries, units=PF_UNITS):
    """min over the offsets of LB(t, q, o) as int64[nq][T] (lower_bounds, vectorised)."""
    lib, queries = np.asarray(lib), np.asarray(queries)
    best = None
    for o in range(-M + 1, M):
        lb = np.zeros((len(queries), len(lib)), dtype=np.int64)
        for j in units:
            s = 4 * j - o
            tu = lib[:, 4 * j:4 * j + 4].reshape(len(lib), -1).astype(np.int16)
            qu = queries[:, s:s + 4].reshape(len(queries), -1).astype(np.int16)
            borrows = (tu[None] < qu[:, None]).sum(axis=2, dtype=np.int64)
            lb += tu.sum(axis=1, dtype=np.int64)[None] - qu.sum(axis=1, dtype=np.int64)[:, None] + 256 * borrows
        best = lb if best is None else np.minimum(best, lb)
    return best


def score_matrix(lib, queries):
    return np.stack([V.vt_scores_library(lib, q) for q in queries]).astype(np.int64)


def verify_rule(bounds, scores):
    """Per query: (candidate block, l^ as a library index, U0, min2, settled) from the
    min-bound and score matrices [nq][T] of a library in blocks of 64."""
    nq, t = bounds.shape
    ntb = (t + 63) // 64
    out = []
    for q in range(nq):
        min1 = [int(bounds[q, 64 * b:64 * b + 64].min()) for b in range(ntb)]
        tb = int(np.argmin(min1))                          # first: the lowest block on ties
        blk = bounds[q, 64 * tb:64 * tb + 64]
        lane = int(np.argmin(blk))                         # first: the lowest lane on ties
        others = np.delete(blk, lane)
        min2 = int(others.min()) if len(others) else NONE
        u0 = int(scores[q, 64 * tb + lane])
        out.append((tb, 64 * tb + lane, u0, min2, min2 > u0))
    return out


def settled_mask(lib, queries):
    return np.array([r[4] for r in verify_rule(min_bounds(lib, queries), score_matrix(lib, queries))])


def small_cases():
    """(library of one block, queries, name)."""
    rng = np.random.default_rng(61)
    lib = V.synthetic_library(12, 64, 32, seed=62)
    hits, _ = V.synthetic_queries(lib, 10, seed=63, hit_frac=1.0)
    rand = rng.integers(0, 256, size=(10, 64, 32), dtype=np.uint8)
    yield lib, hits, 'hit'
    yield lib, rand, 'random'
    # decoy at a lower index than the match: equal bounds, a large score
    dec = lib.copy()
    dec[2] = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
    dec[2, 16:48] = dec[7, 16:48]
    q7 = np.clip(dec[7].astype(np.int16)[None] - rng.integers(0, 4, size=(4, 64, 32)), 0, 255).astype(np.uint8)
    yield dec, q7, 'decoy'
    # two identical templates: a tie of bounds and of scores
    tie = lib.copy()
    tie[9] = tie[4]
    q4 = np.clip(tie[4].astype(np.int16)[None] - rng.integers(0, 4, size=(4, 64, 32)), 0, 255).astype(np.uint8)
    yield tie, q4, 'tie'
    # min2 == U0: X (index 3) has bound = score = 40, Y (index 8) bound 0 and score 40
    q = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
    bnd = lib.copy()
    bnd[3], bnd[8] = boundary_pair(q, units=PF_UNITS)
    yield bnd, q[None], 'boundary'
    yield lib[:1], hits[:3], 'single'


def test_vectorised_bounds_are_lower_bounds():
    lib = V.synthetic_library(5, 64, 32, seed=64)
    qs, _ = V.synthetic_queries(lib, 4, seed=65, hit_frac=0.5)
    mb = min_bounds(lib, qs)
    for i, q in enumerate(qs):
        for j, t in enumerate(lib):
            assert mb[i, j] == lower_bounds(t, q).min()


def test_settled_implies_first_argmin_and_score():
    seen = {}
    for lib, queries, name in small_cases():
        bounds, scores = min_bounds(lib, queries), score_matrix(lib, queries)
        assert (bounds <= scores).all() and (bounds >= 0).all()
        rule = verify_rule(bounds, scores)
        for q, (tb, that, u0, min2, settled) in enumerate(rule):
            assert tb == 0
            if settled:
                assert int(np.argmin(scores[q])) == that and int(scores[q].min()) == u0
        seen[name] = [r[4] for r in rule]
    # the rule does settle what it is for, and holds back where it must
    assert all(seen['hit']) and all(seen['single'])
    assert not any(seen['decoy']) and not any(seen['tie']) and not any(seen['boundary'])


def test_greater_or_equal_would_miss_the_lower_index():
    lib, queries, _ = [c for c in small_cases() if c[2] == 'boundary'][0]
    bounds, scores = min_bounds(lib, queries), score_matrix(lib, queries)
    (tb, that, u0, min2, settled), = verify_rule(bounds, scores)
    assert (that, u0, min2, settled) == (8, 40, 40, False)
    assert int(np.argmin(scores[0])) == 3           # ... which ">=" would have settled as 8
