"""CPU check of the bound the pruned plane scan (vt_prefilter_kernel) prunes by:

    LB(t, q, o) = sum over the prefilter's units J of
                  TS_J(t) - QS_J(q, 4J - o) + 256 * B_J(t, q, o)

TS_J = byte sum of template rows 4J..4J+3, QS_J(q, S) = byte sum of query rows
S..S+3, B_J = number of byte pairs of the unit with T < Q (the borrows).  It is the
exact sum of (T - Q) mod 256 over the unit's byte pairs, a subset of the pairs of
score(t, q, o) whose terms are all >= 0: LB <= score for every offset, with equality
when every non-zero term lies inside the units."""
import numpy as np
import pytest

from oracle import view_templates as V

M = V.MAX_OFFSET
H, W = 64, 32
# the prefilter's template units (pf_unit() of pyratslam_amd/csrc/vt_planes.h)
PF_UNITS = (7,)


def unit_rows(units=PF_UNITS):
    return np.concatenate([np.arange(4 * j, 4 * j + 4) for j in units])


def offset_scores(t, q):
    """The oracle's per-offset sums (vt_score's loop body), o = -(M-1)..M-1."""
    h = t.shape[0]
    qq = q[M:h - M]
    return np.array([int(np.sum(np.abs(t[M + o:h - M + o] - qq), dtype=np.uint64)) for o in range(-M + 1, M)])


def lower_bounds(t, q, units=PF_UNITS):
    """LB(t, q, o) for o = -(M-1)..M-1, by the kernel's formula."""
    out = []
    for o in range(-M + 1, M):
        lb = 0
        for j in units:
            s = 4 * j - o
            assert s >= M and s + 3 <= H - M - 1          # the unit's query rows lie in the window
            tu, qu = t[4 * j:4 * j + 4].astype(np.int64), q[s:s + 4].astype(np.int64)
            lb += int(tu.sum()) - int(qu.sum()) + 256 * int(np.count_nonzero(tu < qu))
        out.append(lb)
    return np.array(out)


def boundary_pair(q, o_x=3, o_y=-2, units=PF_UNITS):
    """X: the query rolled by o_x plus 4 x 10 inside the first unit (LB_X = score = 40).
    Y: the query rolled by o_y plus 2 x 20 on a row outside every unit (LB_Y = 0)."""
    x = np.roll(q, o_x, axis=0)
    r = 4 * units[0] + 1
    x[r, 5:9] += 10                                         # uint8: wraps, (T - Q) mod 256 = 10
    y = np.roll(q, o_y, axis=0)
    free = [r for r in range(20, 44) if r not in set(unit_rows(units))]
    y[free[0], 11:13] += 20
    return x, y


def cases():
    rng = np.random.default_rng(5)
    lib = V.synthetic_library(6, H, W, seed=3)
    hits, _ = V.synthetic_queries(lib, 6, seed=4, hit_frac=1.0)
    miss = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    decoy = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    decoy[16:48] = lib[0][16:48]
    pairs = [(lib[i], miss) for i in range(6)] + [(lib[i], hits[j]) for i in range(6) for j in range(6)]
    pairs += [(decoy, lib[0]), (decoy, hits[0])]
    pairs += [(np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)),
              (np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8))]
    return pairs


@pytest.mark.parametrize('units', [PF_UNITS, (5, 10), (4,), (11,)])
def test_bound_below_every_offset_score(units):
    for t, q in cases():
        lb, sc = lower_bounds(t, q, units), offset_scores(t, q)
        assert (lb >= 0).all() and (lb <= sc).all()
        # the formula is the partial sum of the wrapped differences over the units
        for k, o in enumerate(range(-M + 1, M)):
            part = sum(int(np.sum((t[4 * j:4 * j + 4] - q[4 * j - o:4 * j - o + 4]).astype(np.uint8), dtype=np.uint64))
                       for j in units)
            assert lb[k] == part
        assert lb.min() <= int(V.vt_score(t, q))


@pytest.mark.parametrize('units', [PF_UNITS, (5, 10)])
def test_bound_meets_the_score_in_the_constructed_case(units):
    q = np.random.default_rng(9).integers(0, 256, size=(H, W), dtype=np.uint8)
    x, y = boundary_pair(q, units=units)
    assert int(V.vt_score(x, q)) == int(V.vt_score(y, q)) == 40
    assert lower_bounds(x, q, units).min() == 40       # all of X's score inside the unit
    assert lower_bounds(y, q, units).min() == 0        # all of Y's outside
    assert offset_scores(x, q)[3 + M - 1] == 40 and offset_scores(y, q)[-2 + M - 1] == 40
