"""The dense pose-cell cases of tests/_pc_dense.py and their bound (no GPU): the reference
restated there is the oracle's, byte for byte; every cell of every case is strictly
positive and the peaks are as far apart, or for the halo form's near-tie case as close, as
test_pc_dense_gpu.py needs; the e32 constants behind the bound B32 = 32 * e32 are what the
float32 emulation measures today; and each single mistake planted in the float64 reference
-- a cell that loses its smallest excitation, path or theta tap, a grid face padded with
`edge` instead of `wrap`, a tile that reads zeros on one side of its halo, a layer's shift
off by one, a tile left out of the normalisation's total -- misses B32 by a factor of at
least 20 at the very first step."""
import numpy as np
import pytest

import _pc_asym as A
import _pc_dense as D

SMALLEST = [(16, 16, 36), (16, 40, 10)]     # the smallest halo and rows shapes
# a lost tap shows where the stage of that tap is the wide one; the others show everywhere
PLANTED = [(m, n) for m in D.MISTAKES for n in D.SETS if not m.startswith('tap_') or m == 'tap_' + n]


def test_filters_are_positive_and_one_hot_taps_off_centre():
    ge, gi, k_scale = D.wide_k()
    k3 = A.kernel_3d(ge, gi, k_scale)
    assert (k3 > 0).all() and k3.sum() == pytest.approx(1.0, rel=1e-12)
    assert k3.min() / k3.sum() > 5e-4
    table = D.wide_table()
    assert table.shape == (8, 7, 7) and (table > 0).all()
    for r, f in enumerate(table):
        assert f.sum() == pytest.approx(1.0, rel=1e-12)
        for name, g in (('transpose', f.T), ('x-flip', f[::-1, :]), ('y-flip', f[:, ::-1]), ('rotation', f[::-1, ::-1])):
            assert np.abs(f - g).max() > 1e-3, (r, name)
    for s, zf in enumerate(D.wide_zf(3)):
        assert (zf > 0).all() and np.abs(zf - zf[::-1]).max() > 1e-3, s
    g, z, scale = D.one_hot_k()
    k1 = A.kernel_3d(g, z, scale)
    assert np.count_nonzero(k1) == 1 and k1[4, 4, 4] == 1.0
    hot = D.one_hot_table()
    assert len(set(D.ONE_HOT_TAPS)) == 8 and (3, 3) not in D.ONE_HOT_TAPS
    assert all(np.count_nonzero(f) == 1 and f[t] == 1.0 for f, t in zip(hot, D.ONE_HOT_TAPS))
    # no row is its own transpose, flip or rotation, so orientation still matters
    for x, y in D.ONE_HOT_TAPS:
        assert (x, y) not in {(y, x), (6 - x, y), (x, 6 - y), (6 - x, 6 - y)}, (x, y)
    for zf in D.one_hot_zf(3):
        assert np.count_nonzero(zf) == 1 and zf[3] == 0


@pytest.mark.parametrize('name', D.SETS)
def test_case_inputs(name):
    shape = (17, 30, 18)
    cs = D.case(name, shape)
    assert cs.start.sum() == pytest.approx(1.0, rel=1e-6) and cs.start.min() > 0.45 / cs.start.size
    assert np.array_equal(cs.start, cs.start.astype(np.float32).astype(np.float64))
    assert cs.inhibition == 0.25 / cs.start.size
    c = cs.ctl
    assert c['ox'].shape == (cs.steps, shape[2]) and c['zf'].shape == (cs.steps, 7)
    for o in (c['ox'], c['oy']):
        assert o.min() < -3 and o.max() > 3 and abs(o).max() <= 10
    assert np.array_equal(c['fidx'][1], (3 * np.arange(shape[2]) + 1) % 8)
    assert set(c['fidx'].ravel()) == set(range(8))


@pytest.mark.parametrize('name', D.SETS)
def test_reference_is_the_oracles(name):
    """D.step against _pc_asym.ref_excite and ref_path, byte for byte (skipping a tap that
    is exactly 0 changes no sum of non-negative terms)."""
    cs = D.case(name, (16, 40, 10))
    k3 = A.kernel_3d(cs.ge, cs.gi, cs.k_scale)
    states, peaks, totals = D.rollout(cs)
    p = np.array(cs.start)
    for s in range(cs.steps):
        p, total = A.ref_excite(p, k3, cs.inhibition)
        p = A.ref_path(p, cs.table, cs.ctl['ox'][s], cs.ctl['oy'][s], cs.ctl['fidx'][s], cs.ctl['zf'][s])
        assert p.tobytes() == states[s].tobytes() and total == totals[s], s
        assert peaks[s] == A.first_argmax(p)


def test_product_step_is_the_oracles():
    shape = (21, 21, 36)
    ref = A.P.PoseCellOracle(shape)
    ref.posecells = D.product_start(shape, 3).astype(np.float32).astype(np.float64)
    peak = ref.update(D.PRODUCT_V)
    got, got_peak = D.product_step(shape, 3)
    assert got.tobytes() == ref.posecells.tobytes() and got_peak == peak


@pytest.mark.parametrize('shape', D.SHAPES)
@pytest.mark.parametrize('name', D.SETS)
def test_reference_conditions(name, shape):
    """Dense at every step (reference() itself asserts that and the peak gaps of E, P and
    Z); ALL tends to uniform, and on the halo shapes its last state has a second cell well
    within the halo form's near-tie margin of the peak."""
    states, peaks, totals = D.reference(name, shape)
    assert len(states) == D.STEPS[name]
    for s, p in enumerate(states):
        assert totals[s] > 0 and p.sum() == pytest.approx(1.0, rel=1e-9)
        assert peaks[s] == A.first_argmax(p)
    gaps = [D.top_gap(p) for p in states]
    print(name, shape, 'gaps', ' '.join('%.2e' % g for g in gaps), 'min/max %.3f' % (states[-1].min() / states[-1].max()))
    if name == 'ALL':
        assert states[-1].min() / states[-1].max() > 0.95
        if shape in D.HALO_SHAPES:
            assert gaps[-1] < D.HALO_NEAR / 4


@pytest.mark.parametrize('name', D.SETS)
def test_e32_constants(name):
    """E32[name] is the float32 emulation's error as it measures today, within a factor of 2."""
    per_shape = {shape: D.measured_e32(name, shape) for shape in D.SHAPES}
    print(name, ' '.join('%s=%.2e' % kv for kv in per_shape.items()))
    e32 = max(per_shape.values())
    assert D.E32[name] / 2 <= e32 <= 2 * D.E32[name], (e32, D.E32[name])


@pytest.mark.parametrize('shape', D.PRODUCT_SHAPES)
def test_product_reference_and_e32(shape):
    """product_reference() asserts the peak gap of 1e-3 and the 90 % coverage; about half the
    start cells survive the inhibition and about a quarter of each output is non-zero."""
    outs = D.product_reference(shape)
    assert 0.45 < (D.product_start(shape, 0) > 0.2).mean() < 0.55
    for state, peak in outs:
        assert 0.15 < (state > 0).mean() < 0.35 and peak == A.first_argmax(state)
    e32 = D.measured_e32_product(shape)
    print(shape, 'e32 relative to the maximum = %.2e' % e32)
    assert D.E32_PRODUCT[shape] / 2 <= e32 <= 2 * D.E32_PRODUCT[shape], (e32, D.E32_PRODUCT[shape])


@pytest.mark.parametrize('shape', SMALLEST)
def test_every_planted_mistake_misses_the_bound(shape):
    """Planted at every step, seen at the first: at least 20 * B32 of its set."""
    moved = {}
    for m, name in PLANTED:
        want = D.reference(name, shape)[0][0]
        bad = D.rollout(D.case(name, shape), mistake=m)[0][0]
        moved[m, name] = D.rel_err(bad, want) / D.b32(name)
    print(shape, ' '.join('%s/%s=%.0f' % (m, n, v) for (m, n), v in moved.items()))
    for key, v in moved.items():
        assert v >= 20, (key, v)
