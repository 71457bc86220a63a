"""The asymmetric pose-cell cases of tests/_pc_asym.py can tell a right step from a wrong
one (no GPU): what test_pc_orientation_gpu.py feeds the HIP kernels is asymmetric in every
input an orientation mistake could hide behind, the float64 reference stays alive and has
an unambiguous peak at every step, and each single mistake -- a Gaussian's taps walked
backwards, a path filter transposed or flipped, the theta filter reversed, the shifts
swapped or negated, the filter row off by one, another inhibition -- moves the reference's
final state by far more than the GPU test's tolerance."""
import numpy as np
import pytest

import _pc_asym as A

SHAPES = sorted(A.SEEDS)
PRODUCT_SHAPES = [(16, 40, 10), (24, 40, 13), (16, 16, 36)]


def maxabs(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


def peak_gap(p):
    top = np.partition(p.ravel(), p.size - 2)[-2:]
    return float(top[1] - top[0])


def test_inputs_are_asymmetric():
    ge, gi, k_scale = A.gaussians()
    assert maxabs(ge, ge[::-1]) > 1e-3 and maxabs(gi, gi[::-1]) > 1e-3
    assert k_scale == 1.0 / abs(A.kernel_sum(ge, gi)) and np.isfinite(k_scale)
    table = A.filter_table()
    assert table.shape == (8, 7, 7)
    for r, f in enumerate(table):
        for name, g in (('transpose', f.T), ('x-flip', f[::-1, :]), ('y-flip', f[:, ::-1]),
                        ('rotation', f[::-1, ::-1])):
            assert maxabs(f, g) > 1e-3, (r, name)
    # x is the first filter axis: the tilt grows along it and falls along the second
    f0 = A.F.filter_2d(A.ORIGINS[6])
    assert table[6][6, 3] / f0[6, 3] == pytest.approx(1.18) and table[6][3, 6] / f0[3, 6] == pytest.approx(0.88)


@pytest.mark.parametrize('shape', SHAPES)
def test_control_covers_every_row_sign_and_width(shape):
    case = A.asym_case(shape)
    c = case.ctl
    assert case.steps == A.STEPS and c['ox'].shape == (A.STEPS, shape[2])
    for o in (c['ox'], c['oy']):
        assert o.min() < -3 and o.max() > 3 and abs(o).max() <= A.SHIFT_MAX   # both signs, beyond the window
    assert set(c['fidx'].ravel()) == set(range(8))
    assert np.array_equal(c['fidx'][2], (3 * np.arange(shape[2]) + 2) % 8)
    for s, zf in enumerate(c['zf']):
        assert maxabs(zf, zf[::-1]) > 1e-3, s
    energies = [e for e, _ in case.inject]
    assert len(set(energies)) == 3
    centre = tuple(n // 2 for n in shape)
    assert all(loc != centre for _, loc in case.inject)
    assert any(min(x, shape[0] - 1 - x) < 3 and min(y, shape[1] - 1 - y) < 3 and min(t, shape[2] - 1 - t) < 3
               for _, (x, y, t) in case.inject)                              # a packet that wraps


@pytest.mark.parametrize('shape', SHAPES)
def test_reference_alive_with_unambiguous_peaks(shape):
    """Alive: total > 0 and at least 5 % of the cells non-zero after every step from the
    second on.  After the first step the state is still the three packets of the point
    injections -- the kernel's positive core (57 cells within r^2 <= 5) spread by one path
    step, about 120 cells each -- which no grid above 7,200 cells can count as 5 %; there
    all three packets must be alive (300 cells).  Peaks: the gap between the largest and
    the second largest cell is at least 2 * F32_TOL at every step, so a float32 state
    within F32_TOL of the reference has the reference's argmax."""
    states, peaks, totals = A.asym_reference(shape)
    for s, p in enumerate(states):
        assert totals[s] > 0 and p.sum() > 0, s
        assert np.isfinite(p).all() and (p >= 0).all()
        nnz = int(np.count_nonzero(p))
        assert nnz >= (0.05 * p.size if s else 300), (s, nnz, p.size)
        assert peak_gap(p) >= 2 * A.F32_TOL, (s, peak_gap(p))
        assert peaks[s] == A.first_argmax(p)


@pytest.mark.parametrize('shape', SHAPES)
def test_every_mistake_moves_the_reference(shape):
    case = A.asym_case(shape)
    want = A.asym_reference(shape)[0][-1]
    moved = {}
    for m in A.MISTAKES:
        moved[m] = maxabs(A.reference(case, m)[0][-1], want)
    print(shape, ' '.join('%s=%.1e' % kv for kv in moved.items()))
    for m, d in moved.items():
        assert d > 100 * A.F32_TOL, (m, d)


@pytest.mark.parametrize('shape', PRODUCT_SHAPES)
def test_product_case_tells_inhibitions_apart(shape):
    """The product's parameters at global_inhibition = 0.05: alive (more cells than one
    packet's core), unambiguous peaks, and far from the state the product's own 0.2, or no
    inhibition at all, would leave."""
    case = A.product_case(shape)
    states, peaks, totals = A.product_reference(shape)
    for s, p in enumerate(states):
        assert totals[s] > 0 and np.count_nonzero(p) > 57, s
        assert peak_gap(p) >= 2 * A.F32_TOL, (s, peak_gap(p))
    assert set(case.ctl['fidx'].ravel()) == set(range(case.table.shape[0]))
    for other in (0.2, 0.0):
        c = A.Case(shape, case.seed, case.ge, case.gi, case.k_scale, other, case.table, case.ctl)
        assert maxabs(A.reference(c)[0][-1], states[-1]) > 100 * A.F32_TOL, other


def test_reference_excite_is_the_343_tap_correlation():
    """out[i] = sum_t g[t] * P[i + t - 3] per axis: a single cell's excitation is the
    kernel mirrored round it, on a wrapped grid."""
    ge, gi, k_scale = A.gaussians()
    k3 = A.kernel_3d(ge, gi, k_scale)
    p = np.zeros((9, 10, 11))
    p[1, 8, 5] = 1.0
    q = A.P.conv3d_wrap(p, k3)
    for t in ((0, 0, 0), (6, 2, 3), (1, 6, 5)):
        i = tuple((c - (tt - 3)) % n for c, tt, n in zip((1, 8, 5), t, p.shape))
        assert q[i] == pytest.approx(k3[t], rel=1e-15)
