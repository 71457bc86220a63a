"""The long pose-cell trajectories of tests/_pc_long.py and their bounds (no GPU): the C
oracle steps from every stored reference state to the next one and finds every peak; the
emulation errors the bounds are built from are what the emulations give today; the caps
test_pc_long_gpu.py leans on hold in the fixtures (few windows with e32w above 1e-6, at most
one near-tie of the reference's two largest cells, peaks that cross the grid faces often
enough); and a single mistake planted in the float64 reference -- the theta or the x face
padded with `edge` instead of `wrap`, one layer's shift off by one, a cell that loses its
smallest excitation tap -- misses the window bound Bw by a factor of at least 20 within the
window it is planted in."""
import os

import numpy as np
import pytest

import _pc_asym as A
import _pc_dense as D
import _pc_long as L
from oracle import posecell as P

C_AGREEMENT = 5e-15                 # the C oracle against the NumPy one
SAMPLE = 10
MAX_FIXTURE_BYTES = 512 * 1024


@pytest.mark.parametrize('name', L.NAMES)
def test_fixture_is_consistent(name):
    tr = L.load(name)
    shape, steps = L.TRAJECTORIES[name]
    assert tr.shape == shape and tr.steps == steps and tr.inject == tuple(s // 2 for s in shape)
    assert np.array_equal(tr.odom, L.odometry(name))
    assert tr.max_pc.shape == (steps, 3) and tr.gap.shape == (steps,)
    assert tr.e32w.shape == (tr.windows,) and tr.e32f.shape == tr.e64n.shape == (tr.windows + 1,)
    start = np.zeros(shape)
    start[tr.inject] = 1
    assert np.array_equal(tr.state(0), start) and tr.e32f[0] == 0 and tr.e64n[0] == 0
    peaks = tr.peaks()
    for c in range(1, tr.windows + 1):
        p = tr.state(c)
        assert np.isfinite(p).all() and (p >= 0).all() and p.max() > 0.1, c
        assert A.first_argmax(p) == peaks[c * L.WINDOW - 1], c
        assert L.top_two_gap(p) == tr.gap[c * L.WINDOW - 1], c
    assert os.path.getsize(os.path.join(L.GOLDEN, 'pc_long_%s.npz' % name)) < MAX_FIXTURE_BYTES


@pytest.mark.parametrize('name', L.NAMES)
def test_c_oracle_steps_from_every_stored_state(name):
    """Every window (64x64x36: every fourth) from its stored state: the next stored state
    within 5e-15, and the reference's peak at every step."""
    from oracle import c_oracle as C
    tr = L.load(name)
    peaks = tr.peaks()
    net = C.PoseCellC(tr.shape)
    threads = C.threads()
    C.set_threads(min(threads, 4))      # a step is milliseconds of work: more threads only wait for one another
    worst = 0.0
    try:
        for w in range(0, tr.windows, 4 if name == '64x64x36' else 1):
            net.posecells[...] = tr.state(w)
            for s in range(w * L.WINDOW, (w + 1) * L.WINDOW):
                assert net.update(tr.odom[s]) == peaks[s], s
            e = L.err(net.posecells, tr.state(w + 1))
            worst = max(worst, e)
            assert e <= C_AGREEMENT, (w, e)
    finally:
        C.set_threads(threads)
    print('long %s: C oracle within %.2e of the stored states' % (name, worst))


@pytest.mark.parametrize('name', L.NAMES)
def test_bound_inputs_are_pinned(name):
    """e32w at ten windows spread over the trajectory, e32f and e64n at the first ten
    checkpoints: equal to the stored values."""
    tr = L.load(name)
    for w in np.linspace(0, tr.windows - 1, SAMPLE).astype(int):
        lo = w * L.WINDOW
        assert L.window_e32(tr.state(w), tr.odom[lo:lo + L.WINDOW], tr.state(w + 1)) == tr.e32w[w], w
    for kind, stored in (('e32f', tr.e32f), ('e64n', tr.e64n)):
        got = L.free_errors(tr.state(0), tr.odom, tr.state, kind, upto=SAMPLE)
        assert np.array_equal(got, stored[:SAMPLE + 1]), (kind, got, stored[:SAMPLE + 1])


@pytest.mark.parametrize('name', L.NAMES)
def test_caps_hold_in_the_fixture(name):
    tr = L.load(name)
    loose = int((tr.e32w > L.TIGHT_E32W).sum())
    ties = int((tr.gap <= L.GAP_MIN).sum())
    cx, cy, cth = L.face_crossings(tr.max_pc, tr.shape)
    h = L.horizon(tr)
    print('long %s: e32w max %.2e median %.2e, %d of %d windows above 1e-6; Bw %.2e .. %.2e; %d gaps <= 2e-5; '
          'crossings x %d y %d theta %d; e32f max %.2e, horizon %s; e64n max %.2e, Bf64 at the end %.2e'
          % (name, tr.e32w.max(), np.median(tr.e32w), loose, tr.windows, L.bw(tr).min(), L.bw(tr).max(), ties,
             cx, cy, cth, tr.e32f.max(), h, tr.e64n.max(), L.bf64(tr)[-1]))
    assert loose <= 0.10 * tr.windows, loose
    assert ties <= 1, ties
    assert cx >= L.MIN_XY_CROSSINGS and cy >= L.MIN_XY_CROSSINGS, (cx, cy)
    if name.endswith('_turn'):
        assert cth >= L.MIN_TH_CROSSINGS_TURN, cth
    assert h is None or h >= 1
    assert (L.bf64(tr) >= L.F64_TOL).all() and (np.diff(L.bf32(tr)) >= 0).all()


def crossing_window(tr, axis):
    """The last window in which the reference's peak crosses the face of ``axis``."""
    d = np.abs(np.diff(tr.max_pc[:, axis].astype(np.int64)))
    steps = np.flatnonzero(d > tr.shape[axis] // 2) + 1       # the step that lands beyond the face
    return int(steps[-1]) // L.WINDOW


def lost_tap_cell(p):
    """Where a lost smallest excitation tap shows.  The packet is a few cells wide and the
    inhibition of 0.2 removes every cell whose excitation is below it, so the tap (the most
    negative one, three cells from the centre) reads a zero at most cells, and most cells it
    changes are removed anyway: of the cells that survive the inhibition, the one whose
    smallest tap reads the most activity."""
    k3 = P.dog_kernel_3d()
    t = D.smallest_tap(k3)
    reads = np.roll(p, tuple(P.HALF - int(v) for v in t), axis=(0, 1, 2))     # reads[c] = p[c + t - 3]
    survives = P.conv3d_wrap(p, k3) > P.PC_GLOBAL_INHIB
    return A.first_argmax(np.where(survives, reads, -1.0))


def planted(tr, w, mistake):
    """The float64 reference over window w with ``mistake`` at every step: the error at the
    window's end.  ``ox_off`` is planted in the layer of the peak before the step."""
    lo = w * L.WINDOW
    p = np.array(tr.state(w))
    for s in range(lo, lo + L.WINDOW):
        cell = lost_tap_cell(p) if mistake == 'tap_E' else A.first_argmax(p)
        p = L.step(p, tr.odom[s], mistake, cell)
    return L.err(p, tr.state(w + 1))


# the face mistakes where the packet straddles that face; the two others in a late window
PLANTED = [('edge_th', '32x32x18_turn', 2), ('edge_th', '64x64x36', 2), ('edge_x', '32x32x18', 0),
           ('edge_x', '50x50x10', 0), ('ox_off', '32x32x18', None), ('ox_off', '64x64x36', None),
           ('tap_E', '32x32x18', None), ('tap_E', '50x50x10', None)]


@pytest.mark.parametrize('mistake,name,axis', PLANTED)
def test_planted_mistake_misses_the_window_bound(mistake, name, axis):
    tr = L.load(name)
    w = tr.windows - 3 if axis is None else crossing_window(tr, axis)
    assert w >= tr.windows // 2, w                      # later than any other test reaches
    clean = planted(tr, w, None)
    moved = planted(tr, w, mistake)
    bound = L.bw(tr)[w]
    print('long planted %s at %s window %d: moved %.2e = %.0f x Bw (Bw = %.2e; the reference restated: %.1e)'
          % (mistake, name, w, moved, moved / bound, bound, clean))
    assert clean <= C_AGREEMENT, clean
    assert moved >= 20 * bound, (moved, bound)
