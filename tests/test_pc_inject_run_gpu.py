"""Injections inside a batched run (rs_pc_run_odom_inject): the call is
defined as inject() and update() made one by one on the same handle, and must give the same
peaks, the same resolved cells and a stored volume for which np.array_equal holds, in every
step form and both precisions.  The twin below makes those calls; the float64 oracle, run
through the same sequence, bounds the float32 state by the project's 1e-5 and fixes the
argmax of every step."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from oracle import posecell as P
from test_pc_peak_gpu import EPS, assert_close, odometry, restated

pytestmark = pytest.mark.gpu

F32_TOL = 1e-5   # the project's float32 state bound (tests/test_posecell_gpu.py)
PEAK = 'peak'
FORMS = [((21, 21, 36), 'float32', '', 'halo'), ((32, 32, 18), 'float32', '', 'halo'),
         ((24, 40, 13), 'float32', 'cols', 'cols'), ((24, 40, 13), 'float64', 'cols', 'cols'),
         ((24, 40, 13), 'float32', 'stream:1,8,1,2', 'stream'), ((24, 40, 13), 'float64', 'rows', 'rows'),
         ((7, 7, 7), 'float32', '', None)]


@pytest.fixture(scope='module')
def pcn():
    from pyratslam_amd import _build
    _build.build()
    from pyratslam_amd import PoseCellNetwork
    assert PoseCellNetwork.AT_PEAK == PEAK
    return PoseCellNetwork


def centre(shape):
    return tuple(s // 2 for s in shape)


def sequence(net, od, injections, poses=False):
    """The definition: the injections and updates one by one.  Returns (peaks, cells, poses);
    a KeyError of an update goes to the caller with the cells so far in ``sequence.cells``."""
    cells, peaks, out_poses = [], [], []
    sequence.cells = cells

    def point(s):
        for st, e, loc in injections:
            if st != s:
                continue
            if loc == PEAK:
                cell = tuple(int(v) for v in net.get_pc_max())
            elif loc[0] == 'same':
                cell = cells[loc[1]]
            else:
                cell = tuple(int(v) % n for v, n in zip(loc, net.shape))
            net.inject(e, cell)
            cells.append(cell)

    for s, v in enumerate(od):
        point(s)
        if poses:
            out_poses.append(net.update_pose(v))
            peaks.append(net.max_pc)
        else:
            peaks.append(tuple(int(x) for x in net.update(v)))
    point(len(od))
    return peaks, cells, out_poses


def as_cells(a):
    return [tuple(int(v) for v in c) for c in a]


def table_injections(shape):
    c = centre(shape)
    far = tuple((p + n // 2) % n for p, n in zip(c, shape))
    return [(0, 0.3, ((c[0] + 1) % shape[0], c[1], c[2])),
            (5, 5.0, far), (5, 0.1, PEAK),
            (9, 0.2, ('same', 2)),
            (12, 0.05, (1, 2, 3))], far


# -- forms and precisions ----------------------------------------------------------------
@pytest.mark.parametrize('shape,precision,form,want_form', FORMS)
def test_every_form_equals_the_calls_one_by_one(pcn, monkeypatch, shape, precision, form, want_form):
    monkeypatch.setenv('RS_PC_FORM', form)
    od = odometry(12, 71)
    inj, far = table_injections(shape)
    net, twin = pcn(shape, precision=precision), pcn(shape, precision=precision)
    ref = P.PoseCellOracle(shape)
    for x in (net, twin, ref):
        x.inject(1, centre(shape))
    assert want_form is None or net.step_form() == want_form
    maxes, cells = net.run(od, injections=inj)
    assert maxes.dtype == np.int32 and maxes.shape == (12, 3)
    assert cells.dtype == np.int32 and cells.shape == (5, 3)
    want_peaks, want_cells, _ = sequence(twin, od, inj)
    assert as_cells(maxes) == want_peaks
    assert as_cells(cells) == want_cells
    assert as_cells(cells)[2] == far == as_cells(cells)[3]      # at-peak landed on the new cell
    got, want = net.posecells, twin.posecells
    assert np.array_equal(got, want)
    # a trailing injection: the last step's peak is no longer the state's
    assert net.get_pc_max() == twin.get_pc_max()
    assert net.max_pc == want_peaks[-1]
    if precision == 'float32':
        ref_peaks, ref_cells, _ = sequence(ref, od, inj)
        assert want_peaks == [tuple(int(v) for v in m) for m in ref_peaks]
        assert want_cells == [tuple(int(v) for v in c) for c in ref_cells]
        err = float(np.abs(got - ref.posecells).max())
        print('max |d| against the oracle: %.3e' % err)
        assert err < F32_TOL, err
    net.close()
    twin.close()


# -- halo batch lengths: the camera-only pattern ---------------------------------------
@pytest.mark.parametrize('n', [1, 2, 17, 65])
def test_halo_at_peak_before_every_step(pcn, monkeypatch, n):
    monkeypatch.delenv('RS_PC_FORM', raising=False)
    shape = (21, 21, 36)
    od = odometry(n, 73)
    inj = [(s, 0.02, PEAK) for s in range(n)]
    net, twin = pcn(shape), pcn(shape)
    assert net.step_form() == 'halo'
    for x in (net, twin):
        x.inject(1, centre(shape))
    maxes, cells = net.run(od, injections=inj)
    want_peaks, want_cells, _ = sequence(twin, od, inj)
    assert as_cells(maxes) == want_peaks and as_cells(cells) == want_cells
    assert net.get_pc_max() == want_peaks[-1] == net.max_pc     # (no trailing injection: the cached peak)
    assert np.array_equal(net.posecells, twin.posecells)


# -- mixed calls -------------------------------------------------------------------------
def test_injections_on_a_pending_halo_state(pcn, monkeypatch):
    monkeypatch.delenv('RS_PC_FORM', raising=False)
    shape = (21, 21, 36)
    od = odometry(9, 79)
    net, twin = pcn(shape), pcn(shape)
    for x in (net, twin):
        x.inject(1, centre(shape))
    assert np.array_equal(net.run(od[:4]), twin.run(od[:4]))      # lazy: the state stays pending
    maxes, cells = net.run(od[:0], injections=[(0, 0.3, PEAK)])   # the injections alone
    assert maxes.shape == (0, 3)
    want = twin.get_pc_max()
    twin.inject(0.3, want)
    assert as_cells(cells) == [want]
    assert net.get_pc_max() == twin.get_pc_max()
    assert np.array_equal(net.run(od[4:6]), twin.run(od[4:6]))    # lazy again
    inj = [(0, 0.25, PEAK), (0, 7.0, (2, 3, 4)), (0, 0.1, PEAK), (3, 0.5, ('same', 0))]
    maxes, cells = net.run(od[6:], injections=inj)
    want_peaks, want_cells, _ = sequence(twin, od[6:], inj)
    assert as_cells(maxes) == want_peaks and as_cells(cells) == want_cells
    assert want_cells[2] == (2, 3, 4)       # the second at-peak of one point sees the first two
    assert net.get_pc_max() == twin.get_pc_max()
    assert np.array_equal(net.posecells, twin.posecells)


# -- poses ---------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,precision,form', [((21, 21, 36), 'float32', ''), ((24, 40, 13), 'float64', 'cols'),
                                                  ((24, 40, 13), 'float32', 'rows')])
def test_poses_with_injections(pcn, monkeypatch, shape, precision, form):
    """Step s's pose comes from the state before any injection with step s + 1: the twin reads
    its volume back right after update s, and the restatement of that volume gives the bound."""
    monkeypatch.setenv('RS_PC_FORM', form)
    od = odometry(8, 83)
    c = centre(shape)
    far = tuple((p + n // 2) % n for p, n in zip(c, shape))
    inj = [(0, 0.2, PEAK), (3, 4.0, far), (4, 0.1, PEAK), (8, 3.0, (1, 1, 1))]
    net, twin = pcn(shape, precision=precision), pcn(shape, precision=precision)
    for x in (net, twin):
        x.inject(1, c)
    maxes, poses, cells = net.run(od, poses=True, injections=inj)
    assert poses.shape == (8, 3) and poses.dtype == np.float64
    cur, want_cells = 0, []
    for s, v in enumerate(od):
        while cur < len(inj) and inj[cur][0] == s:
            cell = twin.get_pc_max() if inj[cur][2] == PEAK else inj[cur][2]
            twin.inject(inj[cur][1], cell)
            want_cells.append(tuple(int(x) for x in cell))
            cur += 1
        m = tuple(int(x) for x in twin.update(v))
        assert tuple(int(x) for x in maxes[s]) == m
        want, bound = restated(twin.posecells, m, 3, EPS[precision])
        assert_close(poses[s], want, bound, shape, s)
    twin.inject(3.0, (1, 1, 1))
    assert as_cells(cells) == want_cells + [(1, 1, 1)]
    assert np.array_equal(net.posecells, twin.posecells)


# -- eager readback, poisoned buffers ----------------------------------------------------------
@pytest.mark.parametrize('form,precision', [('', 'float32'), ('rows', 'float64')])
def test_eager_readback_and_poison(pcn, monkeypatch, form, precision):
    from pyratslam_amd import _lib
    monkeypatch.setenv('RS_PC_FORM', form)
    shape = (21, 21, 36)
    od = odometry(6, 89)
    inj = [(0, 0.3, PEAK), (2, 6.0, (4, 5, 6)), (2, 0.2, PEAK), (6, 0.4, ('same', 0))]
    nets = [pcn(shape, precision=precision), pcn(shape, precision=precision, readback='eager'),
            pcn(shape, precision=precision), pcn(shape, precision=precision)]
    lazy, eager, poisoned, twin = nets
    for x in nets:
        x.inject(1, centre(shape))
        x.run(od[:2])
    _lib.check(poisoned._lib.rs_pc_debug(poisoned._h, _lib.RS_PC_DBG_POISON))
    want_peaks, want_cells, _ = sequence(twin, od, inj)
    want = twin.posecells
    for x in (lazy, eager, poisoned):
        maxes, cells = x.run(od, injections=inj)
        assert as_cells(maxes) == want_peaks and as_cells(cells) == want_cells
        assert np.array_equal(x.posecells, want)
    # one step through the eager network's own update() behind the injections
    assert eager.update(od[0]) == twin.update(od[0])
    assert np.array_equal(eager.posecells, twin.posecells)


# -- LUT miss ------------------------------------------------------------------------------
@pytest.mark.parametrize('poses', [False, True])
def test_lut_miss_applies_the_injections_up_to_its_step(pcn, monkeypatch, poses):
    monkeypatch.delenv('RS_PC_FORM', raising=False)
    case = load_golden('pc_keyerror')
    shape, loc = tuple(int(s) for s in case['shape']), (16, 16, 9)
    od = odometry(6, 53)
    od[3] = case['odom'][0]
    inj = [(1, 0.3, PEAK), (3, 5.0, (3, 4, 5)), (3, 0.1, PEAK), (4, 0.2, ('same', 0)), (6, 0.2, (1, 1, 1))]
    net, twin = pcn(shape), pcn(shape)
    for x in (net, twin):
        x.inject(1, loc)
    with pytest.raises(KeyError):
        net.run(od, poses=poses, injections=inj)
    with pytest.raises(KeyError):
        sequence(twin, od, inj)
    want_cells = list(sequence.cells)
    assert len(want_cells) == 3 and want_cells[2] == (3, 4, 5)
    assert as_cells(net.last_injection_cells) == want_cells + [(-1, -1, -1)] * 2
    assert net.max_pc == twin.max_pc
    if poses:
        assert net.last_poses.shape == (3, 3)
    assert net.get_pc_max() == twin.get_pc_max()
    assert np.array_equal(net.posecells, twin.posecells)
    # a miss at step 0: the injections in front of it, then steps 1-4 of it
    with pytest.raises(KeyError):
        net.run(od[3:], injections=[(0, 0.5, (2, 2, 2)), (1, 0.5, PEAK)])
    twin.inject(0.5, (2, 2, 2))
    with pytest.raises(KeyError):
        twin.update(od[3])
    assert as_cells(net.last_injection_cells) == [(2, 2, 2), (-1, -1, -1)]
    assert np.array_equal(net.posecells, twin.posecells)


# -- refusals --------------------------------------------------------------------------------
def inject_abi(net, od, step, energy, loc, sums=None, control=None):
    """The C calls themselves: (status, peaks, cells)."""
    from pyratslam_amd import _lib
    od = np.ascontiguousarray(od, dtype=np.float64).reshape(-1, 2)
    n, ni = len(od), len(step)
    step, energy = np.asarray(step, dtype=np.int32), np.asarray(energy, dtype=np.float64)
    loc = np.ascontiguousarray(loc, dtype=np.int32).reshape(-1, 3)
    out, cells = np.full((n, 3), -7, dtype=np.int32), np.full((ni, 3), -7, dtype=np.int32)
    i32, f64 = ctypes.c_int32, ctypes.c_double
    inj = (ni, _lib.ptr(step, i32), _lib.ptr(energy, f64), _lib.ptr(loc, i32))
    outs = (_lib.ptr(out, i32), _lib.ptr(cells, i32), _lib.ptr(sums, f64))
    if control is None:
        st = net._lib.rs_pc_run_odom_inject(net._h, n, _lib.ptr(od, f64), *inj, *outs, None)
    else:
        ox, oy, rows, zf = control
        st = net._lib.rs_pc_run_inject(net._h, n, _lib.ptr(ox, i32), _lib.ptr(oy, i32), _lib.ptr(rows, i32),
                                       _lib.ptr(zf, f64), *inj, *outs)
    return st, out, cells


@pytest.mark.parametrize('form,precision', [('', 'float32'), ('rows', 'float64')])
def test_refusals_leave_the_state_untouched(pcn, monkeypatch, form, precision):
    from pyratslam_amd import _lib
    monkeypatch.setenv('RS_PC_FORM', form)
    shape = (21, 21, 36)
    od = odometry(4, 97)
    net = pcn(shape, precision=precision)
    net.inject(1, centre(shape))
    net.run(od)                       # (halo: a pending state, which a refusal must not settle either)
    before = net.posecells
    ok = (1, 1, 1)
    bad = [([(2, 1.0, ok), (1, 1.0, ok)], ValueError),          # steps out of order
           ([(5, 1.0, ok)], ValueError), ([(-1, 1.0, ok)], ValueError),   # a step outside [0, n]
           ([(0, 1.0, (21, 0, 0))], IndexError), ([(0, 1.0, (0, -22, 0))], IndexError),
           ([(0, 1.0, (0, 0, 36))], IndexError),                 # an explicit cell outside the grid
           ([(0, 1.0, ('same', 0))], ValueError),                # same-as k >= i
           ([(0, 1.0, ok), (1, 1.0, ('same', 1))], ValueError), ([(0, 1.0, ok), (1, 1.0, ('same', 2))], ValueError),
           ([(0, 1.0, ok), (1, 1.0, ('same', -1))], ValueError)]
    for inj, exc in bad:
        with pytest.raises(exc):
            net.run(od, injections=inj)
        assert np.array_equal(net.posecells, before), inj
    # the library itself: RS_ERR_ARG before any device work
    P_, S_ = _lib.RS_PC_INJ_AT_PEAK, _lib.RS_PC_INJ_SAME_AS
    raw = [([2, 1], [ok, ok]), ([5], [ok]), ([-1], [ok]), ([0], [(21, 0, 0)]), ([0], [(0, -3, 0)]),
           ([0], [(0, 0, 36)]), ([0], [(S_, 0, 0)]), ([0, 1], [ok, (S_, 1, 0)]), ([0, 1], [ok, (S_, -1, 0)]),
           ([0], [(-3, 0, 0)])]
    for step, loc in raw:
        st, _, _ = inject_abi(net, od, step, [1.0] * len(step), loc)
        assert st == _lib.RS_ERR_ARG, (step, loc, st)
        assert np.array_equal(net.posecells, before), (step, loc)
    # sums before rs_pc_set_peak_tables
    st, _, _ = inject_abi(net, od, [0], [1.0], [(P_, 0, 0)], sums=np.zeros((4, 6)))
    assert st == _lib.RS_ERR_STATE
    assert np.array_equal(net.posecells, before)
    # negative indices count from the end, as inject()'s do
    twin = pcn(shape, precision=precision)
    twin.posecells = before
    _, cells = net.run(od[:0], injections=[(0, 0.5, (-1, -2, -3))])
    twin.inject(0.5, (-1, -2, -3))
    assert as_cells(cells) == [(20, 19, 33)]
    assert np.array_equal(net.posecells, twin.posecells)


# -- the C ABI -------------------------------------------------------------------------------
@pytest.mark.parametrize('form,precision', [('', 'float32'), ('stream:1,8,1,2', 'float32'), ('cols', 'float64')])
def test_caller_control_equals_library_control(pcn, monkeypatch, form, precision):
    from pyratslam_amd import _lib
    from pyratslam_amd import filters as F
    monkeypatch.setenv('RS_PC_FORM', form)
    shape = (24, 40, 36)
    od = odometry(7, 101)
    P_, S_ = _lib.RS_PC_INJ_AT_PEAK, _lib.RS_PC_INJ_SAME_AS
    step, energy = [0, 3, 3, 7], [0.2, 6.0, 0.1, 0.3]
    loc = [(P_, 0, 0), (2, 3, 4), (P_, 0, 0), (S_, 0, 0)]
    a, b = pcn(shape, precision=precision), pcn(shape, precision=precision)
    for x in (a, b):
        x.inject(1, centre(shape))
    ox, oy, rows, zf, first_bad = F.batch_control(od, shape[2], a.filter_table)
    assert first_bad is None
    st_a, peaks_a, cells_a = inject_abi(a, od, step, energy, loc)
    st_b, peaks_b, cells_b = inject_abi(b, od, step, energy, loc, control=(ox, oy, rows, zf))
    assert st_a == st_b == _lib.RS_OK
    assert np.array_equal(peaks_a, peaks_b) and np.array_equal(cells_a, cells_b)
    assert as_cells(cells_a)[2] == (2, 3, 4) and (cells_a >= 0).all()
    assert np.array_equal(a.posecells, b.posecells)
    # the Python fallback: odometry outside the library's control tables
    od2 = od.copy()
    od2[1] = (0.3, 6.0)
    inj = [(0, 0.2, PEAK), (2, 0.3, ('same', 0)), (7, 0.1, PEAK)]
    maxes, cells = a.run(od2, injections=inj)
    want_peaks, want_cells, _ = sequence(b, od2, inj)
    assert as_cells(maxes) == want_peaks and as_cells(cells) == want_cells
    assert np.array_equal(a.posecells, b.posecells)
