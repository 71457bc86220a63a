"""Every pose-cell step form against the reference along thousands of steps of the benched
odometry stream (tests/_pc_long.py; fixtures made by the reference itself).

Anchored windows: the reference's state at every 10th step is written to the handle, ten
steps are run and the state is compared with the reference's next stored state.  The bound
is Bw = 32 * max(e32w, median e32w) (float64: Bw * 2^-29), e32w being the float32
emulation's error over that very window, measured on the CPU; wherever e32w <= 1e-6 the
north-star 1e-5 holds too, and the peak of every step is the reference's wherever the
reference's top-two gap exceeds 2e-5.  So a packet that straddles a grid face for the
fiftieth time, control formed deep in a batch and the theta wrap (the _turn trajectory) are
compared cell by cell with the reference, which the 40-step tests never reach.

The free run: the whole trajectory from the injection in run() batches of ten.  The
reference's dynamics amplify rounding, so the bound is the emulations' own
measured drift: Bf64 = max(1e-12, 32 * running max of e64n) with identical peaks at every
step whose gap exceeds 2e-5; Bf32 = 32 * running max of e32f with identical peaks where the
gap exceeds 2 * Bf32, up to the float32 parity horizon (the first checkpoint at which Bf32
exceeds 1e-3).  Beyond it a float32 run is held to what needs no reference: finite,
non-negative, the returned peak its own state's first maximum, and one run() of all steps
byte-identical to the batches.

No bound here derives from a kernel's output; test_pc_long.py pins their inputs and shows
that planted mistakes miss Bw by a factor of 20.  Each test prints its measured ratios."""
import numpy as np
import pytest

import _pc_asym as A
import _pc_long as L

pytestmark = pytest.mark.gpu

F32, F64 = 'float32', 'float64'
STREAM = 'stream:1,8,1,2'


def cols_fits(shape, precision):
    """The column form's limits on a grid (pc_cols_fit): X >= 14, Y >= 18 and a multiple of
    the 16-byte vector, TH >= 10."""
    return shape[0] >= 14 and shape[1] >= 18 and shape[1] % (4 if precision == F32 else 2) == 0 and shape[2] >= 10


def forms(name):
    shape = L.TRAJECTORIES[name][0]
    out = [(None, F32), (None, F64), ('rows', F32), ('rows', F64)]
    out += [('cols', p) for p in (F32, F64) if cols_fits(shape, p)]
    return out + [(STREAM, F32), (STREAM, F64)]


CASES = [(name, form, precision) for name in L.NAMES for form, precision in forms(name)]
# the cases whose windows also go through update() step by step
PER_STEP = {(None, F32), ('rows', F64)}


@pytest.fixture(scope='module')
def pcn():
    from pyratslam_amd import _build
    _build.build()
    from pyratslam_amd import PoseCellNetwork
    return PoseCellNetwork


def make_net(pcn, monkeypatch, form, shape, precision):
    if form is None:
        monkeypatch.delenv('RS_PC_FORM', raising=False)
    else:
        monkeypatch.setenv('RS_PC_FORM', form)
    net = pcn(shape, precision=precision)
    # the default: the halo form in float32 on all three grids, rows in float64
    want = form.split(':')[0] if form else ('halo' if precision == F32 else 'rows')
    assert net.step_form() == want, (net.step_form(), want)
    return net


def label(name, form, precision):
    return '%s %s %s' % (name, form or 'default', precision)


@pytest.mark.parametrize('name,precision', [(n, p) for n in L.NAMES for p in (F32, F64)
                                            if not cols_fits(L.TRAJECTORIES[n][0], p)])
def test_cols_is_refused_where_it_does_not_fit(pcn, monkeypatch, name, precision):
    monkeypatch.setenv('RS_PC_FORM', 'cols')
    with pytest.raises(ValueError):
        pcn(L.TRAJECTORIES[name][0], precision=precision)


@pytest.mark.parametrize('name,form,precision', CASES)
def test_anchored_windows(pcn, monkeypatch, name, form, precision):
    tr = L.load(name)
    bound = L.bw(tr, precision)
    ref_peaks = tr.peaks()
    dt = np.float32 if precision == F32 else np.float64
    errs = np.zeros(tr.windows)
    with make_net(pcn, monkeypatch, form, tr.shape, precision) as net:
        for w in range(tr.windows):
            lo = w * L.WINDOW
            start, od, want = tr.state(w).astype(dt), tr.odom[lo:lo + L.WINDOW], tr.state(w + 1)
            net.posecells = start
            peaks = [tuple(int(v) for v in r) for r in net.run(od)]
            got = net.posecells
            assert np.isfinite(got).all() and (got >= 0).all(), w
            errs[w] = L.err(got, want)
            assert errs[w] <= bound[w], (w, errs[w], bound[w])
            if tr.e32w[w] <= L.TIGHT_E32W:
                assert errs[w] <= L.F32_TOL, (w, errs[w])
            for s in range(L.WINDOW):
                if tr.gap[lo + s] > L.GAP_MIN:
                    assert peaks[s] == ref_peaks[lo + s], (w, s, peaks[s], ref_peaks[lo + s])
            assert peaks[-1] == A.first_argmax(got) == net.max_pc, (w, peaks[-1])
            if (form, precision) in PER_STEP:
                net.posecells = start
                for s, v in enumerate(od):
                    assert net.update(v) == peaks[s], (w, s)
                assert net.posecells.tobytes() == got.tobytes(), w
    ratio = errs / np.where(tr.e32w > 0, tr.e32w, np.inf)
    print('long windows %s: max err %.3e (window %d), max err/e32w %.3g (window %d), max err/Bw %.3g, %d windows'
          % (label(name, form, precision), errs.max(), errs.argmax(), ratio.max(), ratio.argmax(),
             (errs / bound).max(), tr.windows))


@pytest.mark.parametrize('name,form,precision', CASES)
def test_free_run(pcn, monkeypatch, name, form, precision):
    tr = L.load(name)
    ref_peaks = tr.peaks()
    nc = tr.windows + 1
    errs = np.zeros(nc)
    peaks = []
    with make_net(pcn, monkeypatch, form, tr.shape, precision) as net:
        net.inject(1, tr.inject)
        errs[0] = L.err(net.posecells, tr.state(0))
        for c in range(1, nc):
            m = net.run(tr.odom[(c - 1) * L.WINDOW:c * L.WINDOW])
            got = net.posecells
            peaks += [tuple(int(v) for v in r) for r in m]
            errs[c] = L.err(got, tr.state(c))
            assert np.isfinite(got).all() and (got >= 0).all(), c
            assert peaks[-1] == A.first_argmax(got) == net.max_pc, (c, peaks[-1])
        final = got
    differ = [s for s in range(tr.steps) if peaks[s] != ref_peaks[s]]
    first_differ = differ[0] if differ else None
    if precision == F64:
        bound = L.bf64(tr)
        run_max = np.maximum.accumulate(tr.e64n)
        print('long free run %s: max err %.3e, max err/Bf64 %.3g, max err/running max e64n %.3g, first peak that '
              'differs: step %s' % (label(name, form, precision), errs.max(), (errs / bound).max(),
                                    (errs[1:] / run_max[1:]).max(), first_differ))
        for c in range(nc):
            assert errs[c] <= bound[c], (c, errs[c], bound[c])
        for s in range(tr.steps):
            if tr.gap[s] > L.GAP_MIN:
                assert peaks[s] == ref_peaks[s], (s, peaks[s], ref_peaks[s])
        return
    bound, h = L.bf32(tr), L.horizon(tr)
    upto = nc if h is None else h                 # checkpoints below the horizon
    run_max = np.maximum.accumulate(tr.e32f)
    above = np.flatnonzero(errs > L.F32_TOL)
    print('long free run %s: horizon %s, max err/running max e32f up to it %.3g, max err/Bf32 up to it %.3g, '
          'err at the end %.3e, first checkpoint with err > 1e-5: %s, first peak that differs: step %s'
          % (label(name, form, precision), h, (errs[1:upto] / run_max[1:upto]).max(), (errs[1:upto] / bound[1:upto]).max(),
             errs[-1], int(above[0]) if len(above) else None, first_differ))
    for c in range(upto):
        assert errs[c] <= bound[c], (c, errs[c], bound[c])
    for s in range(tr.steps):
        c = L.checkpoint_of_step(s)
        if c < upto and tr.gap[s] > 2 * bound[c]:
            assert peaks[s] == ref_peaks[s], (s, peaks[s], ref_peaks[s])
    # one run() of all steps: the same state as the batches of ten
    with make_net(pcn, monkeypatch, form, tr.shape, precision) as net:
        net.inject(1, tr.inject)
        m = net.run(tr.odom)
        assert [tuple(int(v) for v in r) for r in m] == peaks
        assert net.posecells.tobytes() == final.tobytes()
