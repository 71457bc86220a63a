"""Tap and filter orientation of every pose-cell step form, pinned with asymmetric
parameters (tests/_pc_asym.py): tilted Gaussians, an 8-row table of tilted path filters of
which every row is used, tilted theta filters, per-layer shifts of both signs beyond the
7-tap window, an inhibition and a scale that are not the product's.  Each form runs the six
steps once through rs_pc_update and once through rs_pc_run and must follow the float64
reference -- the 343-tap periodic correlation, then conv_xy_shift with table[fidx] and
conv_z_wrap -- peak by peak and within the project's tolerances.  test_pc_orientation.py
shows, without a GPU, that every single orientation mistake misses these tolerances by a
factor of at least 100."""
import numpy as np
import pytest

import _pc_asym as A

pytestmark = pytest.mark.gpu

TOL = {'float32': A.F32_TOL, 'float64': A.F64_TOL}
CASES = [('rows', (16, 40, 10), 'float32'), ('rows', (16, 40, 10), 'float64'),
         ('cols', (24, 40, 13), 'float32'), ('cols', (24, 40, 13), 'float64'),
         ('cols:5', (24, 40, 13), 'float32'),
         ('stream:1,8,1,2', (24, 40, 13), 'float32'), ('stream:1,8,1,2', (24, 40, 13), 'float64'),
         ('stream:2,8,1,3', (24, 40, 13), 'float32'),
         ('halo', (16, 16, 36), 'float32'), ('halo', (17, 30, 18), 'float32'), ('halo', (20, 24, 10), 'float32')]


@pytest.fixture(scope='module')
def lib():
    from pyratslam_amd import _build, _lib
    _build.build()
    return _lib.require_device()


def check_rollout(lib, case, ref, form, precision, label):
    states, peaks, _ = ref
    got = {}
    for batched in (False, True):
        step_form, got_peaks, state = A.drive(lib, case, precision, batched)
        err = float(np.abs(state - states[-1]).max())
        print('%s %s %s %s %s: max|d| = %.3e' % (label, form, case.shape, precision,
                                                  'rs_pc_run' if batched else 'rs_pc_update', err))
        assert step_form == form.split(':')[0]
        assert got_peaks == peaks, (batched, got_peaks, peaks)
        assert np.isfinite(state).all() and (state >= 0).all()
        assert err < TOL[precision], (batched, err)
        got[batched] = state
    assert got[False].tobytes() == got[True].tobytes()


@pytest.mark.parametrize('form,shape,precision', CASES)
def test_asymmetric_rollout_vs_reference(lib, monkeypatch, form, shape, precision):
    monkeypatch.setenv('RS_PC_FORM', form)
    check_rollout(lib, A.asym_case(shape), A.asym_reference(shape), form, precision, 'asym')


@pytest.mark.parametrize('precision', ['float32', 'float64'])
def test_excite_alone_vs_reference(lib, monkeypatch, precision):
    """rs_pc_excite (the excitation kernel, then pc_scale_kernel) with the tilted Gaussians,
    their scale and the small inhibition, three times over: from the three injected cells,
    then from the dense states it left."""
    from pyratslam_amd import _lib
    monkeypatch.setenv('RS_PC_FORM', 'rows')
    case = A.asym_case((16, 40, 10))
    k3 = A.kernel_3d(case.ge, case.gi, case.k_scale)
    want = A.initial_state(case)
    h = A.create_case(lib, case, precision)
    try:
        assert lib.rs_pc_step_form(h) == b'rows'
        for energy, loc in case.inject:
            _lib.check(lib.rs_pc_inject(h, energy, *loc))
        for s in range(3):
            _lib.check(lib.rs_pc_excite(h))
            want, total = A.ref_excite(want, k3, case.inhibition)
            got = A.read_state(lib, h, case.shape)
            err = float(np.abs(got - want).max())
            print('excite %d %s: max|d| = %.3e' % (s, precision, err))
            assert total > 0 and np.count_nonzero(want) >= 100
            assert np.isfinite(got).all() and (got >= 0).all()
            assert err < TOL[precision], (s, err)
    finally:
        _lib.check(lib.rs_pc_destroy(h))


@pytest.mark.parametrize('form,shape,precision', [('rows', (16, 40, 10), 'float32'), ('rows', (16, 40, 10), 'float64'),
                                                  ('cols', (24, 40, 13), 'float32'),
                                                  ('stream:1,8,1,2', (24, 40, 13), 'float32'),
                                                  ('halo', (16, 16, 36), 'float32')])
def test_product_parameters_at_another_inhibition(lib, monkeypatch, form, shape, precision):
    """The product's Gaussians, table and theta filters with global_inhibition = 0.05: an
    inhibition that is honoured, not merely plumbed through beside a constant 0.2."""
    monkeypatch.setenv('RS_PC_FORM', form)
    check_rollout(lib, A.product_case(shape), A.product_reference(shape), form, precision, 'inhibition 0.05')
