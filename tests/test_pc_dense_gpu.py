"""Every pose-cell step form stepped from dense states (tests/_pc_dense.py) and held to a
per-cell relative bound: every cell, every tile seam, every grid face and every block's
share of the global total carries signal, so one misplaced tap, one wrong halo load or one
dropped partial sum moves a compared number.  The parameter sets E, P and Z isolate the
excitation, the path and the theta stage (the other stages are one-hot, a shifted copy);
ALL has all three wide and drives the state towards uniform, where the halo form has to
settle its peak by the finishing pass.  Each case runs once through rs_pc_update, the
state read back after every step, and once through rs_pc_run from the same start.

The bound is B32 = 32 * e32 of the set (float64: B32 * 2^-29), e32 being the float32
emulation's own error against the float64 reference, measured on the CPU: never a number
derived from the kernels' output.  test_pc_dense.py shows, without a GPU, that a single
lost tap, an `edge` face, a zeroed tile halo, a shift off by one and a tile left out of
the total each miss it by a factor of at least 20.  The measured errors are printed."""
import math

import numpy as np
import pytest

import _pc_asym as A
import _pc_dense as D

pytestmark = pytest.mark.gpu

F32, F64 = 'float32', 'float64'
CASES = ([('halo', s, F32) for s in D.HALO_SHAPES] +
         [('rows', s, p) for s in [(16, 40, 10), (48, 40, 20)] for p in (F32, F64)] +
         [('cols', s, p) for s in [(24, 40, 13), (32, 32, 20)] for p in (F32, F64)] +
         [('cols:5', s, F32) for s in [(24, 40, 13), (32, 32, 20)]] +
         [('stream:1,8,1,2', (24, 40, 13), F32), ('stream:1,8,1,2', (24, 40, 13), F64),
          ('stream:2,8,1,3', (24, 40, 13), F32)])


@pytest.fixture(scope='module')
def lib():
    from pyratslam_amd import _build, _lib
    _build.build()
    return _lib.require_device()


@pytest.fixture(scope='module')
def pcn(lib):
    from pyratslam_amd import PoseCellNetwork
    return PoseCellNetwork


@pytest.mark.parametrize('name', D.SETS)
@pytest.mark.parametrize('form,shape,precision', CASES)
def test_dense_rollout_vs_reference(lib, monkeypatch, form, shape, precision, name):
    monkeypatch.setenv('RS_PC_FORM', form)
    cs = D.case(name, shape)
    want, want_peaks, _ = D.reference(name, shape)
    B = D.bound(name, precision)
    n = cs.steps
    final = {}
    for batched in (False, True):
        step_form, peaks, states, ambig = D.drive(lib, cs, precision, batched)
        assert step_form == form.split(':')[0]
        at = [n - 1] if batched else list(range(n))      # the steps whose state was read
        for s, got in zip(at, states):
            assert np.isfinite(got).all() and (got > 0).all(), (batched, s)
        errs = [D.rel_err(got, want[s]) for s, got in zip(at, states)]
        print('dense %s %s %s %s %s: max|d|/want = %s (B = %.3e)%s' % (
            name, form, shape, precision, 'rs_pc_run' if batched else 'rs_pc_update',
            ' '.join('%.3e' % e for e in errs), B, '' if ambig is None else ' near-tie calls = %d' % ambig))
        for s, e in zip(at, errs):
            assert e <= B, (batched, s, e, B)
        # the returned peak is the first maximum of the handle's own state ...
        for s, got in zip(at, states):
            assert peaks[s] == A.first_argmax(got), (batched, s, peaks[s])
        # ... and the reference's wherever its two largest cells are far enough apart
        for s in range(n):
            if D.top_gap(want[s]) > 100 * B:
                assert peaks[s] == want_peaks[s], (batched, s, peaks[s], want_peaks[s])
        if step_form == 'halo' and name == 'ALL':
            assert ambig >= 1, (batched, ambig)          # the near-tie path was taken
        final[batched] = states[-1]
    assert final[False].tobytes() == final[True].tobytes()


def make_net(pcn, monkeypatch, form, shape):
    if form is None:
        monkeypatch.delenv('RS_PC_FORM', raising=False)
    else:
        monkeypatch.setenv('RS_PC_FORM', form)
    net = pcn(shape)
    assert net.step_form() == (form or 'halo')
    return net


@pytest.mark.parametrize('form', [None, 'rows'])
@pytest.mark.parametrize('shape', D.PRODUCT_SHAPES)
def test_product_parameters_dense_step(pcn, monkeypatch, form, shape):
    """The product's own parameters through the Python class: uniform(0, 0.4) volumes, of
    which about half the cells survive the 0.2 inhibition, stepped once against the float64
    oracle's definition.  Many reference cells are 0 here, so the bound is relative to the
    reference's maximum: 32 times the float32 emulation's error measured the same way."""
    B = D.FACTOR * D.E32_PRODUCT[shape]
    with make_net(pcn, monkeypatch, form, shape) as net:
        for seed, (want, peak) in zip(D.PRODUCT_SEEDS, D.product_reference(shape)):
            net.posecells = D.product_start(shape, seed).astype(np.float32)
            got_peak = net.update(D.PRODUCT_V)
            got = net.posecells
            err = float(np.abs(got - want).max() / want.max())
            print('dense product %s %s seed %d: max|d|/max = %.3e (B = %.3e)' % (form or 'default', shape, seed, err, B))
            assert np.isfinite(got).all() and (got >= 0).all()
            assert got_peak == peak and got_peak == A.first_argmax(got), (seed, got_peak, peak)
            assert err <= B, (seed, err, B)


@pytest.mark.parametrize('form', [None, 'rows'])
@pytest.mark.parametrize('shape', D.PRODUCT_SHAPES)
def test_total_of_a_dense_state(pcn, monkeypatch, form, shape):
    """net.total() of a written dense state: every block's partial sum counts."""
    v = D.product_start(shape, 0).astype(np.float32)
    want = math.fsum(v.ravel().tolist())
    with make_net(pcn, monkeypatch, form, shape) as net:
        net.posecells = v
        got = net.total()
    print('dense total %s %s: rel = %.3e' % (form or 'default', shape, abs(got - want) / want))
    assert abs(got - want) <= 2.0 ** -20 * want, (got, want)
