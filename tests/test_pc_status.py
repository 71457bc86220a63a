"""The status protocol of PoseCellNetwork's odometry calls, pinned without a device: a stub
network over a fake library that returns scripted statuses and records its calls.

Rows: ``update`` (lazy readback), ``update_pose``, ``run`` of 0, 1 and 3 steps, ``run(poses=
True)`` of 0 and 3, ``run(injections=...)`` of 3 with and without an injection behind the last
step (and once with poses).  Columns: RS_OK; RS_ERR_LUT_KEY at step 0 and at step 2;
RS_ERR_CTL_RANGE followed by success and by a host-side LUT miss (the odometry of
test_host_control.py::test_keyerror_at_half_cell); RS_ERR_HIP.  Every cell: the exception and
``KeyError.args``, the library calls in order, ``max_pc``, ``_max_valid``, ``last_poses`` and
``last_injection_cells``.

The rule (``PoseCellNetwork._settle``): the steps before a LUT miss count, ``max_pc`` is the
last of them, the cached maximum is valid only after a call that ran a step, missed nothing
and injected nothing behind its last step, and a miss re-raises the reference's KeyError.

Three cells were left as they stood before the rule had one place, and are False now: a call
of no steps that succeeds used to leave ``_max_valid`` alone in ``run0-ok``, ``run0-range_ok``
and ``poses0-range_ok`` (True here, where every call starts from a valid cache), while
``poses0-ok`` and a ``run(injections=...)`` of no steps already invalidated it.
"""
import ctypes
import threading

import numpy as np
import pytest

from pyratslam_amd import _lib
from pyratslam_amd import filters as F
from pyratslam_amd.posecell_network import PoseCellNetwork

SHAPE = (8, 8, 18)
SENT = (7, 7, 7)            # max_pc before the call, with _max_valid True
GOOD = [[0.2, 0.0], [0.3, 0.01], [0.2, 0.0]]
MISS = [0.1, 0.0]           # half a cell: KeyError((5, 5)) (test_keyerror_at_half_cell)
CELL = (1, 2, 3)            # what the fake library resolves every injection to

# argument positions of the calls the fake library fills outputs for; 'rec' are recorded
LAYOUT = {
    'rs_pc_update_odom': dict(out=3),
    'rs_pc_update_odom_peak': dict(out=3, sums=4),
    'rs_pc_update': dict(out=5),
    'rs_pc_run_odom': dict(n=1, out=3, bad=4, rec=(1,)),
    'rs_pc_run_odom_peaks': dict(n=1, out=3, sums=4, bad=5, rec=(1,)),
    'rs_pc_run_odom_inject': dict(n=1, ni=3, step=4, out=7, cells=8, sums=9, bad=10, rec=(1, 3)),
    'rs_pc_run': dict(n=1, out=6, rec=(1,)),
    'rs_pc_run_peaks': dict(n=1, out=6, sums=7, rec=(1,)),
    'rs_pc_run_inject': dict(n=1, ni=6, step=7, out=10, cells=11, sums=12, rec=(1, 6)),
}


def _array(arg, ctype, count):
    """The ``count`` elements an argument points at: a raw address or a ctypes pointer."""
    if arg is None or count == 0:
        return None
    addr = arg if isinstance(arg, int) else ctypes.cast(arg, ctypes.c_void_p).value
    return (ctype * count).from_address(addr)


class FakeLib:
    """``script``: per call name, the (status, failing step) of its successive calls; a call
    without one returns RS_OK.  Step s finishes with max_pc (s+1, s+1, s+1) and zero sums."""

    def __init__(self, script):
        self.script = {k: list(v) for k, v in script.items()}
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('rs_'):
            raise AttributeError(name)

        def call(*args):
            lay = LAYOUT.get(name, {})
            self.calls.append((name,) + tuple(args[i] for i in lay.get('rec', ())))
            st, bad = self.script[name].pop(0) if self.script.get(name) else (_lib.RS_OK, -1)
            n = args[lay['n']] if 'n' in lay else 1
            done = n if st == _lib.RS_OK else bad if st == _lib.RS_ERR_LUT_KEY else 0
            out = _array(args[lay['out']], ctypes.c_int32, 3 * done) if 'out' in lay else None
            for i in range(3 * done if out is not None else 0):
                out[i] = i // 3 + 1
            sums = _array(args[lay['sums']], ctypes.c_double, 6 * done) if 'sums' in lay else None
            for i in range(6 * done if sums is not None else 0):
                sums[i] = 0.0
            if 'cells' in lay and st in (_lib.RS_OK, _lib.RS_ERR_LUT_KEY):
                ni = args[lay['ni']]
                step = _array(args[lay['step']], ctypes.c_int32, ni)
                cells = _array(args[lay['cells']], ctypes.c_int32, 3 * ni)
                for i in range(ni):
                    if step[i] <= done:
                        cells[3 * i:3 * i + 3] = CELL
            if 'bad' in lay and st == _lib.RS_ERR_LUT_KEY:
                args[lay['bad']]._obj.value = bad
            return st
        return call


class _Stub(PoseCellNetwork):
    """A PoseCellNetwork's host side over a fake library: no device, no handle to destroy."""

    def __init__(self, lib):
        self.shape = SHAPE
        self.cells_to_avg = 1
        self._eager = False
        self._fresh = None
        self._peak_ready = False
        self.last_poses = None
        self.last_injection_cells = None
        self.filter_table = F.FilterTable()
        self.max_pc, self._max_valid = SENT, True
        self._mutex = threading.Lock()
        self._lib = lib
        self._h = ctypes.c_void_p(1)
        self._out3 = np.empty(3, dtype=np.int32)
        self._out3_addr = self._out3.ctypes.data
        self._update = lib.rs_pc_update
        self._update_odom = lib.rs_pc_update_odom
        self._update_odom_read = lib.rs_pc_update_odom_read

    def close(self):
        pass


ROWS = {   # id: (kind, n, poses, injection behind the last step)
    'update': ('update', 1, False, None),
    'update_pose': ('update_pose', 1, True, None),
    'run0': ('run', 0, False, None),
    'run1': ('run', 1, False, None),
    'run3': ('run', 3, False, None),
    'poses0': ('run', 0, True, None),
    'poses3': ('run', 3, True, None),
    'inject3': ('run', 3, False, False),
    'inject3_behind': ('run', 3, False, True),
    'inject3_behind_poses': ('run', 3, True, True),
}
COLS = ['ok', 'key0', 'key2', 'range_ok', 'range_miss', 'hip']
# the call that gets the scripted status, and the host-control call behind RS_ERR_CTL_RANGE
FIRST = {('update', False, False): ('rs_pc_update_odom', 'rs_pc_update'),
         ('update_pose', True, False): ('rs_pc_update_odom_peak', 'rs_pc_run_peaks'),
         ('run', False, False): ('rs_pc_run_odom', 'rs_pc_run'),
         ('run', True, False): ('rs_pc_run_odom_peaks', 'rs_pc_run_peaks'),
         ('run', False, True): ('rs_pc_run_odom_inject', 'rs_pc_run_inject'),
         ('run', True, True): ('rs_pc_run_odom_inject', 'rs_pc_run_inject')}


def _cells():
    for row, (kind, n, poses, behind) in ROWS.items():
        for col in COLS:
            miss = {'key0': 0, 'key2': 2, 'range_miss': n - 1}.get(col)
            if miss is not None and not 0 <= miss < n:
                continue        # (no such step in this row)
            yield pytest.param(row, col, miss, id='%s-%s' % (row, col))


@pytest.mark.parametrize('row, col, miss', list(_cells()))
def test_status_protocol(row, col, miss):
    kind, n, poses, behind = ROWS[row]
    single = kind != 'run' or (n == 1 and not poses and behind is None)   # update()'s prebound call
    first, host = FIRST[('update' if single and kind == 'run' else kind, poses, behind is not None)]
    od = np.array(GOOD[:n], dtype=np.float64).reshape(-1, 2)
    if miss is not None:
        od[miss] = MISS
    status = {'ok': _lib.RS_OK, 'key0': _lib.RS_ERR_LUT_KEY, 'key2': _lib.RS_ERR_LUT_KEY,
              'hip': _lib.RS_ERR_HIP}.get(col, _lib.RS_ERR_CTL_RANGE)
    lib = FakeLib({first: [(status, miss if miss is not None else -1)]})
    net = _Stub(lib)
    injections = None
    if behind is not None:
        injections = [(1, 0.5, (1, 1, 1))] + ([(n, 0.5, PoseCellNetwork.AT_PEAK)] if behind else [])
    ni = len(injections or ())

    def call():
        if kind == 'update':
            return net.update(od[0])
        if kind == 'update_pose':
            return net.update_pose(od[0])
        return net.run(od, poses=poses, injections=injections)

    # -- the exception -------------------------------------------------------------
    if miss is not None:
        with pytest.raises(KeyError) as e:
            call()
        assert e.value.args[0] == (5, 5)
    elif col == 'hip':
        with pytest.raises(_lib.HipLibraryError):
            call()
    else:
        got = call()
        if kind == 'update':
            assert got == (1, 1, 1)
        elif kind == 'update_pose':
            assert got == (1.0, 1.0, 1.0)
        else:
            got = got if isinstance(got, tuple) else (got,)
            assert len(got) == 1 + bool(poses) + (behind is not None)
            want = np.repeat(np.arange(1, n + 1), 3).reshape(n, 3)
            assert got[0].dtype == np.int32 and np.array_equal(got[0], want)
            if poses:
                assert got[1].dtype == np.float64 and np.array_equal(got[1], want)

    # -- the calls, in order ---------------------------------------------------------
    done = n if miss is None else miss
    tail = (ni,) if behind is not None else ()
    want = [('rs_pc_set_peak_tables',)] if poses else []
    want.append((first,) if single else (first, n) + tail)
    if col in ('range_ok', 'range_miss'):
        if kind == 'update' or (single and kind == 'run'):
            want += [(host,)] if miss is None else []
        elif behind is not None:
            want.append((host, done, sum(1 for s in injections if s[0] <= done)))
        elif done > 0:
            want.append((host, done))
        if miss is not None:
            want.append(('rs_pc_excite',))
    assert lib.calls == want

    # -- the state it leaves ---------------------------------------------------------
    if col == 'hip':
        assert net.max_pc == SENT and net._max_valid is True
    else:
        assert net.max_pc == ((done,) * 3 if done > 0 else SENT)
        assert net._max_valid is (miss is None and done > 0 and not behind)
    if poses and miss is not None and not (kind == 'update_pose' and col == 'key0'):
        # (update_pose's own LUT miss leaves no poses; its host-control path an empty array)
        assert net.last_poses.shape == (done, 3) and net.last_poses.dtype == np.float64
        assert np.array_equal(net.last_poses, np.repeat(np.arange(1.0, done + 1), 3).reshape(done, 3))
    else:
        assert net.last_poses is None
    if behind is None:
        assert net.last_injection_cells is None
    else:
        cells = np.full((ni, 3), -1, dtype=np.int32)
        if col != 'hip':
            for i, s in enumerate(injections):
                if s[0] <= done:
                    cells[i] = CELL
        assert np.array_equal(net.last_injection_cells, cells)
