"""``PoseCellEnsemble``: many small pose-cell networks of one shape stepped side by side,
each by one workgroup out of a compute unit's LDS (``csrc/pose_ensemble.hip``, DESIGN
section 35).

    ens = PoseCellEnsemble(256, (21, 21, 36))
    ens.inject(1.0, (10, 10, 18))
    peaks = ens.run(od)            # od (B, n, 2) or (n, 2) -> int32 (B, n, 3)

A member computes what a float32 ``PoseCellNetwork`` of that shape computes (within 1e-5 of
the float64 oracle, the same peaks), whatever the size of the ensemble, its place in it and
the way a run is cut into launches.  The per-step control is the library's
``rs_pc_odom_control`` over the tables of ``filters.odometry_tables``, bit-identical to
``filters.step_control``.  Two deliberate differences from the single network (DESIGN
section 8): a LUT miss anywhere in a run raises ``KeyError`` naming member and step before
any device work, and non-finite odometry raises ``ValueError``.
"""
import ctypes
import threading

import numpy as np

from . import _lib
from . import filters as F
from .posecell_network import grid_cell, pc_params


class PoseCellEnsemble(_lib.HandleOwner):
    """B float32 pose-cell networks of shape (X, Y, TH) on one GPU.

    ``global_inhibition``: None (the reference's 0.2), a scalar, or one value per member.
    A new ensemble is all zeros.  Shapes whose LDS plan does not fit a compute unit, a
    dimension below 7 and ``precision='float64'`` raise ValueError before any device call.
    """

    def __init__(self, members, shape, global_inhibition=None, device=0, precision='float32'):
        if len(shape) != 3:
            raise TypeError('PoseCellEnsemble shape must be (X, Y, TH), got %r' % (shape,))
        self.shape = tuple(int(s) for s in shape)
        self._b = int(members)
        self.device = int(device)
        self.max_pc = None
        self._mutex = threading.Lock()
        if precision not in ('float32', np.float32):
            raise ValueError('PoseCellEnsemble is float32 only, got precision %r' % (precision,))
        if self._b < 1:
            raise ValueError('an ensemble needs one member at least, got %d' % self._b)
        if global_inhibition is None:
            inhib = np.full(self._b, F.PC_GLOBAL_INHIB, dtype=np.float64)
        else:
            inhib = np.ascontiguousarray(np.broadcast_to(np.asarray(global_inhibition, dtype=np.float64), (self._b,)))
        if not np.isfinite(inhib).all():
            raise ValueError('global_inhibition must be finite')
        self.global_inhibition = inhib
        lib = _lib.load()
        _lib.check(lib.rs_pce_fit(*self.shape, None))     # ValueError with the bytes needed
        self._lib = _lib.require_device()
        self.filter_table = F.FilterTable()
        self._table = np.ascontiguousarray(self.filter_table.filters, dtype=np.float64)
        self._odo_tables = F.odometry_tables(self.shape[2], self.filter_table)
        params = pc_params(_lib.RS_PREC_F32, F.PC_GLOBAL_INHIB, self._table)
        self._h = _lib.Handle.create(self._lib, 'rs_pce_create', 'rs_pce_destroy', self._b, *self.shape,
                                     ctypes.byref(params), _lib.ptr(inhib, ctypes.c_double), self.device)

    @staticmethod
    def fits(shape):
        """Whether a member of this shape fits a compute unit's LDS (no device needed)."""
        x, y, th = (int(s) for s in shape)
        return _lib.load().rs_pce_fit(x, y, th, None) == _lib.RS_OK

    @staticmethod
    def lds_bytes(shape):
        """The LDS one member's workgroup needs for this shape, in bytes."""
        x, y, th = (int(s) for s in shape)
        n = ctypes.c_size_t()
        _lib.load().rs_pce_fit(x, y, th, ctypes.byref(n))
        return n.value

    def __len__(self):
        return self._b

    # -- state ------------------------------------------------------------------
    @property
    def posecells(self):
        """Copy of every member's volume, float64 C order (B, X, Y, TH)."""
        out = np.empty((self._b,) + self.shape, dtype=np.float64)
        with self._mutex:
            _lib.check(self._lib.rs_pce_read(self._h, 0, self._b, _lib.ptr(out, ctypes.c_double)))
        return out

    def write(self, volumes, first=0):
        """Set the volumes of members ``first ..`` from an array (count, X, Y, TH) (rounded to
        float32); a non-finite value raises ValueError and changes nothing."""
        v = np.asarray(volumes, dtype=np.float64)
        if v.ndim != 4 or v.shape[1:] != self.shape:
            raise ValueError('volumes must have shape (count, %d, %d, %d), got %r' % (self.shape + (v.shape,)))
        v = np.ascontiguousarray(v)
        with self._mutex:
            _lib.check(self._lib.rs_pce_write(self._h, int(first), v.shape[0], _lib.ptr(v, ctypes.c_double)))

    def inject(self, energy, loc, members=None):
        """posecells[m][loc] += energy for every member, or for those of ``members``."""
        x, y, th = grid_cell(loc, self.shape, 'inject', 'inject expects a tuple (x, y, th)')
        who = [-1] if members is None else [int(m) for m in members]
        for m in who:
            if members is not None and not 0 <= m < self._b:
                raise IndexError('member %d outside the ensemble of %d' % (m, self._b))
        with self._mutex:
            for m in who:
                _lib.check(self._lib.rs_pce_inject(self._h, m, float(energy), x, y, th))

    def get_pc_max(self):
        """Each member's argmax cell (first maximum in C order), int32 (B, 3)."""
        out = np.empty((self._b, 3), dtype=np.int32)
        with self._mutex:
            _lib.check(self._lib.rs_pce_get_max(self._h, _lib.ptr(out, ctypes.c_int32)))
        return out

    # -- stepping ---------------------------------------------------------------
    def _control(self, od, shared):
        """Control arrays of ``od`` (members, n, 2): the library's rs_pc_odom_control, with
        filters.step_control for the steps outside its tables.  KeyError on a LUT miss."""
        members, n = od.shape[:2]
        th = self.shape[2]
        steps = members * n
        ox = np.empty((steps, th), dtype=np.int32)
        oy = np.empty((steps, th), dtype=np.int32)
        fidx = np.empty((steps, th), dtype=np.int32)
        zf = np.empty((steps, F.FILTER_LEN), dtype=np.float64)
        status = np.empty(steps, dtype=np.int32)
        flat = np.ascontiguousarray(od.reshape(steps, 2))
        i32 = ctypes.c_int32
        _lib.check(self._lib.rs_pc_odom_control(
            th, *F.table_args(self._odo_tables), steps, _lib.ptr(flat, ctypes.c_double), _lib.ptr(ox, i32),
            _lib.ptr(oy, i32), _lib.ptr(fidx, i32), _lib.ptr(zf, ctypes.c_double), _lib.ptr(status, i32)))
        for i in np.flatnonzero(status != _lib.RS_OK):
            where = 'every member, step %d' % i if shared else 'member %d, step %d' % (i // n, i % n)
            if status[i] == _lib.RS_ERR_CTL_RANGE:
                try:
                    ox[i], oy[i], fidx[i], zf[i], _ = F.step_control(flat[i, 0], flat[i, 1], th, self.filter_table)
                    continue
                except KeyError as e:
                    raise KeyError('%s: path-integration LUT miss %s' % (where, e.args[0],)) from None
            if status[i] == _lib.RS_ERR_LUT_KEY:
                try:
                    F.step_control(flat[i, 0], flat[i, 1], th, self.filter_table)
                except KeyError as e:
                    raise KeyError('%s: path-integration LUT miss %s' % (where, e.args[0],)) from None
                raise KeyError('%s: path-integration LUT miss' % where)  # pragma: no cover
            _lib.check(int(status[i]))
        return ox, oy, fidx, zf

    def run(self, odometry):
        """``n`` updates of every member with one host round trip.

        ``odometry``: (B, n, 2) rows (vtrans, vrot) per member, or (n, 2) for all members
        alike.  Returns int32 (B, n, 3), each step's max_pc; the last step's are kept in
        ``max_pc``.  A LUT miss in any member's step raises KeyError (naming member and
        step) and non-finite odometry ValueError, both before anything has run."""
        od = np.asarray(odometry, dtype=np.float64)
        if od.ndim == 2 and od.shape[1] == 2:
            shared = True
            od = od[None]
        elif od.ndim == 3 and od.shape[0] == self._b and od.shape[2] == 2:
            shared = False
        else:
            raise ValueError('odometry must have shape (%d, n, 2) or (n, 2), got %r' % (self._b, od.shape))
        if not np.isfinite(od).all():
            raise ValueError('odometry must be finite')
        n = od.shape[1]
        out = np.empty((self._b, n, 3), dtype=np.int32)
        if n == 0:
            return out
        ctl = self._control(od, shared)
        if shared:
            ctl = [np.ascontiguousarray(np.broadcast_to(a[None], (self._b,) + a.shape)) for a in ctl]
        ox, oy, fidx, zf = ctl
        i32 = ctypes.c_int32
        with self._mutex:
            _lib.check(self._lib.rs_pce_run(self._h, n, _lib.ptr(ox, i32), _lib.ptr(oy, i32), _lib.ptr(fidx, i32),
                                            _lib.ptr(zf, ctypes.c_double), _lib.ptr(out, i32)))
            self.max_pc = out[:, -1].copy()
        return out

    def set_timing(self, enable=True):
        """HIP events around the launches of every later run() (device_ms)."""
        _lib.check(self._lib.rs_pce_set_timing(self._h, 1 if enable else 0))

    def device_ms(self):
        """Device time of the last run's launches in ms; -1 when it ran untimed."""
        ms = ctypes.c_double()
        _lib.check(self._lib.rs_pce_last_ms(self._h, ctypes.byref(ms)))
        return ms.value
