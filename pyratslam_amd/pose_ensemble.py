"""``PoseCellEnsemble``: many small pose-cell networks of one shape stepped side by side,
each by one workgroup out of a compute unit's LDS (``csrc/pose_ensemble.hip``, DESIGN
section 35).

    ens = PoseCellEnsemble(256, (21, 21, 36))
    ens.inject(1.0, (10, 10, 18))
    peaks = ens.run(od)            # od (B, n, 2) or (n, 2) -> int32 (B, n, 3)

With ``cells_to_avg`` the ensemble also gives the sub-cell pose (``get_pc_pose``,
``run(od, poses=True)``), and ``run(od, injections=[(member, step, energy, loc), ...])`` applies
view-template feedback inside the batch: both stay in LDS, neither adds a
launch or a host round trip.

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
from . import pc_peak
from .posecell_network import grid_cell, pc_params


F32_ROUNDS_TO_INF = float.fromhex('0x1.ffffffp127')   # the midpoint of float32's largest value and 2^128


class PoseCellEnsemble(_lib.HandleOwner):
    """B float32 pose-cell networks of shape (X, Y, TH) on one GPU.

    ``global_inhibition``: None (the reference's 0.2), a scalar, or one value per member.
    ``cells_to_avg``: None, or the radius (1 .. 3) of the wrapped box the sub-cell pose is
    averaged over (``get_pc_pose``, ``run(poses=True)``); its weights are uploaded at create.
    A new ensemble is all zeros.  Shapes whose LDS plan does not fit a compute unit, a
    dimension below 7, ``precision='float64'`` and a ``cells_to_avg`` whose box the grid does
    not hold raise ValueError before any device call.
    """

    AT_PEAK = 'peak'   # run(injections=...): the member's first maximum at that point

    def __init__(self, members, shape, global_inhibition=None, device=0, precision='float32', cells_to_avg=None):
        if len(shape) != 3:
            raise TypeError('PoseCellEnsemble shape must be (X, Y, TH), got %r' % (shape,))
        self.shape = tuple(int(s) for s in shape)
        self._b = int(members)
        self.device = int(device)
        self.max_pc = None
        self.last_sums = None
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
        self.cells_to_avg = None if cells_to_avg is None else pc_peak.check_radius(self.shape, cells_to_avg)
        self._lib = _lib.require_device()
        self.filter_table = F.FilterTable()
        self._table = np.ascontiguousarray(self.filter_table.filters, dtype=np.float64)
        self._odo_tables = F.odometry_tables(self.shape[2], self.filter_table)
        params = pc_params(_lib.RS_PREC_F32, F.PC_GLOBAL_INHIB, self._table)
        self._h = _lib.Handle.create(self._lib, 'rs_pce_create', 'rs_pce_destroy', self._b, *self.shape,
                                     ctypes.byref(params), _lib.ptr(inhib, ctypes.c_double), self.device)
        if self.cells_to_avg is not None:
            tabs = pc_peak.peak_tables(self.shape)
            _lib.check(self._lib.rs_pce_set_peak_tables(self._h, self.cells_to_avg,
                                                        *(_lib.ptr(t, ctypes.c_double) for t in tabs)))

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

    def _need_tables(self):
        if self.cells_to_avg is None:
            raise ValueError('the sub-cell pose needs PoseCellEnsemble(..., cells_to_avg=r)')

    def _poses(self, cells, sums):
        flat = [pc_peak.pose_from_sums(s, c, self.shape) for c, s in zip(cells.reshape(-1, 3), sums.reshape(-1, 6))]
        return np.array(flat, dtype=np.float64).reshape(cells.shape)

    def get_pc_peak(self):
        """``(cells, sums)``: each member's stored first maximum, int32 (B, 3), and the rule's
        six sums of the box round it, float64 (B, 6) (rs_pce_get_peak)."""
        self._need_tables()
        out = np.empty((self._b, 3), dtype=np.int32)
        sums = np.empty((self._b, 6), dtype=np.float64)
        with self._mutex:
            _lib.check(self._lib.rs_pce_get_peak(self._h, _lib.ptr(out, ctypes.c_int32), _lib.ptr(sums, ctypes.c_double)))
        return out, sums

    def get_pc_pose(self):
        """Each member's sub-cell pose ``(x, y, th)`` in cell units, float64 (B, 3): the circular
        centroid of the activity within ``cells_to_avg`` cells of its first maximum."""
        return self._poses(*self.get_pc_peak())

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

    @classmethod
    def injection_arrays(cls, members, shape, n, injections):
        """``injections`` of ``run`` as rs_pce_run_inject's arrays ``(member, step, energy, loc)``,
        a ``None`` member expanded to one entry per member (ValueError / IndexError as
        ``PoseCellNetwork.run`` words them; no device needed)."""
        inj = [tuple(e) for e in injections]
        first = np.cumsum([0] + [members if e[0] is None else 1 for e in inj])   # entry j's first expanded index
        member = np.empty(first[-1], dtype=np.int32)
        step = np.empty(first[-1], dtype=np.int32)
        energy = np.empty(first[-1], dtype=np.float64)
        loc = np.zeros((first[-1], 3), dtype=np.int32)
        last = np.zeros(members, dtype=np.int64)   # each member's latest step so far
        everyone = np.arange(members)
        for j, (who, st, e, where) in enumerate(inj):
            if who is not None and (int(who) != who or not 0 <= who < members):
                raise IndexError('injection %d: member %r outside the ensemble of %d' % (j, who, members))
            if int(st) != st or not 0 <= st <= n:
                raise ValueError('injection %d: step %r outside 0 .. %d' % (j, st, n))
            if not abs(float(e)) < F32_ROUNDS_TO_INF:
                raise ValueError('injection %d: energy %r is not a finite float32' % (j, e))
            same = None
            if isinstance(where, str) and where == cls.AT_PEAK:
                cell = (_lib.RS_PC_INJ_AT_PEAK, 0, 0)
            elif isinstance(where, tuple) and len(where) == 2 and where[0] == 'same':
                same = where[1]
                if int(same) != same or not 0 <= same < j:
                    raise ValueError("injection %d: ('same', %r) is no earlier injection" % (j, same))
            else:
                cell = grid_cell(where, shape, 'injection %d:' % j, 'an injection location is a tuple (x, y, th)')
            ms = everyone if who is None else everyone[int(who):int(who) + 1]   # (an array at a time: B may be large)
            late = ms[last[ms] > st]
            if late.size:
                raise ValueError('injection %d: step %d after step %d of member %d' % (j, st, last[late[0]], late[0]))
            last[ms] = st
            at = slice(first[j], first[j + 1])
            member[at], step[at], energy[at] = ms, st, float(e)
            if same is None:
                loc[at] = cell
            else:
                other = ms if inj[same][0] is None else ms[ms != inj[same][0]]
                if inj[same][0] is not None and other.size:
                    raise ValueError("injection %d: ('same', %d) is an injection of another member" % (j, same))
                loc[at, 0] = _lib.RS_PC_INJ_SAME_AS
                loc[at, 1] = first[same] + (ms if inj[same][0] is None else 0)
        return member, step, energy, loc

    def run(self, odometry, poses=False, injections=None):
        """``n`` updates of every member with one host round trip.

        ``odometry``: (B, n, 2) rows (vtrans, vrot) per member, or (n, 2) for all members
        alike.  Returns int32 (B, n, 3), each step's max_pc; the last step's are kept in
        ``max_pc``.  A LUT miss in any member's step raises KeyError (naming member and
        step) and non-finite odometry ValueError, both before anything has run.

        ``poses=True`` (needs ``cells_to_avg``): also each step's sub-cell pose, float64
        (B, n, 3), taken on the GPU behind the step; the raw sums stay in ``last_sums``.

        ``injections``: a sequence of ``(member, step, energy, loc)``; ``member`` an index, or
        None for every member (one entry per member, in member order); the steps in ``0 .. n``
        and non-decreasing within each member.  An injection is applied in front of step
        ``step`` (``n``: behind the last one) exactly as ``inject(energy, cell, members=[m])``
        between two ``run`` calls would be.  ``loc`` is a tuple ``(x, y, th)`` (``inject``'s
        rules), ``PoseCellEnsemble.AT_PEAK`` (what ``get_pc_max()`` would return for the member
        at that point) or ``('same', k)``, k an earlier entry of this list for the same member
        (of a None entry: the same member's copy).  The resolved cells come back as an int32
        array, a row per expanded entry.  Returns ``peaks``, then ``poses`` if asked for, then
        the resolved cells if ``injections`` was given."""
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
        if poses:
            self._need_tables()
        inj = None if injections is None else self.injection_arrays(self._b, self.shape, n, injections)
        ni = 0 if inj is None else len(inj[0])
        out = np.empty((self._b, n, 3), dtype=np.int32)
        sums = np.empty((self._b, n, 6), dtype=np.float64) if poses else None
        cells = np.empty((ni, 3), dtype=np.int32)
        i32, f64 = ctypes.c_int32, ctypes.c_double
        ctl = [None] * 4
        if n > 0:
            ctl = self._control(od, shared)
            if shared:
                ctl = [np.ascontiguousarray(np.broadcast_to(a[None], (self._b,) + a.shape)) for a in ctl]
        ox, oy, fidx, zf = ctl
        if n > 0 or ni > 0:
            with self._mutex:
                if inj is None and not poses:
                    _lib.check(self._lib.rs_pce_run(self._h, n, _lib.ptr(ox, i32), _lib.ptr(oy, i32), _lib.ptr(fidx, i32),
                                                    _lib.ptr(zf, f64), _lib.ptr(out, i32)))
                else:
                    member, step, energy, loc = inj if ni else (None,) * 4
                    _lib.check(self._lib.rs_pce_run_inject(
                        self._h, n, _lib.ptr(ox, i32), _lib.ptr(oy, i32), _lib.ptr(fidx, i32), _lib.ptr(zf, f64), ni,
                        _lib.ptr(member, i32), _lib.ptr(step, i32), _lib.ptr(energy, f64), _lib.ptr(loc, i32),
                        _lib.ptr(out, i32), _lib.ptr(cells, i32), _lib.ptr(sums, f64)))
                if n > 0:
                    self.max_pc = out[:, -1].copy()
        result = (out,)
        if poses:
            self.last_sums = sums
            result += (self._poses(out, sums),)
        if inj is not None:
            result += (cells,)
        return result[0] if len(result) == 1 else result

    def set_timing(self, enable=True):
        """HIP events around the launches of every later run() (device_ms)."""
        _lib.check(self._lib.rs_pce_set_timing(self._h, 1 if enable else 0))

    def device_ms(self):
        """Device time of the last run's launches in ms; -1 when it ran untimed."""
        ms = ctypes.c_double()
        _lib.check(self._lib.rs_pce_last_ms(self._h, ctypes.byref(ms)))
        return ms.value
