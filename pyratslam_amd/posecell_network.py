"""Drop-in ``PoseCellNetwork`` backed by the MI355X kernels of libratslam_hip.

API of ``/root/reference/ratslam/posecell_network.py:22-353``: ``PoseCellNetwork(shape)``,
``update(v)`` -> ``max_pc`` (also stored as ``.max_pc``), ``inject(energy, loc)``,
``get_pc_max()``, ``.posecells`` (float64 ndarray, C order (X, Y, TH)), ``.shape``,
plus the filter helpers the reference exposes.  ``step(v)`` is an alias of
``update`` (the name BASELINE.json's north_star uses) and ``run(odometry)``
performs many updates with one host round trip.  ``get_pc_pose()``, ``update_pose(v)`` and
``run(odometry, poses=True)`` add the sub-cell pose ratslam-python returns where the
reference's ``get_pc_max`` is a placeholder: the packet's circular centroid (``pc_peak``).

The pose-cell volume lives on the GPU; ``.posecells`` copies it to the host
on access (and uploads on assignment).  The per-step control scalars are
derived on the host exactly as the reference derives them (``filters``), the
volume work runs in the step kernels of the handle's form: ``pc_excite_*`` + ``pc_path_*``, or
``pc_step_halo`` (``csrc/pc_rows.h``, ``pc_stream.h``, ``pc_cols.h``, ``pc_halo.h``; one translation
unit, ``csrc/posecell.hip``).
"""
import ctypes
import math
import threading
import weakref

import numpy as np

from . import _lib
from . import filters as F
from . import pc_peak

PC_DIM_XY = 21           # posecell_network.py:8 (unused by the reference too)
PC_DIM_TH = 36
PC_E_SIGMA = F.PC_E_SIGMA
PC_I_SIGMA = F.PC_I_SIGMA
PC_E_DIM = F.PC_E_DIM
PC_I_DIM = F.PC_I_DIM
PC_GLOBAL_INHIB = F.PC_GLOBAL_INHIB
PC_CELL_X_SIZE = F.PC_CELL_X_SIZE
PC_C_SIZE_TH = 2.0 * np.pi / PC_DIM_TH

_PRECISIONS = {'float32': _lib.RS_PREC_F32, np.float32: _lib.RS_PREC_F32,
               'float64': _lib.RS_PREC_F64, np.float64: _lib.RS_PREC_F64}


class _PinnedArrays:
    """Float64 arrays in pinned, GPU-visible host memory (rs_host_alloc), handed out
    one per ``.posecells`` read: the GPU writes the volume straight into the array
    the caller gets (rs_pc_read_pinned), so the readback needs no host-side copy.
    Each array owns its block until it is garbage-collected, when the block goes
    back to the free list (the caller's arrays never alias one another).  At most
    ``cap`` blocks exist at once: a caller that keeps every volume (a history list)
    gets ordinary pageable arrays past that (``array`` returns None), so pinned host
    memory stays bounded."""

    CAP = 8

    def __init__(self, lib, n, cap=CAP):
        self._lib, self._n, self._cap = lib, n, cap
        self._free = []
        self._blocks = 0
        # reentrant: a cyclic GC run inside a locked section can finalise one of this
        # pool's arrays on the same thread, and _release takes the lock again
        self._lock = threading.RLock()

    def array(self, shape):
        with self._lock:
            ptr = self._free.pop() if self._free else None
            if ptr is None:
                if self._blocks >= self._cap:
                    return None, None
                self._blocks += 1
        if ptr is None:
            p = ctypes.c_void_p()
            st = self._lib.rs_host_alloc(8 * self._n, ctypes.byref(p))
            if st != _lib.RS_OK:
                with self._lock:
                    self._blocks -= 1
                _lib.check(st)
            ptr = p.value
        view = (ctypes.c_double * self._n).from_address(ptr)
        weakref.finalize(view, self._release, ptr).atexit = False  # the process frees it at exit
        return np.frombuffer(view, dtype=np.float64).reshape(shape), ptr

    def _release(self, ptr):
        with self._lock:
            if not self._closed:
                self._free.append(ptr)
                return
        self._lib.rs_host_free(ctypes.c_void_p(ptr))  # an array that outlived its network

    _closed = False

    def close(self):
        empty = []   # allocated before the lock is taken
        with self._lock:
            self._closed = True
            free, self._free = self._free, empty
        for ptr in free:
            self._lib.rs_host_free(ctypes.c_void_p(ptr))


def round_up(x):  # posecell_network.py:19-20
    return math.ceil(x) if x > 0 else math.floor(x)


def grid_cell(loc, shape, what, not_a_tuple):
    """The cell ``(x, y, th)`` of a grid that ``loc`` names: a tuple only (TypeError
    ``not_a_tuple`` for a list, which the reference would fancy-index whole planes with,
    posecell_network.py:324), indexed as numpy indexes -- negative indices count from the
    end -- and an IndexError '<what> location ... outside grid ...' outside the grid."""
    if isinstance(loc, list):
        raise TypeError(not_a_tuple)
    x, y, th = (int(v) for v in loc)
    X, Y, TH = shape
    x, y, th = x + X if x < 0 else x, y + Y if y < 0 else y, th + TH if th < 0 else th
    if not (0 <= x < X and 0 <= y < Y and 0 <= th < TH):
        raise IndexError('%s location %r outside grid %r' % (what, loc, shape))
    return x, y, th


def pc_params(precision, global_inhibition, table):
    """``rs_pc_params`` of the separable kernel factors and the filter table ``table``
    (float64, C order; the caller keeps it alive until the create call has returned)."""
    ge, gi, scale = F.separable_factors()
    params = _lib.PcParams()
    params.precision = precision
    params.global_inhibition = global_inhibition
    params.ge[:] = list(ge)
    params.gi[:] = list(gi)
    params.k_scale = scale
    params.nfilters = table.shape[0]
    params.xy_filters = _lib.ptr(table, ctypes.c_double)
    return params


class PoseCellNetwork(_lib.HandleOwner):
    """Continuous-attractor pose-cell network on one GPU.

    ``precision``: 'float32' (default; activations within 1e-5 of the float64
    reference) or 'float64'.  ``device``: HIP device ordinal.  ``readback``: 'lazy'
    (default: ``.posecells`` exports the volume when read) or 'eager' (every
    ``update()`` also exports the new volume into a pinned array before its one host
    sync, and the next ``.posecells`` read returns that array: the ROS node's
    update-then-publish step, ros_simulate.py:134-145, as one round trip).
    ``cells_to_avg``: radius (1 .. 3) of the wrapped box the sub-cell pose is averaged over
    (``get_pc_pose``, ``update_pose``, ``run(poses=True)``; ratslam-python's PC_CELLS_TO_AVG);
    a grid too small for the box raises ValueError when a pose is first asked for.
    Extra keyword arguments are accepted and ignored, like the reference (:24).
    """

    AT_PEAK = 'peak'   # run(injections=...): the first maximum of the state at that point

    def __init__(self, shape, precision='float32', device=0, readback='lazy',
                 cells_to_avg=pc_peak.CELLS_TO_AVG, **kwargs):
        if readback not in ('lazy', 'eager'):
            raise ValueError("readback must be 'lazy' or 'eager', got %r" % (readback,))
        self._eager = readback == 'eager'
        if int(cells_to_avg) != cells_to_avg or not 1 <= cells_to_avg <= pc_peak.MAX_CELLS_TO_AVG:
            raise ValueError('cells_to_avg must be 1, 2 or 3, got %r' % (cells_to_avg,))
        self.cells_to_avg = int(cells_to_avg)
        self._peak_ready = False   # the weights are uploaded when a pose is first asked for
        # run(poses=True) that raised the reference's LUT KeyError at step s: the (s, 3) poses
        # of the steps before it (the call's return value is lost to the exception)
        self.last_poses = None
        self.last_injection_cells = None   # run(injections=...): the cells of its last call
        self._fresh = None   # eager: the volume exported by the last update()
        if len(shape) != 3:
            raise TypeError('PoseCellNetwork shape must be (X, Y, TH), got %r' % (shape,))
        self.shape = tuple(int(s) for s in shape)
        self.precision = 'float32' if _PRECISIONS[precision] == _lib.RS_PREC_F32 else 'float64'
        self.device = int(device)
        self.global_inhibition = PC_GLOBAL_INHIB
        self.pc_vtrans_scale = PC_CELL_X_SIZE
        self.pc_vrot_scale = 2.0 * np.pi / self.shape[2]
        self.kernel_3d = F.kernel_3d()
        # the reference's unused attributes (posecell_network.py:30-32)
        self.kernel_2d = F.diff_gaussian(order=2)
        self.kernel_1d = F.diff_gaussian(order=1)
        self.kernel_1d_sep = F.diff_gaussian_separable()
        self.filter_table = F.FilterTable()
        self.filter_dict_2d = self.filter_table.dict
        self.filter_dict_2d_precision = F.LUT_PRECISION
        self.max_pc = None
        self._max_valid = False
        self._mutex = threading.Lock()
        self._pinned = None
        self._lib = _lib.require_device()
        self._table = np.ascontiguousarray(self.filter_table.filters, dtype=np.float64)
        params = pc_params(_PRECISIONS[precision], self.global_inhibition, self._table)
        self._h = _lib.Handle.create(self._lib, 'rs_pc_create', 'rs_pc_destroy', *self.shape,
                                     ctypes.byref(params), self.device)
        # fast path of update(): raw addresses, preallocated output
        self._update = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p)(('rs_pc_update', self._lib))
        self._out3 = np.empty(3, dtype=np.int32)
        self._out3_addr = self._out3.ctypes.data
        self._upload_odometry_tables()
        self._update_odom = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_double,
                                             ctypes.c_double, ctypes.c_void_p)(
            ('rs_pc_update_odom', self._lib))
        self._update_odom_read = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_double,
                                                  ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p)(
            ('rs_pc_update_odom_read', self._lib))

    def _upload_odometry_tables(self):
        """Tables for the library-side control of update()/run() (filters.odometry_tables)."""
        self._odo_tables = F.odometry_tables(self.shape[2], self.filter_table)
        _lib.check(self._lib.rs_pc_set_odometry_tables(self._h, *F.table_args(self._odo_tables)))

    # -- lifetime ---------------------------------------------------------------
    def _close_more(self):
        if getattr(self, '_pinned', None) is not None:
            self._pinned.close()
            self._pinned = None

    # -- state ------------------------------------------------------------------
    @property
    def posecells(self):
        """Copy of the activity volume, float64 C order (X, Y, TH) (posecell_network.py:27).

        The GPU writes it straight into a fresh pinned host array (no host-side copy;
        ros_simulate.py:140,145 reads it after every update)."""
        with self._mutex:
            if self._fresh is not None:   # exported by the last update() (readback='eager')
                out, self._fresh = self._fresh, None
                return out
            out, ptr = self._pinned_array()
            if out is None:   # the pinned pool is all held by the caller: pageable copy
                out = np.empty(self.shape, dtype=np.float64)
                _lib.check(self._lib.rs_pc_read(self._h, _lib.ptr(out, ctypes.c_double)))
            else:
                _lib.check(self._lib.rs_pc_read_pinned(self._h, ctypes.c_void_p(ptr)))
        return out

    def _pinned_array(self):
        if self._pinned is None:
            self._pinned = _PinnedArrays(self._lib, int(np.prod(self.shape)))
        return self._pinned.array(self.shape)

    @posecells.setter
    def posecells(self, value):
        v = np.asarray(value)
        if v.shape != self.shape:
            raise TypeError('posecells must have shape %r, got %r' % (self.shape, v.shape))
        v = np.ascontiguousarray(v, dtype=np.float64)
        with self._mutex:
            self._fresh = None
            _lib.check(self._lib.rs_pc_write(self._h, _lib.ptr(v, ctypes.c_double)))
            self._max_valid = False

    def total(self):
        t = ctypes.c_double()
        with self._mutex:
            _lib.check(self._lib.rs_pc_total(self._h, ctypes.byref(t)))
        return t.value

    # -- reference API ----------------------------------------------------------
    def inject(self, energy, loc):
        """posecells[loc] += energy for one cell ``loc = (x, y, th)`` (posecell_network.py:322-324)."""
        x, y, th = grid_cell(loc, self.shape, 'inject',
                             'inject expects a tuple (x, y, th); the reference would fancy-index '
                             'whole planes with a list (posecell_network.py:324)')
        with self._mutex:
            self._fresh = None
            _lib.check(self._lib.rs_pc_inject(self._h, float(energy), x, y, th))
            self._max_valid = False

    def get_pc_max(self):
        """Argmax cell (first maximum in C order) (posecell_network.py:317-319)."""
        with self._mutex:
            if self._max_valid:
                return self.max_pc
            out = np.empty(3, dtype=np.int32)
            _lib.check(self._lib.rs_pc_get_max(self._h, _lib.ptr(out, ctypes.c_int32)))
        return tuple(int(v) for v in out)

    # -- sub-cell pose (pc_peak) --------------------------------
    def _peak_tables(self):
        """Upload the centroid's sin / cos weights on first use (under the mutex)."""
        if not self._peak_ready:
            pc_peak.check_radius(self.shape, self.cells_to_avg)   # ValueError before any device call
            tabs = pc_peak.peak_tables(self.shape)
            _lib.check(self._lib.rs_pc_set_peak_tables(
                self._h, self.cells_to_avg, *(_lib.ptr(t, ctypes.c_double) for t in tabs)))
            self._peak_sums = np.empty(6, dtype=np.float64)
            self._peak_ready = True

    def get_pc_peak(self):
        """``(cell, sums)``: the stored state's first maximum and the rule's six sums of the
        box round it (rs_pc_get_peak)."""
        out = np.empty(3, dtype=np.int32)
        sums = np.empty(6, dtype=np.float64)
        with self._mutex:
            self._peak_tables()
            _lib.check(self._lib.rs_pc_get_peak(self._h, _lib.ptr(out, ctypes.c_int32),
                                                _lib.ptr(sums, ctypes.c_double)))
        return tuple(int(v) for v in out), sums

    def get_pc_pose(self):
        """Sub-cell pose ``(x, y, th)`` in cell units: the circular centroid of the activity
        within ``cells_to_avg`` cells of the first maximum."""
        cell, sums = self.get_pc_peak()
        return pc_peak.pose_from_sums(sums, cell, self.shape)

    def update_pose(self, v=(0.0, 0.0)):
        """``update(v)`` that returns the sub-cell pose after the step (and sets ``max_pc``):
        the centroid is taken on the GPU behind the step, one host round trip."""
        od = np.array([[float(v[0]), float(v[1])]])
        with self._mutex:
            self._peak_tables()
            self._fresh = None
            st = self._lib.rs_pc_update_odom_peak(self._h, od[0, 0], od[0, 1], _lib.ptr(self._out3, ctypes.c_int32),
                                                  _lib.ptr(self._peak_sums, ctypes.c_double))
            if st != _lib.RS_ERR_CTL_RANGE:
                self._settle(st, od, self._out3.reshape(1, 3))
                return pc_peak.pose_from_sums(self._peak_sums, self.max_pc, self.shape)
        _, poses = self._run_host_control(od, poses=True)
        return tuple(float(x) for x in poses[0])

    def _poses(self, maxes, sums):
        return np.array([pc_peak.pose_from_sums(s, m, self.shape) for m, s in zip(maxes, sums)],
                        dtype=np.float64).reshape(-1, 3)

    def _settle(self, st, od, out, miss=0, sums=None, behind=False, launch=None, launch_empty=False):
        """What the status ``st`` of an odometry call means, for every entry point (call with
        the mutex held).  The call ran the rows of ``od`` and wrote each finished step's
        max_pc to ``out`` (and its six sums to ``sums``, where poses were asked for).

        RS_OK: every step counts.  RS_ERR_LUT_KEY at step ``miss``: the steps before it count
        (steps 1-4 of the failing one ran too), and the reference's KeyError((k, k)) is
        raised by deriving that row's control here; ``last_poses`` keeps the poses of the
        steps that count.  RS_ERR_CTL_RANGE, odometry outside the library's control tables:
        the control is computed here in NumPy (filters.batch_control) and handed to the
        control-taking entry point, ``launch(steps, ox, oy, rows, zf)`` -> status (not called
        for no steps unless ``launch_empty``); after a LUT miss of that control, the steps
        before it and rs_pc_excite, then as for RS_ERR_LUT_KEY.  Anything else raises through
        ``_lib.check``, the state as it was.

        ``max_pc`` is that of the last step that counts; the cached maximum is valid only if
        a step ran, none missed and nothing was injected ``behind`` the last one."""
        if st == _lib.RS_OK:
            miss = None
        elif st == _lib.RS_ERR_CTL_RANGE:
            ox, oy, rows, zf, miss = F.batch_control(od, self.shape[2], self.filter_table)
            todo = len(od) if miss is None else miss
            if todo > 0 or launch_empty:
                i32 = ctypes.c_int32
                _lib.check(launch(todo, _lib.ptr(ox, i32), _lib.ptr(oy, i32), _lib.ptr(rows, i32),
                                  _lib.ptr(zf, ctypes.c_double)))
            if miss is not None:
                # the reference raises inside path_integration, after steps 1-4 ran
                _lib.check(self._lib.rs_pc_excite(self._h))
        elif st != _lib.RS_ERR_LUT_KEY:
            _lib.check(st)
        done = len(od) if miss is None else miss
        if done > 0:
            self.max_pc = tuple(int(v) for v in out[done - 1])
        self._max_valid = miss is None and done > 0 and not behind
        if miss is not None:
            if sums is not None:
                self.last_poses = self._poses(out[:done], sums[:done])
            F.step_control(od[miss, 0], od[miss, 1], self.shape[2], self.filter_table)
            raise KeyError('LUT miss at step %d' % miss)  # pragma: no cover

    def update(self, v=(0.0, 0.0)):
        """One network step (posecell_network.py:326-353); returns and stores max_pc.

        One FFI call: the library derives path_integration's control from (vtrans,
        vrot) bit-identically to filters.step_control (rs_pc_update_odom)."""
        vtrans, vrot = float(v[0]), float(v[1])
        out = self._out3
        with self._mutex:
            self._fresh = None
            arr, ptr = self._pinned_array() if self._eager else (None, None)
            if arr is not None:
                st = self._update_odom_read(self._h, vtrans, vrot, self._out3_addr, ptr)
                if st == _lib.RS_OK:
                    self._fresh = arr
            else:
                st = self._update_odom(self._h, vtrans, vrot, self._out3_addr)
            if st == _lib.RS_OK:
                self.max_pc = (int(out[0]), int(out[1]), int(out[2]))
                self._max_valid = True
                return self.max_pc
            return self._update_settle(st, vtrans, vrot)

    def _update_settle(self, st, vtrans, vrot):
        """update() after a status other than RS_OK: _settle, with rs_pc_update for the
        control computed here."""
        self._settle(st, np.array([[vtrans, vrot]]), self._out3.reshape(1, 3),
                     launch=lambda _, *ctl: self._update(self._h, *ctl, self._out3_addr))
        return self.max_pc

    def _update_host_control(self, vtrans, vrot):
        """update() with the control computed here in NumPy (filters.step_control) and
        handed to rs_pc_update: for odometry outside the library's control tables."""
        with self._mutex:
            return self._update_settle(_lib.RS_ERR_CTL_RANGE, vtrans, vrot)

    step = update

    def run(self, odometry, poses=False, injections=None):
        """``update`` for every row (vtrans, vrot) of ``odometry``; one host round trip.

        Returns an int32 array (n, 3) of max_pc per step; with ``poses=True``,
        ``(maxes, poses)``, poses a float64 (n, 3) array of each step's sub-cell pose.
        A LUT KeyError at step s leaves the state the reference would (steps < s done,
        then steps 1-4 of s).

        ``injections``: a sequence of ``(step, energy, loc)``, steps non-decreasing in
        ``0 .. n``; injection i is applied in front of step ``step`` (``n``: behind the last
        one) exactly as ``inject(energy, cell)`` between two ``update`` calls would be.
        ``loc`` is a tuple ``(x, y, th)`` (``inject``'s rules), ``PoseCellNetwork.AT_PEAK``
        (what ``get_pc_max()`` would return at that point) or ``('same', k)`` with k < i (the
        cell injection k resolved to).  The resolved cells come back as an ``(ni, 3)`` int32
        array, last in the returned tuple; after a LUT KeyError they are in
        ``last_injection_cells``, ``(-1, -1, -1)`` for the injections behind the failing step.
        """
        od = np.ascontiguousarray(np.asarray(odometry, dtype=np.float64).reshape(-1, 2))
        n = od.shape[0]
        if injections is not None:
            return self._run_inject(od, poses, injections)
        if poses:
            return self._run_poses(od)
        if n == 1 and not self._eager:
            # one step (the ROS node's queue drain, usually): update()'s prebound call,
            # the same library step and the same KeyError / host-control fallbacks
            return np.array([self.update(od[0])], dtype=np.int32)
        out = np.empty((n, 3), dtype=np.int32)
        bad = ctypes.c_int(-1)
        with self._mutex:
            self._fresh = None
            st = self._lib.rs_pc_run_odom(self._h, n, _lib.ptr(od, ctypes.c_double),
                                          _lib.ptr(out, ctypes.c_int32), ctypes.byref(bad))
            self._settle(st, od, out, bad.value, launch=self._host_run(out))
        return out

    def _run_poses(self, od):
        """run(poses=True): rs_pc_run_odom_peaks."""
        n = od.shape[0]
        out = np.empty((n, 3), dtype=np.int32)
        sums = np.empty((n, 6), dtype=np.float64)
        bad = ctypes.c_int(-1)
        with self._mutex:
            self._peak_tables()
            self._fresh = None
            st = self._lib.rs_pc_run_odom_peaks(self._h, n, _lib.ptr(od, ctypes.c_double),
                                                _lib.ptr(out, ctypes.c_int32), _lib.ptr(sums, ctypes.c_double),
                                                ctypes.byref(bad))
            # (after a LUT miss the poses of the steps before it stay readable: last_poses)
            self._settle(st, od, out, bad.value, sums, launch=self._host_run(out, sums))
        return out, self._poses(out, sums)

    def _injection_arrays(self, n, injections):
        """``injections`` as rs_pc_run_odom_inject's arrays (ValueError / IndexError before
        any device work, as the library itself refuses what is left)."""
        inj = list(injections)
        step = np.empty(len(inj), dtype=np.int32)
        energy = np.empty(len(inj), dtype=np.float64)
        loc = np.zeros((len(inj), 3), dtype=np.int32)
        for i, (st, e, where) in enumerate(inj):
            if int(st) != st or not 0 <= st <= n:
                raise ValueError('injection %d: step %r outside 0 .. %d' % (i, st, n))
            if i and st < step[i - 1]:
                raise ValueError('injection %d: step %d after step %d' % (i, st, step[i - 1]))
            step[i], energy[i] = st, float(e)
            if isinstance(where, str) and where == self.AT_PEAK:
                loc[i, 0] = _lib.RS_PC_INJ_AT_PEAK
            elif isinstance(where, tuple) and len(where) == 2 and where[0] == 'same':
                k = where[1]
                if int(k) != k or not 0 <= k < i:
                    raise ValueError("injection %d: ('same', %r) is no earlier injection" % (i, k))
                loc[i, :2] = _lib.RS_PC_INJ_SAME_AS, k
            else:
                loc[i] = grid_cell(where, self.shape, 'injection %d:' % i,
                                   'an injection location is a tuple (x, y, th)')
        return step, energy, loc

    def _run_inject(self, od, poses, injections):
        """run(injections=...): rs_pc_run_odom_inject, rs_pc_run_inject with host control."""
        n = od.shape[0]
        step, energy, loc = self._injection_arrays(n, injections)
        ni = len(step)
        out = np.empty((n, 3), dtype=np.int32)
        cells = np.full((ni, 3), -1, dtype=np.int32)
        sums = np.empty((n, 6), dtype=np.float64) if poses else None
        inj_args = (ni, _lib.ptr(step, ctypes.c_int32), _lib.ptr(energy, ctypes.c_double),
                    _lib.ptr(loc, ctypes.c_int32))
        out_args = (_lib.ptr(out, ctypes.c_int32), _lib.ptr(cells, ctypes.c_int32),
                    _lib.ptr(sums, ctypes.c_double) if poses else None)
        bad = ctypes.c_int(-1)
        self.last_injection_cells = cells

        def host(todo, *ctl):
            # (a LUT miss: the steps before it with the injections up to it, then steps 1-4)
            keep = int(np.searchsorted(step, todo, side='right'))
            return self._lib.rs_pc_run_inject(self._h, todo, *ctl, keep, *inj_args[1:], *out_args)

        with self._mutex:
            if poses:
                self._peak_tables()
            self._fresh = None
            st = self._lib.rs_pc_run_odom_inject(self._h, n, _lib.ptr(od, ctypes.c_double), *inj_args, *out_args,
                                                 ctypes.byref(bad))
            # (an injection behind the last step has changed the state since its peak was taken)
            self._settle(st, od, out, bad.value, sums, behind=bool(ni and step[-1] == n),
                         launch=host, launch_empty=True)
        return (out, self._poses(out, sums), cells) if poses else (out, cells)

    def _host_run(self, out, sums=None):
        """_settle's ``launch`` of run(): rs_pc_run, or rs_pc_run_peaks into ``sums``."""
        def launch(todo, *ctl):
            if sums is None:
                return self._lib.rs_pc_run(self._h, todo, *ctl, _lib.ptr(out, ctypes.c_int32))
            self._peak_tables()
            return self._lib.rs_pc_run_peaks(self._h, todo, *ctl, _lib.ptr(out, ctypes.c_int32),
                                             _lib.ptr(sums, ctypes.c_double))
        return launch

    def _run_host_control(self, od, poses=False):
        """run() with the control computed here (filters.batch_control) and handed to
        rs_pc_run (rs_pc_run_peaks with ``poses``): for odometry outside the library's
        control tables."""
        out = np.empty((od.shape[0], 3), dtype=np.int32)
        sums = np.empty((od.shape[0], 6), dtype=np.float64) if poses else None
        with self._mutex:
            self._settle(_lib.RS_ERR_CTL_RANGE, od, out, sums=sums, launch=self._host_run(out, sums))
        return (out, self._poses(out, sums)) if poses else out

    def device_ms(self):
        """Device time (HIP events) of the last update/run, in ms; recorded only while
        profiling is enabled (``set_profiling``), else 0."""
        ms = ctypes.c_double()
        _lib.check(self._lib.rs_pc_last_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def step_form(self):
        """Step kernels in use: 'rows', 'cols', 'halo' or 'stream' (rs_pc_step_form)."""
        return self._lib.rs_pc_step_form(self._h).decode()

    def set_profiling(self, enable=True, per_kernel=True):
        """HIP events around each update()/run() (device_ms) and, with per_kernel, around
        every launch too (kernel_ms; those events add gaps between the kernels)."""
        _lib.check(self._lib.rs_pc_set_profiling(self._h, 0 if not enable else (1 if per_kernel else 2)))

    def kernel_ms(self):
        """Kernel times of the last run (profiling on, per_kernel=True), as
        rs_pc_kernel_ms returns them: (excite_ms, path_ms) summed over the steps for
        the two-launch forms (rows, cols, stream); for the halo form
        (step_ms, finish_ms): the step kernels summed, then the one pc_halo_finish."""
        ms = np.zeros(2)
        _lib.check(self._lib.rs_pc_kernel_ms(self._h, _lib.ptr(ms, ctypes.c_double)))
        return float(ms[0]), float(ms[1])

    # -- filter helpers of the reference class (host-side, NumPy) -----------------
    def diff_gaussian(self, dim_e, dim_i, sigma_e, sigma_i, order=3):
        return F.diff_gaussian(dim_e, dim_i, sigma_e, sigma_i, order)

    def diff_gaussian_separable(self, dim_e, dim_i, sigma_e, sigma_i):
        return F.diff_gaussian_separable(dim_e, dim_i, sigma_e, sigma_i)

    def diff_gaussian_offset_2d(self, sigma_e, sigma_i, shape=(7, 7), origin=(0, 0)):
        return F.filter_2d(origin, sigma_e, sigma_i, shape)

    def diff_gaussian_offset_1d(self, sigma_e, sigma_i, size=7, origin=0):
        return np.array(F.filter_1d(origin, sigma_e, sigma_i, size))

    def build_diff_gaussian_set_2d(self, sigma_e, sigma_i, shape=(7, 7), precision=1):
        if precision != 1 or (sigma_e, sigma_i, tuple(shape)) != (PC_E_SIGMA, PC_I_SIGMA, (7, 7)):
            span = range(-5 * precision, 5 * precision)
            return {(x, y): F.filter_2d((x // (precision * 10), y // (precision * 10)),
                                        sigma_e, sigma_i, shape) for x in span for y in span}
        return dict(self.filter_dict_2d)

    def filters_from_origins_approx(self, origins, shape=(7, 7)):
        """LUT lookup per layer (posecell_network.py:244-250); KeyError on a miss."""
        origins = np.asarray(origins)
        keys = np.trunc(origins[0] * self.filter_dict_2d_precision).astype(np.int64)
        rows = self.filter_table.rows_for_keys(keys)
        return np.ascontiguousarray(np.moveaxis(self.filter_table.filters[rows], 0, -1))
