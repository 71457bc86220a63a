"""``SimpleVisualOdometer``: the module the reference's ROS node imports and does not
ship (``from visual_odometer import SimpleVisualOdometer``, ``ros_simulate.py:5``;
constructed with no arguments at ``:90``; ``delta = self.vis_odom.update(im)`` per
frame, ``:119-122``; the ``(vtrans, vrot)`` deltas go to ``update_posecells`` as
they are, ``:163-165`` -- not divided by ``ODOM_FREQ``).

The reference fixes that interface only, so the arithmetic is defined here: the
scanline-profile odometer of the RatSLAM literature in exact integers, so that the
GPU (``csrc/visual_odometer.hip``) and NumPy agree bit for bit.

* region: rows ``[y0, y1)`` by columns ``[x0, x1)`` of a mono8 frame, one for
  ``trans`` and one for ``rot`` (default: the whole frame); ``R`` rows, ``Wd`` columns;
* ``profile``: ``prof[c] = sum_y frame[y, x0 + c]`` (uint32);
* ``shift_table``: against the previous frame's profile, for signed shifts ``s`` in
  ``[-(S-1), S-1]``, ``tab[s] = sum |cur[k] - prev[k + s]|`` over the ``Wd - |s|``
  valid ``k`` (uint32, at index ``s + S - 1``);
* ``select``: ``best = inf``, ``shift = 0``; for ``o = 0 .. S-1`` the candidates
  ``-o`` then ``+o``: ``v = float64(tab[s]) / float64((Wd - o) * R * 255)``, taken
  if ``v < best`` -- a tie keeps the smaller ``|s|``, the negative before the positive;
* ``vrot = shift_rot * rad_per_column``, ``vtrans = min(best_trans * vtrans_scale,
  vtrans_max)``, ``rad_per_column = math.radians(fov_deg) / im_w``.

A positive shift means the new frame is the old one moved by ``+s`` columns
(``new[k] == old[k + s]``): a positive heading change in ``synthetic.ros_stream``.
The first frame after construction or ``reset()`` returns ``(0.0, 0.0)``.

``fov_deg = 90``, ``vtrans_scale = 100`` and ``vtrans_max = 20`` are placeholders, in the
reference's own spirit ("TODO: put reasonable values here"): calibrate them for a
real camera.

``NumpyVisualOdometer`` is the restatement (no device); ``SimpleVisualOdometer`` runs
the profiles and tables on the GPU and has no CPU fallback.
"""
import ctypes
import math
import threading

import numpy as np

from . import _lib

MAX_SHIFT = 40
FOV_DEG = 90.0
VTRANS_SCALE = 100.0
VTRANS_MAX = 20.0
CHUNK_FRAMES = 256   # host frames per staging chunk of rs_vo_run (VO_CHUNK_FRAMES)


# -- the arithmetic ---------------------------------------------------------------
def profile(frame, rows, cols):
    """Column sums of ``frame[rows[0]:rows[1], cols[0]:cols[1]]`` as uint32."""
    return frame[rows[0]:rows[1], cols[0]:cols[1]].sum(axis=0, dtype=np.uint64).astype(np.uint32)


def shift_table(cur, prev, max_shift):
    """``tab[s + S - 1] = sum_k |cur[k] - prev[k + s]|`` for s in [-(S-1), S-1] (uint32)."""
    c = np.asarray(cur).astype(np.int64)
    p = np.asarray(prev).astype(np.int64)
    wd, S = c.size, int(max_shift)
    tab = np.empty(2 * S - 1, dtype=np.uint32)
    for s in range(-(S - 1), S):
        k0, k1 = max(0, -s), min(wd, wd - s)
        tab[s + S - 1] = np.abs(c[k0:k1] - p[k0 + s:k1 + s]).sum()
    return tab


def select(table, width, rows, max_shift=None):
    """The shift with the smallest normalised difference, and that difference
    (float64): candidates 0, -1, +1, -2, +2, ..., strict ``<``."""
    table = np.asarray(table)
    S = (table.size + 1) // 2 if max_shift is None else int(max_shift)
    best, shift = np.inf, 0
    for o in range(S):
        den = np.float64((width - o) * rows * 255)
        for s in ((0,) if o == 0 else (-o, o)):
            v = np.float64(table[s + S - 1]) / den
            if v < best:
                best, shift = v, s
    return shift, float(best)


def _region(r, n, name):
    lo, hi = (0, n) if r is None else (int(r[0]), int(r[1]))
    if not 0 <= lo < hi <= n:
        raise ValueError('%s [%d, %d) empty or outside [0, %d)' % (name, lo, hi, n))
    return lo, hi


class _Params:
    """Validated odometer geometry for one frame shape (the checks of rs_vo_create)."""

    def __init__(self, shape, trans_rows, trans_cols, rot_rows, rot_cols, max_shift, fov_deg,
                 vtrans_scale, vtrans_max):
        self.im_h, self.im_w = int(shape[0]), int(shape[1])
        if self.im_h <= 0 or self.im_w <= 0:
            raise ValueError('bad frame shape %r' % (shape,))
        self.S = int(max_shift)
        if not 1 <= self.S <= 64:
            raise ValueError('max_shift %d outside [1, 64]' % self.S)
        self.rows = [_region(trans_rows, self.im_h, 'trans rows'), _region(rot_rows, self.im_h, 'rot rows')]
        self.cols = [_region(trans_cols, self.im_w, 'trans columns'), _region(rot_cols, self.im_w, 'rot columns')]
        self.R = [r[1] - r[0] for r in self.rows]
        self.wd = [c[1] - c[0] for c in self.cols]
        for R, wd, name in zip(self.R, self.wd, ('trans', 'rot')):
            if wd < self.S:
                raise ValueError('%s region is %d columns wide, fewer than max_shift %d' % (name, wd, self.S))
            if R * 255 * wd >= 1 << 32:
                raise ValueError('%s region: rows * 255 * columns = %d does not fit 32 bits'
                                 % (name, R * 255 * wd))
        self.rad_per_column = math.radians(fov_deg) / self.im_w
        self.vtrans_scale = float(vtrans_scale)
        self.vtrans_max = float(vtrans_max)

    def c_struct(self):
        p = _lib.VoParams()
        (p.trans_y0, p.trans_y1), (p.rot_y0, p.rot_y1) = self.rows
        (p.trans_x0, p.trans_x1), (p.rot_x0, p.rot_x1) = self.cols
        p.max_shift = self.S
        p.rad_per_column = self.rad_per_column
        p.vtrans_scale = self.vtrans_scale
        p.vtrans_max = self.vtrans_max
        return p


class _OdometerBase:
    def __init__(self, trans_rows=None, trans_cols=None, rot_rows=None, rot_cols=None,
                 max_shift=MAX_SHIFT, fov_deg=FOV_DEG, vtrans_scale=VTRANS_SCALE,
                 vtrans_max=VTRANS_MAX):
        self._kw = dict(trans_rows=trans_rows, trans_cols=trans_cols, rot_rows=rot_rows,
                        rot_cols=rot_cols, max_shift=max_shift, fov_deg=fov_deg,
                        vtrans_scale=vtrans_scale, vtrans_max=vtrans_max)
        self.params = None       # set at the first frame, from its shape
        self._mutex = threading.Lock()

    def _check(self, frames):
        """uint8 (n, im_h, im_w), C-contiguous; the first frame fixes the shape."""
        f = np.asarray(frames)
        if f.dtype != np.uint8:
            raise TypeError('the odometer takes uint8 frames (mono8, ros_simulate.py:119-121); got %s' % f.dtype)
        if f.ndim != 3:
            raise ValueError('frames must be (n, im_h, im_w), got shape %r' % (f.shape,))
        if self.params is None:
            self._setup(f.shape[1:])
        if f.shape[1:] != (self.params.im_h, self.params.im_w):
            raise ValueError('frame shape %r differs from the first frame\'s %r'
                             % (f.shape[1:], (self.params.im_h, self.params.im_w)))
        return np.ascontiguousarray(f)

    def _setup(self, shape):
        self.params = _Params(shape, **self._kw)

    def update(self, im):
        """``SimpleVisualOdometer.update`` (ros_simulate.py:120): one mono8 frame ->
        ``(vtrans, vrot)`` as Python floats."""
        im = np.asarray(im)
        if im.ndim != 2:
            raise ValueError('update() takes one (im_h, im_w) frame, got shape %r' % (im.shape,))
        d = self.run(im[None])
        return float(d[0, 0]), float(d[0, 1])


class NumpyVisualOdometer(_OdometerBase):
    """The odometer in NumPy alone: the restatement the GPU class is checked against."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._prev = None

    def reset(self):
        self._prev = None

    def run(self, frames, tables=None, profiles=None):
        """``(n, 2)`` float64 deltas; optional lists collect each frame's two tables
        (``(2, 2S-1)`` uint32) and profiles (trans then rot, concatenated)."""
        f = self._check(frames)
        p = self.params
        out = np.zeros((f.shape[0], 2), dtype=np.float64)
        with self._mutex:
            for i in range(f.shape[0]):
                cur = [profile(f[i], p.rows[r], p.cols[r]) for r in range(2)]
                if self._prev is None:
                    tab = [np.zeros(2 * p.S - 1, dtype=np.uint32) for _ in range(2)]
                else:
                    tab = [shift_table(cur[r], self._prev[r], p.S) for r in range(2)]
                    _, best_t = select(tab[0], p.wd[0], p.R[0], p.S)
                    shift_r, _ = select(tab[1], p.wd[1], p.R[1], p.S)
                    out[i, 0] = min(best_t * p.vtrans_scale, p.vtrans_max)
                    out[i, 1] = float(shift_r) * p.rad_per_column
                self._prev = cur
                if tables is not None:
                    tables.append(np.stack(tab))
                if profiles is not None:
                    profiles.append(np.concatenate(cur))
        return out

    def close(self):
        pass


class SimpleVisualOdometer(_lib.HandleOwner, _OdometerBase):
    """The odometer on the GPU (``rs_vo_*``).  ``SimpleVisualOdometer()`` as the node
    constructs it; the handle is created at the first frame, from that frame's shape.

    Keyword arguments: ``trans_rows`` / ``trans_cols`` / ``rot_rows`` / ``rot_cols``
    (``(lo, hi)`` or None for the whole axis), ``max_shift``, ``fov_deg``,
    ``vtrans_scale``, ``vtrans_max``, ``device``."""

    def __init__(self, *args, device=0, **kwargs):
        super().__init__(*args, **kwargs)
        self.device = int(device)
        self._h = None
        self._timing = False
        self._lib = _lib.require_device()

    def _setup(self, shape):
        params = _Params(shape, **self._kw)
        cp = params.c_struct()
        self._h = _lib.Handle.create(self._lib, 'rs_vo_create', 'rs_vo_destroy', params.im_h, params.im_w,
                                     ctypes.byref(cp), self.device)
        self.params = params
        if self._timing:
            _lib.check(self._lib.rs_vo_set_timing(self._h, 1))

    def setup(self, shape):
        """Create the handle for ``(im_h, im_w)`` frames before the first frame (needed
        when the first frames are already in a ``DeviceBuffer``)."""
        with self._mutex:
            if self.params is None:
                self._setup(shape)
        if (self.params.im_h, self.params.im_w) != tuple(int(s) for s in shape):
            raise ValueError('frame shape %r differs from the first frame\'s %r'
                             % (tuple(shape), (self.params.im_h, self.params.im_w)))
        return self

    def run(self, frames, tables=False, profiles=False):
        """Deltas of ``n`` frames in one call: ``frames`` is a uint8 ``(n, im_h, im_w)``
        host array, or ``(n, _lib.DeviceBuffer)`` for frames already in HBM (``setup``
        first if no host frame came before).  Returns the ``(n, 2)`` float64 array; with
        ``tables`` / ``profiles`` a tuple that also holds the ``(n, 2, 2S-1)`` uint32
        tables and / or the ``(n, Wd_trans + Wd_rot)`` uint32 profiles."""
        with self._mutex:
            dev = isinstance(frames, tuple)
            if dev and self.params is None:
                raise ValueError('frame shape unknown: call setup((im_h, im_w)) before the '
                                 'first device-resident frames')
            # (a host array goes through _check, where the first frame fixes the shape)
            item = self.params.im_h * self.params.im_w if dev else 0
            too_big = '%%d frames of %d bytes exceed the %%d-byte device buffer' % item
            fptr, (n,), keep = _lib.device_or_host(frames, item, self._check, too_big)
            if n < 0:
                raise ValueError(too_big % (n, keep.nbytes))
            p = self.params
            out = np.zeros((n, 2), dtype=np.float64)
            tab = np.zeros((n, 2, 2 * p.S - 1), dtype=np.uint32) if tables else None
            prof = np.zeros((n, p.wd[0] + p.wd[1]), dtype=np.uint32) if profiles else None
            _lib.check(self._lib.rs_vo_run(self._h, n, fptr, _lib.ptr(out, ctypes.c_double),
                                           _lib.ptr(tab, ctypes.c_uint32), _lib.ptr(prof, ctypes.c_uint32)))
            del keep
        extra = tuple(x for x in (tab, prof) if x is not None)
        return (out,) + extra if extra else out

    def reset(self):
        with self._mutex:
            if self._h is not None:
                _lib.check(self._lib.rs_vo_reset(self._h))

    def set_timing(self, enable=True):
        """HIP events around the two launches of every later ``run`` (default off)."""
        self._timing = bool(enable)
        if self._h is not None:
            _lib.check(self._lib.rs_vo_set_timing(self._h, int(self._timing)))

    def device_ms(self):
        """(profile, shift) kernel times of the last ``run`` in ms (HIP events); -1 each
        when it ran untimed or in several chunks."""
        ms = (ctypes.c_double * 2)(-1.0, -1.0)
        if self._h is not None:
            _lib.check(self._lib.rs_vo_last_ms(self._h, ms))
        return ms[0], ms[1]
