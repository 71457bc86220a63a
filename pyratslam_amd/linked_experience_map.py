"""Experience map with links and loop closure.

The reference's ``ExperienceMap`` is dead reckoning and stops at ``# TODO: linking will
go here`` (``/root/reference/ratslam/experience_map.py:58``); ``experience_map.py`` of this
package restates it as it is.  This module defines the map RatSLAM is built around: one
experience per view template, links between experiences measured by odometry, and a
relaxation that spreads the error of a closed loop over its links.  The reference fixes
no arithmetic for it, so it is defined here, in float64, every operation correctly
rounded and uncontracted, so that NumPy, the host rule (``rs_em_relax_host``) and the GPU
(``csrc/experience_map.hip``) agree to the last bits of ``cos`` / ``sin``.

* ``wrap(a) = a - 2pi * rint(a / 2pi)``.  (``clip_rad_180``'s ceil-based form maps -6.29
  to +6.27: a heading difference crossing -2pi would jump by a turn's remainder.)
* state: a pose ``(x, y, th)`` per experience and the view template that created it; an
  append-only list of links ``l = (a -> b, d, h, f)``: distance, heading and facing of
  ``b`` as seen from ``a``.  The host keeps ``cur`` (the current experience), the dead-
  reckoned heading ``ath`` (never reset), ``thc`` (``ath`` when ``cur`` became current)
  and ``(ax, ay)`` accumulated since then.
* ``update(vtrans, vrot)``: ``ath = wrap(ath + vrot)``, ``ax += vtrans * cos(ath)``,
  ``ay += vtrans * sin(ath)``.  It creates nothing.
* ``on_template(index)``, once per matched frame.  The measurement comes from odometry
  alone: ``d = sqrt(ax^2 + ay^2)``, ``h = wrap(atan2(ay, ax) - thc)``, ``f = wrap(ath - thc)``.
  Unseen template, empty map: experience 0 at ``(0, 0, ath)``.  Unseen template: a new
  experience at ``(x_cur + d cos(th_cur + h), y_cur + d sin(th_cur + h), wrap(th_cur + f))``
  from ``cur``'s relaxed pose, and the link ``cur -> new``.  Seen template whose
  experience ``e != cur``: the link ``cur -> e`` unless it exists.  ``e == cur``: nothing.
  When ``cur`` changes, ``ax = ay = 0`` and ``thc = ath``.  Then ``iterate()``.
* ``on_template(index, rel_rad)``: ``rel_rad`` is the robot's heading minus the heading at
  which the matched template's experience was stored (the view matcher's row offset as an
  angle).  A seen template whose experience ``e != cur`` is then faced
  ``wrap(f - rel_rad)`` by the closure link ``cur -> e`` -- the stored experience's heading,
  not the robot's -- and becomes current with ``thc = ath - rel_rad``: ``thc`` is the dead-
  reckoned heading that corresponds to ``e``'s own heading, which ``get_current_point`` and
  the next measurement turn by.  An unseen template ignores it (the template is the frame
  itself), and ``rel_rad == 0.0`` takes exactly the arithmetic above, bit for bit.
* ``iterate(loops)``: ``loops`` damped-Jacobi sweeps, each reading the previous iterate
  only.  Link ``l``: ``ex = x_b - (x_a + d cos(th_a + h))``, ``ey`` with ``sin``,
  ``df = wrap(th_b - (th_a + f))``.  Experience ``i`` sums, from +0.0 and in order, its
  links with ``i == a`` by ascending link id (``+ex, +ey, +df``), then its links with
  ``i == b`` by ascending link id (``-ex, -ey, -df``) -- ``np.add.at`` over the from-side
  and then the to-side.  ``w = correction / deg_i``; ``x' = x + w sx``, ``y' = y + w sy``,
  ``th' = wrap(th + w st)``; an experience without links keeps its pose.  Dividing by the
  degree is what keeps the parallel sweep stable: an undamped 0.5 per link oscillates on
  even cycles and diverges from degree 3 on.

``NumpyLinkedExperienceMap`` is the restatement (no device) and the oracle;
``LinkedExperienceMap`` keeps the poses on the GPU (``rs_em_*``) and has no CPU fallback.
"""
import ctypes
import threading

import numpy as np

from . import _lib

EXP_LOOPS = 100
EXP_CORRECTION = 0.5
TWO_PI = 2.0 * np.pi
LINK_DTYPE = np.dtype([('a', np.int32), ('b', np.int32), ('d', np.float64), ('h', np.float64),
                       ('f', np.float64)])   # rs::EmLink, 32 bytes


# -- the arithmetic ---------------------------------------------------------------
def wrap(a):
    """``a - 2pi * rint(a / 2pi)`` (scalar or array, float64)."""
    a = np.asarray(a, dtype=np.float64)
    return a - TWO_PI * np.rint(a / TWO_PI)


def residuals(poses, links):
    """``(ex, ey, df)`` of every link at ``poses`` (n, 3)."""
    a, b = links['a'], links['b']
    tha = poses[a, 2]
    ex = poses[b, 0] - (poses[a, 0] + links['d'] * np.cos(tha + links['h']))
    ey = poses[b, 1] - (poses[a, 1] + links['d'] * np.sin(tha + links['h']))
    df = wrap(poses[b, 2] - (tha + links['f']))
    return ex, ey, df


def sweep(poses, links, correction=EXP_CORRECTION):
    """One damped-Jacobi sweep; returns the next iterate (``poses`` is not changed)."""
    n = poses.shape[0]
    out = poses.copy()
    if len(links) == 0 or n == 0:
        return out
    a, b = links['a'], links['b']
    r = np.stack(residuals(poses, links), axis=1)
    s = np.zeros((n, 3), dtype=np.float64)
    np.add.at(s, a, r)          # from-side, ascending link id
    np.add.at(s, b, -r)         # then the to-side
    deg = np.bincount(a, minlength=n) + np.bincount(b, minlength=n)
    on = deg > 0
    w = (np.float64(correction) / deg[on].astype(np.float64))[:, None]
    step = w * s[on]
    out[on, 0] = poses[on, 0] + step[:, 0]
    out[on, 1] = poses[on, 1] + step[:, 1]
    out[on, 2] = wrap(poses[on, 2] + step[:, 2])
    return out


def relax(poses, links, loops=EXP_LOOPS, correction=EXP_CORRECTION):
    """``loops`` sweeps from ``poses``; returns the result."""
    p = np.array(poses, dtype=np.float64).reshape(-1, 3)
    links = as_links(links)
    for _ in range(int(loops)):
        p = sweep(p, links, correction)
    return p


def place(pose, d, h, f):
    """The pose reached from ``pose`` by the measurement ``(d, h, f)``."""
    x, y, th = (np.float64(v) for v in pose)
    d, h, f = np.float64(d), np.float64(h), np.float64(f)
    return np.array([x + d * np.cos(th + h), y + d * np.sin(th + h), wrap(th + f)], dtype=np.float64)


def as_links(links):
    """A ``LINK_DTYPE`` array from such an array or from ``(a, b, d, h, f)`` tuples."""
    if isinstance(links, np.ndarray) and links.dtype == LINK_DTYPE:
        return links
    return np.array([tuple(l) for l in links], dtype=LINK_DTYPE)


def relax_host(poses, links, loops=EXP_LOOPS, correction=EXP_CORRECTION):
    """``relax`` by the library's host rule (``rs_em_relax_host``: the kernels' function and
    the library's incidence-list builder, no device)."""
    lib = _lib.load()
    p = np.array(poses, dtype=np.float64).reshape(-1, 3)
    links = as_links(links)
    col = {k: np.ascontiguousarray(links[k]) for k in LINK_DTYPE.names}
    _lib.check(lib.rs_em_relax_host(p.shape[0], len(links), _lib.ptr(col['a'], ctypes.c_int32),
                                    _lib.ptr(col['b'], ctypes.c_int32), _lib.ptr(col['d'], ctypes.c_double),
                                    _lib.ptr(col['h'], ctypes.c_double), _lib.ptr(col['f'], ctypes.c_double),
                                    _lib.ptr(p, ctypes.c_double), int(loops), float(correction)))
    return p


# -- the map ----------------------------------------------------------------------
class _LinkedMapBase:
    """The host bookkeeping both classes share; the poses are the subclass's."""

    def __init__(self, exp_loops=EXP_LOOPS, exp_correction=EXP_CORRECTION):
        self.exp_loops = int(exp_loops)
        self.exp_correction = float(exp_correction)
        if self.exp_loops < 0:
            raise ValueError('exp_loops %d < 0' % self.exp_loops)
        if not 0.0 < self.exp_correction <= 1.0:
            raise ValueError('exp_correction %g outside (0, 1]' % self.exp_correction)
        self.current_exp = None            # cur
        self.accum_delta_th = np.float64(0.0)   # ath
        self.accum_delta_x = np.float64(0.0)    # ax
        self.accum_delta_y = np.float64(0.0)    # ay
        self.theta_current = np.float64(0.0)    # thc
        self.exp_vt = []                   # experience -> its view template
        self.vt_exp = {}                   # view template -> its experience
        self._links = []                   # (a, b, d, h, f)
        self._pairs = set()                # (a, b) of every link
        self._link_array = None            # links() of the list so far
        self._mutex = threading.Lock()

    @property
    def count(self):
        """Experiences in the map."""
        return len(self.exp_vt)

    def update(self, vtrans, vrot, pc_loc=None, vt=None):
        """Dead reckoning since ``cur`` became current (heading, then position)."""
        self.accum_delta_th = wrap(self.accum_delta_th + np.float64(vrot))
        self.accum_delta_x = self.accum_delta_x + np.float64(vtrans) * np.cos(self.accum_delta_th)
        self.accum_delta_y = self.accum_delta_y + np.float64(vtrans) * np.sin(self.accum_delta_th)

    def measurement(self):
        """``(d, h, f)`` from ``cur`` to here, from the accumulators alone."""
        ax, ay = self.accum_delta_x, self.accum_delta_y
        d = np.sqrt(ax * ax + ay * ay)
        h = wrap(np.arctan2(ay, ax) - self.theta_current)
        f = wrap(self.accum_delta_th - self.theta_current)
        return float(d), float(h), float(f)

    def on_template(self, index, rel_rad=0.0):
        """The frame matched view template ``index``, seen turned by ``rel_rad`` from the
        heading it was stored at: create, link or do nothing (module docstring), relax, and
        return the experience now current."""
        index = int(index)
        if index < 0:
            raise ValueError('template index %d < 0' % index)
        rel = np.float64(rel_rad)
        if not np.isfinite(rel):
            raise ValueError('rel_rad %r is not finite' % (rel_rad,))
        cur = self.current_exp
        d, h, f = self.measurement()
        e = self.vt_exp.get(index)
        if e is None:
            if cur is None:
                e = self.add_experience(-1, 0.0, 0.0, self.accum_delta_th, vt=index)
            else:
                e = self.add_experience(cur, d, h, f, vt=index)
            if cur is not None:
                self._link(cur, e, d, h, f)
            rel = np.float64(0.0)      # unseen: the template is the frame itself
        elif e != cur and (cur, e) not in self._pairs:
            self._link(cur, e, d, h, f if rel == 0.0 else float(wrap(np.float64(f) - rel)))
        if e != cur:
            self.current_exp = e
            self.accum_delta_x = np.float64(0.0)
            self.accum_delta_y = np.float64(0.0)
            self.theta_current = self.accum_delta_th if rel == 0.0 else self.accum_delta_th - rel
        self.iterate()
        return e

    def add_experience(self, src=-1, d=0.0, h=0.0, f=0.0, vt=None):
        """A new experience reached from experience ``src`` by ``(d, h, f)`` (``src = -1``:
        the origin, heading ``f``), owned by view template ``vt`` if given.  It adds no
        link and does not move ``cur``: the building block of ``on_template``, and the way
        to load a map made elsewhere (with ``set_poses`` and ``add_link``)."""
        src = int(src)
        if not -1 <= src < self.count:
            raise ValueError('experience %d outside [-1, %d)' % (src, self.count))
        if vt is not None and vt in self.vt_exp:
            raise ValueError('view template %d owns experience %d' % (vt, self.vt_exp[vt]))
        e = self._add_experience(src, float(d), float(h), float(f))
        self.exp_vt.append(vt)
        if vt is not None:
            self.vt_exp[vt] = e
        return e

    def load(self, poses, links=()):
        """Append ``poses`` (n, 3) as new experiences and ``links`` (ids within the whole
        map) between them."""
        p = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
        first = self.count
        for _ in range(p.shape[0]):
            self.add_experience()
        if p.shape[0]:
            self.set_poses(p, first)
        for a, b, d, h, f in as_links(links).tolist():
            self.add_link(a, b, d, h, f)
        return self

    def add_link(self, a, b, d, h, f):
        """Append the link ``a -> b``; ``ValueError`` for ids outside the map, ``a == b``
        and a link ``a -> b`` that exists."""
        a, b = int(a), int(b)
        n = self.count
        if not (0 <= a < n and 0 <= b < n):
            raise ValueError('link %d -> %d outside the %d experiences' % (a, b, n))
        if a == b:
            raise ValueError('link %d -> %d joins an experience to itself' % (a, b))
        if (a, b) in self._pairs:
            raise ValueError('link %d -> %d exists' % (a, b))
        return self._link(a, b, float(d), float(h), float(f))

    def _link(self, a, b, d, h, f):
        self._add_link(a, b, d, h, f)
        self._links.append((a, b, d, h, f))
        self._pairs.add((a, b))
        return len(self._links) - 1

    def links(self):
        """The link records, a ``LINK_DTYPE`` array in link-id order."""
        if self._link_array is None or len(self._link_array) != len(self._links):
            self._link_array = np.array(self._links, dtype=LINK_DTYPE)
        return self._link_array.copy()

    def get_points(self):
        return [(float(x), float(y)) for x, y, _ in self.poses()]

    def get_current_point(self):
        """The robot: ``cur``'s point plus the displacement accumulated since, turned from
        the dead-reckoned frame into ``cur``'s relaxed heading.  Before the first
        experience: the accumulators themselves."""
        ax, ay = self.accum_delta_x, self.accum_delta_y
        if self.current_exp is None:
            return (float(ax), float(ay))
        x, y, th = self._pose(self.current_exp)
        r = th - self.theta_current
        c, s = np.cos(r), np.sin(r)
        return (float(x + (ax * c - ay * s)), float(y + (ax * s + ay * c)))

    def rms_residual(self):
        """RMS over the links of the position and of the heading residual."""
        links = self.links()
        if len(links) == 0:
            return 0.0, 0.0
        ex, ey, df = residuals(self.poses(), links)
        return float(np.sqrt(np.mean(ex * ex + ey * ey))), float(np.sqrt(np.mean(df * df)))

    def close(self):
        pass


class NumpyLinkedExperienceMap(_LinkedMapBase):
    """The linked map in NumPy alone: the restatement the GPU class is checked against."""

    def __init__(self, exp_loops=EXP_LOOPS, exp_correction=EXP_CORRECTION):
        super().__init__(exp_loops, exp_correction)
        self._buf = np.zeros((16, 3), dtype=np.float64)   # grows by doubling
        self._n = 0

    @property
    def _poses(self):
        return self._buf[:self._n]

    def _add_experience(self, src, d, h, f):
        p = np.array([0.0, 0.0, f]) if src < 0 else place(self._buf[src], d, h, f)
        if self._n == self._buf.shape[0]:
            self._buf = np.concatenate([self._buf, np.zeros_like(self._buf)])
        self._buf[self._n] = p
        self._n += 1
        return self._n - 1

    def _add_link(self, a, b, d, h, f):
        pass

    def iterate(self, loops=None):
        loops = self.exp_loops if loops is None else int(loops)
        self._buf[:self._n] = relax(self._poses, self.links(), loops, self.exp_correction)

    def poses(self):
        return self._poses.copy()

    def set_poses(self, poses, first=0):
        p = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
        if first < 0 or first + p.shape[0] > self.count:
            raise ValueError('experiences [%d, %d) outside the %d of the map' % (first, first + p.shape[0], self.count))
        self._poses[first:first + p.shape[0]] = p

    def _pose(self, i):
        return self._poses[i]


class LinkedExperienceMap(_lib.HandleOwner, _LinkedMapBase):
    """The linked map with its poses on the GPU (``rs_em_*``).  New poses are computed on
    the device from the relaxed pose they start at, ``iterate`` is queued and does not wait;
    ``poses`` / ``get_current_point`` read after everything queued before them.

    ``capacity``: experiences allocated at first (the map grows by doubling).  The kernel
    form follows the map's size (``form()``); ``RS_EM_FORM=lds|sweep`` forces one."""

    def __init__(self, exp_loops=EXP_LOOPS, exp_correction=EXP_CORRECTION, capacity=1024, device=0):
        super().__init__(exp_loops, exp_correction)
        self.device = int(device)
        self._lib = _lib.require_device()
        self._h = _lib.Handle.create(self._lib, 'rs_em_create', 'rs_em_destroy', int(capacity),
                                     self.exp_correction, self.device)

    def _add_experience(self, src, d, h, f):
        out = ctypes.c_int(-1)
        with self._mutex:
            _lib.check(self._lib.rs_em_add_experience(self._h, int(src), d, h, f, ctypes.byref(out)))
        return out.value

    def _add_link(self, a, b, d, h, f):
        with self._mutex:
            _lib.check(self._lib.rs_em_add_link(self._h, a, b, d, h, f, None))

    def iterate(self, loops=None):
        loops = self.exp_loops if loops is None else int(loops)
        with self._mutex:
            _lib.check(self._lib.rs_em_relax(self._h, loops))

    def _read(self, first, n):
        out = np.zeros((n, 3), dtype=np.float64)
        with self._mutex:
            _lib.check(self._lib.rs_em_read(self._h, int(first), int(n), _lib.ptr(out, ctypes.c_double)))
        return out

    def poses(self):
        return self._read(0, self.count)

    def set_poses(self, poses, first=0):
        p = _lib.as_c(poses, np.float64).reshape(-1, 3)
        with self._mutex:
            _lib.check(self._lib.rs_em_write(self._h, int(first), p.shape[0], _lib.ptr(p, ctypes.c_double)))

    def _pose(self, i):
        return self._read(i, 1)[0]

    def form(self):
        """``'lds'`` or ``'sweep'``: the kernel form of the next ``iterate``."""
        return self._lib.rs_em_form(self._h).decode()

    def set_timing(self, enable=True):
        """HIP events around the launches of every later ``iterate`` (default off)."""
        _lib.check(self._lib.rs_em_set_timing(self._h, int(bool(enable))))

    def device_ms(self):
        """Device time of the last ``iterate`` in ms (waits for it); -1 when untimed."""
        ms = ctypes.c_double(-1.0)
        _lib.check(self._lib.rs_em_last_ms(self._h, ctypes.byref(ms)))
        return ms.value
