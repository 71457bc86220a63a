"""Drop-in ``ViewTemplate`` / ``ViewTemplates`` backed by libratslam_hip.

API of ``/root/reference/ratslam/view_templates.py``: ``ViewTemplates(x_range,
y_range, x_step, y_step, im_x, im_y, match_threshold)`` with ``.match(input,
pc_x, pc_y, pc_th)`` -> ``ViewTemplate`` (``.get_index()``, ``.location()``,
``.template``, ``.match(other)``) and the ``.templates`` list.

The library lives on the GPU (``csrc/view_templates.hip``); each match scans it
with the wrapped-uint8 row-shift score (``metric='wrapped'``, the default) or the true sum
of absolute differences (``metric='sad'``: two-sided camera noise) and applies the reference's strict
threshold / first-argmin / append-on-miss rule.  ``match_batch`` runs many
matches with the exact sequential semantics in one call.
``ShardedViewTemplates`` spreads the library over ranks (one GPU each).

The score is a minimum over 2 * max_offset - 1 row offsets; ``offset_profile`` gives the sum
at every offset and the offset that won (OpenRatSLAM's ``vt_relative_rad``, in template
rows), and ``ViewTemplates(..., offsets=True)`` records both after every uint8 match call
(``last_offsets`` / ``last_profiles``).  The reference shifts along template rows; a turn of
the robot moves the view along image columns, so ``shift_axis='cols'`` stores the templates
column-major (transposed) and the offset then means a heading.

``ViewTemplates(..., normalise=(radius, gain))`` patch-normalises every uint8 template and query
on the GPU on its way into the library (``rs_vt_set_normalise``): each pixel
in units of its neighbourhood's standard deviation, so that a place seen again under another
exposure still matches.  The library, ``ViewTemplate.template`` and every score then are of
normalised bytes (``normalise_u8`` is the rule in NumPy); float frames are a ``TypeError``.

Frames are ``uint8`` on the ROS path (``ros_simulate.py:100-101``): the library
then lives on the GPU and a score wraps mod 256 like numpy's uint8 subtraction.
float32 / float64 frames follow the reference's float semantics instead (a true
sum of |T - Q| in numpy's summation order, bit for bit).  When the first frame an
empty ``ViewTemplates`` sees is a float frame, a float library of that dtype is
created on the GPU (``rs_vtf_*``, ``csrc/view_templates_float.hip``): templates are
uploaded once, ``match`` uploads one query and ``match_batch`` one batch, and
``add`` / ``scores`` / ``match_templates`` take arrays of that dtype
(``scan_form() == 'sad-resident'``).  Anything that mixes dtypes -- a float frame
at a library that holds uint8 templates, a float32 frame at a float64 library or
the reverse, a uint8 frame at a float library -- leaves the device library behind
and scores the Python template list pair-wise per match (``rs_sad_scores``): that
mixed state is a fidelity path, not a throughput path.  The subsampling mask is
the reference's, with Python-2 integer division (:44-54).
"""
import ctypes
import threading

import numpy as np

from . import _lib

MAX_OFFSET = 8  # view_templates.py:14
# metric of a uint8 library (rs_vt_create_metric): 'wrapped' is numpy's own uint8 arithmetic,
# sum((T - Q) mod 256), the reference on mono8 frames; 'sad' the true sum of |T - Q|
METRICS = {'wrapped': _lib.RS_VT_METRIC_WRAPPED, 'sad': _lib.RS_VT_METRIC_SAD}
_FLOAT_CODES = {np.dtype(np.float32): _lib.RS_DT_F32, np.dtype(np.float64): _lib.RS_DT_F64}


def sad_scores(templates, queries, max_offset=MAX_OFFSET, device=0):
    """``ViewTemplate.match`` (view_templates.py:16-28) of every (query, template)
    pair of float arrays on the GPU: (nq, nt) scores in numpy's result dtype of the
    two arrays (float32 or float64), bit-exact to the reference's numpy arithmetic."""
    t = np.asarray(templates)
    q = np.asarray(queries)
    dt = np.result_type(t.dtype, q.dtype)
    if dt not in _FLOAT_CODES:
        raise TypeError('ViewTemplate.match takes uint8 (wrapping) or float32/float64 arrays; '
                        'got %s and %s' % (t.dtype, q.dtype))
    if t.ndim != 3 or q.ndim != 3 or t.shape[1:] != q.shape[1:]:
        raise ValueError('template / query shapes %r, %r differ' % (t.shape[1:], q.shape[1:]))
    t = np.ascontiguousarray(t, dtype=dt)
    q = np.ascontiguousarray(q, dtype=dt)
    out = np.empty((q.shape[0], t.shape[0]), dtype=dt)
    lib = _lib.require_device()
    _lib.check(lib.rs_sad_scores(int(device), _FLOAT_CODES[dt], t.shape[1], t.shape[2], int(max_offset),
                                 t.shape[0], ctypes.c_void_p(t.ctypes.data), q.shape[0],
                                 ctypes.c_void_p(q.ctypes.data), ctypes.c_void_p(out.ctypes.data)))
    return out


def numpy_sad_u8_scores(library, query, max_offset=MAX_OFFSET):
    """The 'sad' metric restated in NumPy: uint64[T] scores of one (H, W) uint8 query against
    a (T, H, W) uint8 library, min over the row offsets of sum |T - Q| on the bytes as
    integers -- ``ViewTemplate.match`` (view_templates.py:16-28) on the arrays cast to float."""
    lib = np.asarray(library)
    q = np.asarray(query)
    if lib.dtype != np.uint8 or q.dtype != np.uint8:
        raise TypeError('numpy_sad_u8_scores takes uint8 arrays, got %s and %s' % (lib.dtype, q.dtype))
    t, h, _ = lib.shape
    if t == 0:
        return np.zeros(0, dtype=np.uint64)
    q = q[max_offset:h - max_offset][None]
    best = None
    for o in range(-max_offset + 1, max_offset):
        a = lib[:, max_offset + o:h - max_offset + o, :]
        # |a - q| = max - min: no byte wraps, summed as integers
        d = (np.maximum(a, q) - np.minimum(a, q)).sum(axis=(1, 2), dtype=np.uint64)
        best = d if best is None else np.minimum(best, d)
    return best


def numpy_offset_profile(template, query, max_offset=MAX_OFFSET, metric='wrapped'):
    """The offset rule restated in NumPy for one (H, W) uint8 pair: ``(offset, profile
    uint32[2M-1])``, the explicit loop over the offsets o = -(M-1) .. M-1 on the bytes as
    integers, the first minimal entry's offset (``ViewTemplate.match``'s strict ``<``)."""
    t = np.asarray(template).astype(np.int64)
    q = np.asarray(query).astype(np.int64)
    h, m = t.shape[0], int(max_offset)
    _metric_code(metric)
    prof = np.zeros(2 * m - 1, dtype=np.uint32)
    for k, o in enumerate(range(-m + 1, m)):
        d = t[m + o:h - m + o] - q[m:h - m]
        prof[k] = (np.abs(d) if metric == 'sad' else d % 256).sum()
    return int(np.argmin(prof)) - (m - 1), prof


def refine_offset(profile):
    """The sub-row offset of a profile (or of each row of an (n, 2M-1) array): the vertex of
    the parabola through the minimum and its two neighbours, ``o + 0.5 (p- - p+) / (p- - 2 p0
    + p+)``; the integer offset when the minimum is the first or the last entry or the
    denominator is not positive (a flat profile)."""
    p = np.asarray(profile, dtype=np.float64)
    if p.ndim == 2:
        return np.array([refine_offset(row) for row in p], dtype=np.float64)
    if p.ndim != 1 or p.size % 2 != 1:
        raise ValueError('a profile has 2 * max_offset - 1 entries, got shape %r' % (p.shape,))
    k = int(np.argmin(p))
    o = float(k - (p.size - 1) // 2)
    if k == 0 or k == p.size - 1:
        return o
    den = p[k - 1] - 2.0 * p[k] + p[k + 1]
    if not den > 0.0:
        return o
    return o + 0.5 * (p[k - 1] - p[k + 1]) / den


MAX_NORM_RADIUS, MAX_NORM_GAIN = 7, 127   # rs_vt_set_normalise's ranges (csrc/vt_norm_rule.h)


def _normalise_arg(normalise):
    """``normalise=None`` or ``(radius, gain)`` -> None or a tuple of two checked ints (a
    ValueError before anything is created)."""
    if normalise is None:
        return None
    try:
        radius, gain = normalise
        ok = int(radius) == radius and int(gain) == gain
    except (TypeError, ValueError):
        ok = False
    if not ok or not 1 <= radius <= MAX_NORM_RADIUS or not 1 <= gain <= MAX_NORM_GAIN:
        raise ValueError('normalise=%r: expected None or (radius in [1, %d], gain in [1, %d])'
                         % (normalise, MAX_NORM_RADIUS, MAX_NORM_GAIN))
    return int(radius), int(gain)


def _u8_images(images, what):
    a = np.asarray(images)
    if a.dtype != np.uint8:
        raise TypeError('%s takes uint8 images, got %s' % (what, a.dtype))
    if a.ndim not in (2, 3):
        raise ValueError('%s takes (H, W) or (n, H, W) images, got shape %r' % (what, a.shape))
    return a


def normalise_u8(images, radius, gain):
    """Patch normalisation restated in NumPy (the rule of csrc/vt_norm_rule.h, DESIGN section
    33) for (H, W) or (n, H, W) uint8 images: each pixel in units of the standard deviation of
    its (2 radius + 1)^2 window, clamped to the image, ``gain`` grey levels per unit around
    128.  Summed-area window sums, integer arithmetic throughout, the square root brought to
    the exact floor by an integer step either way."""
    R, G = _normalise_arg((radius, gain))
    a = _u8_images(images, 'normalise_u8')
    p = a.reshape((-1,) + a.shape[-2:]).astype(np.int64)
    n_img, h, w = p.shape
    r0, r1 = np.maximum(np.arange(h) - R, 0)[:, None], (np.minimum(np.arange(h) + R, h - 1) + 1)[:, None]
    c0, c1 = np.maximum(np.arange(w) - R, 0)[None, :], (np.minimum(np.arange(w) + R, w - 1) + 1)[None, :]

    def window_sum(x):
        sat = np.zeros((n_img, h + 1, w + 1), dtype=np.int64)
        sat[:, 1:, 1:] = x.cumsum(axis=1).cumsum(axis=2)
        return sat[:, r1, c1] - sat[:, r0, c1] - sat[:, r1, c0] + sat[:, r0, c0]

    n = (r1 - r0) * (c1 - c0)
    S, S2 = window_sum(p), window_sum(p * p)
    D, N = n * S2 - S * S, n * p - S
    s = np.sqrt(D.astype(np.float64)).astype(np.int64)
    s -= s * s > D                     # the float estimate, then s^2 <= D < (s + 1)^2
    s += (s + 1) * (s + 1) <= D
    q = (G * np.abs(N) + s // 2) // np.maximum(s, 1)
    out = np.where(s == 0, 128, np.clip(128 + np.sign(N) * q, 0, 255))
    return out.astype(np.uint8).reshape(a.shape)


def normalise_host(images, radius, gain):
    """The same rule by the library's own host code (rs_vt_normalise_host: no device)."""
    R, G = _normalise_arg((radius, gain))
    a = np.ascontiguousarray(_u8_images(images, 'normalise_host'))
    out = np.empty_like(a)
    lib = _lib.load()
    src, dst = a.reshape((-1,) + a.shape[-2:]), out.reshape((-1,) + a.shape[-2:])
    for i in range(src.shape[0]):
        _lib.check(lib.rs_vt_normalise_host(a.shape[-2], a.shape[-1], R, G, _lib.ptr(src[i], ctypes.c_uint8),
                                            _lib.ptr(dst[i], ctypes.c_uint8)))
    return out


def _metric_code(metric):
    if metric not in METRICS:
        raise ValueError('unknown metric %r: expected one of %s' % (metric, sorted(METRICS)))
    return METRICS[metric]


def _u8_scores(templates, queries, device=0, metric='wrapped'):
    """uint8 pair scores, by ``metric``, through a temporary device library (float-mode
    libraries that also hold uint8 templates)."""
    t = np.ascontiguousarray(templates, dtype=np.uint8)
    lib = ViewTemplates._from_shape(t.shape[1:], np.inf, device=device, capacity=len(t), metric=metric)
    try:
        lib.add(t)
        return lib.scores(queries)
    finally:
        lib.close()


def py2_mask(x_range, y_range, x_step, y_step, im_x, im_y):
    """``ViewTemplates.__init__`` mask and template shape (view_templates.py:42-57)."""
    pix = np.arange(im_x * im_y)
    r, c = np.divmod(pix, im_x)
    keep = (r > y_range[0]) & (r < y_range[1]) & (c > x_range[0]) & (c < x_range[1])
    keep &= ((r - y_range[0]) % y_step != 0) & ((c - x_range[0]) % x_step != 0)
    shape = ((x_range[1] - x_range[0]) // x_step, (y_range[1] - y_range[0]) // y_step)
    return keep.reshape((im_x, im_y)), shape


class ViewTemplate:
    """One stored view (view_templates.py:4-37)."""

    def __init__(self, pc_x, pc_y, pc_th, index, template, _owner=None):
        self.pc_x = pc_x
        self.pc_y = pc_y
        self.pc_th = pc_th
        self.template = template
        self.index = index
        self.max_offset = MAX_OFFSET
        self._owner = _owner
        self._solo = None

    def match(self, new_template):
        """Row-shift score against ``new_template`` (view_templates.py:16-28), on the
        GPU: uint8 arrays wrap mod 256 (numpy uint8 arithmetic, a numpy.uint64
        score) -- or, for a template owned by a library of metric 'sad', give the true
        sum of |T - Q| (also uint64); float arrays give numpy's true sum of |T - Q| in
        their dtype."""
        if self.template is None:
            owner = self._owner
            raise ValueError('the bytes of template %d live on rank %d (template g is stored on '
                             'rank g %% %d): score it there' % (self.index, self.index % owner.nranks,
                                                                owner.nranks))
        q = np.ascontiguousarray(new_template)
        t = np.asarray(self.template)
        dev = self._owner.device if self._owner is not None else 0
        norm = self._owner.normalise if self._owner is not None else None
        if norm is not None:
            self._owner._normalise_take(q)
        if t.dtype != np.uint8 or q.dtype != np.uint8:
            return sad_scores(t[None], q[None], self.max_offset, dev)[0, 0]
        owner = self._owner
        if owner is not None and owner.nranks == 1 and not owner._float:
            return owner.scores(q[None], self.index, 1)[0, 0]   # (a normalising owner normalises q)
        if norm is not None:
            # self.template holds normalised bytes already, and the helper library below is a
            # plain one: q is normalised here, once
            q = normalise_host(q, *norm)
        if self._solo is None:
            t = np.ascontiguousarray(t)
            self._solo = ViewTemplates._from_shape(t.shape, np.inf, device=dev,
                                                   metric=owner.metric if owner is not None else 'wrapped')
            self._solo.add(t[None])
        return self._solo.scores(q[None], 0, 1)[0, 0]

    refine_offset = staticmethod(refine_offset)

    def location(self):
        return (self.pc_x, self.pc_y, self.pc_th)

    def get_index(self):
        return self.index


class ViewTemplates(_lib.HandleOwner):
    """Library of view templates on one GPU (view_templates.py:40-75)."""

    _handles = ('_h', '_vtf')

    def __init__(self, x_range, y_range, x_step, y_step, im_x, im_y, match_threshold,
                 device=0, capacity=1024, metric='wrapped', offsets=False, shift_axis='rows', normalise=None):
        """``offsets``: record the row offset and the profile of every uint8 match call
        (``last_offsets``, ``last_profiles``).  ``shift_axis``: ``'rows'`` shifts along the
        gathered template's rows as the reference does; ``'cols'`` stores every template
        transposed, so that the offset runs along image columns (``x_step`` columns a row).
        ``normalise``: None, or ``(radius, gain)`` for patch normalisation on the GPU
        (``normalise_u8``): every uint8 template and query is normalised on its way in, the
        library compares normalised bytes, and float frames are a TypeError."""
        normalise = _normalise_arg(normalise)
        self._set_geometry(x_range, y_range, x_step, y_step, im_x, im_y, shift_axis)
        self._init_device(self.shape, match_threshold, device, capacity, metric, offsets, normalise)

    def _set_geometry(self, x_range, y_range, x_step, y_step, im_x, im_y, shift_axis='rows'):
        """The mask and the stored template shape (host only; a ValueError before any device work)."""
        if shift_axis not in ('rows', 'cols'):
            raise ValueError("shift_axis %r: expected 'rows' or 'cols'" % (shift_axis,))
        self.mask, shape = py2_mask(x_range, y_range, x_step, y_step, im_x, im_y)
        self.shift_axis = shift_axis
        self._gathered_shape = shape      # input[mask].reshape(...), before the transpose
        self.shape = shape if shift_axis == 'rows' else shape[::-1]
        return self

    @classmethod
    def _from_shape(cls, shape, match_threshold, device=0, capacity=64, metric='wrapped', offsets=False,
                    normalise=None):
        self = cls.__new__(cls)
        self.mask = None
        self.shape = tuple(int(s) for s in shape)
        self._init_device(self.shape, match_threshold, device, capacity, metric, offsets, normalise)
        return self

    shift_axis = 'rows'

    normalise = None

    def _init_device(self, shape, match_threshold, device, capacity, metric='wrapped', offsets=False,
                     normalise=None):
        code = _metric_code(metric)      # (a ValueError before anything is created)
        normalise = _normalise_arg(normalise)
        self.metric = metric
        self.offsets = bool(offsets)
        self.last_offsets = self.last_profiles = None
        self.shape = (int(shape[0]), int(shape[1]))
        self.match_threshold = match_threshold
        self.templates = []
        self.device = int(device)
        self.rank, self.nranks = 0, 1
        self._float = False      # mixed dtypes seen: pair-wise float scoring (module doc)
        self._vtf = None         # float-resident library (rs_vtf), its dtype in _fdtype
        self._fdtype = None
        self._capacity = int(capacity)
        self._timing = False
        self._mutex = threading.Lock()
        self._lib = _lib.require_device()
        create = ('rs_vt_create',) if code == _lib.RS_VT_METRIC_WRAPPED else ('rs_vt_create_metric', code)
        self._h = h = _lib.Handle.create(self._lib, create[0], 'rs_vt_destroy', self.shape[0], self.shape[1],
                                         MAX_OFFSET, 0, int(capacity), self.device, *create[1:])
        # `min(match_val) > match_threshold` (view_templates.py:67), compared in float64 as
        # numpy compares the uint64 score with a Python number (inf: never, < 0: always)
        _lib.check(self._lib.rs_vt_set_threshold(h, float(match_threshold)))
        if normalise is not None:
            _lib.check(self._lib.rs_vt_set_normalise(h, normalise[0], normalise[1]))
        self.normalise = normalise

    def __len__(self):
        return len(self.templates)

    def __getitem__(self, index):
        return self.templates[index]

    # -- helpers ----------------------------------------------------------------
    def subsample(self, image):
        """``input[self.mask].reshape(self.shape)`` (view_templates.py:64)."""
        im = np.asarray(image)
        if im.dtype != np.uint8 and im.dtype not in _FLOAT_CODES:
            raise TypeError('ViewTemplates matches uint8 (mono8, ros_simulate.py:100-101) or '
                            'float32/float64 frames; got %s' % im.dtype)
        if im.shape != self.mask.shape:
            raise ValueError('frame shape %r does not match the mask %r' % (im.shape, self.mask.shape))
        # input[mask] takes the kept pixels in C order: the same bytes as a take of the
        # mask's flat indices (one gather, no boolean pass over the frame; 12.6 -> ~3 us
        # per ROS frame), the indices cached per mask object
        cache = getattr(self, '_mask_take', None)
        if cache is None or cache[0] is not self.mask:
            cache = (self.mask, np.flatnonzero(self.mask.ravel()))
            self._mask_take = cache
        if self.shift_axis == 'rows':
            return im.reshape(-1).take(cache[1]).reshape(self.shape)
        return np.ascontiguousarray(im.reshape(-1).take(cache[1]).reshape(self._gathered_shape).T)

    def gather_pixels(self):
        """The pixel table of ``rs_vt_set_subsample``: the frame's flat offsets of a
        template's bytes in stored order (``shift_axis='cols'``: the mask's, transposed)."""
        if self.mask is None:
            raise ValueError('no subsampling mask: construct with the frame geometry')
        pix = np.flatnonzero(self.mask.ravel())
        if self.shift_axis == 'cols':
            pix = pix.reshape(self._gathered_shape).T
        return np.ascontiguousarray(pix.reshape(-1), dtype=np.int32)

    def _check_templates(self, t):
        t = np.asarray(t)
        if t.dtype != np.uint8:
            raise TypeError('templates must be uint8, got %s' % t.dtype)
        if t.shape[-2:] != self.shape:
            raise ValueError('template shape %r != %r' % (t.shape[-2:], self.shape))
        return np.ascontiguousarray(t.reshape((-1,) + self.shape))

    def count(self):
        c = ctypes.c_int64()
        if self._vtf is not None:
            _lib.check(self._lib.rs_vtf_count(self._vtf, ctypes.byref(c)))
        else:
            _lib.check(self._lib.rs_vt_count(self._h, ctypes.byref(c)))
        return c.value

    def _append(self, index, template, pcs=None, i=0, raw=False):
        """One more entry of ``templates``: ``index`` (what the device library numbered it) is
        the list's length, ``pcs[i]`` its pose cell ((0, 0, 0) without ``pcs``), and ``raw``
        uint8 bytes are kept as the library keeps them (``_stored``)."""
        assert index == len(self.templates), (index, len(self.templates))
        pc = pcs[i] if pcs is not None else (0, 0, 0)
        new = ViewTemplate(pc[0], pc[1], pc[2], int(index), self._stored(template) if raw else template,
                           _owner=self)
        self.templates.append(new)
        return new

    def _normalise_take(self, arrays):
        # a normalising library compares normalised bytes: a float frame would leave the
        # uint8 device path (module doc), so it is refused before that path is chosen
        if self.normalise is not None and np.asarray(arrays).dtype != np.uint8:
            raise TypeError('normalise=%r normalises uint8 frames only; got %s'
                            % (self.normalise, np.asarray(arrays).dtype))

    def _stored(self, t):
        """The bytes the library keeps of raw uint8 template(s) ``t``: ``ViewTemplate.template``."""
        return t if self.normalise is None else normalise_host(t, *self.normalise)

    def _refuse_float(self, what):
        # after a float frame the Python template list holds templates the uint8 device
        # library does not (they live in the float library, or -- mixed dtypes -- only
        # in the host's list, scored pair-wise)
        if self._float or self._vtf is not None:
            raise TypeError('this library has matched float frames: %s works on uint8 '
                            'device libraries only; use match() / match_batch()' % what)

    # -- float-resident library ----------------------------------------------------
    _resident_ok = True      # (a sharded library keeps the pair-wise float path)

    def _resident_for(self, dtype):
        """True if arrays of ``dtype`` go through the float-resident library, creating
        it when this is the first frame of an empty, unsharded ViewTemplates."""
        if self._float or dtype not in _FLOAT_CODES:
            return False
        if self._vtf is not None:
            return dtype == self._fdtype
        with self._mutex:
            if self._vtf is not None:            # another thread's first frame got here first
                return dtype == self._fdtype
            if not self._resident_ok or self.nranks != 1 or self.templates:
                return False
            h = _lib.Handle.create(self._lib, 'rs_vtf_create', 'rs_vtf_destroy', self.shape[0], self.shape[1],
                                   MAX_OFFSET, _FLOAT_CODES[dtype], int(self._capacity), self.device)
            if self._timing:
                _lib.check(self._lib.rs_vtf_set_timing(h, 1))
            self._vtf, self._fdtype = h, dtype
        return True

    def _use_resident(self, arrays):
        # add() / scores() / match_templates(): on a float-resident library always (a wrong
        # dtype is then a TypeError), and float arrays create one on an empty library
        return self._vtf is not None or self._resident_for(np.asarray(arrays).dtype)

    def _check_float(self, t, what):
        t = np.asarray(t)
        if t.dtype != self._fdtype:
            raise TypeError('this library has matched float frames and holds %s templates: '
                            '%s takes %s arrays, got %s' % (self._fdtype, what, self._fdtype, t.dtype))
        if t.shape[-2:] != self.shape:
            raise ValueError('template shape %r != %r' % (t.shape[-2:], self.shape))
        return np.ascontiguousarray(t.reshape((-1,) + self.shape))

    def _resident_match(self, q, pcs):
        """``[match(x, *pc) for x, pc in zip(q, pcs)]`` (view_templates.py:63-75) on the
        float-resident library: one frozen scan of the batch (with the in-batch scores
        when it holds more than one query), the reference's rule per query on the host
        -- ``min(match_val) > match_threshold`` on a numpy scalar of the scores' dtype,
        first argmin -- and one append of the queries that became templates.
        Returns (index, score, is_new); call with the mutex held."""
        n = q.shape[0]
        best = np.empty(n, dtype=self._fdtype)
        bidx = np.empty(n, dtype=np.int64)
        inb = np.empty((n, n), dtype=self._fdtype) if n > 1 else None
        _lib.check(self._lib.rs_vtf_scan(
            self._vtf, n, ctypes.c_void_p(q.ctypes.data), int(n > 1), ctypes.c_void_p(best.ctypes.data),
            _lib.ptr(bidx, ctypes.c_int64), None if inb is None else ctypes.c_void_p(inb.ctypes.data)))
        base = len(self.templates)
        idx = np.empty(n, dtype=np.int64)
        score = np.empty(n, dtype=self._fdtype)
        new = np.zeros(n, dtype=bool)
        added = []                      # staged queries appended so far, in order
        for i in range(n):
            m, arg = best[i], int(bidx[i])      # min / first argmin over the library as scanned
            if added:
                s = inb[i, added]               # ... then over the templates this batch appended
                k = int(np.argmin(s))
                if arg < 0 or s[k] < m:         # (a tie keeps the earlier, library, index)
                    m, arg = s[k], base + k
            score[i] = m
            if arg < 0 or m > self.match_threshold:
                idx[i], new[i] = base + len(added), True
                added.append(i)
            else:
                idx[i] = arg
        if added:
            first = ctypes.c_int64()
            which = np.asarray(added, dtype=np.int32)
            _lib.check(self._lib.rs_vtf_append_staged(self._vtf, len(added), _lib.ptr(which, ctypes.c_int32),
                                                      ctypes.byref(first)))
            for k, i in enumerate(added):
                self._append(first.value + k, q[i].copy(), pcs, i)
        return idx, score, new

    def add(self, templates, locations=None):
        """Append templates unconditionally (indices len .. len+n-1)."""
        self._offsets_take(templates)
        self._normalise_take(templates)
        resident = self._use_resident(templates)
        if not resident:
            self._refuse_float('add()')
        t = self._check_float(templates, 'add()') if resident else self._check_templates(templates)
        first = ctypes.c_int64()
        with self._mutex:
            if resident:
                _lib.check(self._lib.rs_vtf_add(self._vtf, t.shape[0], ctypes.c_void_p(t.ctypes.data),
                                                ctypes.byref(first)))
            else:
                _lib.check(self._lib.rs_vt_add(self._h, t.shape[0], _lib.ptr(t, ctypes.c_uint8),
                                               ctypes.byref(first)))
                t = self._stored(t)
            for i in range(t.shape[0]):
                self._append(first.value + i, t[i], locations, i)
        return first.value

    def scores(self, queries, t0=0, nt=None):
        """(nq, nt) scores of queries vs templates [t0, t0+nt) -- ViewTemplate.match:
        uint64 on a uint8 library, the library's dtype on a float-resident one."""
        self._normalise_take(queries)
        if self._use_resident(queries):
            q = self._check_float(queries, 'scores()')
            nt = self.count() - t0 if nt is None else nt
            out = np.empty((q.shape[0], nt), dtype=self._fdtype)
            with self._mutex:
                _lib.check(self._lib.rs_vtf_scores(self._vtf, q.shape[0], ctypes.c_void_p(q.ctypes.data),
                                                   int(t0), int(nt), ctypes.c_void_p(out.ctypes.data)))
            return out
        self._refuse_float('scores()')
        q = self._check_templates(queries)
        nt = self.count() - t0 if nt is None else nt
        out = np.empty((q.shape[0], nt), dtype=np.uint64)
        with self._mutex:
            _lib.check(self._lib.rs_vt_scores(self._h, q.shape[0], _lib.ptr(q, ctypes.c_uint8),
                                              int(t0), int(nt), _lib.ptr(out, ctypes.c_uint64)))
        return out

    # -- row offsets -----------------------------------------------------------------
    def _offset_profile(self, index, qptr):
        """rs_vt_offset_profile of ``index`` against the queries at ``qptr`` (None: the staged
        batch); call with the mutex held."""
        index = np.ascontiguousarray(index, dtype=np.int64).reshape(-1)
        n = index.shape[0]
        offset = np.zeros(n, dtype=np.int32)
        profile = np.zeros((n, 2 * MAX_OFFSET - 1), dtype=np.uint32)
        _lib.check(self._lib.rs_vt_offset_profile(self._h, n, qptr, _lib.ptr(index, ctypes.c_int64),
                                                  _lib.ptr(profile, ctypes.c_uint32),
                                                  _lib.ptr(offset, ctypes.c_int32)))
        return offset, profile

    def _refuse_offsets(self, what):
        self._refuse_float(what)
        if self.nranks > 1:
            raise TypeError('%s is not supported by a sharded library: the template of a match '
                            'lives on one rank' % what)

    def offset_profile(self, index, queries=None):
        """The row offset of each (query, template ``index[i]``) pair and the sums it is the
        first argmin of (rs_vt_offset_profile): ``(offset int32[n], profile uint32[n, 2M-1])``,
        ``profile[i, k]`` the sum at offset ``k - (M - 1)`` under the library's metric, so that
        ``profile[i].min()`` is the pair's score.  ``queries``: uint8 (n, H, W), or ``(n,
        _lib.DeviceBuffer)`` read in place, or None for the batch the last match call staged
        (which explicit queries leave as it is).  An index of -1 gives offset 0 and a row of
        UINT32_MAX."""
        self._refuse_offsets('offset_profile()')
        index = np.ascontiguousarray(index, dtype=np.int64).reshape(-1)
        qptr = keep = None
        if queries is not None:
            qptr, (n,), keep = _lib.device_or_host(queries, self.shape[0] * self.shape[1], self._check_templates,
                                                   '%d queries exceed the %d-byte device buffer')
            if n != index.shape[0]:
                raise ValueError('%d queries for %d indices' % (n, index.shape[0]))
        with self._mutex:
            out = self._offset_profile(index, qptr)
        del keep
        return out

    def _record_offsets(self, idx, new):
        """``offsets=True``: the profile launch on the batch a match call just staged, with
        the indices it returned, after its appends (a query that matched a template created
        earlier in the same sequential batch is profiled against that template; one that
        became a template meets itself: offset 0).  Call with the mutex held."""
        if not self.offsets:
            return
        off, prof = self._offset_profile(idx, None)
        off[np.asarray(new, dtype=bool)] = 0
        self.last_offsets, self.last_profiles = off, prof

    # -- matching ----------------------------------------------------------------
    def _record(self, q, pcs, idx, new):
        for i in range(q.shape[0]):
            if new[i]:
                self._append(idx[i], q[i].copy(), pcs, i, raw=True)
        return [self.templates[int(j)] for j in idx]

    def match_templates(self, queries, pcs=None, mode=_lib.RS_VT_SEQUENTIAL):
        """Match already-subsampled (nq, H, W) queries; returns (index, score, is_new).
        On a float-resident library the queries and scores have the library's dtype
        (+inf where the library was empty)."""
        self._offsets_take(queries)
        self._normalise_take(queries)
        if self._use_resident(queries):
            q = self._check_float(queries, 'match_templates()')
            n = q.shape[0]
            with self._mutex:
                if mode == _lib.RS_VT_SEQUENTIAL:
                    return self._resident_match(q, pcs)
                score = np.empty(n, dtype=self._fdtype)
                idx = np.empty(n, dtype=np.int64)
                _lib.check(self._lib.rs_vtf_scan(self._vtf, n, ctypes.c_void_p(q.ctypes.data), 0,
                                                 ctypes.c_void_p(score.ctypes.data),
                                                 _lib.ptr(idx, ctypes.c_int64), None))
            return idx, score, np.zeros(n, dtype=bool)
        self._refuse_float('match_templates()')
        q = self._check_templates(queries)
        n = q.shape[0]
        idx = np.empty(n, dtype=np.int64)
        score = np.empty(n, dtype=np.uint64)
        new = np.zeros(n, dtype=np.uint8)
        with self._mutex:
            _lib.check(self._lib.rs_vt_match_batch(
                self._h, n, _lib.ptr(q, ctypes.c_uint8), mode, _lib.ptr(score, ctypes.c_uint64),
                _lib.ptr(idx, ctypes.c_int64), _lib.ptr(new, ctypes.c_uint8)))
            if mode == _lib.RS_VT_SEQUENTIAL:
                self._record(q, pcs, idx, new)
            self._record_offsets(idx, new)
        return idx, score, new.astype(bool)

    def _check_batches(self, queries):
        q = np.asarray(queries)
        if q.ndim != 4:
            raise ValueError('match_stream takes (nb, nq, H, W) queries, got %r' % (q.shape,))
        return self._check_templates(q.reshape((-1,) + q.shape[2:])).reshape(q.shape)

    def match_stream(self, queries, nq=None):
        """Frozen-library matching of many batches with one host synchronisation
        (rs_vt_match_stream): ``queries`` is a uint8 (nb, nq, H, W) host array, or
        ``(nb, nq, _lib.DeviceBuffer)`` for batches already in HBM.  Returns
        ``(index, score)`` shaped (nb, nq); nothing is appended."""
        self._refuse_float('match_stream()')
        qptr, (nb, nq), keep = _lib.device_or_host(queries, self.shape[0] * self.shape[1], self._check_batches,
                                                   '%d x %d queries exceed the %d-byte device buffer')
        idx = np.empty((nb, nq), dtype=np.int64)
        score = np.empty((nb, nq), dtype=np.uint64)
        with self._mutex:
            _lib.check(self._lib.rs_vt_match_stream(self._h, nb, nq, qptr,
                                                    _lib.ptr(score, ctypes.c_uint64),
                                                    _lib.ptr(idx, ctypes.c_int64)))
        del keep
        return idx, score

    def _offsets_take(self, arrays):
        # offsets=True: the offset rule is defined on bytes; a float frame would move the
        # library off the uint8 device path (module doc)
        if self.offsets and np.asarray(arrays).dtype != np.uint8:
            raise TypeError('offsets=True records row offsets of uint8 frames only; got %s'
                            % np.asarray(arrays).dtype)

    def match(self, input, pc_x, pc_y, pc_th):
        """Best template for a frame, or a new one (view_templates.py:63-75)."""
        t = self.subsample(input)
        self._offsets_take(t)
        self._normalise_take(t)
        if self._resident_for(t.dtype):
            with self._mutex:
                idx, _, _ = self._resident_match(np.ascontiguousarray(t)[None], [(pc_x, pc_y, pc_th)])
            return self.templates[int(idx[0])]
        if t.dtype != np.uint8 or self._float or self._vtf is not None:
            return self._match_float(t, (pc_x, pc_y, pc_th))
        idx, _, _ = self.match_templates(t[None], [(pc_x, pc_y, pc_th)])
        return self.templates[int(idx[0])]

    def match_batch(self, images, pcs):
        """``[match(im, *pc) for im, pc in zip(images, pcs)]`` in one call."""
        q = [self.subsample(im) for im in images]
        if not q:
            return []
        for x in q:
            self._offsets_take(x)
            self._normalise_take(x)
        if all(x.dtype == q[0].dtype for x in q) and self._resident_for(q[0].dtype):
            with self._mutex:
                idx, _, _ = self._resident_match(np.stack(q), pcs)
            return [self.templates[int(i)] for i in idx]
        if self._float or self._vtf is not None or any(x.dtype != np.uint8 for x in q):
            return [self._match_float(x, pc) for x, pc in zip(q, pcs)]
        idx, _, _ = self.match_templates(np.stack(q), pcs)
        return [self.templates[int(i)] for i in idx]

    def _match_float(self, template, pc):
        """ViewTemplates.match (view_templates.py:63-75) on the float path: every
        stored template scored on the GPU in numpy's dtype of the pair, then the
        reference's own rule -- builtin min over the list against the threshold,
        numpy argmin for the best."""
        if self.nranks > 1:
            raise TypeError('float frames are not supported by a sharded library')
        with self._mutex:
            self._float = True
            _lib.check(self._drop('_vtf'))   # mixed dtypes: the host's list is the library
            match_val = [None] * len(self.templates)
            groups = {}
            for i, tm in enumerate(self.templates):
                groups.setdefault(np.asarray(tm.template).dtype, []).append(i)
            for dt, ids in groups.items():
                lib = np.stack([np.asarray(self.templates[i].template) for i in ids])
                if dt == np.uint8 and template.dtype == np.uint8:
                    sc = _u8_scores(lib, template[None], self.device, self.metric)[0]
                else:
                    sc = sad_scores(lib, template[None], MAX_OFFSET, self.device)[0]
                for i, v in zip(ids, sc):
                    match_val[i] = v
            if len(match_val) == 0 or min(match_val) > self.match_threshold:
                return self._append(len(self.templates), np.array(template), [pc])
            return self.templates[int(np.argmin(match_val))]

    # -- on-device subsampling --------------------------------------------------
    def _ensure_gather(self):
        if getattr(self, '_gather_ready', False):
            return
        pix = self.gather_pixels()
        assert pix.size == self.shape[0] * self.shape[1]
        _lib.check(self._lib.rs_vt_set_subsample(self._h, self.mask.size,
                                                 _lib.ptr(pix, ctypes.c_int32)))
        self._gather_ready = True

    def match_frames(self, frames, pcs, mode=_lib.RS_VT_SEQUENTIAL):
        """``match`` for a batch of whole frames, subsampled on the GPU
        (view_templates.py:64 as a device gather through the mask's pixel offsets).

        ``frames``: uint8 (n, im_x, im_y) host array, or frames already in HBM as
        ``(n, _lib.DeviceBuffer)`` (n whole frames back to back), gathered in
        place.  Returns ``(index, score, is_new)`` like ``match_templates``.
        """
        self._refuse_float('match_frames()')
        self._ensure_gather()
        def host(frames):
            f = np.asarray(frames)
            if f.dtype != np.uint8:
                raise TypeError('ViewTemplates matches uint8 frames (mono8, ros_simulate.py:100-101); '
                                'got %s' % f.dtype)
            if f.shape[1:] != self.mask.shape:
                raise ValueError('frame shape %r does not match the mask %r' % (f.shape[1:], self.mask.shape))
            return np.ascontiguousarray(f)

        fptr, (n,), f = _lib.device_or_host(
            frames, self.mask.size, host,
            '%%d frames of %d bytes exceed the %%d-byte device buffer' % self.mask.size)
        idx = np.empty(n, dtype=np.int64)
        score = np.empty(n, dtype=np.uint64)
        new = np.zeros(n, dtype=np.uint8)
        with self._mutex:
            _lib.check(self._lib.rs_vt_match_frames(self._h, n, fptr, mode,
                                                    _lib.ptr(score, ctypes.c_uint64),
                                                    _lib.ptr(idx, ctypes.c_int64),
                                                    _lib.ptr(new, ctypes.c_uint8)))
            for i in np.flatnonzero(new) if mode == _lib.RS_VT_SEQUENTIAL else ():
                if not isinstance(frames, tuple):
                    self._append(idx[i], self.subsample(f[i]), pcs, i, raw=True)
                    continue
                t = None   # the gathered bytes: read back from the owning rank
                if int(idx[i]) % self.nranks == self.rank:
                    t = np.empty(self.shape, dtype=np.uint8)
                    _lib.check(self._lib.rs_vt_read(self._h, int(idx[i]), _lib.ptr(t, ctypes.c_uint8)))
                self._append(idx[i], t, pcs, i)
            self._record_offsets(idx, new)
        return idx, score, new.astype(bool)

    def device_ms(self):
        """Scan kernel time (HIP events) of the last match, ms; -1 if it ran untimed."""
        ms = ctypes.c_double()
        if self._vtf is not None:
            _lib.check(self._lib.rs_vtf_last_ms(self._vtf, ctypes.byref(ms)))
        else:
            _lib.check(self._lib.rs_vt_last_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def set_timing(self, enable=True):
        """HIP events around every scan (default off; rs_vt_set_timing).  While on, a
        call waits for its keys with a stream synchronisation instead of polling them."""
        _lib.check(self._lib.rs_vt_set_timing(self._h, int(bool(enable))))
        self._timing = bool(enable)
        if self._vtf is not None:
            _lib.check(self._lib.rs_vtf_set_timing(self._vtf, int(self._timing)))

    def scan_form(self):
        """Scan kernel family used for this shape ('plane', 'carry', 'sad', ...);
        'sad-resident' for a float-resident library."""
        if self._vtf is not None:
            return 'sad-resident'
        return self._lib.rs_vt_scan_form(self._h).decode()

    def prune_stats(self):
        """Of the last pruned scan launch ('plane-pruned' handles), the two-pass rule's counts:
        (block, query) pairs of pass B1, of pass B2, template blocks x queries, the rule's
        passes; zeros before the first pruned scan (rs_vt_prune_stats).  With a single list
        pass (RS_VT_PASSES=1, the default) they are counted on demand, the same numbers;
        prune_scanned() tells the pairs actually scanned."""
        out = (ctypes.c_int64 * 4)()
        _lib.check(self._lib.rs_vt_prune_stats(self._h, out))
        return tuple(int(v) for v in out)

    def prune_verified(self):
        """Of the last pruned scan launch, the two-pass rule's counts: the queries settled by
        verifying the one template the prefilter singled out, without a block scan in pass
        B1; 0 before the first pruned scan (rs_vt_prune_verified)."""
        out = ctypes.c_int64(0)
        _lib.check(self._lib.rs_vt_prune_verified(self._h, ctypes.byref(out)))
        return int(out.value)

    def prune_scanned(self):
        """Of the last pruned scan launch: the (block, query) pairs its list passes actually
        scanned (with a single list pass, the lists on the verified score: at least the
        rule's pairs); 0 before the first pruned scan (rs_vt_prune_scanned)."""
        out = ctypes.c_int64(0)
        _lib.check(self._lib.rs_vt_prune_scanned(self._h, ctypes.byref(out)))
        return int(out.value)


class ShardedViewTemplates(ViewTemplates):
    """Template library sharded round-robin over ranks (template g on rank g % n).

    ``reducer`` combines the per-rank first-argmin keys (uint64, key = score << 32
    | g, UINT64_MAX = none):
      * ``'rccl'``: an RCCL allreduce(min) on the GPU inside the library; every
        rank calls ``rs_comm_unique_id`` on rank 0's id (``unique_id`` bytes);
      * a callable ``f(keys: uint64 ndarray) -> uint64 ndarray`` returning the
        elementwise min over ranks (e.g. torch.distributed all_reduce MIN).
    Every rank sees all queries and keeps the full ``.templates`` metadata; the
    template bytes of g live only on rank g % n.
    """
    _resident_ok = False

    def __init__(self, x_range, y_range, x_step, y_step, im_x, im_y, match_threshold,
                 rank, nranks, reducer='rccl', unique_id=None, device=0, capacity=1024, metric='wrapped',
                 offsets=False, normalise=None):
        self._no_offsets(offsets)
        normalise = _normalise_arg(normalise)
        self.mask, self.shape = py2_mask(x_range, y_range, x_step, y_step, im_x, im_y)
        self._init_device(self.shape, match_threshold, device, capacity, metric, normalise=normalise)
        self._attach(rank, nranks, reducer, unique_id)

    @classmethod
    def from_shape(cls, shape, match_threshold, rank, nranks, reducer='rccl', unique_id=None,
                   device=0, capacity=1024, metric='wrapped', offsets=False, normalise=None):
        cls._no_offsets(offsets)
        normalise = _normalise_arg(normalise)
        self = cls.__new__(cls)
        self.mask = None
        self._init_device(shape, match_threshold, device, capacity, metric, normalise=normalise)
        self._attach(rank, nranks, reducer, unique_id)
        return self

    @staticmethod
    def _no_offsets(offsets):
        if offsets:
            raise TypeError('offsets=True is not supported by a sharded library: the template of '
                            'a match lives on one rank')

    def _attach(self, rank, nranks, reducer, unique_id):
        self.rank, self.nranks = int(rank), int(nranks)
        self.reducer = reducer
        if reducer == 'rccl':
            if unique_id is None or len(unique_id) != _lib.RS_UNIQUE_ID_BYTES:
                raise ValueError('reducer="rccl" needs the %d-byte unique id from rank 0'
                                 % _lib.RS_UNIQUE_ID_BYTES)
            uid = np.frombuffer(bytes(unique_id), dtype=np.uint8).copy()
            _lib.check(self._lib.rs_vt_attach_comm(self._h, self.rank, self.nranks,
                                                   _lib.ptr(uid, ctypes.c_uint8)))
        elif callable(reducer):
            _lib.check(self._lib.rs_vt_set_shard(self._h, self.rank, self.nranks))
        else:
            raise ValueError('reducer must be "rccl" or a callable')

    @staticmethod
    def unique_id():
        """RCCL unique id (bytes) to broadcast from rank 0."""
        lib = _lib.require_device()
        buf = np.zeros(_lib.RS_UNIQUE_ID_BYTES, dtype=np.uint8)
        _lib.check(lib.rs_comm_unique_id(_lib.ptr(buf, ctypes.c_uint8)))
        return buf.tobytes()

    def match_templates(self, queries, pcs=None, mode=_lib.RS_VT_SEQUENTIAL):
        if self.reducer == 'rccl':
            return super().match_templates(queries, pcs, mode)
        self._normalise_take(queries)
        q = self._check_templates(queries)
        n = q.shape[0]
        local = np.empty(n, dtype=np.uint64)
        idx = np.empty(n, dtype=np.int64)
        score = np.empty(n, dtype=np.uint64)
        new = np.zeros(n, dtype=np.uint8)
        with self._mutex:
            _lib.check(self._lib.rs_vt_scan_local(self._h, n, _lib.ptr(q, ctypes.c_uint8),
                                                  _lib.ptr(local, ctypes.c_uint64)))
            glob = np.ascontiguousarray(self.reducer(local), dtype=np.uint64)
            _lib.check(self._lib.rs_vt_resolve(
                self._h, n, _lib.ptr(glob, ctypes.c_uint64), mode, _lib.ptr(score, ctypes.c_uint64),
                _lib.ptr(idx, ctypes.c_int64), _lib.ptr(new, ctypes.c_uint8)))
            if mode == _lib.RS_VT_SEQUENTIAL:
                self._record(q, pcs, idx, new)
        return idx, score, new.astype(bool)

    def add(self, templates, locations=None):
        # every rank calls add with the same templates; rank g % n keeps the bytes
        return super().add(templates, locations)
