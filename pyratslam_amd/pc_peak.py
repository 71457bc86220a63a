"""Sub-cell pose of the pose-cell network: the activity packet's circular centroid.

ratslam-python and OpenRatSLAM estimate the pose as the circular centroid of the activity
in a small wrapped box round the peak cell, a continuous ``(x, y, th)`` in cell units; the
reference's ``get_pc_max`` is a placeholder for it (posecell_network.py:316-320).  The rule
(``csrc/pc_peak_rule.h``) yields six float64 sums per pose,
``(S_x, C_x, S_y, C_y, S_th, C_th)``, every operation correctly rounded and in a fixed
order; this module holds the weights the rule multiplies by, its NumPy restatement and
the pose formed from the sums.  Nothing here touches the GPU.
"""
import ctypes
import math

import numpy as np

from . import _lib

CELLS_TO_AVG = 3      # ratslam-python's PC_CELLS_TO_AVG: a 7-cell box
MAX_CELLS_TO_AVG = 3


def check_radius(shape, r):
    """``r`` as an int; ValueError unless 1 <= r <= 3 and every axis holds the 2r+1 box."""
    if int(r) != r or not 1 <= r <= MAX_CELLS_TO_AVG:
        raise ValueError('cells_to_avg must be 1, 2 or 3, got %r' % (r,))
    r = int(r)
    if len(shape) != 3 or 2 * r + 1 > min(shape):
        raise ValueError('grid %r does not hold a box of %d cells along every axis'
                         % (tuple(shape), 2 * r + 1))
    return r


def peak_tables(shape):
    """Per axis, the float64 weights ``sin(2 pi c / N)`` then ``cos(2 pi c / N)``, c = 0 .. N-1,
    as one array of 2N: what ``rs_pc_set_peak_tables`` uploads and ``rs_pc_peak_host`` takes.
    Evaluated by NumPy, so that the device, the host rule and the restatement multiply by
    the same bits."""
    out = []
    for n in shape:
        a = 2 * np.pi * np.arange(int(n)) / int(n)
        out.append(np.ascontiguousarray(np.concatenate([np.sin(a), np.cos(a)]), dtype=np.float64))
    return tuple(out)


def _left_sum(terms):
    """+0.0 + terms[0] + terms[1] + ..., left to right (element-wise on arrays)."""
    s = np.zeros_like(terms[0])
    for t in terms:
        s = s + t
    return s


def numpy_peak_sums(volume, cell, r=CELLS_TO_AVG):
    """The rule restated in NumPy: the six sums of the wrapped box round ``cell`` of a
    float64 ``(X, Y, TH)`` volume.  Every sum is an explicit left-to-right chain of ``+`` on
    slices (never ``np.sum``, whose order is NumPy's own), so the order is by construction."""
    vol = np.asarray(volume, dtype=np.float64)
    r = check_radius(vol.shape, r)
    w = 2 * r + 1
    ix = [(int(p) + np.arange(w) - r) % n for p, n in zip(cell, vol.shape)]
    v = vol[np.ix_(*ix)]
    R = _left_sum([v[:, :, k] for k in range(w)])     # R[i][j]
    C = _left_sum([v[:, j, :] for j in range(w)])     # C[i][k]
    marg = (_left_sum([R[:, j] for j in range(w)]),   # sx[i]
            _left_sum([R[i, :] for i in range(w)]),   # sy[j]
            _left_sum([C[i, :] for i in range(w)]))   # sth[k]
    sums = np.empty(6)
    for a, (s, tab, idx, n) in enumerate(zip(marg, peak_tables(vol.shape), ix, vol.shape)):
        sums[2 * a] = _left_sum([s[i] * tab[idx[i]] for i in range(w)])
        sums[2 * a + 1] = _left_sum([s[i] * tab[n + idx[i]] for i in range(w)])
    return sums


def pose_from_sums(sums, cell, shape):
    """``(x, y, th)`` in cell units: ``atan2(S_a, C_a) * N / 2pi mod N`` per axis; the cell's own
    coordinate where both sums are zero (a dead or empty box); NaN where a sum is not finite."""
    pose = []
    for a, n in enumerate(shape):
        s, c = float(sums[2 * a]), float(sums[2 * a + 1])
        if s == 0.0 and c == 0.0:
            pose.append(float(cell[a]))
        elif not (math.isfinite(s) and math.isfinite(c)):
            pose.append(math.nan)
        else:
            pose.append((math.atan2(s, c) * n / (2 * math.pi)) % n)
    return tuple(pose)


def host_peak_sums(volume, cell, r=CELLS_TO_AVG, tables=None):
    """The rule as the library's host code runs it (``rs_pc_peak_host``: no device)."""
    vol = np.ascontiguousarray(volume, dtype=np.float64)
    if vol.ndim != 3:
        raise ValueError('volume must be (X, Y, TH), got shape %r' % (vol.shape,))
    tabs = peak_tables(vol.shape) if tables is None else tables
    xyz = np.array([int(c) for c in cell], dtype=np.int32)
    sums = np.empty(6)
    _lib.check(_lib.load().rs_pc_peak_host(*vol.shape, int(r), _lib.ptr(vol, ctypes.c_double),
                                           _lib.ptr(xyz, ctypes.c_int32),
                                           *(_lib.ptr(t, ctypes.c_double) for t in tabs),
                                           _lib.ptr(sums, ctypes.c_double)))
    return sums
