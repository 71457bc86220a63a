"""Shared inputs of the patch-normalisation tests (tests/test_vt_norm.py, test_vt_norm_gpu.py):
the test images, an independent per-pixel loop of the rule, and the exposure case -- 16 places
of the synthetic panorama seen through the ROS window, each revisited with its grey levels
scaled and moved and with two-sided noise."""
import math

import numpy as np

from pyratslam_amd import synthetic
from pyratslam_amd import view_templates as VT

ROS = dict(x_range=(32, 96), y_range=(32, 96), x_step=2, y_step=2, im_x=256, im_y=256)
EXPOSURES = ((1.0, 40), (1.3, -30))
NOISE_SEED = 2024


def images(shape, seed):
    """Random bytes, a constant, a 0/255 checkerboard, 0/255 stripes (the largest D, clamping at
    both ends), a low-contrast image (small s, large quotients) and a gradient."""
    rng = np.random.default_rng(seed)
    r, c = np.indices(shape)
    return [rng.integers(0, 256, shape, dtype=np.uint8),
            np.full(shape, 77, np.uint8),
            (((r + c) % 2) * 255).astype(np.uint8),
            ((c % 2) * 255).astype(np.uint8),
            ((r // 3 % 2) * 255).astype(np.uint8),
            rng.integers(100, 103, shape, dtype=np.uint8),
            ((r * 7 + c * 3) % 256).astype(np.uint8)]


def loop_rule(p, radius, gain):
    """The rule pixel by pixel in Python integers with math.isqrt: no summed areas, no NumPy
    arithmetic on the sums."""
    p = np.asarray(p)
    h, w = p.shape
    out = np.zeros((h, w), dtype=np.uint8)
    for r in range(h):
        for c in range(w):
            win = [int(p[y, x]) for y in range(max(0, r - radius), min(h - 1, r + radius) + 1)
                   for x in range(max(0, c - radius), min(w - 1, c + radius) + 1)]
            n, s1, s2 = len(win), sum(win), sum(v * v for v in win)
            d, num = n * s2 - s1 * s1, n * int(p[r, c]) - s1
            s = math.isqrt(d)
            if s == 0:
                out[r, c] = 128
                continue
            q = (gain * abs(num) + s // 2) // s
            out[r, c] = min(255, max(0, 128 + q if num > 0 else 128 - q))
    return out


def place_frames():
    """The 16 places: 256 x 256 frames of the panorama at columns 0, 64, .., 960 (wrapping)."""
    pano = synthetic.panorama(256, 1024, 0)
    return np.stack([np.take(pano, np.arange(c, c + 256) % 1024, axis=1) for c in range(0, 1024, 64)])


def revisit_frames(frames, a, b, seed=NOISE_SEED):
    """clip(rint(a t + b) + U{-3..3}) of every frame."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(-3, 4, frames.shape)
    return np.clip(np.rint(a * frames.astype(np.float64) + b).astype(np.int64) + noise, 0, 255).astype(np.uint8)


def ros_templates(frames):
    """``input[mask].reshape(shape)`` of every frame: (n, 32, 32)."""
    mask, shape = VT.py2_mask(ROS['x_range'], ROS['y_range'], ROS['x_step'], ROS['y_step'], ROS['im_x'],
                              ROS['im_y'])
    assert shape == (32, 32)
    return np.stack([f[mask].reshape(shape) for f in frames])


def score_matrix(lib, queries):
    """numpy_sad_u8_scores of every query against the library: (nq, nt)."""
    return np.stack([VT.numpy_sad_u8_scores(lib, q) for q in queries])


def sequence_oracle(queries, threshold, score, lib=()):
    """ViewTemplates.match on the restatement: ``score(library (T, H, W), query) -> uint64[T]``;
    a query whose minimum exceeds the threshold (or an empty library) becomes a template.
    Returns (indices, scores with None for an empty library, the final library)."""
    lib = list(lib)
    idx, sc = [], []
    for q in queries:
        s = score(np.stack(lib), q) if lib else None
        if s is None or s.min() > threshold:
            idx.append(len(lib))
            sc.append(None if s is None else int(s.min()))
            lib.append(q)
        else:
            idx.append(int(np.argmin(s)))
            sc.append(int(s.min()))
    return idx, sc, lib
