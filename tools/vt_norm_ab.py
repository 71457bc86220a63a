#!/usr/bin/env python3
"""Timing of patch-normalised view templates (GPU box).

usage: python tools/vt_norm_ab.py [--rounds 5] [--out profiles/vt_norm/vt_norm_ab.json]
One process, a host clock round calls that end with their results on the host; every leg is
warmed up, then the legs of a comparison alternate over the rounds.  Per leg: the median over
all timed calls and the spread, max - min of the per-round medians.

(a) match() of a ROS frame (256 x 256, 32 x 32 templates, 1,000 stored) under 'sad', on a
    plain handle (off) and on one with normalise=(3, 32) (on).
(b) a frozen match_templates of 1,024 queries against 10,000 templates of 64 x 32 under
    'sad', off and on.
(c) what a user had before: normalise_u8 in NumPy on the host, then the same call on a plain
    handle filled with host-normalised templates.  (b) with normalisation on and (c) return the
    same indices and scores (asserted).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, T, NQ = 64, 32, 10000, 1024
NORM = (3, 32)
CALLS = {'a': 400, 'b': 40, 'c': 10}


def summarise(np, rows, scale=1e6):
    arr = np.array(rows) * scale
    rm = np.median(arr, axis=1)
    return {'median_us': float(np.median(arr)), 'round_medians_us': [float(x) for x in rm],
            'spread_us': float(rm.max() - rm.min())}


def timed(fn, calls):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def alternate(np, legs, calls, rounds):
    """legs: name -> callable; warm-up of each, then the legs in turn, round by round."""
    for fn in legs.values():
        fn()
        fn()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, calls[k] if isinstance(calls, dict) else calls))
    return {k: summarise(np, v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vt_norm', 'vt_norm_ab.json'))
    a = ap.parse_args()
    import numpy as np
    from pyratslam_amd import _lib, replay, synthetic
    from pyratslam_amd.view_templates import ViewTemplates, normalise_u8
    _lib.require_device()
    out = {'normalise': list(NORM), 'metric': 'sad', 'rounds': a.rounds}

    # (a) one ROS frame against 1,000 templates
    rng = np.random.default_rng(0)
    stored = rng.integers(0, 256, (1000, 32, 32), dtype=np.uint8)
    frame = rng.integers(0, 256, replay.IM_SIZE, dtype=np.uint8)
    ros = {}
    for leg, norm in (('off', None), ('on', NORM)):
        ros[leg] = ViewTemplates(replay.X_RANGE, replay.Y_RANGE, replay.X_STEP, replay.Y_STEP, *replay.IM_SIZE,
                                 np.inf, metric='sad', normalise=norm)
        ros[leg].add(stored)
    row = {'call': 'match() of a ROS frame, 1,000 templates of 32 x 32',
           **alternate(np, {k: (lambda v=v: v.match(frame, 0, 0, 0)) for k, v in ros.items()}, CALLS['a'], a.rounds)}
    row['added_us'] = row['on']['median_us'] - row['off']['median_us']
    print(json.dumps(row), flush=True)
    out['match'] = row
    for v in ros.values():
        v.close()

    # (b), (c) 1,024 queries against 10,000 templates of 64 x 32
    data = synthetic.library(T, H, W, seed=1)
    q, _ = synthetic.queries_fast(data, NQ, seed=3)
    off = ViewTemplates._from_shape((H, W), np.inf, capacity=T, metric='sad')
    off.add(data)
    on = ViewTemplates._from_shape((H, W), np.inf, capacity=T, metric='sad', normalise=NORM)
    on.add(data)
    host = ViewTemplates._from_shape((H, W), np.inf, capacity=T, metric='sad')
    host.add(normalise_u8(data, *NORM))
    got = {}

    def leg_on():
        got['on'] = on.match_templates(q, mode=_lib.RS_VT_FROZEN)

    def leg_host():
        got['host'] = host.match_templates(normalise_u8(q, *NORM), mode=_lib.RS_VT_FROZEN)

    legs = {'off': lambda: off.match_templates(q, mode=_lib.RS_VT_FROZEN), 'on': leg_on, 'numpy_then_plain': leg_host}
    res = alternate(np, legs, {'off': CALLS['b'], 'on': CALLS['b'], 'numpy_then_plain': CALLS['c']}, a.rounds)
    assert np.array_equal(got['on'][0], got['host'][0]) and np.array_equal(got['on'][1], got['host'][1])
    row = {'call': 'frozen match_templates, 1,024 queries, 10,000 templates of 64 x 32', **res}
    row['added_us'] = row['on']['median_us'] - row['off']['median_us']
    row['numpy_over_on'] = row['numpy_then_plain']['median_us'] / row['on']['median_us']
    print(json.dumps(row), flush=True)
    out['match_templates'] = row
    for v in (off, on, host):
        v.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
