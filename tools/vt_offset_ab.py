#!/usr/bin/env python3
"""Timing of the row-offset profile of view-template matches (GPU box).

usage: python tools/vt_offset_ab.py [--rounds 5] [--out profiles/vt_offset/vt_offset_ab.json]
One process, a host clock round calls that end with their results on the host; every leg is
warmed up, then the legs of a comparison alternate over the rounds.  Per leg: the median over
all timed calls and the spread, max - min of the per-round medians.

(1) the offsets of the same matches by two routes, 10,000 templates of 64 x 32, at 1 query and
    at 1,024 (stored views rolled by -7..7 rows with one-sided noise):
      read      what the commit before the feature leaves a user: rs_vt_read of every matched
                template, then the profile in NumPy, vectorised over the batch;
      profile   offset_profile(index, queries): one upload, one launch of
                vt_offset_profile_kernel, the results stored into pinned memory;
      staged    offset_profile(index) on the batch the match left on the device.
    The three give the same offsets and profiles (asserted).
(2) what offsets=True adds: match() of a ROS frame (256 x 256, 32 x 32 templates, 1,000
    stored) and a frozen match_templates of 1,024 queries against 10,000 templates of 64 x 32,
    each on one handle with the flag off and on.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, T = 64, 32, 10000
# timed calls per leg and round, by the number of queries (reading 1,024 templates back is
# 131,072 chunk copies)
CALLS = {('read', 1): 100, ('read', 1024): 2, ('profile', 1): 400, ('profile', 1024): 40,
         ('staged', 1): 400, ('staged', 1024): 40}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vt_offset', 'vt_offset_ab.json'))
    a = ap.parse_args()
    import numpy as np
    from pyratslam_amd import _lib, replay, synthetic
    from pyratslam_amd.view_templates import MAX_OFFSET, ViewTemplates
    lib = _lib.require_device()
    data = synthetic.library(T, H, W, seed=1)
    out = {'templates': T, 'shape': [H, W], 'rounds': a.rounds, 'routes': [], 'flag': []}

    # (1) two routes to the offsets of the same matches
    for metric in ('wrapped', 'sad'):
        vts = ViewTemplates._from_shape((H, W), np.inf, capacity=T, metric=metric)
        vts.add(data)
        for nq in (1, 1024):
            q, _ = synthetic.queries_fast(data, nq, seed=nq, hit_frac=1.0)
            idx, score, _ = vts.match_templates(q, mode=_lib.RS_VT_FROZEN)
            got = {}

            def read():
                t = np.empty((nq, H, W), np.uint8)
                for i, g in enumerate(idx):
                    _lib.check(lib.rs_vt_read(vts._h, int(g), _lib.ptr(t[i], ctypes.c_uint8)))
                m = MAX_OFFSET
                ti, qi = t.astype(np.int32), q[:, m:H - m].astype(np.int32)
                prof = np.empty((nq, 2 * m - 1), np.uint32)
                for k in range(2 * m - 1):
                    d = ti[:, k + 1:H - 2 * m + k + 1] - qi
                    prof[:, k] = (np.abs(d) if metric == 'sad' else d & 255).sum(axis=(1, 2))
                got['read'] = (np.argmin(prof, axis=1).astype(np.int32) - (m - 1), prof)

            def profile():
                got['profile'] = vts.offset_profile(idx, q)

            def staged():
                got['staged'] = vts.offset_profile(idx)

            legs = {'read': read, 'profile': profile, 'staged': staged}
            for fn in legs.values():
                fn()
                fn()
            for k in ('profile', 'staged'):
                assert np.array_equal(got[k][0], got['read'][0]) and np.array_equal(got[k][1], got['read'][1])
            assert np.array_equal(got['read'][1].min(axis=1), score)
            times = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, fn in legs.items():
                    times[k].append(timed(fn, CALLS[(k, nq)]))
            row = {'metric': metric, 'queries': nq, **{k: summarise(np, v) for k, v in times.items()}}
            row['read_over_profile'] = row['read']['median_us'] / row['profile']['median_us']
            print(json.dumps(row), flush=True)
            out['routes'].append(row)
        vts.close()

    # (2) the cost of offsets=True, flag off and on on one handle
    rng = np.random.default_rng(0)
    ros = ViewTemplates(replay.X_RANGE, replay.Y_RANGE, replay.X_STEP, replay.Y_STEP, *replay.IM_SIZE, np.inf)
    ros.add(rng.integers(0, 256, (1000, 32, 32), dtype=np.uint8))
    frame = rng.integers(0, 256, replay.IM_SIZE, dtype=np.uint8)
    big = ViewTemplates._from_shape((H, W), np.inf, capacity=T)
    big.add(data)
    q, _ = synthetic.queries_fast(data, 1024, seed=3)
    cases = {'match() of a ROS frame, 1,000 templates of 32 x 32': (ros, lambda: ros.match(frame, 0, 0, 0), 400),
             'frozen match_templates, 1,024 queries, 10,000 templates of 64 x 32':
                 (big, lambda: big.match_templates(q, mode=_lib.RS_VT_FROZEN), 40)}
    for name, (vts, fn, calls) in cases.items():
        times = {'off': [], 'on': []}
        for flag in (False, True):
            vts.offsets = flag
            fn()
            fn()
        for _ in range(a.rounds):
            for leg, flag in (('off', False), ('on', True)):
                vts.offsets = flag
                times[leg].append(timed(fn, calls))
        row = {'call': name, **{k: summarise(np, v) for k, v in times.items()}}
        row['added_us'] = row['on']['median_us'] - row['off']['median_us']
        print(json.dumps(row), flush=True)
        out['flag'].append(row)
        vts.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
