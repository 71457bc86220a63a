#!/usr/bin/env python3
"""A/B timing of the scanline visual odometer on 256x256 frames (GPU box).

usage: python tools/vo_ab.py [--rounds 5] [--out profiles/vo_ab.json] [--big 8192]
One process alternates its legs, round by round, after a warm-up of every leg:
  numpy     NumpyVisualOdometer.update per frame on the host -- the baseline: what a
            user would write without this odometer;
  update    SimpleVisualOdometer.update per frame from host memory;
  run1024   run() of 1,024 host frames (staged in chunks through pinned memory);
  dev1024   run() of 1,024 frames in a DeviceBuffer (64 MiB: fits the Infinity Cache,
            so its profile-kernel rate is a cache figure);
  dev8192   run() of 8,192 frames in a DeviceBuffer (512 MiB: beyond the Infinity Cache).
Every call ends synchronised (its deltas are on the host), so a host clock around the
call is what a caller pays.  Per leg: the median over all calls, per frame, and the
spread (max - min of the per-round medians over the median).  A last pass, with
rs_vo_set_timing on, records rs_vo_last_ms of the resident legs: the profile kernel's
achieved bytes per second = the region bytes the algorithm must read (one pass over the
frame: both regions are the whole frame and are read once), over its time, next to the
6.3 TB/s an HBM stream achieves on this chip.  --trace-leg NAME runs one resident leg
alone a few times, for a `rocprofv3 --kernel-trace --stats -- python tools/vo_ab.py
--trace-leg dev8192` run of its own.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.3e12   # bytes/s, a streaming read on MI355X
IM = (256, 256)


def frames_for(n, seed=0):
    """n frames: column windows of the synthetic panorama at a random walk of offsets
    (true shifts within +-20 columns), plus U{0..2} noise -- ros_stream's frames
    without its per-frame Python loop."""
    import numpy as np
    from pyratslam_amd import synthetic
    rng = np.random.default_rng(seed)
    pano = synthetic.panorama(IM[0], 4 * IM[1], seed)
    offs = np.cumsum(rng.integers(-20, 21, size=n)) % pano.shape[1]
    out = np.empty((n,) + IM, dtype=np.uint8)
    for i0 in range(0, n, 256):
        o = offs[i0:i0 + 256]
        cols = (o[:, None] + np.arange(IM[1])[None, :]) % pano.shape[1]
        blk = pano[:, cols].transpose(1, 0, 2).astype(np.int16)
        blk += rng.integers(0, 3, size=blk.shape, dtype=np.int16)
        out[i0:i0 + 256] = np.clip(blk, 0, 255).astype(np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--big', type=int, default=8192, help='frames of the beyond-cache leg')
    ap.add_argument('--per-frame-calls', type=int, default=200)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace-leg', default=None, choices=['dev1024', 'dev8192'])
    a = ap.parse_args()
    import numpy as np
    from pyratslam_amd import NumpyVisualOdometer, SimpleVisualOdometer, _lib

    fb = IM[0] * IM[1]
    host = frames_for(1024)
    big = frames_for(a.big, seed=1)
    bufs = {'dev1024': (1024, _lib.DeviceBuffer(1024 * fb).upload(host)),
            'dev8192': (a.big, _lib.DeviceBuffer(a.big * fb).upload(big))}
    del big
    npo = NumpyVisualOdometer()
    vo = SimpleVisualOdometer().setup(IM)
    state = {}

    def per_frame(o, key):
        def leg():
            o.reset()
            state[key] = np.array([o.update(f) for f in host[:a.per_frame_calls]])
            return a.per_frame_calls
        return leg

    def run_host():
        vo.reset()
        state['run1024'] = vo.run(host)
        return 1024

    def run_dev(key):
        def leg():
            vo.reset()
            state[key] = vo.run(bufs[key])
            return bufs[key][0]
        return leg

    legs = {'numpy': per_frame(npo, 'numpy'), 'update': per_frame(vo, 'update'),
            'run1024': run_host, 'dev1024': run_dev('dev1024'), 'dev8192': run_dev('dev8192')}
    if a.trace_leg:
        for _ in range(6):
            legs[a.trace_leg]()
        print(json.dumps({'traced': a.trace_leg, 'calls': 6}))
        return
    for f in legs.values():                       # warm-up, and the legs agree bit for bit
        f()
        f()
    n = a.per_frame_calls
    assert state['numpy'].tobytes() == state['update'].tobytes() == state['run1024'][:n].tobytes()
    assert state['run1024'].tobytes() == state['dev1024'].tobytes()
    reps = {'numpy': 1, 'update': 3, 'run1024': 5, 'dev1024': 20, 'dev8192': 5}
    times = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, f in legs.items():
            row = []
            for _ in range(reps[k]):
                t0 = time.perf_counter()
                nfr = f()
                row.append((time.perf_counter() - t0) / nfr)
            times[k].append(row)
    out = {'frame': list(IM), 'rounds': a.rounds, 'frames': {'numpy': n, 'update': n, 'run1024': 1024,
                                                             'dev1024': 1024, 'dev8192': a.big}}
    for k, rows in times.items():
        arr = np.array(rows) * 1e6
        med = float(np.median(arr))
        rm = np.median(arr, axis=1)
        out[k] = {'us_per_frame': med, 'spread_pct': float((rm.max() - rm.min()) / med * 100)}
    # device time of the two kernels, in a pass of its own
    vo.set_timing(True)
    for k in ('dev1024', 'dev8192'):
        ms = []
        for _ in range(15):
            legs[k]()
            ms.append(vo.device_ms())
        ms = np.array(ms)
        prof_ms, shift_ms = float(np.median(ms[:, 0])), float(np.median(ms[:, 1]))
        nbytes = bufs[k][0] * fb                  # one pass over every frame
        rate = nbytes / (prof_ms * 1e-3)
        out[k].update({'profile_ms': prof_ms, 'shift_ms': shift_ms,
                       'profile_ms_spread_pct': float((ms[:, 0].max() - ms[:, 0].min()) / prof_ms * 100),
                       'profile_bytes': nbytes, 'profile_TBps': rate / 1e12,
                       'share_of_hbm_stream_pct': rate / HBM_ACHIEVABLE * 100})
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)
            fh.write('\n')
    print('| leg | frames per call | us per frame (spread) | vs numpy |')
    print('|---|---|---|---|')
    for k in legs:
        print('| %s | %d | %.2f (%.1f%%) | %.1fx |' % (k, out['frames'][k], out[k]['us_per_frame'],
                                                      out[k]['spread_pct'],
                                                      out['numpy']['us_per_frame'] / out[k]['us_per_frame']))
    print('| resident leg | profile kernel ms | shift kernel ms | profile TB/s | of 6.3 TB/s |')
    print('|---|---|---|---|---|')
    for k in ('dev1024', 'dev8192'):
        print('| %s | %.4f | %.4f | %.2f | %.0f%% |' % (k, out[k]['profile_ms'], out[k]['shift_ms'],
                                                      out[k]['profile_TBps'], out[k]['share_of_hbm_stream_pct']))


if __name__ == '__main__':
    main()
