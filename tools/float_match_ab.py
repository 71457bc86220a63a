#!/usr/bin/env python3
"""A/B timing of a float-frame match: the pair-wise path against the resident library (GPU box).

usage: python tools/float_match_ab.py [--rounds 4] [--calls 50] [--sizes 100,1000,10000]
For 32x32 float64 and 64x32 float32 templates and each library size, one child process
(its own time limit) alternates, round by round, three legs over the same library:
  pairwise  sad_scores(np.stack(library), q[None]) plus the host min / argmin: what
            ViewTemplates._match_float does per match (the library re-stacked and
            uploaded on every call);
  match     ViewTemplates.match() of one frame on the float-resident library;
  batch64   ViewTemplates.match_batch() of 64 frames on it.
Every call ends synchronised (its results are on the host), so a host clock around the
call is the cost a caller sees.  The threshold is +inf, so nothing is appended and every
call scans the same library.  Per leg: the median over all calls, the 10th / 90th
percentile, and the run-to-run spread (max - min of the per-round medians over the
median).  A last, separately timed pass records rs_vtf_last_ms (HIP events round the
scan and its argmin) and the share of the VALU peak it reaches, counting 2 operations
(subtract-abs, add) per element and offset.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# geometry -> template shape: the ROS node's 32x32, the bench's 64x32
CONFIGS = {'32x32-f64': (((32, 96), (32, 96), 2, 2, 256, 256), 'float64'),
           '64x32-f32': (((16, 144), (16, 80), 2, 2, 160, 160), 'float32')}
VALU_PEAK = {'float32': 157.3e12, 'float64': 78.6e12}   # MI355X vector FLOP/s (FMA = 2)
BATCH = 64


def child(name, T, rounds, calls):
    sys.path.insert(0, ROOT)
    import numpy as np
    from pyratslam_amd.view_templates import MAX_OFFSET, ViewTemplates, sad_scores
    geom, dt = CONFIGS[name]
    dt = np.dtype(dt)
    rng = np.random.default_rng(1)
    vts = ViewTemplates(*geom, np.inf, capacity=T)
    H, W = vts.shape
    data = rng.random((T, H, W)).astype(dt)
    vts.add(data)
    library = [t.template for t in vts.templates]        # the Python list _match_float stacks
    frames = rng.random((BATCH,) + vts.mask.shape).astype(dt)
    for k in range(0, BATCH, 2):                          # half the frames: noisy stored views
        frames[k][vts.mask] = (data[(k * 131) % T] + rng.normal(0, 0.01, (H, W))).astype(dt).ravel()
    pcs = [(0, 0, 0)] * BATCH
    state = {}

    def pairwise():
        sc = sad_scores(np.stack(library), vts.subsample(frames[0])[None], MAX_OFFSET)[0]
        state['pairwise'] = (int(np.argmin(sc)), float(sc.min()))

    def match():
        state['match'] = vts.match(frames[0], 0, 0, 0).get_index()

    def batch64():
        state['batch'] = [t.get_index() for t in vts.match_batch(frames, pcs)]

    legs = {'pairwise': pairwise, 'match': match, 'batch64': batch64}
    for f in legs.values():                               # warm-up
        for _ in range(5):
            f()
    assert state['pairwise'][0] == state['match'] == state['batch'][0], state
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, f in legs.items():
            row = []
            for _ in range(calls):
                t0 = time.perf_counter()
                f()
                row.append(time.perf_counter() - t0)
            times[k].append(row)
    assert vts.count() == T and vts.scan_form() == 'sad-resident'
    out = {'config': name, 'templates': T, 'calls_per_leg': rounds * calls}
    for k, rows in times.items():
        a = np.array(rows) * 1e6
        med = float(np.median(a))
        rm = np.median(a, axis=1)
        out[k] = {'median_us': med, 'p10_us': float(np.percentile(a, 10)),
                  'p90_us': float(np.percentile(a, 90)),
                  'spread_pct': float((rm.max() - rm.min()) / med * 100)}
    # device time of the resident scans, in a pass of its own
    vts.set_timing(True)
    ops = 2.0 * (H - 2 * MAX_OFFSET) * W * (2 * MAX_OFFSET - 1) * T
    for k, f, nq in (('match', match, 1), ('batch64', batch64, BATCH)):
        ms = []
        for _ in range(30):
            f()
            ms.append(vts.device_ms())
        ms = float(np.median(ms))
        out[k]['scan_ms'] = ms
        out[k]['valu_peak_pct'] = ops * nq / (ms * 1e-3) / VALU_PEAK[dt.name] * 100
    print(json.dumps(out), flush=True)


def table(rows):
    print('| templates | shape | pair-wise us (spread) | match() us (spread) | ratio | batch64 us/call '
          '(us/query) | scan ms 1q / 64q | VALU peak 1q / 64q |')
    print('|---|---|---|---|---|---|---|---|')
    for r in rows:
        p, m, b = r['pairwise'], r['match'], r['batch64']
        print('| %d | %s | %.0f (%.1f%%) | %.0f (%.1f%%) | %.1fx | %.0f (%.1f) | %.3f / %.3f | %.2f%% / %.2f%% |'
              % (r['templates'], r['config'], p['median_us'], p['spread_pct'], m['median_us'],
                 m['spread_pct'], p['median_us'] / m['median_us'], b['median_us'],
                 b['median_us'] / BATCH, m['scan_ms'], b['scan_ms'], m['valu_peak_pct'],
                 b['valu_peak_pct']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--sizes', default='100,1000,10000')
    ap.add_argument('--timeout', type=int, default=240, help='seconds per child process')
    ap.add_argument('--child', nargs=2, metavar=('CONFIG', 'TEMPLATES'))
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), a.rounds, a.calls)
        return
    rows = []
    for name in CONFIGS:
        for T in (int(s) for s in a.sizes.split(',')):
            # one GPU step per child, each under its own time limit; a failure stops the run
            out = subprocess.run([sys.executable, __file__, '--child', name, str(T), '--rounds',
                                  str(a.rounds), '--calls', str(a.calls)], timeout=a.timeout,
                                 check=True, capture_output=True, text=True).stdout
            print(out, end='', flush=True)
            rows.append(json.loads(out.strip().splitlines()[-1]))
    table(rows)


if __name__ == '__main__':
    main()
