#!/usr/bin/env python3
"""Measurements of the pruned plane scan on one GPU, one JSON line each:

  sweep    device time of one frozen scan (HIP events around vt_launch_scan) against
           1,000 templates at several query counts, RS_VT_PRUNE=0 against force: the
           query count from which pruning is faster (VT_PRUNE_MIN_Q)
  allmiss  the headline shape (10 x 1,024 HBM-resident queries, 1,000 templates) with
           hit_frac = 0, 0.5 and 0.9, RS_VT_PRUNE=0 against 1, with prune_stats; under
           ``rocprofv3 --kernel-trace`` the trace holds the passes' own times

usage: python tools/prune_probe.py [sweep] [allmiss] [--reps 20] [--lib OTHER.so] [--noise N] [--hits 0,0.5,0.9]
(--lib: another build of the library, e.g. the parent commit's, for a before/after;
--noise: a hit is its template lowered by 0..N per pixel, 3 as the bench's: the larger, the
closer a hit's score comes to the other blocks' bounds and the less the prefilter prunes)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def handle(prune):
    from pyratslam_amd.view_templates import ViewTemplates
    os.environ['RS_VT_PRUNE'] = prune
    vts = ViewTemplates._from_shape((64, 32), 45000, device=0, capacity=1000)
    vts.set_timing(True)
    return vts


def timed(vts, arg, reps):
    for _ in range(5):
        vts.match_stream(arg)
    ms = []
    for _ in range(reps):
        out = vts.match_stream(arg)
        ms.append(vts.device_ms())
    return float(np.median(ms)), float(np.min(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', nargs='*', default=['sweep', 'allmiss'])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--lib', default=None)
    ap.add_argument('--noise', type=int, default=3)
    ap.add_argument('--hits', default='0,0.5,0.9', help="hit fractions of the 'allmiss' part")
    a = ap.parse_args()
    from pyratslam_amd import _lib, synthetic
    if a.lib:
        _lib.load(a.lib)

    def stats(h):   # with the verified count where the build has it
        return list(h.prune_stats()) + ([h.prune_verified()] if hasattr(_lib.load(), 'rs_vt_prune_verified') else [])

    def scanned(h):   # the pairs actually scanned, beside the rule's (prune_stats()[1]); None: an older build
        return h.prune_scanned() if hasattr(_lib.load(), 'rs_vt_prune_scanned') else None
    lib = synthetic.library(1000, seed=1)
    hs = {p: handle(p) for p in ('0', '1', 'force')}
    for h in hs.values():
        h.add(lib)
    # bring the clocks up before the first timed call
    warm = synthetic.queries_fast(lib, 1024, seed=99)[0]
    wbuf = _lib.DeviceBuffer(warm.nbytes).upload(warm)
    for _ in range(200):
        hs['0'].match_stream((2, 512, wbuf))
    if 'sweep' in a.what:
        for nq in (64, 96, 128, 192, 256, 384, 512, 1024, 2048, 4096):
            q = synthetic.queries_fast(lib, nq, seed=7 + nq, noise=a.noise)[0]
            buf = _lib.DeviceBuffer(q.nbytes).upload(q)
            rec = {'probe': 'sweep', 'lib': a.lib or 'tree', 'noise': a.noise, 'templates': 1000, 'queries': nq}
            outs = {}
            for p in ('0', 'force'):
                med, mn, outs[p] = timed(hs[p], (2, nq // 2, buf), a.reps)   # two batches: one timed scan launch
                rec['ms_prune_' + p] = round(med, 5)
                rec['ms_min_prune_' + p] = round(mn, 5)
            rec['same_keys'] = bool(np.array_equal(outs['0'][0], outs['force'][0]) and
                                    np.array_equal(outs['0'][1], outs['force'][1]))
            rec['prune_stats'] = stats(hs['force'])
            rec['pairs_scanned'] = scanned(hs['force'])
            print(json.dumps(rec), flush=True)
            buf.close()
    if 'allmiss' in a.what:
        for hit in (float(x) for x in a.hits.split(',')):
            qs = np.stack([synthetic.queries_fast(lib, 1024, seed=2 + 1000 * b, hit_frac=hit, noise=a.noise)[0] for b in range(10)])
            buf = _lib.DeviceBuffer(qs.nbytes).upload(qs)
            rec = {'probe': 'allmiss', 'lib': a.lib or 'tree', 'noise': a.noise, 'hit_frac': hit, 'templates': 1000, 'queries': 10240}
            outs = {}
            for p in ('0', '1'):
                med, mn, outs[p] = timed(hs[p], (10, 1024, buf), a.reps)
                rec['ms_prune_' + p] = round(med, 5)
                rec['ms_min_prune_' + p] = round(mn, 5)
            rec['same_keys'] = bool(np.array_equal(outs['0'][0], outs['1'][0]) and
                                    np.array_equal(outs['0'][1], outs['1'][1]))
            rec['prune_stats'] = stats(hs['1'])
            rec['pairs_scanned'] = scanned(hs['1'])
            print(json.dumps(rec), flush=True)
            buf.close()
    for h in hs.values():
        h.close()


if __name__ == '__main__':
    main()
