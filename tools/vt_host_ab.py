#!/usr/bin/env python3
"""A/B of the view-template matcher's host-bound calls across library builds, each build in
its own process, interleaved over rounds (GPU box): frozen match_templates of 1, 16 and 64
queries (read in place from the pinned staging array, keys exported by the scan and polled)
and of 65 and 512 queries (the copy and the export launch; 512 prunes), against 1,000
templates, in microseconds per call.  tools/stream_ab.py [--host] covers match_stream.
usage: python tools/vt_host_ab.py LIB.so [LIB2.so ...] [--rounds 3] [--calls 2000]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 16, 64, 65, 512)


def child(path, calls):
    sys.path.insert(0, ROOT)
    import numpy as np
    from pyratslam_amd import _lib, synthetic
    _lib.load(path)
    from pyratslam_amd.view_templates import ViewTemplates
    vts = ViewTemplates._from_shape((64, 32), 45000, device=0, capacity=1000)
    lib = synthetic.library(1000, seed=1)
    vts.add(lib)
    out, sha = {'lib': path}, hashlib.sha256()
    for n in SIZES:
        q = np.ascontiguousarray(synthetic.queries_fast(lib, n, seed=7 + n)[0])
        t_end = time.perf_counter() + 0.2
        while time.perf_counter() < t_end:
            vts.match_templates(q, mode=_lib.RS_VT_FROZEN)
        k = max(50, calls // max(1, n // 16))
        t0 = time.perf_counter()
        for _ in range(k):
            idx, score, _new = vts.match_templates(q, mode=_lib.RS_VT_FROZEN)
        out['us_per_call_%d' % n] = 1e6 * (time.perf_counter() - t0) / k
        sha.update(np.ascontiguousarray(idx).tobytes() + np.ascontiguousarray(score).tobytes())
    out['keys_sha16'] = sha.hexdigest()[:16]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('libs', nargs='+')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--calls', type=int, default=2000)
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        child(a.libs[0], a.calls)
        return
    keys = None
    for rnd in range(a.rounds):
        for lib in a.libs:
            p = subprocess.run([sys.executable, __file__, lib, '--child', '--calls', str(a.calls)],
                               capture_output=True, text=True, timeout=300)
            if p.returncode != 0:   # a child that failed or faulted ends the A/B
                print(p.stderr[-2000:], file=sys.stderr)
                raise SystemExit(p.returncode)
            r = json.loads(p.stdout.strip().splitlines()[-1])
            r['round'] = rnd
            print(json.dumps(r), flush=True)
            keys = keys or r['keys_sha16']
            if r['keys_sha16'] != keys:
                print('vt_host_ab: INVALID A/B -- %s returns other keys' % lib, file=sys.stderr)
                raise SystemExit(1)


if __name__ == '__main__':
    main()
