#!/usr/bin/env python3
"""Host-clock time of every headline step (rs_vt_match_stream over 10 HBM-resident batches of
1,024 queries against 1,000 templates) of one process: 0.3 s of warm-up as tools/stream_ab.py,
then 600 timed steps; the median, the means of the ten windows of 60 steps and the largest steps
(index, ms).  usage: python tools/step_times.py LIB.so"""
import os
import sys, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pyratslam_amd import _lib, synthetic
_lib.load(sys.argv[1])
from pyratslam_amd.view_templates import ViewTemplates
vts = ViewTemplates._from_shape((64, 32), 45000, device=0, capacity=1000)
lib = synthetic.library(1000, seed=1)
vts.add(lib)
qs = [synthetic.queries_fast(lib, 1024, seed=2 + 1000 * b)[0] for b in range(10)]
arg = (10, 1024, _lib.DeviceBuffer(10 * qs[0].nbytes, device=0).upload(np.stack(qs)))
t_end = time.perf_counter() + 0.3
n = 0
while time.perf_counter() < t_end:
    vts.match_stream(arg); n += 1
ts = []
for _ in range(600):
    t0 = time.perf_counter(); vts.match_stream(arg); ts.append(1e3 * (time.perf_counter() - t0))
a = np.array(ts)
w = a.reshape(10, 60).mean(axis=1)
big = np.argsort(a)[-8:][::-1]
print(json.dumps({'lib': sys.argv[1], 'warm_steps': n, 'median': round(float(np.median(a)), 4), 'mean60': [round(float(x), 4) for x in w],
                  'p90': round(float(np.percentile(a, 90)), 4), 'n_over_0.7': int((a > 0.7).sum()), 'n_over_2': int((a > 2).sum()),
                  'largest': [(int(i), round(float(a[i]), 3)) for i in big]}))
