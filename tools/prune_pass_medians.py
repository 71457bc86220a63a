#!/usr/bin/env python3
"""Per-pass median kernel times (us) of the pruned plane scan from a
``rocprofv3 --kernel-trace --output-format csv`` folder: the prefilter's dispatches, or
the fused front's (vt_front_kernel: prefilter, pick and verification in one launch), mark
the pruned calls; of the list-driven scan's two dispatches per call the first is pass B1
and the second pass B2 (dispatch order), behind vt_prune_first_kernel; a call without that
kernel is the four-kernel chain (qplane, front, the one list pass, export) and its scan `list`.  Only calls of the most common grid of that
first kernel (the headline shape in a plain bench) are counted; a pass that a build
does not launch is not reported.
usage: python tools/prune_pass_medians.py TRACE_DIR [TRACE_DIR ...]   (one JSON object)"""
import collections
import csv
import glob
import json
import os
import sys

NAMES = (('vt_qplane_kernel', 'qplane'), ('vt_prefilter_kernel', 'prefilter'), ('vt_front_kernel', 'front'), ('vt_prune_pick_kernel', 'pick'),
         ('vt_prune_verify_kernel', 'verify'), ('vt_prune_first_kernel', 'first'),
         ('vt_prune_rest_kernel', 'rest'), ('vt_prune_finish_kernel', 'finish'), ('vt_keys_export', 'export'),
         ('vt_scan_plane_kernel<64, false, true>', 'list_scan'))


def passes(d):
    f = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r['Start_Timestamp']))
    calls, cur, pend = [], None, 0.0
    for r in rows:
        tag = next((t for n, t in NAMES if n in r['Kernel_Name']), None)
        if tag is None:
            continue
        us = (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
        if tag == 'qplane':
            pend = us
            continue
        if tag in ('prefilter', 'front'):
            cur = {'grid': r.get('Grid_Size', r.get('Grid_Size_X', '')), 'qplane': pend, tag: us}
            calls.append(cur)
        elif cur is not None:
            if tag == 'list_scan':
                tag = ('B2' if 'B1' in cur else 'B1') if 'first' in cur else 'list'
            cur.setdefault(tag, us)
    grid = collections.Counter(c['grid'] for c in calls).most_common(1)[0][0]
    calls = [c for c in calls if c['grid'] == grid]
    out = {'calls': len(calls)}
    for k in ('qplane', 'prefilter', 'front', 'pick', 'verify', 'first', 'B1', 'rest', 'B2', 'list', 'finish', 'export'):
        v = sorted(c[k] for c in calls if k in c)
        if v:
            out[k] = round(v[len(v) // 2], 1)
    out['sum'] = round(sum(v for k, v in out.items() if k != 'calls'), 1)
    return out


if __name__ == '__main__':
    print(json.dumps({os.path.basename(os.path.normpath(d)): passes(d) for d in sys.argv[1:]}, indent=1))
